// pass_launch.hpp -- which kernel one pass over the matrix runs, and its launch.  Part of emsar_hip.hip's translation unit, included after
// the context and its small helpers: it uses the context, HIPCHK, grid_for, fx_of and the kernels (kernels_tiled.hpp, kernels_csr.hpp).
//   choose_pass_kernel        which TILED kernel runs: a pure function of weighted, mode, tile count and the two knobs
//                             (emsar_hip_debug_pass_kernel shows it to the tests)
//   launch_tile / _multi / _unit / _left / _csr   one launcher per kernel family, the template arguments as tag values
//   set_tiled_lds_attributes  the dynamic LDS of every instantiation choose_pass_kernel can return, once per upload_structure
//   launch_pass               one pass of the chosen layout: the TILED kernel, the leftover rows, the folded rows' likelihood
//   emsar_hip_debug_tiled_stamps / _unit_stamps   the stamped diagnostic instances of the two kernels, one helper (stamped_launch)

namespace {

// ---- which TILED pass kernel runs: a pure function of the sample, the mode, the size and the two knobs ----
constexpr int64_t kPairMinTiles = 2048;   // 256 CUs x 4 resident workgroups x 2 tiles
enum PassFamily { FAMILY_TILE, FAMILY_MULTI, FAMILY_UNIT };      // k_pass_tiled, k_pass_tiled_multi, k_pass_tiled_unit
struct PassKernel { PassFamily family; bool weighted; int mode; int n_multi; /* tiles per workgroup, FAMILY_MULTI only */ };

PassKernel choose_pass_kernel(bool weighted, int mode, int64_t n_tiles, int tiled_multi, int weighted_unit) {
    if (mode == MODE_SCATTER) return {FAMILY_TILE, false, MODE_SCATTER, 0};
    const bool above = tiled_multi == 1 && n_tiles > kPairMinTiles;
    if (!weighted && (tiled_multi >= 2 || above)) {
        // more than one tile per workgroup.  Unweighted rows only: with the row weights in registers as well the body does not
        // fit 128 VGPRs (round 1, two tiles: 0.218 vs 0.179 ms; round 2, the unit kernel on merged rows, 72-92 B of scratch:
        // 0.124 vs 0.103 ms with one tile per workgroup; with the weights kept as integers its EM variant fits without
        // scratch and runs config 3's merged rows in 0.0959 ms against 0.0956 ms for one tile per workgroup: no gain,
        // and the likelihood variant -- twelve logs -- still spills).
        // Only when the tiles outnumber the chip's workgroup slots: below that a pass is one workgroup's latency, and
        // a pair takes twice as long as a tile (40 k reads: 47 -> 26 us per pass with one tile per workgroup)
        if (tiled_multi == 1 || tiled_multi == 5) return {FAMILY_UNIT, false, mode, 0};      // units: one dictionary for up to two tiles
        return {FAMILY_MULTI, false, mode, tiled_multi == 3 ? 3 : tiled_multi == 4 ? 4 : 2};
    }
    if (weighted && (weighted_unit == 2 || (weighted_unit == 1 && mode == MODE_EM)) && (tiled_multi == 5 || above)) {
        // weighted rows (segments with read counts, merged rows) on the unit kernel: the weights are loaded as integers after the
        // forward batch is consumed; both variants fit 128 VGPRs without scratch (round 3).  Measured on the collapsed form of
        // config 3 (14.0 M segments of the family law / 5.4 M of the window law): plain pass 0.1273 -> 0.1221 / 0.0964 -> 0.0962 ms;
        // the likelihood variant takes its twelve logs per lane in one rolled loop (tile_e_step) and is SLOWER than the one-tile
        // kernel's unrolled logs (solve 0.161 against 0.150 ms per pass), so by default (1) only the plain EM pass of a SQUAREM
        // cycle runs here and the two likelihood passes stay with k_pass_tiled; 2 = both, 0 = neither (EMSAR_HIP_WEIGHTED_UNIT)
        return {FAMILY_UNIT, true, mode, 0};
    }
    return {FAMILY_TILE, weighted, mode, 0};
}

// ---- launchers: one per kernel family, the template arguments as tag values ----
template <bool B> using BoolC = std::integral_constant<bool, B>;
template <int M> using ModeC = std::integral_constant<int, M>;
// f(mode tag) / f(weighted tag, mode tag) for a pass of the E- and M-step, with or without the likelihood
template <class F> void with_em_mode(int mode, const F &f) { if (mode == MODE_EM_LL) f(ModeC<MODE_EM_LL>()); else f(ModeC<MODE_EM>()); }
template <class F> void with_em_variant(bool weighted, int mode, const F &f) {
    if (weighted) with_em_mode(mode, [&](auto md) { f(BoolC<true>(), md); });
    else with_em_mode(mode, [&](auto md) { f(BoolC<false>(), md); });
}

constexpr size_t kTiledLds = (size_t)kTiledLdsDoubles * sizeof(double);
struct PassArgs { const double *theta; double *acc, *ll_out; Fx fx; };

template <bool WT, int MD> void launch_tile(BoolC<WT>, ModeC<MD>, emsar_hip_ctx *ctx, const PassArgs &a) {
    const LayoutDev &L = ctx->lay;
    hipLaunchKernelGGL((k_pass_tiled<WT, MD>), dim3((unsigned)L.n_tiles), dim3(kTiledThreads), kTiledLds, ctx->stream, L.d_tiles, L.d_fwd, L.d_bwd,
                       L.d_far, ctx->rw.d_wgt, L.d_rowval, a.theta, a.acc, a.ll_out, a.fx);
}
template <bool WT, int MD, int N> void launch_multi(BoolC<WT>, ModeC<MD>, std::integral_constant<int, N>, emsar_hip_ctx *ctx, const PassArgs &a) {
    const LayoutDev &L = ctx->lay;
    hipLaunchKernelGGL((k_pass_tiled_multi<WT, MD, N>), dim3((unsigned)((L.n_tiles + N - 1) / N)), dim3(kTiledThreads), kTiledLds, ctx->stream, L.d_tiles,
                       (int)L.n_tiles, L.d_fwd, L.d_bwd, L.d_far, ctx->rw.d_wgt, a.theta, a.acc, a.ll_out, a.fx);
}
template <bool WT, int MD> void launch_unit(BoolC<WT>, ModeC<MD>, emsar_hip_ctx *ctx, const PassArgs &a) {
    const LayoutDev &L = ctx->lay;
    hipLaunchKernelGGL((k_pass_tiled_unit<WT, MD>), dim3((unsigned)L.n_units), dim3(kTiledThreads), kTiledLds, ctx->stream, L.d_utiles, L.unit_stride,
                       L.d_far, L.d_fwd, L.d_bwd, ctx->rw.d_wgt, a.theta, a.acc, a.ll_out, a.fx);
}
// the CSR kernel: the caller's rows (32- or 64-bit row_ptr), or the leftover rows of TILED
template <class PT, bool WT, int MD>
void launch_csr_rows(emsar_hip_ctx *ctx, unsigned max_grid, int64_t n_rows, const PT *row_ptr, const int32_t *col, const int32_t *wgt, const double *val, const PassArgs &a) {
    hipLaunchKernelGGL((k_pass_csr<PT, WT, MD>), dim3((unsigned)std::min<int64_t>((n_rows + 255) / 256, max_grid)), dim3(256), 0, ctx->stream, n_rows, row_ptr,
                       col, wgt, val, a.theta, a.acc, a.ll_out, a.fx);
}
template <bool WT, int MD> void launch_left(BoolC<WT>, ModeC<MD>, emsar_hip_ctx *ctx, const PassArgs &a) {
    const LayoutDev &L = ctx->lay;
    launch_csr_rows<uint64_t, WT, MD>(ctx, 8192, L.n_left, L.d_left_ptr, L.d_left_col, ctx->rw.d_left_wgt, L.d_left_val, a);
}
template <bool WT, int MD> void launch_csr(BoolC<WT>, ModeC<MD>, emsar_hip_ctx *ctx, const PassArgs &a) {
    const LayoutDev &L = ctx->lay;
    if (ctx->ptr64) launch_csr_rows<uint64_t, WT, MD>(ctx, 256 * 32, ctx->n_rows, (const uint64_t *)L.d_row_ptr.get(), L.d_col, ctx->rw.d_wgt, L.d_rowval, a);
    else launch_csr_rows<uint32_t, WT, MD>(ctx, 256 * 32, ctx->n_rows, (const uint32_t *)L.d_row_ptr.get(), L.d_col, ctx->rw.d_wgt, L.d_rowval, a);
}

// the dynamic LDS of the TILED kernels, for every instantiation choose_pass_kernel can return (once per upload_structure)
hipError_t set_tiled_lds_attributes() {
    hipError_t e = hipSuccess;
    auto set = [&](auto *kernel) { if (e == hipSuccess) e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTiledLds); };
    set(k_pass_tiled<false, MODE_SCATTER>);
    for (const bool weighted : {false, true})
        for (const int mode : {MODE_EM, MODE_EM_LL})
            with_em_variant(weighted, mode, [&](auto wt, auto md) { set(k_pass_tiled<wt(), md()>); set(k_pass_tiled_unit<wt(), md()>); });
    for (const int mode : {MODE_EM, MODE_EM_LL})
        with_em_mode(mode, [&](auto md) { set(k_pass_tiled_multi<false, md(), 2>); set(k_pass_tiled_multi<false, md(), 3>); set(k_pass_tiled_multi<false, md(), 4>); });
    return e;
}

// one pass of the chosen layout.  mode: MODE_EM / MODE_EM_LL / MODE_SCATTER
int launch_pass(emsar_hip_ctx *ctx, int mode, const double *theta, double *acc, double *ll_out, bool rows_only = false /* the folded rows' likelihood terms are added by the caller */) {
    const PassArgs a{theta, acc, ll_out, fx_of(ctx, mode)};
    const bool scatter = mode == MODE_SCATTER;
    if (ctx->layout == EMSAR_LAYOUT_TILED) {
        if (ctx->lay.n_tiles > 0) {
            const PassKernel k = choose_pass_kernel(ctx->weighted, mode, ctx->lay.n_tiles, ctx->tiled_multi, ctx->weighted_unit);
            if (scatter) launch_tile(BoolC<false>(), ModeC<MODE_SCATTER>(), ctx, a);
            else if (k.family == FAMILY_TILE) with_em_variant(k.weighted, k.mode, [&](auto wt, auto md) { launch_tile(wt, md, ctx, a); });
            else if (k.family == FAMILY_UNIT) with_em_variant(k.weighted, k.mode, [&](auto wt, auto md) { launch_unit(wt, md, ctx, a); });
            else with_em_mode(k.mode, [&](auto md) {
                using std::integral_constant;
                if (k.n_multi == 3) launch_multi(BoolC<false>(), md, integral_constant<int, 3>(), ctx, a);
                else if (k.n_multi == 4) launch_multi(BoolC<false>(), md, integral_constant<int, 4>(), ctx, a);
                else launch_multi(BoolC<false>(), md, integral_constant<int, 2>(), ctx, a);
            });
        }
        if (ctx->lay.n_left > 0) {   // rows too long for a tile: generic CSR kernel on the leftover
            if (scatter) launch_left(BoolC<false>(), ModeC<MODE_SCATTER>(), ctx, a);
            else with_em_variant(ctx->weighted, mode, [&](auto wt, auto md) { launch_left(wt, md, ctx, a); });
        }
        if (mode == MODE_EM_LL && !rows_only)
            hipLaunchKernelGGL(k_single_ll, dim3(std::min(grid_for(ctx->n_tx, 256), 256)), dim3(256), 0, ctx->stream, ctx->n_tx,
                               ctx->lay.d_u, theta, ll_out, fx_of(ctx).ll);
        HIPCHK(hipGetLastError());
        return EMSAR_HIP_OK;
    }
    if (ctx->n_rows == 0) return EMSAR_HIP_OK;
    if (scatter) launch_csr(BoolC<false>(), ModeC<MODE_SCATTER>(), ctx, a);
    else with_em_variant(ctx->weighted, mode, [&](auto wt, auto md) { launch_csr(wt, md, ctx, a); });
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// One stamped diagnostic launch on the current theta: `words` zeroed 64-bit words on the device, launch(words) on the context's stream,
// acc cleared again (theta is left untouched), the words fetched into h.  The first 8 nw of them are nw per-wave records of 8:
// out[0..6] = their means in cycles per wave.
template <class Launch>
int stamped_launch(emsar_hip_ctx *ctx, const void *kernel, size_t nw, size_t words, const Launch &launch, std::vector<unsigned long long> &h, double *out) {
    const size_t bytes = words * sizeof(unsigned long long);
    DevBuf<unsigned long long> d;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(d.alloc(words));
    HIPCHK(hipMemsetAsync(d, 0, bytes, ctx->stream));
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTiledLds));
    launch(d.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(ctx->vec.d_acc, 0, (size_t)ctx->n_tx * 8, ctx->stream));
    h.resize(words);
    HIPCHK(hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 7; i++) {
        double sum = 0;
        for (size_t w = 0; w < nw; w++) sum += (double)h[w * 8 + (size_t)i];
        out[i] = sum / (double)nw;
    }
    return EMSAR_HIP_OK;
}

}  // namespace

extern "C" {

// Diagnostic only (not declared in the public header): one stamped pass of the TILED kernel on the current theta.
// out[0..6] = mean cycles per wave spent in: loads issued + dictionary, barrier, E-step, barrier, M-step, barrier, flush;
// out[7] = tiles.  The result vector theta is left untouched (acc is cleared again).
int emsar_hip_debug_tiled_stamps(emsar_hip_ctx *ctx, double *out) {
    if (!ctx || !out || ctx->layout != EMSAR_LAYOUT_TILED || !ctx->have_sample || ctx->weighted || ctx->lay.n_tiles == 0) return EMSAR_HIP_ERR_STATE;
    const LayoutDev &L = ctx->lay;
    const size_t nw = (size_t)L.n_tiles * (kTiledThreads / 64);
    std::vector<unsigned long long> h;
    const int rc = stamped_launch(ctx, (const void *)k_pass_tiled<false, MODE_EM, true>, nw, nw * 8, [&](unsigned long long *d) {
        hipLaunchKernelGGL((k_pass_tiled<false, MODE_EM, true>), dim3((unsigned)L.n_tiles), dim3(kTiledThreads), kTiledLds, ctx->stream, L.d_tiles, L.d_fwd, L.d_bwd,
                           L.d_far, ctx->rw.d_wgt, L.d_rowval, ctx->vec.d_th[0], ctx->vec.d_acc, &ctx->d_scal->ll[3].s[0].v, Fx{0.0, 0.0}, d);
    }, h, out);
    if (rc == EMSAR_HIP_OK) out[7] = (double)L.n_tiles;
    return rc;
}

// The same for the unit kernel (the one config 3 runs): out[0..5] = mean cycles per wave in: descriptor + dictionary + first loads,
// barrier, E-steps, M-steps, barrier, flush; out[6] = tiles per unit; out[7] = units.
int emsar_hip_debug_unit_stamps(emsar_hip_ctx *ctx, double *out, unsigned long long *timeline /* NULL or 4 words per unit: start, end (100 MHz ticks), place, tiles */) {
    if (!ctx || !out || ctx->layout != EMSAR_LAYOUT_TILED || !ctx->have_sample || ctx->weighted || ctx->lay.n_units == 0) return EMSAR_HIP_ERR_STATE;
    const LayoutDev &L = ctx->lay;
    const size_t nw = (size_t)L.n_units * (kTiledThreads / 64);
    std::vector<unsigned long long> h;
    const int rc = stamped_launch(ctx, (const void *)k_pass_tiled_unit<false, MODE_EM, true>, nw, nw * 8 + (size_t)L.n_units * 4, [&](unsigned long long *d) {
        hipLaunchKernelGGL((k_pass_tiled_unit<false, MODE_EM, true>), dim3((unsigned)L.n_units), dim3(kTiledThreads), kTiledLds, ctx->stream, L.d_utiles, L.unit_stride,
                           L.d_far, L.d_fwd, L.d_bwd, ctx->rw.d_wgt, ctx->vec.d_th[0], ctx->vec.d_acc, &ctx->d_scal->ll[3].s[0].v, Fx{0.0, 0.0}, d);
    }, h, out);
    if (rc != EMSAR_HIP_OK) return rc;
    if (timeline) std::copy(h.begin() + (std::ptrdiff_t)(nw * 8), h.end(), timeline);
    out[7] = (double)L.n_units;
    return EMSAR_HIP_OK;
}

// Diagnostic only (not declared in the public header; needs no device): the name of the TILED pass kernel launch_pass picks for a sample
// (weighted or not), a mode (0: EM, 1: EM with the likelihood, 2: scatter), a tile count and the two knobs' values.
int emsar_hip_debug_pass_kernel(int weighted, int mode, int64_t n_tiles, int tiled_multi, int weighted_unit, char *out, size_t cap) {
    if (!out || mode < MODE_EM || mode > MODE_SCATTER) return EMSAR_HIP_ERR_ARG;
    const PassKernel k = choose_pass_kernel(weighted != 0, mode, n_tiles, tiled_multi, weighted_unit);
    const char *const wt = k.weighted ? "true" : "false";
    const int len = k.family == FAMILY_MULTI  ? snprintf(out, cap, "k_pass_tiled_multi<%s, %d, %d>", wt, k.mode, k.n_multi)
                    : k.family == FAMILY_UNIT ? snprintf(out, cap, "k_pass_tiled_unit<%s, %d>", wt, k.mode)
                                              : snprintf(out, cap, "k_pass_tiled<%s, %d>", wt, k.mode);
    return len >= 0 && (size_t)len < cap ? EMSAR_HIP_OK : EMSAR_HIP_ERR_ARG;
}

}  // extern "C"
