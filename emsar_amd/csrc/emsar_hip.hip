// emsar_hip.hip -- MI355X (gfx950 / CDNA4) abundance-estimation core behind include/emsar_hip.h.
//
// Replaces run_MLE_threads() (/root/reference/src/emsar_main.c:446; MLE/Fp/lambdap,
// emsar_functions.c:2946-3126) by an EM on the same segment Poisson likelihood:
//     E-step  w_c = R_c / S_c ,  S_c = sum_t m_ct theta_t        (rows with E_c == 0 are outside F)
//     M-step  theta_t <- theta_t * (sum_c m_ct w_c) / den_t ,    den_t = sum_c m_ct E_c
// and compute_iEUMA / the TPM + iReadcount arithmetic of print_FPKMfinal (emsar_functions.c:3176-3232).
//
// One pass is HBM-bound integer streaming plus FP64 adds: ~2 flop per nonzero -- no MFMA.
// This file: the context, the launch logic (launch_pass, enqueue_cycles, the set solver's driver) and the C ABI of uploads and solves.
//   context      its device and pinned memory lives in DevBuf / PinBuf owners (devmem.hpp), grouped by lifetime: LayoutDev, TxVectors, GeneMap
//                and AdjEuma go with the structure, RowWeights and SetsDev with the sample; a group is dropped by assigning an empty one
//   launch_pass  choose_pass_kernel says which TILED kernel runs (a pure function of weighted, mode, tile count and the two knobs;
//                emsar_hip_debug_pass_kernel shows it to the tests), one launcher per kernel family launches it
// resample.hpp (same translation unit, included at the end): the resampling driver and its C ABI -- bootstrap, quantiles, subsampling, genes.
// Kernels (one translation unit, included below):
//   kernels_tiled.hpp     k_pass_tiled / k_pass_tiled_multi<2>   the hot ones: one workgroup per tile (or pair of tiles) of the
//                         TILED layout, dictionary of theta/acc in LDS, 10-bit ids, per-slice transposed index
//   kernels_csr.hpp       k_pass_csr                             the caller's CSR as it is (layout 1), leftover rows of TILED
//   kernels_vector.hpp    k_update, k_update_p2/p3, k_sq_extrap_ll (SQUAREM extrapolation / acceptance on the device),
//                         k_normalise, k_adj_euma, small reductions
//   kernels_sets.hpp      k_solve_sets                           one workgroup solves one connected set out of LDS
//   kernels_boot.hpp      k_boot_draw, k_boot_accum, ...         the Poisson bootstrap (draws: boot_rng.hpp; sets: k_solve_sets_boot)
//                         k_sub_draw, k_sub_scale                the depth subsampling: binomial draws, every replicate to its own depth
//   kernels_genes.hpp     k_gene_sums, k_gene_finish             per-gene sums in a fixed order (gene_sums, the bootstrap's gene sd)
//   kernels_quant.hpp     k_boot_quantiles                       quantiles over the held replicates (bootstrap_quantiles)
//   kernels_isoforms.hpp  k_iso_usage, k_iso_dominant, k_iso_accum, k_iso_quantiles   each transcript's share of its gene, the dominant
//                         isoform, and their statistics over the replicates (isoform_usage, bootstrap_isoforms)
//   kernels_fit.hpp       k_fit_rows, k_fit_tx, k_fit_tx_finish, k_fit_totals   per-row residuals of a theta and their attribution to
//                         the transcripts over a transposed index (model_fit; driver: fit.hpp, shared arithmetic: fit_index.hpp)
//   collapse.hip          read-level rows -> weighted segments (own translation unit)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/emsar_hip.h"
#include "layout.hpp"
#include "layout_tiled.hpp"
#include "sets.hpp"
#include "boot_rng.hpp"
#include "internal.hpp"
#include "devmem.hpp"
#include "fit_index.hpp"

#include "kernels_common.hpp"
#include "kernels_csr.hpp"
#include "kernels_tiled.hpp"
#include "kernels_vector.hpp"
#include "kernels_sets.hpp"
#include "kernels_cluster.hpp"
#include "kernels_boot.hpp"
#include "kernels_genes.hpp"
#include "kernels_quant.hpp"
#include "kernels_isoforms.hpp"
#include "kernels_fit.hpp"

// ==================================================================================================
// context
// ==================================================================================================
using emsar::DevBuf;
using emsar::PinBuf;

// The device memory of the context, grouped by lifetime: each group is dropped by assigning a default-constructed one (devmem.hpp).

// What a sample's connected sets put on the device (ensure_sets), dropped by upload_sample
struct SetsDev {
    bool sets_ready = false;
    emsar::ResidentSets RS;      // index vectors are freed after the upload, counters stay
    DevBuf<emsar::SetDesc> d_sdesc[emsar::kSetClasses];
    DevBuf<SetStat> d_sstat; PinBuf<SetStat> h_sstat; int64_t n_sstat = 0;
    DevBuf<int32_t> d_g_tid; DevBuf<double> d_g_u, d_row_w, d_usum;
    DevBuf<uint16_t> d_srp, d_sent, d_scp, d_scrow;
    DevBuf<uint8_t> d_kind;
    // workgroup-cluster sets (kernels_cluster.hpp)
    DevBuf<emsar::ClusterDesc> d_cdesc; DevBuf<uint32_t> d_cblk, d_crp, d_ccp, d_cpart;
    DevBuf<uint16_t> d_cent, d_ccrow; DevBuf<int32_t> d_cg_tid; DevBuf<double> d_cg_u, d_crow_w, d_cscratch;
    DevBuf<unsigned> d_cbar;             // [2 n]: barrier words, then abort words
    DevBuf<ClusterStat> d_cstat; PinBuf<ClusterStat> h_cstat;
    int64_t n_cstat = 0;
    // bootstrap (emsar_hip_bootstrap): the sample's row weights in caller order and the draw map of the set solver, built on first use
    DevBuf<int32_t> d_boot_R;
    DevBuf<int64_t> d_boot_slot;      // caller row -> index into one replicate's [row_w | usum] block, -1 = none
    int64_t boot_n_rw = 0;            // row_w entries of the resident sets (usum follows them)
    bool boot_slot_ready = false;
};

// gene map (emsar_hip_set_gene_map), dropped by upload_structure.  One int32 block: per gene in gene order its transcripts' library
// indices by ascending caller tid (gene_tx), the chunks' begin offsets into gene_tx (chunk_beg, n_gene_chunks + 1), each chunk's
// gene when that gene has one chunk, else -1 (chunk_out), the genes of more than one chunk (gene_multi: gene, first chunk, end), and
// the gene of every library index, -1 = none (gene_of_lib, n_tx)
struct GeneMap {
    bool have_genes = false;
    int32_t n_genes = 0;
    int64_t n_gene_chunks = 0, n_gene_multi = 0;
    DevBuf<int32_t> d_gene_blk;
    int32_t *d_gene_tx = nullptr, *d_chunk_beg = nullptr, *d_chunk_out = nullptr, *d_gene_multi = nullptr, *d_gene_of_lib = nullptr;   // views into d_gene_blk
};

// compute_adjEUMA on the device (emsar_hip_upload_euma), dropped by upload_structure
struct AdjEuma {
    DevBuf<int32_t> d_euma_t; int32_t nfl = 0; DevBuf<double> d_wf, d_adj;
};

// row weights in layout order (0 = row outside F), dropped by upload_sample; an unweighted sample has none
struct RowWeights { DevBuf<int32_t> d_wgt, d_left_wgt; };

// the matrix in the chosen layout, dropped by upload_structure
struct LayoutDev {
    // CSR layout
    DevBuf<void> d_row_ptr;      // uint32 or uint64
    DevBuf<int32_t> d_col;
    // TILED layout
    emsar::TiledLayout TL;       // host copy keeps slot_row / single_* / left_row (index arrays freed after upload)
    DevBuf<Tile> d_tiles;
    DevBuf<Tile> d_utiles; int unit_stride = 1;   // emsar::UnitTables
    DevBuf<uint32_t> d_units; int64_t n_units = 0;     // units of one or two tiles that share a dictionary (k_pass_tiled_unit)
    DevBuf<uint32_t> d_fwd, d_bwd;
    DevBuf<int32_t> d_far;
    DevBuf<uint64_t> d_left_ptr; DevBuf<int32_t> d_left_col; DevBuf<double> d_left_val;
    int64_t n_left = 0, n_tiles = 0, n_slots = 0;
    DevBuf<double> d_u;          // folded single-tid rows: per-transcript weight sum
    DevBuf<double> d_rowval;     // scratch for scatter passes (den, iEUMA)
};

// vectors [n_tx], dropped by upload_structure
struct TxVectors {
    DevBuf<double> d_den, d_acc;
    DevBuf<double> d_th[5];      // th0 th1 th2 thx thn
    DevBuf<double> d_tmp[3];
    DevBuf<int32_t> d_itmp;
};

struct emsar_hip_ctx {
    int device = 0;
    int n_cu = 64;               // compute units of the device (cluster launches: one workgroup per CU at most)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    hipStream_t side[3] = {nullptr, nullptr, nullptr};     // the 256- and 512-thread classes of the set solver and the clusters run next to the 64-thread class
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;   // around the cluster launches (stats)
    std::string err;
    // structure
    bool have_structure = false, have_sample = false;
    int layout = EMSAR_LAYOUT_CSR;
    int64_t n_rows = 0, nnz = 0;
    int32_t n_tx = 0;
    bool ptr64 = false;
    LayoutDev lay;
    TxVectors vec;
    GeneMap genes;
    AdjEuma euma;
    FitDev fit;                  // model fit (fit.hpp): caller-order CSR and transposed index, built on first use, dropped by upload_structure
    // sample
    bool weighted = false;
    RowWeights rw;
    SetsDev sets;
    double loglik_const = 0.0;   // sum_c R_c log E_c over rows inside F
    DevBuf<Scal> d_scal;
    PinBuf<Scal> h_scal;
    int64_t bytes_formula = 0, bytes_stored = 0;
    int64_t tl_fwd_slots = 0, tl_n_fslices = 0;
    double count_floor = 0.0;    // stopping-rule floor in reads for the current solve (emsar_em_params.count_floor)
    double zero_cut = 0.0;       // emsar_em_params.zero_cut of the current solve
    bool use_graph = true;       // replay check_every cycles of the streaming solve from one hipGraph (EMSAR_HIP_GRAPH=0: launch each kernel)
    int64_t graph_launches = 0;  // of the last solve (debug: EMSAR_HIP_DEBUG)
    bool det = false;            // deterministic mode (emsar_hip_set_deterministic / EMSAR_HIP_DETERMINISTIC): fixed-point sums, kernels_common.hpp
    double fx_mass = 0.0, fx_ll = 0.0;   // its scales for the current sample (upload_sample)
    DevBuf<double> d_sqpart;     // per-workgroup partial sums of the SQUAREM vector kernels [4][kSqPart]
    int update_grid = 1024;       // workgroups of k_update (EMSAR_HIP_UPDATE_GRID)
    int sq_grid = 256;           // workgroups of the SQUAREM vector kernels (EMSAR_HIP_SQ_GRID)
    int weighted_unit = 1;       // EMSAR_HIP_WEIGHTED_UNIT: weighted rows on k_pass_tiled_unit -- 1: the plain EM pass, 2: the likelihood passes too, 0: never
    int tiled_multi = 1;         // EMSAR_HIP_TILED_MULTI 1: two tiles per workgroup (k_pass_tiled_multi) above kPairMinTiles tiles, else one
                                 // (k_pass_tiled); 2: always two; 0: always one
    const uint8_t *delta_mask = nullptr;   // sets.d_kind while the streaming solve runs next to resident sets
    // set-resident solver (sets.hpp): host copy of the CSR and of the sample's row weights, built lazily by solve
    std::vector<uint64_t> h_row_ptr;
    std::vector<int32_t> h_col, h_wgt;
    double sets_build_ms = 0.0;
};

namespace {

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
            return e_ == hipErrorOutOfMemory ? EMSAR_HIP_ERR_OOM : EMSAR_HIP_ERR_HIP;                   \
        }                                                                                              \
    } while (0)

inline int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }

// per-solve state, cleared whatever the exit of a solve
inline void clear_solve_state(emsar_hip_ctx *ctx) { ctx->count_floor = 0.0; ctx->zero_cut = 0.0; ctx->delta_mask = nullptr; }
// deterministic mode's scales for a sample of `total` reads: no transcript is assigned more reads than the sample holds, |sum R log S| <= N * 745
inline void set_fx_scales(emsar_hip_ctx *ctx, int64_t total) {
    int e_mass = 0, e_ll = 0;
    (void)std::frexp((double)total + 1.0, &e_mass);
    (void)std::frexp(((double)total + 1.0) * 1024.0, &e_ll);
    ctx->fx_mass = std::ldexp(1.0, 61 - e_mass);
    ctx->fx_ll = std::ldexp(1.0, 61 - e_ll);
}

// The TILED layout may number the transcripts itself (renumber.hpp); every T-sized device vector is then in the LIBRARY's numbering and
// the ABI maps: lib[new_of_old[t]] = caller[t].  Empty map = the caller's numbering.
inline const std::vector<int32_t> &tid_map(const emsar_hip_ctx *ctx) { return ctx->lay.TL.new_of_old; }
inline const double *to_lib(const emsar_hip_ctx *ctx, const double *caller, std::vector<double> &tmp) {
    const auto &m = tid_map(ctx);
    if (m.empty() || ctx->layout != EMSAR_LAYOUT_TILED) return caller;
    tmp.resize(m.size());
    for (size_t t = 0; t < m.size(); t++) tmp[(size_t)m[t]] = caller[t];
    return tmp.data();
}
template <class V> inline void from_lib(const emsar_hip_ctx *ctx, V *v /* in place: library order -> caller order */) {
    const auto &m = tid_map(ctx);
    if (m.empty() || ctx->layout != EMSAR_LAYOUT_TILED) return;
    std::vector<V> tmp(v, v + m.size());
    for (size_t t = 0; t < m.size(); t++) v[t] = tmp[(size_t)m[t]];
}

// bytes one pass actually streams in the chosen layout: index arrays + row weights + the T-sized vectors
inline int64_t stored_bytes(const emsar_hip_ctx *ctx) {
    int64_t rows = ctx->layout == EMSAR_LAYOUT_TILED ? ctx->lay.n_slots + ctx->lay.n_left : ctx->n_rows;
    return ctx->bytes_stored + (ctx->weighted ? 4 * rows : 0) + (ctx->layout == EMSAR_LAYOUT_TILED ? 40 : 32) * (int64_t)ctx->n_tx;
}

// the structure and all that hangs on it: the sample, its sets, the gene map, the adjEUMA arrays
void free_structure(emsar_hip_ctx *ctx) {
    ctx->sets = SetsDev(); ctx->rw = RowWeights();
    ctx->genes = GeneMap(); ctx->euma = AdjEuma(); ctx->fit = FitDev();
    ctx->lay = LayoutDev(); ctx->vec = TxVectors();
    std::vector<uint64_t>().swap(ctx->h_row_ptr); std::vector<int32_t>().swap(ctx->h_col); std::vector<int32_t>().swap(ctx->h_wgt);
    ctx->have_structure = ctx->have_sample = false;
}

// the fixed-point scales the EM kernels get (zeros = plain FP64 atomics; scatter passes always)
inline Fx fx_of(const emsar_hip_ctx *ctx, int mode = MODE_EM) { return (ctx->det && mode != MODE_SCATTER) ? Fx{ctx->fx_mass, ctx->fx_ll} : Fx{0.0, 0.0}; }

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

// a likelihood word of the host copy of the scalars (fixed point in deterministic mode)
inline double host_ll(const emsar_hip_ctx *ctx, int i) {
    const LlSum &L = ctx->h_scal->ll[i];             // the words of the sum, added in a fixed order (kernels_common.hpp)
    if (!ctx->det || ctx->fx_ll == 0.0) { double v = 0.0; for (int j = 0; j < kLlSlots; j++) v += L.s[j].v; return v; }
    long long b = 0;
    for (int j = 0; j < kLlSlots; j++) { long long x; memcpy(&x, &L.s[j].v, 8); b += x; }
    return (double)b / ctx->fx_ll;
}

// th_out = EM(th_in); ll slot receives sum R log S at th_in when want_ll
int em_pass(emsar_hip_ctx *ctx, const double *th_in, double *th_out, bool want_ll, int ll_slot, double abs_floor, int to_delta1 = 0) {
    int rc = launch_pass(ctx, want_ll ? MODE_EM_LL : MODE_EM, th_in, ctx->vec.d_acc, &ctx->d_scal->ll[ll_slot].s[0].v);
    if (rc) return rc;
    hipLaunchKernelGGL(k_update, dim3(std::min(grid_for(ctx->n_tx, 256), ctx->update_grid)), dim3(256), 0, ctx->stream, ctx->n_tx, th_in, ctx->vec.d_acc,
                       ctx->vec.d_den, ctx->layout == EMSAR_LAYOUT_TILED ? ctx->lay.d_u.get() : nullptr, th_out, abs_floor, ctx->count_floor, ctx->zero_cut, ctx->d_scal,
                       ctx->delta_mask, to_delta1, fx_of(ctx).mass);
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// `cycles` cycles of the streaming solve on ctx->stream -- launched, or recorded when the stream is capturing.
// One cycle = one plain EM pass, or one SQUAREM cycle of three passes (8 launches, see k_update_p2).  The current point is
// ctx->vec.d_th[0] before and after (plain EM swaps d_th[0]/d_th[1] on the host: record an even count).
int enqueue_cycles(emsar_hip_ctx *ctx, const emsar_em_params &p, double abs_step_base, int cycles) {
    const int n = ctx->n_tx, g = grid_for(n, 256);
    DevBuf<double> *th = ctx->vec.d_th;     // handles: plain EM swaps two of them
    int rc;
    for (int c = 0; c < cycles; c++) {
        hipLaunchKernelGGL(k_cycle_begin, dim3(1), dim3(kLlSlots), 0, ctx->stream, ctx->d_scal, abs_step_base, p.accel ? 3 : 1);
        if (!p.accel) {
            if ((rc = em_pass(ctx, th[0], th[1], false, 0, p.abs_floor))) return rc;
            std::swap(th[0], th[1]);
            continue;
        }
        // the stopping rule is measured on the first (plain) step of the cycle only (delta1_bits)
        const double *u = ctx->layout == EMSAR_LAYOUT_TILED ? ctx->lay.d_u.get() : nullptr;
        const dim3 gv((unsigned)std::min(std::min(g, ctx->sq_grid), kSqPart)), bv(256);
        if ((rc = em_pass(ctx, th[0], th[1], false, 0, p.abs_floor, 1))) return rc;
        if ((rc = launch_pass(ctx, MODE_EM_LL, th[1], ctx->vec.d_acc, &ctx->d_scal->ll[1].s[0].v, true))) return rc;
        hipLaunchKernelGGL(k_update_p2, gv, bv, 0, ctx->stream, n, th[0], th[1], ctx->vec.d_acc, ctx->vec.d_den, u, th[2], ctx->d_scal, ctx->d_sqpart, fx_of(ctx));
        hipLaunchKernelGGL(k_sq_extrap_ll, gv, bv, 0, ctx->stream, n, th[0], th[1], th[2], ctx->vec.d_den, u, th[3], ctx->d_scal, ctx->d_sqpart, (int)gv.x, fx_of(ctx));
        if ((rc = launch_pass(ctx, MODE_EM_LL, th[3], ctx->vec.d_acc, &ctx->d_scal->ll[2].s[0].v, true))) return rc;
        hipLaunchKernelGGL(k_update_p3, gv, bv, 0, ctx->stream, n, th[3], th[2], ctx->vec.d_acc, ctx->vec.d_den, u, th[0], ctx->d_scal, ctx->d_sqpart, (int)gv.x, fx_of(ctx));
        HIPCHK(hipGetLastError());
    }
    return EMSAR_HIP_OK;
}

struct CycleGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~CycleGraph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// The streaming layout's row weights from per-row weights x(r) (caller order, 0 = outside the likelihood): TILED -- the slots (a merged
// slot sums its member rows), the leftover rows and the per-transcript count of the folded single-transcript rows; CSR -- the rows as
// they are.  w / wl are filled only when `weighted`.  With row_E, llc += sum x log E over the rows with x > 0.  Used by upload_sample
// and by the bootstrap, which swaps a replicate's weights in.  ERR_ARG if a merged slot's sum exceeds INT32_MAX.
struct LayoutWeights { std::vector<int32_t> w, wl; std::vector<double> u; };
template <class WeightOf>
int layout_weights(const emsar_hip_ctx *ctx, const WeightOf &weight_of, const double *row_E, bool weighted, LayoutWeights &out, double &llc) {
    if (ctx->layout != EMSAR_LAYOUT_TILED) {
        if (!weighted) return EMSAR_HIP_OK;
        out.w.assign(std::max<size_t>((size_t)ctx->n_rows, 1), 0);
        for (int64_t r = 0; r < ctx->n_rows; r++) {
            const int32_t x = weight_of(r);
            out.w[(size_t)r] = x;
            if (x > 0 && row_E) llc += (double)x * std::log(row_E[r]);
        }
        return EMSAR_HIP_OK;
    }
    const auto &L = ctx->lay.TL;
    out.u.assign((size_t)ctx->n_tx, 0.0);
    for (size_t i = 0; i < L.single_row.size(); i++) {
        int32_t x = weight_of(L.single_row[i]);
        out.u[(size_t)L.single_tid[i]] += (double)x;
        if (x > 0 && row_E) llc += (double)x * std::log(row_E[L.single_row[i]]);
    }
    if (!weighted) return EMSAR_HIP_OK;
    out.w.assign((size_t)std::max<int64_t>(ctx->lay.n_slots, 1), 0);
    out.wl.assign((size_t)std::max<int64_t>(ctx->lay.n_left, 1), 0);
    for (int64_t i = 0; i < ctx->lay.n_slots; i++) {
        int64_t r = L.slot_row[(size_t)i];
        if (r < 0) continue;
        if (L.merged) {                                   // a slot stands for all rows with this tid multiset
            int64_t sum = 0;
            for (uint64_t q = L.mem_ptr[(size_t)r]; q < L.mem_ptr[(size_t)r + 1]; q++) {
                int64_t o = L.mem_row[(size_t)q];
                int32_t x = weight_of(o);
                sum += x;
                if (x > 0 && row_E) llc += (double)x * std::log(row_E[o]);
            }
            if (sum > INT32_MAX) return EMSAR_HIP_ERR_ARG;
            out.w[(size_t)i] = (int32_t)sum;
            continue;
        }
        int32_t x = weight_of(r);
        out.w[(size_t)i] = x;
        if (x > 0 && row_E) llc += (double)x * std::log(row_E[r]);
    }
    for (int64_t i = 0; i < ctx->lay.n_left; i++) {
        int64_t r = L.left_row[(size_t)i];
        int32_t x = weight_of(r);
        out.wl[(size_t)i] = x;
        if (x > 0 && row_E) llc += (double)x * std::log(row_E[r]);
    }
    return EMSAR_HIP_OK;
}

// a LayoutWeights on the device: d_u of TILED, and for weighted rows d_wgt / d_left_wgt, allocated when absent
int upload_layout_weights(emsar_hip_ctx *ctx, const LayoutWeights &LW, bool weighted) {
    const bool tiled = ctx->layout == EMSAR_LAYOUT_TILED;
    if (weighted) {
        if (!ctx->rw.d_wgt) HIPCHK(ctx->rw.d_wgt.alloc(LW.w.size()));
        HIPCHK(hipMemcpy(ctx->rw.d_wgt, LW.w.data(), LW.w.size() * 4, hipMemcpyHostToDevice));
        if (tiled && !ctx->rw.d_left_wgt) HIPCHK(ctx->rw.d_left_wgt.alloc(LW.wl.size()));
        if (tiled) HIPCHK(hipMemcpy(ctx->rw.d_left_wgt, LW.wl.data(), LW.wl.size() * 4, hipMemcpyHostToDevice));
    }
    if (tiled) HIPCHK(hipMemcpy(ctx->lay.d_u, LW.u.data(), LW.u.size() * 8, hipMemcpyHostToDevice));
    return EMSAR_HIP_OK;
}

// scatter a per-row value (original row order, host) to its columns: out[t] = sum_c m_ct val[c]
int scatter_rows(emsar_hip_ctx *ctx, const double *val_host, double *d_out) {
    try {
        if (ctx->layout == EMSAR_LAYOUT_TILED) {
            const auto &L = ctx->lay.TL;
            std::vector<double> slot((size_t)std::max<int64_t>(ctx->lay.n_slots, 1), 0.0), left((size_t)std::max<int64_t>(ctx->lay.n_left, 1), 0.0);
            std::vector<double> base((size_t)ctx->n_tx, 0.0);
            for (int64_t i = 0; i < ctx->lay.n_slots; i++) {
                int64_t r = L.slot_row[(size_t)i];
                if (r < 0) continue;
                if (L.merged) { double v = 0; for (uint64_t q = L.mem_ptr[(size_t)r]; q < L.mem_ptr[(size_t)r + 1]; q++) v += val_host[L.mem_row[(size_t)q]]; slot[(size_t)i] = v; }
                else slot[(size_t)i] = val_host[r];
            }
            for (int64_t i = 0; i < ctx->lay.n_left; i++) left[(size_t)i] = val_host[L.left_row[(size_t)i]];
            for (size_t i = 0; i < L.single_row.size(); i++) base[(size_t)L.single_tid[i]] += val_host[L.single_row[i]];
            if (!ctx->lay.d_rowval) HIPCHK(ctx->lay.d_rowval.alloc(slot.size()));
            if (!ctx->lay.d_left_val) HIPCHK(ctx->lay.d_left_val.alloc(left.size()));
            HIPCHK(hipMemcpyAsync(ctx->lay.d_rowval, slot.data(), slot.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(ctx->lay.d_left_val, left.data(), left.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(d_out, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            int rc = launch_pass(ctx, MODE_SCATTER, nullptr, d_out, nullptr);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(ctx->stream));
            return EMSAR_HIP_OK;
        }
        const double *src = val_host;
        size_t n = (size_t)ctx->n_rows;
        if (n == 0) return EMSAR_HIP_OK;
        if (!ctx->lay.d_rowval) HIPCHK(ctx->lay.d_rowval.alloc(n));
        HIPCHK(hipMemcpyAsync(ctx->lay.d_rowval, src, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(d_out, 0, (size_t)ctx->n_tx * sizeof(double), ctx->stream));
        int rc = launch_pass(ctx, MODE_SCATTER, nullptr, d_out, nullptr);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return EMSAR_HIP_OK;
    } catch (const std::bad_alloc &) { ctx->err = "out of host memory"; return EMSAR_HIP_ERR_OOM; }
}

// find and pack the connected sets of the current sample (sets.hpp) and move the records to the device
int ensure_sets_impl(emsar_hip_ctx *ctx);
int ensure_sets(emsar_hip_ctx *ctx) {
    if (ctx->sets.sets_ready) return EMSAR_HIP_OK;
    const int rc = ensure_sets_impl(ctx);
    if (rc != EMSAR_HIP_OK) ctx->sets = SetsDev();       // a half-uploaded record set is freed, the next solve starts over
    return rc;
}
int ensure_sets_impl(emsar_hip_ctx *ctx) {
    auto t0 = std::chrono::steady_clock::now();
    auto &S = ctx->sets.RS;
    try {
        emsar::build_sets(ctx->n_rows, ctx->n_tx, ctx->h_row_ptr.data(), ctx->h_col.data(), ctx->h_wgt.data(), S);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    if (ctx->layout == EMSAR_LAYOUT_TILED && !tid_map(ctx).empty()) {
        // the sets were found on the caller's CSR; theta / den on the device are in the library's numbering
        const auto &m = tid_map(ctx);
        try {
            std::vector<uint8_t> kind(S.kind.size());
            std::vector<double> usum(S.usum.size());
            for (size_t t = 0; t < m.size(); t++) { kind[(size_t)m[t]] = S.kind[t]; usum[(size_t)m[t]] = S.usum[t]; }
            S.kind.swap(kind); S.usum.swap(usum);
        } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
        for (int32_t &t : S.g_tid) t = m[(size_t)t];
        for (int32_t &t : S.CL.g_tid) t = m[(size_t)t];
    }
    HIPCHK(ctx->sets.d_kind.upload(S.kind.data(), S.kind.size()));
    HIPCHK(ctx->sets.d_usum.upload(S.usum.data(), S.usum.size()));
    const int64_t n = S.n_resident();
    if (n > 0) {
        HIPCHK(ctx->sets.d_g_tid.upload(S.g_tid.data(), S.g_tid.size()));
        HIPCHK(ctx->sets.d_g_u.upload(S.g_u.data(), S.g_u.size()));
        HIPCHK(ctx->sets.d_row_w.upload(S.row_w.data(), S.row_w.size()));
        HIPCHK(ctx->sets.d_srp.upload(S.rp.data(), S.rp.size()));
        HIPCHK(ctx->sets.d_sent.upload(S.ent.data(), S.ent.size()));
        HIPCHK(ctx->sets.d_scp.upload(S.cp.data(), S.cp.size()));
        HIPCHK(ctx->sets.d_scrow.upload(S.crow.data(), S.crow.size()));
        for (int c = 0; c < emsar::kSetClasses; c++)
            if (!S.desc[c].empty()) HIPCHK(ctx->sets.d_sdesc[c].upload(S.desc[c].data(), S.desc[c].size()));
        HIPCHK(ctx->sets.d_sstat.alloc((size_t)n));
        HIPCHK(ctx->sets.h_sstat.alloc((size_t)n));
        ctx->sets.n_sstat = n;
        HIPCHK(hipFuncSetAttribute((const void *)k_solve_sets<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)emsar::kSetLdsCap[0]));
        HIPCHK(hipFuncSetAttribute((const void *)k_solve_sets<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)emsar::kSetLdsCap[1]));
        HIPCHK(hipFuncSetAttribute((const void *)k_solve_sets<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)emsar::kSetLdsCap[2]));
    }
    const int64_t nc = S.n_cluster_sets();
    if (nc > 0) {
        auto &CL = S.CL;
        HIPCHK(ctx->sets.d_cdesc.upload(CL.desc.data(), CL.desc.size()));
        HIPCHK(ctx->sets.d_cblk.upload(CL.blk_set.data(), CL.blk_set.size()));
        HIPCHK(ctx->sets.d_crp.upload(CL.rp.data(), CL.rp.size()));
        HIPCHK(ctx->sets.d_ccp.upload(CL.cp.data(), CL.cp.size()));
        HIPCHK(ctx->sets.d_cpart.upload(CL.part.data(), CL.part.size()));
        HIPCHK(ctx->sets.d_cent.upload(CL.ent.data(), CL.ent.size()));
        HIPCHK(ctx->sets.d_ccrow.upload(CL.crow.data(), CL.crow.size()));
        HIPCHK(ctx->sets.d_cg_tid.upload(CL.g_tid.data(), CL.g_tid.size()));
        HIPCHK(ctx->sets.d_cg_u.upload(CL.g_u.data(), CL.g_u.size()));
        HIPCHK(ctx->sets.d_crow_w.upload(CL.row_w.data(), CL.row_w.size()));
        HIPCHK(ctx->sets.d_cscratch.alloc((size_t)CL.scratch_doubles));
        HIPCHK(ctx->sets.d_cbar.alloc((size_t)nc * 2));
        HIPCHK(ctx->sets.d_cstat.alloc((size_t)nc));
        HIPCHK(ctx->sets.h_cstat.alloc((size_t)nc));
        ctx->sets.n_cstat = nc;
        HIPCHK(hipFuncSetAttribute((const void *)k_solve_cluster, hipFuncAttributeMaxDynamicSharedMemorySize, (int)emsar::kClusterLdsCap));
        // only the sizes are needed from here on
        std::vector<uint32_t>().swap(CL.rp); std::vector<uint32_t>().swap(CL.cp); std::vector<uint16_t>().swap(CL.ent); std::vector<uint16_t>().swap(CL.crow);
        std::vector<int32_t>().swap(CL.g_tid); std::vector<double>().swap(CL.g_u); std::vector<double>().swap(CL.row_w);
    }
    // the device copies are the only ones needed from here on (desc sizes and counters stay)
    std::vector<int32_t>().swap(S.g_tid); std::vector<double>().swap(S.g_u); std::vector<double>().swap(S.row_w);
    std::vector<uint16_t>().swap(S.rp); std::vector<uint16_t>().swap(S.ent); std::vector<uint16_t>().swap(S.cp); std::vector<uint16_t>().swap(S.crow);
    std::vector<double>().swap(S.usum);
    ctx->sets_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->sets.sets_ready = true;
    return EMSAR_HIP_OK;
}

// The three size classes of the set solver are independent (disjoint sets, disjoint theta entries): the larger two run on side streams next to
// the 64-thread class.  fork_side_streams: the first n_side side streams wait for ctx->stream; launch_set_classes: launch(class, threads,
// stream) for every class that has sets, the big ones first (the fewest, the longest per pass), then ctx->stream waits for those side streams.
int fork_side_streams(emsar_hip_ctx *ctx, int n_side) {
    HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int i = 0; i < n_side; i++) HIPCHK(hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0));
    return EMSAR_HIP_OK;
}
template <class Launch>
int launch_set_classes(emsar_hip_ctx *ctx, int n_side, const Launch &launch) {
    const hipStream_t st[emsar::kSetClasses] = {ctx->stream, ctx->side[0], ctx->side[1]};
    for (int c = emsar::kSetClasses - 1; c >= 0; c--) if (!ctx->sets.RS.desc[c].empty()) launch(c, emsar::kSetThreads[c], st[c]);
    for (int i = 0; i < n_side; i++) {
        HIPCHK(hipEventRecord(ctx->ev_join[i], ctx->side[i]));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
    }
    HIPCHK(hipGetLastError());
    return EMSAR_HIP_OK;
}

// closed-form transcripts and every LDS-resident set, written into theta (the streamed sets' entries are left alone)
int solve_resident_sets(emsar_hip_ctx *ctx, const SetSolveParams &P, const SetSolveParams &Pcluster, double *theta) {
    const auto &S = ctx->sets.RS;
    hipLaunchKernelGGL(k_closed_form, dim3(grid_for(ctx->n_tx, 256)), dim3(256), 0, ctx->stream, ctx->n_tx, ctx->sets.d_kind, ctx->sets.d_usum,
                       ctx->vec.d_den, theta);
    const size_t off[3] = {0, S.desc[0].size(), S.desc[0].size() + S.desc[1].size()};      // per-set results in class order
    if (const int rc = fork_side_streams(ctx, 3)) return rc;
    if (ctx->sets.n_cstat > 0) {
        // The clusters, on a stream of their own.  Every workgroup of a launch must be resident at once (they wait for each other at
        // the cluster barriers): at most one workgroup per CU per launch -- each asks for most of a CU's LDS --, whole sets only.
        const int n_cu = ctx->n_cu;
        HIPCHK(hipMemsetAsync(ctx->sets.d_cbar, 0, (size_t)ctx->sets.n_cstat * 2 * sizeof(unsigned), ctx->side[2]));
        HIPCHK(hipEventRecord(ctx->ev_c0, ctx->side[2]));
        const auto &D = S.CL.desc;
        size_t first = 0;
        while (first < D.size()) {
            size_t last = first, wgs = 0;
            while (last < D.size() && (wgs == 0 || wgs + D[last].g <= (size_t)n_cu)) wgs += D[last++].g;
            hipLaunchKernelGGL(k_solve_cluster, dim3((unsigned)wgs), dim3(emsar::kClusterThreads), S.CL.max_lds, ctx->side[2], ctx->sets.d_cdesc, ctx->sets.d_cblk,
                               D[first].blk0, ctx->sets.d_cg_tid, ctx->sets.d_cg_u, ctx->sets.d_crow_w, ctx->sets.d_crp, ctx->sets.d_cent, ctx->sets.d_ccp, ctx->sets.d_ccrow, ctx->sets.d_cpart,
                               ctx->sets.d_cscratch, ctx->sets.d_cbar, ctx->sets.d_cbar + ctx->sets.n_cstat, ctx->vec.d_den, theta, ctx->sets.d_cstat, Pcluster);
            first = last;
        }
        HIPCHK(hipEventRecord(ctx->ev_c1, ctx->side[2]));
        // The workgroups of a cluster wait for each other inside the launch, so all of them must get a CU: nothing else may hold CUs while
        // the cluster batches run (k_solve_sets<512> asks for most of a CU's LDS too).  The size classes below start after the clusters.
        HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_c1, 0));
        HIPCHK(hipStreamWaitEvent(ctx->side[1], ctx->ev_c1, 0));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_c1, 0));
    }
    return launch_set_classes(ctx, 3, [&](int c, int threads, hipStream_t st) {
        hipLaunchKernelGGL((c == 2 ? k_solve_sets<512> : c == 1 ? k_solve_sets<256> : k_solve_sets<64>), dim3((unsigned)S.desc[c].size()), dim3(threads),
                           S.max_lds[c], st, ctx->sets.d_sdesc[c], ctx->sets.d_g_tid, ctx->sets.d_g_u, ctx->sets.d_row_w, ctx->sets.d_srp, ctx->sets.d_sent, ctx->sets.d_scp,
                           ctx->sets.d_scrow, ctx->vec.d_den, theta, ctx->sets.d_sstat + off[c], P);
    });
}

}  // namespace

hipStream_t emsar_internal_stream(emsar_hip_ctx *ctx) { return ctx->stream; }
int emsar_internal_device(const emsar_hip_ctx *ctx) { return ctx->device; }
void emsar_internal_set_error(emsar_hip_ctx *ctx, const char *call, const char *what) { ctx->err = std::string(call) + ": " + what; }

// ==================================================================================================
// C ABI
// ==================================================================================================
extern "C" {

const char *emsar_hip_strerror(int status) {
    switch (status) {
        case EMSAR_HIP_OK: return "ok";
        case EMSAR_HIP_ERR_ARG: return "invalid argument or malformed CSR";
        case EMSAR_HIP_ERR_NO_DEVICE: return "no usable HIP device";
        case EMSAR_HIP_ERR_OOM: return "out of memory";
        case EMSAR_HIP_ERR_HIP: return "HIP runtime failure";
        case EMSAR_HIP_ERR_STATE: return "wrong call order (upload_structure -> upload_sample -> solve)";
        case EMSAR_HIP_ERR_NUMERIC: return "NaN/Inf in theta";
        default: return "unknown status";
    }
}

const char *emsar_hip_last_error(const emsar_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

int emsar_hip_create(emsar_hip_ctx **out, int device_id) {
    if (!out) return EMSAR_HIP_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return EMSAR_HIP_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return EMSAR_HIP_ERR_NO_DEVICE;
    emsar_hip_ctx *ctx = new (std::nothrow) emsar_hip_ctx();
    if (!ctx) return EMSAR_HIP_ERR_OOM;
    ctx->device = device_id;
    auto fail = [&](int rc) { emsar_hip_destroy(ctx); return rc; };
    if (hipSetDevice(device_id) != hipSuccess) return fail(EMSAR_HIP_ERR_NO_DEVICE);
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && v > 0) ctx->n_cu = v; }
    if (const char *e = getenv("EMSAR_HIP_GRAPH")) ctx->use_graph = atoi(e) != 0;
    if (const char *e = getenv("EMSAR_HIP_DETERMINISTIC")) ctx->det = atoi(e) != 0;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return fail(EMSAR_HIP_ERR_HIP);
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess || hipEventCreate(&ctx->ev2) != hipSuccess) return fail(EMSAR_HIP_ERR_HIP);
    if (hipEventCreate(&ctx->ev_c0) != hipSuccess || hipEventCreate(&ctx->ev_c1) != hipSuccess) return fail(EMSAR_HIP_ERR_HIP);
    for (int i = 0; i < 3; i++)
        if (hipStreamCreateWithFlags(&ctx->side[i], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming) != hipSuccess) return fail(EMSAR_HIP_ERR_HIP);
    if (hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess) return fail(EMSAR_HIP_ERR_HIP);
    if (ctx->d_scal.alloc(1) != hipSuccess) return fail(EMSAR_HIP_ERR_OOM);
    if (ctx->d_sqpart.alloc(4 * kSqPart) != hipSuccess) return fail(EMSAR_HIP_ERR_OOM);
    if (hipMemset(ctx->d_sqpart, 0, 4 * kSqPart * sizeof(double)) != hipSuccess) return fail(EMSAR_HIP_ERR_HIP);
    if (ctx->h_scal.alloc(1) != hipSuccess) return fail(EMSAR_HIP_ERR_OOM);
    *out = ctx;
    return EMSAR_HIP_OK;
}

int emsar_hip_set_deterministic(emsar_hip_ctx *ctx, int on) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    ctx->det = on != 0;
    return EMSAR_HIP_OK;
}

void emsar_hip_destroy(emsar_hip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_structure(ctx);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_c0) (void)hipEventDestroy(ctx->ev_c0);
    if (ctx->ev_c1) (void)hipEventDestroy(ctx->ev_c1);
    for (int i = 0; i < 3; i++) {
        if (ctx->side[i]) { (void)hipStreamSynchronize(ctx->side[i]); (void)hipStreamDestroy(ctx->side[i]); }
        if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;     // its buffers of the context's own lifetime go with it
}

int emsar_hip_upload_structure(emsar_hip_ctx *ctx, int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr,
                               const int32_t *col_idx, int layout) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    const bool merge_rows = (layout & EMSAR_LAYOUT_FLAG_MERGE_ROWS) != 0;
    layout &= ~EMSAR_LAYOUT_FLAG_MERGE_ROWS;
    if (layout != EMSAR_LAYOUT_AUTO && layout != EMSAR_LAYOUT_CSR && layout != EMSAR_LAYOUT_TILED) return EMSAR_HIP_ERR_ARG;
    if (merge_rows && layout != EMSAR_LAYOUT_AUTO && layout != EMSAR_LAYOUT_TILED) return EMSAR_HIP_ERR_ARG;
    if (emsar::validate_csr(n_rows, n_tx, row_ptr, col_idx) != 0) return EMSAR_HIP_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    free_structure(ctx);
    ctx->n_rows = n_rows; ctx->n_tx = n_tx; ctx->nnz = (int64_t)row_ptr[n_rows];
    ctx->ptr64 = (uint64_t)ctx->nnz >= (1ull << 32);
    if (const char *e = getenv("EMSAR_HIP_FORCE_PTR64")) { if (atoi(e) != 0) ctx->ptr64 = true; }   // test hook: the 64-bit row_ptr kernels on small inputs
    if (layout == EMSAR_LAYOUT_AUTO) {
        layout = (n_rows < ((int64_t)1 << 32)) ? EMSAR_LAYOUT_TILED : EMSAR_LAYOUT_CSR;
        if (const char *e = getenv("EMSAR_HIP_LAYOUT")) { int v = atoi(e); if ((v == 1 || v == 3) && (v == 1 || n_rows < ((int64_t)1 << 32))) layout = v; }
        if (merge_rows && layout != EMSAR_LAYOUT_TILED) return EMSAR_HIP_ERR_ARG;
    }
    ctx->layout = layout;
    const size_t T = (size_t)n_tx;
    const bool dbg = getenv("EMSAR_HIP_DEBUG") != nullptr;
    const auto tu0 = std::chrono::steady_clock::now();
    auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    // the host copy of the CSR kept for the set-resident solver (built per sample: sets depend on which rows carry reads)
    // is made by a second thread while this one builds the device layout from the same arrays
    bool copy_failed = false;
    std::thread csr_copy([&] {
        try {
            ctx->h_row_ptr.assign(row_ptr, row_ptr + n_rows + 1);
            ctx->h_col.assign(col_idx, col_idx + ctx->nnz);
        } catch (const std::bad_alloc &) { copy_failed = true; }
    });
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{csr_copy};
    try {
        if (layout == EMSAR_LAYOUT_TILED) {
            auto &L = ctx->lay.TL;
            const int brc = emsar::build_tiled(n_rows, n_tx, row_ptr, col_idx, L, merge_rows);
            if (brc != 0) { ctx->err = "TILED layout builder: code " + std::to_string(brc); return EMSAR_HIP_ERR_ARG; }
            if (dbg) fprintf(stderr, "upload_structure: layout built after %.0f ms\n", since(tu0));
            ctx->lay.n_tiles = (int64_t)L.tiles.size(); ctx->lay.n_slots = L.n_slots(); ctx->lay.n_left = (int64_t)L.left_row.size();
            HIPCHK(ctx->lay.d_tiles.upload(L.tiles.data(), L.tiles.size()));
            HIPCHK(ctx->lay.d_units.upload(L.unit_first.data(), L.unit_first.size()));
            ctx->lay.n_units = L.unit_first.empty() ? 0 : (int64_t)L.unit_first.size() - 1;
            {
                emsar::UnitTables U;
                emsar::build_unit_tables(L, U);
                ctx->lay.unit_stride = U.stride;
                HIPCHK(ctx->lay.d_utiles.upload(U.utiles.data(), U.utiles.size()));
            }
            HIPCHK(ctx->lay.d_fwd.upload(L.fwd.data(), L.fwd.size()));
            HIPCHK(ctx->lay.d_bwd.upload(L.bwd.data(), L.bwd.size()));
            HIPCHK(ctx->lay.d_far.upload(L.far_tid.data(), L.far_tid.size()));
            HIPCHK(ctx->lay.d_left_ptr.upload(L.left_ptr.data(), L.left_ptr.size()));
            HIPCHK(ctx->lay.d_left_col.upload(L.left_col.data(), L.left_col.size()));
            HIPCHK(ctx->lay.d_u.alloc(T));
            HIPCHK(hipMemset(ctx->lay.d_u, 0, T * 8));
            ctx->bytes_stored = (int64_t)L.fwd.size() * 4 + (int64_t)L.bwd.size() * 4 + (int64_t)L.far_tid.size() * 4 +
                                (int64_t)L.tiles.size() * 64 + (int64_t)L.left_col.size() * 4 + (int64_t)L.left_ptr.size() * 8;
            ctx->tl_fwd_slots = L.padded_slots; ctx->tl_n_fslices = L.n_fslices;
            emsar::u32_vec().swap(L.fwd); emsar::u32_vec().swap(L.bwd);
            std::vector<int32_t>().swap(L.left_col);
            HIPCHK(set_tiled_lds_attributes());
            { const char *pe = getenv("EMSAR_HIP_WEIGHTED_UNIT"); ctx->weighted_unit = pe ? atoi(pe) : 1; }
            { const char *pe = getenv("EMSAR_HIP_TILED_MULTI"); ctx->tiled_multi = pe ? atoi(pe) : 1; }
            { const char *pe = getenv("EMSAR_HIP_UPDATE_GRID"); if (pe && atoi(pe) >= 1) ctx->update_grid = atoi(pe); }
            { const char *pe = getenv("EMSAR_HIP_SQ_GRID"); if (pe && atoi(pe) >= 1) ctx->sq_grid = atoi(pe); }
        } else {
            if (ctx->ptr64) {
                HIPCHK(ctx->lay.d_row_ptr.upload(row_ptr, ((size_t)n_rows + 1) * 8));
            } else {
                std::vector<uint32_t> rp((size_t)n_rows + 1);
                for (int64_t r = 0; r <= n_rows; r++) rp[(size_t)r] = (uint32_t)row_ptr[r];
                HIPCHK(ctx->lay.d_row_ptr.upload(rp.data(), rp.size() * 4));
            }
            HIPCHK(ctx->lay.d_col.upload(col_idx, (size_t)ctx->nnz));
            ctx->bytes_stored = ctx->nnz * 4 + (n_rows + 1) * (ctx->ptr64 ? 8 : 4);
        }
    } catch (const std::bad_alloc &) {
        csr_copy.join();
        free_structure(ctx);
        return EMSAR_HIP_ERR_OOM;
    }
    if (dbg) fprintf(stderr, "upload_structure: device copies done after %.0f ms\n", since(tu0));
    csr_copy.join();
    if (copy_failed) { free_structure(ctx); return EMSAR_HIP_ERR_OOM; }
    if (dbg) fprintf(stderr, "upload_structure: host CSR copy joined after %.0f ms\n", since(tu0));
    HIPCHK(ctx->vec.d_den.alloc(T));
    HIPCHK(ctx->vec.d_acc.alloc(T));
    for (auto &p : ctx->vec.d_th) HIPCHK(p.alloc(T));
    for (auto &p : ctx->vec.d_tmp) HIPCHK(p.alloc(T));
    HIPCHK(ctx->vec.d_itmp.alloc(T));
    HIPCHK(hipMemset(ctx->vec.d_acc, 0, T * 8));
    ctx->have_structure = true;
    return EMSAR_HIP_OK;
}

int emsar_hip_upload_sample(emsar_hip_ctx *ctx, const int32_t *row_weight, const double *row_E, const double *den) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int64_t n_rows = ctx->n_rows;
    // arguments first: a rejected call changes nothing
    if (row_weight || row_E) {
        for (int64_t r = 0; r < n_rows; r++) {
            if (row_weight && row_weight[r] < 0) return EMSAR_HIP_ERR_ARG;
            if (row_E && !(row_E[r] >= 0.0)) return EMSAR_HIP_ERR_ARG;  // negative or NaN
        }
    }
    if (den) for (int32_t t = 0; t < ctx->n_tx; t++) if (!(den[t] >= 0.0)) return EMSAR_HIP_ERR_ARG;
    // from here on the previous sample is gone: a call that fails half way (out of memory, HIP error) must not leave a
    // context that still says have_sample with its weight arrays freed (run_passes would launch kernels on null pointers)
    ctx->have_sample = false;
    // a row counts w = R (or 1) when it is inside the likelihood (E != 0), else 0
    ctx->weighted = (row_weight != nullptr) || (row_E != nullptr) || (ctx->layout == EMSAR_LAYOUT_TILED && ctx->lay.TL.merged);
    ctx->loglik_const = 0.0;
    ctx->rw = RowWeights();
    auto weight_of = [&](int64_t r) -> int32_t {
        int32_t x = row_weight ? row_weight[r] : 1;
        if (row_E && row_E[r] == 0.0) x = 0;
        return x;
    };
    ctx->sets = SetsDev();
    try {
        ctx->h_wgt.resize((size_t)n_rows);
        int64_t total_w = 0;
        for (int64_t r = 0; r < n_rows; r++) { const int32_t x = weight_of(r); ctx->h_wgt[(size_t)r] = x; total_w += x; }
        set_fx_scales(ctx, total_w);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    {
        LayoutWeights LW;
        try {
            int rc = layout_weights(ctx, weight_of, row_E, ctx->weighted, LW, ctx->loglik_const);
            if (rc || (rc = upload_layout_weights(ctx, LW, ctx->weighted))) return rc;
        } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    }
    if (den) {
        std::vector<double> tmp;
        try { den = to_lib(ctx, den, tmp); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
        HIPCHK(hipMemcpy(ctx->vec.d_den, den, (size_t)ctx->n_tx * 8, hipMemcpyHostToDevice));
    } else {
        std::vector<double> ones;
        const double *e = row_E;
        if (!e) { ones.assign((size_t)std::max<int64_t>(n_rows, 1), 1.0); e = ones.data(); }
        int rc = scatter_rows(ctx, e, ctx->vec.d_den);
        if (rc) return rc;
    }
    ctx->bytes_formula = 4 * ctx->nnz + (ctx->ptr64 ? 8 : 4) * (ctx->n_rows + 1) + (row_weight ? 4 : 0) * ctx->n_rows + 32 * (int64_t)ctx->n_tx;
    ctx->have_sample = true;
    return emsar_hip_reset_theta(ctx);
}

int emsar_hip_reset_theta(emsar_hip_ctx *ctx) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_fill_start, dim3(grid_for(ctx->n_tx, 256)), dim3(256), 0, ctx->stream, ctx->n_tx, ctx->vec.d_den, ctx->vec.d_th[0]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return EMSAR_HIP_OK;
}

int emsar_hip_set_theta(emsar_hip_ctx *ctx, const double *theta) {
    if (!ctx || !theta) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> tmp;
    try { theta = to_lib(ctx, theta, tmp); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    HIPCHK(hipMemcpyAsync(ctx->vec.d_th[0], theta, (size_t)ctx->n_tx * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return EMSAR_HIP_OK;
}

int emsar_hip_get_theta(emsar_hip_ctx *ctx, double *theta) {
    if (!ctx || !theta) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(theta, ctx->vec.d_th[0], (size_t)ctx->n_tx * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    try { from_lib(ctx, theta); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

int emsar_hip_run_passes(emsar_hip_ctx *ctx, int32_t n_passes, float *elapsed_ms, double *last_ll) {
    if (!ctx || n_passes < 0) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->delta_mask = nullptr;
    hipLaunchKernelGGL(k_cycle_begin, dim3(1), dim3(kLlSlots), 0, ctx->stream, ctx->d_scal, 0.0, 0);
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    int cur = 0;  // th[cur] holds the current point, th[cur^1] receives the next
    for (int i = 0; i < n_passes; i++) {
        bool ll = last_ll && i == n_passes - 1;
        int rc = em_pass(ctx, ctx->vec.d_th[cur], ctx->vec.d_th[cur ^ 1], ll, 0, 1e-6);
        if (rc) return rc;
        cur ^= 1;
    }
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    if (cur == 1) HIPCHK(hipMemcpyAsync(ctx->vec.d_th[0], ctx->vec.d_th[1], (size_t)ctx->n_tx * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, sizeof(Scal), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (elapsed_ms) HIPCHK(hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    if (last_ll) *last_ll = host_ll(ctx, 0);
    return EMSAR_HIP_OK;
}

static int solve_impl(emsar_hip_ctx *ctx, const emsar_em_params *pp, double *fpkm_out, emsar_em_stats *stats);
// the caller's parameters with the defaults filled in
static emsar_em_params solve_params(const emsar_em_params *pp) {
    emsar_em_params p = pp ? *pp : emsar_em_params{0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (p.max_iter <= 0) p.max_iter = 100000;
    if (p.tol <= 0) p.tol = 1e-10;
    if (p.abs_floor <= 0) p.abs_floor = 1e-6;
    if (p.check_every <= 0) p.check_every = 8;
    return p;
}
// what the resident sets get of them
static SetSolveParams set_params(const emsar_em_params &p) {
    // zero_cut / abs_step exist because a boundary optimum is approached like 1/k by the EM; the sets that get Newton steps reach it
    // in a few steps and are held to the strict rule (same pass counts with and without the two rules on every problem measured,
    // and then nothing is printed differently); the rules stay in force for the streamed part and with newton_after < 0
    const bool strict_sets = p.newton_after >= 0;
    return SetSolveParams{p.tol, p.abs_floor, p.count_floor, (!strict_sets && p.zero_cut > 0.0) ? p.zero_cut : 0.0,
                          (!strict_sets && p.abs_step > 0.0) ? p.abs_step : 0.0, p.max_iter, p.accel, p.newton_after == 0 ? 60 : p.newton_after};
}
int emsar_hip_solve(emsar_hip_ctx *ctx, const emsar_em_params *pp, double *fpkm_out, emsar_em_stats *stats) {
    if (!ctx || !fpkm_out) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample) return EMSAR_HIP_ERR_STATE;
    const int rc = solve_impl(ctx, pp, fpkm_out, stats);
    clear_solve_state(ctx);
    return rc;
}
static int solve_impl(emsar_hip_ctx *ctx, const emsar_em_params *pp, double *fpkm_out, emsar_em_stats *stats) {
    emsar_em_params p = solve_params(pp);
    if (!(p.count_floor >= 0.0)) return EMSAR_HIP_ERR_ARG;
    if (p.set_mode != 0 && p.set_mode != 1) return EMSAR_HIP_ERR_ARG;
    ctx->count_floor = p.count_floor;
    ctx->zero_cut = p.zero_cut > 0.0 ? p.zero_cut : 0.0;
    const double abs_step_base = p.abs_step > 0.0 ? p.abs_step : 0.0;
    ctx->delta_mask = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    bool use_sets = p.set_mode == 0;
    if (use_sets && (rc = ensure_sets(ctx))) return rc;
    if (use_sets && ctx->sets.RS.giant) use_sets = false;      // one component holds most transcripts: plain streaming solve
    // the streaming passes run when asked for, or for the sets that do not fit a workgroup
    const bool need_stream = !use_sets || ctx->sets.RS.n_streamed_sets > 0;
    if (use_sets && need_stream) ctx->delta_mask = ctx->sets.d_kind;
    auto t0 = std::chrono::steady_clock::now();
    if ((rc = emsar_hip_reset_theta(ctx))) return rc;
    hipLaunchKernelGGL(k_scal_init, dim3(1), dim3(1), 0, ctx->stream, ctx->d_scal);
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    const int n = ctx->n_tx, g = grid_for(n, 256);
    DevBuf<double> *th = ctx->vec.d_th;  // 0:th0 1:th1 2:th2 3:thx 4:thn (enqueue_cycles leaves the current point in th[0])
    int iters = 0, converged = need_stream ? 0 : 1, cycles = 0;
    double delta = need_stream ? INFINITY : 0.0;
    // The first 4 x check_every cycles are launched kernel by kernel (a quick solve never pays for a graph); after that
    // check_every cycles are recorded once into a hipGraph and replayed between the host's looks at the stopping rule.
    // Measured gain: 1-5 % on problems of 40 k .. 2 M rows (tools/graph_bench.py) -- the launches were already asynchronous,
    // and a pass of a small problem costs one workgroup's latency (12-26 us), not its launch.
    const int per_cycle = p.accel ? 3 : 1;
    const bool graph_ok = ctx->use_graph && (p.accel || p.check_every % 2 == 0);   // plain EM swaps th0/th1: an even count restores them
    CycleGraph G;
    ctx->graph_launches = 0;
    while (need_stream && iters < p.max_iter) {
        int todo = 1;
        if (graph_ok && cycles >= 4 * p.check_every && cycles % p.check_every == 0 &&
            (int64_t)iters + (int64_t)per_cycle * p.check_every <= (int64_t)p.max_iter) {
            todo = p.check_every;
            if (!G.exec) {
                HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
                rc = enqueue_cycles(ctx, p, abs_step_base, todo);
                hipError_t e = hipStreamEndCapture(ctx->stream, &G.graph);      // always closes the capture
                if (rc) return rc;
                HIPCHK(e);
                HIPCHK(hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0));
            }
            HIPCHK(hipGraphLaunch(G.exec, ctx->stream));
            ctx->graph_launches++;
        } else if ((rc = enqueue_cycles(ctx, p, abs_step_base, 1))) return rc;
        cycles += todo;
        iters += todo * per_cycle;
        if (cycles % p.check_every == 0 || iters >= p.max_iter) {
            HIPCHK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, sizeof(Scal), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            unsigned long long bits = p.accel ? ctx->h_scal->delta1_bits : ctx->h_scal->delta_bits;
            memcpy(&delta, &bits, 8);
            if (!std::isfinite(delta) || ctx->h_scal->bad) { ctx->err = "non-finite theta"; return EMSAR_HIP_ERR_NUMERIC; }
            if (delta < p.tol) { converged = 1; break; }
        }
    }
    ctx->delta_mask = nullptr;
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    if (use_sets) {
        const SetSolveParams P = set_params(p);
        // the cluster solver has no Newton step: its sets keep the two print-quantum rules whatever newton_after says (with the strict rule
        // alone a boundary optimum keeps a cluster going for 10^5 passes at ~32 us each)
        SetSolveParams Pc = P;
        Pc.zero_cut = p.zero_cut > 0.0 ? p.zero_cut : 0.0;
        Pc.abs_step = p.abs_step > 0.0 ? p.abs_step : 0.0;
        if ((rc = solve_resident_sets(ctx, P, Pc, th[0]))) return rc;
        if (ctx->sets.n_sstat > 0)
            HIPCHK(hipMemcpyAsync(ctx->sets.h_sstat, ctx->sets.d_sstat, (size_t)ctx->sets.n_sstat * sizeof(SetStat), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sets.n_cstat > 0)
            HIPCHK(hipMemcpyAsync(ctx->sets.h_cstat, ctx->sets.d_cstat, (size_t)ctx->sets.n_cstat * sizeof(ClusterStat), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipEventRecord(ctx->ev2, ctx->stream));
    // F at the returned point: one likelihood-only pass (not counted in iters)
    hipLaunchKernelGGL(k_cycle_begin, dim3(1), dim3(kLlSlots), 0, ctx->stream, ctx->d_scal, 0.0, 0);
    if ((rc = launch_pass(ctx, MODE_EM_LL, th[0], ctx->vec.d_acc, &ctx->d_scal->ll[0].s[0].v))) return rc;
    HIPCHK(hipMemsetAsync(ctx->vec.d_acc, 0, (size_t)n * 8, ctx->stream));
    hipLaunchKernelGGL(k_dot, dim3(1), dim3(1024), 0, ctx->stream, n, th[0], ctx->vec.d_den, &ctx->d_scal->ll[3].s[0].v);
    HIPCHK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, sizeof(Scal), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(fpkm_out, th[0], (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    try { from_lib(ctx, fpkm_out); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    ctx->count_floor = 0.0; ctx->zero_cut = 0.0;
    if (getenv("EMSAR_HIP_DEBUG"))
        fprintf(stderr, "emsar_hip_solve: %d streaming passes, %lld graph replays of %d cycles\n", iters, (long long)ctx->graph_launches, p.check_every);
    for (int32_t t = 0; t < n; t++)
        if (!std::isfinite(fpkm_out[t])) { ctx->err = "non-finite theta"; return EMSAR_HIP_ERR_NUMERIC; }
    int32_t set_max = 0, set_unconv = 0;
    int64_t set_sum = 0;
    if (use_sets)
        for (int64_t i = 0; i < ctx->sets.n_sstat; i++) {
            const SetStat &q = ctx->sets.h_sstat[i];
            set_max = std::max(set_max, q.passes); set_sum += q.passes;
            if (!q.converged) set_unconv++;
            if (!std::isfinite(q.delta)) { ctx->err = "non-finite theta in a connected set"; return EMSAR_HIP_ERR_NUMERIC; }
            if (q.delta > delta) delta = q.delta;
        }
    int32_t cl_max = 0;
    if (use_sets)
        for (int64_t i = 0; i < ctx->sets.n_cstat; i++) {
            const ClusterStat &q = ctx->sets.h_cstat[i];
            if (q.aborted) { ctx->err = "a workgroup cluster gave up waiting at its barrier"; return EMSAR_HIP_ERR_HIP; }
            cl_max = std::max(cl_max, q.passes); set_sum += q.passes;
            if (!q.converged) set_unconv++;
            if (!std::isfinite(q.delta)) { ctx->err = "non-finite theta in a connected set"; return EMSAR_HIP_ERR_NUMERIC; }
            if (q.delta > delta) delta = q.delta;
        }
    set_max = std::max(set_max, cl_max);
    if (set_unconv) converged = 0;
    if (stats) {
        float ms = 0, ms_sets = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        HIPCHK(hipEventElapsedTime(&ms_sets, ctx->ev1, ctx->ev2));
        memset(stats, 0, sizeof(*stats));
        stats->iters = iters + set_max;
        stats->converged = converged;
        stats->final_delta = delta;
        stats->loglik = host_ll(ctx, 0) + ctx->loglik_const - ctx->h_scal->ll[3].s[0].v;
        stats->kernel_ms = ms + (use_sets ? ms_sets : 0.0f);
        stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->bytes_per_pass = ctx->bytes_formula;
        stats->stored_bytes_per_pass = stored_bytes(ctx);
        if (p.set_mode == 0 && ctx->sets.RS.giant) { stats->sets_streamed = 1; stats->sets_build_ms = ctx->sets_build_ms; }
        if (use_sets) {
            stats->sets_resident = (int32_t)ctx->sets.RS.n_resident();
            stats->sets_streamed = (int32_t)ctx->sets.RS.n_streamed_sets;
            stats->set_passes_max = set_max;
            stats->sets_unconverged = set_unconv;
            stats->set_passes_sum = set_sum;
            stats->sets_build_ms = ctx->sets_build_ms;
            stats->sets_kernel_ms = ms_sets;
            stats->sets_cluster = (int32_t)ctx->sets.n_cstat;
            stats->cluster_passes_max = cl_max;
            if (ctx->sets.n_cstat > 0) { float mc = 0; HIPCHK(hipEventElapsedTime(&mc, ctx->ev_c0, ctx->ev_c1)); stats->cluster_kernel_ms = mc; }
        }
    }
    return EMSAR_HIP_OK;
}

int emsar_hip_ieuma(emsar_hip_ctx *ctx, const double *row_L, double *ieuma_out) {
    if (!ctx || !row_L || !ieuma_out) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    int rc = scatter_rows(ctx, row_L, ctx->vec.d_tmp[0]);
    if (rc) return rc;
    HIPCHK(hipMemcpy(ieuma_out, ctx->vec.d_tmp[0], (size_t)ctx->n_tx * 8, hipMemcpyDeviceToHost));
    try { from_lib(ctx, ieuma_out); } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

int emsar_hip_normalise(emsar_hip_ctx *ctx, const double *mean_fpkm, const double *ieuma, int64_t total_read_count,
                        double *tpm_out, double *ir_out, int32_t *iri_out) {
    if (!ctx || !mean_fpkm || !ieuma || !tpm_out || !ir_out || !iri_out) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    const int n = ctx->n_tx, g = grid_for(n, 256);
    const size_t B = (size_t)n * 8;
    HIPCHK(hipMemcpyAsync(ctx->vec.d_tmp[0], mean_fpkm, B, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->vec.d_tmp[1], ieuma, B, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(&ctx->d_scal->sum_b, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, ctx->stream, n, ctx->vec.d_tmp[0], &ctx->d_scal->sum_b);
    // tmp[2] <- tpm, acc <- iReadcount (acc is zero between passes and is cleared again below)
    hipLaunchKernelGGL(k_normalise, dim3(g), dim3(256), 0, ctx->stream, n, ctx->vec.d_tmp[0], ctx->vec.d_tmp[1],
                       (double)total_read_count / 1E6, &ctx->d_scal->sum_b, ctx->vec.d_tmp[2], ctx->vec.d_acc, ctx->vec.d_itmp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tpm_out, ctx->vec.d_tmp[2], B, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ir_out, ctx->vec.d_acc, B, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(iri_out, ctx->vec.d_itmp, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->vec.d_acc, 0, B, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return EMSAR_HIP_OK;
}

int emsar_hip_upload_euma(emsar_hip_ctx *ctx, const int32_t *euma, int32_t nfl) {
    if (!ctx || !euma || nfl <= 0) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->euma = AdjEuma();
    const size_t n = (size_t)ctx->n_rows * (size_t)nfl;
    AdjEuma A;                   // moved into the context when it is complete
    HIPCHK(A.d_euma_t.alloc(n));
    HIPCHK(A.d_wf.alloc((size_t)nfl));
    HIPCHK(A.d_adj.alloc((size_t)ctx->n_rows));
    if (n) {
        DevBuf<int32_t> tmp;
        HIPCHK(tmp.alloc(n));
        HIPCHK(hipMemcpyAsync(tmp, euma, n * 4, hipMemcpyHostToDevice, ctx->stream));
        dim3 grid((unsigned)((ctx->n_rows + 63) / 64), (unsigned)((nfl + 63) / 64));
        hipLaunchKernelGGL(k_transpose_i32, grid, dim3(256), 0, ctx->stream, ctx->n_rows, (int)nfl, tmp, A.d_euma_t);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    A.nfl = nfl;
    ctx->euma = std::move(A);
    return EMSAR_HIP_OK;
}

int emsar_hip_adj_euma(emsar_hip_ctx *ctx, const double *wf, double *out) {
    if (!ctx || !wf || !out) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure || ctx->euma.nfl <= 0) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->n_rows == 0) return EMSAR_HIP_OK;
    HIPCHK(hipMemcpyAsync(ctx->euma.d_wf, wf, (size_t)ctx->euma.nfl * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_adj_euma, dim3((unsigned)((ctx->n_rows + 255) / 256)), dim3(256), 0, ctx->stream, ctx->n_rows, (int)ctx->euma.nfl,
                       ctx->euma.d_euma_t, ctx->euma.d_wf, ctx->euma.d_adj);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, ctx->euma.d_adj, (size_t)ctx->n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return EMSAR_HIP_OK;
}

int emsar_hip_get_info(const emsar_hip_ctx *ctx, emsar_hip_info *o) {
    if (!ctx || !o) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_structure) return EMSAR_HIP_ERR_STATE;
    memset(o, 0, sizeof(*o));
    o->n_rows = ctx->n_rows; o->nnz = ctx->nnz; o->n_tx = ctx->n_tx; o->device_id = ctx->device;
    o->layout = ctx->layout | ((ctx->layout == EMSAR_LAYOUT_TILED && ctx->lay.TL.merged) ? EMSAR_LAYOUT_FLAG_MERGE_ROWS : 0);
    if (ctx->layout == EMSAR_LAYOUT_TILED) {
        o->n_chunks = ctx->lay.n_tiles; o->n_slices = ctx->tl_n_fslices; o->padded_entries = ctx->tl_fwd_slots;
        o->far_entries = ctx->lay.TL.far_entries; o->window = emsar::kTileDict;
        o->tiled_entries = ctx->lay.TL.tiled_entries; o->tiled_ids = ctx->lay.TL.tiled_ids; o->renumbered = ctx->lay.TL.renum.applied ? 1 : 0;
        o->n_units = ctx->lay.n_units;
    }
    o->bytes_per_pass = ctx->bytes_formula;
    o->stored_bytes_per_pass = stored_bytes(ctx);
    return EMSAR_HIP_OK;
}

// Diagnostic only (not declared in the public header): one stamped pass of the TILED kernel on the current theta.
// out[0..6] = mean cycles per wave spent in: loads issued + dictionary, barrier, E-step, barrier, M-step, barrier, flush;
// out[7] = tiles.  The result vector theta is left untouched (acc is cleared again).
int emsar_hip_debug_tiled_stamps(emsar_hip_ctx *ctx, double *out) {
    if (!ctx || !out || ctx->layout != EMSAR_LAYOUT_TILED || !ctx->have_sample || ctx->weighted || ctx->lay.n_tiles == 0) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nw = (size_t)ctx->lay.n_tiles * (kTiledThreads / 64), bytes = nw * 8 * sizeof(unsigned long long), lds = kTiledLds;
    DevBuf<unsigned long long> d;
    HIPCHK(d.alloc(nw * 8));
    HIPCHK(hipMemsetAsync(d, 0, bytes, ctx->stream));
    HIPCHK(hipFuncSetAttribute((const void *)k_pass_tiled<false, MODE_EM, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_pass_tiled<false, MODE_EM, true>), dim3((unsigned)ctx->lay.n_tiles), dim3(kTiledThreads), lds, ctx->stream, ctx->lay.d_tiles,
                       ctx->lay.d_fwd, ctx->lay.d_bwd, ctx->lay.d_far, ctx->rw.d_wgt, ctx->lay.d_rowval, ctx->vec.d_th[0], ctx->vec.d_acc, &ctx->d_scal->ll[3].s[0].v, Fx{0.0, 0.0}, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(ctx->vec.d_acc, 0, (size_t)ctx->n_tx * 8, ctx->stream));
    std::vector<unsigned long long> h(nw * 8);
    HIPCHK(hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 7; i++) {
        double sum = 0;
        for (size_t w = 0; w < nw; w++) sum += (double)h[w * 8 + (size_t)i];
        out[i] = sum / (double)nw;   // mean cycles per wave
    }
    out[7] = (double)ctx->lay.n_tiles;
    return EMSAR_HIP_OK;
}

// The same for the unit kernel (the one config 3 runs): out[0..5] = mean cycles per wave in: descriptor + dictionary + first loads,
// barrier, E-steps, M-steps, barrier, flush; out[6] = tiles per unit; out[7] = units.
int emsar_hip_debug_unit_stamps(emsar_hip_ctx *ctx, double *out, unsigned long long *timeline /* NULL or 4 words per unit: start, end (100 MHz ticks), place, tiles */) {
    if (!ctx || !out || ctx->layout != EMSAR_LAYOUT_TILED || !ctx->have_sample || ctx->weighted || ctx->lay.n_units == 0) return EMSAR_HIP_ERR_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nw = (size_t)ctx->lay.n_units * (kTiledThreads / 64), words = nw * 8 + (size_t)ctx->lay.n_units * 4, bytes = words * sizeof(unsigned long long), lds = kTiledLds;
    DevBuf<unsigned long long> d;
    HIPCHK(d.alloc(words));
    HIPCHK(hipMemsetAsync(d, 0, bytes, ctx->stream));
    HIPCHK(hipFuncSetAttribute((const void *)k_pass_tiled_unit<false, MODE_EM, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_pass_tiled_unit<false, MODE_EM, true>), dim3((unsigned)ctx->lay.n_units), dim3(kTiledThreads), lds, ctx->stream, ctx->lay.d_utiles, ctx->lay.unit_stride,
                       ctx->lay.d_far, ctx->lay.d_fwd, ctx->lay.d_bwd, ctx->rw.d_wgt, ctx->vec.d_th[0], ctx->vec.d_acc, &ctx->d_scal->ll[3].s[0].v, Fx{0.0, 0.0}, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(ctx->vec.d_acc, 0, (size_t)ctx->n_tx * 8, ctx->stream));
    std::vector<unsigned long long> h(words);
    HIPCHK(hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (timeline) std::copy(h.begin() + (std::ptrdiff_t)(nw * 8), h.end(), timeline);
    for (int i = 0; i < 7; i++) {
        double sum = 0;
        for (size_t w = 0; w < nw; w++) sum += (double)h[w * 8 + (size_t)i];
        out[i] = sum / (double)nw;
    }
    out[7] = (double)ctx->lay.n_units;
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

int emsar_hip_layout_selfcheck_tiled(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                                     int merge_rows, emsar_hip_info *info_out) {
    try {
        if (emsar::validate_csr(n_rows, n_tx, row_ptr, col_idx) != 0) return EMSAR_HIP_ERR_ARG;
        emsar::TiledLayout L;
        if (emsar::build_tiled(n_rows, n_tx, row_ptr, col_idx, L, merge_rows != 0) != 0) return EMSAR_HIP_ERR_ARG;
        int rc = emsar::check_tiled(L, row_ptr, col_idx);
        if (rc == 0) { emsar::UnitTables U; emsar::build_unit_tables(L, U); rc = emsar::check_unit_tables(L, U); }     // what k_pass_tiled_unit reads first
        if (info_out) {
            memset(info_out, 0, sizeof(*info_out));
            info_out->n_rows = n_rows; info_out->nnz = L.nnz; info_out->n_tx = n_tx;
            info_out->layout = EMSAR_LAYOUT_TILED | (L.merged ? EMSAR_LAYOUT_FLAG_MERGE_ROWS : 0);
            info_out->n_chunks = (int64_t)L.tiles.size();
            info_out->n_slices = L.n_fslices;
            info_out->padded_entries = L.padded_slots; info_out->far_entries = L.far_entries; info_out->window = emsar::kTileDict;
            info_out->stored_bytes_per_pass = (int64_t)L.fwd.size() * 4 + (int64_t)L.bwd.size() * 4 +
                                              (int64_t)L.far_tid.size() * 4 + (int64_t)L.tiles.size() * 64 + (int64_t)L.left_col.size() * 4;
            info_out->bytes_per_pass = (int64_t)L.single_row.size();   /* diagnostic: number of folded single-tid rows */
            info_out->tiled_entries = L.tiled_entries; info_out->tiled_ids = L.tiled_ids; info_out->renumbered = L.renum.applied ? 1 : 0;
            info_out->n_units = L.unit_first.empty() ? 0 : (int64_t)L.unit_first.size() - 1;
        }
        return rc == 0 ? EMSAR_HIP_OK : EMSAR_HIP_ERR_ARG - 100 + rc;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }     // nothing may leave the C ABI as an exception
}

int emsar_hip_sets_selfcheck(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                             const int32_t *row_weight, emsar_hip_sets_info *o) {
    try {
        if (emsar::validate_csr(n_rows, n_tx, row_ptr, col_idx) != 0) return EMSAR_HIP_ERR_ARG;
        if (row_weight) for (int64_t r = 0; r < n_rows; r++) if (row_weight[r] < 0) return EMSAR_HIP_ERR_ARG;
        emsar::ResidentSets S;
        try {
            emsar::build_sets(n_rows, n_tx, row_ptr, col_idx, row_weight, S);
        } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
        int rc = emsar::check_sets(n_rows, n_tx, row_ptr, col_idx, row_weight, S);
        if (o) {
            memset(o, 0, sizeof(*o));
            o->n_components = S.n_components;
            for (int c = 0; c < emsar::kSetClasses; c++) { o->sets_resident[c] = (int64_t)S.desc[c].size(); o->max_lds_bytes[c] = (int64_t)S.max_lds[c]; }
            o->sets_streamed = S.n_streamed_sets;
            o->tids_closed = S.n_closed_tids; o->tids_resident = S.n_resident_tids; o->tids_streamed = S.n_streamed_tids;
            o->rows_in = S.rows_in; o->rows_stored = S.rows_stored + S.CL.rows_stored;
            o->sets_cluster = S.n_cluster_sets(); o->tids_cluster = S.CL.n_tids; o->max_lds_cluster = (int64_t)S.CL.max_lds;
        }
        return rc == 0 ? EMSAR_HIP_OK : EMSAR_HIP_ERR_ARG - 200 + rc;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }     // nothing may leave the C ABI as an exception
}

}  // extern "C"

#include "resample.hpp"   // the resampling driver and its entry points: bootstrap, genes, quantiles, subsampling
#include "fit.hpp"        // the model fit and its entry points (after resample.hpp: the gene step is launch_gene_sums)
