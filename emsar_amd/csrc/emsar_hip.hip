// emsar_hip.hip -- MI355X (gfx950 / CDNA4) abundance-estimation core behind include/emsar_hip.h.
//
// Replaces the reference's run_MLE_threads() (src/emsar_main.c:446; MLE/Fp/lambdap,
// emsar_functions.c:2946-3126) by an EM on the same segment Poisson likelihood:
//     E-step  w_c = R_c / S_c ,  S_c = sum_t m_ct theta_t        (rows with E_c == 0 are outside F)
//     M-step  theta_t <- theta_t * (sum_c m_ct w_c) / den_t ,    den_t = sum_c m_ct E_c
// and compute_iEUMA / the TPM + iReadcount arithmetic of print_FPKMfinal (emsar_functions.c:3176-3232).
//
// One pass is HBM-bound integer streaming plus FP64 adds: ~2 flop per nonzero -- no MFMA.
// This file: the context, its small helpers, and the C ABI of create / upload / theta / normalise / info / self-checks.
//   context      its device and pinned memory lives in DevBuf / PinBuf owners (devmem.hpp), grouped by lifetime: LayoutDev, TxVectors, GeneMap
//                and AdjEuma go with the structure, RowWeights and SetsDev with the sample; a group is dropped by assigning an empty one.
//                Nothing of a solve lives in it (solve.hpp: PassRules)
// The drivers, same translation unit, included where their first user stands:
//   pass_launch.hpp   choose_pass_kernel, one launcher per kernel family, launch_pass; the stamped diagnostic launches
//   solve.hpp         the set solver's driver (ensure_sets, solve_resident_sets), em_pass / enqueue_cycles, SolveRun: one solve in stages;
//                     emsar_hip_solve, emsar_hip_run_passes
//   set_items.hpp     the batch rule (item_batch); SetItemRunner: batches of items, one workgroup each, through a set-kernel family
//                     (presence, profile, compare); SetQuery: where a call's queried transcripts stand in a context before any solve
//   resample.hpp     the resampling driver and its C ABI -- bootstrap, quantiles, subsampling, genes
//   fit.hpp           the model fit and its C ABI
//   presence.hpp      the presence test (a likelihood-ratio test per transcript on its resident set) and its C ABI
//   profile.hpp       the profile-likelihood intervals (two confidence limits per transcript, each a root search over set solves) and their C ABI
//   compare.hpp       the two-sample likelihood-ratio test (two contexts; per transcript a multiplier search over set solves of both samples) and its C ABI
//   gene_parts.hpp    what the gene-level drivers share: the queried genes' members grouped into parts, the owner of a call's part lists
//   compare_genes.hpp the same test per gene (the null on the gene sum; per evaluation a loop over the gene's parts in both samples) and its C ABI
//   asym.hpp          the asymptotic standard errors (the observed information of every component, factorised on the device) and their C ABI
// Kernels (one translation unit, included below):
//   kernels_tiled.hpp     k_pass_tiled_unit                      the hot one (the default above 2048 tiles): one workgroup per UNIT of up to
//                         two tiles of the TILED layout that share a dictionary of theta/acc in LDS (60 blocks x 16 subset sums),
//                         10-bit ids, per-slice transposed index
//                         k_pass_tiled / k_pass_tiled_multi<N>   one tile per workgroup (small problems, weighted likelihood passes,
//                         scatter) / N tiles per workgroup, each with its own dictionary (opt-in: EMSAR_HIP_TILED_MULTI)
//   kernels_csr.hpp       k_pass_csr                             the caller's CSR as it is (layout 1), leftover rows of TILED
//   kernels_vector.hpp    k_update, k_update_p2/p3, k_sq_extrap_ll (SQUAREM extrapolation / acceptance on the device),
//                         k_normalise, k_adj_euma, small reductions
//   kernels_sets.hpp      k_solve_sets                           one workgroup solves one connected set out of LDS
//   kernels_presence.hpp  k_solve_sets_drop                      a set solved without one of its transcripts, and F at the result out of the same LDS
//   kernels_profile.hpp   k_profile_sets                         one workgroup searches one confidence limit: set solves with den_t scaled, F as above
//                         (solve_set_scaled); ProfileStep: the search step kernel and host share; IllinoisBracket
//   kernels_compare.hpp   k_compare_sets                         one workgroup searches one transcript's multiplier: per evaluation a set solve of each sample
//                         (solve_set_scaled); CompareStep: the search step kernel and host share
//   kernels_compare_groups.hpp  k_compare_groups_sets            one workgroup runs one common-value fit of a transcript across a subset
//                         of K samples, two levels (groups_search, shared with the host)
//   kernels_gene_parts.hpp      what the gene-level kernels share: the part lists, solve_gene_part (a set part solved with the members' den
//                         edited; solve_one_set's DenEdit hook), eval_gene_side (one sample: its set parts, then its closed-form parts)
//   kernels_compare_genes.hpp   k_compare_gene_sets              one workgroup searches one gene's multiplier: per evaluation every part of
//                         both samples with the members' den shifted (compare_gene_search, shared with the host)
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
#include <memory>
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
#include "asym_plan.hpp"

#include "kernels_common.hpp"
#include "kernels_csr.hpp"
#include "kernels_tiled.hpp"
#include "kernels_vector.hpp"
#include "kernels_sets.hpp"
#include "kernels_presence.hpp"
#include "kernels_profile.hpp"
#include "kernels_compare.hpp"
#include "kernels_compare_groups.hpp"
#include "kernels_gene_parts.hpp"
#include "kernels_compare_genes.hpp"
#include "kernels_profile_genes.hpp"
#include "kernels_cluster.hpp"
#include "kernels_boot.hpp"
#include "kernels_genes.hpp"
#include "kernels_quant.hpp"
#include "kernels_isoforms.hpp"
#include "kernels_fit.hpp"
#include "kernels_asym.hpp"
#include "kernels_compare_usage.hpp"
#include "kernels_profile_usage.hpp"
#include "kernels_compare_groups_genes.hpp"

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
    std::vector<int32_t> h_gene_of_tx;   // the map as given, caller numbering (asym.hpp: the host finish)
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
    bool use_graph = true;       // replay check_every cycles of the streaming solve from one hipGraph (EMSAR_HIP_GRAPH=0: launch each kernel)
    bool det = false;            // deterministic mode (emsar_hip_set_deterministic / EMSAR_HIP_DETERMINISTIC): fixed-point sums, kernels_common.hpp
    double fx_mass = 0.0, fx_ll = 0.0;   // its scales for the current sample (upload_sample)
    DevBuf<double> d_sqpart;     // per-workgroup partial sums of the SQUAREM vector kernels [4][kSqPart]
    int update_grid = 1024;       // workgroups of k_update (EMSAR_HIP_UPDATE_GRID)
    int sq_grid = 256;           // workgroups of the SQUAREM vector kernels (EMSAR_HIP_SQ_GRID)
    int weighted_unit = 1;       // EMSAR_HIP_WEIGHTED_UNIT: weighted rows on k_pass_tiled_unit -- 1: the plain EM pass, 2: the likelihood passes too, 0: never
    int tiled_multi = 1;         // EMSAR_HIP_TILED_MULTI 1: one unit of up to two tiles per workgroup (k_pass_tiled_unit) above kPairMinTiles tiles,
                                 // else one tile (k_pass_tiled); 5: always units; 2 / 3 / 4: always that many tiles (k_pass_tiled_multi); 0: always one
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
inline bool renumbered(const emsar_hip_ctx *ctx) { return ctx->layout == EMSAR_LAYOUT_TILED && !tid_map(ctx).empty(); }
// the inverse of tid_map: library index -> caller tid; empty = the caller's numbering
inline std::vector<int32_t> caller_of_lib(const emsar_hip_ctx *ctx) {
    const auto &m = tid_map(ctx);
    std::vector<int32_t> inv(renumbered(ctx) ? m.size() : 0);
    for (size_t t = 0; t < inv.size(); t++) inv[(size_t)m[t]] = (int32_t)t;
    return inv;
}
inline const double *to_lib(const emsar_hip_ctx *ctx, const double *caller, std::vector<double> &tmp) {
    const auto &m = tid_map(ctx);
    if (!renumbered(ctx)) return caller;
    tmp.resize(m.size());
    for (size_t t = 0; t < m.size(); t++) tmp[(size_t)m[t]] = caller[t];
    return tmp.data();
}
template <class V> inline void from_lib(const emsar_hip_ctx *ctx, V *v /* in place: library order -> caller order */) {
    const auto &m = tid_map(ctx);
    if (!renumbered(ctx)) return;
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

}  // namespace

#include "pass_launch.hpp"   // choose_pass_kernel, the launchers, launch_pass; the stamped diagnostic launches

namespace {

// a likelihood word of the host copy of the scalars (fixed point in deterministic mode)
inline double host_ll(const emsar_hip_ctx *ctx, int i) {
    const LlSum &L = ctx->h_scal->ll[i];             // the words of the sum, added in a fixed order (kernels_common.hpp)
    if (!ctx->det || ctx->fx_ll == 0.0) { double v = 0.0; for (int j = 0; j < kLlSlots; j++) v += L.s[j].v; return v; }
    long long b = 0;
    for (int j = 0; j < kLlSlots; j++) { long long x; memcpy(&x, &L.s[j].v, 8); b += x; }
    return (double)b / ctx->fx_ll;
}

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


// ---- upload_structure in stages: layout choice, the TILED or the CSR upload, the T-sized vectors ----

// the layout a call asks for: the merge flag taken off, AUTO resolved (EMSAR_HIP_LAYOUT may choose).  ERR_ARG: no such layout, or merged rows without TILED
int choose_layout(int64_t n_rows, int &layout, bool &merge_rows) {
    merge_rows = (layout & EMSAR_LAYOUT_FLAG_MERGE_ROWS) != 0;
    layout &= ~EMSAR_LAYOUT_FLAG_MERGE_ROWS;
    if (layout != EMSAR_LAYOUT_AUTO && layout != EMSAR_LAYOUT_CSR && layout != EMSAR_LAYOUT_TILED) return EMSAR_HIP_ERR_ARG;
    if (layout == EMSAR_LAYOUT_AUTO) {
        layout = (n_rows < ((int64_t)1 << 32)) ? EMSAR_LAYOUT_TILED : EMSAR_LAYOUT_CSR;
        if (const char *e = getenv("EMSAR_HIP_LAYOUT")) { int v = atoi(e); if ((v == 1 || v == 3) && (v == 1 || n_rows < ((int64_t)1 << 32))) layout = v; }
    }
    return merge_rows && layout != EMSAR_LAYOUT_TILED ? EMSAR_HIP_ERR_ARG : EMSAR_HIP_OK;
}

// EMSAR_HIP_DEBUG: where the time of an upload goes
struct UploadTrace {
    const bool on = getenv("EMSAR_HIP_DEBUG") != nullptr;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void say(const char *what) const {
        if (on) fprintf(stderr, "upload_structure: %s after %.0f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// the TILED layout built and on the device; the four launch knobs are read here
int upload_tiled(emsar_hip_ctx *ctx, const uint64_t *row_ptr, const int32_t *col_idx, bool merge_rows, const UploadTrace &trace) {
    auto &L = ctx->lay.TL;
    LayoutDev &D = ctx->lay;
    const size_t T = (size_t)ctx->n_tx;
    const int brc = emsar::build_tiled(ctx->n_rows, ctx->n_tx, row_ptr, col_idx, L, merge_rows);
    if (brc != 0) { ctx->err = "TILED layout builder: code " + std::to_string(brc); return EMSAR_HIP_ERR_ARG; }
    trace.say("layout built");
    D.n_tiles = (int64_t)L.tiles.size(); D.n_slots = L.n_slots(); D.n_left = (int64_t)L.left_row.size();
    HIPCHK(D.d_tiles.upload(L.tiles.data(), L.tiles.size()));
    HIPCHK(D.d_units.upload(L.unit_first.data(), L.unit_first.size()));
    D.n_units = L.unit_first.empty() ? 0 : (int64_t)L.unit_first.size() - 1;
    {
        emsar::UnitTables U;
        emsar::build_unit_tables(L, U);
        D.unit_stride = U.stride;
        HIPCHK(D.d_utiles.upload(U.utiles.data(), U.utiles.size()));
    }
    HIPCHK(D.d_fwd.upload(L.fwd.data(), L.fwd.size()));
    HIPCHK(D.d_bwd.upload(L.bwd.data(), L.bwd.size()));
    HIPCHK(D.d_far.upload(L.far_tid.data(), L.far_tid.size()));
    HIPCHK(D.d_left_ptr.upload(L.left_ptr.data(), L.left_ptr.size()));
    HIPCHK(D.d_left_col.upload(L.left_col.data(), L.left_col.size()));
    HIPCHK(D.d_u.alloc(T));
    HIPCHK(hipMemset(D.d_u, 0, T * 8));
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
    return EMSAR_HIP_OK;
}

// the caller's CSR as it is, row_ptr narrowed to 32 bits when nnz allows
int upload_csr(emsar_hip_ctx *ctx, const uint64_t *row_ptr, const int32_t *col_idx) {
    const int64_t n_rows = ctx->n_rows;
    if (ctx->ptr64) {
        HIPCHK(ctx->lay.d_row_ptr.upload(row_ptr, ((size_t)n_rows + 1) * 8));
    } else {
        std::vector<uint32_t> rp((size_t)n_rows + 1);
        for (int64_t r = 0; r <= n_rows; r++) rp[(size_t)r] = (uint32_t)row_ptr[r];
        HIPCHK(ctx->lay.d_row_ptr.upload(rp.data(), rp.size() * 4));
    }
    HIPCHK(ctx->lay.d_col.upload(col_idx, (size_t)ctx->nnz));
    ctx->bytes_stored = ctx->nnz * 4 + (n_rows + 1) * (ctx->ptr64 ? 8 : 4);
    return EMSAR_HIP_OK;
}

int alloc_tx_vectors(emsar_hip_ctx *ctx) {
    const size_t T = (size_t)ctx->n_tx;
    HIPCHK(ctx->vec.d_den.alloc(T));
    HIPCHK(ctx->vec.d_acc.alloc(T));
    for (auto &p : ctx->vec.d_th) HIPCHK(p.alloc(T));
    for (auto &p : ctx->vec.d_tmp) HIPCHK(p.alloc(T));
    HIPCHK(ctx->vec.d_itmp.alloc(T));
    HIPCHK(hipMemset(ctx->vec.d_acc, 0, T * 8));
    return EMSAR_HIP_OK;
}

// a new structure into an emptied context; the caller frees what a failing exit leaves half built
int upload_structure_impl(emsar_hip_ctx *ctx, int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx, int layout, bool merge_rows) {
    ctx->n_rows = n_rows; ctx->n_tx = n_tx; ctx->nnz = (int64_t)row_ptr[n_rows];
    ctx->ptr64 = (uint64_t)ctx->nnz >= (1ull << 32);
    if (const char *e = getenv("EMSAR_HIP_FORCE_PTR64")) { if (atoi(e) != 0) ctx->ptr64 = true; }   // test hook: the 64-bit row_ptr kernels on small inputs
    ctx->layout = layout;
    const UploadTrace trace;
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
        if (const int rc = layout == EMSAR_LAYOUT_TILED ? upload_tiled(ctx, row_ptr, col_idx, merge_rows, trace) : upload_csr(ctx, row_ptr, col_idx)) return rc;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    trace.say("device copies done");
    csr_copy.join();
    if (copy_failed) return EMSAR_HIP_ERR_OOM;
    trace.say("host CSR copy joined");
    if (const int rc = alloc_tx_vectors(ctx)) return rc;
    ctx->have_structure = true;
    return EMSAR_HIP_OK;
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
    // arguments first: a rejected call changes nothing
    bool merge_rows = false;
    if (choose_layout(n_rows, layout, merge_rows) != EMSAR_HIP_OK) return EMSAR_HIP_ERR_ARG;
    if (emsar::validate_csr(n_rows, n_tx, row_ptr, col_idx) != 0) return EMSAR_HIP_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    free_structure(ctx);
    const int rc = upload_structure_impl(ctx, n_rows, n_tx, row_ptr, col_idx, layout, merge_rows);
    if (rc != EMSAR_HIP_OK) free_structure(ctx);         // a half-built structure is freed, whatever the failing exit
    return rc;
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

#include "solve.hpp"      // the set solver's driver and the solve driver: emsar_hip_solve, emsar_hip_run_passes
#include "set_items.hpp"  // the batch rule, the item runner of the set kernels and the locator (after solve.hpp: fork_side_streams, plan_solve, set_params)
#include "resample.hpp"   // the resampling driver and its entry points: bootstrap, genes, quantiles, subsampling
#include "fit.hpp"        // the model fit and its entry points (after resample.hpp: the gene step is launch_gene_sums)
#include "presence.hpp"   // the presence test and its entry points (after set_items.hpp: SetItemRunner, SetQuery, query_ok)
#include "profile.hpp"    // the profile-likelihood intervals and their entry points (after presence.hpp: PresenceRun)
#include "compare.hpp"    // the two-sample likelihood-ratio test and its entry points (after set_items.hpp: SetItemRunner, SetQuery)
#include "gene_parts.hpp"      // what the gene-level drivers share: GeneQueryMembers, GeneSideParts, GenePartLists (after compare.hpp)
#include "compare_genes.hpp"   // the gene-level two-sample test and its entry points (after gene_parts.hpp; compare.hpp: compare_reduce)
#include "profile_genes.hpp"   // the gene-level profile intervals and the gene presence test (after gene_parts.hpp; profile.hpp: profile_cut)
#include "compare_groups.hpp"  // the K-sample test across replicate groups (after compare.hpp: side_ok; profile_genes.hpp: gene_presence_pvalue)
#include "compare_groups_genes.hpp"  // the gene-level K-sample test (after compare_groups.hpp: GroupsLayout, groups_reduce; gene_parts.hpp)
#include "compare_usage.hpp"   // the two-sample test of isoform usage (after gene_parts.hpp; compare.hpp: compare_pvalue)
#include "profile_usage.hpp"   // the profile intervals of isoform usage (after compare_usage.hpp; profile_genes.hpp: profile_params_ok)
#include "asym.hpp"       //the asymptotic standard errors and their entry points (after fit.hpp: fit_ensure_csr, launch_gene_sums)
