// kernels_asym.hpp -- asymptotic standard errors (emsar_hip_asymptotic): the observed information of every connected component of the
// active transcripts, its LDL^T factorisation, the inverse and what each transcript reads off it.  FP64, no atomics, no fused
// multiply-add: the arithmetic is asym_plan.hpp's, the functions the host restatement calls too; the kernels only hand out rows,
// column elements and row elements to lanes.
//   k_asym_rows         one lane per caller row of the caller-order CSR: S_c, then w_c = R_c / (S_c * S_c).
//   k_asym_single       one lane per one-transcript component: D = J_tt, Sigma = 1 / D, in registers.
//   k_asym_sets<G, T>   G lanes per component, T / G components per workgroup, everything in LDS over a packed lower triangle
//                       (8 n (n + 1) / 2 bytes) next to D[n] and the saved diagonal:
//                         <8, 64>     n <= 8: eight components per wave; every lane group runs the same eight trips under predicates,
//                                     so every barrier is reached by the whole workgroup
//                         <64, 64>    n <= 64: one wave per component, at most 17 KiB
//                         <256, 256>  n <= 192: at most 148 KiB, the dynamic LDS size is opted into by the driver
//                       Lane i builds row i of J from its own entries (no atomics).  Column j of the factorisation has one lane per
//                       i >= j; row i of the inverse one lane per j < i with a read phase and a write phase; Sigma replaces M row by
//                       row from the top (row i of M is dead once Sigma's row i is done), as many whole rows at a time as the group
//                       has lanes.
#pragma once
// included by emsar_hip.hip only (one translation unit: the kernels live in its anonymous namespace)

namespace {

// rows: row_ptr [n_rows + 1], col [nnz] caller tids, wgt [n_rows] R_c, theta [n_tx] caller order -> w [n_rows]
__global__ __launch_bounds__(256) void k_asym_rows(int64_t n_rows, const uint64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                   const int32_t *__restrict__ wgt, const double *__restrict__ theta, double *__restrict__ w) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_rows) return;
    double S = 0.0;
    for (uint64_t k = row_ptr[c]; k < row_ptr[c + 1]; k++) S = S + theta[col[k]];
    w[c] = emsar::asym_row_w((double)wgt[c], S);
}

// what the component kernels write: per slot, per descriptor, the scattered genesum (library index, null without a gene map) and
// the block of one descriptor (block_desc, -1 = none)
struct AsymOut {
    double *var, *rowsum, *gsum, *pcov;
    int32_t *partner, *fail;
    double *ratio;
    const int32_t *lib;
    double *gsum_lib;
    double *block;
    int32_t block_desc;
};

__global__ __launch_bounds__(256) void k_asym_single(emsar::AsymRecords X, const uint32_t *__restrict__ items, int64_t n_items,
                                                     const double *__restrict__ w, double tol, AsymOut O) {
#pragma clang fp contract(off)
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= n_items) return;
    const uint32_t di = items[it];
    const emsar::AsymDesc d = X.desc[di];
    double A[1], D[1], ratio[1];
    emsar::asym_build_row(X, d, 0, w, A);
    D[0] = emsar::asym_col_acc(A, D, 0, 0);
    const int fail = emsar::asym_pivot_ok(D[0], A[0], tol) ? -1 : 0;
    ratio[0] = D[0] / A[0];
    O.fail[di] = fail;
    O.ratio[di] = emsar::asym_min_ratio(ratio, 1, fail);
    if (fail >= 0) return;
    A[0] = emsar::asym_cov_acc(A, D, 1, 0, 0);
    const emsar::AsymRowOut o = emsar::asym_row_out(A, 1, 0, X.gene ? X.gene + d.tid_off : nullptr);
    const uint32_t s = d.tid_off;
    O.var[s] = o.var; O.rowsum[s] = o.rowsum; O.gsum[s] = o.genesum; O.pcov[s] = o.pcov; O.partner[s] = o.partner;
    if (O.gsum_lib) O.gsum_lib[O.lib[s]] = o.genesum;
    if ((int32_t)di == O.block_desc) O.block[0] = A[0];
}

template <int G, int T>
__global__ __launch_bounds__(T) void k_asym_sets(emsar::AsymRecords X, const uint32_t *__restrict__ items, int64_t n_items,
                                                 const double *__restrict__ w, double tol, AsymOut O) {
#pragma clang fp contract(off)
    constexpr int PER = T / G;
    constexpr bool SMALL = PER > 1;                  // several components per workgroup: fixed trip counts, fixed LDS stride
    extern __shared__ double lds[];
    __shared__ int s_fail[PER];
    const int grp = threadIdx.x / G, l = threadIdx.x % G;
    const int64_t it = (int64_t)blockIdx.x * PER + grp;
    const bool live = it < n_items;
    const uint32_t di = live ? items[it] : 0u;
    emsar::AsymDesc d{};
    if (live) d = X.desc[di];
    const int n = (int)d.n;                          // 0 for a lane group without a component
    const int trips = SMALL ? G : n;
    const int tri_n = trips * (trips + 1) / 2;
    double *const A = lds + grp * (tri_n + 2 * trips), *const D = A + tri_n, *const diag = D + trips;

    if (l < n) { emsar::asym_build_row(X, d, l, w, A); diag[l] = A[emsar::asym_tri(l, l)]; }
    if (l == 0) s_fail[grp] = -1;
    __syncthreads();

    // the factorisation, column by column
    for (int j = 0; j < trips; j++) {
        const bool on = j < n && l >= j && l < n;
        double acc = 0.0;
        if (on) acc = emsar::asym_col_acc(A, D, l, j);
        if (on && l == j) {
            D[j] = acc;
            if (s_fail[grp] < 0 && !emsar::asym_pivot_ok(acc, diag[j], tol)) s_fail[grp] = j;
            diag[j] = acc / diag[j];
        }
        __syncthreads();
        const int failed = s_fail[grp];              // read between the barriers: the next column's owner writes it after the second
        if (on && l > j) A[emsar::asym_tri(l, j)] = acc / D[j];
        __syncthreads();
        if (!SMALL && failed >= 0) break;            // one component per workgroup: the same for every lane
    }
    const int fail = s_fail[grp];
    const bool ok = live && fail < 0;
    if (live && l == 0) { O.fail[di] = fail; O.ratio[di] = emsar::asym_min_ratio(diag, n, fail); }
    if (!SMALL && !ok) return;

    // M = L^-1 in place, row by row: all of row i is read before any of it is written
    for (int i = 1; i < trips; i++) {
        const bool on = ok && i < n && l < i;
        double m = 0.0;
        if (on) m = emsar::asym_inv_acc(A, i, l);
        __syncthreads();
        if (on) A[emsar::asym_tri(i, l)] = m;
        __syncthreads();
    }

    // Sigma in place from the top: rows [i0, i1) at a time, one lane per element of the packed triangle
    for (int i0 = 0; i0 < trips;) {
        int i1 = i0, cnt = 0;
        if (SMALL) { i1 = i0 + 1; cnt = i0 + 1; }
        else while (i1 < n && cnt + i1 + 1 <= G) { cnt += i1 + 1; i1++; }
        const bool on = ok && i0 < n && l < cnt;
        double v = 0.0;
        if (on) {
            int i = i0, j = l;
            while (j > i) { j -= i + 1; i++; }
            v = emsar::asym_cov_acc(A, D, n, i, j);
        }
        __syncthreads();
        if (on) A[emsar::asym_tri(i0, 0) + l] = v;
        __syncthreads();
        i0 = i1;
    }

    if (ok && l < n) {
        const emsar::AsymRowOut o = emsar::asym_row_out(A, n, l, X.gene ? X.gene + d.tid_off : nullptr);
        const uint32_t s = d.tid_off + (uint32_t)l;
        O.var[s] = o.var; O.rowsum[s] = o.rowsum; O.gsum[s] = o.genesum; O.pcov[s] = o.pcov; O.partner[s] = o.partner;
        if (O.gsum_lib) O.gsum_lib[O.lib[s]] = o.genesum;
    }
    if (ok && (int32_t)di == O.block_desc)
        for (int p = l; p < n * n; p += G) {
            const int i = p / n, j = p % n;
            O.block[p] = i >= j ? A[emsar::asym_tri(i, j)] : A[emsar::asym_tri(j, i)];
        }
}

}  // namespace
