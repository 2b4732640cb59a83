// asym_plan.hpp -- what the host and the device side of the asymptotic standard errors (include/emsar_hip.h "asymptotic standard
// errors") share: the active set, the connected components of the active transcripts and their packed records, every arithmetic step
// of the definition, and the host finish.  Pure C++ (no HIP call): the host function in asym.hpp is these functions in loops, the
// kernels in kernels_asym.hpp are these functions with one lane per row of J / column element / row element, so both do the same
// operations in the same order and return the same bits.
//
// The records of one component of n <= kAsymMaxN active transcripts (AsymDesc; all offsets index the plan's pools):
//     g_tid [tid_off .. + n)          caller tids, ascending: local index i = position here ("slot" = tid_off + i)
//     crow  [row_off .. + nrows)      the caller rows with w_c != 0 that hold one of them, ascending
//     rp    [rp_off .. + nrows + 1)   per such row its run in ids
//     ids                             the row's ACTIVE entries as 8-bit local ids, in position order
//     tp    [tp_off .. + n + 1)       per local transcript its run in tent
//     tent                            the transcript's entries in (row ascending, position ascending) order, as indices into crow
// A transcript that stands twice in a row has two entries in tent, and each of them walks the whole row in ids.
// The matrix lives in a packed lower triangle A[i (i + 1) / 2 + j] next to D[n] and diag[n]: first J, then L below the diagonal (D
// apart), then M = L^-1 in place, then Sigma in place, row by row.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define EMSAR_ASYM_HD __host__ __device__
#else
#define EMSAR_ASYM_HD
#endif
// hipcc contracts a * b + c into a fused multiply-add by default, on the host side too; every operation here is rounded on its own
#if defined(__clang__)
#define EMSAR_ASYM_NO_FMA _Pragma("clang fp contract(off)")
#else
#define EMSAR_ASYM_NO_FMA
#endif

namespace emsar {

constexpr int kAsymMaxN = 192;                               // EMSAR_ASYM_MAX_N
constexpr int kAsymClasses = 4;                              // one lane (n == 1), 8 lanes, one wave, 256 threads
constexpr int kAsymClassN[kAsymClasses] = {1, 8, 64, 192};
constexpr int kAsymChunk = 256;                              // the chunked sums of the finish: gene_sums' chunk
enum : int32_t { ASYM_ESTIMATED = 0, ASYM_BOUNDARY = 1, ASYM_UNIDENTIFIABLE = 2, ASYM_TOO_LARGE = 3, ASYM_INFEASIBLE = 4 };

struct AsymDesc { uint32_t n, tid_off, nrows, row_off, rp_off, tp_off; };

// the pools of the records as plain pointers: what the kernels get, and what the host evaluation reads
struct AsymRecords {
    const AsymDesc *desc;
    const int32_t *crow, *gene;          // gene [slots]: the gene of every slot, -1 = none
    const uint32_t *rp, *tp, *tent;
    const uint8_t *ids;
};

// ---- the arithmetic, step by step ---------------------------------------------------------------------------------------------------

EMSAR_ASYM_HD inline int asym_tri(int i, int j) { return i * (i + 1) / 2 + j; }
EMSAR_ASYM_HD inline bool asym_finite(double x) { return x - x == 0.0; }

EMSAR_ASYM_HD inline double asym_row_w(double R, double S) {
EMSAR_ASYM_NO_FMA
    return (R > 0.0 && S > 0.0) ? R / (S * S) : 0.0;
}

// row i of J (columns 0 .. i) into A, from the transcript's own entries; w [n_rows] by caller row
EMSAR_ASYM_HD inline void asym_build_row(const AsymRecords &X, const AsymDesc &d, int i, const double *w, double *A) {
EMSAR_ASYM_NO_FMA
    double *a = A + asym_tri(i, 0);
    for (int j = 0; j <= i; j++) a[j] = 0.0;
    const uint32_t *tp = X.tp + d.tp_off, *rp = X.rp + d.rp_off;
    for (uint32_t e = tp[i]; e < tp[i + 1]; e++) {
        const uint32_t r = X.tent[e];
        const double wc = w[X.crow[d.row_off + r]];
        for (uint32_t q = rp[r]; q < rp[r + 1]; q++) {
            const int j = X.ids[q];
            if (j <= i) a[j] = a[j] + wc;
        }
    }
}

// the element (i, j), i >= j, of column j of the factorisation before its division: D_j for i == j
EMSAR_ASYM_HD inline double asym_col_acc(const double *A, const double *D, int i, int j) {
EMSAR_ASYM_NO_FMA
    const double *ri = A + asym_tri(i, 0), *rj = A + asym_tri(j, 0);
    double acc = ri[j];
    for (int k = 0; k < j; k++) acc = acc - (ri[k] * D[k]) * rj[k];
    return acc;
}
EMSAR_ASYM_HD inline bool asym_pivot_ok(double d, double jjj, double tol) {
EMSAR_ASYM_NO_FMA
    return asym_finite(d) && d > tol * jjj;
}

// M_ij, j < i: rows < i of A hold M already, row i still L
EMSAR_ASYM_HD inline double asym_inv_acc(const double *A, int i, int j) {
EMSAR_ASYM_NO_FMA
    const double *ri = A + asym_tri(i, 0);
    double acc = ri[j];
    for (int k = j + 1; k < i; k++) acc = acc + ri[k] * A[asym_tri(k, j)];
    return -acc;
}

// Sigma_ij, i >= j, from M (rows >= i of A) and D
EMSAR_ASYM_HD inline double asym_cov_acc(const double *A, const double *D, int n, int i, int j) {
EMSAR_ASYM_NO_FMA
    const double mii = 1.0, mij = i == j ? 1.0 : A[asym_tri(i, j)];
    double acc = (mii * mij) / D[i];
    for (int k = i + 1; k < n; k++) acc = acc + (A[asym_tri(k, i)] * A[asym_tri(k, j)]) / D[k];
    return acc;
}

// what one transcript reads off its row of Sigma (A holds Sigma's lower triangle); gene [n] local, or null
struct AsymRowOut { double var, rowsum, genesum, pcov; int32_t partner; };
EMSAR_ASYM_HD inline AsymRowOut asym_row_out(const double *A, int n, int i, const int32_t *gene) {
EMSAR_ASYM_NO_FMA
    auto sig = [&](int a, int b) { return a >= b ? A[asym_tri(a, b)] : A[asym_tri(b, a)]; };
    AsymRowOut o;
    o.var = sig(i, i);
    o.rowsum = sig(i, 0);
    for (int j = 1; j < n; j++) o.rowsum = o.rowsum + sig(i, j);
    o.genesum = 0.0;
    const int32_t gi = gene ? gene[i] : -1;
    if (gi >= 0) {
        bool first = true;
        for (int j = 0; j < n; j++)
            if (gene[j] == gi) { o.genesum = first ? sig(i, j) : o.genesum + sig(i, j); first = false; }
    }
    o.partner = -1;
    o.pcov = NAN;
    double best = 0.0;
    for (int j = 0; j < n; j++) {
        if (j == i) continue;
        const double s = sig(i, j), v = s * (s < 0.0 ? -s : s) / sig(j, j);
        if (o.partner < 0 || v < best) { o.partner = j; o.pcov = s; best = v; }
    }
    return o;
}

// the smallest D_j / J_jj (ratio [n], left by the factorisation) up to the first failing pivot, that one included
EMSAR_ASYM_HD inline double asym_min_ratio(const double *ratio, int n, int fail) {
    double m = INFINITY;
    const int last = fail >= 0 ? fail : n - 1;
    for (int j = 0; j <= last; j++) if (ratio[j] < m) m = ratio[j];
    return m;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------------

struct AsymPlan {
    std::vector<int32_t> status;         // [n_tx] BOUNDARY / TOO_LARGE / INFEASIBLE, and ESTIMATED for whatever is factorised
    std::vector<int32_t> comp_of, loc;   // [n_tx] descriptor or -1; local index
    std::vector<AsymDesc> desc;          // the components that are factorised, ordered by their smallest tid
    std::vector<int32_t> g_tid, crow;
    std::vector<uint32_t> rp, tp, tent;
    std::vector<uint8_t> ids;
    int64_t components = 0, too_large = 0, infeasible = 0, rows_infeasible = 0;
    int32_t max_n = 0;
    size_t slots() const { return g_tid.size(); }
};

// wgt [n_rows]: R_c (0 for a row outside).  0 = fine, -2 = the records would not fit 32-bit offsets
inline int asym_build_plan(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col, const int32_t *wgt, const double *theta,
                           double cut, AsymPlan &P) {
EMSAR_ASYM_NO_FMA
    const size_t T = (size_t)n_tx;
    std::vector<uint8_t> active(T), link((size_t)n_rows, 0);
    std::vector<int32_t> par(T), seeds;
    for (size_t t = 0; t < T; t++) { active[t] = theta[t] > cut; par[t] = (int32_t)t; }
    auto find = [&](int32_t x) { while (par[(size_t)x] != x) { par[(size_t)x] = par[(size_t)par[(size_t)x]]; x = par[(size_t)x]; } return x; };
    for (int64_t c = 0; c < n_rows; c++) {
        const uint64_t b = row_ptr[c], e = row_ptr[c + 1];
        if (b == e) continue;
        double S = 0.0;
        for (uint64_t k = b; k < e; k++) S = S + theta[col[k]];
        const double R = (double)wgt[c];
        const bool infeasible = R > 0.0 && S == 0.0;
        P.rows_infeasible += infeasible;
        if (!(asym_row_w(R, S) != 0.0) && !infeasible) continue;
        int32_t first = -1;
        for (uint64_t k = b; k < e; k++) {
            const int32_t t = col[k];
            if (!active[(size_t)t]) continue;
            if (first < 0) first = find(t);
            else { const int32_t r = find(t); if (r != first) { par[(size_t)std::max(r, first)] = std::min(r, first); first = std::min(r, first); } }
        }
        if (first < 0) continue;
        if (infeasible) seeds.push_back(first); else link[(size_t)c] = 1;
    }
    // components by their smallest tid (the root of a set is its smallest member), locals by ascending tid
    std::vector<int32_t> cid(T, -1), csize;
    P.loc.assign(T, -1);
    for (size_t t = 0; t < T; t++)
        if (active[t]) {
            const int32_t r = find((int32_t)t);
            if (cid[(size_t)r] < 0) { cid[(size_t)r] = (int32_t)csize.size(); csize.push_back(0); }
            cid[t] = cid[(size_t)r];
            P.loc[t] = csize[(size_t)cid[t]]++;
        }
    const size_t nc = csize.size();
    std::vector<int32_t> state(nc, ASYM_ESTIMATED), dix(nc, -1);
    for (int32_t s : seeds) state[(size_t)cid[(size_t)find(s)]] = ASYM_INFEASIBLE;
    P.components = (int64_t)nc;
    for (size_t k = 0; k < nc; k++) {
        P.max_n = std::max(P.max_n, csize[k]);
        if (csize[k] > kAsymMaxN) state[k] = ASYM_TOO_LARGE;         // a giant component is not packed at all
        if (state[k] == ASYM_TOO_LARGE) P.too_large++;
        else if (state[k] == ASYM_INFEASIBLE) P.infeasible++;
        else {
            dix[k] = (int32_t)P.desc.size();
            AsymDesc d{};
            d.n = (uint32_t)csize[k];
            P.desc.push_back(d);
        }
    }
    P.status.assign(T, ASYM_BOUNDARY);
    P.comp_of.assign(T, -1);
    const size_t nd = P.desc.size();
    size_t slots = 0;
    for (size_t i = 0; i < nd; i++) { P.desc[i].tid_off = (uint32_t)slots; P.desc[i].tp_off = (uint32_t)(slots + i); slots += P.desc[i].n; }
    P.g_tid.resize(slots);
    for (size_t t = 0; t < T; t++)
        if (active[t]) {
            P.status[t] = state[(size_t)cid[t]];
            P.comp_of[t] = dix[(size_t)cid[t]];
            if (P.comp_of[t] >= 0) P.g_tid[P.desc[(size_t)P.comp_of[t]].tid_off + (size_t)P.loc[t]] = (int32_t)t;
        }
    // count, then fill: the rows of every component, their active entries, every transcript's entries
    std::vector<uint64_t> n_ids(nd, 0), n_ent(slots + 1, 0);
    auto comp_of_row = [&](int64_t c) {
        for (uint64_t k = row_ptr[c]; k < row_ptr[c + 1]; k++) if (active[(size_t)col[k]]) return P.comp_of[(size_t)col[k]];
        return (int32_t)-1;
    };
    for (int64_t c = 0; c < n_rows; c++) {
        if (!link[(size_t)c]) continue;
        const int32_t d = comp_of_row(c);
        if (d < 0) { link[(size_t)c] = 0; continue; }
        P.desc[(size_t)d].nrows++;
        for (uint64_t k = row_ptr[c]; k < row_ptr[c + 1]; k++)
            if (active[(size_t)col[k]]) { n_ids[(size_t)d]++; n_ent[P.desc[(size_t)d].tid_off + (size_t)P.loc[(size_t)col[k]]]++; }
    }
    uint64_t rows = 0, ids = 0, ent = 0;
    std::vector<uint64_t> id_cur(nd), row_cur(nd, 0);
    for (size_t i = 0; i < nd; i++) {
        P.desc[i].row_off = (uint32_t)rows; P.desc[i].rp_off = (uint32_t)(rows + i);
        rows += P.desc[i].nrows;
        id_cur[i] = ids; ids += n_ids[i];
    }
    for (size_t s = 0; s < slots; s++) ent += n_ent[s];
    if (rows + nd > UINT32_MAX || ids > UINT32_MAX || ent > UINT32_MAX) return -2;
    P.crow.resize((size_t)rows); P.rp.resize((size_t)rows + nd); P.ids.resize((size_t)ids);
    P.tp.resize(slots + nd); P.tent.resize((size_t)ent);
    std::vector<uint64_t> ent_cur(slots);
    ent = 0;
    for (size_t i = 0; i < nd; i++) {
        const AsymDesc &d = P.desc[i];
        for (uint32_t l = 0; l < d.n; l++) { const size_t s = d.tid_off + l; P.tp[d.tp_off + l] = (uint32_t)ent; ent_cur[s] = ent; ent += n_ent[s]; }
        P.tp[d.tp_off + d.n] = (uint32_t)ent;
        P.rp[d.rp_off + d.nrows] = (uint32_t)(id_cur[i] + n_ids[i]);
    }
    for (int64_t c = 0; c < n_rows; c++) {
        if (!link[(size_t)c]) continue;
        const size_t i = (size_t)comp_of_row(c);
        const AsymDesc &d = P.desc[i];
        const uint64_t r = row_cur[i]++;
        P.crow[d.row_off + (size_t)r] = (int32_t)c;
        P.rp[d.rp_off + (size_t)r] = (uint32_t)id_cur[i];
        for (uint64_t k = row_ptr[c]; k < row_ptr[c + 1]; k++)
            if (active[(size_t)col[k]]) {
                const int32_t l = P.loc[(size_t)col[k]];
                P.ids[(size_t)id_cur[i]++] = (uint8_t)l;
                P.tent[(size_t)ent_cur[d.tid_off + (size_t)l]++] = (uint32_t)r;
            }
    }
    return 0;
}

// every index of the records against its component and its pool, before anything walks them.  0 = fine
inline int asym_check_plan(const AsymPlan &P, int64_t n_rows, int32_t n_tx) {
    for (size_t i = 0; i < P.desc.size(); i++) {
        const AsymDesc &d = P.desc[i];
        if (d.n < 1 || d.n > (uint32_t)kAsymMaxN) return 1;
        if ((size_t)d.tid_off + d.n > P.g_tid.size() || (size_t)d.row_off + d.nrows > P.crow.size()) return 2;
        if ((size_t)d.rp_off + d.nrows + 1 > P.rp.size() || (size_t)d.tp_off + d.n + 1 > P.tp.size()) return 3;
        for (uint32_t l = 0; l < d.n; l++) {
            const int32_t t = P.g_tid[d.tid_off + l];
            if (t < 0 || t >= n_tx || (l > 0 && t <= P.g_tid[d.tid_off + l - 1])) return 4;
            const uint32_t b = P.tp[d.tp_off + l], e = P.tp[d.tp_off + l + 1];
            if (b > e || e > P.tent.size()) return 5;
            for (uint32_t k = b; k < e; k++) if (P.tent[k] >= d.nrows || (k > b && P.tent[k] < P.tent[k - 1])) return 6;
        }
        for (uint32_t r = 0; r < d.nrows; r++) {
            const int32_t c = P.crow[d.row_off + r];
            if (c < 0 || c >= n_rows || (r > 0 && c <= P.crow[d.row_off + r - 1])) return 7;
            const uint32_t b = P.rp[d.rp_off + r], e = P.rp[d.rp_off + r + 1];
            if (b >= e || e > P.ids.size()) return 8;
            for (uint32_t k = b; k < e; k++) if (P.ids[k] >= d.n) return 9;
        }
    }
    return 0;
}

inline int asym_class_of(int n) { int c = 0; while (n > kAsymClassN[c]) c++; return c; }

// One component on the host: the steps above in the order of the definition.  A / D / diag are scratch; the slot outputs are written
// at tid_off + i when the component is factorised; returns the first failing pivot or -1, *min_ratio as asym_min_ratio.
inline int asym_eval_component(const AsymRecords &X, const AsymDesc &d, const double *w, double tol, std::vector<double> &A, std::vector<double> &D,
                               std::vector<double> &diag, double *s_var, double *s_rowsum, double *s_gsum, double *s_pcov, int32_t *s_partner,
                               double *min_ratio) {
EMSAR_ASYM_NO_FMA
    const int n = (int)d.n;
    A.resize((size_t)asym_tri(n, 0)); D.resize((size_t)n); diag.resize((size_t)n);
    for (int i = 0; i < n; i++) { asym_build_row(X, d, i, w, A.data()); diag[(size_t)i] = A[(size_t)asym_tri(i, i)]; }
    int fail = -1;
    for (int j = 0; j < n && fail < 0; j++) {
        const double dj = asym_col_acc(A.data(), D.data(), j, j);
        D[(size_t)j] = dj;
        if (!asym_pivot_ok(dj, diag[(size_t)j], tol)) fail = j;
        diag[(size_t)j] = dj / diag[(size_t)j];
        for (int i = j + 1; i < n; i++) A[(size_t)asym_tri(i, j)] = asym_col_acc(A.data(), D.data(), i, j) / dj;
    }
    *min_ratio = asym_min_ratio(diag.data(), n, fail);
    if (fail >= 0) return fail;
    for (int i = 1; i < n; i++) {
        double row[kAsymMaxN];
        for (int j = 0; j < i; j++) row[j] = asym_inv_acc(A.data(), i, j);
        for (int j = 0; j < i; j++) A[(size_t)asym_tri(i, j)] = row[j];
    }
    for (int i = 0; i < n; i++) {
        double row[kAsymMaxN];
        for (int j = 0; j <= i; j++) row[j] = asym_cov_acc(A.data(), D.data(), n, i, j);
        for (int j = 0; j <= i; j++) A[(size_t)asym_tri(i, j)] = row[j];
    }
    for (int i = 0; i < n; i++) {
        const AsymRowOut o = asym_row_out(A.data(), n, i, X.gene ? X.gene + d.tid_off : nullptr);
        const size_t s = d.tid_off + (size_t)i;
        s_var[s] = o.var; s_rowsum[s] = o.rowsum; s_gsum[s] = o.genesum; s_pcov[s] = o.pcov; s_partner[s] = o.partner;
    }
    return -1;
}

// ---- from the slots to the caller's transcripts, and the host finish --------------------------------------------------------------------

// per transcript in caller order, whatever its status
struct AsymTx {
    std::vector<double> var, rowsum, genesum, pcov;
    std::vector<int32_t> status, partner, blocker;
};

// c_fail [descriptors]: the first failing pivot or -1
inline void asym_assemble(const AsymPlan &P, int32_t n_tx, const double *s_var, const double *s_rowsum, const double *s_gsum, const double *s_pcov,
                          const int32_t *s_partner, const int32_t *c_fail, AsymTx &R) {
    const size_t T = (size_t)n_tx;
    R.var.assign(T, 0.0); R.rowsum.assign(T, 0.0); R.genesum.assign(T, 0.0); R.pcov.assign(T, NAN);
    R.status = P.status; R.partner.assign(T, -1); R.blocker.assign(T, -1);
    for (size_t t = 0; t < T; t++) {
        if (R.status[t] == ASYM_TOO_LARGE || R.status[t] == ASYM_INFEASIBLE) R.var[t] = R.rowsum[t] = NAN;
        const int32_t c = P.comp_of[t];
        if (c < 0) continue;
        const AsymDesc &d = P.desc[(size_t)c];
        if (c_fail[c] >= 0) {
            R.status[t] = ASYM_UNIDENTIFIABLE;
            R.var[t] = R.rowsum[t] = INFINITY;
            R.blocker[t] = P.g_tid[d.tid_off + (size_t)c_fail[c]];
            continue;
        }
        const size_t s = d.tid_off + (size_t)P.loc[t];
        R.var[t] = s_var[s]; R.rowsum[t] = s_rowsum[s]; R.genesum[t] = s_gsum[s]; R.pcov[t] = s_pcov[s];
        R.partner[t] = s_partner[s] < 0 ? -1 : P.g_tid[d.tid_off + (size_t)s_partner[s]];
    }
}

// gene_sums' rule over x[0 .. n): chunks of kAsymChunk left to right from their first term, then the chunk sums left to right
template <class F> inline double asym_chunked_sum(int64_t n, const F &x) {
EMSAR_ASYM_NO_FMA
    double sum = 0.0;
    for (int64_t b = 0; b < n; b += kAsymChunk) {
        const int64_t e = std::min<int64_t>(b + kAsymChunk, n);
        double s = x(b);
        for (int64_t i = b + 1; i < e; i++) s += x(i);
        sum = b == 0 ? s : sum + s;
    }
    return sum;
}

// the genes' transcripts by ascending tid
struct AsymGenes {
    std::vector<int64_t> gp;
    std::vector<int32_t> gtx;
    void build(int32_t n_tx, int32_t n_genes, const int32_t *gene_of_tx) {
        gp.assign((size_t)n_genes + 1, 0);
        for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] >= 0) gp[(size_t)gene_of_tx[t] + 1]++;
        for (int32_t g = 0; g < n_genes; g++) gp[(size_t)g + 1] += gp[(size_t)g];
        gtx.resize((size_t)gp[(size_t)n_genes]);
        std::vector<int64_t> fill(gp.begin(), gp.end() - 1);
        for (int32_t t = 0; t < n_tx; t++) if (gene_of_tx[t] >= 0) gtx[(size_t)fill[(size_t)gene_of_tx[t]]++] = t;
    }
    double sum(int32_t g, const double *x) const {
        const int64_t b = gp[(size_t)g];
        return asym_chunked_sum(gp[(size_t)g + 1] - b, [&](int64_t i) { return x[gtx[(size_t)(b + i)]]; });
    }
};

inline double asym_max0(double x) { return x > 0.0 ? x : 0.0; }
// sqrt with one NaN for everything that has no root (the hardware's NaN of a negative argument carries a sign)
inline double asym_sqrt(double x) { return x >= 0.0 ? sqrt(x) : (double)NAN; }

// The finish of the header.  VG [n_genes] = the gene sums of genesum (null without a gene map); any output may be null.
inline void asym_finish(int32_t n_tx, const double *theta, const AsymTx &R, int32_t n_genes, const int32_t *gene_of_tx, const AsymGenes *genes,
                        const double *VG, double *sd_fpkm, double *sd_tpm, double *usage_sd, double *gene_sd, int32_t *gene_status,
                        double *unestimated_share) {
EMSAR_ASYM_NO_FMA
    const double S = asym_chunked_sum(n_tx, [&](int64_t t) { return theta[t]; });
    const double VS = asym_chunked_sum(n_tx, [&](int64_t t) { return R.status[(size_t)t] == ASYM_ESTIMATED ? R.rowsum[(size_t)t] : 0.0; });
    const double lost = asym_chunked_sum(n_tx, [&](int64_t t) {
        return R.status[(size_t)t] != ASYM_ESTIMATED && R.status[(size_t)t] != ASYM_BOUNDARY ? theta[t] : 0.0; });
    *unestimated_share = S == 0.0 ? 0.0 : lost / S;
    std::vector<int32_t> gst;
    if (gene_of_tx) {
        // a gene's status by the rank TOO_LARGE > INFEASIBLE > UNIDENTIFIABLE > ESTIMATED > BOUNDARY
        static const int rank_of[5] = {1, 0, 2, 4, 3};
        static const int32_t status_of[5] = {ASYM_BOUNDARY, ASYM_ESTIMATED, ASYM_UNIDENTIFIABLE, ASYM_INFEASIBLE, ASYM_TOO_LARGE};
        std::vector<int> rank((size_t)n_genes, 0);
        for (int32_t t = 0; t < n_tx; t++)
            if (gene_of_tx[t] >= 0) rank[(size_t)gene_of_tx[t]] = std::max(rank[(size_t)gene_of_tx[t]], rank_of[R.status[(size_t)t]]);
        gst.resize((size_t)n_genes);
        for (int32_t g = 0; g < n_genes; g++) gst[(size_t)g] = status_of[rank[(size_t)g]];
    }
    auto by_status = [](int32_t st, double v) { return st == ASYM_UNIDENTIFIABLE ? (double)INFINITY : (st == ASYM_TOO_LARGE || st == ASYM_INFEASIBLE) ? (double)NAN : v; };
    for (int32_t t = 0; t < n_tx; t++) {
        const size_t i = (size_t)t;
        if (sd_fpkm) sd_fpkm[t] = asym_sqrt(R.var[i]);
        if (sd_tpm) {
            if (S == 0.0) sd_tpm[t] = 0.0;
            else if (R.status[i] != ASYM_ESTIMATED && R.status[i] != ASYM_BOUNDARY) sd_tpm[t] = by_status(R.status[i], 0.0);
            else {
                const double a = theta[t] / S;
                const double var_tpm = ((1e6 / S) * (1e6 / S)) * asym_max0(R.var[i] - 2 * a * R.rowsum[i] + a * a * VS);
                sd_tpm[t] = asym_sqrt(var_tpm);
            }
        }
    }
    if (!gene_of_tx) return;
    for (int32_t g = 0; g < n_genes; g++) {
        if (gene_sd) gene_sd[g] = by_status(gst[(size_t)g], asym_sqrt(VG[g]));
        if (gene_status) gene_status[g] = gst[(size_t)g];
    }
    if (usage_sd) {
        std::vector<double> G((size_t)n_genes);
        for (int32_t g = 0; g < n_genes; g++) G[(size_t)g] = genes->sum(g, theta);
        for (int32_t t = 0; t < n_tx; t++) {
            const int32_t g = gene_of_tx[t];
            if (g < 0) { usage_sd[t] = NAN; continue; }
            const double Gg = G[(size_t)g];
            if (Gg == 0.0) { usage_sd[t] = 0.0; continue; }
            const double u = theta[t] / Gg;
            const size_t i = (size_t)t;
            usage_sd[t] = by_status(gst[(size_t)g], 0.0);
            if (gst[(size_t)g] == ASYM_ESTIMATED || gst[(size_t)g] == ASYM_BOUNDARY)
                usage_sd[t] = asym_sqrt(asym_max0(R.var[i] - 2 * u * R.genesum[i] + u * u * VG[g])) / Gg;
        }
    }
}

}  // namespace emsar
