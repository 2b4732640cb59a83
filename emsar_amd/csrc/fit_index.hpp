// fit_index.hpp -- what the host and the device side of the model fit (include/emsar_hip.h "model fit") share: the per-row terms, the
// walk of one chunk of a transcript's entries, the order of the three totals, and the builder of the transposed index that both walk.
// Pure C++ (no HIP call): the host restatement in fit.hpp is these functions in a loop, the kernels in kernels_fit.hpp are these
// functions with one lane per row / chunk, so both do the same operations in the same order.
//
// The transposed index.  The entries of transcript t, ordered by (caller row ascending, position in the row ascending), are cut into
// consecutive chunks of kFitChunk = 256; a transcript without entries gets one empty chunk, so that every transcript has an owner
// for its outputs.  Chunks are numbered in transcript order ("original chunk number": a transcript's chunks are consecutive), which
// is the order in which k_fit_tx_finish adds their partial sums.  One lane walks one chunk, so the row ids are NOT stored chunk after
// chunk -- lane i of a wave would then read 64 different cache lines in every step.  Instead the chunks are sorted by length,
// longest first (ties by chunk number), cut into groups of 64 (one wave), and slot j of the group's i-th chunk is stored at
//     group_base + 64 * j + i,        padded with -1 up to the group's longest chunk,
// so step j of a wave is one 256-byte load.  Because the lengths are sorted the padding telescopes: a group pads at most
// 63 * (its longest - its shortest) <= 63 * (its longest - the next group's longest) slots, in total at most 63 * 256
// (index_slots <= nnz + 64 * 255, checked by the builder).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define EMSAR_FIT_HD __host__ __device__
#else
#define EMSAR_FIT_HD
#endif

// hipcc contracts a * b + c into a fused multiply-add by default, on the host side too; the fit's sums round every operation on its own
#if defined(__clang__)
#define EMSAR_FIT_NO_FMA _Pragma("clang fp contract(off)")
#else
#define EMSAR_FIT_NO_FMA
#endif

namespace emsar {

constexpr int kFitChunk = 256;    // entries per chunk of a transcript (the order is part of the ABI, include/emsar_hip.h)
constexpr int kFitGroup = 64;     // chunks per group = lanes of a wave

// What stage 1 leaves per row for stage 2, one aligned 32-byte gather per entry: S is the row's sum when the row reaches its
// transcripts (inside, mu > 0), else 0 -- an entry of such a row has share 0 and adds nothing.  An infeasible row (mu == 0, R > 0)
// keeps q = d = +inf and a = R next to S = 0: that is how the totals tell it from a row that merely has nothing to add.
struct alignas(32) FitRec { double S, q, d, a; };

// The terms of one row that is not outside: mu = E * S and, by the cases of the header, q (Pearson), d (deviance, clamped at 0) and
// a (|R - mu|).  Returns the record's S.  Every operation rounded on its own (no fused multiply-add).
EMSAR_FIT_HD inline double fit_row_terms(double R, double E, double S, double *mu, double *q, double *d, double *a) {
EMSAR_FIT_NO_FMA
    const double m = E * S;
    *mu = m;
    if (m > 0.0) {
        const double diff = R - m;
        *q = diff * diff / m;
        *a = fabs(diff);
        const double l = R > 0.0 ? R * log(R / m) : 0.0;
        double dv = 2.0 * (l - diff);
        if (dv < 0.0) dv = 0.0;
        *d = dv;
        return S;
    }
    if (R > 0.0) { *q = INFINITY; *d = INFINITY; *a = R; }
    else { *q = 0.0; *d = 0.0; *a = 0.0; }
    return 0.0;
}
EMSAR_FIT_HD inline bool fit_rec_infeasible(const FitRec &r) { return r.S == 0.0 && r.q == INFINITY; }

// The five accumulators of a chunk (and of a transcript): four sums and the first largest p * a with its row.
struct FitAcc { double chi2, dev, miss, df, best; int32_t row; };

// One chunk: its slots base + 64 * j (j < steps) of the interleaved index, left to right; th = theta of the chunk's transcript.
// All terms are >= 0, so starting from 0.0 is starting from the first term.  Rows ascend along a chunk and a strict > keeps the
// first maximum: the smallest row among equal products.
EMSAR_FIT_HD inline FitAcc fit_walk_chunk(const int32_t *idx, int64_t base, int32_t steps, double th, const FitRec *rec) {
EMSAR_FIT_NO_FMA
    FitAcc A = {0.0, 0.0, 0.0, 0.0, 0.0, -1};
    for (int32_t j = 0; j < steps; j++) {
        const int32_t r = idx[base + (int64_t)kFitGroup * j];
        if (r < 0) break;                         // padding: the chunk has ended
        const FitRec x = rec[r];
        if (!(x.S > 0.0)) continue;
        const double p = th / x.S;
        const double tq = p * x.q, td = p * x.d, ta = p * x.a;
        A.chi2 = A.chi2 + tq;
        A.dev = A.dev + td;
        A.miss = A.miss + ta;
        A.df = A.df + p;
        if (ta > A.best) { A.best = ta; A.row = r; }
    }
    return A;
}

// The partials of a transcript of more than one chunk, in chunk order, starting from the first.
//   part [5][n_chunks] chi2, dev, miss, df, best; part_row [n_chunks]
EMSAR_FIT_HD inline FitAcc fit_finish(const double *part, const int32_t *part_row, int64_t n_chunks, int32_t c0, int32_t c1) {
    FitAcc A = {part[c0], part[n_chunks + c0], part[2 * n_chunks + c0], part[3 * n_chunks + c0], part[4 * n_chunks + c0], part_row[c0]};
    for (int32_t c = c0 + 1; c < c1; c++) {
        A.chi2 = A.chi2 + part[c];
        A.dev = A.dev + part[n_chunks + c];
        A.miss = A.miss + part[2 * n_chunks + c];
        A.df = A.df + part[3 * n_chunks + c];
        if (part[4 * n_chunks + c] > A.best) { A.best = part[4 * n_chunks + c]; A.row = part_row[c]; }
    }
    return A;
}

// The totals' order (k_fit_totals, one workgroup of 1024 lanes, the shape of k_sum): lane l adds the rows l, l + 1024, .. in row
// order; the 64 lanes of a wave are folded by the butterfly v[i] += v[i ^ o], o = 32, 16, .. 1; the 16 wave sums are added left to
// right.  Infeasible rows are counted, not added.  out = sum q, sum d, sum a, number of infeasible rows.
inline void fit_totals_host(const FitRec *rec, int64_t n_rows, double out[4]) {
    std::vector<double> lane(4 * 1024, 0.0);
    for (int64_t r = 0; r < n_rows; r++) {
        double *v = &lane[4 * (size_t)(r & 1023)];
        if (fit_rec_infeasible(rec[r])) v[3] += 1.0;
        else { v[0] += rec[r].q; v[1] += rec[r].d; v[2] += rec[r].a; }
    }
    for (int k = 0; k < 4; k++) {
        double tot = 0.0;
        for (int w = 0; w < 16; w++) {
            double v[64], u[64];
            for (int i = 0; i < 64; i++) v[i] = lane[4 * (size_t)(64 * w + i) + k];
            for (int o = 32; o > 0; o >>= 1) {
                for (int i = 0; i < 64; i++) u[i] = v[i] + v[i ^ o];
                for (int i = 0; i < 64; i++) v[i] = u[i];
            }
            tot += v[0];
        }
        out[k] = tot;
    }
}

// ---- the transposed index -------------------------------------------------------------------------------------------------------
struct FitIndex {
    int64_t n_chunks = 0, n_groups = 0, n_multi = 0;
    std::vector<int32_t> idx;           // [index_slots] caller row ids, interleaved by group, -1 = padding
    std::vector<int64_t> group_base;    // [n_groups] first slot of the group
    std::vector<int32_t> group_steps;   // [n_groups] length of the group's longest chunk
    // per chunk in SORTED order (lane order): the transcript whose theta it needs, and where its result goes:
    // >= 0 the transcript (it has this one chunk), else -1 - (original chunk number) = the partial's slot
    std::vector<int32_t> chunk_tid, chunk_out;
    std::vector<int32_t> multi;         // [n_multi][3] transcript, first original chunk, end
    int64_t index_slots() const { return (int64_t)idx.size(); }
    int64_t index_bytes() const {
        return 4 * (int64_t)(idx.size() + group_steps.size() + chunk_tid.size() + chunk_out.size() + multi.size()) + 8 * (int64_t)group_base.size();
    }
};

// 0 ok; -1 the index does not fit (more than INT32_MAX chunks); -2 the padding bound is broken (a bug).  Throws std::bad_alloc.
// The CSR has been validated (layout.hpp) and n_rows <= INT32_MAX.
inline int build_fit_index(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col, FitIndex &X) {
    const int64_t nnz = n_rows > 0 ? (int64_t)row_ptr[n_rows] : 0;
    const size_t T = (size_t)n_tx;
    // counting sort of the entries by transcript: CSR order is (row, position) ascending already
    std::vector<int64_t> tp(T + 1, 0);
    for (int64_t k = 0; k < nnz; k++) tp[(size_t)col[k] + 1]++;
    int64_t n_chunks = 0;
    for (size_t t = 0; t < T; t++) {
        const int64_t len = tp[t + 1];
        n_chunks += len == 0 ? 1 : (len + kFitChunk - 1) / kFitChunk;
        tp[t + 1] += tp[t];
    }
    if (n_chunks > (int64_t)INT32_MAX - kFitGroup) return -1;
    std::vector<int32_t> rows((size_t)nnz);
    {
        std::vector<int64_t> fill(tp.begin(), tp.end() - 1);
        for (int64_t r = 0; r < n_rows; r++)
            for (uint64_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) rows[(size_t)fill[(size_t)col[k]]++] = (int32_t)r;
    }
    // the chunks in original order: transcript, begin in rows[], length; then sorted by length descending (stable: ties by number)
    std::vector<int32_t> c_tid((size_t)n_chunks), c_len((size_t)n_chunks);
    std::vector<int64_t> c_beg((size_t)n_chunks);
    X = FitIndex();
    X.n_chunks = n_chunks;
    {
        int64_t c = 0;
        for (size_t t = 0; t < T; t++) {
            const int64_t b = tp[t], e = tp[t + 1];
            const int64_t first = c;
            int64_t at = b;
            do {
                const int64_t len = std::min<int64_t>(kFitChunk, e - at);
                c_tid[(size_t)c] = (int32_t)t; c_beg[(size_t)c] = at; c_len[(size_t)c] = (int32_t)len;
                c++; at += len;
            } while (at < e);
            if (c - first > 1) { X.multi.push_back((int32_t)t); X.multi.push_back((int32_t)first); X.multi.push_back((int32_t)c); }
        }
        X.n_multi = (int64_t)X.multi.size() / 3;
    }
    std::vector<int32_t> order((size_t)n_chunks);
    {
        int64_t start[kFitChunk + 2] = {0};
        for (int64_t c = 0; c < n_chunks; c++) start[kFitChunk - c_len[(size_t)c] + 1]++;       // bucket 0 = the longest
        for (int b = 0; b <= kFitChunk; b++) start[b + 1] += start[b];
        for (int64_t c = 0; c < n_chunks; c++) order[(size_t)start[kFitChunk - c_len[(size_t)c]]++] = (int32_t)c;
    }
    // groups of 64 sorted chunks, interleaved
    X.n_groups = (n_chunks + kFitGroup - 1) / kFitGroup;
    X.group_base.resize((size_t)X.n_groups); X.group_steps.resize((size_t)X.n_groups);
    X.chunk_tid.resize((size_t)n_chunks); X.chunk_out.resize((size_t)n_chunks);
    int64_t slots = 0;
    for (int64_t g = 0; g < X.n_groups; g++) {
        const int32_t longest = c_len[(size_t)order[(size_t)(g * kFitGroup)]];
        X.group_base[(size_t)g] = slots; X.group_steps[(size_t)g] = longest;
        slots += (int64_t)kFitGroup * longest;
    }
    if (slots > nnz + (int64_t)kFitGroup * (kFitChunk - 1)) return -2;
    X.idx.assign((size_t)slots, -1);
    for (int64_t s = 0; s < n_chunks; s++) {
        const int32_t c = order[(size_t)s];
        const int32_t t = c_tid[(size_t)c];
        X.chunk_tid[(size_t)s] = t;
        const bool alone = tp[(size_t)t + 1] - tp[(size_t)t] <= kFitChunk;
        X.chunk_out[(size_t)s] = alone ? t : -1 - c;
        const int64_t base = X.group_base[(size_t)(s / kFitGroup)] + s % kFitGroup;
        const int32_t *src = rows.data() + c_beg[(size_t)c];
        for (int32_t j = 0; j < c_len[(size_t)c]; j++) X.idx[(size_t)(base + (int64_t)kFitGroup * j)] = src[j];
    }
    return 0;
}

}  // namespace emsar
