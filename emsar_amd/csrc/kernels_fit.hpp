// kernels_fit.hpp -- model fit (emsar_hip_model_fit): per-row residuals of a theta against the sample, and their attribution to the
// transcripts of every row.  FP64, plain stores, no atomics, no LDS in the two sweeps: the order of every sum is fixed by the index.
//
// Definitions: include/emsar_hip.h "model fit".  The arithmetic is fit_index.hpp's (fit_row_terms, fit_walk_chunk, fit_finish), the
// functions the host restatement calls too; the kernels only hand out rows and chunks to lanes.
//   stage 1  k_fit_rows        one lane per caller row of the caller-order CSR: S_c, then the 32-byte record {S, q, d, a} of the row
//                              (fit_index.hpp FitRec) and the optional row outputs.  Reads the CSR once (8 B per row, 4 B per entry)
//                              and gathers theta (8 B per entry); writes 32 B per row.
//   stage 2  k_fit_tx          one lane per chunk of <= 256 entries of one transcript, over the interleaved transposed index: step j of
//                              a wave is one 256-byte load of row ids, then one aligned 32-byte record gather per lane.
//            k_fit_tx_finish   one lane per transcript of more than one chunk: its chunks' partials in chunk order.
//            (k_gene_sums / k_gene_finish on the [4][n_tx] block give the gene outputs.)
//   totals   k_fit_totals      one workgroup, fixed order, the shape of k_sum: sum q, sum d, sum a and the infeasible rows' count.
#pragma once
// included by emsar_hip.hip only (one translation unit: the kernels live in its anonymous namespace)

namespace {

// rows: row_ptr [n_rows + 1], col [nnz] caller tids, wgt [n_rows] R_c, row_E [n_rows] or null (= 1.0), theta [n_tx] caller order
// rec [n_rows]; mu / chi2 / dev [n_rows] or null
__global__ __launch_bounds__(256) void k_fit_rows(int64_t n_rows, const uint64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                  const int32_t *__restrict__ wgt, const double *__restrict__ row_E,
                                                  const double *__restrict__ theta, emsar::FitRec *__restrict__ rec,
                                                  double *__restrict__ mu_out, double *__restrict__ chi2_out, double *__restrict__ dev_out) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_rows) return;
    const uint64_t b = row_ptr[c], e = row_ptr[c + 1];
    const double E = row_E ? row_E[c] : 1.0;
    emsar::FitRec x = {0.0, 0.0, 0.0, 0.0};
    double mu = 0.0;
    if (b < e && E != 0.0) {
        double S = 0.0;
        for (uint64_t k = b; k < e; k++) S = S + theta[col[k]];
        x.S = emsar::fit_row_terms((double)wgt[c], E, S, &mu, &x.q, &x.d, &x.a);
    }
    rec[c] = x;
    if (mu_out) mu_out[c] = mu;
    if (chi2_out) chi2_out[c] = x.q;
    if (dev_out) dev_out[c] = x.d;
}

// One lane per chunk in the index' sorted order: lane i of wave g owns chunk 64 g + i.
//   idx, group_base [n_groups], group_steps [n_groups], chunk_tid / chunk_out [n_chunks] (emsar::FitIndex; chunk_out >= 0 holds the
//   LIBRARY's index of the transcript: the [4][n_tx] block feeds k_gene_sums), theta [n_tx] caller order, rec [n_rows]
//   tx [4][n_tx] chi2, dev, miss, df and worst [n_tx] in library order; part [5][n_chunks], part_row [n_chunks] by original chunk number
__global__ __launch_bounds__(256) void k_fit_tx(int64_t n_chunks, const int32_t *__restrict__ idx, const int64_t *__restrict__ group_base,
                                                const int32_t *__restrict__ group_steps, const int32_t *__restrict__ chunk_tid,
                                                const int32_t *__restrict__ chunk_out, const double *__restrict__ theta,
                                                const emsar::FitRec *__restrict__ rec, int64_t n_tx, double *__restrict__ tx,
                                                int32_t *__restrict__ worst, double *__restrict__ part, int32_t *__restrict__ part_row) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_chunks) return;
    const int64_t g = s / emsar::kFitGroup;
    const emsar::FitAcc A = emsar::fit_walk_chunk(idx, group_base[g] + (s % emsar::kFitGroup), group_steps[g], theta[chunk_tid[s]], rec);
    const int32_t o = chunk_out[s];
    if (o >= 0) {
        tx[o] = A.chi2; tx[n_tx + o] = A.dev; tx[2 * n_tx + o] = A.miss; tx[3 * n_tx + o] = A.df;
        worst[o] = A.row;
    } else {
        const int64_t k = -1 - (int64_t)o;
        part[k] = A.chi2; part[n_chunks + k] = A.dev; part[2 * n_chunks + k] = A.miss; part[3 * n_chunks + k] = A.df;
        part[4 * n_chunks + k] = A.best;
        part_row[k] = A.row;
    }
}

// One lane per transcript of more than one chunk.  multi [n_multi][3] = library index, first original chunk, end
__global__ __launch_bounds__(256) void k_fit_tx_finish(int64_t n_multi, const int32_t *__restrict__ multi, const double *__restrict__ part,
                                                       const int32_t *__restrict__ part_row, int64_t n_chunks, int64_t n_tx,
                                                       double *__restrict__ tx, int32_t *__restrict__ worst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_multi) return;
    const int32_t o = multi[3 * i];
    const emsar::FitAcc A = emsar::fit_finish(part, part_row, n_chunks, multi[3 * i + 1], multi[3 * i + 2]);
    tx[o] = A.chi2; tx[n_tx + o] = A.dev; tx[2 * n_tx + o] = A.miss; tx[3 * n_tx + o] = A.df;
    worst[o] = A.row;
}

// out[0..3] = sum q, sum d, sum a over the rows that are not infeasible, and the number of infeasible rows, in the order
// emsar::fit_totals_host restates: ONE workgroup, lane l takes the rows l, l + 1024, ..
__global__ __launch_bounds__(1024) void k_fit_totals(int64_t n_rows, const emsar::FitRec *__restrict__ rec, double *__restrict__ out) {
    __shared__ double red[16];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = threadIdx.x; r < n_rows; r += 1024) {
        const emsar::FitRec x = rec[r];
        if (emsar::fit_rec_infeasible(x)) v[3] += 1.0;
        else { v[0] += x.q; v[1] += x.d; v[2] += x.a; }
    }
    for (int k = 0; k < 4; k++) {
        const double tot = block_sum<1024>(v[k], red);
        if (threadIdx.x == 0) out[k] = tot;
        __syncthreads();
    }
}

}  // namespace

// What the model fit keeps on the device per structure, built on first use (fit.hpp) and dropped by upload_structure: the CSR in the
// caller's order and numbering (the layout's own CSR may carry the library's tids), the transposed index, the rows' records and the
// chunks' partials.
struct FitDev {
    bool ready = false, csr_ready = false;      // the index with its tables; the CSR alone (fit_ensure_csr: asym.hpp needs no index)
    int64_t n_chunks = 0, n_groups = 0, n_multi = 0, index_slots = 0, index_bytes = 0;
    emsar::DevBuf<uint64_t> d_row_ptr;
    emsar::DevBuf<int32_t> d_col;
    emsar::DevBuf<int32_t> d_idx, d_group_steps, d_chunk_tid, d_chunk_out, d_multi, d_part_row;
    emsar::DevBuf<int64_t> d_group_base;
    emsar::DevBuf<emsar::FitRec> d_rec;
    emsar::DevBuf<double> d_part;     // [5][n_chunks], allocated when a transcript has more than one chunk
};
