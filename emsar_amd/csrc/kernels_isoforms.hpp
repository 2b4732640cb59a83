// kernels_isoforms.hpp -- isoform usage (emsar_hip_isoform_usage, emsar_hip_bootstrap_isoforms): each transcript's share of its gene's
// sum, the gene's dominant isoform, and their statistics over the bootstrap's replicates.  FP64, no atomics.
//
// Definitions (include/emsar_hip.h "isoform usage"): for a column x of non-negative values and the gene sums G of kernels_genes.hpp,
//   usage     u_t = G_g(t) > 0 ? x_t / G_g(t) : 0, one IEEE division (iso_usage below, the one expression host and device share);
//             0 for a transcript in no gene
//   dominant  the transcript of gene g with the largest x_t, the smallest caller tid among equal maxima, -1 when G_g is not > 0.
//             Values are compared, not usages: x_t / G rounds, and two different values may round to one usage.
// A gene's transcripts are stored by ascending caller tid (GeneMap), so the first maximum of a left-to-right walk with a strict > is
// the one with the smallest caller tid whatever the library's own numbering.
#pragma once
#include <cstdint>

namespace emsar {

__host__ __device__ inline double iso_usage(double x, double gene_sum) { return gene_sum > 0.0 ? x / gene_sum : 0.0; }

}  // namespace emsar

// included by emsar_hip.hip only (one translation unit: the kernels live in its anonymous namespace)
namespace {

// One lane per (transcript, column y), library order: out[y][t] = usage of x[y][t] in its gene's sum.
//   x, out [ncol][n], gsum [ncol][n_genes], gene_of_lib [n] gene of library index t, -1 = none
__global__ __launch_bounds__(256) void k_iso_usage(int n, const int32_t *__restrict__ gene_of_lib, const double *__restrict__ x,
                                                   const double *__restrict__ gsum, int64_t n_genes, double *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t y = blockIdx.y;
    const int32_t g = gene_of_lib[t];
    out[y * n + t] = g >= 0 ? emsar::iso_usage(x[y * n + t], gsum[y * n_genes + g]) : 0.0;
}

// One lane per (chunk, column y), the walk of k_gene_sums: the chunk's first maximum.  cout[k] >= 0: the gene has this one chunk,
// dom[y][cout[k]] = its library index, or -1 when the gene's sum is not > 0 (an empty gene included); -1: a (value, index) partial
// for k_iso_dominant_finish.
//   x [ncol][n], gsum, dom [ncol][n_genes], part_v, part_i [ncol][n_chunks]
__global__ __launch_bounds__(256) void k_iso_dominant(int64_t n_chunks, const int32_t *__restrict__ cbeg, const int32_t *__restrict__ cout,
                                                      const int32_t *__restrict__ gtx, const double *__restrict__ x, int64_t n,
                                                      const double *__restrict__ gsum, int32_t *__restrict__ dom, int64_t n_genes,
                                                      double *__restrict__ part_v, int32_t *__restrict__ part_i) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_chunks) return;
    const int64_t y = blockIdx.y;
    const double *xr = x + y * n;
    const int32_t b = cbeg[k], e = cbeg[k + 1];
    double best = 0.0;
    int32_t at = -1;
    if (b < e) {
        at = gtx[b];
        best = xr[at];
        for (int32_t i = b + 1; i < e; i++) {
            const int32_t t = gtx[i];
            const double v = xr[t];
            if (v > best) { best = v; at = t; }
        }
    }
    const int32_t g = cout[k];
    if (g >= 0) dom[y * n_genes + g] = gsum[y * n_genes + g] > 0.0 ? at : -1;
    else { part_v[y * n_chunks + k] = best; part_i[y * n_chunks + k] = at; }
}

// One lane per (gene of more than one chunk, column y): the first maximum over its chunks' partials, in chunk order.
//   multi [n_multi][3] = gene, first chunk, end chunk
__global__ __launch_bounds__(256) void k_iso_dominant_finish(int64_t n_multi, const int32_t *__restrict__ multi,
                                                             const double *__restrict__ part_v, const int32_t *__restrict__ part_i,
                                                             int64_t n_chunks, const double *__restrict__ gsum, int32_t *__restrict__ dom,
                                                             int64_t n_genes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_multi) return;
    const int64_t y = blockIdx.y;
    const int32_t g = multi[3 * i], c0 = multi[3 * i + 1], c1 = multi[3 * i + 2];
    const double *pv = part_v + y * n_chunks;
    const int32_t *pi = part_i + y * n_chunks;
    double best = pv[c0];
    int32_t at = pi[c0];
    for (int32_t c = c0 + 1; c < c1; c++)
        if (pv[c] > best) { best = pv[c]; at = pi[c]; }
    dom[y * n_genes + g] = gsum[y * n_genes + g] > 0.0 ? at : -1;
}

// k_boot_accum's Welford recurrence on the usage of the batch's replicates, in replicate order, continuing from the `done`
// replicates before it, and the number of replicates in which the transcript is its gene's dominant isoform.  One lane per
// transcript (library order).  Subtract, divide, multiply and add rounded separately (contraction off): the host restates it bit for bit.
//   theta [nb][n], gsum, dom [nb][n_genes]; acc [2][n] mean, M2 of the usage; count [n]
__global__ __launch_bounds__(256) void k_iso_accum(int n, int nb, int64_t done, const int32_t *__restrict__ gene_of_lib,
                                                   const double *__restrict__ theta, const double *__restrict__ gsum,
                                                   const int32_t *__restrict__ dom, int64_t n_genes, double *__restrict__ acc,
                                                   int32_t *__restrict__ count) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int32_t g = gene_of_lib[t];
    double m = acc[t], q = acc[n + t];
    int32_t cnt = count[t];
    for (int y = 0; y < nb; y++) {
        const double k = (double)(done + y + 1);
        const double u = g >= 0 ? emsar::iso_usage(theta[(int64_t)y * n + t], gsum[(int64_t)y * n_genes + g]) : 0.0;
        const double d = u - m;
        m += d / k;
        q += d * (u - m);
        if (g >= 0 && dom[(int64_t)y * n_genes + g] == t) cnt++;
    }
    acc[t] = m; acc[n + t] = q;
    count[t] = cnt;
}

// Quantiles of the usage over the held replicates: k_boot_quantiles' tile (kernels_quant.hpp), loaded as u = usage of theta[r][t] in
// gsum[r][gene of t], sorted once.  Usage is the same for FPKM and TPM (the replicate's scale cancels): one pass.
//   theta [B][n], gsum [B][n_genes], q [n_q]; out [n_q][n]; dynamic LDS: (Bp << cs) doubles
__global__ __launch_bounds__(256) void k_iso_quantiles(int64_t n, int B, int Bp, int cs, const int32_t *__restrict__ gene_of_lib,
                                                       const double *__restrict__ theta, const double *__restrict__ gsum, int64_t n_genes,
                                                       int n_q, const double *__restrict__ q, double *__restrict__ out) {
    extern __shared__ double smem[];
    const int C = 1 << cs, cmask = C - 1;
    const int64_t col0 = (int64_t)blockIdx.x << cs;
    const int nc = (int)(n - col0 < C ? n - col0 : C);
    for (int k = threadIdx.x; k < (Bp << cs); k += 256) {
        const int r = k >> cs, c = k & cmask;
        double v = INFINITY;
        if (r < B && c < nc) {
            const int32_t g = gene_of_lib[col0 + c];
            v = g >= 0 ? emsar::iso_usage(theta[(int64_t)r * n + col0 + c], gsum[(int64_t)r * n_genes + g]) : 0.0;
        }
        smem[k] = v;
    }
    __syncthreads();
    quant_sort_tile(smem, Bp, cs);
    for (int64_t k = threadIdx.x; k < ((int64_t)n_q << cs); k += 256) {
        const int qi = (int)(k >> cs), c = (int)(k & cmask);
        if (c < nc) out[(int64_t)qi * n + col0 + c] = emsar::quantile_sorted(smem + c, C, B, q[qi]);
    }
}

}  // namespace
