// kernels_genes.hpp -- gene-level sums (emsar_hip_gene_sums, emsar_hip_bootstrap_genes): per gene, the sum of its transcripts' values,
// in a fixed order.  The Welford reduction of the bootstrap's gene sums over the replicates is k_boot_accum (kernels_boot.hpp) run on
// the [nb][n_genes] sums instead of theta: same arithmetic, so a one-transcript gene gets that transcript's bits.
#pragma once
// included by emsar_hip.hip only (one translation unit: the kernels live in its anonymous namespace)

namespace {

constexpr int kGeneChunk = 256;   // transcripts per chunk of a gene (the order is part of the ABI, include/emsar_hip.h)

// One lane per (chunk, column y): the chunk's transcripts, library indices gtx[cbeg[k] .. cbeg[k+1]), ascending caller tid, added left
// to right.  cout[k] >= 0: the gene has this one chunk and the sum is final (out[y][cout[k]]); -1: a partial for k_gene_finish.
//   x [ncol][n], out [ncol][n_genes], part [ncol][n_chunks]
__global__ __launch_bounds__(256) void k_gene_sums(int64_t n_chunks, const int32_t *__restrict__ cbeg, const int32_t *__restrict__ cout,
                                                   const int32_t *__restrict__ gtx, const double *__restrict__ x, int64_t n,
                                                   double *__restrict__ out, int64_t n_genes, double *__restrict__ part) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_chunks) return;
    const int64_t y = blockIdx.y;
    const double *xr = x + y * n;
    const int32_t b = cbeg[k], e = cbeg[k + 1];
    double s = 0.0;
    if (b < e) {
        s = xr[gtx[b]];
        for (int32_t i = b + 1; i < e; i++) s += xr[gtx[i]];
    }
    const int32_t g = cout[k];
    if (g >= 0) out[y * n_genes + g] = s;
    else part[y * n_chunks + k] = s;
}

// One lane per (gene of more than one chunk, column y): its chunk partials added in chunk order.
//   multi [n_multi][3] = gene, first chunk, end chunk
__global__ __launch_bounds__(256) void k_gene_finish(int64_t n_multi, const int32_t *__restrict__ multi, const double *__restrict__ part,
                                                     int64_t n_chunks, double *__restrict__ out, int64_t n_genes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_multi) return;
    const int64_t y = blockIdx.y;
    const int32_t g = multi[3 * i], c0 = multi[3 * i + 1], c1 = multi[3 * i + 2];
    const double *pr = part + y * n_chunks;
    double s = pr[c0];
    for (int32_t c = c0 + 1; c < c1; c++) s += pr[c];
    out[y * n_genes + g] = s;
}

}  // namespace
