// kernels_quant.hpp -- quantiles over the bootstrap's replicates (emsar_hip_bootstrap_quantiles, emsar_hip_quantiles_host).
//
// Definition (include/emsar_hip.h): for the order statistics x_(0) <= ... <= x_(B-1) of one column and a probability q in [0, 1],
//   h = q * (double)(B - 1), i = (int64)floor(h), g = h - (double)i,
//   result = x_(i) when g == 0 or i == B - 1, else x_(i) + g * (x_(i+1) - x_(i)),
// subtract, multiply and add rounded separately (contraction off): host and device give the same bits, and since sorting does not
// round, the result does not depend on the batch, the layout, the numbering or the device.
//
// k_boot_quantiles: one workgroup of 256 lanes per tile of C neighbouring columns of a [B][n] buffer, the tile kept in LDS as
// [Bp][C] (Bp = B rounded up to a power of two, the padding +inf) -- the buffer's own order, so a global row of the tile is C
// consecutive doubles (coalesced across the columns) and the LDS stores of the load are conflict-free.  A bitonic network sorts
// all C columns in lockstep: lane k takes compare-exchange (pair k / C, column k % C) of a stage (its last stages, j <= 2, put the
// wave's groups of C doubles a multiple of 256 B apart: bank conflicts there, not measured).  C = 2048 / Bp clamped to
// 1 .. 32: 16 KiB of LDS or less for B <= 2048 (16 KiB at B = 100: ten workgroups to a CU's 160 KiB), 32 KiB for B up to 4096, the
// limit (kQuantMaxRep).  After FPKM the tile is loaded again as TPM_b = S_b > 0 ? x_b * 1e6 / S_b : 0 (k_boot_accum's expression)
// and sorted again: TPM's order is not FPKM's, S_b differs from replicate to replicate.
//
// k_quant_sums: the S_b of the quantile stage.  k_boot_sums adds theta_b in the library's order, so its S_b carries the library's own
// transcript numbering in its last bits (mean and sd keep it, as before).  The quantiles must not: k_quant_sums adds the same values with
// the same reduction tree in the CALLER's order, through the caller -> library map.  Without renumbering the two are the same bits.
#pragma once
#include <cmath>
#include <cstdint>

namespace emsar {

constexpr int kQuantMaxRep = 4096;        // replicates per column that fit the LDS path: 32 KiB of doubles

// the q-quantile of B sorted values x[0], x[stride], ..., x[(B - 1) * stride]; q in [0, 1]
__host__ __device__ inline double quantile_sorted(const double *x, int64_t stride, int32_t B, double q) {
#pragma clang fp contract(off)
    const double h = q * (double)(B - 1);
    const int64_t i = (int64_t)floor(h);
    const double g = h - (double)i;
    const double lo = x[i * stride];
    if (g == 0.0 || i == (int64_t)B - 1) return lo;
    const double d = x[(i + 1) * stride] - lo;
    const double s = g * d;
    return lo + s;
}

// columns per tile for Bp padded replicates (both powers of two), and its log2
inline int quant_tile_shift(int Bp) {
    int sh = 0;
    while (sh < 5 && ((int64_t)Bp << (sh + 1)) <= 2048) sh++;
    return sh;
}

}  // namespace emsar

// included by emsar_hip.hip only (one translation unit: the kernels live in its anonymous namespace)
namespace {

// sum_t theta_b,t per held replicate over caller tids t = 0 .. n-1 (lib_of null: library order = caller order): one workgroup per
// replicate, lane i adds t = i, i + 1024, ... in turn, then the fixed-order workgroup sum of k_boot_sums
__global__ __launch_bounds__(1024) void k_quant_sums(int n, const int32_t *__restrict__ lib_of, const double *__restrict__ theta,
                                                     double *__restrict__ sums) {
    __shared__ double red[16];
    const double *x = theta + (int64_t)blockIdx.x * n;
    double s = 0.0;
    for (int t = threadIdx.x; t < n; t += 1024) s += x[lib_of ? lib_of[t] : t];
    const double tot = block_sum<1024>(s, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// The bitonic network over a tile [Bp][1 << cs] in LDS, all columns in lockstep, ascending down every column; called by all 256
// lanes of the workgroup after the barrier that follows the tile's stores, ends behind a barrier.  (k_boot_quantiles, k_iso_quantiles)
__device__ __forceinline__ void quant_sort_tile(double *smem, int Bp, int cs) {
    const int cmask = (1 << cs) - 1;
    for (int size = 2; size <= Bp; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int k = threadIdx.x; k < ((Bp >> 1) << cs); k += 256) {
                const int p = k >> cs, c = k & cmask;
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const double a = smem[(i << cs) + c], b = smem[(l << cs) + c];
                if ((a > b) == ((i & size) == 0)) { smem[(i << cs) + c] = b; smem[(l << cs) + c] = a; }
            }
            __syncthreads();
        }
}

//   x [B][n] the held replicates, sums [B] their TPM denominators, q [n_q]; out_f, out_t [n_q][n]
//   Bp = B rounded up to a power of two, cs = log2 of the tile's columns; dynamic LDS: (Bp << cs) doubles
__global__ __launch_bounds__(256) void k_boot_quantiles(int64_t n, int B, int Bp, int cs, const double *__restrict__ x,
                                                        const double *__restrict__ sums, int n_q, const double *__restrict__ q,
                                                        double *__restrict__ out_f, double *__restrict__ out_t) {
    extern __shared__ double smem[];
    const int C = 1 << cs, cmask = C - 1;
    const int64_t col0 = (int64_t)blockIdx.x << cs;
    const int nc = (int)(n - col0 < C ? n - col0 : C);
    for (int pass = 0; pass < 2; pass++) {
        for (int k = threadIdx.x; k < (Bp << cs); k += 256) {
            const int r = k >> cs, c = k & cmask;
            double v = INFINITY;
            if (r < B && c < nc) {
                v = x[(int64_t)r * n + col0 + c];
                if (pass) { const double s = sums[r]; v = s > 0.0 ? v * 1e6 / s : 0.0; }
            }
            smem[k] = v;
        }
        __syncthreads();
        quant_sort_tile(smem, Bp, cs);
        double *out = pass ? out_t : out_f;
        for (int64_t k = threadIdx.x; k < ((int64_t)n_q << cs); k += 256) {
            const int qi = (int)(k >> cs), c = (int)(k & cmask);
            if (c < nc) out[(int64_t)qi * n + col0 + c] = emsar::quantile_sorted(smem + c, C, B, q[qi]);
        }
        __syncthreads();
    }
}

}  // namespace
