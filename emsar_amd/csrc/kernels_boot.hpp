// kernels_boot.hpp -- the Poisson bootstrap (emsar_hip_bootstrap): draws, the closed-form and merge steps of a batch of replicates,
// and the per-transcript reduction over the replicates.  The batched set solver is k_solve_sets_boot (kernels_sets.hpp).
// The depth subsampling (emsar_hip_subsample) runs the same steps on binomial draws (k_sub_draw) and scales every replicate to its
// own depth (k_sub_scale) before the reduction.
#pragma once
// included by emsar_hip.hip only (one translation unit: the kernels live in its anonymous namespace)

namespace {

// the drawn weight w of caller row c in replicate y of the batch: into w_out and into the row's slot of the set solver
__device__ __forceinline__ void boot_place(int64_t c, int64_t y, int32_t w, int64_t n_rows, const int64_t *__restrict__ slot,
                                           int32_t *__restrict__ w_out, double *__restrict__ slots, int64_t slot_stride) {
    if (w_out) w_out[y * n_rows + c] = w;
    if (slot && w > 0) {
        const int64_t s = slot[c];
        if (s >= 0) atomic_add_f64(slots + y * slot_stride + s, (double)w);
    }
}

// One lane per (caller row, replicate of the batch): w = Poisson(R_c) under key (seed, first + y), counter (c, j, 0, 0).
//   w_out (may be null): [nb][n_rows] the drawn weights in caller order
//   slot  (may be null): [n_rows] where the weight of row c feeds the set solver -- an index into one replicate's [row_w | usum]
//                         block of slot_stride doubles, -1 = nowhere (streamed rows, rows outside the likelihood)
// The slot values are integers held in doubles, so the adds are exact and their order does not matter.
__global__ __launch_bounds__(256) void k_boot_draw(int64_t n_rows, uint64_t seed, int64_t first, const int32_t *__restrict__ R,
                                                   const int64_t *__restrict__ slot, int32_t *__restrict__ w_out,
                                                   double *__restrict__ slots, int64_t slot_stride) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_rows) return;
    const int64_t y = blockIdx.y;
    const int32_t w = emsar::boot_poisson(seed, (uint64_t)(first + y), (uint64_t)c, R[c]);
    boot_place(c, y, w, n_rows, slot, w_out, slots, slot_stride);
}

// The subsampling's draw: w = Binomial(R_c, f) under key (seed, first + y), counter (c, j, 1, bits of f), placed like the bootstrap's.
// n_drawn[y] += the replicate's total sum_c w_c: one integer atomic per wavefront (integers commute: exact, any order).
__global__ __launch_bounds__(256) void k_sub_draw(int64_t n_rows, uint64_t seed, int64_t first, double f, const int32_t *__restrict__ R,
                                                  const int64_t *__restrict__ slot, int32_t *__restrict__ w_out,
                                                  double *__restrict__ slots, int64_t slot_stride, long long *__restrict__ n_drawn) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t y = blockIdx.y;
    int32_t w = 0;
    if (c < n_rows) {
        w = emsar::boot_binomial(seed, (uint64_t)(first + y), (uint64_t)c, R[c], f);
        boot_place(c, y, w, n_rows, slot, w_out, slots, slot_stride);
    }
    long long tot = w;
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if ((threadIdx.x & 63) == 0 && tot > 0) __hip_atomic_fetch_add(n_drawn + y, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// theta_b -> theta_b * N_R / N_b, the FPKM of replicate b at its own depth (0 when nothing was drawn): E carries the full sample's
// read total and the fixed point is linear in that scale.  blockIdx.y = replicate of the batch; the factor is computed once per workgroup.
__global__ __launch_bounds__(256) void k_sub_scale(int n, double n_full, const long long *__restrict__ n_drawn, double *__restrict__ theta) {
    __shared__ double factor;
    if (threadIdx.x == 0) { const long long nb = n_drawn[blockIdx.y]; factor = nb > 0 ? n_full / (double)nb : 0.0; }
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) theta[(int64_t)blockIdx.y * n + t] *= factor;
}

// g_u of every resident transcript from the replicate's folded single-row counts: g_u[k] = usum[g_tid[k]]
__global__ void k_boot_gather_u(int64_t n_gu, const int32_t *__restrict__ g_tid, const double *__restrict__ slots, int64_t slot_stride,
                                int64_t usum_off, double *__restrict__ g_u) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_gu) return;
    const int64_t y = blockIdx.y;
    g_u[y * n_gu + k] = slots[y * slot_stride + usum_off + g_tid[k]];
}

// closed-form transcripts of every replicate (k_closed_form): theta = usum / den
__global__ void k_boot_closed(int n, const uint8_t *__restrict__ kind, const double *__restrict__ slots, int64_t slot_stride,
                              int64_t usum_off, const double *__restrict__ den, double *__restrict__ theta) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t y = blockIdx.y;
    if (kind[t] == emsar::KIND_CLOSED) theta[y * n + t] = den[t] > 0.0 ? slots[y * slot_stride + usum_off + t] / den[t] : 0.0;
}

// the streaming solve's result of one replicate into its row of the batch: every transcript (kind null), or those the set
// solver does not cover (streamed and cluster sets)
__global__ void k_boot_take_streamed(int n, const uint8_t *__restrict__ kind, const double *__restrict__ src, double *__restrict__ dst) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (!kind || kind[t] == emsar::KIND_STREAMED || kind[t] == emsar::KIND_CLUSTER) dst[t] = src[t];
}

// sum_t theta_b,t per replicate (the TPM denominator): one workgroup per replicate, fixed order
__global__ __launch_bounds__(1024) void k_boot_sums(int n, const double *__restrict__ theta, double *__restrict__ sums) {
    __shared__ double red[16];
    const double *x = theta + (int64_t)blockIdx.x * n;
    double s = 0.0;
    for (int t = threadIdx.x; t < n; t += 1024) s += x[t];
    const double tot = block_sum<1024>(s, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// Welford's running mean / sum of squared deviations per transcript over the batch's replicates, in replicate order, continuing from
// the `done` replicates before it: the result does not depend on how the replicates were cut into batches.
// acc: [4][n] mean FPKM, M2 FPKM, mean TPM, M2 TPM
__global__ void k_boot_accum(int n, int nb, int64_t done, const double *__restrict__ theta, const double *__restrict__ sums,
                             double *__restrict__ acc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    double mf = acc[t], qf = acc[n + t], mt = acc[2 * n + t], qt = acc[3 * n + t];
    for (int y = 0; y < nb; y++) {
        const double k = (double)(done + y + 1);
        const double x = theta[(int64_t)y * n + t];
        const double s = sums[y];
        const double tp = s > 0.0 ? x * 1e6 / s : 0.0;
        const double df = x - mf;
        mf += df / k;
        qf += df * (x - mf);
        const double dt = tp - mt;
        mt += dt / k;
        qt += dt * (tp - mt);
    }
    acc[t] = mf; acc[n + t] = qf; acc[2 * n + t] = mt; acc[3 * n + t] = qt;
}

}  // namespace
