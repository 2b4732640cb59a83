// boot_rng.hpp -- the counter-based draws of the bootstrap (emsar_hip_bootstrap: Poisson) and of the depth subsampling
// (emsar_hip_subsample: binomial, at the end of this comment), host and device alike.
//
// Replicate b of seed s gives caller row c the weight w ~ Poisson(R_c).  Every draw is a pure function of (s, b, c, R_c):
//   * generator: Philox4x64-10 (Salmon et al., SC'11), key = (s, b), counter = (c, j, 0, 0) with j = 0, 1, ... the 4-word
//     blocks one draw consumes in turn -- the generator numpy ships as numpy.random.Philox;
//   * uniform = (word >> 11) * 2^-53, words taken in order (block 0 words 0..3, block 1 words 0..3, ...);
//   * R <= 16: inversion from the correctly rounded e^-R, one uniform;
//   * R > 16: transformed rejection with squeeze (PTRS, Hoermann 1993 -- the method numpy uses for lambda >= 10), two uniforms per
//     trial, with its own Stirling series for log k!.
// So a draw does not depend on the layout, the set partition, the batch or the launch shape.  The inversion uses only *, /, +
// and compares with floating contraction off: host and device give the same bits.  PTRS calls log and sqrt; sqrt is correctly
// rounded on both sides, log may differ by an ulp between the host libm and the device library, which can flip an acceptance
// test that lands on its edge.
//
// Subsampling at fraction f gives row c the weight w ~ Binomial(R_c, f), a pure function of (s, b, c, R_c, f): the same generator and
// key with counter (c, j, 1, bits of the double f), so the draws of a fraction do not depend on the other fractions of a call and are
// independent of the bootstrap's under the same seed.  p = min(f, 1 - f), k ~ Binomial(R, p), w = k or R - k;
//   * R p < 10: inversion from q^R (square and multiply), one uniform, *, /, +, - and compares only: host and device give the same bits;
//   * R p >= 10: transformed rejection with squeeze (BTRS, Hoermann 1993, "The generation of binomial random variates"), two uniforms
//     per trial, log-factorials from boot_loggam; log as for PTRS.
#pragma once
#include <cmath>
#include <cstdint>

namespace emsar {

constexpr uint64_t kPhiloxM0 = 0xD2E7470EE14C6C93ull, kPhiloxM1 = 0xCA5A826395121157ull;
constexpr uint64_t kPhiloxW0 = 0x9E3779B97F4A7C15ull, kPhiloxW1 = 0xBB67AE8584CAA73Bull;
constexpr int kBootInversionMax = 16;      // R up to this: inversion; above: PTRS

__host__ __device__ inline void philox_mulhilo(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// one block: the four output words of counter (c0, c1, c2, c3) under key (k0, k1)
__host__ __device__ inline void philox4x64_10(uint64_t &c0, uint64_t &c1, uint64_t &c2, uint64_t &c3, uint64_t k0, uint64_t k1) {
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += kPhiloxW0; k1 += kPhiloxW1; }
        uint64_t hi0, lo0, hi1, lo1;
        philox_mulhilo(kPhiloxM0, c0, hi0, lo0);
        philox_mulhilo(kPhiloxM1, c2, hi1, lo1);
        const uint64_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
}

// the uniforms of one draw, in order
struct BootUniforms {
    uint64_t k0, k1, row, c2, c3, j = 0;     // counter (row, j, c2, c3): c2 = c3 = 0 the bootstrap, (1, bits of f) the subsampling
    uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    int i = 4;
    __host__ __device__ BootUniforms(uint64_t seed, uint64_t rep, uint64_t r, uint64_t c2_ = 0, uint64_t c3_ = 0)
        : k0(seed), k1(rep), row(r), c2(c2_), c3(c3_) {}
    __host__ __device__ double next() {
        if (i == 4) {
            w0 = row; w1 = j++; w2 = c2; w3 = c3;
            philox4x64_10(w0, w1, w2, w3, k0, k1);
            i = 0;
        }
        const uint64_t w = i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3;     // no indexed register array (scratch on the device)
        i++;
        return (double)(w >> 11) * 0x1p-53;
    }
};

// log Gamma(x) for integer-valued x >= 1: Stirling series at x0 = max(x, 7), then log Gamma(x) = log Gamma(x0) - sum log(x0 - k)
__host__ __device__ inline double boot_loggam(double x) {
#pragma clang fp contract(off)
    if (x == 1.0 || x == 2.0) return 0.0;
    const int n = x < 7.0 ? (int)(7.0 - x) : 0;
    double x0 = x + (double)n;
    const double x2 = 1.0 / (x0 * x0);
    // Bernoulli coefficients B_2k / (2k (2k-1)), k = 10 .. 1 (Horner from the top)
    const double c[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
                          8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
                          1.796443723688307e-01, -1.39243221690590e+00};
    double g = c[9];
    for (int k = 8; k >= 0; k--) { g = g * x2; g = g + c[k]; }
    double gl = g / x0 + 0.5 * log(2.0 * 3.141592653589793) + (x0 - 0.5) * log(x0) - x0;
    for (int k = 1; k <= n; k++) { gl = gl - log(x0 - 1.0); x0 = x0 - 1.0; }
    return gl;
}

// w ~ Poisson(R) for caller row `row` of replicate `rep` of seed `seed`; R <= 0 gives 0.  Saturates at INT32_MAX.
__host__ __device__ inline int32_t boot_poisson(uint64_t seed, uint64_t rep, uint64_t row, int32_t R) {
#pragma clang fp contract(off)
    if (R <= 0) return 0;
    BootUniforms U(seed, rep, row);
    if (R <= kBootInversionMax) {
        // e^-n, n = 0..16, correctly rounded
        constexpr double kExpNeg[kBootInversionMax + 1] = {
            0x1.0000000000000p+0, 0x1.78b56362cef38p-2, 0x1.152aaa3bf81ccp-3, 0x1.97db0ccceb0afp-5, 0x1.2c155b8213cf4p-6,
            0x1.b993fe00d5376p-8, 0x1.44e51f113d4d6p-9, 0x1.de16b9c24a98fp-11, 0x1.5fc21041027adp-12, 0x1.02cf22526545ap-13,
            0x1.7cd79b5647c9bp-15, 0x1.18354238f6764p-16, 0x1.9c54c3b43bc8bp-18, 0x1.2f6053b981d98p-19, 0x1.be6c6fdb01612p-21,
            0x1.4875ca227ec38p-22, 0x1.e355bbaee85cbp-24};
        const double u = U.next(), lam = (double)R;
        double p = kExpNeg[R], F = p;
        int k = 0;
        while (u >= F && k < 64) { k++; p = p * lam / (double)k; F = F + p; }
        return k;
    }
    const double lam = (double)R, slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (;;) {
        const double Uc = U.next() - 0.5, V = U.next();
        const double us = 0.5 - fabs(Uc);
        const double kd = floor((2.0 * a / us + b) * Uc + lam + 0.43);
        if (us >= 0.07 && V <= vr) return kd >= 2147483647.0 ? 2147483647 : (int32_t)kd;
        if (kd < 0.0 || (us < 0.013 && V > us)) continue;
        if ((log(V) + log(invalpha) - log(a / (us * us) + b)) <= (-lam + kd * loglam - boot_loggam(kd + 1.0)))
            return kd >= 2147483647.0 ? 2147483647 : (int32_t)kd;
    }
}

constexpr double kSubInversionMax = 10.0;  // R * min(f, 1 - f) below this: inversion; from it on: BTRS

// w ~ Binomial(R, f) for caller row `row` of replicate `rep` of seed `seed` at fraction f in (0, 1]; R <= 0 gives 0, f >= 1 gives R.
__host__ __device__ inline int32_t boot_binomial(uint64_t seed, uint64_t rep, uint64_t row, int32_t R, double f) {
#pragma clang fp contract(off)
    if (R <= 0) return 0;
    if (f >= 1.0) return R;
    BootUniforms U(seed, rep, row, 1, __builtin_bit_cast(uint64_t, f));
    const bool flip = f > 0.5;
    const double p = flip ? 1.0 - f : f, q = 1.0 - p, n = (double)R;
    if (n * p < kSubInversionMax) {
        double pr = 1.0, sq = q;                   // q^R
        for (uint32_t e = (uint32_t)R; e; e >>= 1) { if (e & 1u) pr = pr * sq; sq = sq * sq; }
        const double u = U.next(), s = p / q;
        double F = pr;
        int32_t k = 0;
        while (u >= F && k < R) { k++; pr = pr * s * (double)(R - k + 1) / (double)k; F = F + pr; }
        return flip ? R - k : k;
    }
    const double spq = sqrt(n * p * q);
    const double b = 1.15 + 2.53 * spq;
    const double a = -0.0873 + 0.0248 * b + 0.01 * p;
    const double c = n * p + 0.5;
    const double vr = 0.92 - 4.2 / b;
    const double alpha = (2.83 + 5.1 / b) * spq;
    const double lpq = log(p / q);
    const double m = floor((n + 1.0) * p);
    const double h = boot_loggam(m + 1.0) + boot_loggam(n - m + 1.0);
    for (;;) {
        const double Uc = U.next() - 0.5, V = U.next();
        const double us = 0.5 - fabs(Uc);
        const double kd = floor((2.0 * a / us + b) * Uc + c);
        if (!(us >= 0.07 && V <= vr)) {
            if (kd < 0.0 || kd > n) continue;
            if (!(log(V * alpha / (a / (us * us) + b)) <= h - boot_loggam(kd + 1.0) - boot_loggam(n - kd + 1.0) + (kd - m) * lpq)) continue;
        }
        const int32_t k = (int32_t)kd;
        return flip ? R - k : k;
    }
}

}  // namespace emsar
