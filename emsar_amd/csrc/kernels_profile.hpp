// kernels_profile.hpp -- k_profile_sets: one confidence limit of a profile-likelihood interval (emsar_hip_profile; driver: profile.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_presence.hpp

namespace {

// One unit of work: one limit of local transcript `t` of set `set` of its size class.  side 0 = lower (multipliers s > 1), 1 = upper
// (s < 1).  theta_hat is the baseline's value of t, F_hat the baseline's F of the set (PresenceRec.F of the item (set, -1)).
struct ProfileItem { int32_t set, t, side, reserved0; double theta_hat, F_hat; };
// What a search leaves: the last evaluation's x = theta_t(s), its deviance and its multiplier; the solves spent, their passes summed,
// and flags: bit 0 = the search met its stopping rule, bit 1 = every solve of it converged
struct ProfileRec { double x, dev, s, F; int32_t evals, passes, flags, infeasible; };
static_assert(sizeof(ProfileItem) == 32, "ProfileItem is written by the host as 32 bytes");
static_assert(sizeof(ProfileRec) == 48, "ProfileRec is read by the host as 48 bytes");
enum { PROFILE_REC_SEARCH_OK = 1, PROFILE_REC_SOLVES_OK = 2 };

struct ProfileSearchParams { double q, dev_tol; int32_t max_evals, reserved0; };

// The root search of one limit, in z = log s on h(z) = sqrt(dev) - sqrt(q); the same code runs in the kernel (every value it sees is
// the same in all threads of the workgroup) and on the host (one-transcript components).  h(0) = -sqrt(q) is known without a solve.
//   bracket   start at z0 = +-log(1 + sqrt(q / n_t)), n_t = theta_hat_t den_t; while h < 0 there, double z (s squares its distance from
//             1).  On the upper side with n_t < q -- theta_hat_t = 0 included: fewer expected reads than the cut, the Poisson guess says
//             nothing and would ask for a solve at s ~ sqrt(n_t / q), a problem scaled out of all proportion -- start at s = 1/2 and
//             quarter s instead
//   refine    Illinois (regula falsi that halves the weight of an end it keeps twice) on the bracket, replaced by the midpoint when
//             its point does not fall strictly inside the bracket
// Every step is one evaluation: z names its point, update() takes its h and sets the next z.
struct ProfileSearch {
    double z_lo, h_lo, z_hi, h_hi;       // h_lo < 0 <= h_hi once bracketed; |z_lo| < |z_hi|
    double z;                            // the point of the evaluation under way
    int bracketed, kept;                 // kept: +1 / -1 = the hi / lo end survived the last update
    bool from_zero;

    __host__ __device__ void start(int side, double n_t, double q) {
        const double sgn = side == 0 ? 1.0 : -1.0;
        from_zero = side == 1 && !(n_t >= q);
        z_lo = 0.0; h_lo = -sqrt(q); z_hi = 0.0; h_hi = 0.0; bracketed = 0; kept = 0;
        z = from_zero ? -0.6931471805599453 : sgn * log1p(sqrt(q / n_t));
        clamp();
    }
    __host__ __device__ void clamp() { z = z > 690.0 ? 690.0 : z < -690.0 ? -690.0 : z; }
    __host__ __device__ void update(double h) {
        if (!bracketed) {
            if (h >= 0.0) { z_hi = z; h_hi = h; bracketed = 1; }
            else { z_lo = z; h_lo = h; z = from_zero ? z - 1.3862943611198906 : 2.0 * z; clamp(); return; }
        } else if (h >= 0.0) {
            z_hi = z; h_hi = h;
            if (kept == -1) h_lo *= 0.5;
            kept = -1;
        } else {
            z_lo = z; h_lo = h;
            if (kept == 1) h_hi *= 0.5;
            kept = 1;
        }
        const double w = z_hi - z_lo;
        const double zn = z_lo - h_lo * w / (h_hi - h_lo);
        const bool inside = w > 0.0 ? (zn > z_lo && zn < z_hi) : (zn < z_lo && zn > z_hi);
        z = inside ? zn : z_lo + 0.5 * w;
    }
};

// a value every thread of the workgroup holds with the same bits, moved to scalar registers
__device__ __forceinline__ double profile_uniform(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Workgroup x runs the whole search of item x: each evaluation is solve_one_set with den_t taken as s * den_t in LDS (the maximiser of
// F - lambda theta_t, lambda = (s - 1) den_t: the constrained maximum of F at theta_t = x_t(s)), then the presence epilogue's F with the
// ORIGINAL den_t, dev = 2 (F_hat - F), and one step of ProfileSearch.  solve_one_set reloads the set and restarts from the uniform
// point each time: a record is a pure function of (item, P, Q).  The worst case is Q.max_evals * P.max_iter passes.
// Every branch of the loop is taken by the whole workgroup: it is decided on the reductions' results alone (set_reduce_sum leaves every
// thread the same bits; profile_uniform hands them to the scalar unit), the strided loops and the reductions stand outside any branch.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_profile_sets(const emsar::SetDesc *__restrict__ desc, const ProfileItem *__restrict__ items,
                                                          const int32_t *__restrict__ g_tid, const double *__restrict__ g_u,
                                                          const double *__restrict__ row_w, const uint16_t *__restrict__ rp_g,
                                                          const uint16_t *__restrict__ ent_g, const uint16_t *__restrict__ cp_g,
                                                          const uint16_t *__restrict__ crow_g, const double *__restrict__ den_g,
                                                          ProfileRec *__restrict__ rec, SetSolveParams P, ProfileSearchParams Q) {
    const ProfileItem it = items[blockIdx.x];
    const emsar::SetDesc d = desc[it.set];
    const int t = it.t;
    const double den_t = den_g[g_tid[d.tid_off + t]];
    const double sqrt_q = sqrt(Q.q);
    ProfileSearch S;
    S.start(it.side, it.theta_hat * den_t, Q.q);
    int evals = 0, passes = 0, solves_ok = 1, search_ok = 0, infeasible = 0;
    double x_t = it.theta_hat, dev = 0.0, s = 1.0, F = it.F_hat;
    for (;;) {
        s = exp(S.z);
        SetSolved K;
        solve_one_set<THREADS, true>(d, g_tid, g_u, row_w, rp_g, ent_g, cp_g, crow_g, den_g, nullptr, nullptr, P, t, &K, s);
        const SetLds &L = K.L;
        const double *x = K.res;
        set_sync<THREADS>();
        double s3[3] = {0.0, 0.0, 0.0};        // sum R log S + u log x, sum x den (t at its original den), infeasible
        set_objective_terms<THREADS>(L, x, s3, [&](int i) { return i == t ? den_t : L.den[i]; }, [](int, double, double) {});
        const double xt_now = x[t];
        set_reduce_sum<THREADS, 3>(s3, L.red);
        set_sync<THREADS>();                   // the next solve_one_set overwrites the LDS this epilogue read
        evals++;
        passes += K.passes;
        solves_ok &= K.converged;
        infeasible += (int)s3[2];
        x_t = xt_now;
        F = profile_uniform(s3[0] - s3[1]);
        const double raw = 2.0 * (it.F_hat - F);
        dev = raw > 0.0 ? raw : 0.0;
        if (!(raw == raw)) break;                                      // a non-finite likelihood: reported unconverged
        if (fabs(dev - Q.q) <= Q.dev_tol * Q.q) { search_ok = 1; break; }
        if (evals >= Q.max_evals) break;
        S.update(sqrt(dev) - sqrt_q);
    }
    if (threadIdx.x == 0) {
        ProfileRec r;
        r.x = x_t; r.dev = dev; r.s = s; r.F = F;
        r.evals = evals; r.passes = passes; r.flags = (search_ok ? PROFILE_REC_SEARCH_OK : 0) | (solves_ok ? PROFILE_REC_SOLVES_OK : 0);
        r.infeasible = infeasible;
        rec[blockIdx.x] = r;
    }
}
const auto kProfileSets = set_kernels(k_profile_sets<64>, k_profile_sets<256>, k_profile_sets<512>);

}  // namespace
