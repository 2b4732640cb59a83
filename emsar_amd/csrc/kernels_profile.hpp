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

// A bracket (lo, hi) of a root in a coordinate p, h of opposite signs at its ends, and the Illinois step on it: regula falsi that
// halves the weight of an end it keeps twice, replaced by the midpoint when its point does not fall strictly inside the bracket.
// The searches decide by rules of their own which end an evaluation replaces (ProfileSearch, CompareSearch).
struct IllinoisBracket {
    double p_lo, h_lo, p_hi, h_hi;
    int kept;                            // +1 / -1 = the hi / lo end survived the last replace, 0 = none yet
    __host__ __device__ double next() const {
        const double w = p_hi - p_lo;
        const double pn = p_lo - h_lo * w / (h_hi - h_lo);
        const bool inside = w > 0.0 ? (pn > p_lo && pn < p_hi) : (pn < p_lo && pn > p_hi);
        return inside ? pn : p_lo + 0.5 * w;
    }
    // the evaluation at p gave h and takes the place of the lo end (lo_end) or of the hi end
    __host__ __device__ void replace(bool lo_end, double p, double h) {
        if (lo_end) {
            p_lo = p; h_lo = h;
            if (kept == 1) h_hi *= 0.5;
            kept = 1;
        } else {
            p_hi = p; h_hi = h;
            if (kept == -1) h_lo *= 0.5;
            kept = -1;
        }
    }
};

// The root search of one limit, in z = log s on h(z) = sqrt(dev) - sqrt(q); the same code runs in the kernel (every value it sees is
// the same in all threads of the workgroup) and on the host (one-transcript components).  h(0) = -sqrt(q) is known without a solve.
//   bracket   start at z0 = +-log(1 + sqrt(q / n_t)), n_t = theta_hat_t den_t; while h < 0 there, double z (s squares its distance from
//             1).  On the upper side with n_t < q -- theta_hat_t = 0 included: fewer expected reads than the cut, the Poisson guess says
//             nothing and would ask for a solve at s ~ sqrt(n_t / q), a problem scaled out of all proportion -- start at s = 1/2 and
//             quarter s instead
//   refine    Illinois steps on the bracket; an evaluation with h >= 0 replaces the hi end
// Every step is one evaluation: z names its point, update() takes its h and sets the next z.
struct ProfileSearch {
    IllinoisBracket B;                   // in z: h_lo < 0 <= h_hi once bracketed; |z_lo| < |z_hi|
    double z;                            // the point of the evaluation under way
    int bracketed;
    bool from_zero;

    __host__ __device__ void start(int side, double n_t, double q) {
        const double sgn = side == 0 ? 1.0 : -1.0;
        from_zero = side == 1 && !(n_t >= q);
        B.p_lo = 0.0; B.h_lo = -sqrt(q); B.p_hi = 0.0; B.h_hi = 0.0; B.kept = 0; bracketed = 0;
        z = from_zero ? -0.6931471805599453 : sgn * log1p(sqrt(q / n_t));
        clamp();
    }
    __host__ __device__ void clamp() { z = z > 690.0 ? 690.0 : z < -690.0 ? -690.0 : z; }
    __host__ __device__ void update(double h) {
        if (!bracketed) {
            if (h >= 0.0) { B.p_hi = z; B.h_hi = h; bracketed = 1; }                    // the first bracket: neither end has been kept yet
            else { B.p_lo = z; B.h_lo = h; z = from_zero ? z - 1.3862943611198906 : 2.0 * z; clamp(); return; }
        } else B.replace(!(h >= 0.0), z, h);
        z = B.next();
    }
};

// One search and what its record needs, driven by k_profile_sets and by the host (ProfileRun::closed_limit): the caller evaluates at
// the multiplier scale() and hands x_t and F there to step(), until step() says stop.  In the kernel every argument that steers step()
// is the same in all threads and scalar (the item's fields, F made uniform; x_t is only kept for the record): what it returns is a
// branch the whole workgroup takes.
struct ProfileStep {
    ProfileSearch S;
    int evals, search_ok;                // search_ok: the stopping rule was met; else a non-finite likelihood or the cap ended it
    double x, dev, s, F;                 // the last evaluation: theta_t, its deviance, its multiplier, its F

    __host__ __device__ void start(int side, double theta_hat, double den_t, double F_hat, const ProfileSearchParams &Q) {
        S.start(side, theta_hat * den_t, Q.q);
        evals = 0; search_ok = 0;
        x = theta_hat; dev = 0.0; s = 1.0; F = F_hat;
    }
    __host__ __device__ double scale() { return s = exp(S.z); }
    // true = evaluate again, at the new scale()
    __host__ __device__ bool step(double x_t, double F_now, double F_hat, double sqrt_q, const ProfileSearchParams &Q) {
        x = x_t; F = F_now;
        evals++;
        const double raw = 2.0 * (F_hat - F);
        dev = raw > 0.0 ? raw : 0.0;
        if (!(raw == raw)) return false;                               // a non-finite likelihood: reported unconverged
        if (fabs(dev - Q.q) <= Q.dev_tol * Q.q) { search_ok = 1; return false; }
        if (evals >= Q.max_evals) return false;
        S.update(sqrt(dev) - sqrt_q);
        return true;
    }
};

// One evaluation of the searches (k_profile_sets, k_compare_sets): the set solved with den_t taken as scale * den_t in LDS, then the
// presence epilogue's F with the ORIGINAL den_t.  F comes back through set_uniform: both kernels branch on it.  x_t is every thread's
// own read of the same LDS word and is left in a vector register: k_profile_sets only stores it, and k_compare_sets, which branches on
// it, makes it uniform itself (the bits are the same either way; scalar registers are the scarce ones in these kernels).  P travels by
// value as into solve_one_set: by reference hipcc keeps the kernel argument in other registers, and k_profile_sets ran 2 % longer.
struct ScaledSolve { double x_t, F; int passes, converged, infeasible; };
template <int THREADS>
__device__ __forceinline__ ScaledSolve solve_set_scaled(const emsar::SetDesc d, const int32_t *__restrict__ g_tid, const double *__restrict__ g_u,
                                                        const double *__restrict__ row_w, const uint16_t *__restrict__ rp_g,
                                                        const uint16_t *__restrict__ ent_g, const uint16_t *__restrict__ cp_g,
                                                        const uint16_t *__restrict__ crow_g, const double *__restrict__ den_g,
                                                        SetSolveParams P, int t, double den_t, double scale) {
    SetSolved K;
    solve_one_set<THREADS, true>(d, g_tid, g_u, row_w, rp_g, ent_g, cp_g, crow_g, den_g, nullptr, nullptr, P, t, &K, scale);
    const SetLds &L = K.L;
    const double *x = K.res;
    set_sync<THREADS>();
    double s3[3] = {0.0, 0.0, 0.0};        // sum R log S + u log x, sum x den (t at its original den), infeasible
    set_objective_terms<THREADS>(L, x, s3, [&](int i) { return i == t ? den_t : L.den[i]; }, [](int, double, double) {});
    const double xt_now = x[t];
    set_reduce_sum<THREADS, 3>(s3, L.red);
    set_sync<THREADS>();                   // the next solve_one_set overwrites the LDS this epilogue read
    return ScaledSolve{xt_now, set_uniform(s3[0] - s3[1]), K.passes, K.converged, (int)s3[2]};
}

// Workgroup x runs the whole search of item x: each evaluation is solve_set_scaled at s (the maximiser of F - lambda theta_t,
// lambda = (s - 1) den_t: the constrained maximum of F at theta_t = x_t(s)), dev = 2 (F_hat - F), and one step of ProfileSearch
// (ProfileStep).  solve_one_set reloads the set and restarts from the uniform point each time: a record is a pure function of
// (item, P, Q).  The worst case is Q.max_evals * P.max_iter passes.
// Every branch of the loop is taken by the whole workgroup: it is decided on the reductions' results alone (set_reduce_sum leaves every
// thread the same bits; set_uniform hands F to the scalar unit), the strided loops and the reductions stand outside any branch.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_profile_sets(const emsar::SetDesc *__restrict__ desc, const ProfileItem *__restrict__ items,
                                                          const int32_t *__restrict__ g_tid, const double *__restrict__ g_u,
                                                          const double *__restrict__ row_w, const uint16_t *__restrict__ rp_g,
                                                          const uint16_t *__restrict__ ent_g, const uint16_t *__restrict__ cp_g,
                                                          const uint16_t *__restrict__ crow_g, const double *__restrict__ den_g,
                                                          ProfileRec *__restrict__ rec, SetSolveParams P, ProfileSearchParams Q) {
    const ProfileItem it = items[blockIdx.x];
    const emsar::SetDesc d = desc[it.set];
    const double den_t = den_g[g_tid[d.tid_off + it.t]];
    const double sqrt_q = sqrt(Q.q);
    ProfileStep T;
    T.start(it.side, it.theta_hat, den_t, it.F_hat, Q);
    int passes = 0, solves_ok = 1, infeasible = 0;
    for (;;) {
        const ScaledSolve e = solve_set_scaled<THREADS>(d, g_tid, g_u, row_w, rp_g, ent_g, cp_g, crow_g, den_g, P, it.t, den_t, T.scale());
        passes += e.passes;
        solves_ok &= e.converged;
        infeasible += e.infeasible;
        if (!T.step(e.x_t, e.F, it.F_hat, sqrt_q, Q)) break;
    }
    if (threadIdx.x == 0) {
        ProfileRec r;
        r.x = T.x; r.dev = T.dev; r.s = T.s; r.F = T.F;
        r.evals = T.evals; r.passes = passes; r.flags = (T.search_ok ? PROFILE_REC_SEARCH_OK : 0) | (solves_ok ? PROFILE_REC_SOLVES_OK : 0);
        r.infeasible = infeasible;
        rec[blockIdx.x] = r;
    }
}
const auto kProfileSets = set_kernels(k_profile_sets<64>, k_profile_sets<256>, k_profile_sets<512>);

}  // namespace
