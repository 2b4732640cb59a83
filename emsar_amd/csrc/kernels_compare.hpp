// kernels_compare.hpp -- k_compare_sets: the two-sample likelihood-ratio test of one transcript (emsar_hip_compare; driver: compare.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_profile.hpp

namespace {

// One unit of work: transcript t_a of set set_a (size class cls_a) of sample A against t_b of set_b (cls_b) of sample B.  A side whose
// set is -1 is a one-transcript component: u reads on the transcript alone, x = u / den', F = u log x - x den.  den_a / den_b are
// den_t of the two samples (the bits the kernel would read from den).
struct CompareItem { int32_t set_a, t_a, cls_a, set_b, t_b, cls_b; double u_a, den_a, u_b, den_b; };
// What a search leaves: the multiplier of the last evaluation, the two values of t and the two F there (FA, FB: summed with the
// original den), the same at lambda = 0 (x0_a, x0_b, FhatA, FhatB), the solves spent per sample, the passes of both samples summed,
// and flags: bit 0 = the search met its stopping rule, bit 1 = every solve of it converged
struct CompareRec { double lambda_mult, x_a, x_b, x0_a, x0_b, FhatA, FhatB, FA, FB; int32_t evals, passes, flags, infeasible; };
static_assert(sizeof(CompareItem) == 56, "CompareItem is written by the host as 56 bytes");
static_assert(sizeof(CompareRec) == 88, "CompareRec is read by the host as 88 bytes");
enum { COMPARE_REC_SEARCH_OK = 1, COMPARE_REC_SOLVES_OK = 2 };

struct CompareSearchParams { double ratio, dev_tol; int32_t max_evals, reserved0; };

// the set records of one sample (SetsDev), as the kernel takes them
struct CompareSide {
    const emsar::SetDesc *desc0, *desc1, *desc2;     // by size class
    const int32_t *g_tid;
    const double *g_u, *row_w;
    const uint16_t *rp, *ent, *cp, *crow;
    const double *den;
};
// Its descriptors of size class cls.  The three pointers are read before the choice is made: G may be one of two kernel arguments picked
// at run time, and a choice among loads would turn into a load from a computed address, which keeps a copy of the arguments in scratch.
__device__ __forceinline__ const emsar::SetDesc *side_desc(const CompareSide &G, int cls) {
    const emsar::SetDesc *const d0 = G.desc0, *const d1 = G.desc1, *const d2 = G.desc2;
    return cls == 0 ? d0 : cls == 1 ? d1 : d2;
}

// The root search of the multiplier lambda = v * lambda_end on v in [0, 1), on h(v) = (x_A - r x_B) / (x_A + r x_B): h(0) comes from the
// evaluation at lambda = 0, h(1) = -sign h(0) is known without a solve (x_B -> inf or x_A -> inf at the end of the range).  Illinois
// steps on the bracket (IllinoisBracket, kernels_profile.hpp); an evaluation whose h has the sign of h_lo replaces the lo end.  The root
// lies in (v_lo, v_hi) at all times -- at v_hi = 1 itself when t has no read to its name on the side that would have to grow (x stays 0
// there whatever its den): the search then closes in on the end.  v names the point of the evaluation under way.
struct CompareSearch {
    IllinoisBracket B;                   // in v: h_lo has the sign of h(0), h_hi the other; v_lo < v_hi
    double v;

    __host__ __device__ void start(double h0) {
        B.p_lo = 0.0; B.h_lo = h0; B.p_hi = 1.0; B.h_hi = h0 > 0.0 ? -1.0 : 1.0; B.kept = 0;
        v = B.next();
    }
    __host__ __device__ void update(double h) { B.replace((h > 0.0) == (B.h_lo > 0.0), v, h); v = B.next(); }
};

// lambda_end and the two den scales of a point v of the search; up = the root lies at lambda > 0 (g(0) > 0)
struct ComparePoint {
    double lambda, scale_a, scale_b;
    __host__ __device__ static double end(bool up, double ratio, double den_a, double den_b) { return up ? den_b / ratio : den_a; }      // |lambda_end|
    __host__ __device__ void at(double v, bool up, double ratio, double den_a, double den_b) {
        if (up) { lambda = v * (den_b / ratio); scale_a = 1.0 + lambda / den_a; scale_b = 1.0 - v; }
        else { lambda = -(v * den_a); scale_a = 1.0 - v; scale_b = 1.0 - ratio * lambda / den_b; }
    }
};

// a one-transcript component at den' = scale * den: x = u / den', F = u log x - x den
__host__ __device__ inline void compare_closed_form(double u, double den, double scale, double &x, double &F) {
    x = u > 0.0 ? u / (den * scale) : 0.0;
    F = u > 0.0 ? u * log(x) - x * den : 0.0;
}

// One search and what its record needs, driven by k_compare_sets and by the host (compare_closed_pair, compare.hpp): the caller
// evaluates both samples at pt's scales and hands the two values of t and the two F there to step(), until step() says stop.  In the
// kernel every argument of step() is the same in all threads (the item's fields, reduction results made uniform): what it returns is a
// branch the whole workgroup takes.
struct CompareStep {
    CompareSearch S;
    ComparePoint pt;                     // the point of the evaluation under way; evaluation 0 is lambda = 0, both scales exactly 1
    bool up;
    int evals, search_ok;                // search_ok: a stopping rule was met; else a non-finite value or the cap ended it
    double x0_a, x0_b, F0_a, F0_b;       // at lambda = 0
    double x_a, x_b, F_a, F_b;           // the last evaluation

    __host__ __device__ void start() {
        pt.lambda = 0.0; pt.scale_a = 1.0; pt.scale_b = 1.0;
        up = false; evals = 0; search_ok = 0;
        x0_a = x0_b = F0_a = F0_b = x_a = x_b = F_a = F_b = 0.0;
    }
    // true = evaluate again, at the new pt
    __host__ __device__ bool step(double xa, double Fa, double xb, double Fb, double den_a, double den_b, const CompareSearchParams &Q) {
        const double r = Q.ratio;
        x_a = xa; F_a = Fa; x_b = xb; F_b = Fb;
        evals++;
        const double g = x_a - r * x_b;
        if (evals == 1) {
            x0_a = x_a; x0_b = x_b; F0_a = F_a; F0_b = F_b;
            if (!(F_a - F_a == 0.0) || !(F_b - F_b == 0.0)) return false;           // a non-finite likelihood at lambda = 0: the host's error
            if (g == 0.0) { search_ok = 1; return false; }
            up = g > 0.0;
        }
        if (!(g - g == 0.0) || !(F_a - F_a == 0.0) || !(F_b - F_b == 0.0)) return false;   // a non-finite value: reported unconverged
        if (evals > 1 && 2.0 * fabs(pt.lambda * g) <= Q.dev_tol) { search_ok = 1; return false; }
        const double h = g / (x_a + r * x_b);
        if (evals == 1) S.start(h); else S.update(h);
        // the root lies in the bracket and L is convex with slope -g: the dual value cannot fall further than |g| times the bracket
        if (2.0 * fabs(g) * ((S.B.p_hi - S.B.p_lo) * ComparePoint::end(up, r, den_a, den_b)) <= Q.dev_tol) { search_ok = 1; return false; }
        if (evals >= Q.max_evals) return false;
        pt.at(S.v, up, r, den_a, den_b);
        return true;
    }
    // the record; the host's closed-form pairs have no passes, no solve that could fail and nothing infeasible: (0, 1, 0)
    __host__ __device__ CompareRec record(int passes, int solves_ok, int infeasible) const {
        CompareRec o;
        o.lambda_mult = pt.lambda; o.x_a = x_a; o.x_b = x_b; o.x0_a = x0_a; o.x0_b = x0_b;
        o.FhatA = F0_a; o.FhatB = F0_b; o.FA = F_a; o.FB = F_b;
        o.evals = evals; o.passes = passes; o.flags = (search_ok ? COMPARE_REC_SEARCH_OK : 0) | (solves_ok ? COMPARE_REC_SOLVES_OK : 0);
        o.infeasible = infeasible;
        return o;
    }
};

// Workgroup x runs the whole search of item x (CompareStep).  One evaluation = the two samples one after the other in the same LDS:
// solve_set_scaled (kernels_profile.hpp) with den_t taken as scale * den_t (the maximiser of F_A - lambda theta_t, of
// F_B + r lambda theta_t) and F with the ORIGINAL den_t, exactly as k_profile_sets does; solve_one_set reloads the set and restarts
// from the uniform point each time, so a record is a pure function of (item, P, Q).  Evaluation 0 is lambda = 0 (both scales exactly
// 1): theta_hat and F_hat of both samples come from the code path of every later evaluation.  The launch has the thread count and the
// LDS of the larger of the two classes.
// Every branch is taken by the whole workgroup: it is decided on the item's fields and on reduction results handed to the scalar unit
// (set_uniform); the strided loops and the reductions stand outside any branch that threads could take differently.
// The worst case is 2 * Q.max_evals * P.max_iter passes.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_compare_sets(const CompareItem *__restrict__ items, CompareSide GA, CompareSide GB,
                                                          CompareRec *__restrict__ rec, SetSolveParams P, CompareSearchParams Q) {
    const CompareItem it = items[blockIdx.x];
    CompareStep T;
    T.start();
    int passes = 0, solves_ok = 1, infeasible = 0;
    for (;;) {
        double x_a = 0.0, F_a = 0.0, x_b = 0.0, F_b = 0.0;
#pragma nounroll
        for (int side = 0; side < 2; side++) {
            const bool b = side != 0;
            const int set = b ? it.set_b : it.set_a, t = b ? it.t_b : it.t_a, cls = b ? it.cls_b : it.cls_a;
            const double den_t = b ? it.den_b : it.den_a, scale = b ? T.pt.scale_b : T.pt.scale_a;
            double x_t, F;
            if (set < 0) compare_closed_form(b ? it.u_b : it.u_a, den_t, scale, x_t, F);
            else {
                const CompareSide &G = b ? GB : GA;
                const ScaledSolve e = solve_set_scaled<THREADS>(side_desc(G, cls)[set], G.g_tid, G.g_u, G.row_w, G.rp, G.ent, G.cp, G.crow, G.den, P, t,
                                                                den_t, scale);
                passes += e.passes;
                solves_ok &= e.converged;
                infeasible += e.infeasible;
                x_t = set_uniform(e.x_t); F = e.F;
            }
            if (b) { x_b = x_t; F_b = F; } else { x_a = x_t; F_a = F; }
        }
        if (!T.step(x_a, F_a, x_b, F_b, it.den_a, it.den_b, Q)) break;
    }
    if (threadIdx.x == 0) rec[blockIdx.x] = T.record(passes, solves_ok, infeasible);
}
const auto kCompareSets = set_kernels(k_compare_sets<64>, k_compare_sets<256>, k_compare_sets<512>);

}  // namespace
