// kernels_compare_usage.hpp -- k_compare_usage_sets: the two-sample test of one transcript's share of its gene (emsar_hip_compare_usage;
// driver: compare_usage.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_gene_parts.hpp

namespace {

// The null  theta_t^A / X^A = theta_t^B / X^B = u  (X = the gene sum, members and parts as kernels_gene_parts.hpp defines them) is not linear
// in theta, so the search has two levels.
//   inner   u fixed: the samples decouple, and in one sample the constraint theta_t - u X = 0 is linear.  Its dual
//           D(lambda) = max [F - lambda (theta_t - u X)] is the ordinary problem with den_t + lambda (1 - u) on t and den_s - lambda u on
//           every other member s taking part, lambda in (-den_t / (1 - u), mn / u), mn = the smallest den of the others.  The gap
//           g(lambda) = theta_t - u X falls in lambda, D is convex with slope -g, D >= P(u) = max {F : theta_t = u X} with equality at
//           the root.  CompareSearch runs on h = g / (theta_t + u X) in v in [0, 1), lambda = v * (the end of the range on the side of
//           sign g(0)); h at v = 1 is known without a solve.
//   outer   dP_k/du = lambda_k Xc^k (envelope theorem), Xc = the gene sum of the FEASIBLE point next to the inner search's last
//           evaluation (UsageLeft; X itself at a root): an Illinois search on s = lambda_A Xc^A + lambda_B Xc^B, normalised by the sum of
//           the two magnitudes, over the bracket of the two estimated shares, where its sign is known without an evaluation.
// Evaluation 0 is lambda = 0 in both samples: one "inner search" of one evaluation each, through the code of every later evaluation.

// One unit of work: transcript t of `gene`.  The gene's slice of the part list (CompareGenePart: n_parts_a of A, then n_parts_b of B)
// and of the closed-form list (CompareGeneClosed: n_closed_a of A, then n_closed_b of B, each side by caller tid); t by its library tid
// in each context (t_a, t_b) and, where t is a one-transcript component of a sample, its place in that side's closed-form slice (tc_a,
// tc_b; -1 = t lies in a set part); den_t and mn = the smallest den of the OTHER members taking part, per sample
struct UsageItem {
    int32_t part_off, n_parts_a, n_parts_b, closed_off, n_closed_a, n_closed_b, gene, t_a, t_b, tc_a, tc_b, reserved0;
    double den_ta, den_tb, mn_a, mn_b;
};
// What a search leaves: theta_t, X and F of both samples at lambda = 0; the largest P_A + P_B among the outer points and its u; the
// outer stopping quantity; outer points (evaluation 0 included), inner evaluations and passes summed; flags: bit 0 = the outer search
// met its stopping rule, bit 1 = every solve converged, bit 2 = every inner search met its stopping rule
struct UsageRec { double t0_a, X0_a, F0_a, t0_b, X0_b, F0_b, best, best_u, slope; int32_t outer, evals, passes, flags, infeasible, reserved0; };
static_assert(sizeof(UsageItem) == 80, "UsageItem is written by the host as 80 bytes");
static_assert(sizeof(UsageRec) == 96, "UsageRec is read by the host as 96 bytes");
enum { USAGE_REC_OUTER_OK = 1, USAGE_REC_SOLVES_OK = 2, USAGE_REC_INNER_OK = 4 };

struct UsageSearchParams { double dev_tol; int32_t max_evals, max_outer; };

// The den of one sample's members at a point of an inner search: t takes den_t, another member taking part compare_gene_den(dn, mn,
// scale, shift).  On the side that shrinks the member(s) at the limiting den take den * (1 - v) and the others den - v * (their share
// of the limit): both stay positive in floating point.  At lambda = 0 every den keeps its own bits.
struct UsagePoint {
    double lambda, den_t, scale, shift;
    __host__ __device__ void zero(double den_t0) { lambda = 0.0; den_t = den_t0; scale = 1.0; shift = 0.0; }
    // |lambda| at the end of the range
    __host__ __device__ static double end(bool up, double u, double den_t0, double mn) { return up ? mn / u : den_t0 / (1.0 - u); }
    __host__ __device__ void at(double v, bool up, double u, double den_t0, double mn) {
        if (up) {                        // the others shrink: mn -> mn (1 - v), t grows
            lambda = v * (mn / u); shift = -(v * mn); scale = 1.0 - v; den_t = den_t0 + lambda * (1.0 - u);
        } else {                         // t shrinks, the others grow
            lambda = -(v * (den_t0 / (1.0 - u))); den_t = den_t0 * (1.0 - v); shift = -(lambda * u); scale = 1.0 + shift / mn;
        }
    }
};

// The multiplier search of one sample at one share u, driven by usage_search below: the caller evaluates the sample at pt and
// hands theta_t, X and F there to step(), until step() says stop.  Every argument is the same in all threads of the workgroup.
struct UsageInner {
    CompareSearch S;
    UsagePoint pt;
    bool up;
    int evals, ok;                       // ok: a stopping rule was met
    double th, X, F;                     // the last evaluation

    // true = evaluate at pt.  first: evaluation 0, the point lambda = 0.  Otherwise (t0, X0, F0) is the sample at lambda = 0: g(0) and
    // h(0) need no solve
    __host__ __device__ bool start(bool first, double u, double t0, double X0, double F0, double den_t0, double mn) {
        pt.zero(den_t0);
        up = false; evals = 0; ok = 0;
        th = t0; X = X0; F = F0;
        if (first) return true;
        const double g0 = t0 - u * X0;
        if (g0 == 0.0) { ok = 1; return false; }
        up = g0 > 0.0;
        S.start(g0 / (t0 + u * X0));
        pt.at(S.v, up, u, den_t0, mn);
        return true;
    }
    // product_rule: stop at 2 |lambda g| <= dev_tol as well as by the bracket.  The product bounds the error of the dual value only
    // where lambda lies beyond the root; a search that must not stop short of it (the usage profile, whose first point lies next to
    // lambda = 0 while the root may be the end of the range) turns it off and keeps the bracket rule, which always bounds it
    __host__ __device__ bool step(bool first, double th_, double X_, double F_, double u, double den_t0, double mn, const UsageSearchParams &Q,
                                  bool product_rule = true) {
        th = th_; X = X_; F = F_;
        evals++;
        if (first) { ok = 1; return false; }
        const double g = th - u * X;
        if (!(g - g == 0.0) || !(F - F == 0.0)) return false;                         // a non-finite value: reported unconverged
        if (product_rule && 2.0 * fabs(pt.lambda * g) <= Q.dev_tol) { ok = 1; return false; }
        S.update(g / (th + u * X));
        if (2.0 * fabs(g) * ((S.B.p_hi - S.B.p_lo) * UsagePoint::end(up, u, den_t0, mn)) <= Q.dev_tol) { ok = 1; return false; }
        if (evals >= Q.max_evals) return false;
        pt.at(S.v, up, u, den_t0, mn);
        return true;
    }
    __host__ __device__ struct UsageLeft left(double u) const;
};
// What an inner search leaves the outer one: the last evaluation, its multiplier and Xc = the gene sum of the feasible point next to
// it.  At the root theta_t = u X and Xc = X.  Short of it the member that the multiplier makes cheaper is the one in deficit: t when t
// shrinks (theta_t < u X: filling t up to the constraint gives Xc = (X - theta_t) / (1 - u)), the others when they do (Xc = theta_t / u).
// The two agree with X at the root.  They differ from it where the root is the end of the range: the member in deficit has no read
// to its name and stays 0 at every evaluated point whatever its den, while at the end itself, where its den' is 0, its value is free
// and the constraint sets it.  dP/du = lambda X still holds there with the X of that constrained point; the X of any EVALUATED point
// lacks the member's share and would make the slope too small by the factor 1 - u (or u).
struct UsageLeft {
    double th, X, F, lambda, Xc;
    // the dual value at the last lambda, an upper bound of P(u), and the slope dP/du = lambda Xc
    __host__ __device__ double value(double u) const { return F - lambda * (th - u * X); }
    __host__ __device__ double slope() const { return lambda * Xc; }
};
__host__ __device__ inline UsageLeft UsageInner::left(double u) const {
    return UsageLeft{th, X, F, pt.lambda, pt.lambda == 0.0 ? X : up ? th / u : (X - th) / (1.0 - u)};
}

// The search in u.  Outer point 0 is evaluation 0; every later point is one inner search per sample.  At least one point of the null
// is evaluated whatever max_outer says.
struct UsageOuter {
    IllinoisBracket B;                   // in u: h_lo = +1 at the smaller estimated share, h_hi = -1 at the larger
    double u;                            // the point under way
    int outer, ok;                       // points evaluated, evaluation 0 included; ok: a stopping rule was met
    double t0_a, X0_a, F0_a, t0_b, X0_b, F0_b;     // evaluation 0
    double best, best_u, slope;

    __host__ __device__ void start() {
        u = 0.0; outer = 0; ok = 0; best = 0.0; best_u = 0.0; slope = 0.0;
        t0_a = t0_b = X0_a = X0_b = F0_a = F0_b = 0.0;
        B.p_lo = B.p_hi = B.h_lo = B.h_hi = 0.0; B.kept = 0;
    }
    // after both samples of the point: what their inner searches left.  true = another point, at the new u
    __host__ __device__ bool step(const UsageLeft &A, const UsageLeft &Bs, const UsageSearchParams &Q) {
        outer++;
        if (outer == 1) {
            t0_a = A.th; X0_a = A.X; F0_a = A.F; t0_b = Bs.th; X0_b = Bs.X; F0_b = Bs.F;
            best = A.F + Bs.F;
            if (!(best - best == 0.0)) return false;                                  // a non-finite likelihood at lambda = 0: the host's error
            if (!(X0_a > 0.0) || !(X0_b > 0.0)) return false;                         // no share to speak of: the host's status
            const double ua = t0_a / X0_a, ub = t0_b / X0_b;
            best_u = ua;
            if (ua == ub) { ok = 1; return false; }
            B.p_lo = ua < ub ? ua : ub; B.h_lo = 1.0; B.p_hi = ua < ub ? ub : ua; B.h_hi = -1.0; B.kept = 0;
            u = B.next();
            return true;
        }
        const double val = A.value(u) + Bs.value(u), sa = A.slope(), sb = Bs.slope(), s = sa + sb;
        if (outer == 2 || val > best) { best = val; best_u = u; }
        if (!(s - s == 0.0) || !(val - val == 0.0)) return false;                     // a non-finite value: reported unconverged
        if (s == 0.0) { slope = 0.0; ok = 1; return false; }
        const double h = s / (fabs(sa) + fabs(sb));
        B.replace(h > 0.0, u, h);
        slope = 2.0 * fabs(s) * (B.p_hi - B.p_lo);
        if (slope <= Q.dev_tol) { ok = 1; return false; }
        if (outer >= Q.max_outer) return false;
        u = B.next();
        return true;
    }
    __host__ __device__ UsageRec record(int evals, int passes, int solves_ok, int inner_ok, int infeasible) const {
        UsageRec o;
        o.t0_a = t0_a; o.X0_a = X0_a; o.F0_a = F0_a; o.t0_b = t0_b; o.X0_b = X0_b; o.F0_b = F0_b;
        o.best = best; o.best_u = best_u; o.slope = slope;
        o.outer = outer; o.evals = evals; o.passes = passes;
        o.flags = (ok ? USAGE_REC_OUTER_OK : 0) | (solves_ok ? USAGE_REC_SOLVES_OK : 0) | (inner_ok ? USAGE_REC_INNER_OK : 0);
        o.infeasible = infeasible; o.reserved0 = 0;
        return o;
    }
};

// The whole search of one transcript, both levels, driven by k_compare_usage_sets and by the host (genes whose parts are all closed
// form): eval(b, pt, S) adds sample b (false = A) at pt into S.  tc_a, tc_b: t's place in each side's closed-form slice (-1: none).
struct UsageSearched {
    UsageOuter O;
    int evals, inner_ok;                 // inner evaluations summed; every inner search met its stopping rule
    __host__ __device__ UsageRec record(const GeneSolveCount &C) const { return O.record(evals, C.passes, C.solves_ok, inner_ok, C.infeasible); }
};
template <class Eval>
__host__ __device__ __forceinline__ UsageSearched usage_search(double den_ta, double mn_a, int tc_a, double den_tb, double mn_b, int tc_b,
                                                               const UsageSearchParams &Q, const Eval &eval) {
    UsageSearched R;
    UsageOuter &O = R.O;
    O.start();
    R.evals = 0; R.inner_ok = 1;
    UsageLeft LA{0.0, 0.0, 0.0, 0.0, 0.0}, LB{0.0, 0.0, 0.0, 0.0, 0.0};
    do {
        const bool first = O.outer == 0;
#pragma nounroll
        for (int side = 0; side < 2; side++) {
            const bool b = side != 0;
            const double den_t0 = b ? den_tb : den_ta, mn = b ? mn_b : mn_a;
            UsageInner J;
            bool more = J.start(first, O.u, b ? O.t0_b : O.t0_a, b ? O.X0_b : O.X0_a, b ? O.F0_b : O.F0_a, den_t0, mn);
            while (more) {
                GeneSums S{0.0, 0.0, 0.0};
                eval(b, GenePoint{mn, J.pt.scale, J.pt.shift, b ? tc_b : tc_a, J.pt.den_t}, S);
                more = J.step(first, S.T, S.X, S.F, O.u, den_t0, mn, Q);
            }
            R.evals += J.evals;
            R.inner_ok &= J.ok;
            if (b) LB = J.left(O.u); else LA = J.left(O.u);
        }
    } while (O.step(LA, LB, Q));
    return R;
}

// solve_one_set's den hook: t (by its library tid) takes den_t of the point, every other member of the gene that takes part its
// shifted den; membership is gene_of_lib[library tid] == gene, so no member list and no LDS array is needed
struct UsageDenEdit {
    static constexpr bool kActive = true;
    const int32_t *gene_of;
    int32_t gene, t;
    double den_t, mn, scale, shift;
    __device__ double operator()(int32_t tid, double dn) const {
        if (!(dn > 0.0) || gene_of[tid] != gene) return dn;
        return tid == t ? den_t : compare_gene_den(dn, mn, scale, shift);
    }
};

// Workgroup x runs the whole search of item x, both levels (usage_search), one evaluation of a sample by eval_gene_side
// (kernels_gene_parts.hpp: the uniformity of every branch, the worst case per evaluation) with theta_t riding on the reduction
// (UsageTally), so a record is a pure function of (item, its slices of the lists, P, Q).  The launch has the thread count of the largest
// class among the item's set parts and the LDS of that class and every smaller one, of both samples.
// The worst case is max(Q.max_outer, 2) * 2 * Q.max_evals * parts * P.max_iter passes, parts <= 64 per sample (the driver's rule).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_compare_usage_sets(const UsageItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                                const CompareGeneClosed *__restrict__ closed, CompareSide GA, CompareSide GB,
                                                                const int32_t *__restrict__ gene_of_a, const int32_t *__restrict__ gene_of_b,
                                                                UsageRec *__restrict__ rec, SetSolveParams P, UsageSearchParams Q) {
    const UsageItem it = items[blockIdx.x];
    GeneSolveCount C;
    const UsageSearched R = usage_search(it.den_ta, it.mn_a, it.tc_a, it.den_tb, it.mn_b, it.tc_b, Q, [&](bool b, const GenePoint &pt, GeneSums &S) {
        const CompareSide &G = b ? GB : GA;
        eval_gene_side<THREADS, true, UsageTally>(G, parts + it.part_off + (b ? it.n_parts_a : 0), b ? it.n_parts_b : it.n_parts_a,
                                                  closed + it.closed_off + (b ? it.n_closed_a : 0), b ? it.n_closed_b : it.n_closed_a, pt, P,
                                                  UsageDenEdit{b ? gene_of_b : gene_of_a, it.gene, b ? it.t_b : it.t_a, pt.den_t, pt.mn, pt.scale,
                                                               pt.shift}, S, C);
    });
    if (threadIdx.x == 0) rec[blockIdx.x] = R.record(C);
}
const auto kCompareUsageSets = set_kernels(k_compare_usage_sets<64>, k_compare_usage_sets<256>, k_compare_usage_sets<512>);

}  // namespace

