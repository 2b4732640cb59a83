// kernels_profile_usage.hpp -- k_profile_usage_base, k_profile_usage_sets: the profile-likelihood interval of one transcript's share of
// its gene (emsar_hip_profile_usage; driver: profile_usage.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_compare_usage.hpp (UsagePoint, UsageInner, UsageLeft, UsageDenEdit) and
// kernels_profile_genes.hpp (UsageDropEdit)

namespace {

// One sample.  Members, parts, X, F and mn are those of kernels_compare_usage.hpp for one sample; usage = theta_hat_t / X_hat at
// lambda = 0.  D(u) = 2 (F_hat - P(u)), P(u) = max {F : theta_t = u X}: one point of the curve is one inner multiplier search at fixed u
// (UsageInner / UsagePoint, the functors of the two-sample test, stopped by the bracket rule alone: below), its value the dual value
// UsageLeft::value(u) >= P(u) -- so the D reported is a lower bound of the true one, the error of second order in the gap the inner
// search leaves --, its slope dD/du = -2 lambda Xc (UsageLeft::slope).  A limit is the root of D(u) = q on one side of usage.
//
// Two families, as for the gene total (kernels_profile_genes.hpp): a search item needs theta_hat_t, X_hat, F_hat and the deviance at
// the end of its side, so the baselines and the drops run in an earlier launch.

// One (gene, t): the gene's slices of the lists, t by its library tid and by its place among the closed-form parts (-1: t lies in a
// set part), den_t and mn = the smallest den of the other members taking part.  skip: bit 0 = the host has decided the drop of t
// (t has reads only it explains), bit 1 = the drop of the others (one of them has)
struct ProfileUsageBaseItem { int32_t part_off, n_parts, closed_off, n_closed, gene, t, tc, skip; double den_t, mn; };
// t0, X0, F0: theta_t, the gene sum and F with every den its own; F_drop_t / F_drop_o: F with den_t / with the den of every other member
// taken as 0 in LDS; infeasible_*: rows and folded counts with reads that nothing explains in those solves
struct ProfileUsageBaseRec { double t0, X0, F0, F_drop_t, F_drop_o; int32_t infeasible_t, infeasible_o, passes, converged; };
// One limit of one (gene, t).  side 0 = lower (u in (0, usage)), 1 = upper (u in (usage, 1)); t0, X0, F0 are the baseline record's;
// D_end = the deviance at the end of the side (lambda_zero, lambda_one; > q, +inf allowed)
struct ProfileUsageItem { int32_t part_off, n_parts, closed_off, n_closed, gene, t, tc, side; double den_t, mn, t0, X0, F0, D_end; };
// What a search leaves: u, D and dD/du of the last outer point; outer points, inner evaluations and passes summed; flags as UsageRec's
struct ProfileUsageRec { double u, dev, slope; int32_t outer, evals, passes, flags, infeasible, reserved0; };
static_assert(sizeof(ProfileUsageBaseItem) == 48, "ProfileUsageBaseItem is written by the host as 48 bytes");
static_assert(sizeof(ProfileUsageBaseRec) == 56, "ProfileUsageBaseRec is read by the host as 56 bytes");
static_assert(sizeof(ProfileUsageItem) == 80, "ProfileUsageItem is written by the host as 80 bytes");
static_assert(sizeof(ProfileUsageRec) == 48, "ProfileUsageRec is read by the host as 48 bytes");
enum { PROFILE_USAGE_SKIP_T = 1, PROFILE_USAGE_SKIP_OTHERS = 2 };

struct ProfileUsageSearchParams { double q, dev_tol; int32_t max_evals, max_outer; };
// The inner searches stop when 2 |g| * (the width of their bracket in lambda) <= kProfileUsageInner * dev_tol * q: a quarter of what the
// outer rule allows.  The root lies in the bracket and the dual is convex with slope -g, so this bounds the error of the dual value.
// UsageInner's other rule, 2 |lambda g| <= tolerance, is turned off: next to usage the first multiplier tried is small, and the product
// would end the search there while the root lies at the end of the range (a sibling without reads of its own)
constexpr double kProfileUsageInner = 0.25;

// The root search of one limit in the coordinate u itself, on h(u) = sqrt(D(u)) - sqrt(q) (D is close to quadratic next to usage, so
// sqrt(D) is close to linear there).  It never leaves a bracket whose ends have known signs: h = -sqrt(q) at usage, and
// sqrt(D_end) - sqrt(q) > 0 (or +inf) at the end of the side, both known without an evaluation.
//   first point   the Poisson guess of the transcript profile for t's own expected reads n = usage * c, c = den_t X_hat (t alone, every
//                 read it takes unambiguously its own: an upper bound of the information, so the step is short rather than long):
//                 u = usage - sqrt(q usage / c) below, usage + sqrt(q usage / c) + q / (2 c) above (q / (2 c) is the whole step where
//                 usage is 0); the midpoint of the bracket where that falls outside it
//   later points  a Newton step on h with the known slope, h' = D' / (2 sqrt(D)), where D > 0, the slope has the sign of the side and
//                 the step falls strictly inside the bracket; else, while no point beyond the root has been seen, twice the distance
//                 from usage; else the Illinois step of the bracket (a bisection while the far end is +inf)
//   stop          |D - q| <= dev_tol q;  or the larger |dD/du| of the bracket's two ends times its width <= dev_tol q (the bracket can
//                 no longer move D by that much; the end at usage has slope 0, an end not yet evaluated +inf);  or after max_outer
//                 points, or at a non-finite value: unconverged
// The same code runs in the kernel (every value it sees is the same in all threads) and on the host (closed-form genes).
struct ProfileUsageOuter {
    IllinoisBracket B;                   // in u: p_lo on the side of usage (h < 0), p_hi on the side of the end (h > 0)
    double u, dev, slope;                // the point under way; D and dD/du of the last point
    double usage, sqrt_q, s_lo, s_hi;    // |dD/du| at the two ends
    int side, outer, ok;

    __host__ __device__ bool inside(double p) const { return side ? (p > B.p_lo && p < B.p_hi) : (p < B.p_lo && p > B.p_hi); }
    __host__ __device__ void start(int side_, double usage_, double c, double D_end, const ProfileUsageSearchParams &Q) {
        side = side_; usage = usage_; sqrt_q = sqrt(Q.q);
        outer = 0; ok = 0; dev = 0.0; slope = 0.0; s_lo = 0.0; s_hi = INFINITY;
        B.p_lo = usage; B.h_lo = -sqrt_q; B.p_hi = side ? 1.0 : 0.0; B.h_hi = sqrt(D_end) - sqrt_q; B.kept = 0;
        const double root = sqrt(Q.q * usage / c);
        const double first = side ? usage + root + Q.q / (2.0 * c) : usage - root;
        u = inside(first) ? first : B.p_lo + 0.5 * (B.p_hi - B.p_lo);
    }
    // after the inner search at u: what it left.  true = another point, at the new u
    __host__ __device__ bool step(const UsageLeft &L, double F_hat, const ProfileUsageSearchParams &Q) {
        outer++;
        const double raw = 2.0 * (F_hat - L.value(u));
        dev = raw > 0.0 ? raw : 0.0;
        slope = -2.0 * L.slope();
        if (!(raw - raw == 0.0) || !(slope - slope == 0.0)) return false;            // a non-finite value: reported unconverged
        if (fabs(dev - Q.q) <= Q.dev_tol * Q.q) { ok = 1; return false; }
        const double h = sqrt(dev) - sqrt_q;
        const bool below = h < 0.0;
        B.replace(below, u, h);
        if (below) s_lo = fabs(slope); else s_hi = fabs(slope);
        if ((s_lo > s_hi ? s_lo : s_hi) * fabs(B.p_hi - B.p_lo) <= Q.dev_tol * Q.q) { ok = 1; return false; }
        if (outer >= Q.max_outer) return false;
        double un = u - 2.0 * h * sqrt(dev) / slope;
        if (!(dev > 0.0 && (side ? slope > 0.0 : slope < 0.0) && inside(un))) {
            un = u + (u - usage);
            if (!(below && s_hi == INFINITY && inside(un))) un = B.next();
        }
        u = un;
        return true;
    }
};

// The whole search of one limit, both levels, driven by k_profile_usage_sets and by the host (genes whose parts are all closed form):
// eval(pt, S) adds the sample at pt into S
struct ProfileUsageSearched {
    ProfileUsageOuter O;
    int evals, inner_ok;                 // inner evaluations summed; every inner search met its stopping rule
    __host__ __device__ ProfileUsageRec record(const GeneSolveCount &C) const {
        ProfileUsageRec r;
        r.u = O.u; r.dev = O.dev; r.slope = O.slope;
        r.outer = O.outer; r.evals = evals; r.passes = C.passes;
        r.flags = (O.ok ? USAGE_REC_OUTER_OK : 0) | (C.solves_ok ? USAGE_REC_SOLVES_OK : 0) | (inner_ok ? USAGE_REC_INNER_OK : 0);
        r.infeasible = C.infeasible; r.reserved0 = 0;
        return r;
    }
};
template <class Eval>
__host__ __device__ __forceinline__ ProfileUsageSearched profile_usage_search(int side, double t0, double X0, double F0, double den_t, double mn,
                                                                              double D_end, const ProfileUsageSearchParams &Q, const Eval &eval) {
    ProfileUsageSearched R;
    ProfileUsageOuter &O = R.O;
    O.start(side, t0 / X0, den_t * X0, D_end, Q);
    R.evals = 0; R.inner_ok = 1;
    const UsageSearchParams Qi{kProfileUsageInner * Q.dev_tol * Q.q, Q.max_evals, 0};
    UsageLeft L{0.0, 0.0, 0.0, 0.0, 0.0};
    do {
        UsageInner J;
        bool more = J.start(false, O.u, t0, X0, F0, den_t, mn);
        while (more) {
            GeneSums S{0.0, 0.0, 0.0};
            eval(J.pt, S);
            more = J.step(false, S.T, S.X, S.F, O.u, den_t, mn, Qi, false);
        }
        R.evals += J.evals;
        R.inner_ok &= J.ok;
        L = J.left(O.u);
    } while (O.step(L, F0, Q));
    return R;
}

// Workgroup x runs (gene, t) x: the sample at lambda = 0 (eval_gene_side with UsageDenEdit and UsageTally: the code path of every
// evaluation of the searches, every den exactly its own), then -- unless the host has decided them -- every part without t, and every
// part without the other members (UsageDropEdit; F with the den that lies in LDS).  The closed-form parts stand in all three sums with
// their own den: one that a drop takes out has no reads (else the host has decided that drop) and adds 0 either way.  A record is a
// pure function of (item, its slices of the lists, P).  The launch has the thread count of the largest class among the item's set parts
// and the LDS of that class and every smaller one.  Every branch is taken by the whole workgroup, as the comment at eval_gene_side
// requires: the kernel branches on the item's fields alone.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_profile_usage_base(const ProfileUsageBaseItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                                const CompareGeneClosed *__restrict__ closed, CompareSide G,
                                                                const int32_t *__restrict__ gene_of, ProfileUsageBaseRec *__restrict__ rec,
                                                                SetSolveParams P) {
    const ProfileUsageBaseItem it = items[blockIdx.x];
    const GenePoint own{it.mn, 1.0, 0.0, it.tc, it.den_t};
    GeneSums S{0.0, 0.0, 0.0}, DT{0.0, 0.0, 0.0}, DO{0.0, 0.0, 0.0};
    GeneSolveCount C, CT, CO;
    eval_gene_side<THREADS, true, UsageTally>(G, parts + it.part_off, it.n_parts, closed + it.closed_off, it.n_closed, own, P,
                                              UsageDenEdit{gene_of, it.gene, it.t, it.den_t, it.mn, 1.0, 0.0}, S, C);
    if (!(it.skip & PROFILE_USAGE_SKIP_T))
        eval_gene_side<THREADS, false, NoTally>(G, parts + it.part_off, it.n_parts, closed + it.closed_off, it.n_closed, own, P,
                                                UsageDropEdit{gene_of, it.gene, it.t, false}, DT, CT);
    if (!(it.skip & PROFILE_USAGE_SKIP_OTHERS))
        eval_gene_side<THREADS, false, NoTally>(G, parts + it.part_off, it.n_parts, closed + it.closed_off, it.n_closed, own, P,
                                                UsageDropEdit{gene_of, it.gene, it.t, true}, DO, CO);
    if (threadIdx.x == 0)
        rec[blockIdx.x] = ProfileUsageBaseRec{S.T, S.X, S.F, DT.F, DO.F, CT.infeasible, CO.infeasible, C.passes + CT.passes + CO.passes,
                                              C.solves_ok & CT.solves_ok & CO.solves_ok};
}
const auto kProfileUsageBase = set_kernels(k_profile_usage_base<64>, k_profile_usage_base<256>, k_profile_usage_base<512>);

// Workgroup x runs the whole search of item x, both levels (profile_usage_search), one evaluation by eval_gene_side with theta_t riding
// on the reduction (UsageTally), so a record is a pure function of (item, its slices of the lists, P, Q).  Launch class and uniformity
// as k_compare_usage_sets.  The worst case is Q.max_outer * Q.max_evals * parts * P.max_iter passes, parts <= 64 (the driver's rule).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_profile_usage_sets(const ProfileUsageItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                                const CompareGeneClosed *__restrict__ closed, CompareSide G,
                                                                const int32_t *__restrict__ gene_of, ProfileUsageRec *__restrict__ rec,
                                                                SetSolveParams P, ProfileUsageSearchParams Q) {
    const ProfileUsageItem it = items[blockIdx.x];
    GeneSolveCount C;
    const ProfileUsageSearched R = profile_usage_search(it.side, it.t0, it.X0, it.F0, it.den_t, it.mn, it.D_end, Q, [&](const UsagePoint &pt, GeneSums &S) {
        eval_gene_side<THREADS, true, UsageTally>(G, parts + it.part_off, it.n_parts, closed + it.closed_off, it.n_closed,
                                                  GenePoint{it.mn, pt.scale, pt.shift, it.tc, pt.den_t}, P,
                                                  UsageDenEdit{gene_of, it.gene, it.t, pt.den_t, it.mn, pt.scale, pt.shift}, S, C);
    });
    if (threadIdx.x == 0) rec[blockIdx.x] = R.record(C);
}
const auto kProfileUsageSets = set_kernels(k_profile_usage_sets<64>, k_profile_usage_sets<256>, k_profile_usage_sets<512>);

}  // namespace
