// kernels_compare_groups.hpp -- k_compare_groups_sets: the common-value fit of one transcript across a subset of K samples, the building
// block of the K-sample test (emsar_hip_compare_groups; driver: compare_groups.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_compare.hpp

namespace {

// C(S) = max over x >= 0 of sum_{k in S} P_k(s_k x),  P_k(y) = max {F^k : theta_t^k = y}: the samples of S pooled inside the likelihood,
// s_k the size factors.  Two levels, as the usage test has them (kernels_compare_usage.hpp):
//   inner   one sample at a target y = s_k x > 0.  The dual D(lambda) = max [F - lambda (theta_t - y)] is the set problem with den_t + lambda
//           on t (solve_set_scaled) and F summed with the original den_t; g(lambda) = theta_t(lambda) - y falls in lambda, D is convex with
//           slope -g, D >= P_k(y) with equality at the root, and dP_k/dy = lambda there.  The side is the sign of theta_hat - y, which needs
//           no solve.  Where t must grow den' = den (1 - v), lambda = -v den; where it must shrink den' = den / (1 - v),
//           lambda = den v / (1 - v), unbounded, v -> 1 the drop solve.  CompareSearch runs on h = g / (theta_t + y) in v in [0, 1);
//           h(1) = -+1 is known without a solve.
//   outer   sum_k P_k(s_k x) is concave in x with slope Gs(x) = sum_k s_k lambda_k(x).  At x_lo = min_k theta_hat^k / s_k no sample has to
//           grow beyond its estimate, so every lambda_k >= 0 and Gs >= 0; at x_hi = max_k theta_hat^k / s_k every lambda_k <= 0: the signs
//           at the two ends are known without an evaluation.  Illinois steps on h = Gs / sum_k |s_k lambda_k| over (x_lo, x_hi); every
//           evaluated x lies strictly inside, so a target is never 0.
// Outer point 0 is lambda = 0 in every sample of S: theta_hat^k and F_hat^k come from the code path of every later evaluation.

// One unit of work: the transcript at position q of the locator table, the samples of `mask` (bit k = sample k).  row >= 0: the item
// writes theta_hat^k and F_hat^k of its samples to row `row` of the two [row][K] tables (the all-samples item of a transcript does).
struct GroupItem { int32_t q, row; uint32_t mask; int32_t reserved0; };
// where transcript q stands in sample k (table [q][K]): transcript t of set `set` of size class cls, or a one-transcript component
// (set -1) with u reads; den = den_t of that sample
struct GroupLoc { int32_t set, t, cls, reserved0; double u, den; };
// one sample (table [K]): its set records and its size factor
struct GroupSample { CompareSide side; double size; };
// What a search leaves: the largest sum of dual values among the outer points and its x (outer point 0: sum F_hat, and the first
// sample's theta_hat / s), F0 = sum F_hat in ascending sample order, the outer stopping quantity; outer points (point 0 included), inner
// evaluations and passes summed; flags: bit 0 = the outer search met its stopping rule, bit 1 = every solve converged, bit 2 = every
// inner search met its stopping rule
struct GroupRec { double best, best_x, slope, F0; int32_t outer, evals, passes, flags, infeasible, reserved0; };
static_assert(sizeof(GroupItem) == 16, "GroupItem is written by the host as 16 bytes");
static_assert(sizeof(GroupLoc) == 32, "GroupLoc is written by the host as 32 bytes");
static_assert(sizeof(GroupRec) == 56, "GroupRec is read by the host as 56 bytes");
enum { GROUP_REC_OUTER_OK = 1, GROUP_REC_SOLVES_OK = 2, GROUP_REC_INNER_OK = 4 };

struct GroupSearchParams { double dev_tol; int32_t max_evals, max_outer; };

// The multiplier search of one sample at one target y, driven by groups_search below: the caller evaluates the sample with den_t taken
// as scale * den_t and hands theta_t and F there to step(), until step() says stop.  Every argument is the same in all threads.
struct GroupInner {
    CompareSearch S;
    bool up;                             // t must shrink: the root lies at lambda > 0
    int evals, ok;                       // ok: a stopping rule was met
    double y, lambda, scale;             // the target; the point of the evaluation under way
    double root;                         // the multiplier at the root as the bracket's Illinois point estimates it: dP/dy for the outer search
    double th, F;                        // the last evaluation

    __host__ __device__ double lambda_at(double v, double den) const { return up ? den * v / (1.0 - v) : -(den * v); }
    __host__ __device__ void at(double v, double den) {
        scale = up ? 1.0 / (1.0 - v) : 1.0 - v;
        lambda = lambda_at(v, den);
    }
    // true = evaluate at scale.  first: outer point 0, lambda = 0.  Otherwise t0 = theta_hat of the sample: g(0) and h(0) need no solve;
    // a target that IS the estimate is evaluated at lambda = 0 once more and ends there
    __host__ __device__ bool start(bool first, double y_, double t0, double den) {
        y = y_; lambda = 0.0; scale = 1.0; root = 0.0; up = false; evals = 0; ok = 0; th = t0; F = 0.0;
        if (first) return true;
        const double g0 = t0 - y;
        if (g0 == 0.0) return true;
        up = g0 > 0.0;
        S.start(g0 / (t0 + y));
        at(S.v, den);
        return true;
    }
    // The stopping rules bound D(lambda) - P(y) by dev_tol / 2.  D is convex with slope -g and the root lies in the bracket:
    // D(lambda) - D(root) <= |g| |lambda - root|.  |lambda - root| <= |lambda| where the evaluation lies beyond the root (g has changed its
    // sign since lambda = 0): the product rule; <= the width of the bracket in lambda always: the bracket rule, which on the shrinking
    // side needs a finite upper end (v_hi < 1).  The dual value is taken at the last evaluation; the slope handed to the outer search is
    // the multiplier of the bracket's next Illinois point, whose error is of second order in the bracket where the last lambda's is of
    // first: the outer search divides by the sum of slopes that nearly cancel
    __host__ __device__ bool step(bool first, double th_, double F_, double den, const GroupSearchParams &Q) {
        th = th_; F = F_;
        evals++;
        if (first) { ok = 1; return false; }
        const double g = th - y;
        if (!(g - g == 0.0) || !(F - F == 0.0)) return false;                         // a non-finite value: reported unconverged
        root = lambda;
        if (lambda == 0.0 || g == 0.0) { ok = 1; return false; }
        S.update(g / (th + y));
        root = lambda_at(S.v, den);
        if ((g > 0.0) != up && 2.0 * fabs(lambda * g) <= Q.dev_tol) { ok = 1; return false; }
        const double lo = S.B.p_lo, hi = S.B.p_hi;
        if (!up || hi < 1.0) {
            const double width = up ? den * (hi / (1.0 - hi) - lo / (1.0 - lo)) : den * (hi - lo);
            if (2.0 * fabs(g) * width <= Q.dev_tol) { ok = 1; return false; }
        }
        if (evals >= Q.max_evals) return false;
        at(S.v, den);
        return true;
    }
    // the dual value at the last lambda, an upper bound of P(y); dP/dy = the multiplier at the root
    __host__ __device__ double value() const { return F - lambda * (th - y); }
};

// The search in x.  Outer point 0 is lambda = 0 in every sample; every later point is one inner search per sample.  At least one point
// of the null is evaluated whatever max_outer says.
struct GroupOuter {
    IllinoisBracket B;                   // in x: h_lo = +1 at x_lo, h_hi = -1 at x_hi
    double x;                            // the point under way
    int outer, ok, n0;                   // points evaluated, point 0 included; ok: a stopping rule was met; samples seen at point 0
    double x_lo, x_hi, x_first, F0;      // point 0: the range of theta_hat^k / s_k, the first sample's, sum F_hat
    double best, best_x, slope;

    __host__ __device__ void start() {
        x = 0.0; outer = 0; ok = 0; n0 = 0; x_lo = x_hi = x_first = F0 = best = best_x = slope = 0.0;
        B.p_lo = B.p_hi = B.h_lo = B.h_hi = 0.0; B.kept = 0;
    }
    // a sample of point 0: theta_hat^k / s_k and F_hat^k
    __host__ __device__ void first(double xk, double F) {
        if (n0 == 0) { x_lo = x_hi = x_first = xk; }
        else { x_lo = xk < x_lo ? xk : x_lo; x_hi = xk > x_hi ? xk : x_hi; }
        F0 += F; n0++;
    }
    // after every sample of the point: the sum of the dual values, Gs and sum |s_k lambda_k|.  true = another point, at the new x
    __host__ __device__ bool step(double val, double gs, double ab, const GroupSearchParams &Q) {
        outer++;
        if (outer == 1) {
            best = F0; best_x = x_first;
            if (!(F0 - F0 == 0.0) || !(x_hi - x_lo >= 0.0)) return false;            // a non-finite value at lambda = 0: the host's error
            if (x_lo == x_hi) { ok = 1; return false; }
            B.p_lo = x_lo; B.h_lo = 1.0; B.p_hi = x_hi; B.h_hi = -1.0; B.kept = 0;
            x = B.next();
            return true;
        }
        if (outer == 2 || val > best) { best = val; best_x = x; }
        if (!(gs - gs == 0.0) || !(val - val == 0.0)) return false;                   // a non-finite value: reported unconverged
        if (gs == 0.0) { slope = 0.0; ok = 1; return false; }
        const double h = gs / ab;
        B.replace(h > 0.0, x, h);
        slope = 2.0 * fabs(gs) * (B.p_hi - B.p_lo);
        if (slope <= Q.dev_tol) { ok = 1; return false; }
        if (outer >= Q.max_outer) return false;
        x = B.next();
        return true;
    }
};

struct GroupSearched {
    GroupOuter O;
    int evals, inner_ok;                 // inner evaluations summed; every inner search met its stopping rule
    __host__ __device__ GroupRec record(int passes, int solves_ok, int infeasible) const {
        GroupRec o;
        o.best = O.best; o.best_x = O.best_x; o.slope = O.slope; o.F0 = O.F0;
        o.outer = O.outer; o.evals = evals; o.passes = passes;
        o.flags = (O.ok ? GROUP_REC_OUTER_OK : 0) | (solves_ok ? GROUP_REC_SOLVES_OK : 0) | (inner_ok ? GROUP_REC_INNER_OK : 0);
        o.infeasible = infeasible; o.reserved0 = 0;
        return o;
    }
};
// The whole search of one item, both levels, driven by k_compare_groups_sets and by the host (transcripts that are closed form in every
// sample).  The samples of `mask` are visited in ascending index, so every sum has one order.  E gives the samples:
//   E.size(k), E.den(k)          s_k and den_t^k
//   E.eval(k, scale, lambda, x, F)   sample k with den_t taken as scale * den_t = den_t + lambda: theta_t and F there.  A transcript needs
//                                scale alone; the gene-level samples (kernels_compare_groups_genes.hpp) shift their other members by lambda
//   E.put_hat(k, x, F)           keeps theta_hat^k (and F_hat^k for the record) after point 0;  E.hat(k) gives theta_hat^k back
template <class Samples>
__host__ __device__ __forceinline__ GroupSearched groups_search(int K, uint32_t mask, const GroupSearchParams &Q, Samples &E) {
    GroupSearched R;
    GroupOuter &O = R.O;
    O.start();
    R.evals = 0; R.inner_ok = 1;
    double val, gs, ab;
    do {
        const bool first = O.outer == 0;
        val = 0.0; gs = 0.0; ab = 0.0;
#pragma nounroll
        for (int k = 0; k < K; k++) {
            if (!((mask >> k) & 1u)) continue;
            const double s = E.size(k), den = E.den(k);
            GroupInner J;
            bool more = J.start(first, s * O.x, first ? 0.0 : E.hat(k), den);
            while (more) {
                double x_t, F;
                E.eval(k, J.scale, J.lambda, x_t, F);
                more = J.step(first, x_t, F, den, Q);
            }
            R.evals += J.evals;
            R.inner_ok &= J.ok;
            if (first) { E.put_hat(k, J.th, J.F); O.first(J.th / s, J.F); }
            else { const double sl = s * J.root; val += J.value(); gs += sl; ab += fabs(sl); }
        }
    } while (O.step(val, gs, ab, Q));
    return R;
}

// The samples of an item as the kernel sees them.  The two tables are written by the host before the launch and never on the device: an
// item indexes them with a workgroup-uniform k, and the loads are the scalar unit's.  theta_hat^k lives in LDS behind the set's own
// arrays (lds_hat = smem + the launch's set bytes): thread 0 writes it after point 0, a barrier publishes it, and every thread reads it
// back from there -- no run-time-indexed local array, which would live in scratch, and no hand-over through global memory.
template <int THREADS>
struct GroupDeviceSamples {
    const GroupSample *__restrict__ samples;
    const GroupLoc *__restrict__ loc;    // the item's row of the locator table
    double *lds_hat;                     // [K] in LDS
    double *row_theta, *row_F;           // the item's rows of the [row][K] tables, null when it writes none
    SetSolveParams P;
    int passes, solves_ok, infeasible;

    __device__ double size(int k) const { return samples[k].size; }
    __device__ double den(int k) const { return loc[k].den; }
    __device__ double hat(int k) const { return set_uniform(lds_hat[k]); }
    __device__ void put_hat(int k, double x, double F) {
        if (threadIdx.x == 0) {
            lds_hat[k] = x;
            if (row_theta) { row_theta[k] = x; row_F[k] = F; }
        }
        __syncthreads();
    }
    __device__ void eval(int k, double scale, double /* lambda */, double &x_t, double &F) {
        const GroupLoc l = loc[k];
        if (l.set < 0) { compare_closed_form(l.u, l.den, scale, x_t, F); return; }
        const CompareSide G = samples[k].side;
        const ScaledSolve e = solve_set_scaled<THREADS>(side_desc(G, l.cls)[l.set], G.g_tid, G.g_u, G.row_w, G.rp, G.ent, G.cp, G.crow, G.den, P, l.t, l.den,
                                                        scale);
        passes += e.passes;
        solves_ok &= e.converged;
        infeasible += e.infeasible;
        x_t = set_uniform(e.x_t); F = e.F;
    }
};

// Workgroup x runs the whole two-level search of item x (groups_search).  One evaluation of a sample is solve_set_scaled
// (kernels_profile.hpp) in the same LDS, one sample after the other; solve_one_set reloads the set and restarts from the uniform point
// each time, and no inner bracket is carried from one outer point to the next, so a record is a pure function of (item, the tables, P,
// Q).  The launch has the thread count of the largest class among the item's sets; its LDS is hat_off bytes for the set (the largest
// any sample's sets of that class or a smaller one need) and K doubles behind them.
// Every branch is taken by the whole workgroup: it is decided on the item's fields, the tables' entries (uniform loads) and reduction
// results handed to the scalar unit (set_uniform); the strided loops, the reductions and the barrier of put_hat stand outside any
// branch that threads could take differently.
// The worst case is max(Q.max_outer, 2) * |S| * Q.max_evals * P.max_iter passes.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_compare_groups_sets(const GroupItem *__restrict__ items, const GroupSample *__restrict__ samples,
                                                                 const GroupLoc *__restrict__ locs, double *__restrict__ row_theta,
                                                                 double *__restrict__ row_F, GroupRec *__restrict__ rec, int K, uint32_t hat_off,
                                                                 SetSolveParams P, GroupSearchParams Q) {
    extern __shared__ double smem[];
    const GroupItem it = items[blockIdx.x];
    GroupDeviceSamples<THREADS> E{samples, locs + (size_t)it.q * (size_t)K, smem + hat_off / sizeof(double),
                                  it.row >= 0 ? row_theta + (size_t)it.row * (size_t)K : nullptr,
                                  it.row >= 0 ? row_F + (size_t)it.row * (size_t)K : nullptr, P, 0, 1, 0};
    const GroupSearched R = groups_search(K, it.mask, Q, E);
    if (threadIdx.x == 0) rec[blockIdx.x] = R.record(E.passes, E.solves_ok, E.infeasible);
}
const auto kCompareGroupsSets = set_kernels(k_compare_groups_sets<64>, k_compare_groups_sets<256>, k_compare_groups_sets<512>);

}  // namespace
