// kernels_compare_genes.hpp -- k_compare_gene_sets: the two-sample likelihood-ratio test of one gene (emsar_hip_compare_genes; driver:
// compare_genes.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_compare.hpp

namespace {

// The null  sum_{t in g} theta_t^A = r sum_{t in g} theta_t^B  has the dual  L(lambda) = max [F_A - lambda X_A] + max [F_B + r lambda X_B],
// X = the gene sum: the shift +lambda (A) or -r lambda (B) goes onto den of EVERY member of the gene, and the members of one sample may
// lie in several connected sets and one-transcript components -- the PARTS of the gene in that sample.  One evaluation is a loop over
// the parts of both samples; X and F are summed over them in the order of the lists below.

// A set part: packed set `set` of size class `cls` of sample `side` (0 = A, 1 = B) holds at least one member that takes part.  A
// gene's parts are A's then B's, each side by the smallest caller tid of the part's members.
struct CompareGenePart { int32_t side, set, cls, reserved0; };
// A closed-form part: a member that is a one-transcript component, u reads and den (the bits of the sample's den)
struct CompareGeneClosed { double u, den; };
// One unit of work: the gene's slice of the part list (n_parts_a of A, then n_parts_b of B), its slice of the closed-form list
// (n_closed_a of A, then n_closed_b of B, each side by caller tid), the gene id (gene_of_lib of either context names it: the map is
// one, each context indexes it by its own library numbering) and the smallest den of the members taking part in each sample
struct CompareGeneItem { int32_t part_off, n_parts_a, n_parts_b, closed_off, n_closed_a, n_closed_b, gene, reserved0; double min_a, min_b; };
static_assert(sizeof(CompareGenePart) == 16, "CompareGenePart is written by the host as 16 bytes");
static_assert(sizeof(CompareGeneClosed) == 16, "CompareGeneClosed is written by the host as 16 bytes");
static_assert(sizeof(CompareGeneItem) == 48, "CompareGeneItem is written by the host as 48 bytes");
// The record is k_compare_sets' (CompareRec): x = the gene sums, F summed over the parts.

// den of a member taking part (dn > 0) at a point of the search.  mn = the smallest such den of the sample, (scale, shift) = the side's
// values of compare_gene_shifts.  The member(s) at the minimum take mn * scale -- on the side that shrinks scale = 1 - v > 0, where
// mn - v * mn could round to 0 --, the others dn + shift, which stays above dn - mn >= 0 there.  At lambda = 0 (scale 1, shift 0)
// both are dn itself.
__host__ __device__ inline double compare_gene_den(double dn, double mn, double scale, double shift) { return dn == mn ? mn * scale : dn + shift; }

// The two shifts of the point T.pt (CompareStep driven with den_a := min_a, den_b := min_b): +lambda on A and -r lambda on B.  On the
// side that shrinks the shift is -(v * min) -- what ComparePoint makes lambda of, so pt.lambda itself when A shrinks, and
// r lambda = v * min_b up to rounding when B does: v * min_b <= min_b holds exactly, r * (v * (min_b / r)) need not.
__host__ __device__ inline void compare_gene_shifts(const CompareStep &T, double ratio, double min_b, double &shift_a, double &shift_b) {
    shift_a = T.pt.lambda;
    shift_b = T.up ? -(T.S.v * min_b) : -(ratio * T.pt.lambda);
}

// the closed-form parts of one side, summed in list order into X and F: x = u / den', F = u log x - x den
__host__ __device__ inline void compare_gene_closed_sum(const CompareGeneClosed *c, int n, double mn, double scale, double shift, double &X, double &F) {
    for (int k = 0; k < n; k++) {
        const double u = c[k].u, den = c[k].den;
        const double x = u > 0.0 ? u / compare_gene_den(den, mn, scale, shift) : 0.0;
        X += x;
        F += u > 0.0 ? u * log(x) - x * den : 0.0;
    }
}

// solve_one_set's den hook: every member of the gene that takes part gets its shifted den in LDS; membership of a local transcript is
// gene_of_lib[its library tid] == gene, so no member list and no LDS array is needed
struct GeneDenEdit {
    static constexpr bool kActive = true;
    const int32_t *gene_of;
    int32_t gene;
    double mn, scale, shift;
    __device__ double operator()(int32_t tid, double dn) const {
        return (dn > 0.0 && gene_of[tid] == gene) ? compare_gene_den(dn, mn, scale, shift) : dn;
    }
};

// One set part at one point: the set solved with the members' shifted den in LDS, then the presence epilogue's F with the ORIGINAL den
// of every transcript (den_g is read again: a member's original bits, anyone else's the bits that lie in LDS) and, from the same
// reduction, the part's share of the gene sum.  X and F come back through set_uniform: the kernel branches on them.
struct GenePartSolve { double X, F; int passes, converged, infeasible; };
template <int THREADS>
__device__ __forceinline__ GenePartSolve solve_gene_part(const emsar::SetDesc d, const int32_t *__restrict__ g_tid, const double *__restrict__ g_u,
                                                         const double *__restrict__ row_w, const uint16_t *__restrict__ rp_g,
                                                         const uint16_t *__restrict__ ent_g, const uint16_t *__restrict__ cp_g,
                                                         const uint16_t *__restrict__ crow_g, const double *__restrict__ den_g,
                                                         SetSolveParams P, const int32_t *__restrict__ gene_of, int32_t gene, double mn,
                                                         double scale, double shift) {
    SetSolved K;
    solve_one_set<THREADS, true, GeneDenEdit>(d, g_tid, g_u, row_w, rp_g, ent_g, cp_g, crow_g, den_g, nullptr, nullptr, P, -1, &K, 0.0,
                                              GeneDenEdit{gene_of, gene, mn, scale, shift});
    const SetLds &L = K.L;
    const double *x = K.res;
    set_sync<THREADS>();
    double s3[3] = {0.0, 0.0, 0.0};        // sum R log S + u log x, sum x den (original den), infeasible
    double xs = 0.0;                       // this thread's share of the members' sum
    set_objective_terms<THREADS>(L, x, s3, [&](int i) { return den_g[g_tid[d.tid_off + i]]; },
                                 [&](int i, double xi, double) { if (gene_of[g_tid[d.tid_off + i]] == gene) xs += xi; });
    double s4[4] = {s3[0], s3[1], s3[2], xs};
    set_reduce_sum<THREADS, 4>(s4, L.red);
    set_sync<THREADS>();                   // the next solve_one_set overwrites the LDS this epilogue read
    return GenePartSolve{set_uniform(s4[3]), set_uniform(s4[0] - s4[1]), K.passes, K.converged, (int)s4[2]};
}

// Workgroup x runs the whole search of item x (CompareStep, unchanged: den_a := min_a, den_b := min_b, x := the gene sums, F summed over
// the parts).  One evaluation = every set part of the item one after the other in the same LDS (solve_gene_part), A's then B's, then
// the closed-form parts in registers, by every thread alike.  solve_one_set reloads the set and restarts from the uniform point each
// time, so a record is a pure function of (item, its slices of the lists, P, Q).  Evaluation 0 is lambda = 0 (every den exactly its
// own): the gene sums and F1 come from the code path of every later evaluation.  The launch has the thread count of the largest class
// among the item's set parts and the LDS of that class and every smaller one, of both samples.
// Every branch is taken by the whole workgroup: the part fields come from the item list by scalar loads of an address no thread
// differs in, X and F go through set_uniform; the strided loops and the reductions stand outside any branch that threads could take
// differently.
// The worst case is (n_parts_a + n_parts_b) * Q.max_evals * P.max_iter passes; the driver admits at most 64 parts per sample.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_compare_gene_sets(const CompareGeneItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                               const CompareGeneClosed *__restrict__ closed, CompareSide GA, CompareSide GB,
                                                               const int32_t *__restrict__ gene_of_a, const int32_t *__restrict__ gene_of_b,
                                                               CompareRec *__restrict__ rec, SetSolveParams P, CompareSearchParams Q) {
    const CompareGeneItem it = items[blockIdx.x];
    const int n_parts = it.n_parts_a + it.n_parts_b;
    CompareStep T;
    T.start();
    int passes = 0, solves_ok = 1, infeasible = 0;
    for (;;) {
        double shift_a, shift_b;
        compare_gene_shifts(T, Q.ratio, it.min_b, shift_a, shift_b);
        double x_a = 0.0, F_a = 0.0, x_b = 0.0, F_b = 0.0;
#pragma nounroll
        for (int k = 0; k < n_parts; k++) {
            const CompareGenePart pt = parts[it.part_off + k];
            const bool b = pt.side != 0;
            const emsar::SetDesc *dp = pt.cls == 0 ? (b ? GB.desc0 : GA.desc0) : pt.cls == 1 ? (b ? GB.desc1 : GA.desc1) : (b ? GB.desc2 : GA.desc2);
            const GenePartSolve e = solve_gene_part<THREADS>(dp[pt.set], b ? GB.g_tid : GA.g_tid, b ? GB.g_u : GA.g_u, b ? GB.row_w : GA.row_w,
                                                             b ? GB.rp : GA.rp, b ? GB.ent : GA.ent, b ? GB.cp : GA.cp, b ? GB.crow : GA.crow,
                                                             b ? GB.den : GA.den, P, b ? gene_of_b : gene_of_a, it.gene, b ? it.min_b : it.min_a,
                                                             b ? T.pt.scale_b : T.pt.scale_a, b ? shift_b : shift_a);
            passes += e.passes;
            solves_ok &= e.converged;
            infeasible += e.infeasible;
            if (b) { x_b += e.X; F_b += e.F; } else { x_a += e.X; F_a += e.F; }
        }
        compare_gene_closed_sum(closed + it.closed_off, it.n_closed_a, it.min_a, T.pt.scale_a, shift_a, x_a, F_a);
        compare_gene_closed_sum(closed + it.closed_off + it.n_closed_a, it.n_closed_b, it.min_b, T.pt.scale_b, shift_b, x_b, F_b);
        if (!T.step(x_a, F_a, x_b, F_b, it.min_a, it.min_b, Q)) break;
    }
    if (threadIdx.x == 0) rec[blockIdx.x] = T.record(passes, solves_ok, infeasible);
}
const auto kCompareGeneSets = set_kernels(k_compare_gene_sets<64>, k_compare_gene_sets<256>, k_compare_gene_sets<512>);

}  // namespace
