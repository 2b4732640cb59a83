// kernels_compare_genes.hpp -- k_compare_gene_sets: the two-sample likelihood-ratio test of one gene (emsar_hip_compare_genes; driver:
// compare_genes.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_gene_parts.hpp

namespace {

// The null  sum_{t in g} theta_t^A = r sum_{t in g} theta_t^B  has the dual  L(lambda) = max [F_A - lambda X_A] + max [F_B + r lambda X_B],
// X = the gene sum: the shift +lambda (A) or -r lambda (B) goes onto den of EVERY member of the gene, in every part of the gene in
// that sample (kernels_gene_parts.hpp).  One evaluation is a loop over the parts of both samples.

// One unit of work: the gene's slice of the part list (n_parts_a of A, then n_parts_b of B), its slice of the closed-form list
// (n_closed_a of A, then n_closed_b of B, each side by caller tid), the gene id (gene_of_lib of either context names it: the map is
// one, each context indexes it by its own library numbering) and the smallest den of the members taking part in each sample
struct CompareGeneItem { int32_t part_off, n_parts_a, n_parts_b, closed_off, n_closed_a, n_closed_b, gene, reserved0; double min_a, min_b; };
static_assert(sizeof(CompareGeneItem) == 48, "CompareGeneItem is written by the host as 48 bytes");
// The record is k_compare_sets' (CompareRec): x = the gene sums, F summed over the parts.

// The two shifts of the point T.pt (CompareStep driven with den_a := min_a, den_b := min_b): +lambda on A and -r lambda on B.  On the
// side that shrinks the shift is -(v * min) -- what ComparePoint makes lambda of, so pt.lambda itself when A shrinks, and
// r lambda = v * min_b up to rounding when B does: v * min_b <= min_b holds exactly, r * (v * (min_b / r)) need not.
__host__ __device__ inline void compare_gene_shifts(const CompareStep &T, double ratio, double min_b, double &shift_a, double &shift_b) {
    shift_a = T.pt.lambda;
    shift_b = T.up ? -(T.S.v * min_b) : -(ratio * T.pt.lambda);
}

// The search of one gene (CompareStep, unchanged: den_a := min_a, den_b := min_b, x := the gene sums, F summed over the parts), driven
// by k_compare_gene_sets and by the host (genes whose parts are all closed form): eval(b, pt, S) adds sample b (false = A) at pt into
// S.  Evaluation 0 is lambda = 0 (every den exactly its own): the gene sums and F1 come from the code path of every later evaluation.
template <class Eval>
__host__ __device__ __forceinline__ CompareStep compare_gene_search(double min_a, double min_b, const CompareSearchParams &Q, const Eval &eval) {
    CompareStep T;
    T.start();
    for (;;) {
        double shift_a, shift_b;
        compare_gene_shifts(T, Q.ratio, min_b, shift_a, shift_b);
        GeneSums A{0.0, 0.0, 0.0}, B{0.0, 0.0, 0.0};
#pragma nounroll
        for (int side = 0; side < 2; side++) {
            const bool b = side != 0;
            GeneSums S{0.0, 0.0, 0.0};
            eval(b, GenePoint{b ? min_b : min_a, b ? T.pt.scale_b : T.pt.scale_a, b ? shift_b : shift_a, -1, 0.0}, S);
            if (b) B = S; else A = S;
        }
        if (!T.step(A.X, A.F, B.X, B.F, min_a, min_b, Q)) break;
    }
    return T;
}

// Workgroup x runs the whole search of item x (compare_gene_search), one evaluation of a sample by eval_gene_side
// (kernels_gene_parts.hpp: the uniformity of every branch, the worst case per evaluation), so a record is a pure function of (item,
// its slices of the lists, P, Q).  The launch has the thread count of the largest class among the item's set parts and the LDS of that
// class and every smaller one, of both samples.
// The worst case is (n_parts_a + n_parts_b) * Q.max_evals * P.max_iter passes; the driver admits at most 64 parts per sample.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_compare_gene_sets(const CompareGeneItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                               const CompareGeneClosed *__restrict__ closed, CompareSide GA, CompareSide GB,
                                                               const int32_t *__restrict__ gene_of_a, const int32_t *__restrict__ gene_of_b,
                                                               CompareRec *__restrict__ rec, SetSolveParams P, CompareSearchParams Q) {
    const CompareGeneItem it = items[blockIdx.x];
    GeneSolveCount C;
    const CompareStep T = compare_gene_search(it.min_a, it.min_b, Q, [&](bool b, const GenePoint &pt, GeneSums &S) {
        const CompareSide &G = b ? GB : GA;
        eval_gene_side<THREADS, true, GeneSumTally>(G, parts + it.part_off + (b ? it.n_parts_a : 0), b ? it.n_parts_b : it.n_parts_a,
                                                    closed + it.closed_off + (b ? it.n_closed_a : 0), b ? it.n_closed_b : it.n_closed_a, pt, P,
                                                    GeneDenEdit{b ? gene_of_b : gene_of_a, it.gene, pt.mn, pt.scale, pt.shift}, S, C);
    });
    if (threadIdx.x == 0) rec[blockIdx.x] = T.record(C.passes, C.solves_ok, C.infeasible);
}
const auto kCompareGeneSets = set_kernels(k_compare_gene_sets<64>, k_compare_gene_sets<256>, k_compare_gene_sets<512>);

}  // namespace
