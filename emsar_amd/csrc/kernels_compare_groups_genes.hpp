// kernels_compare_groups_genes.hpp -- k_compare_groups_gene_sets: the common-value fit of one gene's sum across a subset of K samples,
// the building block of the gene-level K-sample test (emsar_hip_compare_groups_genes; driver: compare_groups_genes.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_gene_parts.hpp and kernels_compare_groups.hpp

namespace {

// C_g(S) = max over x >= 0 of sum_{k in S} P_k(s_k x),  P_k(y) = max {F^k : X^k = y}, X^k = the sum of theta over the members of g taking
// part in sample k, F^k summed over the gene's parts there.  The search is groups_search (kernels_compare_groups.hpp), unchanged, with
//   theta_t := X^k,   den_t := mn^k = the smallest den among the members taking part in sample k,
//   one evaluation := eval_gene_side (kernels_gene_parts.hpp) with the den of EVERY member taking part shifted in LDS: GroupInner's
//   (scale, lambda) are compare_gene_den's (scale, shift) -- growing: scale = 1 - v, lambda = -(v mn); shrinking: scale = 1 / (1 - v),
//   lambda = mn v / (1 - v) --, so the member(s) at mn take mn * scale and the others den + lambda, both positive in floating point.
// The dual value of a sample is F - lambda (X - y), F summed with the ORIGINAL den.  Outer point 0 is lambda = 0 in every sample of S:
// X_hat^k and F_hat^k come from the code path of every later evaluation.

// One unit of work: gene `gene` at row q of the locator table, the samples of `mask` (bit k = sample k).  row >= 0: the item writes
// X_hat^k and F_hat^k of its samples to row `row` of the two [row][K] tables (the all-samples item of a gene does).
struct GroupGeneItem { int32_t q, row; uint32_t mask; int32_t gene; };
// the gene's parts in sample k (table [q][K]): its slices of the part list and of the closed-form list, and mn^k
struct GroupGeneLoc { int32_t part_off, n_parts, closed_off, n_closed; double min_den; };
// one sample (table [K]): its set records, its size factor and its gene_of_lib (the map is one, each context indexes it by its own
// library numbering)
struct GroupGeneSample { CompareSide side; double size; const int32_t *gene_of_lib; };
static_assert(sizeof(GroupGeneItem) == 16, "GroupGeneItem is written by the host as 16 bytes");
static_assert(sizeof(GroupGeneLoc) == 24, "GroupGeneLoc is written by the host as 24 bytes");
// The record is k_compare_groups_sets' (GroupRec): x = the gene sums, F summed over the parts, passes over every part's solves.

// The samples of an item as the kernel sees them (the interface of groups_search).  The two tables and the part lists are written by
// the host before the launch and never on the device: an item indexes them with a workgroup-uniform k, and the loads are the scalar
// unit's.  X_hat^k lives in LDS behind the set's own arrays, as GroupDeviceSamples keeps theta_hat^k: thread 0 writes it after point 0,
// a barrier publishes it, every thread reads it back through set_uniform -- no run-time-indexed local array.
template <int THREADS>
struct GroupGeneDeviceSamples {
    const GroupGeneSample *__restrict__ samples;
    const GroupGeneLoc *__restrict__ loc;          // the item's row of the locator table
    const CompareGenePart *__restrict__ parts;
    const CompareGeneClosed *__restrict__ closed;
    double *lds_hat;                     // [K] in LDS
    double *row_X, *row_F;               // the item's rows of the [row][K] tables, null when it writes none
    SetSolveParams P;
    int32_t gene;
    GeneSolveCount C;

    __device__ double size(int k) const { return samples[k].size; }
    __device__ double den(int k) const { return loc[k].min_den; }
    __device__ double hat(int k) const { return set_uniform(lds_hat[k]); }
    __device__ void put_hat(int k, double x, double F) {
        if (threadIdx.x == 0) {
            lds_hat[k] = x;
            if (row_X) { row_X[k] = x; row_F[k] = F; }
        }
        __syncthreads();
    }
    __device__ void eval(int k, double scale, double lambda, double &x, double &F) {
        const GroupGeneLoc l = loc[k];
        GeneSums S{0.0, 0.0, 0.0};
        eval_gene_side<THREADS, true, GeneSumTally>(samples[k].side, parts + l.part_off, l.n_parts, closed + l.closed_off, l.n_closed,
                                                    GenePoint{l.min_den, scale, lambda, -1, 0.0}, P,
                                                    GeneDenEdit{samples[k].gene_of_lib, gene, l.min_den, scale, lambda}, S, C);
        x = set_uniform(S.X); F = set_uniform(S.F);
    }
};

// Workgroup x runs the whole two-level search of item x (groups_search), one evaluation of a sample by eval_gene_side: its set parts one
// after the other in the same LDS, then its closed-form parts in registers.  solve_one_set reloads the set and restarts from the
// uniform point each time and no inner bracket is carried from one outer point to the next, so a record is a pure function of (item,
// the tables, its slices of the lists, P, Q).  The launch has the thread count of the largest class among the set parts of the item's
// samples (class 0 where they have none); its LDS is hat_off bytes for the set (the largest any sample's sets of that class or a
// smaller one need) and K doubles behind them.
// Every branch is taken by the whole workgroup: it is decided on the item's fields, the tables' entries (uniform loads) and reduction
// results handed to the scalar unit (set_uniform); the strided loops, the reductions and the barrier of put_hat stand outside any
// branch that threads could take differently (eval_gene_side and k_compare_groups_sets keep the same rule).
// The worst case is max(Q.max_outer, 2) * |S| * Q.max_evals * 64 * P.max_iter passes: the driver admits at most 64 parts per sample.
// The three instances use no scratch (tools/kernel_regs.py lists registers and scratch per kernel).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_compare_groups_gene_sets(const GroupGeneItem *__restrict__ items, const GroupGeneSample *__restrict__ samples,
                                                                      const GroupGeneLoc *__restrict__ locs, const CompareGenePart *__restrict__ parts,
                                                                      const CompareGeneClosed *__restrict__ closed, double *__restrict__ row_X,
                                                                      double *__restrict__ row_F, GroupRec *__restrict__ rec, int K, uint32_t hat_off,
                                                                      SetSolveParams P, GroupSearchParams Q) {
    extern __shared__ double smem[];
    const GroupGeneItem it = items[blockIdx.x];
    GroupGeneDeviceSamples<THREADS> E{samples, locs + (size_t)it.q * (size_t)K, parts, closed, smem + hat_off / sizeof(double),
                                      it.row >= 0 ? row_X + (size_t)it.row * (size_t)K : nullptr,
                                      it.row >= 0 ? row_F + (size_t)it.row * (size_t)K : nullptr, P, it.gene, GeneSolveCount{}};
    const GroupSearched R = groups_search(K, it.mask, Q, E);
    if (threadIdx.x == 0) rec[blockIdx.x] = R.record(E.C.passes, E.C.solves_ok, E.C.infeasible);
}
const auto kCompareGroupsGeneSets = set_kernels(k_compare_groups_gene_sets<64>, k_compare_groups_gene_sets<256>, k_compare_groups_gene_sets<512>);

}  // namespace
