// kernels_gene_parts.hpp -- what the gene-level set kernels share (kernels_compare_genes.hpp, kernels_profile_genes.hpp,
// kernels_compare_usage.hpp; host half: gene_parts.hpp): the part lists, the den of a member at a point of a search, the solve of one
// set part and the evaluation of one sample
#pragma once
// included by emsar_hip.hip only, after kernels_compare.hpp (CompareSide, side_desc) and before the three kernel headers above

namespace {

// The members of a gene that take part in a sample (den > 0) may lie in several connected sets and one-transcript components -- the
// PARTS of the gene in that sample.  One evaluation of a sample is a loop over its parts; the gene sum X, F and whatever else a search
// asks for are summed over them in the order of the lists below.

// A set part: packed set `set` of size class `cls` of sample `side` (0 = A, 1 = B; sample k of a K-sample call) holds at least one
// member that takes part.  A gene's parts are A's then B's (sample 0's, then 1's, ..), each side by the smallest caller tid of the
// part's members.
struct CompareGenePart { int32_t side, set, cls, reserved0; };
// A closed-form part: a member that is a one-transcript component, u reads and den (the bits of the sample's den)
struct CompareGeneClosed { double u, den; };
static_assert(sizeof(CompareGenePart) == 16, "CompareGenePart is written by the host as 16 bytes");
static_assert(sizeof(CompareGeneClosed) == 16, "CompareGeneClosed is written by the host as 16 bytes");

// den of a member taking part (dn > 0) at a point of the search.  mn = the smallest such den of the sample, (scale, shift) = the side's
// values of compare_gene_shifts.  The member(s) at the minimum take mn * scale -- on the side that shrinks scale = 1 - v > 0, where
// mn - v * mn could round to 0 --, the others dn + shift, which stays above dn - mn >= 0 there.  At lambda = 0 (scale 1, shift 0)
// both are dn itself.
__host__ __device__ inline double compare_gene_den(double dn, double mn, double scale, double shift) { return dn == mn ? mn * scale : dn + shift; }

// The den of one sample's members at one point of a search: member k_t of the closed-form list (-1: none is marked) takes den_t, every
// other member taking part compare_gene_den(dn, mn, scale, shift).  The edit functors say the same of the members in set parts.
struct GenePoint { double mn, scale, shift; int k_t; double den_t; };
// What one evaluation of a sample sums over its parts: T = the marked member's value (the searches that mark none leave it 0),
// X = the gene sum, F
struct GeneSums { double T, X, F; };
// The solves of a record: passes summed, every solve converged, rows and folded counts with reads that nothing explains
struct GeneSolveCount { int passes = 0, solves_ok = 1, infeasible = 0; };

// the closed-form parts of one side at pt, added in list order: x = u / den', F = u log x - x den
__host__ __device__ inline void gene_closed_sum(const CompareGeneClosed *c, int n, const GenePoint &pt, GeneSums &S) {
    for (int k = 0; k < n; k++) {
        const double u = c[k].u, den = c[k].den;
        const double x = u > 0.0 ? u / (k == pt.k_t ? pt.den_t : compare_gene_den(den, pt.mn, pt.scale, pt.shift)) : 0.0;
        S.X += x;
        if (k == pt.k_t) S.T += x;
        S.F += u > 0.0 ? u * log(x) - x * den : 0.0;
    }
}

// solve_one_set's den hook of the gene searches: every member of the gene that takes part gets its shifted den in LDS; membership of
// a local transcript is gene_of_lib[its library tid] == gene, so no member list and no LDS array is needed
struct GeneDenEdit {
    static constexpr bool kActive = true;
    const int32_t *gene_of;
    int32_t gene;
    double mn, scale, shift;
    __device__ double operator()(int32_t tid, double dn) const {
        return (dn > 0.0 && gene_of[tid] == gene) ? compare_gene_den(dn, mn, scale, shift) : dn;
    }
};

// What rides on the reduction of a part's epilogue besides F: kSums extra sums, and what the local transcript with library tid `tid`
// and value xi adds to this thread's share of them (by the fields of the edit functor of the solve)
struct NoTally { static constexpr int kSums = 0; };
struct GeneSumTally {                    // X: the members' sum
    static constexpr int kSums = 1;
    template <class Edit> __device__ static void add(const Edit &e, int32_t tid, double xi, double *acc) { if (e.gene_of[tid] == e.gene) acc[0] += xi; }
};
struct UsageTally {                      // X, and T: member e.t's own value
    static constexpr int kSums = 2;
    template <class Edit> __device__ static void add(const Edit &e, int32_t tid, double xi, double *acc) {
        if (e.gene_of[tid] == e.gene) { acc[0] += xi; if (tid == e.t) acc[1] += xi; }
    }
};

// One set part at one point: the set solved with the den that `edit` puts into LDS, then the presence epilogue's F and, from the same
// reduction, the tally's sums.  ORIGINAL_DEN: F takes the den of every transcript from den_g again -- a member's original bits, anyone
// else's the bits that lie in LDS -- (the shifted solves); else from LDS (the drop: the members are at 0 whatever their den).  Every
// value comes back through set_uniform: the kernels branch on them.
struct GenePartSolved { GeneSums S; int passes, converged, infeasible; };
template <int THREADS, bool ORIGINAL_DEN, class Tally, class Edit>
__device__ __forceinline__ GenePartSolved solve_gene_part(const CompareSide &G, const CompareGenePart pt, SetSolveParams P, const Edit edit) {
    constexpr int N = Tally::kSums;
    const emsar::SetDesc d = side_desc(G, pt.cls)[pt.set];
    const int32_t *__restrict__ g_tid = G.g_tid;
    const double *__restrict__ den_g = G.den;
    SetSolved K;
    solve_one_set<THREADS, true, Edit>(d, g_tid, G.g_u, G.row_w, G.rp, G.ent, G.cp, G.crow, den_g, nullptr, nullptr, P, -1, &K, 0.0, edit);
    const SetLds &L = K.L;
    set_sync<THREADS>();
    double s3[3] = {0.0, 0.0, 0.0};        // sum R log S + u log x, sum x den, infeasible
    double s[3 + N] = {};                  // s3, then this thread's share of the tally's sums
    set_objective_terms<THREADS>(L, K.res, s3,
                                 [&](int i) { if constexpr (ORIGINAL_DEN) return den_g[g_tid[d.tid_off + i]]; else return L.den[i]; },
                                 [&](int i, double xi, double) { if constexpr (N > 0) Tally::add(edit, g_tid[d.tid_off + i], xi, s + 3); });
    s[0] = s3[0]; s[1] = s3[1]; s[2] = s3[2];
    set_reduce_sum<THREADS, 3 + N>(s, L.red);
    set_sync<THREADS>();                   // the next solve_one_set overwrites the LDS this epilogue read
    GenePartSolved e{{0.0, 0.0, set_uniform(s[0] - s[1])}, K.passes, K.converged, (int)s[2]};
    if constexpr (N > 0) e.S.X = set_uniform(s[3]);
    if constexpr (N > 1) e.S.T = set_uniform(s[4]);
    return e;
}

// One sample at one point: its set parts one after the other in the same LDS (solve_gene_part), in list order, then its closed-form
// parts in registers, by every thread alike, added into S and C.  solve_one_set reloads the set and restarts from the uniform point
// each time, so what is added is a pure function of (the lists, pt, edit, P).
// Every branch is taken by the whole workgroup: the part fields come from the lists by scalar loads of an address no thread differs
// in, T, X and F go through set_uniform; the strided loops and the reductions stand outside any branch that threads could take
// differently.  The kernels that call this keep to the same rule: they branch on their item's fields and on S alone.
// The worst case is n_parts * P.max_iter passes; the drivers admit at most 64 parts per sample.
template <int THREADS, bool ORIGINAL_DEN, class Tally, class Edit>
__device__ __forceinline__ void eval_gene_side(const CompareSide &G, const CompareGenePart *__restrict__ parts, int n_parts,
                                               const CompareGeneClosed *__restrict__ closed, int n_closed, const GenePoint &pt, SetSolveParams P,
                                               const Edit edit, GeneSums &S, GeneSolveCount &C) {
#pragma nounroll
    for (int k = 0; k < n_parts; k++) {
        const GenePartSolved e = solve_gene_part<THREADS, ORIGINAL_DEN, Tally>(G, parts[k], P, edit);
        C.passes += e.passes;
        C.solves_ok &= e.converged;
        C.infeasible += e.infeasible;
        if constexpr (Tally::kSums > 1) S.T += e.S.T;
        if constexpr (Tally::kSums > 0) S.X += e.S.X;
        S.F += e.S.F;
    }
    gene_closed_sum(closed, n_closed, pt, S);
}

}  // namespace
