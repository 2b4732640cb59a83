// kernels_profile_genes.hpp -- k_profile_gene_base, k_profile_gene_sets: the profile-likelihood interval of a gene's total and the gene
// presence test (emsar_hip_profile_genes; driver: profile_genes.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_gene_parts.hpp

namespace {

// A gene's members taking part, its parts (CompareGenePart with side 0, CompareGeneClosed), X and F are those of kernels_gene_parts.hpp
// for one sample.  The path: the maximiser of F - lambda X is the same problem with den_t + lambda on every member taking part, lambda in
// (-mn, inf), mn = the smallest such den; the coordinate is s = 1 + lambda / mn, a member's den in LDS compare_gene_den(dn, mn, s,
// mn * (s - 1)).  s > 1 is the lower side, 0 < s < 1 the upper side, s = 1 every den exactly its own.
//
// Two families, not one with a mode: a search item needs X_hat, F_hat and (to know whether a lower limit exists) Lambda of its gene, so
// the baselines run in an earlier launch in any case; and a kernel that holds no ProfileStep keeps fewer scalar registers live across
// the solves.

// One gene's baseline and drop: its slice of the part list and of the closed-form list, the gene id, mn.  skip_drop: the host knows
// the gene to be essential (a member has reads only it explains), so the drop solves would decide nothing.
struct ProfileGeneBaseItem { int32_t part_off, n_parts, closed_off, n_closed, gene, skip_drop; double mn; };
// X_hat, F_hat: the gene sum and F with every den its own; F_drop: F with every member's den 0 (closed-form members with reads are
// never dropped here: skip_drop); infeasible: rows and folded counts with reads that nothing explains in the drop solves
struct ProfileGeneBaseRec { double X_hat, F_hat, F_drop; int32_t infeasible, passes, converged, reserved0; };
// One limit of one gene.  side 0 = lower (s > 1), 1 = upper (s < 1).  end: the range of the upper side has a reachable end at s = 0
// (mn0, ProfileGeneStep); X_hat, F_hat are the baseline record's.
struct ProfileGeneItem { int32_t part_off, n_parts, closed_off, n_closed, gene, side, end, reserved0; double mn, mn0, X_hat, F_hat; };
static_assert(sizeof(ProfileGeneBaseItem) == 32, "ProfileGeneBaseItem is written by the host as 32 bytes");
static_assert(sizeof(ProfileGeneBaseRec) == 40, "ProfileGeneBaseRec is read by the host as 40 bytes");
static_assert(sizeof(ProfileGeneItem) == 64, "ProfileGeneItem is written by the host as 64 bytes");
// The record of a search is k_profile_sets' (ProfileRec): x = the gene sum of the last evaluation.

// The search of one limit of a gene: ProfileStep, unchanged, driven with den_t := mn, theta_hat := X_hat -- and, in front of it, the end
// of the range on the upper side.  Z = the closed-form members without reads, mn0 = their smallest den: they add nothing to X while
// lambda > -mn0 and absorb any amount at lambda = -mn0 at a cost of mn0 per unit, so beyond X_end = X(s = 0) the profile is the straight
// line D_end + 2 mn0 (x - X_end).  Where mn0 lies strictly below the den of every other member taking part (`end`), s = 0 can be
// evaluated -- the others get dn - mn0 > 0 -- and is evaluated first: D_end < q puts the limit on the line, with no further solve;
// otherwise the limit lies at some s in (0, 1) and the ordinary search finds it, with one evaluation less to spend.
// The same code runs in the kernel (every argument of step() is uniform and scalar there) and on the host (genes whose parts are
// all closed form).
struct ProfileGeneStep {
    ProfileStep T;
    ProfileSearchParams Qs;              // Q with the end evaluation taken off max_evals
    int end_pending, end_evals;

    __host__ __device__ void start(int side, int end, double X_hat, double mn, double F_hat, const ProfileSearchParams &Q) {
        T.start(side, X_hat, mn, F_hat, Q);
        Qs = Q;
        end_pending = end; end_evals = 0;
        if (end) Qs.max_evals = Q.max_evals - 1;
    }
    __host__ __device__ double scale() { return end_pending ? (T.s = 0.0) : T.scale(); }
    __host__ __device__ int evals() const { return T.evals + end_evals; }
    // true = evaluate again, at the new scale()
    __host__ __device__ bool step(double X, double F_now, double F_hat, double mn0, double sqrt_q) {
        if (!end_pending) return T.step(X, F_now, F_hat, sqrt_q, Qs);
        end_pending = 0; end_evals = 1;
        const double raw = 2.0 * (F_hat - F_now), D_end = raw > 0.0 ? raw : 0.0;
        T.x = X; T.dev = D_end; T.F = F_now;
        if (!(raw == raw)) return false;                               // a non-finite likelihood: reported unconverged
        if (D_end < Qs.q) { T.x = X + (Qs.q - D_end) / (2.0 * mn0); T.dev = Qs.q; T.search_ok = 1; return false; }
        return Qs.max_evals >= 1;
    }
};

// solve_one_set's den hook of the drop: every member of the gene has den 0 in LDS, so it starts at 0 and stays there, as a transcript
// outside F does (k_solve_sets_drop's rule, for several transcripts at once)
struct GeneDropEdit {
    static constexpr bool kActive = true;
    const int32_t *gene_of;
    int32_t gene;
    __device__ double operator()(int32_t tid, double dn) const { return gene_of[tid] == gene ? 0.0 : dn; }
};
// The drops of the usage profile (kernels_profile_usage.hpp): member t of the gene alone (others = false), or every member but t
struct UsageDropEdit {
    static constexpr bool kActive = true;
    const int32_t *gene_of;
    int32_t gene, t;
    bool others;
    __device__ double operator()(int32_t tid, double dn) const { return (gene_of[tid] == gene && (tid == t) != others) ? 0.0 : dn; }
};

// the record of a search (k_profile_gene_sets; profile_gene_closed_limit, profile_genes.hpp); the host's closed-form genes have no
// passes, no solve that could fail and nothing infeasible: GeneSolveCount()
__host__ __device__ inline ProfileRec profile_gene_record(const ProfileGeneStep &T, const GeneSolveCount &C) {
    ProfileRec r;
    r.x = T.T.x; r.dev = T.T.dev; r.s = T.T.s; r.F = T.T.F;
    r.evals = T.evals(); r.passes = C.passes; r.flags = (T.T.search_ok ? PROFILE_REC_SEARCH_OK : 0) | (C.solves_ok ? PROFILE_REC_SOLVES_OK : 0);
    r.infeasible = C.infeasible;
    return r;
}

// Workgroup x runs gene x: the sample at s = 1 (eval_gene_side with GeneDenEdit: the code path of every evaluation of the searches,
// every den exactly its own), then -- unless the host has decided it -- every set part without the gene's members (GeneDropEdit; F
// with the den that lies in LDS: the members are at 0, anyone else's has its own bits).  A record is a pure function of (item, its
// slices of the lists, P).  The launch has the thread count of the largest class among the item's set parts and the LDS of that class
// and every smaller one.  Every branch is taken by the whole workgroup, as the comment at eval_gene_side requires.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_profile_gene_base(const ProfileGeneBaseItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                               const CompareGeneClosed *__restrict__ closed, CompareSide G,
                                                               const int32_t *__restrict__ gene_of, ProfileGeneBaseRec *__restrict__ rec,
                                                               SetSolveParams P) {
    const ProfileGeneBaseItem it = items[blockIdx.x];
    const GenePoint own{it.mn, 1.0, 0.0, -1, 0.0};
    GeneSums S{0.0, 0.0, 0.0}, D{0.0, 0.0, 0.0};
    GeneSolveCount C, CD;
    eval_gene_side<THREADS, true, GeneSumTally>(G, parts + it.part_off, it.n_parts, closed + it.closed_off, it.n_closed, own, P,
                                                GeneDenEdit{gene_of, it.gene, it.mn, 1.0, 0.0}, S, C);
    if (!it.skip_drop)
        eval_gene_side<THREADS, false, NoTally>(G, parts + it.part_off, it.n_parts, closed, 0, own, P, GeneDropEdit{gene_of, it.gene}, D, CD);
    if (threadIdx.x == 0)
        rec[blockIdx.x] = ProfileGeneBaseRec{S.X, S.F, D.F, CD.infeasible, C.passes + CD.passes, C.solves_ok & CD.solves_ok, 0};
}
const auto kProfileGeneBase = set_kernels(k_profile_gene_base<64>, k_profile_gene_base<256>, k_profile_gene_base<512>);

// Workgroup x runs the whole search of item x (ProfileGeneStep), one evaluation by eval_gene_side at s, so a record is a pure function
// of (item, its slices of the lists, P, Q).  Launch class and uniformity as k_profile_gene_base.  The worst case is
// n_parts * Q.max_evals * P.max_iter passes; the driver admits 64 parts.  The loop is written out here and in profile_gene_closed_limit:
// run through a driver shared with the host, as compare_gene_search is, it took ten more scalar spills at 256 and 512 threads and
// emsar_hip_profile_genes ran 1.5 % longer.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_profile_gene_sets(const ProfileGeneItem *__restrict__ items, const CompareGenePart *__restrict__ parts,
                                                               const CompareGeneClosed *__restrict__ closed, CompareSide G,
                                                               const int32_t *__restrict__ gene_of, ProfileRec *__restrict__ rec, SetSolveParams P,
                                                               ProfileSearchParams Q) {
    const ProfileGeneItem it = items[blockIdx.x];
    const double sqrt_q = sqrt(Q.q);
    GeneSolveCount C;
    ProfileGeneStep T;
    T.start(it.side, it.end, it.X_hat, it.mn, it.F_hat, Q);
    for (;;) {
        const double s = T.scale();
        const GenePoint pt{it.mn, s, it.mn * (s - 1.0), -1, 0.0};
        GeneSums S{0.0, 0.0, 0.0};
        eval_gene_side<THREADS, true, GeneSumTally>(G, parts + it.part_off, it.n_parts, closed + it.closed_off, it.n_closed, pt, P,
                                                    GeneDenEdit{gene_of, it.gene, pt.mn, pt.scale, pt.shift}, S, C);
        if (!T.step(S.X, S.F, it.F_hat, it.mn0, sqrt_q)) break;
    }
    if (threadIdx.x == 0) rec[blockIdx.x] = profile_gene_record(T, C);
}
const auto kProfileGeneSets = set_kernels(k_profile_gene_sets<64>, k_profile_gene_sets<256>, k_profile_gene_sets<512>);

}  // namespace

