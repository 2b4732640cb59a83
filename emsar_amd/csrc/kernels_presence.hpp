// kernels_presence.hpp -- k_solve_sets_drop: the presence test's set solves (emsar_hip_presence; driver: presence.hpp)
#pragma once
// included by emsar_hip.hip only, after kernels_sets.hpp

namespace {

// One unit of work: set `set` of its size class, solved without its local transcript `drop` (-1: the baseline, nothing dropped)
struct PresenceItem { int32_t set, drop; };
// What an item leaves: F at its optimum, the rows with reads that nothing explains there, the solve's statistics, and for a drop item
// the transcript of the set that gained most expected reads against the baseline (local index, -1 = none gained) with that gain
struct PresenceRec { double F, gain; int32_t infeasible, passes, converged, heir; };
static_assert(sizeof(PresenceRec) == 32, "PresenceRec is read by the host as 32 bytes");

// Workgroup x solves item x with solve_one_set, then evaluates the result where it lies, in LDS:
//   F = sum_c R_c log S_c + sum_t u_t log x_t - sum_t x_t den_t and the infeasible count, by set_objective_terms (one E-step
//   with log; L.red carries the reduction, nothing else of LDS is written);
//   for a drop item the arg-max over s != drop of (x_s - theta[s]) den_s, ties to the lowest local index, theta = the baseline
//   written by an EARLIER launch of baseline items into the same vector (a drop item writes nothing to it).
// Every thread reaches every barrier of the epilogue: the loops are strided over the whole workgroup and the reductions stand outside
// any branch.  A record depends on (set, drop, P) alone: no atomics, nothing shared between workgroups.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_solve_sets_drop(const emsar::SetDesc *__restrict__ desc, const PresenceItem *__restrict__ items,
                                                             const int32_t *__restrict__ g_tid, const double *__restrict__ g_u,
                                                             const double *__restrict__ row_w, const uint16_t *__restrict__ rp_g,
                                                             const uint16_t *__restrict__ ent_g, const uint16_t *__restrict__ cp_g,
                                                             const uint16_t *__restrict__ crow_g, const double *__restrict__ den_g,
                                                             double *theta, PresenceRec *__restrict__ rec, SetSolveParams P) {
    const PresenceItem it = items[blockIdx.x];
    const emsar::SetDesc d = desc[it.set];
    const int drop = it.drop;
    SetSolved K;
    solve_one_set<THREADS, true>(d, g_tid, g_u, row_w, rp_g, ent_g, cp_g, crow_g, den_g, theta, nullptr, P, drop, &K);
    const SetLds &L = K.L;
    const double *x = K.res;
    set_sync<THREADS>();
    double s3[3] = {0.0, 0.0, 0.0};        // sum R log S + u log x, sum x den, infeasible
    double best = 0.0, at = 0.0;           // this thread's largest gain and 65536 - its local index (0: none)
    set_objective_terms<THREADS>(L, x, s3, [&](int i) { return L.den[i]; }, [&](int i, double xi, double dn) {
        if (drop >= 0 && i != drop) {
            const double gain = (xi - theta[g_tid[d.tid_off + i]]) * dn;
            if (gain > best) { best = gain; at = (double)(65536 - i); }      // i ascends: the first of equal gains stays
        }
    });
    set_reduce_sum<THREADS, 3>(s3, L.red);
    const double top = set_reduce_max<THREADS>(best, L.red);
    const double who = set_reduce_max<THREADS>((top > 0.0 && best == top) ? at : 0.0, L.red);      // the lowest index among the holders of the maximum
    if (threadIdx.x == 0) {
        PresenceRec r;
        r.F = s3[0] - s3[1]; r.gain = top;
        r.infeasible = (int32_t)s3[2]; r.passes = K.passes; r.converged = K.converged;
        r.heir = who > 0.0 ? 65536 - (int32_t)who : -1;
        rec[blockIdx.x] = r;
    }
}
const auto kSolveSetsDrop = set_kernels(k_solve_sets_drop<64>, k_solve_sets_drop<256>, k_solve_sets_drop<512>);

}  // namespace
