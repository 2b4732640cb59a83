"""GPU: every cycle and the Newton step of the set-resident solver (set_mode 0; kernels_sets.hpp: solve_one_set, set_newton_step; through
k_solve_sets<64|256|512> and k_solve_sets_boot) against the long-double reference of tests/cycle_reference.py, each from its own start
point -- no trajectory is followed, so no error and no differing branch carries over.

The set solver starts at theta = 1 where den > 0, has no atomics (bit-reproducible in any mode) and looks at max_iter at fixed places.
With a rule that cannot fire (tol 1e-300, zero_cut = abs_step = 0, newton_after -1) the solve with max_iter = 3 k returns exactly the
point A_k that the solve with max_iter = 3 (k + 1) passes through, max_iter = 3 k + 1 returns EM(A_k), final_delta of the 3 (k + 1) solve
is the measure of the step A_k -> EM(A_k), loglik is F at the returned point, and with one resident set set_passes_max is that set's
pass counter.  The reference is started at the device's A_k and must give the device's A_{k+1}.  The only hidden state is the set's own
stepmax, which the reference carries; test_set_cycle_cpu.py shows that every decision of the K checked cycles has a margin.

Tolerances.  theta, per component, in reads: cycle_reference.theta_bound without a fixed-point grid, 4 (1 + s)^2 1e-11 kappa_t theta_t den_t;
components with kappa_t > 1e4 are left out, at most 1 % per cycle.  final_delta: 1e-9 relative.  loglik: 1e-10 |F| + 1e-9.  The plain step:
1e-11 |theta| + 1e-300.  After a Newton step: |dtheta_t| den_t <= B (theta_t den_t + 1e-6) with B = max(1e-11, 100 NEWTON_DIST) = 1.4e-9,
NEWTON_DIST = 1.4e-11 the distance measured between the restatement in float64 and in long double (test_set_cycle_cpu.py); its
final_delta within 1e-9 relative + 2 (2 + measure) B, what B leaves open in |y - x| / (|y| + 1e-6).

Worst ratio to the bound over the checked cycles of a case, MI355X (theta / final_delta / loglik; CSR and TILED give the same figures):
    class 0   edge0 1.9e-3 / 1.6e-6 / 3.0e-6    edge2 2.9e-6 / 1.1e-4 / 2.3e-6    ragged 3.7e-6 / 3.4e-7 / 2.9e-6
              40x80x227-s307 1.9e-4 / 7.1e-7 / 4.1e-6    -s308 6.9e-5 / 7.5e-7 / 2.9e-6
              ragged-s2 1.6e-5 / 8.4e-7 / 3.3e-6    -s4 1.0e-4 / 5.7e-7 / 3.7e-6    -s7 9.9e-5 / 2.9e-7 / 1.7e-6
    class 1   edge1 3.8e-3 / 6.7e-7 / 4.1e-6    edge3 3.3e-6 / 1.8e-4 / 1.9e-6    edge4 2.3e-5 / 2.9e-6 / 2.3e-6    edge6 3.4e-5 / 2.0e-5 / 1.9e-6
              40x80x228-s325 9.2e-3 / 6.0e-7 / 3.0e-6    -s302 4.8e-5 / 1.2e-6 / 2.9e-6    250x500x4784-s308 5.6e-5 / 7.9e-7 / 3.5e-6
              fast_slow_linked 2.6e-6 / 7.2e-7 / 4.2e-6
    class 2   edge5 1.4e-4 / 1.3e-6 / 3.3e-6    edge7 1.3e-5 / 3.5e-5 / 3.6e-6    edge8 2.7e-4 / 4.5e-7 / 3.9e-6
              100x513x1100-s302 4.0e-4 / 6.7e-7 / 1.8e-6    -s311 1.3e-3 / 3.8e-7 / 3.5e-6
              250x500x4785-s300 .. -s311: 1.9e-4 .. 1.1e-3 / 2.1e-7 .. 2.4e-6 / 2.2e-6 .. 4.4e-6, up to 0.8 % left out
    22 sets in one launch   theta 0.044, final_delta 4.9e-7 (the largest of the sets' measures)
    plain steps and plain EM   theta <= 5.6e-5 of 1e-11 relative, final_delta <= 1.8e-4
    Newton step   theta <= 7.0e-3 of its bound (edge4 after 50 cycles; a refused step would be 8e12 .. 9e15 bounds away), final_delta <= 3.2e-4
                  of its bound, pass counts equal (31, 82, 32, 177, 20 and 209 passes); every point had its margins at the device's A_k too
                  the refused step (40x80x227-s307 after 18 cycles): theta 2.0e-5 of 1e-11 relative, final_delta 8.5e-7, 79 passes
    replicates    theta <= 0.011; every replicate kept its margins for all K cycles
So theta has two decimal digits of room and more, the measure and the likelihood four to six.

Each of these changes to kernels_sets.hpp fails the tests named (tried on an MI355X, the library built with the change and not kept):
    acceptance without "- s2[1]"                         test_every_cycle_from_its_own_start (the 10 seeded cases that have a rejected cycle), test_every_set_of_one_launch..,
                                                         test_stopping_rules[0-10, 1-10], test_the_newton_step[late class 0 and 1], test_replicates..[0, 2]: 32 tests
    a rejected cycle keeps the extrapolated A            the same 32
    no stepmax / 4 after a clamped rejection             test_every_cycle_from_its_own_start[40x80x228-s325, 100x513x1100-s302, ragged-s4, ragged-s7] (the next clamped
                                                         cycle is clamped at the larger bound), test_every_set_of_one_launch.., test_stopping_rules[1-10],
                                                         test_the_newton_step[edge4]: 13 tests
    s > 1.0 for s > 1.01                                 test_every_cycle_from_its_own_start[fast_slow_linked-*] alone (cycle 2 has s = 1.0051)
    set_reduce_sum for THREADS > 64 without the last     test_every_cycle_from_its_own_start[edge4, edge5, edge6, edge8, 250x500x4784-s308, 100x513x1100-s302, 250x500x4785-s300,
    wave's partial                                       -s301, -s302, -s303, -s305, -s307, -s308, -s311], test_every_set_of_one_launch.., test_stopping_rules[2-10],
                                                         test_the_newton_step[edge4, 100x513x1100-s302, edge8], test_replicates..[2]: 39 tests; every class 0 case passes,
                                                         and so do the other cases of class 1 and 2: none of their transcripts lies in the last wave, only rows at the most
    delta taken in pass 2 as well                        test_every_cycle_from_its_own_start, test_the_plain_step_and_plain_em (every case of both),
                                                         test_every_set_of_one_launch.., test_stopping_rules: 107 tests
    a Newton step accepted whatever Fn is                test_the_newton_step, all 14 (the refused point among them)
    CG iterations not counted in passes                  test_the_newton_step, all 14
"""
import numpy as np
import pytest

from emsar_amd import EmsarHip
from emsar_amd.hip import LAYOUT_CSR, LAYOUT_TILED
from tests import cycle_reference as CR
from tests import set_problems as SP
from tests.test_set_cycle_cpu import BOOT_MIN, BOOT_N, BOOT_SEED, LATE_CASE, LATE_PASSES, RULE_CASES, RULE_POINTS, first_stop, flip_tol
from tests.test_squarem_cycle_gpu import KNOBS

pytestmark = pytest.mark.gpu

LAYOUTS = {"csr": (LAYOUT_CSR, "1"), "tiled": (LAYOUT_TILED, "2")}      # as test_set_edges_gpu.py: TILED with the library's own numbering forced on
NAMES = list(CR.SET_CASES)
QUIET = dict(set_mode=0, tol=1e-300, newton_after=-1)                    # no rule can fire, no Newton step
PLAIN_PASSES = 6
RES_MUST, RES_K = 3, 12        # the resident problem: cycles every edge-shaped set must have margins for (the smallest K of the edge problems), prefixes solved
NEWTON_B = max(1e-11, 100 * CR.NEWTON_DIST)

_solves, _resident = {}, []


def _context(monkeypatch, P, lid):
    layout, renumber = LAYOUTS[lid]
    for k in KNOBS:
        monkeypatch.delenv("EMSAR_HIP_" + k, raising=False)
    monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
    ctx = EmsarHip(0)
    try:
        ctx.upload_structure(P.n_tx, P.rp, P.ci, layout)
        ctx.upload_sample(P.R, P.E, P.den)
    except Exception:
        ctx.close()
        raise
    return ctx


def _quiet(ctx, n_sets=1, **kw):
    """a solve in which no rule can fire: it ends at max_iter, in the set solver alone"""
    th, st = ctx.solve(**dict(QUIET, **kw))
    assert st.sets_resident == n_sets and st.sets_streamed == 0 and st.sets_cluster == 0, (st.sets_resident, st.sets_streamed, st.sets_cluster)
    assert st.converged == 0 and st.iters == st.set_passes_max == kw["max_iter"], (st.converged, st.iters, st.set_passes_max, kw)
    if n_sets == 1:
        assert st.set_passes_sum == kw["max_iter"]
    return th, st


def resident():
    if not _resident:
        _resident.append(CR.SetCase("resident", RES_K, None, SP.all_resident_members()))
    return _resident[0]


def solves(monkeypatch, name, lid):
    """One context, one upload (cached): 'cycle': the prefix solves max_iter = 3, 6, .. 3 K; for a single set under CSR, where
    test_the_plain_step_and_plain_em reads them, also 'step': max_iter = 3 k + 1, k = 0 .. K - 1, and 'em': accel = 0,
    max_iter = 1 .. PLAIN_PASSES.  Each (theta, stats)."""
    key = (name, lid)
    if key not in _solves:
        P = resident() if name == "resident" else CR.set_case(name)
        n = len(P.models)
        with _context(monkeypatch, P, lid) as ctx:
            out = {"cycle": [_quiet(ctx, n, max_iter=3 * k, accel=1) for k in range(1, P.K + 1)]}
            if n == 1 and lid == "csr":
                out["step"] = [_quiet(ctx, n, max_iter=3 * k + 1, accel=1) for k in range(P.K)]
                out["em"] = [_quiet(ctx, n, max_iter=j, accel=0) for j in range(1, PLAIN_PASSES + 1)]
        _solves[key] = out
    return _solves[key]


def reference_cycle(m, A, stepmax, k):
    """the reference's cycle from the device's point (cached: layouts that give the same bits share it)"""
    cache = m.__dict__.setdefault("_cycles", {})             # kept with the model: it lives as long as the model does
    key = (A.tobytes(), stepmax, k)
    if key not in cache:
        cache[key] = m.cycle(A, stepmax, 3 * k)
    return cache[key]


def check_set(what, m, points, must, worst):
    """Every cycle of one set from its own start: points[k] is the device's A_k (points[0] the uniform start).  The first `must` cycles
    must have margins at the device's points (a failure there is "no margin", not a kernel error); after them the run ends at the first
    cycle without.  Returns the reference's cycles; worst collects the largest ratios to the bounds."""
    stepmax, out = 1.0, []
    for k in range(len(points) - 1):
        A, th = points[k], points[k + 1]
        c = reference_cycle(m, A, stepmax, k)
        at = "%s cycle %d: %s" % (what, k + 1, CR.margins(c))
        bound, covered = CR.theta_bound(m, c, False)
        if not (CR.comparable(c) and (~covered).mean() <= CR.LEFT_OUT_MAX):
            assert k >= must, "no margin: " + at
            break
        worst["left_out"] = max(worst["left_out"], float((~covered).mean()))
        want = c.A_next.astype(np.float64)
        err = np.abs(th - want) * m.den
        ratio = float(np.max(np.where(covered & (err > 0), err / np.maximum(bound, 1e-300), 0.0)))
        worst["theta"] = max(worst["theta"], ratio)
        if ratio > 1.0:                         # which point DID the device continue from?
            other = {"EM(thx)": m.em(c.thx)[0], "th2": c.th2, "thx": c.thx, "th1": c.th1}
            near = {n: float(np.max(np.abs(th - v.astype(np.float64)) * m.den)) for n, v in other.items()}
            t = int(np.argmax(np.where(covered, err / np.maximum(bound, 1e-300), 0.0)))
            pytest.fail("%s\n  theta off by %.3g of its bound at t = %d (got %.17g want %.17g kappa %.3g); the reference continues from %s; "
                        "largest distance in reads from: %s" % (at, ratio, t, th[t], want[t], float(c.kappa[t]), "EM(thx)" if c.ok else "th2", near))
        out.append(c)
        stepmax = c.stepmax_next
    return out


def new_worst():
    return {"theta": 0.0, "delta": 0.0, "loglik": 0.0, "left_out": 0.0, "step": 0.0}


def close(got, want, rel, worst=None, key=None):
    r = abs(got - want) / (rel * abs(want)) if want != 0 else (0.0 if got == 0 else np.inf)
    if worst is not None:
        worst[key] = max(worst[key], r)
    return r <= 1.0


# ---- a. every cycle from its own start ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lid", list(LAYOUTS))
@pytest.mark.parametrize("name", NAMES)
def test_every_cycle_from_its_own_start(monkeypatch, name, lid):
    P = CR.set_case(name)
    m = P.model
    sols = solves(monkeypatch, name, lid)["cycle"]
    worst = new_worst()
    points = [m.start] + [th for th, _ in sols]
    cycles = check_set("%s-%s" % (name, lid), m, points, P.K, worst)
    assert len(cycles) == P.K
    for k, (c, (th, st)) in enumerate(zip(cycles, sols)):
        at = "%s-%s cycle %d: %s" % (name, lid, k + 1, CR.margins(c))
        assert close(st.final_delta, float(c.measure), 1e-9, worst, "delta"), "%s\n  final_delta %.17g, the measure of the first step %.17g" % (
            at, st.final_delta, float(c.measure))
        if k > 0:                               # F at this cycle's start is the loglik of the solve that stopped there
            F, ll = float(c.F_A), sols[k - 1][1].loglik
            worst["loglik"] = max(worst["loglik"], abs(ll - F) / (1e-10 * abs(F) + 1e-9))
            assert abs(ll - F) <= 1e-10 * abs(F) + 1e-9, (at, ll, F)
    F, ll = float(m.F(points[-1])[0]), sols[-1][1].loglik
    worst["loglik"] = max(worst["loglik"], abs(ll - F) / (1e-10 * abs(F) + 1e-9))
    assert abs(ll - F) <= 1e-10 * abs(F) + 1e-9, (name, ll, F)
    print("%s-%s class %d: %d cycles, worst ratio to the bound: theta %.3g final_delta %.3g loglik %.3g; left out %.4f; kinds %s" % (
        name, lid, P.cls, len(cycles), worst["theta"], worst["delta"], worst["loglik"], worst["left_out"], " ".join(c.kind for c in cycles)))


# ---- b. several sets in one launch -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lid", list(LAYOUTS))
def test_every_set_of_one_launch_runs_its_own_cycles(monkeypatch, lid):
    """all_resident_problem(): all three classes in one solve, descriptor offsets that are not 0, a step and a stepmax per set"""
    P = resident()
    sets = SP.resident_sets()
    sols = solves(monkeypatch, "resident", lid)["cycle"]
    worst = new_worst()
    measures = np.zeros((len(sets), RES_K))
    for i, (s, m, tids) in enumerate(zip(sets, P.models, P.tids)):
        points = [m.start] + [th[tids] for th, _ in sols]
        must = RES_MUST if s.n_t >= 18 else 1                # a small family is checked while its own margins hold: one cycle at least
        cycles = check_set("resident-%s set %d %s" % (lid, i, s.shape), m, points, must, worst)
        assert len(cycles) >= must
        print("set %2d %-18s %2d cycles %s" % (i, s.shape, len(cycles), " ".join(c.kind for c in cycles)))
        for k in range(RES_K):                               # the measure of the step A_k -> EM(A_k) needs no margin
            measures[i, k] = float(m.plain(points[k], 3 * k).measure)
    for k, (_, st) in enumerate(sols):
        assert close(st.final_delta, measures[:, k].max(), 1e-9, worst, "delta"), (k + 1, st.final_delta, measures[:, k].max(), int(np.argmax(measures[:, k])))
    print("resident-%s: worst ratio to the bound: theta %.3g final_delta %.3g; left out %.4f" % (lid, worst["theta"], worst["delta"], worst["left_out"]))


# ---- c. the plain step and plain EM ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_the_plain_step_and_plain_em(monkeypatch, name):
    """max_iter = 3 k + 1 ends after the first pass of cycle k + 1 and returns its B = EM(A_k); accel = 0 swaps A and B after every pass"""
    P = CR.set_case(name)
    m = P.model
    S = solves(monkeypatch, name, "csr")
    worst = new_worst()
    points = [m.start] + [th for th, _ in S["cycle"]]
    for k, (th, st) in enumerate(S["step"]):
        c = m.plain(points[k], 3 * k)
        want = c.A_next.astype(np.float64)
        worst["step"] = max(worst["step"], float(np.max(np.abs(th - want) / (1e-11 * np.abs(want) + 1e-300))))
        assert np.all(np.abs(th - want) <= 1e-11 * np.abs(want) + 1e-300), (name, k)
        assert close(st.final_delta, float(c.measure), 1e-9, worst, "delta"), (name, k, st.final_delta, float(c.measure))
        assert close(st.final_delta, S["cycle"][k][1].final_delta, 1e-15)                  # the same step, measured by the 3 (k + 1) solve
    A = m.start
    for j, (th, st) in enumerate(S["em"]):
        c = m.plain(A, j)
        want = c.A_next.astype(np.float64)
        worst["step"] = max(worst["step"], float(np.max(np.abs(th - want) / (1e-11 * np.abs(want) + 1e-300))))
        assert np.all(np.abs(th - want) <= 1e-11 * np.abs(want) + 1e-300), (name, "plain EM pass", j + 1)
        assert close(st.final_delta, float(c.measure), 1e-9, worst, "delta"), (name, j + 1, st.final_delta, float(c.measure))
        if j > 0:
            F, ll = float(c.F_A), S["em"][j - 1][1].loglik
            assert abs(ll - F) <= 1e-10 * abs(F) + 1e-9, (name, j, ll, F)
        A = th
    print("%s: plain steps, worst ratio to the bound: theta %.3g final_delta %.3g" % (name, worst["step"], worst["delta"]))


# ---- d. the stopping rules ---------------------------------------------------------------------------------------------------------------

def _rule_kw(r):
    return dict(abs_floor=r.abs_floor, count_floor=r.count_floor, zero_cut=r.zero_cut, abs_step=r.abs_step)


@pytest.mark.parametrize("k", RULE_POINTS)
@pytest.mark.parametrize("cls", list(RULE_CASES))
def test_stopping_rules(monkeypatch, cls, k):
    """newton_after -1: the resident sets keep the two print-quantum rules.  final_delta is the measure of the cycle's first step under each
    rule, and with a tol between the ruled and the plain measure the solve stops at the first first-step below it -- with the rule at
    another pass than without."""
    name = RULE_CASES[cls]
    P = CR.set_case(name)
    m = P.model
    sols = solves(monkeypatch, name, "csr")["cycle"]
    points = [m.start] + [th for th, _ in sols]
    before = check_set(name, m, points[:k + 2], k + 1, new_worst())               # the cycles that start at A_0 .. A_k
    assert len(before) == k + 1
    c = before[k]
    rules = CR.choose_rules(m, c.A, c.th1, 3 * k)
    assert set(rules) == {"plain", "count_floor", "zero_cut", "abs_step"}, list(rules)
    plain = float(rules["plain"][2])
    half_gap = (np.sqrt(CR.GAP_MIN) - 1) / 2
    with _context(monkeypatch, P, "csr") as ctx:
        for rule, (r, gap, measure) in rules.items():
            measure = float(measure)
            margin = CR.stop_measure(c.A, c.th1, m.den, r, 3 * k)[1]
            # conditions on the reference alone (the CPU test shows them for the reference's own trajectory)
            assert gap >= CR.GAP_MIN and measure > 0 and margin >= half_gap, (rule, gap, measure, margin)
            th, st = _quiet(ctx, max_iter=3 * k + 3, accel=1, **_rule_kw(r))
            print("%s k %d %-11s gap %.4g margin %.3g: final_delta %.17g reference %.17g plain %.6g, %.3g of 1e-9" % (
                name, k, rule, gap, margin, st.final_delta, measure, plain, abs(st.final_delta - measure) / (1e-9 * measure)))
            assert close(st.final_delta, measure, 1e-9), (rule, st.final_delta, measure)
            assert np.array_equal(th.view(np.int64), points[k + 1].view(np.int64))         # a rule that does not fire changes no point
            if rule == "plain":
                continue
            assert abs(measure - plain) > (0.1 if rule == "count_floor" else 1e-3) * plain, (rule, measure, plain)
            tol = flip_tol(measure, plain)
            ruled = [CR.stop_measure(e.A, e.th1, m.den, r, 3 * j)[0] for j, e in enumerate(before)]
            j_r, m_r = first_stop(ruled, tol)
            j_p, m_p = first_stop([e.measure for e in before], tol)
            assert j_r is not None and min(m_r, m_p) >= half_gap, ("no margin", rule, j_r, j_p, m_r, m_p)
            th, st = ctx.solve(set_mode=0, newton_after=-1, accel=1, tol=tol, max_iter=3 * k + 1, **_rule_kw(r))
            print("    tol %.6g with the rule: converged %d after %d passes (reference: cycle %d)" % (tol, st.converged, st.set_passes_max, j_r + 1))
            assert (st.converged, st.iters, st.set_passes_max, st.sets_unconverged) == (1, 3 * j_r + 1, 3 * j_r + 1, 0), (rule, j_r)
            assert close(st.final_delta, float(ruled[j_r]), 1e-9) and st.final_delta < tol
            th, st = ctx.solve(set_mode=0, newton_after=-1, accel=1, tol=tol, max_iter=3 * k + 1)
            print("    tol %.6g without: converged %d after %d passes (reference: %s)" % (tol, st.converged, st.set_passes_max, j_p))
            j_end = k if j_p is None else j_p
            assert (st.converged, st.iters, st.set_passes_max) == (int(j_p is not None), 3 * j_end + 1, 3 * j_end + 1), (rule, j_p)
            assert close(st.final_delta, float(before[j_end].measure), 1e-9)


def test_abs_step_bound_follows_the_set_s_own_pass_count(monkeypatch):
    """Past 1000 passes the bound shrinks like 1 / (passes + 1), passes being the counter of the workgroup that solves the set.  A bound
    frozen at pass 1000 is three times larger here and silences every component (the reference's measure under it differs: asserted)."""
    P = CR.set_case(LATE_CASE)
    m = P.model
    with _context(monkeypatch, P, "csr") as ctx:
        A, _ = _quiet(ctx, max_iter=LATE_PASSES, accel=0)
        c = m.plain(A, LATE_PASSES)
        found = CR.choose_late_abs_step(m, A, c.A_next, LATE_PASSES)
        assert found is not None
        r, gap, measure, frozen = found
        margin = CR.stop_measure(A, c.A_next, m.den, r, LATE_PASSES)[1]
        assert gap >= CR.GAP_MIN ** 2 and margin >= (np.sqrt(CR.GAP_MIN) - 1) / 2, (gap, margin)
        assert abs(float(frozen) - float(measure)) > 1e-3 * float(measure)
        th, st = _quiet(ctx, max_iter=LATE_PASSES + 1, accel=0, **_rule_kw(r))
    print("abs_step %.6g gap %.4g margin %.3g: final_delta %.17g reference %.17g (plain %.6g, with the bound of pass 1000 %.6g), %.3g of 1e-9" % (
        r.abs_step, gap, margin, st.final_delta, float(measure), float(c.measure), float(frozen), abs(st.final_delta - float(measure)) / (1e-9 * float(measure))))
    assert close(st.final_delta, float(measure), 1e-9), (st.final_delta, float(measure))
    assert np.all(np.abs(th - c.A_next.astype(np.float64)) <= 1e-11 * np.abs(th) + 1e-300)


# ---- e. the Newton step ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lid", list(LAYOUTS))
@pytest.mark.parametrize("cls,name,when,k", [(c, n, w, ks[0]) for c, pts in CR.NEWTON_POINTS.items() for (n, w, ks) in pts])
def test_the_newton_step(monkeypatch, cls, name, when, k, lid):
    """newton_after = max_iter = 3 k returns A_k (the step would come after the look at max_iter); max_iter = 3 k + 1 makes the step from
    A_k and one plain pass: EM(N(A_k)), or EM(A_k) where the step is refused, after 3 k + 1 + n_cg + n_trials + 1 passes either way."""
    P = CR.set_case(name)
    m = P.model
    with _context(monkeypatch, P, lid) as ctx:
        A, _ = _quiet(ctx, max_iter=3 * k, accel=1, newton_after=3 * k)
        o = CR.newton_step(m, A)
        print("%s-%s k %d: %s" % (name, lid, k, CR.newton_margins(o)))
        # conditions on the reference at the device's point (the CPU test shows them on the reference's own trajectory)
        assert CR.newton_comparable(o) and o.accepted == (when != "refused"), "no margin: " + CR.newton_margins(o)
        assert when != "late" or o.bound.any()               # the late points are there for the bound components
        plain, _ = _quiet(ctx, max_iter=3 * k, accel=1)
        assert np.array_equal(A.view(np.int64), plain.view(np.int64))                    # newton_after changes no point before the step
        passes = 3 * k + o.passes + 1
        th, st = ctx.solve(set_mode=0, tol=1e-300, accel=1, newton_after=3 * k, max_iter=3 * k + 1)
    want = o.y.astype(np.float64)
    measure = float(o.measure)
    assert (st.iters, st.set_passes_max, st.set_passes_sum, st.converged) == (passes, passes, passes, 0)
    if when == "refused":                                    # the point is left alone: a plain step from A_k, the passes of the attempt counted
        assert o.n_trials == 4 and np.array_equal(o.x_new.astype(np.float64), A)
        err = np.abs(th - want) / (1e-11 * np.abs(want) + 1e-300)
        print("%s-%s k %d refused: theta %.3g of 1e-11 relative, passes %d (reference %d), final_delta %.3g of 1e-9" % (
            name, lid, k, float(err.max()), st.set_passes_max, passes, abs(st.final_delta - measure) / (1e-9 * measure)))
        assert float(err.max()) <= 1.0, (int(np.argmax(err)), float(err.max()))
        assert close(st.final_delta, measure, 1e-9), (st.final_delta, measure)
        return
    refused = m.em(A)[0].astype(np.float64)                  # what a refused step would return
    err = np.abs(th - want) * m.den / (NEWTON_B * (want * m.den + CR.NEWTON_FLOOR_READS))
    moved = float(np.max(np.abs(refused - want) * m.den / (NEWTON_B * (want * m.den + CR.NEWTON_FLOOR_READS))))
    d_tol = 1e-9 * measure + 2 * (2 + measure) * NEWTON_B
    print("%s-%s k %d: theta %.3g of the bound (a refused step: %.3g), passes %d (reference %d), final_delta %.17g reference %.17g: %.3g of the bound" % (
        name, lid, k, float(err.max()), moved, st.set_passes_max, passes, st.final_delta, measure, abs(st.final_delta - measure) / d_tol))
    assert moved > 100.0                                     # a condition: the step shows
    assert float(err.max()) <= 1.0, (int(np.argmax(err)), float(err.max()))
    assert abs(st.final_delta - measure) <= d_tol, (st.final_delta, measure)
    if when == "late":
        assert np.all(th[o.bound & (o.y == 0)] == 0.0)       # bound components go to exactly 0 and stay there under the EM


# ---- f. replicates -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lid", list(LAYOUTS))
@pytest.mark.parametrize("cls", list(RULE_CASES))
def test_replicates_run_the_same_cycles_on_their_draws(monkeypatch, cls, lid):
    """k_solve_sets_boot: replicate b of the bootstrap with max_iter = 3 (k + 1) is the reference's cycle from replicate b with
    max_iter = 3 k, on the drawn weights.  Rows that drew 0 stay in the set.  The margins of the drawn samples are what they are: a
    replicate's run ends at its first cycle without, after BOOT_MIN at least (test_set_cycle_cpu.py shows them on the host's draws)."""
    P = CR.set_case(RULE_CASES[cls])
    kw = dict(QUIET, accel=1, want_replicates=True)
    with _context(monkeypatch, P, lid) as ctx:
        w = [ctx.bootstrap_weights(BOOT_SEED, b) for b in range(BOOT_N)]
        reps = []
        for k in range(1, P.K + 1):
            out = ctx.bootstrap(BOOT_N, BOOT_SEED, max_iter=3 * k, **kw)
            assert out[4].n_replicates == BOOT_N and out[4].replicates_unconverged == BOOT_N and out[4].set_passes_max == 3 * k
            reps.append(out[3])
    worst = new_worst()
    for b in range(BOOT_N):
        m = CR.Model(P.n_tx, P.rp, P.ci, w[b], P.den, P.E)
        assert (w[b][P.E == 0] == 0).all()
        cycles = check_set("%s-%s replicate %d" % (P.name, lid, b), m, [m.start] + [r[b] for r in reps], BOOT_MIN, worst)
        print("%s-%s replicate %d (%d rows drew 0): %d cycles %s" % (P.name, lid, b, int(((w[b] == 0) & (P.E != 0)).sum()), len(cycles), " ".join(c.kind for c in cycles)))
        assert len(cycles) >= BOOT_MIN
    print("%s-%s replicates: worst ratio to the bound: theta %.3g; left out %.4f" % (P.name, lid, worst["theta"], worst["left_out"]))
