"""CPU: the long-double reference of the set-resident solver's cycle and Newton step (tests/cycle_reference.py: Model per connected set,
newton_step) alone, from the uniform start, on the problems and for the K cycles that test_set_cycle_gpu.py checks on the device.  It
shows that the GPU test is meaningful there: every discontinuous choice of every checked cycle has a margin that two correct
implementations cannot disagree about, and the checked cycles of every size class (k_solve_sets<64>, <256>, <512>) contain every kind.

Conditions per cycle, as for the streaming solve (cycle_reference: comparable(), LEFT_OUT_MAX): acceptance 1e-9 of the sum of |terms|,
s against 1.01 1e-3, interior 1e-7, clamp 1e-6, at most 1 % of the components with kappa > 1e4.  Both are caps: K of a case is the
longest run from the start that meets them, 12 at the most for the problems of set_problems.py as the edge tests solve them and 14 for
the seeded ones.  ragged_problem() stops at K = 3: its fourth cycle leaves one of its 60 components out, 1.7 %.

Kinds (p plain, a / A accepted free / clamped, r / R rejected free / clamped), reference only:
    class 0   40x80x227-s307 paaAaaaAarrrrr   -s308 paAaaaAarrrrrr   ragged-s2 paaAaaAarrrrrr   ragged-s4 paAaaaaRAArrrr   ragged-s7 paAaaaaAaaarRA
    class 1   40x80x228-s325 paAaaarRAAaaa    -s302 paAaaarrR        250x500x4784-s308 paAaaaAarrrrrr
    class 2   100x513x1100-s302 paaaAaaRAA    -s311 paaaAaaAarr      250x500x4785-s300 .. -s311: a / A only, 2 .. 5 components keep th2 per cycle
The class 1 seeds come from a search of 40 seeds (300 .. 339) of each of (40,80,228), (250,500,4784), (18,129,258) and (100,512,1100);
the last two showed no clamped rejection.  No checked cycle of any of the 240 sets tried (those four shapes, (40,80,227) and
(100,513,1100)) has a step in (1, 1.01).  The s > 1.01 switch is shown by fast_slow_linked instead: the fast_slow sample of the streaming
test with its 128 pairs linked into one set of class 1 (cycle 2: s = 1.0051; K = 2, cycle 3 has an acceptance margin of 9.5e-10).

The Newton step: newton_step in float64 and in long double from the same points.  Where both agree on n_cg, n_trials and the
acceptance and the long-double margins hold, the largest distance between the two results (in reads, against reads + 1e-6) is
1.39e-11 over the points of cycle_reference.NEWTON_POINTS (edge4 after 55 cycles): NEWTON_DIST = 1.4e-11, and every distance is held
here to NEWTON_DIST_CAP = 2e-11.  CG amplifies rounding by the conditioning of -H: other points of these sets show up to 6e-5
(ragged-s7 after 2 cycles), and 1.3e-10 where CG stops within 1 % of its threshold (edge8 after 56 cycles: no margin, left out), which
is why the points are chosen.  test_set_cycle_gpu.py compares the device at the larger of 1e-11 and 100 NEWTON_DIST = 1.4e-9, in reads
against reads + 1e-6.  40x80x227-s307 after 18 cycles is a point where all four trial steps are refused, with margins."""
import numpy as np
import pytest

from emsar_amd import hip
from tests import cycle_reference as CR
from tests import set_problems as SP

NAMES = list(CR.SET_CASES)
KINDS = ("plain", "accepted_free", "accepted_clamped", "rejected_free", "rejected_clamped")
_runs = {}


def run(name, model=None, limit=None):
    """the reference's cycles from the uniform start while they meet the conditions, one past the cap at the most (cached)"""
    if name not in _runs:
        m = model or CR.set_case(name).model
        _runs[name] = CR.longest_run(m, limit or CR.SET_CASES[name][2] + 1)
    return _runs[name]


def trajectory(name, n):
    """the reference's points A_0 .. A_n of a case, margins or not (cached)"""
    key = ("traj", name)
    have = _runs.setdefault(key, [(CR.set_case(name).model.start, 1.0)])
    m = CR.set_case(name).model
    while len(have) <= n:
        A, sm = have[-1]
        c = m.cycle(A, sm, 3 * (len(have) - 1))
        have.append((c.A_next.astype(np.float64), c.stepmax_next))
    return [a for a, _ in have[:n + 1]]


# ---- membership ----------------------------------------------------------------------------------------------------------------------------

def test_compose_members_is_compose_and_a_partition():
    sets = SP.resident_sets()
    n_tx, rp, ci, R, E, members = SP.all_resident_members()
    for a, b in zip(SP.compose(sets, seed=16), (n_tx, rp, ci, R, E)):
        assert np.array_equal(a, b)
    for a, b in zip(SP.all_resident_problem(), (n_tx, rp, ci, R, E)):
        assert np.array_equal(a, b)
    assert len(members) == len(sets)
    tids = np.concatenate([t for t, _ in members])
    rows = np.concatenate([r for _, r in members])
    assert sorted(tids) == list(range(n_tx)) and sorted(rows) == list(range(len(rp) - 1))
    n = np.diff(rp.astype(np.int64))
    for s, (t, r) in zip(sets, members):
        assert len(t) == s.n_t
        inside = (E[r] != 0) & (n[r] >= 2)
        assert inside.sum() == len(s.rows) and sorted(R[r][inside]) == sorted(s.weights)
        held = set(t.tolist())
        for j in r:
            assert set(ci[int(rp[j]):int(rp[j + 1])].tolist()) <= held


def test_the_model_of_a_single_set_is_the_whole_sample_s():
    """edge_problem(0) through its membership: the same cycle as the whole-sample Model, in the set's own order of transcripts"""
    composed = SP.compose_members([SP.edge_set(*SP.EDGES[0][0], seed=SP.SEEDS[0])], seed=200)
    for a, b in zip(composed[:5], SP.edge_problem(0)):
        assert np.array_equal(a, b)
    P = CR.SetCase("edge0-members", 3, 0, composed)
    whole, (m,), (tids,) = P.whole, P.models, P.tids
    assert np.array_equal(m.den, whole.den[tids]) and m.N == whole.N and abs(m.const - whole.const) <= 1e-15 * abs(whole.const)
    A, B, sa, sb = whole.start, m.start, 1.0, 1.0
    for k in range(3):
        a, b = whole.cycle(A, sa, 3 * k), m.cycle(B, sb, 3 * k)
        assert a.kind == b.kind and a.stepmax_next == b.stepmax_next
        assert np.all(np.abs(a.A_next[tids] - b.A_next) <= 1e-16 * np.abs(b.A_next))
        assert abs(a.measure - b.measure) <= 1e-16 * b.measure and abs(a.F_A - b.F_A) <= 1e-16 * abs(b.F_A)
        A, B, sa, sb = a.A_next, b.A_next, a.stepmax_next, b.stepmax_next


def test_every_set_of_the_resident_problem_has_checked_cycles():
    """the sets of all_resident_problem(): the edge shapes and the ragged set keep the K of their own problems' kind (at least 3 cycles),
    the small families converge within a few cycles and are checked while their margins hold"""
    P = resident_case()
    sets = SP.resident_sets()
    for k, (s, m) in enumerate(zip(sets, P.models)):
        r = CR.longest_run(m, 12)
        print("set %2d %s: %d cycles %s" % (k, s.shape, len(r), " ".join(c.kind for c in r)))
        assert len(r) >= (3 if s.n_t >= 18 else 1)
        assert m.den.min() > 0


def resident_case():
    if "resident" not in _runs:
        _runs["resident"] = CR.SetCase("resident", 12, None, SP.all_resident_members())
    return _runs["resident"]


# ---- the cycles ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_every_checked_cycle_has_margins_and_K_is_the_longest_run(name):
    cls, K, cap, _ = CR.SET_CASES[name]
    cycles = run(name)
    worst = dict(F=np.inf, s=np.inf, y=np.inf, clamp=np.inf, left_out=0.0)
    for k, c in enumerate(cycles[:K]):
        left_out = float((c.kappa > CR.KAPPA_MAX).mean())
        print("%s cycle %2d %s left out %.4f" % (name, k + 1, CR.margins(c), left_out))
        assert CR.comparable(c), (k + 1, CR.margins(c))
        assert left_out <= CR.LEFT_OUT_MAX, (k + 1, left_out)
        worst = dict(F=min(worst["F"], c.F_margin), s=min(worst["s"], c.s_margin), y=min(worst["y"], c.y_margin),
                     clamp=min(worst["clamp"], c.clamp_margin), left_out=max(worst["left_out"], left_out))
    print(name, "class", cls, "K", K, "worst", worst)
    assert K == min(len(cycles), cap), (K, len(cycles), cap)
    assert cycles[0].kind == "plain"                         # stepmax starts at 1: the first cycle cannot extrapolate


def test_the_checked_cycles_of_every_class_contain_every_kind():
    for cls in (0, 1, 2):
        names = [n for n in NAMES if CR.SET_CASES[n][0] == cls]
        runs = {n: run(n)[:CR.SET_CASES[n][1]] for n in names}
        kinds = {n: [c.kind for c in r] for n, r in runs.items()}
        print(cls, kinds)
        for kind in KINDS:
            assert any(kind in ks for ks in kinds.values()), (cls, kind)
        assert any(c.kept.any() for r in runs.values() for c in r), cls
        # the step bound moves in both directions, visibly, and a later cycle of the same run is clamped at the smaller bound
        shrunk = [(n, k + 1) for n, r in runs.items() for k, c in enumerate(r) if c.kind == "rejected_clamped" and c.stepmax_next < float(c.stepmax)]
        grown = [(n, k + 1) for n, r in runs.items() for k, c in enumerate(r) if c.kind == "accepted_clamped" and c.stepmax_next > float(c.stepmax)]
        assert shrunk and grown, (cls, shrunk, grown)
        assert any(runs[n][k].clamped and runs[n][k].extrap for n, k in shrunk if k < len(runs[n])), (cls, shrunk)


def test_a_step_between_1_and_1_01_is_not_extrapolated_and_it_shows():
    """fast_slow_linked, cycle 2: s = 1.0051 in one connected set of 256 transcripts.  No extrapolation is made; had one been made (a
    switch at 1.0), the next point would be far outside the bound of the GPU test."""
    P = CR.set_case("fast_slow_linked")
    assert len(P.models) == 1 and SP._component(P.n_tx, [tuple(P.ci[int(a):int(b)]) for a, b in zip(P.rp[:-1], P.rp[1:]) if b - a > 1]) == P.n_tx
    assert SP.lds_bytes(256, 255, 510) <= 48 * 1024 and P.cls == 1            # 256 transcripts: not the one-wave class
    c = run("fast_slow_linked")[1]
    assert not c.extrap and 1.001 < float(c.s_raw) < 1.009 and float(c.stepmax) == 4.0, CR.margins(c)
    alt = P.model.cycle(c.A, 4.0, 3, s_switch="1.0")
    assert alt.extrap and alt.ok and alt.s == c.s
    bound, covered = CR.theta_bound(P.model, c, False)
    off = np.abs(alt.A_next - c.A_next).astype(np.float64) * P.model.den
    ratio = float(np.max(np.where(covered, off / np.maximum(bound, 1e-300), 0)))
    print("extrapolating at s = %.5f moves the next point by %.3g of the bound" % (float(c.s), ratio))
    assert ratio >= 100.0


@pytest.mark.parametrize("name", NAMES)
def test_F_never_falls(name):
    P = CR.set_case(name)
    cycles = run(name)[:P.K]
    F = [float(c.F_A) for c in cycles] + [float(P.model.F(cycles[-1].A_next)[0])]
    assert all(b >= a for a, b in zip(F, F[1:])), F


# ---- the stopping rules: the values test_set_cycle_gpu.py derives at its prefix points ---------------------------------------------------------

RULE_CASES = {0: "40x80x227-s307", 1: "40x80x228-s325", 2: "250x500x4785-s300"}
RULE_POINTS = (2, 10)          # prefix solves of 2 and of 10 cycles: the measured step is the first of cycle 3 and of cycle 11


def flip_tol(ruled, plain):
    """a tol between the ruled measure and the plain one: the solve stops at that step with the rule and goes on without it"""
    return float(np.sqrt(ruled * plain))


def first_stop(measures, tol):
    """(the first step whose measure is below tol or None, the smallest relative distance of a measure up to there from tol)"""
    margin = np.inf
    for j, m in enumerate(measures):
        margin = min(margin, abs(float(m) / tol - 1.0))
        if m < tol:
            return j, margin
    return None, margin


@pytest.mark.parametrize("k", RULE_POINTS)
@pytest.mark.parametrize("cls", list(RULE_CASES))
def test_rule_values_are_far_from_every_threshold(cls, k):
    name = RULE_CASES[cls]
    P = CR.set_case(name)
    assert k < P.K
    c = run(name)[k]                                          # the cycle that starts at A_k
    rules = CR.choose_rules(P.model, c.A, c.th1, 3 * k)
    plain = float(rules["plain"][2])
    assert abs(plain - float(c.measure)) <= 1e-15 * plain
    assert set(rules) == {"plain", "count_floor", "zero_cut", "abs_step"}
    shows = []
    for rule, (r, gap, measure) in rules.items():
        m2, margin, _, _ = CR.stop_measure(c.A, c.th1, P.model.den, r, 3 * k)
        print("%s k %d %-11s gap %.4g measure %.6g (plain %.6g) margin %.3g" % (name, k, rule, gap, float(measure), plain, margin))
        assert m2 == measure and measure > 0
        if rule == "plain":
            continue
        assert gap >= CR.GAP_MIN, (rule, gap)
        assert margin >= (np.sqrt(CR.GAP_MIN) - 1) / 2, (rule, margin)
        assert abs(float(measure) - plain) > (0.1 if rule == "count_floor" else 1e-3) * plain, (rule, float(measure), plain)
        # where converged flips: the first steps of the earlier cycles are measured too (SQUAREM's measures do not fall monotonically),
        # so the solve stops at the first of them below tol -- with margins, and for one rule at least at another step than without it
        tol = flip_tol(float(measure), plain)
        before = run(name)[:k + 1]
        j_r, m_r = first_stop([CR.stop_measure(e.A, e.th1, P.model.den, r, 3 * j)[0] for j, e in enumerate(before)], tol)
        j_p, m_p = first_stop([e.measure for e in before], tol)
        print("    tol %.6g: stops at cycle %s with the rule (margin %.3g), %s without (margin %.3g)" % (tol, j_r, m_r, j_p, m_p))
        assert j_r is not None and min(m_r, m_p) >= (np.sqrt(CR.GAP_MIN) - 1) / 2, (rule, j_r, j_p, m_r, m_p)
        shows.append(j_r != j_p)
    assert any(shows), shows                                  # (an earlier plain step can lie below a tol too: 40x80x228-s325, k = 10, count_floor)


LATE_CASE, LATE_PASSES = "ragged-s2", 2999


def test_the_late_point_of_the_abs_step_rule():
    """Past 1000 passes the abs_step bound shrinks like 1 / (passes + 1) of the set's own counter.  LATE_CASE after 2999 plain EM passes: of
    the class 0 cases that were searched by seed the one whose plain EM is slowest (the largest measure left).  choose_rules silences the
    component that decides the plain measure, and in a set of 60 transcripts that one moves most or has a neighbour within 0.1 %; so the
    bound is placed by choose_late_abs_step: in a gap between two moves, where the measure differs from the plain one and from what a
    bound frozen at pass 1000, three times larger, would give."""
    left = {}
    for name in [n for n in NAMES if CR.SET_CASES[n][0] == 0 and CR.SET_CASES[n][2] == 14]:
        m = CR.set_case(name).model
        A = m.start.astype(np.float64)
        for _ in range(LATE_PASSES):
            A = m.em(A)[0].astype(np.float64)
        left[name] = (float(m.plain(A, LATE_PASSES).measure), A)
    print({n: v[0] for n, v in left.items()})
    assert max(left, key=lambda n: left[n][0]) == LATE_CASE
    m, A = CR.set_case(LATE_CASE).model, left[LATE_CASE][1]
    c = m.plain(A, LATE_PASSES)
    r, gap, measure, frozen = CR.choose_late_abs_step(m, A, c.A_next, LATE_PASSES)
    margin = CR.stop_measure(A, c.A_next, m.den, r, LATE_PASSES)[1]
    print("abs_step %.6g gap %.4g margin %.3g: measure %.6g, plain %.6g, with the bound of pass 1000 %.6g" % (
        r.abs_step, gap, margin, float(measure), float(c.measure), float(frozen)))
    assert gap >= CR.GAP_MIN ** 2 and margin >= (np.sqrt(CR.GAP_MIN) - 1) / 2
    assert float(CR.abs_step_bound(r.abs_step, 0)) == pytest.approx(float(CR.abs_step_bound(r.abs_step, LATE_PASSES)) * 3.0, rel=1e-12)


# ---- the Newton step -------------------------------------------------------------------------------------------------------------------------

def test_newton_step_on_a_quadratic_like_problem_is_a_newton_step():
    """two transcripts, one shared row and reads of their own: the step solves (-H) d = g exactly in two CG iterations"""
    rp = np.array([0, 2, 3, 4], dtype=np.uint64)
    ci = np.array([0, 1, 0, 1], dtype=np.int32)
    m = CR.Model(2, rp, ci, np.array([30, 10, 20]), np.array([1.0, 2.0]))
    x = np.array([25.0, 18.0])
    o = CR.newton_step(m, x)
    S = x.sum()
    g = np.array([30 / S - 1 + 10 / x[0], 30 / S - 2 + 20 / x[1]])
    H = 30 / S ** 2 * np.ones((2, 2)) + np.diag([10 / x[0] ** 2, 20 / x[1] ** 2])
    d = np.linalg.solve(H, g)
    assert o.n_cg == 2 and not o.bound.any()
    assert np.allclose(o.z.astype(np.float64), d, rtol=1e-12)
    assert o.accepted and np.allclose(o.x_new.astype(np.float64), x + float(o.alpha) * d, rtol=1e-12)
    assert o.passes == 1 + o.n_cg + o.n_trials


def test_a_bound_component_goes_to_zero_and_stays():
    """a transcript without reads of its own that holds 1e-7 reads under a negative gradient is bound: 0 after a full step, and the EM
    step that follows leaves it there (its gradient at 0 stays negative: not re-opened)"""
    rp = np.array([0, 2, 3], dtype=np.uint64)
    ci = np.array([0, 1, 0], dtype=np.int32)
    m = CR.Model(2, rp, ci, np.array([5, 100]), np.array([1.0, 1.0]))
    o = CR.newton_step(m, np.array([104.0, 1e-7]))
    assert o.bound.tolist() == [False, True] and o.accepted and o.alpha == 1 and o.x_new[1] == 0 and o.y[1] == 0 and o.reopened == 0
    assert o.mask_margin > 0.5 and o.reopen_margin > 0.5
    # the same point with reads of its own: free
    rp2 = np.array([0, 2, 3, 4], dtype=np.uint64)
    m2 = CR.Model(2, rp2, np.array([0, 1, 0, 1], dtype=np.int32), np.array([5, 100, 1]), np.array([1.0, 1.0]))
    assert not CR.newton_step(m2, np.array([104.0, 1e-7])).bound.any()


@pytest.mark.parametrize("cls,case,when,ks", [(c, n, w, ks) for c, pts in CR.NEWTON_POINTS.items() for (n, w, ks) in pts])
def test_newton_float64_against_long_double(cls, case, when, ks):
    """at every point on the reference's own trajectory: where both precisions make the same choices and the long-double margins
    hold, the distance is within NEWTON_DIST_CAP; the first point, the one the device is checked at, is such a point.  Early and late
    points have an accepted step, the refused point has all four trial steps refused."""
    m = CR.set_case(case).model
    assert CR.SET_CASES[case][0] == cls
    pts = trajectory(case, max(ks))
    ok = []
    for k in ks:
        a, b = CR.newton_step(m, pts[k], CR.LD), CR.newton_step(m, pts[k], np.float64)
        same = (a.n_cg, a.n_trials, a.accepted) == (b.n_cg, b.n_trials, b.accepted)
        dist = max(CR.newton_distance(b.x_new, a.x_new, m.den), CR.newton_distance(b.y, a.y, m.den))
        print("%s k %d: %s | float64 the same choices: %s, distance %.3g" % (case, k, CR.newton_margins(a), same, dist))
        if same and CR.newton_comparable(a) and a.accepted == (when != "refused"):
            ok.append(k)
            assert dist <= CR.NEWTON_DIST_CAP, (k, dist)
            assert abs(float(a.measure) - float(b.measure)) <= 1e-9 * float(a.measure)
            if when == "late":                                # the late points are there for the bound components
                assert a.bound.any()
            if when == "refused":
                assert a.n_trials == 4 and np.array_equal(a.x_new, pts[k].astype(CR.LD))
    assert ks[0] in ok, (ks, ok)


# ---- replicates ------------------------------------------------------------------------------------------------------------------------------

BOOT_SEED, BOOT_N, BOOT_MIN = 9, 3, 3


@pytest.mark.parametrize("cls", list(RULE_CASES))
def test_replicates_have_checked_cycles(cls):
    """the drawn samples of the replicate test (the same draws on the host): at least BOOT_MIN cycles with margins from the start"""
    P = CR.set_case(RULE_CASES[cls])
    for b in range(BOOT_N):
        w = hip.bootstrap_draw_host(BOOT_SEED, b, np.where(P.E != 0, P.R, 0))
        m = CR.Model(P.n_tx, P.rp, P.ci, w, P.den, P.E)
        r = CR.longest_run(m, P.K)
        print("%s replicate %d: %d cycles %s" % (P.name, b, len(r), " ".join(c.kind for c in r)))
        assert len(r) >= BOOT_MIN
