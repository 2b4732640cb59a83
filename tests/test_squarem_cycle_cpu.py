"""CPU: the long-double cycle reference (tests/cycle_reference.py) alone, from the uniform start, on the problems and for the K cycles
that test_squarem_cycle_gpu.py checks on the device.  It shows that the GPU test is meaningful there: every discontinuous choice of
every checked cycle has a margin that two correct implementations cannot disagree about, and the checked cycles contain every kind.

Conditions per cycle (cycle_reference: F_MARGIN, S_MARGIN, Y_MARGIN, CLAMP_MARGIN, LEFT_OUT_MAX):
    acceptance        |F(thx) - F(th1)| >= 1e-9 of the sum of |terms| of both F
    s > 1.01          |s - 1.01| / s >= 1e-3
    interior          min |y_t| / scale_t >= 1e-7
    clamp             |s_raw - stepmax| / stepmax >= 1e-6  (FP64 sums of a few thousand terms agree to 1e-12)
    left out          at most 1 % of the components have a cancellation factor kappa_t > 1e4
Found (long double; K = 14 cfg3, 14 human, 9 segments, 11 cfg3_family_shuffled, 2 fast_slow): acceptance >= 4.8e-9 / 4.5e-9 / 2.2e-7 /
2.9e-9, s >= 0.39 where an extrapolation is made (fast_slow cycle 2: s = 1.0049, 0.005 below the switch), interior >= 7.1e-6 / 1.5e-6 /
2.1e-6 / 2.6e-5, clamp >= 0.055, left out <= 0.7 %.  One cycle more would break a condition on segments (2 % left out) and on
cfg3_family_shuffled (acceptance 1.6e-9 in cycle 12 is still above the bar, the choice there is caution)."""
import numpy as np
import pytest

from tests import cycle_reference as CR

NAMES = ["cfg3", "human", "segments", "cfg3_family_shuffled", "fast_slow"]         # human_w is human with its equal rows merged: the same model
_runs = {}


def run(name):
    """the reference's K cycles from the uniform start (cached)"""
    if name not in _runs:
        P = CR.problem(name)
        A, stepmax, out = P.model.start, 1.0, []
        for k in range(P.K):
            c = P.model.cycle(A, stepmax, 3 * k)
            out.append(c)
            A, stepmax = c.A_next, c.stepmax_next
        _runs[name] = out
    return _runs[name]


def test_scatter_by_sorting_is_the_scatter():
    """ld_pass scatters by np.add.reduceat over the entries sorted by id; the plain statement is np.add.at"""
    P = CR.problem("segments")
    m = P.model
    th = np.random.default_rng(5).uniform(0.1, 3.0, size=m.n_tx) * (m.den > 0)
    got, ll, ll_abs = m.em(th)
    n = np.diff(m.rp.astype(np.int64))
    S = np.add.reduceat(np.append(th.astype(CR.LD)[m.ci], CR.LD(0)), m.rp[:-1].astype(np.int64))
    S[n == 0] = 0
    live = (m.w > 0) & (S > 0)
    q = np.zeros(m.n_rows, dtype=CR.LD)
    q[live] = m.w[live] / S[live]
    acc = np.zeros(m.n_tx, dtype=CR.LD)
    np.add.at(acc, m.ci, np.repeat(q, n))
    want = np.where(m.den > 0, th * acc / np.where(m.den > 0, m.den, 1).astype(CR.LD), 0)
    assert np.all(np.abs(got - want) <= 1e-17 * np.abs(want))
    assert abs(ll - np.sum(m.w[live] * np.log(S[live]))) <= 1e-17 * ll_abs
    assert abs(float(np.sum(got * m.den)) - P.mass) <= 1e-12 * P.mass      # an EM step distributes the reads


@pytest.mark.parametrize("name", NAMES)
def test_every_checked_cycle_has_margins(name):
    P = CR.problem(name)
    worst = dict(F=np.inf, s=np.inf, y=np.inf, clamp=np.inf, left_out=0.0)
    for k, c in enumerate(run(name)):
        left_out = float((c.kappa > CR.KAPPA_MAX).mean())
        print("%s cycle %2d %s left out %.4f" % (name, k + 1, CR.margins(c), left_out))
        assert c.F_margin >= CR.F_MARGIN, (k + 1, CR.margins(c))
        assert c.s_margin >= CR.S_MARGIN, (k + 1, CR.margins(c))
        assert c.y_margin >= CR.Y_MARGIN, (k + 1, CR.margins(c))
        assert c.clamp_margin >= CR.CLAMP_MARGIN, (k + 1, CR.margins(c))
        assert CR.comparable(c)
        assert left_out <= CR.LEFT_OUT_MAX, (k + 1, left_out)
        worst = dict(F=min(worst["F"], c.F_margin), s=min(worst["s"], c.s_margin), y=min(worst["y"], c.y_margin),
                     clamp=min(worst["clamp"], c.clamp_margin), left_out=max(worst["left_out"], left_out))
    print(name, "K", P.K, "worst", worst)


def test_the_checked_cycles_contain_every_kind():
    kinds = {name: [c.kind for c in run(name)] for name in NAMES}
    print(kinds)
    for kind in ("plain", "accepted_free", "accepted_clamped", "rejected_free", "rejected_clamped"):
        assert any(kind in ks for ks in kinds.values()), kind
    for name in NAMES:
        assert kinds[name][0] == "plain"                     # stepmax starts at 1: the first cycle cannot extrapolate
    assert any(c.kept.any() for name in NAMES for c in run(name))
    # the step bounds move in both directions, visibly: a clamped rejection after which the bound IS smaller (max(1, 4 / 4) x 4 = 4
    # would hide a missing division), and a clamped acceptance after which it is larger
    shrunk = [(n, k + 1) for n in NAMES for k, c in enumerate(run(n)) if c.kind == "rejected_clamped" and c.stepmax_next < float(c.stepmax)]
    grown = [(n, k + 1) for n in NAMES for k, c in enumerate(run(n)) if c.kind == "accepted_clamped" and c.stepmax_next > float(c.stepmax)]
    assert shrunk and grown, (shrunk, grown)
    # ... and a later cycle of the same run is clamped at the smaller bound, so that a bound that never shrank gives another point
    assert any(run(n)[k].clamped and run(n)[k].extrap for n, k in shrunk if k < len(run(n))), shrunk


def test_a_step_between_1_and_1_01_is_not_extrapolated_and_it_shows():
    """fast_slow, cycle 2: s = 1.0049.  No extrapolation is made; had one been made (a switch at 1.0), the next point would be far
    outside the bound of the GPU test, with and without the deterministic mode's resolution."""
    P = CR.problem("fast_slow")
    c = run("fast_slow")[1]
    assert not c.extrap and 1.001 < float(c.s_raw) < 1.009 and float(c.stepmax) == 4.0, CR.margins(c)
    alt = P.model.cycle(c.A, 4.0, 3, s_switch="1.0")
    assert alt.extrap and alt.ok and alt.s == c.s
    for det in (True, False):
        bound, covered = CR.theta_bound(P.model, c, det)
        off = np.abs(alt.A_next - c.A_next).astype(np.float64) * P.model.den
        ratio = float(np.max(np.where(covered, off / np.maximum(bound, 1e-300), 0)))
        print("extrapolating at s = %.5f moves the next point by %.3g of the bound (%s)" % (float(c.s), ratio, "deterministic" if det else "floating"))
        assert ratio >= 100.0


@pytest.mark.parametrize("name", NAMES)
def test_F_never_falls(name):
    P = CR.problem(name)
    cycles = run(name)
    F = [float(c.F_A) for c in cycles] + [float(P.model.F(cycles[-1].A_next)[0])]
    assert all(b >= a for a, b in zip(F, F[1:])), F
    for c in cycles:                                          # every point distributes the same reads
        assert abs(P.model.reads(c.A_next) - P.mass) <= 1e-12 * P.mass


def test_step_bound_arithmetic():
    """stepmax_next of the four extrapolating kinds, as k_update_p3 states it"""
    seen = {}
    for name in NAMES:
        for c in run(name):
            seen.setdefault(c.kind, []).append((float(c.s), float(c.stepmax), c.stepmax_next))
    for s, sm, nxt in seen["accepted_free"] + seen["rejected_free"]:
        assert s < sm and nxt == sm
    for s, sm, nxt in seen["accepted_clamped"]:
        assert s == sm and nxt == 4 * sm
    for s, sm, nxt in seen["rejected_clamped"]:
        assert s == sm and nxt == (4.0 if sm <= 4 else sm / 4)
    assert seen["plain"][0] == (1.0, 1.0, 4.0)


# ---- the stopping rule: the values test_squarem_cycle_gpu.py derives at its two prefix points of "human" ---------------------------------

RULE_POINTS = (2, 10)          # prefix solves of 2 and of 10 cycles: the measured step is the first of cycle 3 and of cycle 11


@pytest.mark.parametrize("k", RULE_POINTS)
def test_rule_values_are_far_from_every_threshold(k):
    P = CR.problem("human")
    c = run("human")[k]                                       # the cycle that starts at A_k
    rules = CR.choose_rules(P.model, c.A, c.th1, 3 * k)
    plain = rules["plain"][2]
    assert abs(float(plain) - float(c.measure)) <= 1e-15 * float(plain)
    assert set(rules) == {"plain", "count_floor", "zero_cut", "abs_step"}
    for name, (r, gap, measure) in rules.items():
        m2, margin, _, _ = CR.stop_measure(c.A, c.th1, P.model.den, r, 3 * k)
        print("k %d %-11s gap %.4g measure %.6g (plain %.6g) margin %.3g" % (k, name, gap, float(measure), float(plain), margin))
        assert m2 == measure and measure > 0
        if name == "plain":
            continue
        assert gap >= CR.GAP_MIN, (name, gap)
        assert margin >= (np.sqrt(CR.GAP_MIN) - 1) / 2, (name, margin)                # the midpoint of a gap of 1.01 is 0.5 % from both ends
        assert abs(float(measure) - float(plain)) > (0.1 if name == "count_floor" else 1e-3) * float(plain), (name, float(measure), float(plain))


@pytest.mark.parametrize("k", RULE_POINTS)
def test_rule_values_after_plain_passes(k):
    """the same for accel = 0: the step after 3 k plain EM passes"""
    m = CR.problem("human").model
    A = m.start.astype(CR.LD)
    for _ in range(3 * k):
        A = m.em(A)[0]
    c = m.plain(A, 3 * k)
    rules = CR.choose_rules(m, A, c.A_next, 3 * k)
    plain = float(rules["plain"][2])
    assert plain == float(c.measure) and set(rules) == {"plain", "count_floor", "zero_cut", "abs_step"}
    for name, (r, gap, measure) in rules.items():
        margin = CR.stop_measure(A, c.A_next, m.den, r, 3 * k)[1]
        print("%d passes %-11s gap %.4g measure %.6g (plain %.6g) margin %.3g" % (3 * k, name, gap, float(measure), plain, margin))
        assert gap >= CR.GAP_MIN and measure > 0, (name, gap)
        if name != "plain":
            assert margin >= (np.sqrt(CR.GAP_MIN) - 1) / 2, (name, margin)
            assert abs(float(measure) - plain) > (0.1 if name == "count_floor" else 1e-3) * plain, (name, float(measure), plain)


@pytest.mark.parametrize("name,cycle", [("human", 3), ("cfg3_family_shuffled", 2), ("cfg3", 12)])
def test_fixed_point_grid_moves_the_measure_by_more_than_1e_9(name, cycle):
    """Why final_delta is compared at 1e-9 only with floating atomics.  The measure is decided by a transcript that is falling to zero
    and holds 1e-6 reads or fewer, and deterministic mode rounds every row's contribution to a grid of N 2^-61 = 1e-13 reads: the same
    step restated with that rounding (one contribution per read, as the CSR kernel adds them) gives a measure 1e-9 .. 1e-7 away from
    the exact one, inside the interval of measure_interval."""
    P = CR.problem(name)
    m = P.model
    c = run(name)[cycle - 1]
    grid = CR.LD(2.0) ** (int(np.frexp(m.N + 1.0)[1]) - 61)
    n = np.diff(m.rp.astype(np.int64))
    S = np.add.reduceat(np.append(c.A[m.ci], CR.LD(0)), m.rp[:-1].astype(np.int64))
    rows = np.repeat(np.arange(m.n_rows), n)
    live = (m.w > 0) & (S > 0)
    one = np.where(live[rows], c.A[m.ci] / np.where(live, S, 1)[rows], 0)        # the mass one read of the row gives the transcript
    mass = np.zeros(m.n_tx, dtype=CR.LD)
    np.add.at(mass, m.ci, m.w[rows] * np.rint(one / grid) * grid)
    y_q = np.where(m.den > 0, mass / np.where(m.den > 0, m.den, 1), 0)
    assert np.all(np.abs(y_q - c.th1) <= P.dy)
    got = float(CR.stop_measure(c.A, y_q, m.den, CR.Rules(), 0)[0])
    lo, hi = CR.measure_interval(c.A, c.th1, m.den, CR.Rules(), 0, P.dy)
    want = float(c.measure)
    print("%s cycle %d: measure %.17g, with the contributions on the grid %.17g: %.3g relative; interval %.3g below, %.3g above" % (
        name, cycle, want, got, abs(got - want) / want, (want - lo) / want, (hi - want) / want))
    assert lo <= got <= hi
    assert abs(got - want) > 1e-9 * want
    assert hi - lo <= 2e-3 * want                    # n / 2 grid steps for a transcript of n reads: the widest is cfg3's, 4000 reads each
    assert CR.measure_interval(c.A, c.th1, m.den, CR.Rules(), 0, 0.0) == (want, want)


def test_measure_rules_one_by_one():
    """stop_measure on five components with known terms"""
    den = np.array([2.0, 2.0, 2.0, 2.0, 0.0])
    x = np.array([1.0, 1e-3, 4.0, 2e-7, 0.0])
    y = np.array([0.5, 2e-3, 4.1, 1e-7, 0.0])
    f = lambda **kw: float(CR.stop_measure(x, y, den, CR.Rules(**kw), 0)[0])
    assert f() == pytest.approx(0.5 / (0.5 + 1e-6), rel=1e-15)
    assert f(abs_floor=0.5) == pytest.approx(0.5, rel=1e-15)
    assert f(count_floor=3.0) == pytest.approx(0.5 / 2.0, rel=1e-15)                  # floor 3 / 2 reads on every component
    assert f(zero_cut=0.6) == pytest.approx(1e-3 / (2e-3 + 1e-6), rel=1e-15)          # the rising component is not cut
    assert f(zero_cut=0.4) == pytest.approx(0.5 / (0.5 + 1e-6), rel=1e-15)
    # abs_step 1e-3: bound 0.2 up to pass 1000 silences all but the first; at pass 4000 the bound is 0.05
    assert f(abs_step=1e-3) == pytest.approx(0.5 / (0.5 + 1e-6), rel=1e-15)
    assert f(abs_step=3e-3) == 0.0
    assert float(CR.abs_step_bound(1e-3, 999)) == pytest.approx(0.2, rel=1e-15)
    assert float(CR.abs_step_bound(1e-3, 3999)) == pytest.approx(0.05, rel=1e-15)
    assert float(CR.stop_measure(x, y, den, CR.Rules(abs_step=3e-3), 3999)[0]) == pytest.approx(0.5 / (0.5 + 1e-6), rel=1e-15)
