"""GPU: every cycle of the streaming solve (set_mode 1) against the long-double reference of tests/cycle_reference.py, each cycle from
its own start point -- no trajectory is followed, so no error and no differing branch carries over.

emsar_hip_solve starts at the uniform point and is bit-reproducible in deterministic mode.  With a rule that cannot fire (tol 1e-300)
the solve with max_iter = 3 k returns exactly the point A_k that the solve with max_iter = 3 (k + 1) passes through; final_delta of the
latter is the stopping measure of the plain step A_k -> EM(A_k), loglik of the former is F(A_k).  The reference is started at the
device's A_k and must give the device's A_{k+1}.  The only hidden state is stepmax, a function of the decisions so far, which the
reference carries along; test_squarem_cycle_cpu.py shows that every decision of the K checked cycles has a margin.

Tolerances.  theta, per component, in reads:  |dtheta_t| den_t <= c_k (res + 1e-11 kappa_t theta_t den_t)
    res      N 2^-61 20000 in deterministic mode (the bound of the pass tests), 0 with floating atomics
    c_k      4 (1 + s)^2, s the reference's step: errors of th1 and th2 enter thx with the weights 2 s and s^2, one pass before, one after
    kappa_t  scale_t / thx_t, the cancellation of that component's extrapolation (1 where it kept th2, in a rejected cycle and without
             extrapolation); components with kappa_t > 1e4 are left out, at most 1 % per cycle
loglik: 1e-10 |F| + 1e-9.
final_delta: 1e-9 relative with floating atomics.  In deterministic mode the accumulators are fixed point (include/emsar_hip.h: a grid of
N 2^-61 reads, 1e-13 here), and the measure is decided by a transcript on its way to zero that holds 1e-6 reads or fewer: th1 of that
transcript, and with it the measure, is only known to 1e-9 .. 1e-4 relative.  The comparison there is against the interval that
cycle_reference.measure_interval derives from the grid (n / 2 + 1 grid steps for a transcript that n uploaded rows contribute to), plus the
same 1e-9; test_squarem_cycle_cpu.py restates the step with every contribution rounded to the grid and finds the distances seen on the
device (cfg3, one contribution per read as in the CSR kernel: 4.5e-5 relative; the device's CSR kernel: 4.7e-5).  Not a bug of the
stopping rule: with floating atomics the same comparison holds to 1e-15.

Worst ratio to the bound over the checked cycles of a case, MI355X (theta / final_delta / loglik; in brackets final_delta against a plain
1e-9 relative):
    deterministic      cfg3-tiled     6.7e-5 / 0.007 / 2.9e-6   (95)        cfg3-csr     0.013  / 0.14  / 1.6e-5  (4.7e4)
                       human-tiled    1.7e-4 / 0.007 / 3.6e-6   (101)       human-csr    0.0035 / 0.073 / 1.4e-5  (2.7e3)
                       human_w-tiled  1.3e-4 / 0.013 / 3.6e-6   (84)        human_w-csr  9.1e-4 / 0.047 / 7.2e-6  (770)
                       segments-tiled 3.8e-5 / 0.005 / 3.0e-4   (0.11)      segments-csr 2.8e-4 / 0.020 / 3.9e-4  (0.70)
                       shuffled-renumber 1.6e-4 / 0.049 / 2.9e-6 (99)       the knob cases of cfg3 and human: the figures of the tiled case
    floating atomics   cfg3 2.7e-4 / 3.2e-7 / 4.3e-6    human 8.7e-5 / 4.4e-7 / 3.6e-6    human_w 5.7e-4 / 1.6e-7 / 1.8e-6
                       segments 1.2e-3 / 7.1e-7 / 1.5e-4    human-csr 1.4e-3 / 1.1e-6 / 9.0e-6
    stopping rules     final_delta inside the interval with 0.0002 .. 0.018 of its width used; against 1e-9 relative 0.03 .. 361
So theta has three to four decimal digits of room, the likelihood three and more, and the measure six with floating atomics.

Each of these changes to the kernels fails the tests named (tried on an MI355X):
    no "- penx" in the acceptance test of k_update_p3       test_every_cycle_from_its_own_start, all problems but fast_slow
    a rejected cycle continues from thx                      the same
    no stepmax / 4 after a clamped rejection                 test_every_cycle_from_its_own_start[human*] (cycle 12 is clamped at 4, not 16)
    s > 1.0 instead of s > 1.01                              test_every_cycle_from_its_own_start[fast_slow-*], test_first_cycles_with_floating_atomics[fast_slow-tiled]
    penx summed from the words of pen1 (a wrong stride)      test_every_cycle_from_its_own_start[segments-*] (19 components keep th2 there)
    k_update_p2 writes delta1_bits as well                   test_every_cycle_from_its_own_start, test_stopping_rules_*
    abs_step bound from a pass count kept on the host        test_abs_step_bound_follows_the_device_side_pass_count
"""
import numpy as np
import pytest

from emsar_amd import EmsarHip
from emsar_amd.hip import LAYOUT_CSR, LAYOUT_TILED
from tests import cycle_reference as CR
from tests import pass_problems

pytestmark = pytest.mark.gpu

KNOBS = ("RENUMBER", "SQ_GRID", "UPDATE_GRID", "GRAPH", "DEBUG") + pass_problems.LAYOUT_KNOBS

# case -> problem, layout, knobs (read when the context is created), check_every
CASES = {
    "cfg3-tiled": ("cfg3", LAYOUT_TILED, {}, 8),
    "cfg3-csr": ("cfg3", LAYOUT_CSR, {}, 8),
    "human-tiled": ("human", LAYOUT_TILED, {}, 8),
    "human-csr": ("human", LAYOUT_CSR, {}, 8),
    "human_w-tiled": ("human_w", LAYOUT_TILED, {}, 8),
    "human_w-csr": ("human_w", LAYOUT_CSR, {}, 8),
    "segments-tiled": ("segments", LAYOUT_TILED, {}, 8),
    "segments-csr": ("segments", LAYOUT_CSR, {}, 8),
    # cycle 2 has s = 1.0049: between 1 and the switch at 1.01 (test_squarem_cycle_cpu.py shows what an extrapolation would move)
    "fast_slow-tiled": ("fast_slow", LAYOUT_TILED, {}, 8),
    "fast_slow-csr": ("fast_slow", LAYOUT_CSR, {}, 8),
    "shuffled-renumber": ("cfg3_family_shuffled", LAYOUT_TILED, dict(RENUMBER="2"), 8),
    # check_every 2: cycles 9 and up come from the replayed graph (solve.hpp: stream)
    "cfg3-graph": ("cfg3", LAYOUT_TILED, {}, 2),
    "human-graph": ("human", LAYOUT_TILED, {}, 2),
    # human has 12 workgroups of 256 transcripts: 1 and 3 make the kernels stride, 1000 is clamped to 12, the default (256) too
    "human-sq_grid_1": ("human", LAYOUT_TILED, dict(SQ_GRID="1"), 8),
    "human-sq_grid_3": ("human", LAYOUT_TILED, dict(SQ_GRID="3"), 8),
    "human-sq_grid_1000": ("human", LAYOUT_TILED, dict(SQ_GRID="1000"), 8),
    "human-update_grid_1": ("human", LAYOUT_TILED, dict(UPDATE_GRID="1"), 8),
}
PAIRS = [("cfg3-tiled", "cfg3-csr"), ("human-tiled", "human-csr"), ("human_w-tiled", "human_w-csr"), ("segments-tiled", "segments-csr"),
         ("fast_slow-tiled", "fast_slow-csr")]
FLOAT_CYCLES = 5

_solves, _cycles, _kinds = {}, {}, {}


def _context(monkeypatch, P, layout, knobs, det):
    for k in KNOBS:
        monkeypatch.delenv("EMSAR_HIP_" + k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("EMSAR_HIP_" + k, v)
    ctx = EmsarHip(0)
    try:
        ctx.set_deterministic(det)
        if P.collapse:
            rp, ci, w, _, _ = ctx.collapse_rows(P.n_tx, P.rp, P.ci)
            ctx.upload_structure(P.n_tx, rp, ci, layout)
            ctx.upload_sample(w, None, P.den)
        else:
            ctx.upload_structure(P.n_tx, P.rp, P.ci, layout)
            ctx.upload_sample(P.R, P.E, P.den)
    except Exception:
        ctx.close()
        raise
    return ctx


def _stream(ctx, **kw):
    th, st = ctx.solve(set_mode=1, tol=1e-300, **kw)
    assert st.converged == 0 or st.final_delta == 0.0
    return th, (st.iters, st.final_delta, st.loglik)


def prefixes(monkeypatch, case, det=True, K=None):
    """(theta, (iters, final_delta, loglik)) of the solves with max_iter = 3, 6, .. 3 K, from one context (cached)"""
    key = (case, det)
    if key not in _solves:
        name, layout, knobs, ce = CASES[case]
        P = CR.problem(name)
        with _context(monkeypatch, P, layout, knobs, det) as ctx:
            _solves[key] = [_stream(ctx, max_iter=3 * k, accel=1, check_every=ce) for k in range(1, (K or P.K) + 1)]
    return _solves[key]


def reference_cycle(P, A, stepmax, k):
    """the reference's cycle from the device's point (cached: cases whose knobs do not change the bits share it)"""
    key = (P.name, hash(A.tobytes()), stepmax, k)
    if key not in _cycles:
        _cycles[key] = P.model.cycle(A, stepmax, 3 * k)
    return _cycles[key]


def check_cycles(case, P, sols, det):
    """Every cycle from its own start.  Returns the kinds of the cycles."""
    m = P.model
    A, stepmax, kinds = m.start, 1.0, []
    worst = {"theta": 0.0, "delta": 0.0, "delta_1e-9": 0.0, "loglik": 0.0, "left_out": 0.0}
    for k, (th, (iters, delta, _)) in enumerate(sols):
        c = reference_cycle(P, A, stepmax, k)
        what = "%s cycle %d: %s" % (case, k + 1, CR.margins(c))
        assert iters == 3 * (k + 1), what
        # a condition, shown on the CPU for the reference's own trajectory: the decisions of the checked cycles have margins
        assert CR.comparable(c), "no margin: " + what
        bound, covered = CR.theta_bound(m, c, det)
        worst["left_out"] = max(worst["left_out"], float((~covered).mean()))
        assert (~covered).mean() <= CR.LEFT_OUT_MAX, what
        want = c.A_next.astype(np.float64)
        err = np.abs(th - want) * m.den
        ratio = float(np.max(np.where(covered & (err > 0), err / np.maximum(bound, 1e-300), 0.0)))
        worst["theta"] = max(worst["theta"], ratio)
        if ratio > 1.0:                         # which point DID the device continue from?
            other = {"EM(thx)": m.em(c.thx)[0], "th2": c.th2, "thx": c.thx, "th1": c.th1}
            near = {n: float(np.max(np.abs(th - v.astype(np.float64)) * m.den)) for n, v in other.items()}
            t = int(np.argmax(np.where(covered, err / np.maximum(bound, 1e-300), 0.0)))
            pytest.fail("%s\n  theta off by %.3g of its bound at t = %d (got %.17g want %.17g kappa %.3g); the reference continues from %s; "
                        "largest distance in reads from: %s" % (what, ratio, t, th[t], want[t], float(c.kappa[t]), "EM(thx)" if c.ok else "th2", near))
        measure = float(c.measure)
        lo, hi = CR.measure_interval(A, c.th1, m.den, CR.Rules(), 3 * k, P.dy if det else 0.0)
        worst["delta_1e-9"] = max(worst["delta_1e-9"], abs(delta - measure) / (1e-9 * measure))
        d_ratio = abs(delta - measure) / (1e-9 * measure + max(hi - measure, measure - lo))
        worst["delta"] = max(worst["delta"], d_ratio)
        assert lo - 1e-9 * measure <= delta <= hi + 1e-9 * measure, "%s\n  final_delta %.17g, the measure of the first step %.17g in [%.17g, %.17g]" % (
            what, delta, measure, lo, hi)
        if k > 0:                               # F at this cycle's start is the loglik of the solve that stopped there
            F, ll = float(c.F_A), sols[k - 1][1][2]
            worst["loglik"] = max(worst["loglik"], abs(ll - F) / (1e-10 * abs(F) + 1e-9))
            assert abs(ll - F) <= 1e-10 * abs(F) + 1e-9, (what, ll, F)
        kinds.append(c.kind)
        A, stepmax = th, c.stepmax_next
    F, ll = float(m.F(A)[0]), sols[-1][1][2]
    worst["loglik"] = max(worst["loglik"], abs(ll - F) / (1e-10 * abs(F) + 1e-9))
    assert abs(ll - F) <= 1e-10 * abs(F) + 1e-9, (case, ll, F)
    print("%s %s: %d cycles, worst ratio to the bound: theta %.3g final_delta %.3g (%.3g of 1e-9 relative) loglik %.3g; left out %.4f; kinds %s" % (
        case, "deterministic" if det else "floating atomics", len(sols), worst["theta"], worst["delta"], worst["delta_1e-9"], worst["loglik"], worst["left_out"],
        " ".join(kinds)))
    return kinds


# ---- a. every cycle from its own start, deterministic mode -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_every_cycle_from_its_own_start(monkeypatch, case):
    P = CR.problem(CASES[case][0])
    _kinds[case] = check_cycles(case, P, prefixes(monkeypatch, case), True)
    assert len(_kinds[case]) == P.K


@pytest.mark.parametrize("tiled,csr", PAIRS)
def test_tiled_and_csr_state_the_same_F_and_decide_alike(monkeypatch, tiled, csr):
    """The folded single-transcript term u log theta exists in TILED only."""
    P = CR.problem(CASES[tiled][0])
    a, b = prefixes(monkeypatch, tiled), prefixes(monkeypatch, csr)
    for c in (tiled, csr):
        if c not in _kinds:
            _kinds[c] = check_cycles(c, P, prefixes(monkeypatch, c), True)
    assert _kinds[tiled] == _kinds[csr]
    res = max(P.model.N, 1) * 2.0 ** -61 * 20000
    for k, ((th_a, (_, d_a, ll_a)), (th_b, (_, d_b, ll_b))) in enumerate(zip(a, b)):
        assert abs(ll_a - ll_b) <= 2 * (1e-10 * abs(ll_a) + 1e-9), (k + 1, ll_a, ll_b)
        if k == 0:                              # one plain cycle from the same start: the pass tests' bound, three passes
            assert np.all(np.abs(th_a - th_b) * P.model.den <= 3 * (res + 1e-11 * th_a * P.model.den))
            assert abs(d_a - d_b) <= 1e-9 * d_a


# ---- b. a few cycles with floating atomics ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["cfg3-tiled", "human-tiled", "human_w-tiled", "segments-tiled", "human-csr", "fast_slow-tiled"])
def test_first_cycles_with_floating_atomics(monkeypatch, case):
    P = CR.problem(CASES[case][0])
    kinds = check_cycles(case, P, prefixes(monkeypatch, case, det=False, K=min(FLOAT_CYCLES, P.K)), False)
    assert len(kinds) == min(FLOAT_CYCLES, P.K)


# ---- c. the stopping rules -------------------------------------------------------------------------------------------------------------

RULE_CASE = "human-tiled"
RULE_POINTS = (2, 10)          # as test_squarem_cycle_cpu.py


def _rule_kw(r):
    return dict(abs_floor=r.abs_floor, count_floor=r.count_floor, zero_cut=r.zero_cut, abs_step=r.abs_step)


def _check_rules(ctx, P, A, passes_done, accel, check_every, what):
    """rule values from the reference's step A -> EM(A); the device's final_delta of the solve that ends with that step"""
    m = P.model
    y = m.em(A)[0]
    rules = CR.choose_rules(m, A, y, passes_done)
    assert set(rules) == {"plain", "count_floor", "zero_cut", "abs_step"}, (what, list(rules))
    plain = float(rules["plain"][2])
    out = {}
    for name, (r, gap, measure) in rules.items():
        measure = float(measure)
        margin = CR.stop_measure(A, y, m.den, r, passes_done)[1]
        # conditions on the reference alone (the CPU test shows them for the reference's own trajectory)
        assert gap >= CR.GAP_MIN and measure > 0, (what, name, gap, measure)
        if name != "plain":
            assert abs(measure - plain) > (0.1 if name == "count_floor" else 1e-3) * plain, (what, name, measure, plain)
        _, (iters, delta, _) = _stream(ctx, max_iter=passes_done + (3 if accel else 1), accel=accel, check_every=check_every, **_rule_kw(r))
        lo, hi = CR.measure_interval(A, y, m.den, r, passes_done, P.dy)         # deterministic mode: the fixed-point grid
        width = max(hi - measure, measure - lo)
        ratio = abs(delta - measure) / (1e-9 * measure + width)
        print("%s %-11s gap %.4g margin %.3g: final_delta %.17g reference %.17g (grid: %.3g relative) plain %.6g, %.3g of the bound, %.3g of 1e-9" % (
            what, name, gap, margin, delta, measure, width / measure, plain, ratio, abs(delta - measure) / (1e-9 * measure)))
        assert iters == passes_done + (3 if accel else 1)
        if name != "plain":                     # what the grid leaves open is small against what the rule changes
            assert width <= 0.1 * abs(measure - plain), (what, name, width, measure, plain)
        assert lo - 1e-9 * measure <= delta <= hi + 1e-9 * measure, (what, name, delta, measure, lo, hi)
        out[name] = (r, gap, measure)
    return out


@pytest.mark.parametrize("k", RULE_POINTS)
def test_stopping_rules_squarem(monkeypatch, k):
    """final_delta is the measure of the cycle's first step under each rule: the later steps of the cycle do not overwrite it"""
    name, layout, knobs, ce = CASES[RULE_CASE]
    P = CR.problem(name)
    A = prefixes(monkeypatch, RULE_CASE)[k - 1][0]
    with _context(monkeypatch, P, layout, knobs, True) as ctx:
        _check_rules(ctx, P, A, 3 * k, 1, ce, "accel 1 after %d cycles" % k)


@pytest.mark.parametrize("k", RULE_POINTS)
def test_stopping_rules_plain_em(monkeypatch, k):
    """the same pass counts with accel = 0: the step after 3 k plain passes"""
    name, layout, knobs, ce = CASES[RULE_CASE]
    P = CR.problem(name)
    with _context(monkeypatch, P, layout, knobs, True) as ctx:
        A, _ = _stream(ctx, max_iter=3 * k, accel=0, check_every=ce)
        _check_rules(ctx, P, A, 3 * k, 0, ce, "accel 0 after %d passes" % (3 * k))


LATE_PASSES = 2999


def test_abs_step_bound_follows_the_device_side_pass_count(monkeypatch):
    """Beyond 1000 passes the abs_step bound shrinks like 1 / K, K counted by k_cycle_begin on the device.  Plain EM, check_every 2:
    the 3000th pass comes from a graph that was recorded at pass 9, where a bound computed on the host would have been frozen at
    K = 1000, three times too large.  The gap that holds the threshold is narrower than that factor (asserted), so such a bound silences
    the next deciding component too."""
    name, layout, knobs, _ = CASES[RULE_CASE]
    P = CR.problem(name)
    m = P.model
    with _context(monkeypatch, P, layout, knobs, True) as ctx:
        A, _ = _stream(ctx, max_iter=LATE_PASSES, accel=0, check_every=2)
        rules = _check_rules(ctx, P, A, LATE_PASSES, 0, 2, "accel 0 after %d passes" % LATE_PASSES)
    r, gap, measure = rules["abs_step"]
    frozen = float(CR.stop_measure(A, m.em(A)[0], m.den, r, 0)[0])
    print("abs_step %.6g gap %.4g: measure %.6g, with the bound of pass 1000 %.6g" % (r.abs_step, gap, measure, frozen))
    assert gap * CR.GAP_MIN < ((LATE_PASSES + 1) / 1000.0) ** 2, gap
    assert abs(frozen - measure) > 1e-3 * measure, (frozen, measure)


# ---- d. properties that need no reference point ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_loglik_never_falls_and_the_reads_are_distributed(monkeypatch, case):
    P = CR.problem(CASES[case][0])
    sols = prefixes(monkeypatch, case)
    ll = [s[1][2] for s in sols]
    for a, b in zip(ll, ll[1:]):
        assert b >= a - 1e-12 * abs(a), ll
    for th, _ in sols:
        assert np.isfinite(th).all() and (th >= 0).all()
        got = float(np.dot(th, P.model.den))
        assert abs(got - P.mass) <= 1e-9 * P.mass, (got, P.mass)
