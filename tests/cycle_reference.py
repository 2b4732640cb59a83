"""A long-double restatement of one cycle of the streaming solve (solve.hpp: enqueue_cycles; kernels_vector.hpp: k_update,
k_cycle_begin, k_update_p2, k_sq_extrap_ll, k_update_p3), CPU only.  test_squarem_cycle_cpu.py runs it alone, test_squarem_cycle_gpu.py
starts it at the device's own points, test_pass_kernels_gpu.py uses its EM pass.

One SQUAREM cycle from A with the step bound stepmax, as the comments above em_new_theta state it:
    th1 = EM(A), th2 = EM(th1), r = th1 - A, v = (th2 - th1) - r
    s = |r| / |v| (1 where v = 0), clamped to [1, stepmax]; an extrapolation is made iff s > 1.01
    y = A + 2 s r + s^2 v; thx_t = y_t where y_t > 0 and th2_t > 0, else th2_t (the component keeps th2); no extrapolation: thx = th2
    accepted iff no extrapolation was made or F(thx) >= F(th1), F = sum w log S + sum w log E - sum theta den
    A_next = accepted ? EM(thx) : th2
    rejected and s >= stepmax: stepmax = max(1, stepmax / 4); then (accepted ? s : 1) >= stepmax: stepmax *= 4   (s counts as 1 where
    no extrapolation was made)
The stopping rule is measured on the first step A -> th1 (k_update with to_delta1):
    d_t = |th1_t - A_t| / (|th1_t| + max(abs_floor, count_floor / den_t))
    d_t = 0 where th1_t < zero_cut and th1_t <= A_t, and where |th1_t - A_t| < abs_step * 2e5 / max(passes done + 1, 1000)
    measure = max d_t
Every discontinuous choice comes with its margin, so that a caller can tell a wrong decision from one that has no margin."""
import numpy as np

LD = np.longdouble


def _scatter_plan(p):
    """the entries of the CSR sorted by id, for a scatter by np.add.reduceat (np.add.at is ten times slower in long double)"""
    plan = getattr(p, "_scatter_plan", None)
    if plan is None:
        order = np.argsort(p.ci, kind="stable")
        ids = p.ci[order]
        starts = np.flatnonzero(np.append(True, ids[1:] != ids[:-1])) if len(ids) else np.zeros(0, dtype=np.int64)
        plan = p._scatter_plan = (order, starts, ids[starts])
    return plan


def ld_pass(p, w, den, th):
    """One EM pass in long double: S by add.reduceat, w / S, acc by scattering; returns (theta', sum w log S, sum |w log S|).
    p: rp, ci, n_rows, n_tx; w: what a row counts (int64, 0 outside F); den: float64."""
    n = np.diff(p.rp.astype(np.int64))
    x = th.astype(LD)
    S = np.add.reduceat(np.append(x[p.ci], LD(0)), p.rp[:-1].astype(np.int64))
    S[n == 0] = 0
    live = (w > 0) & (S > 0)
    q = np.zeros(p.n_rows, dtype=LD)
    q[live] = w[live].astype(LD) / S[live]
    acc = np.zeros(p.n_tx, dtype=LD)
    order, starts, ids = _scatter_plan(p)
    if len(starts):
        acc[ids] = np.add.reduceat(np.repeat(q, n)[order], starts)
    d = den.astype(LD)
    out = np.where(den > 0, x * acc / np.where(den > 0, d, 1), 0)
    terms = w[live].astype(LD) * np.log(S[live])
    return out, np.sum(terms), np.sum(np.abs(terms))


class Rules:
    """The parameters of k_update's stopping rule (emsar_em_params)."""

    def __init__(self, abs_floor=1e-6, count_floor=0.0, zero_cut=0.0, abs_step=0.0):
        self.abs_floor, self.count_floor, self.zero_cut, self.abs_step = abs_floor, count_floor, zero_cut, abs_step


def abs_step_bound(abs_step, passes_done):
    """k_cycle_begin: the bound on |dtheta| at the cycle that begins after passes_done passes"""
    return LD(abs_step) * LD(2e5) / LD(max(passes_done + 1, 1000)) if abs_step > 0.0 else LD(0)


def stop_measure(x, y, den, rules, passes_done):
    """The stopping measure of the step x -> y.  Returns (measure, margin, d, move): margin is the smallest relative distance from the
    zero_cut and abs_step thresholds of the components that decide the maximum (the one that holds it, and every silenced one that would
    hold it otherwise); d the per-component terms after the rules, move = |y - x|."""
    x, y = x.astype(LD), y.astype(LD)
    fl = np.full(len(x), LD(rules.abs_floor))
    if rules.count_floor > 0.0:
        pos = den > 0
        fl[pos] = np.maximum(fl[pos], LD(rules.count_floor) / den[pos].astype(LD))
    move = np.abs(y - x)
    raw = move / (np.abs(y) + fl)
    bound = abs_step_bound(rules.abs_step, passes_done)
    cut = LD(rules.zero_cut)
    by_cut = (y < cut) & (y <= x)
    by_step = move < bound
    d = np.where(by_cut | by_step, LD(0), raw)
    measure = d.max() if len(d) else LD(0)
    margin = np.inf
    top = int(np.argmax(d)) if len(d) else -1
    if top >= 0 and measure > 0:
        if cut > 0 and y[top] <= x[top]:
            margin = min(margin, float((y[top] - cut) / cut))
        if bound > 0:
            margin = min(margin, float((move[top] - bound) / bound))
    hidden = (raw > measure) & (by_cut | by_step)
    if hidden.any():
        m = np.full(len(x), -np.inf)            # a hidden component comes back when it leaves EVERY rule that silences it
        if cut > 0:
            m = np.where(by_cut, np.maximum(m, ((cut - y) / cut).astype(np.float64)), m)
        if bound > 0:
            m = np.where(by_step, np.maximum(m, ((bound - move) / bound).astype(np.float64)), m)
        margin = min(margin, float(m[hidden].min()))
    return measure, margin, d, move


def measure_interval(x, y, den, rules, passes_done, dy):
    """The interval that holds the measure of the step x -> y when every y_t is known to dy_t only (deterministic mode: the fixed-point
    grid of the accumulators): d_t = |y_t - x_t| / (|y_t| + floor_t) moves by at most (1 + d_t) dy_t / (|y_t| + floor_t), and the
    maximum lies between the largest lower and the largest upper end.  Silenced components stay silenced (their margins are the
    caller's to check).  dy = 0 gives (measure, measure)."""
    x, y = x.astype(LD), y.astype(LD)
    _, _, d, _ = stop_measure(x, y, den, rules, passes_done)
    fl = np.full(len(x), LD(rules.abs_floor))
    if rules.count_floor > 0.0:
        pos = den > 0
        fl[pos] = np.maximum(fl[pos], LD(rules.count_floor) / den[pos].astype(LD))
    a = np.where(d > 0, (1 + d) * dy / (np.abs(y) + fl), 0)
    return float(np.max(d - a)), float(np.max(d + a))


def fixed_point_dy(total_weight, contributions, den):
    """Deterministic mode keeps the reads assigned to a transcript in fixed point, at a grid of N 2^-61 reads rounded up to a power of
    two (include/emsar_hip.h, set_fx_scales): at most 2 (N + 1) 2^-61.  Every contribution is rounded to the grid once, so a
    transcript that n rows contribute to is within (n / 2 + 1) grid steps of the exact sum, in theta: that over den."""
    grid = 2.0 * (total_weight + 1) * 2.0 ** -61
    return np.where(den > 0, (contributions / 2.0 + 1.0) * grid / np.where(den > 0, den, 1.0), 0.0)


class Cycle:
    """What one cycle computed (attributes; see cycle())."""


class Model:
    """A sample as the likelihood sees it: the CSR (rp, ci), what each row counts (w, 0 for rows outside F), den, and
    const = sum w log E over the rows inside F."""

    def __init__(self, n_tx, rp, ci, w=None, den=None, E=None):
        self.n_tx = int(n_tx)
        self.rp, self.ci = np.ascontiguousarray(rp, dtype=np.uint64), np.ascontiguousarray(ci, dtype=np.int32)
        self.n_rows = len(self.rp) - 1
        n = np.diff(self.rp.astype(np.int64))
        w = np.ones(self.n_rows, dtype=np.int64) if w is None else np.array(w, dtype=np.int64)
        self.const = LD(0)
        if E is not None:
            w[np.asarray(E) == 0] = 0
            inside = w > 0
            self.const = np.sum(w[inside].astype(LD) * np.log(np.asarray(E)[inside].astype(LD)))
        if den is None:                         # the E-scatter, as upload_sample computes it
            den = np.zeros(self.n_tx)
            np.add.at(den, self.ci, np.repeat(np.ones(self.n_rows) if E is None else np.asarray(E, dtype=np.float64), n))
        self.w, self.den = w, np.ascontiguousarray(den, dtype=np.float64)
        self.N = int(w.sum())
        self.start = np.where(self.den > 0, 1.0, 0.0)          # k_fill_start

    def em(self, th):
        return ld_pass(self, self.w, self.den, th)

    def F(self, th):
        """(F, sum of |terms|) in long double, F as Case.loglik of test_pass_kernels_gpu.py states it"""
        _, ll, ll_abs = self.em(th)
        pen = th.astype(LD) * self.den.astype(LD)
        return ll + self.const - np.sum(pen), ll_abs + np.sum(np.abs(pen))

    def reads(self, th):
        return float(np.sum(th.astype(LD) * self.den.astype(LD)))

    def plain(self, A, pass_index, rules=None):
        """One plain EM step (accel = 0): A_next, F(A), the stopping measure of the step and its margin."""
        c = Cycle()
        c.A = A = A.astype(LD)
        c.A_next, ll0, _ = self.em(A)
        c.F_A = ll0 + self.const - np.sum(A * self.den.astype(LD))
        c.measure, c.measure_margin, c.d, c.move = stop_measure(A, c.A_next, self.den, rules or Rules(), pass_index)
        return c

    def cycle(self, A, stepmax, pass_index, rules=None, s_switch="1.01"):
        """One SQUAREM cycle from A (any float type) with the step bound stepmax, after pass_index passes.  s_switch: the step above
        which an extrapolation is made (another value only to show what a cycle with another switch would give)."""
        c = Cycle()
        den = self.den.astype(LD)
        c.A = A = A.astype(LD)
        c.th1, ll0, _ = self.em(A)
        c.F_A = ll0 + self.const - np.sum(A * den)
        c.measure, c.measure_margin, c.d, c.move = stop_measure(A, c.th1, self.den, rules or Rules(), pass_index)
        c.th2, ll1, ll1_abs = self.em(c.th1)
        c.r = c.th1 - A
        c.v = (c.th2 - c.th1) - c.r
        c.sr2, c.sv2 = np.sum(c.r * c.r), np.sum(c.v * c.v)
        c.s_raw = np.sqrt(c.sr2 / c.sv2) if c.sv2 > 0 else LD(1)
        c.stepmax = LD(stepmax)
        c.s = min(max(c.s_raw, LD(1)), c.stepmax)
        c.clamped = bool(c.s_raw >= c.stepmax)
        c.extrap = bool(c.s > LD(s_switch))
        c.s_margin = float(abs(c.s - LD(s_switch)) / c.s)
        # the clamp is a choice too: s_raw against stepmax decides whether the step bounds move
        c.clamp_margin = float(abs(c.s_raw - c.stepmax) / c.stepmax) if c.extrap else np.inf
        one = np.ones(self.n_tx, dtype=LD)
        c.kept = np.zeros(self.n_tx, dtype=bool)
        c.kappa, c.y_margin = one, np.inf
        if c.extrap:
            y = A + 2 * c.s * c.r + c.s * c.s * c.v
            c.scale = np.abs(A) + 2 * c.s * np.abs(c.r) + c.s * c.s * np.abs(c.v)
            inside = c.th2 > 0
            c.kept = inside & ~(y > 0)
            c.thx = np.where(inside & (y > 0), y, c.th2)
            if inside.any():
                c.y_margin = float(np.min(np.abs(y[inside]) / c.scale[inside]))
            took = inside & (y > 0)
            c.kappa = np.where(took, c.scale / np.where(took, c.thx, 1), one)
        else:
            c.thx, c.scale = c.th2, np.abs(c.th2)
        th3, llx, llx_abs = self.em(c.thx)
        pen1, penx = c.th1 * den, c.thx * den
        c.F_th1, c.F_thx = ll1 + self.const - np.sum(pen1), llx + self.const - np.sum(penx)
        c.F_terms = ll1_abs + np.sum(np.abs(pen1)) + llx_abs + np.sum(np.abs(penx))
        c.F_margin = float(abs(c.F_thx - c.F_th1) / c.F_terms) if c.extrap else np.inf
        c.ok = bool(not c.extrap or c.F_thx >= c.F_th1)
        c.A_next = th3 if c.ok else c.th2
        if not c.ok:
            c.kappa = one                        # th2 does not depend on the extrapolation
        s_used = c.s if c.extrap else LD(1)
        sm = c.stepmax
        if not c.ok and s_used >= sm:
            sm = max(LD(1), sm / 4)
        if (s_used if c.ok else LD(1)) >= sm:
            sm = sm * 4
        c.stepmax_next = float(sm)
        c.kind = "plain" if not c.extrap else ("accepted" if c.ok else "rejected") + ("_clamped" if c.clamped else "_free")
        return c


# the conditions under which a cycle's decisions can be compared between two implementations (test_squarem_cycle_cpu.py asserts them
# of the reference alone, test_squarem_cycle_gpu.py ends a case's run of checked cycles where one fails)
F_MARGIN, S_MARGIN, Y_MARGIN, CLAMP_MARGIN, KAPPA_MAX, LEFT_OUT_MAX = 1e-9, 1e-3, 1e-7, 1e-6, 1e4, 0.01


def comparable(c):
    return c.F_margin >= F_MARGIN and c.s_margin >= S_MARGIN and c.y_margin >= Y_MARGIN and c.clamp_margin >= CLAMP_MARGIN


def margins(c):
    return "kind %s s_raw %.6g s %.6g stepmax %.6g | margins: F %.3g s %.3g y %.3g clamp %.3g | kept %d kappa>%.0e %d" % (
        c.kind, float(c.s_raw), float(c.s), float(c.stepmax), c.F_margin, c.s_margin, c.y_margin, c.clamp_margin, int(c.kept.sum()),
        KAPPA_MAX, int((c.kappa > KAPPA_MAX).sum()))


def theta_bound(model, c, deterministic):
    """Per component, in reads: c_k (res + 1e-11 kappa_t theta_t den_t), c_k = 4 (1 + s)^2; and the components it covers
    (kappa_t <= KAPPA_MAX)."""
    res = max(model.N, 1) * 2.0 ** -61 * 20000 if deterministic else 0.0
    s = float(c.s) if c.extrap else 1.0
    ck = 4.0 * (1.0 + s) ** 2
    kappa = c.kappa.astype(np.float64)
    want = c.A_next.astype(np.float64)
    return ck * (res + 1e-11 * kappa * want * model.den), kappa <= KAPPA_MAX


# ---- the problems of the two cycle tests, and the rule values of the stopping-rule test ------------------------------------------------

class Problem:
    """What a test uploads (rp, ci, R, E, den as upload_sample takes them; collapse: the device collapses the rows first and their
    counts become R), the reference's model of the same sample, and K, the cycles that are checked."""

    def __init__(self, name, K, n_tx, rp, ci, R=None, E=None, den=None, collapse=False, structure="window"):
        from emsar_amd import synth
        self.name, self.K, self.n_tx, self.rp, self.ci, self.R, self.E, self.den = name, K, int(n_tx), rp, ci, R, E, den
        self.collapse, self.structure = collapse, structure
        if R is None:                           # the same likelihood with equal rows merged: a shorter sum for the reference
            mrp, mci, cnt = synth.collapse(rp, ci)
            self.model = Model(n_tx, mrp, mci, cnt, den, E)
        else:
            self.model = Model(n_tx, rp, ci, R, den, E)
        m = self.model
        S = np.add.reduceat(np.append(m.start[m.ci], 0.0), m.rp[:-1].astype(np.int64))
        S[np.diff(m.rp.astype(np.int64)) == 0] = 0
        self.mass = int(m.w[S > 0].sum())       # the reads an EM step distributes
        # deterministic mode: what the fixed-point accumulators leave open in theta (the rows as uploaded: each adds once)
        up_ci, total = (m.ci, int(m.w.sum())) if (collapse or R is not None) else (np.asarray(ci), len(rp) - 1)
        if R is not None:
            total = int(np.asarray(R, dtype=np.int64).sum())
        self.dy = fixed_point_dy(total, np.bincount(up_ci, minlength=self.n_tx), m.den)


def _cfg3(structure, K):
    from emsar_amd import synth
    s = synth.make_config("cfg3", 0.004, structure)
    return Problem("cfg3" if structure == "window" else "cfg3_" + structure, K, s["n_tx"], s["row_ptr"], s["col_idx"], den=s["den"], structure=structure)


def _human(collapse, K):
    from emsar_amd import synth
    s = synth.make_matrix(n_tx=3000, n_reads=200000, law="human", xfam=0.02, seed=21)
    return Problem("human_w" if collapse else "human", K, s["n_tx"], s["row_ptr"], s["col_idx"], den=s["den"], collapse=collapse)


def _segments(K):
    from tests import pass_problems
    p = pass_problems.problem("segments")
    return Problem("segments", K, p.n_tx, p.rp, p.ci, R=p.R, E=p.E)


def _fast_slow(K):
    """A sample whose second cycle has a step between 1 and 1.01 (s = 1.0049), with something to lose if it were extrapolated.
    64 pairs of abundant transcripts (about 1000 reads each of their own, 0.5 % of them shared: EM contracts by 0.005 per pass there,
    and den = 1e-5 puts their optimum at 1e8, far from the start) carry |r| and |v|; 64 pairs of rare ones (2-8 reads of their own,
    8-13 shared: contraction about 0.5) start within 30 % of their optimum and are what an extrapolation would move."""
    rng = np.random.default_rng(3)
    rows, w, den = [], [], np.zeros(256)
    for i in range(0, 128, 2):
        U1, U2 = int(rng.integers(800, 1200)), int(rng.integers(800, 1200))
        rows += [[i], [i + 1], [i, i + 1]]
        w += [U1, U2, max(1, int(0.005 * (U1 + U2)))]
        den[i], den[i + 1] = 1e-5, 1e-5
    for i in range(128, 256, 2):
        u1, u2, m = int(rng.integers(2, 9)), int(rng.integers(2, 9)), int(rng.integers(8, 14))
        rows += [[i], [i + 1], [i, i + 1]]
        w += [u1, u2, m]
        den[i] = (u1 + m / 2) * (1 + 0.3 * rng.uniform(-1, 1))
        den[i + 1] = (u2 + m / 2) * (1 + 0.3 * rng.uniform(-1, 1))
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return Problem("fast_slow", K, 256, rp, np.concatenate(rows).astype(np.int32), R=np.array(w, dtype=np.int32), den=den)


# K: the longest run of cycles from the uniform start in which the reference meets every condition below (test_squarem_cycle_cpu.py).
# segments: cycle 10 would leave 2 % of the components out (kappa > 1e4); cfg3_family_shuffled: cycle 12 has an acceptance margin of 1.6e-9
PROBLEMS = {"cfg3": lambda: _cfg3("window", 14), "human": lambda: _human(False, 14), "human_w": lambda: _human(True, 14),
            "segments": lambda: _segments(9), "cfg3_family_shuffled": lambda: _cfg3("family_shuffled", 11),
            "fast_slow": lambda: _fast_slow(2)}
_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = PROBLEMS[name]()
    return _problems[name]


GAP_MIN = 1.01          # a threshold sits at the geometric midpoint of a gap of at least this factor


def choose_rules(model, x, y, passes_done):
    """Rule values for the step x -> y from the reference's own numbers, each far from every threshold.  Returns
    {name: (Rules, gap, measure)} for count_floor, zero_cut and abs_step; gap is the factor between the component the rule silences (the
    one that decides the plain measure) and the next one that matters (inf for count_floor, which has no threshold)."""
    den = model.den
    x, y = x.astype(LD), y.astype(LD)
    base, _, d, move = stop_measure(x, y, den, Rules(), passes_done)
    top = int(np.argmax(d))
    out = {"plain": (Rules(), np.inf, base)}
    # count_floor: the deciding component's own inferred reads, which about halves its term
    cf = float(max(y[top], x[top] / 2) * den[top])
    out["count_floor"] = (Rules(count_floor=cf), np.inf, stop_measure(x, y, den, Rules(count_floor=cf), passes_done)[0])
    # zero_cut silences falling components below it: between the decider and the next decider that is falling
    falling = y <= x
    if falling[top] and y[top] > 0:
        rest = ~falling | (y > y[top])
        t2 = int(np.argmax(np.where(rest, d, -1)))
        b = y[t2] if falling[t2] else 4 * y[top]
        zc = float(np.sqrt(y[top] * b))
        out["zero_cut"] = (Rules(zero_cut=zc), float(b / y[top]), stop_measure(x, y, den, Rules(zero_cut=zc), passes_done)[0])
    # abs_step silences components that move less than its bound: between the decider's move and the next decider's
    rest = move > move[top]
    b = move[int(np.argmax(np.where(rest, d, -1)))] if rest.any() else 4 * move[top]
    step = float(np.sqrt(move[top] * b) * max(passes_done + 1, 1000) / LD(2e5))
    out["abs_step"] = (Rules(abs_step=step), float(b / move[top]), stop_measure(x, y, den, Rules(abs_step=step), passes_done)[0])
    return out
