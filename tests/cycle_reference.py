"""A long-double restatement of one cycle of the streaming solve (solve.hpp: enqueue_cycles; kernels_vector.hpp: k_update,
k_cycle_begin, k_update_p2, k_sq_extrap_ll, k_update_p3), CPU only.  test_squarem_cycle_cpu.py runs it alone, test_squarem_cycle_gpu.py
starts it at the device's own points, test_pass_kernels_gpu.py uses its EM pass.  The set-resident solver (kernels_sets.hpp) runs the
same cycle per connected set: the second half of this file holds one Model per set, the set solver's Newton step restated
(newton_step) and the cases of test_set_cycle_cpu.py / test_set_cycle_gpu.py.

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
    n_tx, rp, ci, R, den = _fast_slow_rows(linked=False)
    return Problem("fast_slow", K, n_tx, rp, ci, R=R, den=den)


def _fast_slow_rows(linked):
    """the rows of fast_slow -> (n_tx, rp, ci, R, den).  linked: one more row of one read {i + 1, i + 2} between every two neighbouring
    pairs, which makes the 128 pairs ONE connected set of 256 transcripts and 255 rows (the set solver's 256-thread class) and
    leaves the second cycle's step where it was (s = 1.0051)."""
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
    if linked:
        for i in range(1, 255, 2):
            rows.append([i, i + 1])
            w.append(1)
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return 256, rp, np.concatenate(rows).astype(np.int32), np.array(w, dtype=np.int32), den


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


# ---- the set-resident solver (kernels_sets.hpp: solve_one_set, set_newton_step) ----------------------------------------------------------
# One workgroup runs the same cycle on one connected set, with a step s and a stepmax of its own.  A single-transcript row {t} with count
# R is the folded u_t of the kernel: x (R / x) = u in the update, R log x in F -- so Model states the set's cycle as it stands, once it
# holds the set's rows only.

def set_model(rp, ci, R, E, den, tids, rows):
    """The Model of one connected set of a sample: tids its transcripts in the caller's numbering (their order is the model's), rows the
    caller's rows that hold them (single-transcript rows included, E = 0 rows count 0), den the whole sample's den."""
    rp = np.asarray(rp).astype(np.int64)
    local = np.full(len(den), -1, dtype=np.int64)
    local[tids] = np.arange(len(tids))
    n = np.diff(rp)[rows]
    srp = np.zeros(len(rows) + 1, dtype=np.uint64)
    srp[1:] = np.cumsum(n)
    sci = local[np.concatenate([np.asarray(ci)[rp[r]:rp[r + 1]] for r in rows])]
    assert (sci >= 0).all(), "a row of the set holds a transcript outside it"
    return Model(len(tids), srp, sci, np.asarray(R)[rows], np.asarray(den)[tids], np.asarray(E)[rows])


class SetCase:
    """A sample for the set solver: what a test uploads (den is the E-scatter, computed once on the host), one Model per connected
    set with the set's caller tids, the size class of the kernel that solves each set, and K, the cycles that are checked."""

    def __init__(self, name, K, cls, composed, den=None):
        self.name, self.K, self.cls = name, K, cls
        self.n_tx, self.rp, self.ci, self.R, self.E = composed[:5]
        self.whole = Model(self.n_tx, self.rp, self.ci, self.R, den, self.E)      # den given (then E is None): the caller's own
        self.den = self.whole.den
        if len(composed) > 5:
            self.tids = [m[0] for m in composed[5]]
            self.models = [set_model(self.rp, self.ci, self.R, self.E, self.den, t, r) for t, r in composed[5]]
        else:                                   # one connected set: the whole sample's model is the set's
            self.tids, self.models = [np.arange(self.n_tx)], [self.whole]
        self.model = self.models[0]
        for a in (self.rp, self.ci, self.R, self.E, self.den):
            if a is not None:
                a.setflags(write=False)


def _shape_case(shape, seed):
    from tests import set_problems as SP
    return SP.compose([SP.edge_set(*shape, seed=seed)], seed=seed)


def _ragged_case(seed):
    from tests import set_problems as SP
    return SP.compose([SP.ragged_set(seed)], seed=seed)


def _edge_case(k):
    from tests import set_problems as SP
    return SP.edge_problem(k)


# name -> (size class, K, the cap on K, builder).  K: the longest run of cycles from the uniform start, the cap at the most, in which the
# reference meets comparable() and LEFT_OUT_MAX (test_set_cycle_cpu.py holds every K to that).  The cap is 12 for the problems of
# set_problems.py as the edge tests solve them and 14 for the seeded ones, compose([set], seed) of a shape or of ragged_set(seed): these
# were searched, 40 seeds a shape, for kinds of cycle with the reference alone.  Nothing the device computes entered a choice.
# ragged_problem() stops at 3: cycle 4 leaves one component of its 60 out, 1.7 %.
SET_EDGE_K = {0: 12, 1: 12, 2: 3, 3: 4, 4: 12, 5: 12, 6: 8, 7: 6, 8: 12}
SET_RAGGED_K = 3
SET_SEEDED = {((40, 80, 227), 307): (0, 14), ((40, 80, 227), 308): (0, 14),
              ((40, 80, 228), 325): (1, 13), ((40, 80, 228), 302): (1, 9), ((250, 500, 4784), 308): (1, 14),
              ((100, 513, 1100), 302): (2, 10), ((100, 513, 1100), 311): (2, 11)}
# accepted cycles only, but the most components that keep th2 in the 512-thread class (2 .. 5 per cycle), up to 0.8 % left out
SET_SEEDED.update({((250, 500, 4785), seed): (2, 14) for seed in range(300, 312)})
SET_RAGGED_SEEDED = {2: 14, 4: 14, 7: 14}
SET_CASES = {}


def _add_set_cases():
    from tests import set_problems as SP
    for k, K in SET_EDGE_K.items():
        SET_CASES["edge%d" % k] = (SP.EDGES[k][2], K, 12, lambda k=k: _edge_case(k))
    SET_CASES["ragged"] = (0, SET_RAGGED_K, 12, lambda: SP.ragged_problem())
    for (shape, seed), (cls, K) in SET_SEEDED.items():
        SET_CASES["%dx%dx%d-s%d" % (shape + (seed,))] = (cls, K, 14, lambda shape=shape, seed=seed: _shape_case(shape, seed))
    for seed, K in SET_RAGGED_SEEDED.items():
        SET_CASES["ragged-s%d" % seed] = (0, K, 14, lambda seed=seed: _ragged_case(seed))
    # cycle 2 has s = 1.0051: between 1 and the switch at 1.01; cycle 3 has an acceptance margin of 9.5e-10
    SET_CASES["fast_slow_linked"] = (1, 2, 14, lambda: _fast_slow_rows(linked=True))


_add_set_cases()
_set_cases = {}


def set_case(name):
    if name not in _set_cases:
        cls, K, _, make = SET_CASES[name]
        made = make()
        if name == "fast_slow_linked":                     # (n_tx, rp, ci, R, den): no E, a den of its own
            _set_cases[name] = SetCase(name, K, cls, made[:4] + (None,), den=made[4])
        else:
            _set_cases[name] = SetCase(name, K, cls, made)
    return _set_cases[name]


def longest_run(model, limit=14):
    """the cycles from the uniform start while each meets comparable() and LEFT_OUT_MAX, limit at the most"""
    A, stepmax, out = model.start, 1.0, []
    for k in range(limit):
        c = model.cycle(A, stepmax, 3 * k)
        if not comparable(c) or float((c.kappa > KAPPA_MAX).mean()) > LEFT_OUT_MAX:
            break
        out.append(c)
        A, stepmax = c.A_next, c.stepmax_next
    return out


# ---- the projected Newton step of the set solver -------------------------------------------------------------------------------------------

BOUND_READS = 1e-6          # kBoundReads of set_newton_step
# the conditions under which a Newton step's choices can be compared between two implementations
NEWTON_MASK_MARGIN, NEWTON_RQ_MARGIN, NEWTON_F_MARGIN, NEWTON_REOPEN_MARGIN = 1e-6, 1e-2, 1e-11, 1e-7
NEWTON_FLOOR_READS = 1e-6   # the distance between two results is measured in reads against reads + this
# Where the step is checked on the device: size class -> (case, early / late / refused, k's): the step from A_k, the point after k cycles.
# The device is checked at the FIRST k, which has margins on the reference's own trajectory (test_set_cycle_cpu.py; the GPU test asserts
# them again at the device's A_k, which is another point, the more so the later it is).  The other k's are neighbours at which the
# distance between the two precisions is measured too.  The late points have bound components: transcripts without reads of their own on
# their way to 0.  At the refused point all four trial steps lose F: the solver leaves the point alone and counts the passes.
NEWTON_POINTS = {0: [("40x80x227-s307", "early", (2, 3, 4)), ("40x80x227-s307", "late", (20, 22)), ("40x80x227-s307", "refused", (18,))],
                 1: [("40x80x228-s325", "early", (2, 3, 4)), ("edge4", "late", (50, 55, 60))],
                 2: [("100x513x1100-s302", "early", (2, 3, 4)), ("edge8", "late", (60, 64, 56))]}
# The largest distance between newton_step in float64 and in long double at those points: 1.39e-11 (edge4, k = 55; then 7.6e-12 at edge8,
# k = 64).  The GPU test derives its bound from the measured figure; test_set_cycle_cpu.py holds every distance to the cap, which leaves
# room for another libm or numpy.
NEWTON_DIST, NEWTON_DIST_CAP = 1.4e-11, 2e-11


class Newton:
    """What one Newton step computed (attributes; see newton_step())."""


def _rows_dot(p, v):
    n = np.diff(p.rp.astype(np.int64))
    S = np.add.reduceat(np.append(v[p.ci], v.dtype.type(0)), p.rp[:-1].astype(np.int64))
    S[n == 0] = 0
    return S


def _cols_sum(p, rowv):
    n = np.diff(p.rp.astype(np.int64))
    out = np.zeros(p.n_tx, dtype=rowv.dtype)
    order, starts, ids = _scatter_plan(p)
    if len(starts):
        out[ids] = np.add.reduceat(np.repeat(rowv, n)[order], starts)
    return out


def newton_step(model, x, T=LD):
    """set_newton_step restated in the float type T, and the plain EM step that follows it in solve_one_set (with its re-opening of a
    bound component whose gradient at 0 has turned positive).  Returns a Newton: x_new (x if refused), accepted, n_cg, n_trials, passes
    (1 + n_cg + n_trials), bound (mask), y = EM(x_new), measure (of x_new -> y, abs_floor 1e-6, no other rule), and the margins of every
    choice: mask_margin (g < 0 and x den < 1e-6 of the components without reads of their own), rq_margin (rq against rq_stop at every
    look, relative to rq_stop), F_margin (Fn against Fx - 1e-13 |Fx| at every trial, relative to the sum of |terms| of both),
    reopen_margin (acc against den (1 + 1e-9) at the components at 0)."""
    o = Newton()
    n = np.diff(model.rp.astype(np.int64))
    single = n == 1
    w = model.w.astype(T)
    rw = np.where(single, T(0), w)                       # the rows of the set; a single-transcript row is folded into u
    u = np.zeros(model.n_tx, dtype=T)
    np.add.at(u, model.ci[model.rp[:-1].astype(np.int64)[single]], w[single])
    den, x = model.den.astype(T), x.astype(T)
    pos = x > 0
    safe_x = np.where(pos, x, T(1))

    def F(v):
        S = _rows_dot(model, v)
        live, vp = S > 0, (u > 0) & (v > 0)
        terms = np.concatenate([rw[live] * np.log(S[live]), u[vp] * np.log(v[vp]), -(v * den)])
        bad = int(((rw > 0) & ~live).sum() + ((u > 0) & ~(v > 0)).sum())
        return np.sum(terms), np.sum(np.abs(terms)), bad

    S = _rows_dot(model, x)
    live = (S > 0) & (rw > 0)
    inv = np.where(live, T(1) / np.where(live, S, T(1)), T(0))
    acc = _cols_sum(model, rw * inv)
    hrow = rw * inv * inv
    up2 = np.where(pos, u / (safe_x * safe_x), T(0))
    g = acc - den + np.where(pos, u / safe_x, T(0))
    Fx, Fx_abs, _ = F(x)
    inF = den > 0
    o.bound = bound = inF & (g < 0) & (x * den < T(BOUND_READS)) & (u == 0)
    free = inF & ~bound
    cand = inF & (u == 0)                                # what could be bound: both conditions have a margin there
    o.mask_margin = np.inf
    if cand.any():
        mg = np.abs(g[cand]) / (acc[cand] + den[cand])
        mx = np.abs(x[cand] * den[cand] - T(BOUND_READS)) / T(BOUND_READS)
        small, neg = (x * den < T(BOUND_READS))[cand], (g < 0)[cand]
        # a condition matters only where the other one holds
        o.mask_margin = float(min(np.min(np.where(small, mg, np.inf)), np.min(np.where(neg, mx, np.inf))))
    diag = _cols_sum(model, hrow) + up2
    mi = np.where(free, np.where(diag > 0, T(1) / np.where(diag > 0, diag, T(1)), T(1)), T(0))
    r = np.where(free, g, T(0))
    z = np.zeros(model.n_tx, dtype=T)
    p = mi * r
    rq = np.sum(r * p)
    rq_stop = T(1e-8) * rq
    o.n_cg, o.rq_margin = 0, np.inf
    for it in range(model.n_tx):
        if rq_stop > 0:
            o.rq_margin = min(o.rq_margin, float(abs(rq - rq_stop) / rq_stop))
        if not (rq > rq_stop and rq > 0):
            break
        hp = np.where(free, _cols_sum(model, hrow * _rows_dot(model, p)) + up2 * p, T(0))
        s1 = np.sum(p * hp)
        o.n_cg += 1
        if not s1 > 0:
            break
        al = rq / s1
        z = z + al * p
        r = r - al * hp
        s2 = np.sum(np.where(free, r * (mi * r), T(0)))
        beta = s2 / rq
        rq = s2
        p = mi * r + beta * p
    else:
        o.rq_margin = min(o.rq_margin, float(abs(rq - rq_stop) / rq_stop)) if rq_stop > 0 else o.rq_margin
    o.z = z
    o.n_trials, o.accepted, o.F_margin, o.x_new, o.alpha = 0, False, np.inf, x, T(0)
    alpha = T(1)
    for tr in range(4):
        xn = np.where(free, np.maximum(x + alpha * z, T(0)), np.where(bound, T(0) if alpha == 1 else x * (1 - alpha), T(0)))
        Fn, Fn_abs, bad = F(xn)
        o.n_trials += 1
        if bad == 0:
            o.F_margin = min(o.F_margin, float(abs(Fn - (Fx - T(1e-13) * abs(Fx))) / (Fx_abs + Fn_abs)))
        if bad == 0 and Fn >= Fx - T(1e-13) * abs(Fx):
            o.accepted, o.x_new, o.alpha = True, xn, alpha
            break
        alpha = alpha * T(0.25)
    o.passes = 1 + o.n_cg + o.n_trials
    # the plain step that follows: B = EM(x_new), a component at 0 whose gradient there is positive is re-opened just above 0
    v = o.x_new
    S = _rows_dot(model, v)
    live = (S > 0) & (rw > 0)
    acc = _cols_sum(model, rw * np.where(live, T(1) / np.where(live, S, T(1)), T(0)))
    safe_den = np.where(inF, den, T(1))
    y = np.where(inF & (v > 0), (v * acc + u) / safe_den, T(0))
    at0 = inF & (v == 0)
    reopen = at0 & (acc > den * (1 + T(1e-9)))
    o.reopen_margin = float(np.min(np.abs(acc[at0] / den[at0] - (1 + T(1e-9))))) if at0.any() else np.inf
    o.y = np.where(reopen, T(1e-9) / safe_den, y)
    o.reopened = int(reopen.sum())
    d = np.abs(o.y - v) / (np.abs(o.y) + T(1e-6))
    o.measure = T(1) if reopen.any() else (d.max() if len(d) else T(0))
    return o


def newton_comparable(o):
    return (o.mask_margin >= NEWTON_MASK_MARGIN and o.rq_margin >= NEWTON_RQ_MARGIN and o.F_margin >= NEWTON_F_MARGIN
            and o.reopen_margin >= NEWTON_REOPEN_MARGIN)


def newton_margins(o):
    return "accepted %s alpha %g n_cg %d n_trials %d bound %d reopened %d | margins: mask %.3g rq %.3g F %.3g reopen %.3g" % (
        o.accepted, float(o.alpha), o.n_cg, o.n_trials, int(o.bound.sum()), o.reopened, o.mask_margin, o.rq_margin, o.F_margin, o.reopen_margin)


def newton_distance(a, b, den):
    """the largest distance between two results in reads, against the reads of the component plus NEWTON_FLOOR_READS (below that many
    reads the step itself takes a component for 0)"""
    a, b, den = a.astype(LD), b.astype(LD), den.astype(LD)
    return float(np.max(np.abs(a - b) * den / (np.abs(b) * den + LD(NEWTON_FLOOR_READS))))


def choose_late_abs_step(model, x, y, passes_done):
    """An abs_step for a step x -> y past 1000 passes that shows the pass count in its bound: the bound at this pass lies at the geometric
    midpoint of a gap of at least GAP_MIN^2 between two components' moves, the measure under it is positive and differs by more than
    1e-3 both from the plain one and from the measure under the bound of pass 1000, which is (passes_done + 1) / 1000 times larger.
    Returns (Rules, gap, measure, measure under the bound of pass 1000) of the smallest such bound, or None."""
    assert passes_done + 1 > 1000
    x, y = x.astype(LD), y.astype(LD)
    plain, _, _, move = stop_measure(x, y, model.den, Rules(), passes_done)
    moves = np.unique(move[move > 0])
    for a, b in zip(moves, moves[1:]):
        if b / a < GAP_MIN * GAP_MIN:
            continue
        r = Rules(abs_step=float(np.sqrt(a * b) * (passes_done + 1) / LD(2e5)))
        measure = stop_measure(x, y, model.den, r, passes_done)[0]
        frozen = stop_measure(x, y, model.den, r, 0)[0]
        if measure > 0 and abs(measure - plain) > 1e-3 * plain and abs(frozen - measure) > 1e-3 * measure:
            return r, float(b / a), measure, frozen
    return None
