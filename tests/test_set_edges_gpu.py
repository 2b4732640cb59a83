"""GPU: the set-resident solver (k_solve_sets<64|256|512>, k_solve_sets_boot) at the edges of its size classes -- the shapes of
tests/set_problems.py, which test_set_edges_cpu.py pins to their class and LDS footprint: either side of the 6 / 48 / 156 KiB caps
and of the 128 / 129 and 512 / 513 thread edges, a set whose rows and columns give the 4-way unrolled gathers every tail length,
and all of them in one problem behind non-zero descriptor offsets.  Every criterion is free of the trajectory: the optimum reached
(against the CPU oracle and the streaming solve), bit-reproducibility, and for resampled replicates the solve of the same draws.

The zero-draw row: in a replicate a row that draws 0 stays in its set with r = 0; when all its transcripts decay geometrically its
row sum S passes through the denormal range, where 1 / S is no longer finite -- the row must still contribute exactly 0."""
import numpy as np
import pytest

import oracle as O
from emsar_amd import EmsarHip, hip
from emsar_amd.hip import LAYOUT_CSR, LAYOUT_TILED
from tests import set_problems as SP
from tests.test_bootstrap_gpu import SOLVE as BOOT_SOLVE, _check_same_mle

pytestmark = pytest.mark.gpu
SOLVE = dict(max_iter=400000, tol=1e-10)
LAYOUTS = [(LAYOUT_CSR, "1"), (LAYOUT_TILED, "2")]       # TILED with the library's own transcript numbering forced on: the set records,
LAYOUT_IDS = ["csr", "tiled-renumbered"]                 # found on the caller's CSR, are mapped

EDGE_NAMES = ["%dx%dx%d" % e[0] for e in SP.EDGES]
PROBLEMS = {name: (lambda k=k: SP.edge_problem(k)) for k, name in enumerate(EDGE_NAMES)}
PROBLEMS.update(ragged=SP.ragged_problem, resident=SP.all_resident_problem)
# (sets_resident, sets_streamed) of each problem: test_set_edges_cpu.py holds the builder to these
EXPECT = {name: ((0, 1) if e[2] == SP.STREAMED else (1, 0)) for name, e in zip(EDGE_NAMES, SP.EDGES)}
EXPECT.update(ragged=(1, 0), resident=(len(SP.resident_sets()), 0))
CAP2 = EDGE_NAMES[8]                                     # 159 744 B of dynamic LDS under 512 threads: the largest launch there is
# the plain EM path (no SQUAREM, no Newton step) of the same kernels: the three smallest footprints and the ragged set; the oracle's
# plain EM needs 60 .. 1200 passes on these.  The larger shapes are left out: thousands of passes more for no further code path.
PLAIN = [EDGE_NAMES[2], EDGE_NAMES[3], EDGE_NAMES[0], "ragged"]

_refs = {}


class Ref:
    """a problem, the oracle's model of it and the oracle's optimum (computed once, never written to)"""

    def __init__(self, name):
        self.name = name
        self.n_tx, self.rp, self.ci, self.R, self.E = PROBLEMS[name]()
        self.m = O.Csr(self.n_tx, self.rp, self.ci, R=self.R, E=self.E)
        self.den = self.m.den()                          # from the host: the device's own scatter adds with floating atomics
        self.th_o, st = self.m.em_solve(max_iter=400000, accel=1, tol=1e-10, n_threads=4)
        assert st.converged == 1
        self.F_o = self.m.loglik(self.th_o)
        for a in (self.rp, self.ci, self.R, self.E, self.den, self.th_o):
            a.setflags(write=False)

    def upload(self, dev, layout, renumber, monkeypatch):
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
        dev.upload_structure(self.n_tx, self.rp, self.ci, layout)
        dev.upload_sample(self.R, self.E, self.den)
        if layout == LAYOUT_TILED and self.n_tx >= 100:
            assert dev.info()["renumbered"] == 1


def components(m):
    """label of every transcript's connected component through the rows of m (any weight)"""
    parent = np.arange(m.n_tx)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    rp = m.row_ptr.astype(np.int64)
    for r in range(m.n_rows):
        a = find(m.col_idx[rp[r]])
        for t in m.col_idx[rp[r] + 1:rp[r + 1]]:
            parent[find(t)] = a
    return np.array([find(t) for t in range(m.n_tx)])


def oracle_optimum(m, max_iter=400000):
    """The oracle's SQUAREM solve of a replicate's draws, one connected component at a time.  F is a sum over the components, so this
    is the optimum of the whole problem; solved as one, a single step length for every component can make the oracle take 10^5
    passes where the slowest component alone takes 1500 (it depends on the draws), and a test has seconds."""
    comp = components(m)
    rp = m.row_ptr.astype(np.int64)
    row_comp = comp[m.col_idx[rp[:-1]]]
    theta = np.zeros(m.n_tx)
    for c in np.unique(comp):
        tids = np.nonzero(comp == c)[0]
        rows = np.nonzero(row_comp == c)[0]
        if len(rows) == 0:
            continue
        local = np.full(m.n_tx, -1, dtype=np.int64)
        local[tids] = np.arange(len(tids))
        ci = np.concatenate([local[m.col_idx[rp[r]:rp[r + 1]]] for r in rows])
        srp = np.concatenate([[0], np.cumsum(np.diff(rp)[rows])])
        th, st = O.Csr(len(tids), srp, ci, R=m.R[rows], E=m.E[rows]).em_solve(max_iter=max_iter, accel=1, tol=1e-10)
        assert st.converged == 1
        theta[tids] = th
    return theta


def ref(name):
    if name not in _refs:
        _refs[name] = Ref(name)
    return _refs[name]


@pytest.fixture(scope="module")
def dev():
    with EmsarHip(0) as d:
        yield d


def check_optimum(r, th, st, th_s, what):
    """test_set_solver.py's criteria for test_every_class_and_a_streamed_set: likelihood, fitted rates of the rows inside the likelihood
    (what the MLE pins down when transcripts only ever occur together), total inferred reads"""
    m, F_o = r.m, r.F_o
    F = m.loglik(th)
    print("%s: loglik off the oracle's by %.3g, off F(theta) by %.3g (relative)" % (what, abs(st.loglik - F_o) / abs(F_o), abs(F - st.loglik) / abs(F_o)))
    assert abs(st.loglik - F_o) <= 1e-10 * abs(F_o), what
    assert abs(F - st.loglik) <= 1e-10 * abs(F_o), what
    inside = (r.E > 0) & (r.R > 0)
    S = lambda x: np.add.reduceat(x[r.ci], r.rp[:-1].astype(np.int64))[inside]
    S_o, S_r, S_s = S(r.th_o), S(th), S(th_s)
    print("%s: worst fitted rate off the oracle's by %.3g, off the streaming solve's by %.3g (in units of the bound)"
          % (what, np.max(np.abs(S_r - S_o) / (1e-5 * S_o + 1.5e-6)), np.max(np.abs(S_r - S_s) / (1e-5 * S_s + 1.5e-6))))
    assert np.all(np.abs(S_r - S_o) <= 1e-5 * S_o + 1.5e-6), what
    assert np.all(np.abs(S_r - S_s) <= 1e-5 * S_s + 1.5e-6), what
    total = (r.th_o * r.den).sum()
    assert abs((th * r.den).sum() - total) <= 1e-8 * total, what


@pytest.mark.parametrize("layout,renumber", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_solve_reaches_the_optimum_and_is_reproducible(dev, name, layout, renumber, monkeypatch):
    r = ref(name)
    r.upload(dev, layout, renumber, monkeypatch)
    streamed = EXPECT[name][1] > 0
    dev.set_deterministic(streamed)        # a set left to the streaming passes adds with floating atomics unless told otherwise;
    try:                                   # the resident path has none
        th, st = dev.solve(set_mode=0, accel=1, **SOLVE)
        th2, st2 = dev.solve(set_mode=0, accel=1, **SOLVE)
        th_s, st_s = dev.solve(set_mode=1, accel=1, **SOLVE)
    finally:
        dev.set_deterministic(False)
    print("%s: %d passes in the slowest set, %d in all; streaming solve %d passes" % (name, st.set_passes_max, st.set_passes_sum, st_s.iters))
    assert st.converged == 1 and st.sets_unconverged == 0 and st_s.converged == 1
    assert (st.sets_resident, st.sets_streamed) == EXPECT[name] and st.sets_cluster == 0
    assert st_s.sets_resident == 0
    check_optimum(r, th, st, th_s, name)
    assert np.array_equal(th.view(np.int64), th2.view(np.int64))
    assert st2.set_passes_sum == st.set_passes_sum and st2.set_passes_max == st.set_passes_max


@pytest.mark.parametrize("layout,renumber", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", PLAIN)
def test_plain_em_reaches_the_optimum(dev, name, layout, renumber, monkeypatch):
    r = ref(name)
    r.upload(dev, layout, renumber, monkeypatch)
    th, st = dev.solve(set_mode=0, accel=0, newton_after=-1, **SOLVE)
    th2, st2 = dev.solve(set_mode=0, accel=0, newton_after=-1, **SOLVE)
    th_s, st_s = dev.solve(set_mode=1, accel=1, **SOLVE)
    print("%s: plain EM, %d passes" % (name, st.set_passes_max))
    assert st.converged == 1 and st.sets_unconverged == 0 and st_s.converged == 1
    assert (st.sets_resident, st.sets_streamed) == EXPECT[name]
    check_optimum(r, th, st, th_s, name + " plain EM")
    assert np.array_equal(th.view(np.int64), th2.view(np.int64)) and st2.set_passes_sum == st.set_passes_sum


_oracle_reps = {}


def oracle_of_draw(r, key, w):
    """the oracle's optimum for the drawn weights w (the same draws under every layout: solved once)"""
    if key not in _oracle_reps:
        _oracle_reps[key] = (w.copy(), oracle_optimum(O.Csr(r.n_tx, r.rp, r.ci, R=w, E=r.E), max_iter=BOOT_SOLVE["max_iter"]))
    assert np.array_equal(_oracle_reps[key][0], w)
    return _oracle_reps[key][1]


@pytest.mark.parametrize("layout,renumber", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["resident", CAP2])
def test_bootstrap_and_subsample_replicates_are_solves_of_their_draws(name, layout, renumber, monkeypatch):
    r = ref(name)
    seed, n = 9, 3
    with EmsarHip(0) as a, EmsarHip(0) as b:
        r.upload(a, layout, renumber, monkeypatch)
        one = a.bootstrap(n, seed, want_replicates=True, set_mode=0, **BOOT_SOLVE)
        reps = one[3]
        assert reps.shape == (n, r.n_tx) and one[4].n_replicates == n and one[4].replicates_unconverged == 0
        b.upload_structure(r.n_tx, r.rp, r.ci, layout)
        for k in range(n):
            w = a.bootstrap_weights(seed, k)
            assert np.array_equal(w, hip.bootstrap_draw_host(seed, k, np.where(r.E != 0, r.R, 0)))
            b.upload_sample(w, r.E, r.den)
            th_b, st_b = b.solve(set_mode=0, **BOOT_SOLVE)
            assert st_b.converged == 1
            _check_same_mle(r.m, w, reps[k], th_b, "%s rep %d vs solve" % (name, k))
            _check_same_mle(r.m, w, reps[k], oracle_of_draw(r, (name, "boot", k), w), "%s rep %d vs oracle" % (name, k))
        # one replicate to a launch: the same bits in all four outputs
        monkeypatch.setenv("EMSAR_HIP_BOOT_BATCH", "1")
        single = a.bootstrap(n, seed, want_replicates=True, set_mode=0, **BOOT_SOLVE)
        monkeypatch.delenv("EMSAR_HIP_BOOT_BATCH")
        assert single[4].batch == 1 and one[4].batch == n
        for x, y in zip(one[:4], single[:4]):
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), name
        # subsampling: the replicate is scaled to the full depth, its draws are binomial
        f, ns = 0.3, 2
        s = a.subsample([f], ns, seed, want_replicates=True, set_mode=0, **BOOT_SOLVE)
        assert s["replicates"].shape == (1, ns, r.n_tx) and s["stats"].replicates_unconverged == 0
        N_R = int(np.where(r.E != 0, r.R, 0).astype(np.int64).sum())
        for j in range(ns):
            w = a.subsample_weights(seed, j, f)
            N_b = int(w.astype(np.int64).sum())
            assert N_b > 0
            raw = s["replicates"][0, j] / (N_R / N_b)
            b.upload_sample(w, r.E, r.den)
            th_b, st_b = b.solve(set_mode=0, **BOOT_SOLVE)
            assert st_b.converged == 1
            _check_same_mle(r.m, w, raw, th_b, "%s f %g rep %d vs solve" % (name, f, j))
            _check_same_mle(r.m, w, raw, oracle_of_draw(r, (name, "sub", j), w), "%s f %g rep %d vs oracle" % (name, f, j))


# ---- the zero-draw row ----------------------------------------------------------------------------------------------------------

ZD_ROWS = [(0, 1), (0, 2), (1, 2), (0, 3), (3, 4), (3,), (4,)]
ZD_R = np.array([200, 200, 1, 50, 2000, 1, 1], dtype=np.int32)
ZD_DEN = np.array([1.0, 2.0, 2.0, 1.0, 1.0])
# row lengths E whose scatter IS den (binary fractions: every sum is exact), so that the oracle's likelihood -- which knows E, not
# den -- is the objective the device maximises: t0: .375 + .375 + .25, t1 = t2: .375 + 1.625, t3: .25 + .25 + .5, t4: .25 + .75
ZD_E = np.array([0.375, 0.375, 1.625, 0.25, 0.25, 0.5, 0.75])
ZD_DEAD = 2                                              # the row {1, 2}
TINY = 2.0 ** -1024                                      # below it 1 / S overflows


def numpy_em(w, tol, abs_floor=1e-6, max_iter=20000):
    """Plain float64 EM of the zero-draw problem under the weights w, from theta = 1, with the library's stopping rule
    max_t |y - x| / (|y| + abs_floor) < tol.  Returns (theta, passes, the passes whose E-step saw 0 < theta_1 + theta_2 < 2^-1024)."""
    x = np.ones(5)
    window = []
    for it in range(1, max_iter + 1):
        if 0.0 < x[1] + x[2] < TINY:
            window.append(it)
        acc, u = np.zeros(5), np.zeros(5)
        for row, wr in zip(ZD_ROWS, w):
            if len(row) == 1:
                u[row[0]] += wr
                continue
            S = x[list(row)].sum()
            if wr > 0 and S > 0:                         # a row with weight 0 contributes exactly 0, whatever S is
                acc[list(row)] += wr / S
        y = np.where(x > 0, (x * acc + u) / ZD_DEN, 0.0)
        delta = np.max(np.abs(y - x) / (np.abs(y) + abs_floor))
        x = y
        if delta < tol:
            return x, it, window
    return x, -1, window


def zero_draw():
    """the first (seed, replicate) in which the row {1, 2} draws 0 and every other row more -- picked on the host"""
    for seed in range(1, 50):
        for rep in range(64):
            w = hip.bootstrap_draw_host(seed, rep, ZD_R)
            if w[ZD_DEAD] == 0 and (np.delete(w, ZD_DEAD) > 0).all():
                return seed, rep, w
    raise AssertionError("no such draw")


@pytest.mark.parametrize("params", [dict(accel=0, newton_after=-1), dict(accel=1, newton_after=0)], ids=["plain-em", "default"])
def test_a_row_that_draws_zero_contributes_zero_whatever_its_row_sum(dev, params):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in ZD_ROWS])]).astype(np.uint64)
    ci = np.concatenate([np.array(r) for r in ZD_ROWS]).astype(np.int32)
    seed, rep, w = zero_draw()
    want, passes, window = numpy_em(w, tol=1e-10)
    # the reference itself goes through the range where 1 / (theta_1 + theta_2) is not finite, and before it stops: the device, which
    # makes the same steps when it runs plain EM, cannot pass by missing it
    assert window and 0 < window[0] <= window[-1] < passes, (window, passes)
    assert want[1] == 0.0 and want[2] == 0.0 and np.isfinite(want).all()
    print("draw (seed %d, replicate %d): weights %s; the reference sees a denormal row sum in passes %d-%d and stops after pass %d"
          % (seed, rep, w.tolist(), window[0], window[-1], passes))
    dev.upload_structure(5, rp, ci)
    dev.upload_sample(ZD_R, ZD_E, ZD_DEN)
    assert dev.solve(set_mode=0)[1].sets_resident == 1   # one set of five transcripts, the two single-transcript rows folded
    assert np.array_equal(dev.bootstrap_weights(seed, rep), w)
    mean, sd, tsd, reps, st = dev.bootstrap(1, seed, first=rep, want_replicates=True, set_mode=0, tol=1e-10, max_iter=20000, **params)
    th = reps[0]
    print("device: %s after %d passes" % (th.tolist(), st.set_passes_max))
    assert st.replicates_unconverged == 0 and np.isfinite(th).all()
    if not params["accel"]:
        assert th[1] == 0.0 and th[2] == 0.0
        assert st.set_passes_max > window[-1]            # the same steps: the device went through the window too
    m = O.Csr(5, rp, ci, R=ZD_R, E=ZD_E)
    _check_same_mle(m, w, th, want, "zero-draw replicate vs the numpy fixed point")
