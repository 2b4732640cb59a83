"""GPU: every TILED pass kernel that launch_pass can pick, forced with the knobs it reads at upload_structure
(EMSAR_HIP_TILED_MULTI, EMSAR_HIP_WEIGHTED_UNIT), and the unit kernel under the layout knobs that change its control flow,
against the CPU oracle.

Tolerances (FP64; the kernels and the oracle differ in summation order only):
  * plain passes from the same theta:     |dtheta| <= 1e-11 * theta + 1e-300
  * likelihood by-product of a pass:      1e-11 relative + 1e-9
  * deterministic mode:                   bit-identical repeats; N * 2^-61 * 20000 reads of the oracle and of the one-tile kernel
  * extremes (weights up to INT32_MAX, theta at 1e+-70 / 1e-300): a long-double restatement of the pass, 1e-11 relative
"""
import numpy as np
import pytest

import oracle as O
from emsar_amd import EmsarHip, EmsarHipError
from emsar_amd.hip import LAYOUT_TILED
from tests import pass_problems as P
from tests.cycle_reference import ld_pass as _ld_pass      # one EM pass in long double
from tests.pass_problems import VARIANTS

pytestmark = pytest.mark.gpu
INT32_MAX = 2 ** 31 - 1
ERR_ARG = -1

MATRICES = ["segments", "cfg5_reads", "cfg5_segments", "ugly"]


@pytest.fixture(scope="module")
def dev():
    ctx = EmsarHip(0)
    yield ctx
    ctx.set_deterministic(False)
    ctx.close()


def _knobs(monkeypatch, knobs):
    for k in P.LAYOUT_KNOBS:
        monkeypatch.delenv("EMSAR_HIP_" + k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("EMSAR_HIP_" + k, v)


class Case:
    """A problem with the sample one variant uploads (R and / or E, or neither) and the oracle of that sample."""

    def __init__(self, p, weights):
        self.p = p
        self.R = p.R if "R" in weights else None
        self.E = p.E if "E" in weights else None
        self.m = O.Csr(p.n_tx, p.rp, p.ci, R=self.R, E=self.E)
        self.den = self.m.den() if p.den is None else p.den
        n = np.diff(p.rp.astype(np.int64))
        w = np.ones(p.n_rows, dtype=np.int64) if self.R is None else self.R.astype(np.int64)
        w[self.m.E == 0] = 0
        self.w = w                                                   # what a row counts in the likelihood
        has = np.add.reduceat(np.append((self.den[p.ci] > 0).astype(np.int64), 0), p.rp[:-1].astype(np.int64))
        has[n == 0] = 0
        self.mass = int(w[has > 0].sum())                            # the rows an EM step distributes: some id with theta > 0
        self.N = int(w.sum())
        self.th0 = np.where(self.den > 0, 1.0, 0.0)
        th, self.want = self.th0, []
        for _ in range(4):                                           # passes 1-3 plain, pass 4 with the likelihood at its input
            th, ll = self.m.em_step(th, self.den, n_threads=4)
            self.want.append((th, ll))

    def loglik(self, th):
        """Fp as the device states it: sum over the rows inside F of r log(E S) - E S, rows with S = 0 counting r log E
        (the oracle calls such a point infeasible; only the ugly matrix has them)."""
        if self.p.den is None:
            return self.m.loglik(th)
        p, n = self.p, np.diff(self.p.rp.astype(np.int64))
        S = np.add.reduceat(np.append(th[p.ci], 0.0), p.rp[:-1].astype(np.int64))
        S[n == 0] = 0.0
        inside = self.m.E != 0
        live = inside & (S > 0) & (self.w > 0)
        return float(np.sum(self.w[live] * np.log(S[live])) + np.sum(self.w[inside & (self.w > 0)] * np.log(self.m.E[inside & (self.w > 0)]))
                     - np.dot(th, self.den))

    def upload(self, dev, merged):
        dev.upload_structure(self.p.n_tx, self.p.rp, self.p.ci, LAYOUT_TILED, merge_rows=merged)
        dev.upload_sample(self.R, self.E, self.p.den)


_cases, _ref_F, _one_tile_det = {}, {}, {}


def _case(matrix, weights):
    if (matrix, weights) not in _cases:
        _cases[(matrix, weights)] = Case(P.problem(matrix), weights)
    return _cases[(matrix, weights)]


def _passes(dev, c, what):
    """3 plain passes, then one with the likelihood: against the oracle's em_step.  Returns (theta after 4, likelihood)."""
    dev.set_theta(c.th0)
    dev.run_passes(3)
    got = dev.get_theta()
    want3 = c.want[2][0]
    assert np.all(np.abs(got - want3) <= 1e-11 * np.abs(want3) + 1e-300), (what, np.max(np.abs(got - want3) / np.maximum(want3, 1e-300)))
    _, ll = dev.run_passes(1, want_loglik=True)
    got4, (want4, ll4) = dev.get_theta(), c.want[3]
    assert np.all(np.abs(got4 - want4) <= 1e-11 * np.abs(want4) + 1e-300), what
    assert abs(ll - ll4) <= 1e-11 * abs(ll4) + 1e-9, (what, ll, ll4)
    return got4, ll


def _det_passes(dev, c, what):
    """Deterministic mode: two runs bit-identical, within the fixed-point resolution of the oracle."""
    dev.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            dev.set_theta(c.th0)
            dev.run_passes(3)
            _, ll = dev.run_passes(1, want_loglik=True)
            runs.append((dev.get_theta(), ll))
    finally:
        dev.set_deterministic(False)
    (a, la), (b, lb) = runs
    np.testing.assert_array_equal(a, b, err_msg=what)
    assert la == lb, what
    want4, ll4 = c.want[3]
    res = max(c.N, 1) * 2.0 ** -61 * 20000
    assert np.all(np.abs(a - want4) * c.den <= res + 1e-11 * want4 * c.den), what
    assert abs(la - ll4) <= 1e-10 * abs(ll4) + 1e-9, (what, la, ll4)
    return a, la


def _check_solve(dev, c, what):
    th, st = dev.solve(set_mode=1, max_iter=3000, accel=1, tol=1e-10)      # a tighter stop than the oracle's below
    assert np.isfinite(th).all() and (th >= 0).all(), what
    F = c.loglik(th)
    assert abs(st.loglik - F) <= 1e-9 * abs(F) + 1e-9, (what, st.loglik, F)
    key = (c.p.name, c.R is not None, c.E is not None)
    if key not in _ref_F:               # the oracle's EM (SQUAREM) at a smaller budget; plain EM where the caller gives den
        if c.p.den is None:
            _ref_F[key] = c.m.loglik(c.m.em_solve(max_iter=2000, tol=1e-9)[0])
        else:
            x = c.th0
            for _ in range(300):
                x, _ = c.m.em_step(x, c.den)
            _ref_F[key] = c.loglik(x)
    F_o = _ref_F[key]
    assert F >= F_o - 1e-9 * abs(F_o) - 1e-9, (what, F, F_o)
    assert abs(np.dot(th, c.den) - c.mass) <= 1e-9 * c.mass, (what, np.dot(th, c.den), c.mass)


def _one_tile(dev, monkeypatch, c, merged, knobs):
    """The deterministic result of the one-tile kernel on the same sample (cached)."""
    key = (c.p.name, c.R is not None, c.E is not None, merged)
    if key not in _one_tile_det:
        _knobs(monkeypatch, dict(TILED_MULTI="0"))
        c.upload(dev, merged)
        _one_tile_det[key] = _det_passes(dev, c, "one-tile")
        _knobs(monkeypatch, knobs)
    return _one_tile_det[key]


def _full_check(dev, monkeypatch, c, merged, knobs, what, solve=True):
    _knobs(monkeypatch, knobs)
    ref = _one_tile(dev, monkeypatch, c, merged, knobs)
    c.upload(dev, merged)
    _passes(dev, c, what)
    th_d, ll_d = _det_passes(dev, c, what + " det")
    res = max(c.N, 1) * 2.0 ** -61 * 20000
    assert np.all(np.abs(th_d - ref[0]) * c.den <= res + 1e-11 * ref[0] * c.den), what
    assert abs(ll_d - ref[1]) <= 1e-11 * abs(ref[1]) + 1e-9, what
    if solve:
        _check_solve(dev, c, what)


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_dispatch_variant_matches_oracle(dev, monkeypatch, variant, matrix):
    knobs, weights, merged, _, _ = VARIANTS[variant]
    c = _case(matrix, weights)
    _full_check(dev, monkeypatch, c, merged, knobs, "%s on %s" % (variant, matrix))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name,knobs,matrix,facts", P.SHAPES, ids=[s[0] for s in P.SHAPES])
def test_unit_kernel_shapes_match_oracle(dev, monkeypatch, name, knobs, matrix, facts, weighted):
    """The unit kernel (weighted: both its variants) on the layouts test_pass_kernel_shapes.py shows to have the shape."""
    k = dict(knobs, TILED_MULTI="5", WEIGHTED_UNIT="2")
    c = _case(matrix, "RE" if weighted else "")
    _full_check(dev, monkeypatch, c, False, k, "%s %s" % (name, "weighted" if weighted else "unweighted"), solve=False)


def test_dense_coo_lists_are_refused_and_the_context_stays_usable(dev, monkeypatch):
    c = _case("segments", "RE")
    _knobs(monkeypatch, dict(TILE_DENSE="2"))
    with pytest.raises(EmsarHipError) as e:
        dev.upload_structure(c.p.n_tx, c.p.rp, c.p.ci, LAYOUT_TILED)
    assert e.value.status == ERR_ARG and "code -27" in str(e.value), str(e.value)
    _knobs(monkeypatch, dict(TILED_MULTI="5", WEIGHTED_UNIT="2"))
    c.upload(dev, False)
    _passes(dev, c, "after a refused layout")


@pytest.mark.parametrize("variant", ["tiled_RE", "unit_wu0", "unit_wu1", "unit_wu2", "merged_unit"])
def test_weighted_extremes_against_long_double(dev, monkeypatch, variant):
    """Row weights from 1 to INT32_MAX in one sample (the unit kernel keeps them as int in registers), and theta at 1e+-70 and
    mixed with 1e-300 (weights up to 1000 there: INT32_MAX / 1e-300 leaves the double range in any FP64 pass)."""
    knobs, _, merged, _, _ = VARIANTS[variant]
    _knobs(monkeypatch, knobs)
    p = P.problem("cfg5_segments")
    rng = np.random.default_rng(17)
    big = np.exp(rng.uniform(0.0, np.log(INT32_MAX), size=p.n_rows)).astype(np.int64)
    big[rng.random(p.n_rows) < 0.02] = INT32_MAX
    big = np.clip(big, 1, INT32_MAX).astype(np.int32)
    small = rng.integers(1, 1001, size=p.n_rows).astype(np.int32)
    E = p.E
    den = O.Csr(p.n_tx, p.rp, p.ci, E=E).den()
    base = rng.uniform(0.5, 2.0, size=p.n_tx)
    mixed = base.copy()
    mixed[rng.random(p.n_tx) < 0.3] = 1e-300
    dev.upload_structure(p.n_tx, p.rp, p.ci, LAYOUT_TILED, merge_rows=merged)
    for R, thetas in ((big, (base, base * 1e-70, base * 1e70)), (small, (mixed, base * 1e-70))):
        dev.upload_sample(R, E, den)
        w = R.astype(np.int64)
        w[E == 0] = 0
        for th in thetas:
            th = np.where(den > 0, th, 0.0)
            want, ll, ll_abs = _ld_pass(p, w, den, th)
            dev.set_theta(th)
            _, ll_dev = dev.run_passes(1, want_loglik=True)
            got = dev.get_theta()
            want = want.astype(np.float64)
            assert np.isfinite(got).all() and np.isfinite(ll_dev), (variant, th[:2])
            assert np.all(np.abs(got - want) <= 1e-11 * np.abs(want) + 1e-300), (variant, th[:2], np.max(np.abs(got - want) / np.maximum(want, 1e-300)))
            assert abs(ll_dev - float(ll)) <= 1e-11 * float(ll_abs) + 1e-9, (variant, th[:2], ll_dev, float(ll))


def test_production_dispatch_above_the_pair_threshold(dev, monkeypatch):
    """No knobs: a weighted sample of more than 2048 tiles runs the plain passes on k_pass_tiled_unit<true, MODE_EM>, the
    default of every SQUAREM cycle on segment-level input of real size."""
    _knobs(monkeypatch, {})
    p = P.big_segments()
    m = O.Csr(p.n_tx, p.rp, p.ci, R=p.R, E=p.E)
    den = m.den()
    dev.upload_structure(p.n_tx, p.rp, p.ci, LAYOUT_TILED)
    dev.upload_sample(p.R, p.E, None)
    info = dev.info()
    assert info["n_chunks"] > 2048 and 0 < info["n_units"] < info["n_chunks"], info
    th = np.where(den > 0, 1.0, 0.0)
    dev.set_theta(th)
    want, _ = m.em_step(th, den, n_threads=16)
    want, _ = m.em_step(want, den, n_threads=16)
    dev.run_passes(2)
    got = dev.get_theta()
    assert np.all(np.abs(got - want) <= 1e-11 * np.abs(want) + 1e-300)
    want3, ll = m.em_step(want, den, n_threads=16)
    _, ll_dev = dev.run_passes(1, want_loglik=True)
    assert np.all(np.abs(dev.get_theta() - want3) <= 1e-11 * np.abs(want3) + 1e-300)
    assert abs(ll_dev - ll) <= 1e-11 * abs(ll) + 1e-9


def test_golden_through_the_weighted_unit_kernel(dev, golden, monkeypatch):
    """The reference's own fixtures with both weighted unit variants forced: 5 passes against em_step, a streaming solve against
    the reference's .fpkm."""
    _knobs(monkeypatch, dict(TILED_MULTI="5", WEIGHTED_UNIT="2"))
    m = golden.model
    dev.upload_structure(m.n_tx, m.row_ptr, m.col_idx, LAYOUT_TILED)
    dev.upload_sample(m.R, m.E, None)
    den = m.den()
    th = np.where(den > 0, 1.0, 0.0)
    for _ in range(5):
        th, ll = m.em_step(th, den)
        _, ll_dev = dev.run_passes(1, want_loglik=True)
        got = dev.get_theta()
        assert np.all(np.abs(got - th) <= 1e-11 * np.abs(th) + 1e-300)
        assert abs(ll_dev - ll) <= 1e-11 * abs(ll) + 1e-9
        dev.set_theta(th)
    th, st = dev.solve(set_mode=1, max_iter=600000, accel=1, tol=1e-10, check_every=16)
    assert st.converged == 1
    golden.check_fpkm_parity(th, "weighted unit kernel, streaming solve")
    F = m.loglik(th)
    assert abs(st.loglik - F) <= 1e-9 * abs(F)
