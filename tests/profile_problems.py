"""The CPU reference of the profile-likelihood intervals (include/emsar_hip.h "profile-likelihood intervals"), shared by
test_profile_cpu.py and test_profile_gpu.py: the chi2_1 cut by a bisection of its own, and the deviance D_ref(x) of a pinned value
theta_t = x from a pinned EM built on oracle.Csr.em_step alone -- apply em_step, put theta_t back to x, a SQUAREM (scheme S3, the
likelihood safeguard of oracle_em_solve) in numpy around that map.  No multiplier, no scaled den: nothing of the device's path.

    python -m tests.profile_problems        measures the reference's own spread (tol 1e-10 against 1e-13) at the reference's own limits
                                            of the oracle cases: the figure LAMBDA_SPREAD of test_profile_gpu.py comes from here
"""
import math

import numpy as np

import oracle
from tests import set_problems as SP

TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED = range(5)
QUERY_SEED = 5
# problems of the oracle comparison: name -> (problem, how many transcripts to query: None = all of them); one per workgroup class
# (64 / 256 / 512 threads), the ragged set, and the largest set of the two larger classes
ORACLE_CASES = {
    "ragged60": (SP.ragged_problem, None),
    "edge0_c0": (lambda: SP.edge_problem(0), None),
    "edge1_c1": (lambda: SP.edge_problem(1), None),
    "edge4_c1_250": (lambda: SP.edge_problem(4), 3),
    "edge8_c2_900": (lambda: SP.edge_problem(8), 3),
}


def cut(level):
    """2 * erfinv(level)^2 by bisection on math.erf"""
    lo, hi = 0.0, 8.0
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            return 2.0 * hi * hi
        if math.erf(mid) < level:
            lo = mid
        else:
            hi = mid


class Reference:
    """one problem: the oracle's full solve and the pinned EM"""

    def __init__(self, prob, tol=1e-12):
        self.n_tx, rp, ci, R, E = prob
        self.m = oracle.Csr(self.n_tx, rp, ci, R=R, E=E)
        self.den = self.m.den()
        self.theta, _ = self.m.em_solve(tol=tol)
        self.F = self.m.loglik(self.theta)
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp).astype(np.int64))
        live = (np.asarray(R)[rows] > 0) & (np.asarray(E)[rows] > 0)
        n_all = np.bincount(rows[live], minlength=len(rp) - 1)
        self._rows, self._live, self._n_all, self._ci = rows, live, n_all, np.asarray(ci)

    def essential(self, t):
        """a row inside the likelihood with reads whose every entry is t"""
        mine = np.bincount(self._rows[self._live & (self._ci == t)], minlength=len(self._n_all))
        return bool(np.any((self._n_all > 0) & (mine == self._n_all)))

    def pinned(self, t, x, tol=1e-12, max_iter=400000):
        """theta maximising the likelihood with theta_t = x, and its log-likelihood"""
        m, den = self.m, self.den

        def G(th):
            y, _ = m.em_step(th, den)
            y[t] = x
            return y
        th0 = np.where(den > 0, 1.0, 0.0)
        th0[t] = x
        stepmax, it = 1.0, 0
        while it < max_iter:
            th1 = G(th0)
            it += 1
            if np.max(np.abs(th1 - th0) / (np.abs(th1) + 1e-6)) < tol:
                th0 = th1
                break
            th2 = G(th1)
            it += 1
            r = th1 - th0
            v = (th2 - th1) - r
            sv = float(v @ v)
            s = min(max(math.sqrt(float(r @ r) / sv) if sv > 0 else 1.0, 1.0), stepmax)
            if s > 1.01:
                thx = th0 + 2.0 * s * r + s * s * v
                thx = np.where((thx > 0) & (th2 > 0), thx, th2)
                thx[t] = x
                if m.loglik(thx) >= m.loglik(th1):
                    if s >= stepmax:
                        stepmax *= 4.0
                else:
                    thx = th2
                    if s >= stepmax:
                        stepmax = max(1.0, stepmax / 4.0)
            else:
                thx = th2
                if s >= stepmax:
                    stepmax *= 4.0
            th0 = G(thx)
            it += 1
        return th0, m.loglik(th0)

    def deviance(self, t, x, tol=1e-12):
        """D_ref(x) = 2 (F_full - F_pinned) and |F_full| + |F_pinned|; (+inf, nan) where a row with reads is left with nothing"""
        if x == 0.0 and self.essential(t):
            return math.inf, math.nan
        _, Fp = self.pinned(t, x, tol)
        return 2.0 * (self.F - Fp), abs(self.F) + abs(Fp)

    def limit(self, t, side, q, rel=1e-6):
        """the reference's own limit: a root of D_ref(x) = q below (side 0) or above (side 1) theta_hat_t, by bisection in x"""
        th = float(self.theta[t])
        if side == 0:
            lo, hi = 0.0, th                  # D(lo) > q >= D(hi)
        else:
            lo, hi = th, max(2.0 * th, q / self.den[t])
            while self.deviance(t, hi, 1e-10)[0] < q:
                hi *= 2.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            d = self.deviance(t, mid, 1e-10)[0]
            if abs(d - q) <= rel * q:
                return mid
            if (d > q) == (side == 0):
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)


def queries(prob, count, ref):
    """all transcripts, or `count` of those with theta_hat den >= 1e-9 chosen by QUERY_SEED"""
    if count is None:
        return np.arange(prob[0], dtype=np.int32)
    alive = np.flatnonzero(ref.theta * ref.den >= 1e-9)
    return np.sort(np.random.default_rng(QUERY_SEED).choice(alive, size=count, replace=False)).astype(np.int32)


_cache = {}


def oracle_case(name):
    """problem, its Reference, the queried tids and the reference's Lambda per query (NaN for a transcript outside the likelihood),
    computed once per session"""
    if name not in _cache:
        make, count = ORACLE_CASES[name]
        prob = make()
        ref = Reference(prob)
        q = queries(prob, count, ref)
        lam = []
        for t in q:
            if ref.den[t] == 0:
                lam.append((math.nan, math.nan))
            elif ref.theta[t] * ref.den[t] < 1e-9:
                lam.append((0.0, 2 * abs(ref.F)))
            else:
                d, scale = ref.deviance(int(t), 0.0)
                lam.append((max(d, 0.0), scale))
        _cache[name] = (prob, ref, q, lam)
    return _cache[name]


def measure_spread(levels=(0.95,)):
    """the pinned reference against itself, tol 1e-10 vs 1e-13, at its own limits: max |dD| / (|F_full| + |F_pinned|)"""
    worst = 0.0
    for name in ORACLE_CASES:
        prob, ref, q, lam = oracle_case(name)
        for level in levels:
            c = cut(level)
            for t, (lm, _) in zip(q, lam):
                if not lm == lm:
                    continue
                for side in ((0, 1) if lm > c else (1,)):
                    x = ref.limit(int(t), side, c)
                    a, sa = ref.deviance(int(t), x, 1e-10)
                    b, _ = ref.deviance(int(t), x, 1e-13)
                    worst = max(worst, abs(a - b) / sa)
                    print(name, level, int(t), side, "x", x, "D", a, "spread/scale", abs(a - b) / sa, "worst", worst, flush=True)
    return worst


if __name__ == "__main__":
    print("LAMBDA_SPREAD", measure_spread())
