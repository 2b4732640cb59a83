"""The gene-level profile intervals and the gene presence test (include/emsar_hip.h "gene-level profile intervals"): their independent
reference in numpy, shared by test_profile_genes_cpu.py and test_profile_genes_gpu.py.  Problems and samples are those of
tests/compare_problems.py and tests/compare_gene_problems.py; nothing the device computes enters anything here.

The reference knows no multiplier and no path.  It is a PINNED-SUM EM over the gene's parts (CP.component / CP.Block of each member with
den > 0): the E-step gives the expected reads n_t = x_t * sum_c R_c m_ct / S_c; a transcript outside the gene gets n_t / den_t; the
members get n_t / (den_t + mu) with mu the root of sum n_t / (den_t + mu) = x, found by bisection in every pass until the bracket
cannot be halved -- the exact M-step under the constraint "the members sum to x".  For x = 0 the members are held at 0 (the drop).
    D_ref(x) = 2 (F_hat_ref - F_pinned(x)),  F = sum R log S - sum x_t den_t with the original den.

`python -m tests.profile_gene_problems` measures the reference against itself (relative step 1e-10 against 1e-13) at its own limits:
SPREAD below is that figure, relative to |F_hat| + |F_pinned|."""
import numpy as np

from tests import compare_gene_problems as GP
from tests import compare_problems as CP

REL_STEP = 1e-13
MAX_PASSES = 400000
SPREAD = 2.3e-16         # 2.22e-16 measured by __main__: the largest over the genes of class_genes(64) and (256) near their 0.95 limits


class Gene:
    """the parts of one gene in one sample, laid side by side in one vector"""

    def __init__(self, prob, R, members, den=None):
        den = CP.den_of(prob) if den is None else den
        self.parts = GP.parts_of(prob, R, den, members)
        self.n_parts = len(self.parts)
        off = np.cumsum([0] + [len(p.tids) for p in self.parts])
        self.n = int(off[-1])
        self.blocks = [(p.block, np.arange(off[k], off[k + 1])) for k, p in enumerate(self.parts)]
        self.den = np.concatenate([p.den for p in self.parts]) if self.parts else np.zeros(0)
        self.is_member = np.concatenate([p.is_member for p in self.parts]) if self.parts else np.zeros(0, dtype=bool)
        self.members = int(self.is_member.sum())

    def rows(self, x):
        return [(b, cmap[b.col], np.bincount(b.rowid, weights=x[cmap[b.col]], minlength=b.n_r)) for b, cmap in self.blocks]

    def F_at(self, x):
        F = -float(np.dot(x, self.den))
        for b, col, S in self.rows(x):
            inside = np.bincount(b.rowid, weights=self.den[col], minlength=b.n_r) > 0
            if np.any((S <= 0) & (b.R > 0) & inside):
                return -np.inf
            ok = S > 0
            F += float(np.sum(b.R[ok] * np.log(S[ok])))
        return F

    def em(self, pin=None, rel_step=REL_STEP, max_passes=MAX_PASSES):
        """pin None: the free maximum; pin = x >= 0: the maximum with the members summing to x.  -> (x vector, F, passes)"""
        den, mem = self.den, self.is_member
        live = den > 0
        safe = np.where(live, den, 1.0)
        x = np.where(live, 1.0, 0.0)
        if pin is not None:
            x[mem] = pin / max(self.members, 1)
        midx = np.flatnonzero(mem)
        mden = [float(d) for d in den[midx]]
        passes = 0
        while True:
            acc = np.zeros(self.n)
            for b, col, S in self.rows(x):
                w = np.where(S > 0, b.R / np.where(S > 0, S, 1.0), 0.0)
                acc += np.bincount(col, weights=w[b.rowid], minlength=self.n)
            n = x * acc
            y = np.where(live, n / safe, 0.0)
            if pin is not None:
                y[midx] = pinned_mstep([float(v) for v in n[midx]], mden, pin)
            passes += 1
            step = np.max(np.abs(y - x) / (np.abs(y) + 1e-6)) if self.n else 0.0
            x = y
            if step < rel_step or passes >= max_passes:
                break
        return x, self.F_at(x), passes

    def deviance(self, x, F_hat, rel_step=REL_STEP):
        _, F, _ = self.em(pin=x, rel_step=rel_step)
        return 2.0 * (F_hat - F), F


def pinned_mstep(n, den, x):
    """y_t = n_t / (den_t + mu) with sum y_t = x: mu by bisection until the bracket cannot be halved.  The bracket comes from
    sum n / (den_max + mu) <= x <= sum n / (den_min + mu) over the members with n_t > 0."""
    if not x > 0:
        return [0.0] * len(n)
    pos = [(a, d) for a, d in zip(n, den) if a > 0]
    if not pos:
        raise ValueError("no member has expected reads: the constraint cannot be met by the EM")
    tot = sum(a for a, _ in pos)
    dmin, dmax = min(d for _, d in pos), max(d for _, d in pos)
    lo, hi = max(tot / x - dmax, -dmin), tot / x - dmin          # g(lo) >= x >= g(hi), g falling
    if lo > hi:
        lo = hi
    while True:
        mid = lo + 0.5 * (hi - lo)
        if not (lo < mid < hi):
            break
        if sum(a / (d + mid) for a, d in pos) > x:
            lo = mid
        else:
            hi = mid
    mu = hi
    return [a / (d + mu) if a > 0 else 0.0 for a, d in zip(n, den)]


def analytic_problem():
    """rows {a}: 30, {a, b}: 50, E = 1 (den_a = 2, den_b = 1); gene {a, b}  -> (prob, R, members)"""
    n_tx, rp, ci = CP.csr([[0], [0, 1]], 2)
    R = np.array([30, 50], dtype=np.int32)
    return (n_tx, rp, ci, R, np.ones(2)), R, [0, 1]


def analytic_fit():
    """The free maximum of 30 log a + 50 log(a + b) - 2 a - b: a = 30, b = 20, X_hat = 50, F_hat = 30 log 30 + 50 log 50 - 80."""
    return 50.0, 30.0 * np.log(30.0) + 50.0 * np.log(50.0) - 80.0


def analytic_D(x):
    """D(x) of gene {a, b} for x >= 30: with a + b = x pinned, 30 log a - a - x + 50 log x is maximal at a = 30 (b = x - 30 >= 0):
    D(x) = 2 (50 log(50 / x) - (50 - x))"""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 * (50.0 * np.log(50.0 / x) - (50.0 - x))


def scalar_root(f, lo, hi):
    """the root of a monotone f in [lo, hi] by bisection until the bracket cannot be halved"""
    flo = f(lo)
    while True:
        mid = lo + 0.5 * (hi - lo)
        if not (lo < mid < hi):
            return mid
        if (f(mid) > 0) == (flo > 0):
            lo = mid
        else:
            hi = mid


def closed_limits(u, den, q):
    """A gene of one-transcript components WITH reads, without the library's search: on the path x_i = u_i / (den_i + lam),
    D(lam) = 2 sum u_i (log(1 + lam / den_i) - lam / (den_i + lam)); the two roots of D = q by bisection in lam
    -> (lower, upper, X_hat)"""
    u, den = np.asarray(u, dtype=np.float64), np.asarray(den, dtype=np.float64)
    D = lambda lam: 2.0 * float(np.sum(u * (np.log1p(lam / den) - lam / (den + lam))))
    X = lambda lam: float(np.sum(u / (den + lam)))
    hi = 1.0
    while D(hi) < q:
        hi *= 2.0
    lam_lo = scalar_root(lambda l: D(l) - q, 0.0, hi)
    end = -float(den.min())
    v = 0.5
    while D(v * end) < q:
        v = 0.5 * (1.0 + v)
    lam_up = scalar_root(lambda l: q - D(l), v * end, 0.0)
    return X(lam_lo), X(lam_up), X(0.0)


_refs = {}


def class_reference(threads, k, q, limits):
    """the reference of gene k of GP.class_genes(threads) on sample A of CP.class_problem(threads), computed once per session:
    dict(F_hat, X_hat, lam (the drop's deviance), parts, members, D (per given limit: D_ref, F_pinned))"""
    key = (threads, k, tuple(float(x) for x in limits))
    if key not in _refs:
        prob, RA, _, _ = CP.class_problem(threads)
        g = Gene(prob, RA, GP.class_genes(threads)[k])
        xh, F_hat, _ = g.em()
        _, F_drop, _ = g.em(pin=0.0)
        _refs[key] = dict(F_hat=F_hat, X_hat=float(xh[g.is_member].sum()), lam=2.0 * (F_hat - F_drop), F_drop=F_drop, parts=g.n_parts,
                          members=g.members, D=[g.deviance(float(x), F_hat) for x in limits])
    return _refs[key]


def measure_spread(q=3.841458820694124):
    """the reference against itself, relative step 1e-10 against 1e-13, at its own 0.95 limits of the class-64 and class-256 genes"""
    worst = 0.0
    for threads in (64, 256):
        prob, RA, _, _ = CP.class_problem(threads)
        for members in GP.class_genes(threads):
            g = Gene(prob, RA, members)
            xh, F_hat, _ = g.em()
            X_hat = float(xh[g.is_member].sum())
            _, F_hat10, _ = g.em(rel_step=1e-10)
            for lower in (True, False):
                # a dozen halvings land near the cut: the spread does not depend on hitting it
                a, b = (1e-3 * X_hat, X_hat) if lower else (X_hat, 3.0 * X_hat)
                for _ in range(12):
                    x = 0.5 * (a + b)
                    if (g.deviance(x, F_hat, 1e-10)[0] > q) == lower:
                        a = x
                    else:
                        b = x
                d13, F13 = g.deviance(x, F_hat)
                d10, _ = g.deviance(x, F_hat10, 1e-10)
                rel = abs(d13 - d10) / (abs(F_hat) + abs(F13))
                worst = max(worst, rel)
                print(threads, members, "x", x, "X_hat", X_hat, "D 1e-13", d13, "D 1e-10", d10, "spread / (|F_hat| + |F_pinned|)", rel)
    print("largest spread", worst)
    return worst


if __name__ == "__main__":
    measure_spread()
