"""The two-sample test of isoform usage (include/emsar_hip.h "two-sample test of isoform usage"): its independent reference in numpy and
the genes it is tried on, shared by test_compare_usage_cpu.py and test_compare_usage_gpu.py.  Problems, samples and genes are those of
tests/compare_problems.py and tests/compare_gene_problems.py; nothing the device computes enters anything here.

P_k(u) = max {F^k : theta_t = u X} of one sample comes from the dual: the parts of the gene (GP.parts_of) are solved by plain EM (CP.em's
iteration, to a relative step of 1e-13, warm-started from the previous multiplier's point with every value raised to at least a
hundredth of the largest: EM leaves a value near 0 too slowly for the stopping rule to see) with den_t + lambda (1 - u) on t and
den_s - lambda u on the other members, F with the original den is F_shifted + sum x (den' - den); g(lambda) = theta_t - u X falls in
lambda and a bracketed search (Illinois steps with bisection as the safeguard, the signs at the ends of the range known) finds its
root.  Two values come back per sample and u:
    dual    F - lambda g at the last multiplier: >= P_k(u) whatever the multiplier;
    feas    F of a primal FEASIBLE point: the last point with theta_t, or with the other members, rescaled onto theta_t = u X, or with
            every member at 0 (X = 0 satisfies the constraint too; split_problem's sample A ends there), the best of the three: <= P_k(u).
The outer maximum over u is taken on a grid of 201 shares over [min u_hat, max u_hat], then by golden-section refinement between the
neighbours of the best grid point (on the dual values).  Lambda_ref is the midpoint of [2 (F1 - dual), 2 (F1 - feas)] at the best u and
w_ref its width, the reference's own error.  `peaks` counts the local maxima of the grid: the tested genes have one."""
import json
import os

import numpy as np

from tests import compare_gene_problems as GP
from tests import compare_problems as CP

GRID = 201
GOLD = 0.6180339887498949


def _em(part, den, x0):
    """CP.em's iteration on one part from x0 -> (x, F with den)"""
    b = part.block
    x = np.where(den > 0, x0, 0.0)
    safe = np.where(den > 0, den, 1.0)
    for _ in range(CP.MAX_PASSES):
        S = np.bincount(b.rowid, weights=x[b.col], minlength=b.n_r)
        w = np.where(S > 0, b.R / np.where(S > 0, S, 1.0), 0.0)
        acc = np.bincount(b.col, weights=w[b.rowid], minlength=len(x))
        y = np.where(den > 0, x * acc / safe, 0.0)
        step = np.max(np.abs(y - x) / (np.abs(y) + 1e-6)) if len(x) else 0.0
        x = y
        if step < CP.REL_STEP:
            break
    S = np.bincount(b.rowid, weights=x[b.col], minlength=b.n_r)
    ok = S > 0
    return x, float(np.sum(b.R[ok] * np.log(S[ok]))) - float(np.dot(x, den))


class Sample:
    """the gene's parts in one sample and transcript t among them"""

    def __init__(self, prob, R, den, members, t):
        self.parts = GP.parts_of(prob, R, den, members)
        self.is_t = [p.is_member & (p.tids == t) for p in self.parts]
        self.others = [p.is_member & (p.tids != t) for p in self.parts]
        self.den_t = float(den[t])
        rest = [float(p.den[o].min()) for p, o in zip(self.parts, self.others) if o.any()]
        self.mn = min(rest) if rest else np.inf
        self.members = int(sum(p.is_member.sum() for p in self.parts))
        self.start = [np.ones(len(p.tids)) for p in self.parts]

    def at(self, lam, u, warm=None):
        """-> dict(x per part, th, X, F with the original den) at the multiplier lam"""
        xs, th, X, F = [], 0.0, 0.0, 0.0
        for k, p in enumerate(self.parts):
            den = np.where(self.is_t[k], p.den + lam * (1.0 - u), np.where(self.others[k], p.den - lam * u, p.den))
            x, Fs = _em(p, den, self.start[k] if warm is None else np.maximum(warm[k], 1e-2 * warm[k].max()))
            xs.append(x)
            th += float(x[self.is_t[k]].sum())
            X += float(x[p.is_member].sum())
            F += Fs + float(np.dot(x, den - p.den))
        return dict(lam=lam, xs=xs, th=th, X=X, F=F, g=th - u * X)

    def F_at(self, xs):
        return sum(p.F_at(x) for p, x in zip(self.parts, xs))

    def feasible(self, e, u):
        """the best of the feasible points made from the point e (module docstring)"""
        O = e["X"] - e["th"]
        cands = []
        if O > 0:        # t set to the share u of the others' sum
            cands.append(self.F_at([np.where(it, 0.0, x) + it * (u * O / (1.0 - u)) for x, it in zip(e["xs"], self.is_t)]))
        if e["th"] > 0 and O > 0:      # the others scaled
            c = e["th"] * (1.0 - u) / (u * O)
            cands.append(self.F_at([np.where(o, x * c, x) for x, o in zip(e["xs"], self.others)]))
        # the gene absent altogether: theta_t = u X holds with X = 0 (where the reads of the members' rows can go to their neighbours)
        cands.append(self.F_at([np.where(p.is_member, 0.0, x) for x, p in zip(e["xs"], self.parts)]))
        return max(cands)

    def profile(self, u, e0, evals=60, g_stop=0.0):
        """P(u) -> dict(dual, feas, lam, X, th, evals); e0 = self.at(0, .)"""
        g0 = e0["th"] - u * e0["X"]
        if g0 == 0.0:
            return dict(dual=e0["F"], feas=e0["F"], lam=0.0, X=e0["X"], th=e0["th"], evals=0)
        up = g0 > 0
        end = self.mn / u if up else -self.den_t / (1.0 - u)
        h = lambda e: e["g"] / (e["th"] + u * e["X"])
        v_lo, h_lo, v_hi, h_hi, kept = 0.0, g0 / (e0["th"] + u * e0["X"]), 1.0, (-1.0 if up else 1.0), 0
        last, n = dict(e0, lam=0.0, g=g0), 0
        while n < evals:
            v = 0.5 * (v_lo + v_hi)
            vs = v_lo - h_lo * (v_hi - v_lo) / (h_hi - h_lo)
            if v_lo < vs < v_hi and n % 3 != 2:          # every third step a plain bisection
                v = vs
            if not (v_lo < v < v_hi):
                break
            last = self.at(v * end, u, warm=last["xs"])
            n += 1
            hv = h(last)
            if hv == 0.0 or abs(2.0 * last["lam"] * last["g"]) <= g_stop:
                break
            if (hv > 0) == (h_lo > 0):
                v_lo, h_lo = v, hv
                h_hi *= 0.5 if kept == 1 else 1.0
                kept = 1
            else:
                v_hi, h_hi = v, hv
                h_lo *= 0.5 if kept == -1 else 1.0
                kept = -1
            if abs(2.0 * last["g"] * (v_hi - v_lo) * end) <= g_stop:
                break
        return dict(dual=last["F"] - last["lam"] * last["g"], feas=self.feasible(last, u), lam=last["lam"], X=last["X"], th=last["th"], evals=n)


def count_peaks(v, noise):
    """local maxima of the sequence v that stand out by more than `noise` (the reference's own error in a value): a fall of more than
    noise after a rise of more than noise"""
    peaks, rising, ext = 0, True, v[0]
    for x in v[1:]:
        if rising:
            if x > ext:
                ext = x
            elif x < ext - noise:
                peaks, rising, ext = peaks + 1, False, x
        else:
            if x < ext:
                ext = x
            elif x > ext + noise:
                rising, ext = True, x
    return peaks + (1 if rising else 0)


def reference(prob, RA, RB, members, t, den_a=None, den_b=None, grid=GRID, g_stop=1e-9, refine=30):
    """Lambda of transcript t of the gene `members` -> dict(lam, w_ref, lo, hi, F1, usage_a, usage_b, usage_null, peaks, parts, solves,
    grid_u, grid_v), or None where the test does not apply (t outside, a single member, a gene sum of 0)"""
    den_a = CP.den_of(prob) if den_a is None else den_a
    den_b = CP.den_of(prob) if den_b is None else den_b
    members = np.asarray(sorted(int(m) for m in members))
    if not (den_a[t] > 0 and den_b[t] > 0):
        return None
    A, B = Sample(prob, RA, den_a, members, t), Sample(prob, RB, den_b, members, t)
    if A.members < 2 or B.members < 2:
        return None
    ea, eb = A.at(0.0, 0.5), B.at(0.0, 0.5)
    if not (ea["X"] > 0 and eb["X"] > 0):
        return None
    F1 = ea["F"] + eb["F"]
    ua, ub = ea["th"] / ea["X"], eb["th"] / eb["X"]
    out = dict(F1=F1, usage_a=ua, usage_b=ub, parts=len(A.parts) + len(B.parts), solves=0)
    if ua == ub:
        return dict(out, lam=0.0, w_ref=0.0, lo=0.0, hi=0.0, usage_null=ua, peaks=1, grid_u=np.array([ua]), grid_v=np.array([F1]))

    def both(u):
        pa, pb = A.profile(u, ea, g_stop=g_stop), B.profile(u, eb, g_stop=g_stop)
        out["solves"] += (pa["evals"] * len(A.parts) + pb["evals"] * len(B.parts))
        return pa["dual"] + pb["dual"], pa["feas"] + pb["feas"], pa, pb
    us = np.linspace(min(ua, ub), max(ua, ub), grid)
    vals = np.array([both(u)[0] for u in us[1:-1]])
    # the ends: at u = u_hat_k that sample is free and the other one's profile is evaluated like any point
    ends = [both(min(max(u, 1e-12), 1.0 - 1e-12))[0] for u in (us[0], us[-1])]
    gv = np.concatenate([[ends[0]], vals, [ends[1]]])
    peaks = count_peaks(gv, 1e-8 + 1e-12 * abs(F1))
    k = int(np.argmax(gv))
    lo_u, hi_u = us[max(k - 1, 0)], us[min(k + 1, len(us) - 1)]
    lo_u, hi_u = min(max(lo_u, 1e-12), 1 - 1e-12), min(max(hi_u, 1e-12), 1 - 1e-12)
    x1, x2 = hi_u - GOLD * (hi_u - lo_u), lo_u + GOLD * (hi_u - lo_u)
    f1, f2 = both(x1), both(x2)
    best = (gv[k], None, min(max(us[k], 1e-12), 1 - 1e-12))
    for _ in range(refine):
        if f1[0] < f2[0]:
            lo_u, x1, f1 = x1, x2, f2
            x2 = lo_u + GOLD * (hi_u - lo_u)
            f2 = both(x2)
        else:
            hi_u, x2, f2 = x2, x1, f1
            x1 = hi_u - GOLD * (hi_u - lo_u)
            f1 = both(x1)
    u_best, f_best = (x1, f1) if f1[0] >= f2[0] else (x2, f2)
    if best[0] > f_best[0]:
        u_best, f_best = best[2], both(best[2])
    lo, hi = 2.0 * (F1 - f_best[0]), 2.0 * (F1 - f_best[1])
    return dict(out, lam=0.5 * (lo + hi), w_ref=abs(hi - lo), lo=lo, hi=hi, usage_null=u_best, peaks=peaks, grid_u=us, grid_v=gv,
                point_parts=len(A.parts) + len(B.parts))


def lone_pair_lambda(u_a, den_a, u_b, den_b):
    """A gene of two one-transcript components, t first: with theta_t = o theta_s in both samples,
        theta_s = (u_t + u_s) / (o den_t + den_s),  P(o) = u_t log o + (u_t + u_s) log theta_s - (u_t + u_s),
    maximised over log o by golden section on the concave sum (P is concave in log o) -> (Lambda, the common share)"""
    u_a, den_a, u_b, den_b = (np.asarray(x, dtype=np.float64) for x in (u_a, den_a, u_b, den_b))

    def P(z, u, d):
        n = u[0] + u[1]
        return u[0] * z + n * np.log(n / (np.exp(z) * d[0] + d[1])) - n

    def F(u, d):
        ok = u > 0
        return float(np.sum(u[ok] * np.log(u[ok] / d[ok]))) - float(u.sum())
    f = lambda z: P(z, u_a, den_a) + P(z, u_b, den_b)
    lo, hi = -40.0, 40.0
    x1, x2 = hi - GOLD * (hi - lo), lo + GOLD * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(200):
        if f1 < f2:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + GOLD * (hi - lo)
            f2 = f(x2)
        else:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - GOLD * (hi - lo)
            f1 = f(x1)
    z = 0.5 * (lo + hi)
    return 2.0 * (F(u_a, den_a) + F(u_b, den_b) - f(z)), float(np.exp(z) / (1.0 + np.exp(z)))


def lone_problem(u_a, den_a, u_b, den_b):
    """one-transcript rows only, with den given: every member is a closed-form part -> (prob, RA, RB, den_a, den_b)"""
    n = len(u_a)
    n_tx, rp, ci = CP.csr([[t] for t in range(n)], n)
    RA, RB = np.asarray(u_a, dtype=np.int32), np.asarray(u_b, dtype=np.int32)
    prob = (n_tx, rp, ci, RA, np.ones(n))
    return prob, RA, RB, np.asarray(den_a, dtype=np.float64), np.asarray(den_b, dtype=np.float64)


# ---- the genes the tests compare with the reference, by name: (gene, t) -----------------------------------------------------------------
_refs = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_usage_refs.json")
KEPT = ("lam", "w_ref", "lo", "hi", "F1", "usage_a", "usage_b", "usage_null", "peaks", "parts", "solves")


def small_case(members, t):
    prob, RA, RB, den_a, den_b = CP.small_problem()
    return prob, RA, RB, den_a, den_b, list(members), t


def _class(threads, k, which):
    prob, RA, RB, _ = CP.class_problem(threads)
    members = GP.class_genes(threads)[k]
    den = CP.den_of(prob)
    return prob, RA, RB, den, den, members, members[which]


def _mixed():
    prob, RA, RB, members = GP.mixed_problem()
    den = CP.den_of(prob)
    return prob, RA, RB, den, den, members, members[0]


def _split():
    prob, RA, RB, members = CP.split_problem()
    den = CP.den_of(prob)
    return prob, RA, RB, den, den, members, members[0]


def _awkward():
    from tests import awkward_problems as AP
    prob, (RA, RB), members = AP.awkward_problem(), AP.awkward_samples(), GP.awkward_gene()
    den = CP.den_of(prob)
    return prob, RA, RB, den, den, members, members[0]


# every (gene, t) the tests compare with the reference, by name
CASES = {
    "class64-0": lambda: _class(64, 0, 0),
    "class64-1": lambda: _class(64, 1, 0),
    "class64-2": lambda: _class(64, 2, 1),
    "class256": lambda: _class(256, 0, 0),
    "class512": lambda: _class(512, 0, 0),
    "small-0-3-6:0": lambda: small_case([0, 3, 6], 0),          # t is a closed-form part of both samples
    "small-0-3-6:3": lambda: small_case([0, 3, 6], 3),
    "small-0-3-6:6": lambda: small_case([0, 3, 6], 6),
    "mixed": _mixed,
    "split": _split,
    "awkward": _awkward,
}


def case(name):
    """-> (prob, RA, RB, den_a, den_b, members, t)"""
    return CASES[name]()


def recorded():
    """the references kept in tests/golden/compare_usage_refs.json (python -m tests.compare_usage_problems --write NAME ... computes
    them: a 201-point grid of bracketed searches over plain EMs takes from ten seconds to hours per gene)"""
    if "recorded" not in _refs:
        with open(GOLDEN) as f:
            _refs["recorded"] = json.load(f)
    return _refs["recorded"]


def tested_reference(name):
    """the recorded reference of a case -> dict of KEPT"""
    return recorded()[name]


if __name__ == "__main__":
    import sys
    import time
    write = "--write" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    for name in names:
        t0 = time.time()
        r = reference(*case(name)[:3], case(name)[5], case(name)[6], case(name)[3], case(name)[4])
        kept = {k: (int(r[k]) if k in ("peaks", "parts", "solves") else float(r[k])) for k in KEPT}
        print(name, kept, "%.1f s" % (time.time() - t0), flush=True)
        if write:
            have = json.load(open(out)) if os.path.exists(out) else {}
            have[name] = kept
            with open(out, "w") as f:
                json.dump(have, f, indent=1, sort_keys=True)
                f.write("\n")
