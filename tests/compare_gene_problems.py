"""The gene-level two-sample test (include/emsar_hip.h "gene-level two-sample test"): its independent reference in numpy and the genes
it is tried on, shared by test_compare_genes_cpu.py and test_compare_genes_gpu.py.  Problems and samples are those of
tests/compare_problems.py; nothing the device computes enters anything here.

The reference works on the dual.  In one sample the members of the gene with den > 0 fall into parts (CP.component of each member);
an evaluation at a multiplier lambda is CP.em on every part with the members' den shifted by +lambda (A) or -r lambda (B), to a relative
step of 1e-13, and F with the original den is F_shifted + shift * X_part.  g(lambda) = X_A - r X_B falls in lambda; a bracketed search
finds its root.  Two values come back:
    L       the dual value F_A + F_B - lambda g at the last multiplier: L >= F0 whatever the multiplier;
    F_feas  F of a primal FEASIBLE point made from the last evaluation: F_feas <= F0 whatever the multiplier.  Two candidates, the
            better one is kept: A's members rescaled so that X_A = r X_B (when both sums are positive), and the point that adds the
            missing amount to the member with the smallest den on the side that is short (the only finite one when that side's sum is
            exactly 0 because no read supports it: the root then lies at the end of the range, where that member's den' is 0 and its
            value is free).
Lambda_ref is the midpoint of [2 (F1 - L), 2 (F1 - F_feas)], and its width w_ref is the reference's own error."""
import numpy as np

from tests import compare_problems as CP


class Part:
    """one connected set of one sample that holds members of the gene: tids, the rows as a CP.Block, den, which local columns are members"""

    def __init__(self, prob, R, den, tids, rows, members):
        self.tids = tids
        self.block = CP.Block(prob, R, tids, rows)
        self.den = den[tids].astype(np.float64)
        self.is_member = np.isin(tids, members) & (self.den > 0)
        self.ident = np.arange(len(tids))

    def solve(self, shift):
        """(x, X_part, F with the original den) at den' = den + shift on the members"""
        den = np.where(self.is_member, self.den + shift, self.den)
        x, F, _ = CP.em(len(self.tids), [(self.block, self.ident, 1.0)], den)
        X = float(x[self.is_member].sum())
        return x, X, F + shift * X

    def F_at(self, x):
        b = self.block
        S = np.bincount(b.rowid, weights=x[b.col], minlength=b.n_r)
        inside = np.bincount(b.rowid, weights=self.den[b.col], minlength=b.n_r) > 0      # a row of den = 0 transcripts alone is outside F, as in CP.em
        if np.any((S <= 0) & (b.R > 0) & inside):
            return -np.inf
        ok = S > 0
        return float(np.sum(b.R[ok] * np.log(S[ok]))) - float(np.dot(x, self.den))


def parts_of(prob, R, den, members):
    """the parts of the gene in one sample, by the smallest member tid; a member with den == 0 takes no part"""
    parts, seen = [], set()
    for t in sorted(int(m) for m in members):
        if not den[t] > 0 or t in seen:
            continue
        tids, rows = CP.component(prob, R, t)
        seen.update(int(x) for x in tids)
        parts.append(Part(prob, R, den, tids, rows, np.asarray(members)))
    return parts


def evaluate(parts, shift):
    """-> (list of x per part, X, F) of one sample at a shift"""
    xs, X, F = [], 0.0, 0.0
    for p in parts:
        x, Xp, Fp = p.solve(shift)
        xs.append(x)
        X += Xp
        F += Fp
    return xs, X, F


def _scaled(parts, xs, c):
    return sum(p.F_at(np.where(p.is_member, x * c, x)) for p, x in zip(parts, xs))


def _filled(parts, xs, amount):
    """F with `amount` added to the member with the smallest den"""
    best = min((float(p.den[i]), k, int(i)) for k, p in enumerate(parts) for i in np.flatnonzero(p.is_member))
    F = 0.0
    for k, (p, x) in enumerate(zip(parts, xs)):
        if k == best[1]:
            x = x.copy()
            x[best[2]] += amount
        F += p.F_at(x)
    return F


def feasible_value(pa, xa, Xa, pb, xb, Xb, ratio):
    """the best of the feasible candidates (module docstring)"""
    cands = []
    if Xa > 0 and Xb > 0:
        cands.append(_scaled(pa, xa, ratio * Xb / Xa) + sum(p.F_at(x) for p, x in zip(pb, xb)))
    g = Xa - ratio * Xb
    if g >= 0:
        cands.append(sum(p.F_at(x) for p, x in zip(pa, xa)) + _filled(pb, xb, g / ratio))
    else:
        cands.append(_filled(pa, xa, -g) + sum(p.F_at(x) for p, x in zip(pb, xb)))
    return max(cands)


def reference(prob, RA, RB, members, ratio=1.0, den_a=None, den_b=None, method="bisect", evals=None):
    """Lambda of the gene `members` -> dict(lam, w_ref, lo, hi, F1, L, F_feas, gene_a, gene_b, gene_null, multiplier, parts, evals).
    method "bisect": plain bisection of the range, 50 evaluations; "secant": Illinois steps on h = g / (X_A + r X_B) with the known
    values -+1 at the ends of the range, 14 evaluations (the large classes, where an evaluation costs seconds)."""
    den_a = CP.den_of(prob) if den_a is None else den_a
    den_b = CP.den_of(prob) if den_b is None else den_b
    members = np.asarray(sorted(int(m) for m in members))
    pa, pb = parts_of(prob, RA, den_a, members), parts_of(prob, RB, den_b, members)
    if not pa or not pb:
        return None
    min_a = min(float(p.den[p.is_member].min()) for p in pa)
    min_b = min(float(p.den[p.is_member].min()) for p in pb)
    evals = evals or (50 if method == "bisect" else 14)

    def at(lam):
        xa, Xa, Fa = evaluate(pa, lam)
        xb, Xb, Fb = evaluate(pb, -ratio * lam)
        return dict(lam=lam, xa=xa, Xa=Xa, Fa=Fa, xb=xb, Xb=Xb, Fb=Fb, g=Xa - ratio * Xb)
    e0 = at(0.0)
    F1 = e0["Fa"] + e0["Fb"]
    last, n = e0, 1
    if e0["g"] != 0.0:
        end = min_b / ratio if e0["g"] > 0 else -min_a
        h = lambda e: e["g"] / (e["Xa"] + ratio * e["Xb"])
        v_lo, h_lo, v_hi, h_hi, kept = 0.0, h(e0), 1.0, (-1.0 if e0["g"] > 0 else 1.0), 0
        while n < evals:
            v = 0.5 * (v_lo + v_hi)
            if method == "secant":
                vs = v_lo - h_lo * (v_hi - v_lo) / (h_hi - h_lo)
                if v_lo < vs < v_hi:
                    v = vs
            if not (v_lo < v < v_hi):
                break
            last = at(v * end)
            n += 1
            hv = h(last)
            if hv == 0.0:
                break
            if (hv > 0) == (h_lo > 0):
                v_lo, h_lo = v, hv
                h_hi *= 0.5 if kept == 1 else 1.0
                kept = 1
            else:
                v_hi, h_hi = v, hv
                h_lo *= 0.5 if kept == -1 else 1.0
                kept = -1
    L = last["Fa"] + last["Fb"] - last["lam"] * last["g"]
    F_feas = feasible_value(pa, last["xa"], last["Xa"], pb, last["xb"], last["Xb"], ratio)
    lo, hi = 2.0 * (F1 - L), 2.0 * (F1 - F_feas)
    # |.|: both ends carry the EM's own error (a relative step of 1e-13), which can put them the other way round by 1e-10
    return dict(lam=0.5 * (lo + hi), w_ref=abs(hi - lo), lo=lo, hi=hi, F1=F1, L=L, F_feas=F_feas, gene_a=e0["Xa"], gene_b=e0["Xb"],
                gene_null=last["Xa"], multiplier=last["lam"], gap=last["g"], parts=len(pa) + len(pb), evals=n)


def closed_gene_lambda(u_a, den_a, u_b, den_b, ratio=1.0):
    """A gene of one-transcript components, solved without the library's search: the root of
    sum u_A / (den_A + lambda) = r sum u_B / (den_B - r lambda) by plain bisection in lambda (200 halvings), Lambda from the primal
    values there.  One side without reads: the root is the end of the range and Lambda its limit, 2 sum u log(1 + shift / den) on the
    side with reads.  -> (Lambda, lambda)"""
    u_a, den_a, u_b, den_b = (np.asarray(x, dtype=np.float64) for x in (u_a, den_a, u_b, den_b))

    def F(u, x, d):
        ok = u > 0
        return float(np.sum(u[ok] * np.log(x[ok]))) - float(np.dot(x, d))
    xa0, xb0 = u_a / den_a, u_b / den_b
    g0 = xa0.sum() - ratio * xb0.sum()
    if g0 == 0.0:
        return 0.0, 0.0
    lo, hi = (0.0, den_b.min() / ratio) if g0 > 0 else (-den_a.min(), 0.0)
    g = lambda lam: float(np.sum(u_a / (den_a + lam))) - ratio * float(np.sum(u_b / (den_b - ratio * lam)))
    if u_a.sum() == 0 or u_b.sum() == 0:
        lam = hi if g0 > 0 else lo
        side_u, side_d, shift = (u_a, den_a, lam) if u_b.sum() == 0 else (u_b, den_b, -ratio * lam)
        ok = side_u > 0
        return 2.0 * float(np.sum(side_u[ok] * np.log1p(shift / side_d[ok]))), lam
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if g(mid) > 0:
            lo = mid
        else:
            hi = mid
    lam = 0.5 * (lo + hi)
    xa, xb = u_a / (den_a + lam), u_b / (den_b - ratio * lam)
    return 2.0 * (F(u_a, xa0, den_a) + F(u_b, xb0, den_b) - F(u_a, xa, den_a) - F(u_b, xb, den_b)), lam


def gene_map(n_tx, genes):
    """gene_of_tx for a list of member lists (every other transcript has no gene)"""
    g = np.full(n_tx, -1, dtype=np.int32)
    for k, members in enumerate(genes):
        g[list(members)] = k
    return g


def class_genes(threads):
    """the genes tried on CP.class_problem(threads): 64 -> three genes of three members (the two tested tids apart, with neighbours);
    256, 512 -> one gene of the two tested tids plus a neighbour"""
    prob, RA, RB, tids = CP.class_problem(threads)
    t0, t1 = tids
    if threads == 64:
        free = [t for t in range(prob[0]) if t not in tids]
        return [[t0, free[0], free[1]], [t1, free[2], free[3]], [free[4], free[5], free[6]]]
    return [[t0, t1, t0 + 1 if t0 + 1 != t1 else t0 + 2]]


_mixed = {}


def mixed_problem():
    """a 64-class and a 256-class edge set side by side under two fitted samples; the gene holds one transcript of each
    -> (prob, RA, RB, gene)"""
    from tests import set_problems as SP
    if not _mixed:
        n_tx, rp, ci, R, E, members = SP.compose_members([SP.edge_set(*SP.EDGES[0][0], seed=SP.SEEDS[0]), SP.edge_set(*SP.EDGES[4][0], seed=SP.SEEDS[4])], seed=77)
        prob = (n_tx, rp, ci, R, E)
        gene = [int(members[0][0][3]), int(members[1][0][11])]
        _mixed["p"] = (prob, CP.fitted_weights(prob, 51), CP.fitted_weights(prob, 52, apart=gene), gene)
    return _mixed["p"]


def awkward_gene():
    """on awkward_problem: a transcript that occurs twice in a row, the den = 0 transcript and the one alone in its row"""
    from tests import awkward_problems as AP
    prob, notes = AP.awkward_members()
    return [int(AP.twice_in_a_row(prob)[0]), int(notes["outside"]), int(notes["alone"])]


# every gene the GPU tests compare with the reference, by name
TESTED_GENES = ("class64-0", "class64-1", "class64-2", "class256", "class512", "small-0-3-6", "small-4-10", "mixed", "split", "awkward")
_refs = {}


def tested_reference(name):
    """the reference of a gene of TESTED_GENES with what it was taken on, computed once per session -> (dict of reference(), members)"""
    if name not in _refs:
        if name.startswith("class"):
            threads, _, k = name[5:].partition("-")
            prob, RA, RB, _ = CP.class_problem(int(threads))
            members = class_genes(int(threads))[int(k or 0)]
            _refs[name] = (reference(prob, RA, RB, members, method="bisect" if threads == "64" else "secant"), members)
        elif name.startswith("small"):
            prob, RA, RB, den_a, den_b = CP.small_problem()
            members = [int(x) for x in name.split("-")[1:]]
            _refs[name] = (reference(prob, RA, RB, members, 1.0, den_a, den_b), members)
        elif name == "mixed":
            prob, RA, RB, members = mixed_problem()
            _refs[name] = (reference(prob, RA, RB, members, method="secant"), members)
        elif name == "split":
            prob, RA, RB, members = CP.split_problem()
            _refs[name] = (reference(prob, RA, RB, members, method="secant"), members)
        else:
            from tests import awkward_problems as AP
            prob, (RA, RB), members = AP.awkward_problem(), AP.awkward_samples(), awkward_gene()
            _refs[name] = (reference(prob, RA, RB, members), members)
    return _refs[name]
