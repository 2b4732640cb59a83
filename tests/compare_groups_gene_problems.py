"""The gene-level K-sample test across replicate groups (include/emsar_hip.h "gene-level K-sample test"): its independent reference in
numpy and the genes it is tried on, shared by test_compare_groups_genes_cpu.py and test_compare_groups_genes_gpu.py.  Problems and
samples are those of tests/compare_problems.py, tests/compare_gene_problems.py (GP) and tests/compare_groups_problems.py (CGP); nothing
the device computes enters anything here.

A gene-sum constraint X^k = s_k x cannot be stacked into one plain EM the way the transcript test's shared column can, so the reference
bounds C_g(S) = max_x sum_{k in S} P_k(s_k x) from both sides and knows nothing of the library's search:
    U   for ANY multipliers with sum_k s_k lambda_k = 0,  C_g(S) <= sum_k max [F^k - lambda_k X^k]  (the x-term of the Lagrangian
        vanishes).  The multipliers are the roots of a plain nested bisection with secant points (outer on x between the smallest and
        the largest X_hat^k / s_k, inner on lambda_k until X^k(lambda_k) = s_k x), projected onto that hyperplane,
        lambda_k - s_k (sum_j s_j lambda_j) / sum_j s_j^2, and every sample is evaluated again there; a projected multiplier outside
        (-mn^k, inf) refuses the case.  One evaluation is GP's: a plain EM on every part with the members' den shifted (here to a
        relative step of CGP.REL_STEP), F with the original den = F_shifted + lambda X.  An EM errs low, so its own mixture bound
        (CGP.mixture_bound, at the shifted den) is added.
    L   F at a primal feasible point: in every sample the members of the last evaluation rescaled so that X^k = s_k x; where X^k = 0
        because no read supports it, the amount is added to the member with the smallest den (GP._filled).  Evaluated exactly
        (Part.F_at).
C_ref is the midpoint and U - L the reference's own error.  A sample in which every member taking part is a lone transcript without
reads is closed form: P_k(y) = -mn^k y, its multiplier is -mn^k at every target (the end of the range), and the projection leaves
it there (it runs over the other samples, the sum s_k lambda_k = 0 taken over all).
A free fit F_hat^k errs low by at most its mixture bounds: its interval is [F_hat, F_hat + bound].  w_between and w_within are the sums
of the widths and bounds of the fits that enter each Lambda, times 2.

record() (python -m tests.compare_groups_gene_problems) writes the cases that take minutes in numpy to
tests/golden/compare_groups_gene_refs.json; it refuses a case whose w exceeds W_REF_MAX or one of whose EMs ended at MAX_PASSES."""
import json
import os

import numpy as np

from tests import compare_gene_problems as GP
from tests import compare_groups_problems as CGP
from tests import compare_problems as CP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_groups_gene_refs.json")
W_REF_MAX = CGP.W_REF_MAX            # 1e-7: the cap of test_compare_genes_gpu.py and compare_groups_problems.py
INNER_STEPS, OUTER_STEPS = 40, 30    # evaluations at most per level
INNER_REL, OUTER_REL = 1e-10, 1e-8   # a level ends when its residual or its bracket is this small (relative): U - L is of second order in both


def sample_at(parts, shift):
    """one sample at a shift on every member's den -> dict(shift, xs, X, F (original den), bound, ended)"""
    xs, X, F, bound, ended = [], 0.0, 0.0, 0.0, True
    for p in parts:
        den = np.where(p.is_member, p.den + shift, p.den)
        blocks = [(p.block, p.ident, 1.0)]
        x, Fs, passes = CP.em(len(p.tids), blocks, den, rel_step=CGP.REL_STEP)
        Xp = float(x[p.is_member].sum())
        xs.append(x)
        X += Xp
        F += Fs + shift * Xp
        bound += CGP.mixture_bound(len(p.tids), blocks, den, x)
        ended = ended and passes < CP.MAX_PASSES
    return dict(shift=shift, xs=xs, X=X, F=F, bound=bound, ended=ended)


class Sample:
    """the gene's parts in one sample, its free fit and the inner root"""

    def __init__(self, prob, R, den, members, size):
        self.parts = GP.parts_of(prob, R, den, members)
        self.size = float(size)
        self.mn = min(float(p.den[p.is_member].min()) for p in self.parts) if self.parts else np.inf
        self.hat = sample_at(self.parts, 0.0) if self.parts else None
        # every member taking part alone in its rows and without reads: P(y) = -mn y
        self.dead = bool(self.parts) and all(len(p.tids) == 1 and p.block.R.sum() == 0 for p in self.parts)
        self.ended = self.hat["ended"] if self.hat else True

    def at(self, shift):
        e = sample_at(self.parts, shift)
        self.ended = self.ended and e["ended"]
        return e

    def root(self, y):
        """the multiplier at which X(lambda) = y (X falls in lambda) -> lambda.  Bisection of v in (0, 1) -- lambda = mn v / (1 - v) where
        the sum must shrink, -mn v where it must grow -- with the secant point of h = (X - y) / (X + y) tried first (h = -+1 at v = 1)"""
        X0 = self.hat["X"]
        if self.dead:
            return -self.mn
        if y == X0:
            return 0.0
        shrink = y < X0
        lam_of = (lambda v: self.mn * v / (1.0 - v)) if shrink else (lambda v: -self.mn * v)
        v_lo, h_lo, v_hi, h_hi, kept = 0.0, (X0 - y) / (X0 + y), 1.0, (-1.0 if shrink else 1.0), 0
        v = 0.0
        for _ in range(INNER_STEPS):
            v = 0.5 * (v_lo + v_hi)
            vs = v_lo - h_lo * (v_hi - v_lo) / (h_hi - h_lo)
            if v_lo < vs < v_hi:
                v = vs
            if not (v_lo < v < v_hi):
                break
            X = self.at(lam_of(v))["X"]
            h = (X - y) / (X + y)
            if abs(h) <= INNER_REL:
                break
            if (h > 0) == (h_lo > 0):
                v_lo, h_lo = v, h
                h_hi *= 0.5 if kept == 1 else 1.0
                kept = 1
            else:
                v_hi, h_hi = v, h
                h_lo *= 0.5 if kept == -1 else 1.0
                kept = -1
            if v_hi - v_lo <= INNER_REL * (1.0 - v_lo):
                break
        return lam_of(v)

    def feasible(self, e, y):
        """F at a point with X = y made from the evaluation e"""
        if e["X"] > 0:
            return GP._scaled(self.parts, e["xs"], y / e["X"])
        return GP._filled(self.parts, e["xs"], y)


def common_fit(samples, S):
    """C_g(S) from both sides -> dict(C, U, L, width, x)"""
    xs = [samples[k].hat["X"] / samples[k].size for k in S]
    lo, hi = min(xs), max(xs)
    slope = lambda lam: sum(samples[k].size * l for k, l in zip(S, lam))
    x, lam = lo, [0.0 if not samples[k].dead else -samples[k].mn for k in S]
    if lo < hi:
        h_lo, h_hi, kept = 1.0, -1.0, 0                 # sum s_k lambda_k over sum |s_k lambda_k|: its signs at the ends are known
        for _ in range(OUTER_STEPS):
            mid = 0.5 * (lo + hi)
            xs_ = lo - h_lo * (hi - lo) / (h_hi - h_lo)
            if lo < xs_ < hi:
                mid = xs_
            if not (lo < mid < hi):
                break
            x = mid
            lam = [samples[k].root(samples[k].size * x) for k in S]
            ab = sum(abs(samples[k].size * l) for k, l in zip(S, lam))
            h = slope(lam) / ab if ab > 0 else 0.0
            if abs(h) <= OUTER_REL:
                break
            if h > 0:
                lo, h_lo = mid, h
                h_hi *= 0.5 if kept == 1 else 1.0
                kept = 1
            else:
                hi, h_hi = mid, h
                h_lo *= 0.5 if kept == -1 else 1.0
                kept = -1
            if (hi - lo) <= OUTER_REL * hi:
                break
    free = [i for i, k in enumerate(S) if not samples[k].dead]
    if lo < hi or any(samples[k].dead for k in S):
        over = slope(lam) / sum(samples[S[i]].size ** 2 for i in free) if free else 0.0
        lam = [l - samples[k].size * over if i in free else l for i, (k, l) in enumerate(zip(S, lam))]
    U = L = 0.0
    for k, l in zip(S, lam):
        s = samples[k]
        assert l > -s.mn or (s.dead and l == -s.mn), ("a projected multiplier left its range", k, l, s.mn)
        e = s.hat if l == 0.0 else s.at(l) if not s.dead else dict(s.hat, shift=l)
        U += e["F"] - l * e["X"] + e["bound"]
        L += s.feasible(e, s.size * x)
    return dict(C=0.5 * (U + L), U=U, L=L, width=abs(U - L), x=x)


def reference(prob, Rs, dens, members, groups, sizes=None):
    """Both Lambdas of the gene `members` and what went into them -> dict(lam_between, lam_within, w_between, w_within, gene_common,
    gene_group, gene_hat, F_hat, parts (per sample), n_members, bracket, searched, ended_by_step); None where a sample has no member
    taking part"""
    K = len(Rs)
    G = max(groups) + 1
    sizes = [1.0] * K if sizes is None else [float(s) for s in sizes]
    members = sorted(int(m) for m in members)
    samples = [Sample(prob, Rs[k], dens[k], members, sizes[k]) for k in range(K)]
    if any(not s.parts for s in samples):
        return None
    F_hat = [s.hat["F"] + 0.5 * s.hat["bound"] for s in samples]
    b_hat = [s.hat["bound"] for s in samples]
    gene_hat = [s.hat["X"] for s in samples]
    al = common_fit(samples, list(range(K)))
    C_group, x_group, w_group, searched = [], [], [], [K]
    for g in range(G):
        S = [k for k in range(K) if groups[k] == g]
        if len(S) == 1:
            C_group.append(F_hat[S[0]]); x_group.append(gene_hat[S[0]] / sizes[S[0]]); w_group.append(b_hat[S[0]])
        elif len(S) == K:
            C_group.append(al["C"]); x_group.append(al["x"]); w_group.append(al["width"])
        else:
            c = common_fit(samples, S)
            C_group.append(c["C"]); x_group.append(c["x"]); w_group.append(c["width"])
            searched.append(len(S))
    xs = [gene_hat[k] / sizes[k] for k in range(K)]
    return dict(lam_between=2.0 * (sum(C_group) - al["C"]), lam_within=2.0 * (sum(F_hat) - sum(C_group)),
                w_between=2.0 * (sum(w_group) + al["width"]), w_within=2.0 * (sum(b_hat) + sum(w_group)),
                gene_common=al["x"], gene_group=x_group, gene_hat=gene_hat, F_hat=F_hat, parts=[len(s.parts) for s in samples],
                n_members=len(members), bracket=max(xs) - min(xs), searched=searched, ended_by_step=bool(all(s.ended for s in samples)))


def closed_gene_groups(members, groups, sizes=None):
    """A gene of one-transcript components in every sample -- members[k] = [(u, den), ..] -- without the library's search: C_g(S) by
    plain bisection, 200 halvings each: inner on lambda_k (sum u / (den + lambda_k) = s_k x), outer on x (sum s_k lambda_k = 0).  A
    sample without reads has P(y) = -mn y.  -> dict(lam_between, lam_within, gene_common, gene_group, gene_hat)"""
    K = len(members)
    s = np.ones(K) if sizes is None else np.asarray(sizes, dtype=np.float64)
    u = [np.asarray([m[0] for m in ms], dtype=np.float64) for ms in members]
    d = [np.asarray([m[1] for m in ms], dtype=np.float64) for ms in members]

    def F(k, x):
        ok = u[k] > 0
        return float(np.sum(u[k][ok] * np.log(x[ok]))) - float(np.dot(x, d[k]))
    hat = [float(np.sum(u[k] / d[k])) for k in range(K)]
    F_hat = [F(k, u[k] / d[k]) for k in range(K)]

    def root(k, y):
        """(lambda, P_k(y))"""
        mn = d[k].min()
        X = lambda lam: float(np.sum(u[k] / (d[k] + lam)))
        if y == hat[k]:
            return 0.0, F_hat[k]
        if y < hat[k]:
            lo, hi = 0.0, mn
            while X(hi) > y:
                lo, hi = hi, 2.0 * hi
        else:
            lo, hi = -mn, 0.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if not (lo < mid < hi):
                break
            if X(mid) > y:
                lo = mid
            else:
                hi = mid
        lam = 0.5 * (lo + hi)
        if lam <= -mn * (1.0 - 1e-12):   # the end of the range: the member at mn (no reads) takes what is missing
            x = np.where(d[k] == mn, 0.0, u[k] / np.where(d[k] == mn, 1.0, d[k] - mn))
            return -mn, F(k, x) - mn * (y - float(x.sum()))
        return lam, F(k, u[k] / (d[k] + lam))

    def C(S):
        xs = [hat[k] / s[k] for k in S]
        lo, hi = min(xs), max(xs)
        if lo == hi:
            return sum(F_hat[k] for k in S), lo
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if sum(s[k] * root(k, s[k] * mid)[0] for k in S) > 0:
                lo = mid
            else:
                hi = mid
        x = 0.5 * (lo + hi)
        return sum(root(k, s[k] * x)[1] for k in S), x
    G = max(groups) + 1
    sets = [[k for k in range(K) if groups[k] == g] for g in range(G)]
    Cg = [C(S) for S in sets]
    Ca = C(list(range(K)))
    return dict(lam_between=2.0 * (sum(c for c, _ in Cg) - Ca[0]), lam_within=2.0 * (sum(F_hat) - sum(c for c, _ in Cg)),
                gene_common=Ca[1], gene_group=[x for _, x in Cg], gene_hat=hat)


# ---- the problems ---------------------------------------------------------------------------------------------------------------
_cache = {}


def small_case(members):
    """a gene on CGP.small_samples(), groups (0, 0, 1) -> (prob, Rs, dens, members, groups, sizes)"""
    prob, Rs, dens = CGP.small_samples()
    return prob, Rs, dens, list(members), (0, 0, 1), None


def awkward_case():
    """GP.awkward_gene() under three samples: the two of awkward_samples() and the first once more with other counts
    -> (prob, Rs, dens, members, groups, sizes)"""
    from tests import awkward_problems as AP
    prob, (RA, RB) = AP.awkward_problem(), AP.awkward_samples()
    RC = np.where(RA > 0, (RA.astype(np.int64) * 3 + 1) // 2, 0).astype(np.int32)
    den = CP.den_of(prob)
    return prob, [RA, RC, RB], [den, den, den], GP.awkward_gene(), (0, 0, 1), None


def class_case(threads, case, gene=0):
    """gene `gene` of GP.class_genes(threads) under CGP.CLASS_CASES' case -> (prob, Rs, dens, members, groups, sizes)"""
    prob, smp, _ = CGP.class_samples(threads)
    _, order, groups, sizes = next(c for c in CGP.CLASS_CASES if c[0] == case)
    den = CP.den_of(prob)
    return prob, [smp[c] for c in order], [den] * len(order), GP.class_genes(threads)[gene], groups, sizes


def mixed_case():
    """GP.mixed_problem's gene (a 64-class and a 256-class part) under three samples -> (prob, Rs, dens, members, groups, sizes)"""
    prob, RA, RB, gene = GP.mixed_problem()
    den = CP.den_of(prob)
    return prob, [RA, CP.fitted_weights(prob, 53), RB], [den] * 3, gene, (0, 0, 1), None


def split_case():
    """CGP.split_samples: the gene's set in the 64 class in one sample (the 11-transcript chain) and in the 512 class in the others.
    The chain's sample is drawn ten times as deep here (scale 300): at CGP's depth its gene sum is a tenth of the others', the roots
    lie far out on the multiplier's range and the reference's own EMs on the chain end at MAX_PASSES there"""
    prob, smp, tids, order, groups = CGP.split_samples()
    den = CP.den_of(prob)
    deep = np.where(smp["A"] > 0, CP.fitted_weights(prob, 1512, scale=300.0), 0).astype(np.int32)
    return prob, [dict(smp, A=deep)[c] for c in order], [den] * 3, list(tids), groups, None


def no_reads_case():
    """The end of the range on the device: gene {0, 1} over the rows {0}, {1}, {0, 1}, {1, 2}, {2}.  In samples A and C every row has
    reads and the gene lies in one set; in B only {2} has reads, so 0 and 1 are lone transcripts without reads: X_hat^B = 0, the member
    at the smallest den (0, den 2) has none, and P_B(y) = -2 y.  -> (prob, Rs, dens, members, groups, sizes)"""
    n_tx, rp, ci = CP.csr([[0], [1], [0, 1], [1, 2], [2]], 3)
    RA = np.array([21, 13, 30, 9, 17], dtype=np.int32)
    RB = np.array([0, 0, 0, 0, 25], dtype=np.int32)
    RC = np.array([35, 8, 22, 14, 11], dtype=np.int32)
    prob = (n_tx, rp, ci, RA, np.ones(5))
    den = CP.den_of(prob)
    return prob, [RA, RB, RC], [den, den, den], [0, 1], (0, 0, 1), None


LIVE = {"small-0-3-6": lambda: small_case([0, 3, 6]), "small-4-10": lambda: small_case([4, 10]), "awkward": awkward_case, "no-reads": no_reads_case}
RECORDED = {
    "class64-0/k3_001": lambda: class_case(64, "k3_001", 0), "class64-1/k3_001": lambda: class_case(64, "k3_001", 1),
    "class64-2/k3_001": lambda: class_case(64, "k3_001", 2),
    "class64-0/k4_0011": lambda: class_case(64, "k4_0011", 0), "class64-1/k4_0011": lambda: class_case(64, "k4_0011", 1),
    "class64-2/k4_0011": lambda: class_case(64, "k4_0011", 2),
    "class64-0/k3_012": lambda: class_case(64, "k3_012", 0), "class64-1/k3_012": lambda: class_case(64, "k3_012", 1),
    "class64-2/k3_012": lambda: class_case(64, "k3_012", 2),
    "class256/k3_001": lambda: class_case(256, "k3_001"), "class512/k3_001": lambda: class_case(512, "k3_001"),
    "mixed": mixed_case, "split": split_case,
}


def case_inputs(name):
    return (LIVE.get(name) or RECORDED[name])()


def checked(name, r):
    """the conditions every reference has to meet before a test may use it"""
    assert r is not None, (name, "a sample has no member taking part")
    assert r["ended_by_step"], (name, "an EM ended at MAX_PASSES")
    assert r["w_between"] <= W_REF_MAX and r["w_within"] <= W_REF_MAX, (name, r["w_between"], r["w_within"])
    return r


def live_reference(name):
    if ("live", name) not in _cache:
        prob, Rs, dens, members, groups, sizes = case_inputs(name)
        _cache[("live", name)] = checked(name, reference(prob, Rs, dens, members, groups, sizes))
    return _cache[("live", name)]


def record(path=GOLDEN, names=None):
    """compute the recorded cases (all, or `names`, kept next to what the file holds) and write the JSON"""
    out = {}
    if names and os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    for name in names or RECORDED:
        prob, Rs, dens, members, groups, sizes = case_inputs(name)
        r = reference(prob, Rs, dens, members, groups, sizes)
        print(name, None if r is None else ("between", r["lam_between"], "within", r["lam_within"], "w", r["w_between"], r["w_within"]), flush=True)
        out[name] = checked(name, r)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def recorded():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


if __name__ == "__main__":
    import sys
    record(names=sys.argv[1:] or None)
