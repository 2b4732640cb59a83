"""K samples over one structure for the K-sample test across replicate groups (include/emsar_hip.h "K-sample test"), and its
independent reference in numpy, shared by test_compare_groups_cpu.py and test_compare_groups_gpu.py.

Structures and the first two samples are those of tests/compare_problems.py (CP); further samples are CP.fitted_weights with new seeds,
the tested transcripts' theta* set apart on the samples of group 1.  Nothing the device computes entered any choice here.

The reference knows nothing of multipliers or of a two-level search.  The free fit F_hat^k is a plain EM (CP.em) on t's component (CP.component).  The
common-value fit C(S) is ONE plain EM on the stacked problem, CP.reference's construction generalised: the blocks of t's component in
every sample of S, every transcript but t once per sample, t as ONE shared column x whose entries in the rows of sample k carry the
coefficient s_k (theta_t^k = s_k x) and whose den is sum_k s_k den_t^k.

Its own error is a bound, not a difference of two runs.  For a problem max sum_c R_c log S_c - sum_j x_j den_j with S = M x and
N = sum_c R_c, every EM iterate has sum_j x_j den_j = N, and there the mixture bound holds:
    F* - F(x) <= N log max_j (acc_j / den_j),   acc_j = sum_c R_c M_cj / S_c
(the objective is concave in the shares p_j = x_j den_j / N, and acc_j / den_j is its gradient over N).  Every fit errs low by at most
its bound, so a Lambda = 2 (a sum of fits - another sum of fits) errs by at most w_ref = 2 x the sum of the bounds of the fits in it.

The class and split cases take minutes in numpy: they are recorded in tests/golden/compare_groups_refs.json by record() (python -m
tests.compare_groups_problems), which refuses a case whose w_ref exceeds 1e-7 or one of whose EMs ended at MAX_PASSES."""
import json
import os

import numpy as np

from tests import compare_problems as CP

REL_STEP = 2e-15                 # the EMs here run further than CP's 1e-13: the mixture bound is about N x the last relative step
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_groups_refs.json")
W_REF_MAX = 1e-7


def mixture_bound(n, blocks, den, x):
    """N log max_j (acc_j / den_j) at x, over the columns with den > 0; blocks as CP.em takes them"""
    acc = np.zeros(n)
    N = 0.0
    for b, cmap, coef in blocks:
        col = cmap[b.col]
        S = np.bincount(b.rowid, weights=x[col] * coef, minlength=b.n_r)
        w = np.where(S > 0, b.R / np.where(S > 0, S, 1.0), 0.0)
        acc += np.bincount(col, weights=w[b.rowid] * coef, minlength=n)
        N += float(b.R.sum())
    live = den > 0
    g = float(np.max(acc[live] / den[live])) if live.any() else 1.0
    return N * float(np.log(max(g, 1.0)))


def free_fit(prob, R, t, den):
    """F_hat of t's component in one sample and its bound -> dict(F, theta_t, bound, passes, fit)"""
    tids, rows = CP.component(prob, R, t)
    blk = CP.Block(prob, R, tids, rows)
    n = len(tids)
    blocks = [(blk, np.arange(n), 1.0)]
    x, F, passes = CP.em(n, blocks, den[tids], rel_step=REL_STEP)
    return dict(F=F, theta_t=float(x[np.searchsorted(tids, t)]), bound=mixture_bound(n, blocks, den[tids], x), passes=passes,
                fit=dict(tids=tids, block=blk))


def common_fit(prob, Rs, dens, sizes, t, S, fits=None):
    """C(S) by one stacked EM -> dict(C, x, bound, passes).  Rs, dens, sizes: per sample; S: sample indices; fits: free_fit per sample"""
    fits = fits or {k: free_fit(prob, Rs[k], t, dens[k]) for k in S}
    n = 1 + sum(len(fits[k]["fit"]["tids"]) - 1 for k in S)
    den = np.zeros(n)
    blocks = []
    off = 1
    for k in S:
        f = fits[k]["fit"]
        nk = len(f["tids"])
        tk = int(np.searchsorted(f["tids"], t))
        cmap = np.arange(nk) + off
        cmap[tk] = 0
        cmap[tk + 1:] -= 1
        others = np.arange(nk) != tk
        den[cmap[others]] = dens[k][f["tids"][others]]
        den[0] += sizes[k] * dens[k][t]
        blocks.append((f["block"], cmap, np.where(f["block"].col == tk, float(sizes[k]), 1.0)))
        off += nk - 1
    x, C, passes = CP.em(n, blocks, den, rel_step=REL_STEP)
    return dict(C=C, x=float(x[0]), bound=mixture_bound(n, blocks, den, x), passes=passes)


def reference(prob, Rs, dens, groups, sizes, t):
    """Both Lambdas of transcript t and what went into them -> dict(lam_between, lam_within, w_between, w_within, theta_common,
    theta_group, theta_hat, F_hat, C_all, C_group, searched, ended_by_step)"""
    K = len(Rs)
    G = max(groups) + 1
    sizes = [1.0] * K if sizes is None else [float(s) for s in sizes]
    fits = {k: free_fit(prob, Rs[k], t, dens[k]) for k in range(K)}
    F_hat = [fits[k]["F"] for k in range(K)]
    theta_hat = [fits[k]["theta_t"] for k in range(K)]
    members = [[k for k in range(K) if groups[k] == g] for g in range(G)]
    al = common_fit(prob, Rs, dens, sizes, t, list(range(K)), fits)
    ended = al["passes"] < CP.MAX_PASSES and all(fits[k]["passes"] < CP.MAX_PASSES for k in range(K))
    C_group, theta_group, b_group, searched = [], [], [], [K]
    for S in members:
        if len(S) == 1:
            C_group.append(F_hat[S[0]]); theta_group.append(theta_hat[S[0]] / sizes[S[0]]); b_group.append(fits[S[0]]["bound"])
        elif len(S) == K:
            C_group.append(al["C"]); theta_group.append(al["x"]); b_group.append(al["bound"])
        else:
            c = common_fit(prob, Rs, dens, sizes, t, S, fits)
            C_group.append(c["C"]); theta_group.append(c["x"]); b_group.append(c["bound"])
            searched.append(len(S))
            ended = ended and c["passes"] < CP.MAX_PASSES
    b_hat = sum(fits[k]["bound"] for k in range(K))
    return dict(lam_between=2.0 * (sum(C_group) - al["C"]), lam_within=2.0 * (sum(F_hat) - sum(C_group)),
                w_between=2.0 * (sum(b_group) + al["bound"]), w_within=2.0 * (b_hat + sum(b_group)),
                theta_common=al["x"], theta_group=theta_group, theta_hat=theta_hat, F_hat=F_hat, C_all=al["C"], C_group=C_group,
                searched=searched, ended_by_step=bool(ended))


# ---- the problems ---------------------------------------------------------------------------------------------------------------
_cache = {}

# per class problem: (name, sample order, groups, sizes).  Samples: A, B = CP.class_problem's (B's theta* apart on the tested
# transcripts), C = a further sample like A, D = a further sample like B
CLASS_CASES = (
    ("k3_001", ("A", "C", "B"), (0, 0, 1), None),
    ("k4_0011", ("A", "C", "B", "D"), (0, 0, 1, 1), (1.0, 1.25, 0.8, 1.0)),
    ("k3_012", ("A", "B", "C"), (0, 1, 2), None),
)


def class_samples(threads):
    """(prob, dict of the four samples by letter, tids)"""
    key = ("class", threads)
    if key not in _cache:
        prob, RA, RB, tids = CP.class_problem(threads)
        _cache[key] = (prob, dict(A=RA, B=RB, C=CP.fitted_weights(prob, 3000 + threads), D=CP.fitted_weights(prob, 4000 + threads, apart=tids)), tids)
    return _cache[key]


def split_samples():
    """CP.split_problem plus one more whole-set sample: t's set lies in the 64 class in A and in the 512 class in B and C.
    -> (prob, samples by letter, tids, sample order, groups)"""
    if "split" not in _cache:
        prob, RA, RB, tids = CP.split_problem()
        _cache["split"] = (prob, dict(A=RA, B=RB, C=CP.fitted_weights(prob, 3512)), tids, ("A", "C", "B"), (0, 0, 1))
    return _cache["split"]


def small_samples():
    """CP.small_problem plus a hand-made third sample -> (prob, [RA, RB, RC], [den_a, den_b, den_c]).  In C transcripts 0 and 1 are closed
    form as in A and B (1 with the reads it has in both: identical in all three); 2 is closed form with no reads at all; 6 has reads of
    its own; 8, 9 stay absent; 10 has den > 0."""
    prob, RA, RB, den_a, den_b = CP.small_problem()
    RC = np.array([48, 25, 0, 0, 11, 26, 6, 18, 5, 12, 8, 14, 0, 6, 2], dtype=np.int32)
    return prob, [RA, RB, RC], [den_a, den_b, den_a.copy()]


def closed_groups(u, den, groups, sizes=None):
    """K one-transcript components: C(S) in closed form, x_S = sum_{k in S} u_k / sum_{k in S} s_k den_k -> dict like reference()'s"""
    u, den = np.asarray(u, dtype=np.float64), np.asarray(den, dtype=np.float64)
    K = len(u)
    s = np.ones(K) if sizes is None else np.asarray(sizes, dtype=np.float64)
    F = lambda uk, th, dk: (uk * np.log(th) if uk > 0 else 0.0) - th * dk
    F_hat = [F(u[k], u[k] / den[k], den[k]) for k in range(K)]

    def C(S):
        x = u[S].sum() / (s[S] * den[S]).sum()
        return sum(F(u[k], s[k] * x, den[k]) for k in S), x
    G = max(groups) + 1
    members = [np.array([k for k in range(K) if groups[k] == g]) for g in range(G)]
    Cg = [C(S) for S in members]
    Ca = C(np.arange(K))
    return dict(lam_between=2.0 * (sum(c for c, _ in Cg) - Ca[0]), lam_within=2.0 * (sum(F_hat) - sum(c for c, _ in Cg)),
                theta_common=Ca[1], theta_group=[x for _, x in Cg], theta_hat=list(u / den))


def case_inputs(name):
    """a recorded case by name ("64/k3_001", "split") -> (prob, [R per sample], groups, sizes, tids)"""
    if name == "split":
        prob, smp, tids, order, groups = split_samples()
        return prob, [smp[c] for c in order], groups, None, tids
    th, case = name.split("/")
    prob, smp, tids = class_samples(int(th))
    _, order, groups, sizes = next(c for c in CLASS_CASES if c[0] == case)
    return prob, [smp[c] for c in order], groups, sizes, tids


CASE_NAMES = tuple("%d/%s" % (th, c[0]) for th in (64, 256, 512) for c in CLASS_CASES) + ("split",)


def record(path=GOLDEN):
    """compute every recorded case and write the JSON; refuses a case that misses the conditions on the inputs"""
    out = {}
    for name in CASE_NAMES:
        prob, Rs, groups, sizes, tids = case_inputs(name)
        den = CP.den_of(prob)
        for t in tids:
            r = reference(prob, Rs, [den] * len(Rs), groups, sizes, t)
            print(name, t, "between", r["lam_between"], "within", r["lam_within"], "w", r["w_between"], r["w_within"], flush=True)
            assert r["ended_by_step"], (name, t, "an EM ended at MAX_PASSES")
            assert r["w_between"] <= W_REF_MAX and r["w_within"] <= W_REF_MAX, (name, t, r["w_between"], r["w_within"])
            out["%s:%d" % (name, t)] = r
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def recorded():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


if __name__ == "__main__":
    record()
