"""Two samples over one structure for the two-sample test (include/emsar_hip.h "two-sample test"), and its independent reference in
numpy, shared by test_compare_cpu.py and test_compare_gpu.py.

Structures come from tests/set_problems.py (edge_problem, family, compose); a sample is a weight vector over the structure's rows.
Weights are drawn so that the plain EM of the reference reaches a relative step of 1e-13 quickly: R_c = round(K E_c S_c(theta*)) for
a positive theta* per sample (data the model fits almost exactly: an interior optimum near K theta*), with the tested transcripts'
theta* set apart between the samples.  Nothing the device computes entered any choice here.

The reference knows nothing of multipliers: F1 is two plain EMs, F0 one plain EM on the stacked problem (A's rows and B's rows, every
transcript but t once per sample, t as ONE column whose entries in B's rows are 1 / r and whose den is den_tA + den_tB / r)."""
import numpy as np

from tests import set_problems as SP

REL_STEP = 1e-13
MAX_PASSES = 200000


def den_of(prob):
    """den_t = sum of E over the rows that hold t (a row with E = 0 adds nothing), as upload_sample computes it"""
    n_tx, rp, ci, _, E = prob
    rowid = np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))
    return np.bincount(ci, weights=E[rowid], minlength=n_tx)


def component(prob, R, t):
    """the connected set of t in the sample R: (tids ascending, rows ascending) over the rows with R > 0 and E > 0; rows of t alone included"""
    n_tx, rp, ci, _, E = prob
    rp = rp.astype(np.int64)
    live = np.flatnonzero((R > 0) & (E > 0))
    parent = np.arange(n_tx)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for c in live:
        r0 = find(ci[rp[c]])
        for k in range(rp[c] + 1, rp[c + 1]):
            parent[find(ci[k])] = r0
    root = find(t)
    rows = np.array([c for c in live if find(ci[rp[c]]) == root], dtype=np.int64)
    tids = np.array(sorted({int(x) for c in rows for x in ci[rp[c]:rp[c + 1]]} | {int(t)}), dtype=np.int64)
    return tids, rows


class Block:
    """the rows of one sample's component as index arrays over local columns"""

    def __init__(self, prob, R, tids, rows):
        _, rp, ci, _, _ = prob
        rp = rp.astype(np.int64)
        local = {int(g): i for i, g in enumerate(tids)}
        self.n_r = len(rows)
        self.rowid = np.concatenate([np.full(rp[c + 1] - rp[c], j, dtype=np.int64) for j, c in enumerate(rows)]) if len(rows) else np.zeros(0, dtype=np.int64)
        self.col = np.array([local[int(x)] for c in rows for x in ci[rp[c]:rp[c + 1]]], dtype=np.int64)
        self.R = R[rows].astype(np.float64)


def em(n, blocks, den, rel_step=REL_STEP, max_passes=MAX_PASSES):
    """Plain EM of sum_c R_c log S_c - sum_j x_j den_j, S = M x, from x = 1 (0 where den = 0) to a relative step of rel_step (floor 1e-6,
    the solver's abs_floor).  blocks: (Block, column map local -> 0 .. n-1, per-entry coefficient).  Returns (x, F, passes)."""
    x = np.where(den > 0, 1.0, 0.0)
    safe = np.where(den > 0, den, 1.0)
    ent = [(b, cmap[b.col], coef) for b, cmap, coef in blocks]
    passes = 0
    while True:
        acc = np.zeros(n)
        for b, col, coef in ent:
            S = np.bincount(b.rowid, weights=x[col] * coef, minlength=b.n_r)
            w = np.where(S > 0, b.R / np.where(S > 0, S, 1.0), 0.0)
            acc += np.bincount(col, weights=w[b.rowid] * coef, minlength=n)
        y = np.where(den > 0, x * acc / safe, 0.0)
        passes += 1
        step = np.max(np.abs(y - x) / (np.abs(y) + 1e-6)) if n else 0.0
        x = y
        if step < rel_step or passes >= max_passes:
            break
    F = -float(np.dot(x, den))
    for b, col, coef in ent:
        S = np.bincount(b.rowid, weights=x[col] * coef, minlength=b.n_r)
        ok = S > 0
        F += float(np.sum(b.R[ok] * np.log(S[ok])))
    return x, F, passes


def sample_fit(prob, R, t, den=None):
    """the free fit of t's component in one sample -> dict(tids, rows, x, F, passes, theta_t)"""
    den = den_of(prob) if den is None else den
    tids, rows = component(prob, R, t)
    blk = Block(prob, R, tids, rows)
    ident = np.arange(len(tids))
    x, F, passes = em(len(tids), [(blk, ident, 1.0)], den[tids])
    return dict(tids=tids, rows=rows, block=blk, x=x, F=F, passes=passes, theta_t=float(x[np.searchsorted(tids, t)]))


def reference(prob, RA, RB, t, ratio=1.0, den_a=None, den_b=None):
    """Lambda_t of the two-sample test and what went into it -> dict(lam, F1, F0, theta_a, theta_b, theta_null, passes)"""
    den_a = den_of(prob) if den_a is None else den_a
    den_b = den_of(prob) if den_b is None else den_b
    a, b = sample_fit(prob, RA, t, den_a), sample_fit(prob, RB, t, den_b)
    nA, nB = len(a["tids"]), len(b["tids"])
    ta, tb = int(np.searchsorted(a["tids"], t)), int(np.searchsorted(b["tids"], t))
    # stacked columns: A's transcripts 0 .. nA-1 (t among them), then B's without t
    map_b = np.arange(nB) + nA
    map_b[tb] = ta
    map_b[tb + 1:] -= 1
    n = nA + nB - 1
    den = np.zeros(n)
    den[:nA] = den_a[a["tids"]]
    den[map_b] = den_b[b["tids"]]
    den[ta] = den_a[t] + den_b[t] / ratio
    coef_b = np.where(b["block"].col == tb, 1.0 / ratio, 1.0)
    x, F0, passes = em(n, [(a["block"], np.arange(nA), 1.0), (b["block"], map_b, coef_b)], den)
    F1 = a["F"] + b["F"]
    return dict(lam=2.0 * (F1 - F0), F1=F1, F0=F0, FA=a["F"], FB=b["F"], theta_a=a["theta_t"], theta_b=b["theta_t"], theta_null=float(x[ta]),
                passes=(a["passes"], b["passes"], passes), n=(nA, nB))


def fitted_weights(prob, seed, scale=30.0, apart=(), factor=1.6):
    """R_c = round(scale E_c S_c(theta*)), theta* uniform in [1, 3], multiplied by `factor` for the transcripts in `apart`; rows with E = 0
    keep the structure's own weight (they are outside the likelihood)"""
    n_tx, rp, ci, R, E = prob
    rng = np.random.default_rng(seed)
    th = rng.uniform(1.0, 3.0, size=n_tx)
    th[list(apart)] *= factor
    rowid = np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))
    S = np.bincount(rowid, weights=th[ci], minlength=len(rp) - 1)
    out = np.maximum(np.rint(scale * E * S), 1).astype(np.int32)
    return np.where(E > 0, out, R).astype(np.int32)


# ---- the problems ---------------------------------------------------------------------------------------------------------------
_cache = {}

# EDGES index of the shape used per class: one inside the 64 class, the upper edges of the 256 and the 512 class
CLASS_EDGE = {64: 0, 256: 4, 512: 8}


def class_problem(threads):
    """(prob, RA, RB, tids to test): the edge set of the class under two fitted samples; the tested transcripts' theta* lie apart"""
    key = ("class", threads)
    if key not in _cache:
        k = CLASS_EDGE[threads]
        n_tx, rp, ci, R, E, members = SP.compose_members([SP.edge_set(*SP.EDGES[k][0], seed=SP.SEEDS[k])], seed=200 + k)
        prob = (n_tx, rp, ci, R, E)
        tids = [int(members[0][0][i]) for i in (0, 7)]
        RA = fitted_weights(prob, 1000 + threads)
        RB = fitted_weights(prob, 2000 + threads, apart=tids)
        _cache[key] = (prob, RA, RB, tids)
    return _cache[key]


def split_problem():
    """The 512-class edge set whose sample A has reads on the first ten chain rows only: the component of local transcript 0 is an
    11-transcript chain in A (64 class) and the whole set in B (512 class).  -> (prob, RA, RB, [tid of local 0, tid of local 5])"""
    if "split" not in _cache:
        k = CLASS_EDGE[512]
        n_tx, rp, ci, R, E, members = SP.compose_members([SP.edge_set(*SP.EDGES[k][0], seed=SP.SEEDS[k])], seed=200 + k)
        prob = (n_tx, rp, ci, R, E)
        loc = members[0][0]
        rp64 = rp.astype(np.int64)
        chain = {frozenset((int(loc[i]), int(loc[i + 1]))) for i in range(10)}
        keep = np.array([E[c] > 0 and frozenset(int(x) for x in ci[rp64[c]:rp64[c + 1]]) in chain for c in range(len(rp) - 1)])
        tids = [int(loc[0]), int(loc[5])]
        RB = fitted_weights(prob, 2512, apart=tids)
        RA = np.where(keep, fitted_weights(prob, 1512), 0).astype(np.int32)
        _cache["split"] = (prob, RA, RB, tids)
    return _cache["split"]


def csr(rows, n_tx):
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return n_tx, rp, np.concatenate([np.array(r, dtype=np.int32) for r in rows]).astype(np.int32)


def small_problem():
    """Hand-made: transcripts 0, 1 alone in their rows in both samples (closed form both); 2 closed form in A (its linking row {2, 3} has
    no reads there) and in a set in B; 3, 4, 5 a family in both; 6 with theta_hat = 0 in B (its only reads there go to 7 by the row
    {7} alone) and 30 reads of its own in A; 8 and 9 share one row that has no reads in either sample and no row of their own: absent in
    both; 10 has den = 0 in B.  E = 1 everywhere.  -> (prob, RA, RB, den_a, den_b)"""
    rows = [[0], [1], [2], [2, 3], [3], [3, 4], [4, 5], [3, 4, 5], [5], [6], [6, 7], [7], [8, 9], [10], [10, 4]]
    n_tx, rp, ci = csr(rows, 11)
    RA = np.array([40, 25, 33, 0, 12, 20, 9, 14, 6, 30, 25, 11, 0, 5, 3], dtype=np.int32)
    RB = np.array([55, 25, 18, 9, 10, 31, 4, 22, 7, 0, 0, 17, 0, 4, 2], dtype=np.int32)
    E = np.ones(len(rows))
    prob = (n_tx, rp, ci, RA, E)
    den_a = den_of(prob)
    den_b = den_a.copy()
    den_b[10] = 0.0
    return prob, RA, RB, den_a, den_b


def closed_pair_lambda(u_a, d_a, u_b, d_b, ratio=1.0):
    """two one-transcript components: the null MLE is x = (u_A + u_B) / (d_A + r d_B)... on the A scale with B's value x / r:
    maximise u_A log x - x d_A + u_B log(x / r) - (x / r) d_B  ->  x = (u_A + u_B) / (d_A + d_B / r)"""
    F = lambda u, x, d: (u * np.log(x) if u > 0 else 0.0) - x * d
    xa, xb = u_a / d_a, u_b / d_b
    x = (u_a + u_b) / (d_a + d_b / ratio)
    return 2.0 * (F(u_a, xa, d_a) + F(u_b, xb, d_b) - F(u_a, x, d_a) - F(u_b, x / ratio, d_b)), x


if __name__ == "__main__":
    import time
    for th in (64, 256, 512):
        prob, RA, RB, tids = class_problem(th)
        for t in tids:
            t0 = time.time()
            r = reference(prob, RA, RB, t)
            print(th, t, "Lambda", r["lam"], "theta", r["theta_a"], r["theta_b"], r["theta_null"], "passes", r["passes"], "n", r["n"], "%.2f s" % (time.time() - t0))
    prob, RA, RB, tids = split_problem()
    for t in tids:
        t0 = time.time()
        r = reference(prob, RA, RB, t)
        print("split", t, "Lambda", r["lam"], "theta", r["theta_a"], r["theta_b"], "passes", r["passes"], "n", r["n"], "%.2f s" % (time.time() - t0))
