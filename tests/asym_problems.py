"""Builders and a pure-Python restatement for the asymptotic standard errors (include/emsar_hip.h "asymptotic standard errors").

A problem is a dict: n_tx, row_ptr, col_idx, weight, theta (and whatever the caller adds).  component(n) makes the rows of one
connected component of exactly n active transcripts: a chain {t_i, t_i+1}, one single-tid row with reads per transcript, a few 3- and
4-tid rows and one row with a repeated tid; weights 1 .. 40, theta uniform in [0.1, 50]."""
import math

import numpy as np

STATUS = ("ESTIMATED", "BOUNDARY", "UNIDENTIFIABLE", "TOO_LARGE", "INFEASIBLE")
EST, BND, UNI, BIG, INF = range(5)


def component(n, rng, long_walk=0):
    """rows (lists of local tids), weights and theta of one connected component of n transcripts; long_walk: transcript 0 gets that
    many more rows (pairs with a neighbour and single-tid rows)"""
    rows = [[i, i + 1] for i in range(n - 1)] + [[i] for i in range(n)]
    for k in (3, 4):
        if n >= k:
            for _ in range(max(1, n // 8)):
                rows.append(list(rng.choice(n, size=k, replace=False)))
    rows.append([0, 0, 1] if n >= 2 else [0, 0])
    for r in range(long_walk):
        rows.append([0, 1 + r % (n - 1)] if (n > 1 and r % 2) else [0])
    w = rng.integers(1, 41, size=len(rows))
    theta = rng.uniform(0.1, 50.0, size=n)
    return rows, w, theta


def assemble(parts, rng=None, shuffle_tids=False):
    """parts: (rows, weights, theta) per component, each with local tids -> one problem; with rng the components' rows are merged at
    random (each component's own rows stay in order, so its sums do not depend on its neighbours), with shuffle_tids the transcripts
    are numbered at random too.  comp_tids[k] = the tids of part k, ascending."""
    n_tx = sum(len(p[2]) for p in parts)
    new = np.arange(n_tx)
    if shuffle_tids:
        new = rng.permutation(n_tx)
    rows, w, theta, comp_tids, base = [], [], np.zeros(n_tx), [], 0
    for prow, pw, pth in parts:
        ids = new[base:base + len(pth)]
        theta[ids] = pth
        comp_tids.append(np.sort(ids))
        rows += [[int(ids[t]) for t in r] for r in prow]
        w += [int(x) for x in pw]
        base += len(pth)
    if rng is not None:                      # a random merge: every component keeps the order of its own rows
        first = np.cumsum([0] + [len(p[0]) for p in parts])
        nxt = list(first[:-1])
        order = []
        for k in rng.permutation(np.repeat(np.arange(len(parts)), np.diff(first))):
            order.append(nxt[k])
            nxt[k] += 1
        rows, w = [rows[i] for i in order], [w[i] for i in order]
    return from_rows(n_tx, rows, w, theta, comp_tids=comp_tids)


def from_rows(n_tx, rows, weight, theta, **extra):
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([t for r in rows for t in r], dtype=np.int32)
    d = dict(n_tx=int(n_tx), row_ptr=rp, col_idx=col, weight=np.array(weight, dtype=np.int32), theta=np.array(theta, dtype=np.float64))
    d.update(extra)
    return d


def single(n, seed, **kw):
    rng = np.random.default_rng(seed)
    return assemble([component(n, rng, **kw)], rng)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- the definition, operation by operation, in Python floats (IEEE doubles, no fused multiply-add) --------------------------------

def _chunked(x):
    total = 0.0
    for b in range(0, len(x), 256):
        s = x[b]
        for v in x[b + 1:b + 256]:
            s = s + v
        total = s if b == 0 else total + s
    return total


def _max0(x):
    return x if x > 0.0 else 0.0


def _sqrt(x):
    return math.nan if (x != x or x < 0.0) else math.inf if x == math.inf else math.sqrt(x)


def restate(p, E=None, boundary_cut=None, pivot_tol=0.0, gene_of_tx=None, n_genes=0):
    n_tx, rp, col = p["n_tx"], [int(x) for x in p["row_ptr"]], [int(x) for x in p["col_idx"]]
    theta = [float(x) for x in p["theta"]]
    cut = 5e-7 if boundary_cut is None else boundary_cut
    tol = 1e-10 if pivot_tol <= 0 else pivot_tol
    n_rows = len(rp) - 1
    R = [float(x) for x in p["weight"]]
    if E is not None:
        R = [0.0 if E[c] == 0.0 else R[c] for c in range(n_rows)]
    active = [theta[t] > cut for t in range(n_tx)]
    w, rows_infeasible, adj, bad = [], 0, {t: set() for t in range(n_tx) if active[t]}, set()
    for c in range(n_rows):
        ts = col[rp[c]:rp[c + 1]]
        S = 0.0
        for t in ts:
            S = S + theta[t]
        wc = R[c] / (S * S) if (R[c] > 0 and S > 0) else 0.0
        w.append(wc)
        infeasible = bool(ts) and R[c] > 0 and S == 0
        rows_infeasible += infeasible
        if wc != 0 or infeasible:
            act = [t for t in ts if active[t]]
            for t in act:
                adj[t].update(act)
            if infeasible:
                bad.update(act)
    entries = {t: [] for t in adj}                       # (row, position), row ascending then position ascending
    for c in range(n_rows):
        for pos in range(rp[c], rp[c + 1]):
            if col[pos] in entries:
                entries[col[pos]].append((c, pos))
    out = dict(var=[0.0] * n_tx, rowsum=[0.0] * n_tx, genesum=[0.0] * n_tx, partner=[-1] * n_tx, partner_cov=[math.nan] * n_tx,
               status=[BND] * n_tx, blocker=[-1] * n_tx, blocks={})
    seen, min_ratio, comps = set(), math.inf, 0
    for t0 in range(n_tx):
        if not active[t0] or t0 in seen:
            continue
        comp, todo = {t0}, [t0]
        while todo:
            for u in adj[todo.pop()]:
                if u not in comp:
                    comp.add(u)
                    todo.append(u)
        seen |= comp
        comps += 1
        tids = sorted(comp)
        n = len(tids)
        if n > 192 or comp & bad:
            for t in tids:
                out["status"][t] = BIG if n > 192 else INF
                out["var"][t] = out["rowsum"][t] = math.nan
            continue
        J = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1):
                acc = 0.0
                for c, _ in entries[tids[i]]:
                    for pos in range(rp[c], rp[c + 1]):
                        if col[pos] == tids[j]:
                            acc = acc + w[c]
                J[i][j] = acc
        L, D, fail = [[0.0] * n for _ in range(n)], [0.0] * n, -1
        for j in range(n):
            for i in range(j, n):
                acc = J[i][j]
                for k in range(j):
                    acc = acc - (L[i][k] * D[k]) * L[j][k]
                if i == j:
                    D[j] = acc
                    ratio = acc / J[j][j] if J[j][j] != 0 else math.nan
                    if ratio < min_ratio:
                        min_ratio = ratio
                    if not (math.isfinite(acc) and acc > tol * J[j][j]):
                        fail = j
                        break
                else:
                    L[i][j] = acc / D[j]
            if fail >= 0:
                break
        if fail >= 0:
            for t in tids:
                out["status"][t], out["var"][t], out["rowsum"][t], out["blocker"][t] = UNI, math.inf, math.inf, tids[fail]
            continue
        M = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
        for i in range(n):
            for j in range(i):
                acc = L[i][j]
                for k in range(j + 1, i):
                    acc = acc + L[i][k] * M[k][j]
                M[i][j] = -acc
        Sg = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for j in range(n):
                k0 = max(i, j)
                acc = (M[k0][i] * M[k0][j]) / D[k0]
                for k in range(k0 + 1, n):
                    acc = acc + (M[k][i] * M[k][j]) / D[k]
                Sg[i][j] = acc
        out["blocks"][tids[0]] = (tids, Sg)
        for i, t in enumerate(tids):
            out["status"][t] = EST
            out["var"][t] = Sg[i][i]
            rs = Sg[i][0]
            for j in range(1, n):
                rs = rs + Sg[i][j]
            out["rowsum"][t] = rs
            if gene_of_tx is not None and gene_of_tx[t] >= 0:
                gs = None
                for j in range(n):
                    if gene_of_tx[tids[j]] == gene_of_tx[t]:
                        gs = Sg[i][j] if gs is None else gs + Sg[i][j]
                out["genesum"][t] = gs
            best = None
            for j in range(n):
                if j != i:
                    v = Sg[i][j] * abs(Sg[i][j]) / Sg[j][j]
                    if best is None or v < best:
                        best, out["partner"][t], out["partner_cov"][t] = v, tids[j], Sg[i][j]
    # the host finish
    st = out["status"]
    S = _chunked(theta) if n_tx else 0.0
    VS = _chunked([out["rowsum"][t] if st[t] == EST else 0.0 for t in range(n_tx)]) if n_tx else 0.0
    lost = _chunked([theta[t] if st[t] not in (EST, BND) else 0.0 for t in range(n_tx)]) if n_tx else 0.0
    out["sd_fpkm"] = [_sqrt(v) for v in out["var"]]
    by_status = lambda s, v: math.inf if s == UNI else math.nan if s in (BIG, INF) else v
    out["sd_tpm"] = []
    for t in range(n_tx):
        if S == 0:
            out["sd_tpm"].append(0.0)
        elif st[t] not in (EST, BND):
            out["sd_tpm"].append(by_status(st[t], 0.0))
        else:
            a = theta[t] / S
            out["sd_tpm"].append(_sqrt((1e6 / S) * (1e6 / S) * _max0(out["var"][t] - 2 * a * out["rowsum"][t] + a * a * VS)))
    out["stats"] = dict(rows_infeasible=rows_infeasible, min_pivot_ratio=min_ratio, components=comps,
                        theta_unestimated_share=0.0 if S == 0 else lost / S)
    if gene_of_tx is not None:
        members = [[t for t in range(n_tx) if gene_of_tx[t] == g] for g in range(n_genes)]
        rank = {BND: 0, EST: 1, UNI: 2, INF: 3, BIG: 4}
        gst = [max([BND] + [st[t] for t in m], key=lambda s: rank[s]) for m in members]
        VG = [_chunked([out["genesum"][t] for t in m]) if m else 0.0 for m in members]
        G = [_chunked([theta[t] for t in m]) if m else 0.0 for m in members]
        out["gene_status"] = gst
        out["gene_sd"] = [by_status(gst[g], _sqrt(VG[g])) for g in range(n_genes)]
        out["usage_sd"] = []
        for t in range(n_tx):
            g = gene_of_tx[t]
            if g < 0:
                out["usage_sd"].append(math.nan)
            elif G[g] == 0:
                out["usage_sd"].append(0.0)
            elif gst[g] not in (EST, BND):
                out["usage_sd"].append(by_status(gst[g], 0.0))
            else:
                u = theta[t] / G[g]
                out["usage_sd"].append(_sqrt(_max0(out["var"][t] - 2 * u * out["genesum"][t] + u * u * VG[g])) / G[g])
    return out


TX_KEYS = ("var", "sd_fpkm", "sd_tpm", "rowsum", "partner_cov", "status", "partner", "blocker")
GENE_KEYS = ("usage_sd", "gene_sd", "gene_status")


def assert_equals_restatement(got, want, genes=False):
    for k in TX_KEYS + (GENE_KEYS if genes else ()):
        w = np.array(want[k], dtype=got[k].dtype)
        assert same_bits(got[k], w), (k, got[k], w)


def assert_same_result(a, b, keys=None):
    """two results of the library, bit for bit (NaNs by position and payload)"""
    for k in (keys or [k for k in a if k != "stats"]):
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), k
