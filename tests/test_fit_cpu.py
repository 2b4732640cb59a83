"""CPU: the model fit's host function (emsar_hip_model_fit_host) against a plain numpy restatement of include/emsar_hip.h "model fit" --
bit for bit except the deviance, which goes through log -- on a staircase of chunk sizes, its properties, a planted misfit, and the
errors.  No GPU: tests/test_fit_gpu.py compares the device with this host function on the same problems."""
import ctypes as C

import numpy as np
import pytest

from emsar_amd import hip
from tests.test_genes_gpu import chunked_sums, family_problem

CHUNK = 256
STAIRS = [1, 255, 256, 257, 512, 513, 64 * 256, 64 * 256 + 1]      # entries owned by transcripts 0 .. 7
EPS = 2.0 ** -52


# ---- the definition in numpy ------------------------------------------------------------------------------------------------------

def np_rows(rp, ci, R, E, theta):
    """per row: S (left to right), mu, q, d, a, the flags inside / infeasible, and L = R |log(R / mu)| (0 where it is not taken)"""
    rp = np.asarray(rp).astype(np.int64)
    n_rows = len(rp) - 1
    lens = np.diff(rp)
    R = np.ones(n_rows) if R is None else np.asarray(R, dtype=np.float64)
    E = np.ones(n_rows) if E is None else np.asarray(E, dtype=np.float64)
    S = np.zeros(n_rows)
    for j in range(int(lens.max()) if n_rows else 0):                 # position by position: every row is added left to right
        m = lens > j
        S[m] = S[m] + theta[ci[rp[:-1][m] + j]]
    inside = (lens > 0) & (E != 0.0)
    S = np.where(inside, S, 0.0)
    mu = np.where(inside, E * S, 0.0)
    pos = inside & (mu > 0)
    with np.errstate(all="ignore"):
        diff = R - mu
        q = np.where(pos, diff * diff / mu, 0.0)
        a = np.where(pos, np.abs(diff), 0.0)
        lg = np.where(pos & (R > 0), np.log(R / mu), 0.0)
        l = np.where(pos & (R > 0), R * lg, 0.0)
        d = 2.0 * (l - diff)
        d = np.where(pos, np.where(d < 0, 0.0, d), 0.0)
    bad = inside & (mu == 0) & (R > 0)
    q[bad], d[bad], a[bad] = np.inf, np.inf, R[bad]
    return dict(S=S, mu=mu, q=q, d=d, a=a, inside=inside, pos=pos, bad=bad, L=np.abs(l))


def seq_chunked(x):
    """chunks of 256 left to right, then the chunk sums left to right (np.cumsum adds sequentially)"""
    if len(x) == 0:
        return 0.0
    parts = np.array([x[c:c + CHUNK].cumsum()[-1] for c in range(0, len(x), CHUNK)])
    return parts.cumsum()[-1]


def np_fit(n_tx, rp, ci, R, E, theta, gene_of_tx=None, n_genes=0):
    """the whole definition: rows, transcripts (entries by row then position), genes.  tx_dev_scale = sum p (2 L + d), the scale of
    the deviance's tolerance."""
    rp64 = np.asarray(rp).astype(np.int64)
    ci = np.asarray(ci)
    theta = np.asarray(theta, dtype=np.float64)
    r = np_rows(rp64, ci, R, E, theta)
    row_of = np.repeat(np.arange(len(rp64) - 1), np.diff(rp64))
    order = np.argsort(ci, kind="stable")                               # by transcript; CSR order (row, position) inside
    start = np.searchsorted(ci[order], np.arange(n_tx + 1))
    Srec = np.where(r["pos"], r["S"], 0.0)
    out = {k: np.zeros(n_tx) for k in ("tx_chi2", "tx_dev", "tx_miss", "tx_df", "tx_dev_scale")}
    out["tx_worst_row"] = np.full(n_tx, -1, dtype=np.int32)
    for t in range(n_tx):
        rows = row_of[order[start[t]:start[t + 1]]]
        s = Srec[rows]
        ok = s > 0
        with np.errstate(all="ignore"):
            p = np.where(ok, theta[t] / np.where(ok, s, 1.0), 0.0)
            tq, td, ta = (np.where(ok, p * r[k][rows], 0.0) for k in ("q", "d", "a"))
            scale = np.where(ok, p * (2.0 * r["L"][rows] + r["d"][rows]), 0.0)
        out["tx_chi2"][t], out["tx_dev"][t], out["tx_miss"][t], out["tx_df"][t] = seq_chunked(tq), seq_chunked(td), seq_chunked(ta), seq_chunked(p)
        out["tx_dev_scale"][t] = scale.sum()
        if len(ta) and ta.max() > 0:
            out["tx_worst_row"][t] = rows[int(np.argmax(ta))]           # the first maximum: rows ascend
    out.update(row_mu=r["mu"], row_chi2=r["q"], row_dev=r["d"], rows=r)
    if gene_of_tx is not None:
        g = np.asarray(gene_of_tx)
        for k in ("chi2", "dev", "miss", "df"):
            out["gene_" + k] = chunked_sums(out["tx_" + k], g, n_genes)[0]
        out["gene_dev_scale"] = np.bincount(g[g >= 0], weights=out["tx_dev_scale"][g >= 0], minlength=n_genes)
    return out


def assert_fit_equal(got, want, what="", rows=True, genes=False):
    """bit for bit except dev; dev to the tolerances of the log's last place"""
    keys = ["tx_chi2", "tx_miss", "tx_df", "tx_worst_row"] + (["row_mu", "row_chi2"] if rows else []) + (
        ["gene_chi2", "gene_miss", "gene_df"] if genes else [])
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:5])
    if rows:
        r = want["rows"]
        fin = np.isfinite(want["row_dev"])
        assert np.array_equal(np.isinf(got["row_dev"]), ~fin), what
        err = np.abs(got["row_dev"][fin] - want["row_dev"][fin])
        tol = EPS * (8.0 * r["L"][fin] + 2.0 * want["row_dev"][fin])
        print("%s row dev: max error %.3g, max error / tolerance %.3g" % (what, err.max(initial=0.0), (err / np.maximum(tol, 1e-300)).max(initial=0.0)))
        assert np.all(err <= tol), (what, "row_dev", err.max())
    for k, sc in [("tx_dev", "tx_dev_scale")] + ([("gene_dev", "gene_dev_scale")] if genes else []):
        # (a share of a row whose mu is denormal can overflow: +inf on both sides is agreement)
        err = np.where(got[k] == want[k], 0.0, np.abs(got[k] - np.where(np.isinf(want[k]), 0.0, want[k])))
        print("%s %s: max error %.3g, max error / scale %.3g" % (what, k, err.max(initial=0.0), (err / np.maximum(want[sc], 1e-300)).max(initial=0.0)))
        assert np.all(err <= 1e-12 * want[sc]), (what, k)


# ---- problems ---------------------------------------------------------------------------------------------------------------------

def staircase_problem(seed=11):
    """Transcripts 0 .. 7 own exactly 1, 255, 256, 257, 512, 513, 16 384 and 16 385 entries: rows {t, filler} with a few {t, t, filler},
    shuffled, among empty rows, rows with E = 0 and rows with R = 0.  Theta lognormal with 20 % zeros."""
    rng = np.random.default_rng(seed)
    n_fill = 300
    n_tx = len(STAIRS) + n_fill
    rows = []
    for t, n in enumerate(STAIRS):
        left = n
        while left > 0:
            k = 2 if (left >= 2 and rng.random() < 0.02) else 1
            f = len(STAIRS) + int(rng.integers(n_fill))
            rows.append([t] * k + [f] if rng.random() < 0.7 else [f] + [t] * k)
            left -= k
    rows += [[] for _ in range(200)]
    rows += [[len(STAIRS) + int(rng.integers(n_fill))] for _ in range(100)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([x for r in rows for x in r], dtype=np.int32)
    assert np.array_equal(np.bincount(ci, minlength=n_tx)[:len(STAIRS)], STAIRS)
    R = rng.integers(0, 40, size=len(rows)).astype(np.int32)
    R[rng.random(len(rows)) < 0.1] = 0
    E = rng.uniform(0.5, 2.0, size=len(rows))
    E[rng.random(len(rows)) < 0.05] = 0.0
    theta = rng.lognormal(0.0, 2.0, size=n_tx) * (rng.random(n_tx) >= 0.2)
    theta[6], theta[7] = 3.0, 0.25                                  # the two long ones carry something
    gene_of_tx = np.concatenate([np.arange(len(STAIRS)), len(STAIRS) + np.arange(n_fill) // 7]).astype(np.int32)
    return dict(n_tx=n_tx, rp=rp, ci=ci, R=R, E=E, theta=theta, gene_of_tx=gene_of_tx, n_genes=int(gene_of_tx.max()) + 1)


_memo = {}


def staircase_reference():
    """the staircase problem with numpy's answer, computed once and shared (tests/test_fit_gpu.py reads it too)"""
    if "stair" not in _memo:
        p = staircase_problem()
        _memo["stair"] = (p, np_fit(p["n_tx"], p["rp"], p["ci"], p["R"], p["E"], p["theta"], p["gene_of_tx"], p["n_genes"]))
    return _memo["stair"]


def host_fit(p, theta=None, R="own", E="own", rows=True, genes=True):
    return hip.model_fit_host(p["n_tx"], p["rp"], p["ci"], p["theta"] if theta is None else theta, row_weight=p["R"] if isinstance(R, str) else R,
                              E=p["E"] if isinstance(E, str) else E, rows=rows, gene_of_tx=p["gene_of_tx"] if genes else None,
                              n_genes=p["n_genes"] if genes else 0)


def family_fit_problem():
    """family_problem (4620 transcripts, 13 860 rows, a gene of 1100 transcripts) with the oracle's CPU EM solve as theta"""
    if "family" not in _memo:
        m, gmap, ng = family_problem()
        theta, _ = m.em_solve(max_iter=3000, tol=1e-6)       # a second of CPU: F is within 1e-9 of the converged one, and nothing is refitted
        _memo["family"] = dict(n_tx=m.n_tx, rp=m.row_ptr, ci=m.col_idx, R=m.R, E=m.E, theta=np.asarray(theta), gene_of_tx=gmap, n_genes=ng, model=m)
    return _memo["family"]


# ---- against numpy ----------------------------------------------------------------------------------------------------------------

def test_staircase_against_numpy():
    p, want = staircase_reference()
    got = host_fit(p)
    assert want["rows"]["bad"].sum() > 0 and (~want["rows"]["inside"]).sum() > 200      # infeasible rows, outside rows
    assert (want["rows"]["inside"] & (np.asarray(p["R"]) == 0)).sum() > 1000
    assert_fit_equal(got, want, "staircase", genes=True)
    st = got["stats"]
    nnz = len(p["ci"])
    assert nnz <= st.index_slots <= nnz + 64 * 255                                     # the padding telescopes
    assert st.index_bytes >= 4 * st.index_slots
    assert st.rows_inside == want["rows"]["inside"].sum() and st.rows_infeasible == want["rows"]["bad"].sum()
    # every stair is there: 1, 1, 1, 2, 2, 3, 64 and 65 chunks
    assert np.all(want["tx_df"][[0, 1, 2, 3, 4, 5]] >= 0) and want["tx_df"][6] > 1000 and want["tx_df"][7] > 10


def test_family_against_numpy():
    p = family_fit_problem()
    want = np_fit(p["n_tx"], p["rp"], p["ci"], p["R"], p["E"], p["theta"], p["gene_of_tx"], p["n_genes"])
    got = host_fit(p)
    assert (np.bincount(p["gene_of_tx"][p["gene_of_tx"] >= 0]) >= 1000).any()
    assert_fit_equal(got, want, "family", genes=True)
    # defaults: no weights = 1 per row, no E = 1.0
    want1 = np_fit(p["n_tx"], p["rp"], p["ci"], None, None, p["theta"])
    assert_fit_equal(host_fit(p, R=None, E=None, genes=False), want1, "family, defaults")


# ---- properties -------------------------------------------------------------------------------------------------------------------

def test_exact_fit_gives_zeros():
    p = family_fit_problem()
    theta = np.random.default_rng(2).integers(0, 50, size=p["n_tx"]).astype(np.float64)
    rp = p["rp"].astype(np.int64)
    R = np.add.reduceat(np.append(theta[p["ci"]], 0.0), rp[:-1])[:len(rp) - 1].astype(np.int32)       # integers: exact in any order
    got = host_fit(p, theta=theta, R=R, E=None)
    assert np.array_equal(got["row_mu"], R.astype(np.float64))
    for k in ("row_chi2", "row_dev", "tx_chi2", "tx_dev", "tx_miss", "gene_chi2", "gene_dev", "gene_miss"):
        assert not got[k].any(), k
    assert np.all(got["tx_worst_row"] == -1)
    st = got["stats"]
    assert (st.sum_chi2, st.sum_dev, st.sum_miss, st.rows_infeasible) == (0.0, 0.0, 0.0, 0)


@pytest.mark.parametrize("zeros", [False, True])
def test_shares_of_a_row_sum_to_one(zeros):
    p, _ = staircase_reference()
    theta = p["theta"] if zeros else np.where(p["theta"] > 0, p["theta"], 0.5)
    got = host_fit(p, theta=theta)
    st = got["stats"]
    r = np_rows(p["rp"], p["ci"], p["R"], p["E"], theta)
    # rows whose transcripts are all at zero and that hold no read have nothing to share out; with theta > 0 there are none
    silent = int((r["inside"] & ~r["pos"] & ~r["bad"]).sum())
    assert (silent > 0) == zeros and (st.rows_infeasible > 0) == zeros
    want_df = st.rows_inside - st.rows_infeasible - silent
    assert abs(got["tx_df"].sum() - want_df) <= 1e-9 * want_df
    for k, tot in (("tx_chi2", st.sum_chi2), ("tx_dev", st.sum_dev), ("tx_miss", st.sum_miss)):
        assert np.isfinite(tot) and tot > 0 and abs(got[k].sum() - tot) <= 1e-9 * tot, k
    fin = np.isfinite(got["row_chi2"])
    assert abs(got["row_chi2"][fin].sum() - st.sum_chi2) <= 1e-9 * st.sum_chi2


def test_infeasible_row():
    # row 1 holds reads but both its transcripts are at zero
    rp, ci = np.array([0, 2, 4, 5], dtype=np.uint64), np.array([0, 1, 1, 2, 0], dtype=np.int32)
    got = hip.model_fit_host(3, rp, ci, [2.0, 0.0, 0.0], row_weight=[3, 4, 1], rows=True)
    assert np.isinf(got["row_chi2"][1]) and np.isinf(got["row_dev"][1]) and got["row_mu"][1] == 0.0
    assert np.isfinite(got["row_chi2"][[0, 2]]).all() and np.isfinite(got["row_dev"][[0, 2]]).all()
    for k in ("tx_chi2", "tx_dev", "tx_miss", "tx_df"):
        assert np.isfinite(got[k]).all(), k
    st = got["stats"]
    assert st.rows_infeasible == 1 and st.rows_inside == 3 and np.isfinite([st.sum_chi2, st.sum_dev, st.sum_miss]).all()
    assert got["tx_df"].tolist() == [2.0, 0.0, 0.0] and got["tx_miss"].tolist() == [2.0, 0.0, 0.0] and got["tx_worst_row"].tolist() == [0, -1, -1]
    # no reads there: not infeasible, nothing to report
    got = hip.model_fit_host(3, rp, ci, [2.0, 0.0, 0.0], row_weight=[3, 0, 1], rows=True)
    assert got["stats"].rows_infeasible == 0 and got["row_chi2"][1] == 0.0 and got["row_dev"][1] == 0.0


def test_worst_row_ties_go_to_the_smaller_row():
    # rows 1 and 3 are the same row with the same reads: equal products, the smaller row wins; row 2 misses less
    rp, ci = np.array([0, 0, 2, 4, 6], dtype=np.uint64), np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    got = hip.model_fit_host(2, rp, ci, [1.0, 3.0], row_weight=[9, 10, 5, 10])
    assert got["tx_worst_row"].tolist() == [1, 1]
    got = hip.model_fit_host(2, rp, ci, [1.0, 3.0], row_weight=[9, 5, 10, 10])
    assert got["tx_worst_row"].tolist() == [2, 2]
    # across chunks: 600 equal rows, three chunks
    n = 600
    rp, ci = np.arange(0, 2 * n + 1, 2).astype(np.uint64), np.tile([0, 1], n).astype(np.int32)
    got = hip.model_fit_host(2, rp, ci, [1.0, 3.0], row_weight=np.full(n, 7))
    assert got["tx_worst_row"].tolist() == [0, 0]
    w = np.full(n, 7)
    w[[300, 599]] = 9
    assert hip.model_fit_host(2, rp, ci, [1.0, 3.0], row_weight=w)["tx_worst_row"].tolist() == [300, 300]


def test_one_transcript_gene_gets_its_transcripts_bits():
    p, _ = staircase_reference()
    got = host_fit(p)
    for k in ("chi2", "dev", "miss", "df"):
        assert np.array_equal(got["gene_" + k][:len(STAIRS)], got["tx_" + k][:len(STAIRS)]), k
    assert got["tx_dev"][:len(STAIRS)].max() > 0


# ---- a planted misfit -------------------------------------------------------------------------------------------------------------

def test_planted_misfit_shows_up_on_its_transcript_only():
    p = family_fit_problem()
    rp = p["rp"].astype(np.int64)
    ci, R, theta = p["ci"], np.asarray(p["R"]), p["theta"]
    lens = np.diff(rp)
    first = ci[np.minimum(rp[:-1], len(ci) - 1)]
    single = (lens > 0) & (np.maximum.reduceat(np.append(ci, 0), rp[:-1])[:len(lens)] == first) & (
        np.minimum.reduceat(np.append(ci, np.iinfo(np.int32).max), rp[:-1])[:len(lens)] == first)
    r = np_rows(rp, ci, R, p["E"], theta)
    # a transcript whose single-tid rows all hold at least the reads the model expects: for R >= mu > 0, 5 R - mu > R - mu >= 0, so the
    # row's miss, Pearson term and deviance (increasing in R above mu) all grow strictly wherever R > 0
    pick = -1
    for t in range(p["n_tx"]):
        rows_t = np.nonzero(single & (first == t))[0]
        if len(rows_t) and theta[t] > 0 and r["pos"][rows_t].all() and (R[rows_t] >= r["mu"][rows_t]).all() and (R[rows_t] > 0).any():
            pick = t
            break
    assert pick >= 0
    rows_t = np.nonzero(single & (first == pick))[0]
    R5 = R.copy()
    R5[rows_t] *= 5
    a, b = host_fit(p), host_fit(p, R=R5)
    others = np.arange(p["n_tx"]) != pick
    for k in ("tx_chi2", "tx_dev", "tx_miss", "tx_df", "tx_worst_row"):
        assert np.array_equal(a[k][others], b[k][others]), k
    print("transcript %d, rows %s: miss %.4g -> %.4g, chi2 %.4g -> %.4g, dev %.4g -> %.4g" % (
        pick, rows_t.tolist(), a["tx_miss"][pick], b["tx_miss"][pick], a["tx_chi2"][pick], b["tx_chi2"][pick], a["tx_dev"][pick], b["tx_dev"][pick]))
    for k in ("tx_chi2", "tx_dev", "tx_miss"):
        assert b[k][pick] > a[k][pick], k
    assert a["tx_df"][pick] == b["tx_df"][pick]
    want = np_fit(p["n_tx"], rp, ci, R5, p["E"], theta)
    assert b["tx_worst_row"][pick] == want["tx_worst_row"][pick]
    r5 = want["rows"]
    rows_of_pick = np.repeat(np.arange(len(lens)), lens)[ci == pick]
    pa = theta[pick] / r5["S"][rows_of_pick] * r5["a"][rows_of_pick]
    if rows_of_pick[int(np.argmax(pa))] in rows_t:
        assert b["tx_worst_row"][pick] in rows_t


# ---- errors -----------------------------------------------------------------------------------------------------------------------

def test_host_errors():
    rp, ci = np.array([0, 2, 3], dtype=np.uint64), np.array([0, 1, 1], dtype=np.int32)
    ok = hip.model_fit_host(2, rp, ci, [1.0, 2.0])
    assert ok["tx_df"].tolist() == [1.0 / 3.0, 2.0 / 3.0 + 1.0]

    def status(**kw):
        a = dict(n_tx=2, row_ptr=rp, col_idx=ci, theta=[1.0, 2.0])
        a.update(kw)
        with pytest.raises(hip.EmsarHipError) as e:
            hip.model_fit_host(**a)
        return e.value.status

    assert status(theta=None) == -1
    for bad in (-1.0, np.nan, np.inf):
        assert status(theta=[1.0, bad]) == -1
        assert status(E=[1.0, bad]) == -1
    assert status(row_weight=[1, -1]) == -1
    assert status(row_ptr=np.array([0, 3, 2], dtype=np.uint64)) == -1            # not monotone
    assert status(col_idx=np.array([0, 2, 1], dtype=np.int32)) == -1             # tid outside [0, n_tx)
    assert status(col_idx=np.array([0, -1, 1], dtype=np.int32)) == -1
    assert status(gene_of_tx=[0, 1], n_genes=1) == -1                            # the checks of set_gene_map
    assert status(gene_of_tx=[0, -2], n_genes=1) == -1
    assert status(gene_of_tx=[0, 0], n_genes=0) == -1
    assert status(genes=True) == -5                                              # gene outputs without a map
    # straight at the ABI: no transcripts, a gene output group only partly given, more rows than an int32 row id holds
    L = hip.load_library()
    th = np.array([1.0, 2.0])
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    call = lambda n_rows, n_tx, out: L.emsar_hip_model_fit_host(n_rows, n_tx, rp.ctypes.data_as(C.POINTER(C.c_uint64)), ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                None, None, d(th), 0, None, out, None)
    assert call(2, 2, None) == 0
    assert call(2, 0, None) == -1
    assert call(2 ** 31, 2, None) == -1
    part = hip.FitOutputs()
    buf = np.zeros(4)
    part.gene_chi2 = d(buf)
    assert call(2, 2, C.byref(part)) == -1
