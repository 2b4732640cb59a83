"""GPU: isoform usage (emsar_hip_isoform_usage, emsar_hip_bootstrap_isoforms) -- the point estimate against the host function bit for bit
across layouts and numberings, the bootstrap's usage statistics against the call's own replicates bit for bit, the usage quantiles
against quantiles_host, every other output against bootstrap_genes / bootstrap_quantiles, invariance under batching and numbering, no
side effects on the context, errors, and the CLI's .isoforms file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from emsar_amd import EmsarHip, _build, hip
from tests.conftest import aln_path, get_fixture
from tests.test_bootq_gpu import Q, host_den, same
from tests.test_bootstrap_gpu import CLI, SOLVE, _family, _run_cli
from tests.test_genes_gpu import family_problem, vicugna_genes, welford
from tests.test_isoforms_cpu import lognormal_columns, tie_columns

pytestmark = pytest.mark.gpu
STATS = ("fpkm_mean", "fpkm_sd", "tpm_sd", "replicates", "gene_fpkm_mean", "gene_fpkm_sd", "gene_tpm_sd")
QUANT = ("fpkm_q", "tpm_q", "gene_fpkm_q", "gene_tpm_q", "replicate_sums")
ISO = ("usage_mean", "usage_sd", "dominant_count")


def solve_kw(set_mode):
    """set_mode 1 solves every replicate by streaming passes over the whole matrix, 10^4 or more of them to tol 1e-10 on the family
    problem.  Nothing checked here depends on convergence -- the statistics are compared with the call's own replicates and with other
    calls of the same parameters -- so the streaming replicates stop after 300 passes (deterministic mode: still the same bits)."""
    return SOLVE if set_mode == 0 else dict(max_iter=300, tol=1e-10)


@pytest.fixture(scope="module")
def point_case():
    """family_problem with 5 lognormal columns (20 % zeros) and the tie columns; the host function's answer, computed once"""
    m, gmap, ng = family_problem()
    X = np.vstack([lognormal_columns(m.n_tx, 5, 7), tie_columns(gmap, ng)])
    usage, dom = hip.isoform_usage_host(gmap, ng, X, want_dominant=True)
    return m, gmap, ng, X, usage, dom


@pytest.mark.parametrize("renumber", ["2", "0"])
def test_point_estimate_equals_the_host_function(renumber, point_case, monkeypatch):
    monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
    m, gmap, ng, X, usage, dom = point_case
    with EmsarHip(0) as d:
        for layout, merge in ((hip.LAYOUT_TILED, False), (hip.LAYOUT_TILED, True), (hip.LAYOUT_CSR, False)):
            d.upload_structure(m.n_tx, m.row_ptr, m.col_idx, layout=layout, merge_rows=merge)
            if layout == hip.LAYOUT_TILED:
                assert d.info()["renumbered"] == int(renumber == "2")
            d.set_gene_map(gmap, ng)
            u, k = d.isoform_usage(X, want_dominant=True)
            assert u.shape == usage.shape and k.shape == dom.shape and k.dtype == np.int32
            assert same(u, usage) and np.array_equal(k, dom), (layout, merge)
            assert same(d.isoform_usage(X), usage)
            u1, k1 = d.isoform_usage(X[1], want_dominant=True)              # one column given as 1-D
            assert u1.shape == (m.n_tx,) and same(u1, usage[1]) and np.array_equal(k1, dom[1])
            assert same(d.isoform_usage(X[6]), usage[6])


def _boot_case(d, name):
    if name == "vicugna_pe":
        m = get_fixture("vicugna_pe").model
        names, gmap = vicugna_genes()
        gmap, ng = np.asarray(gmap, dtype=np.int32), len(names)
    else:
        m, gmap, ng = family_problem(5)
    d.set_deterministic(True)              # set_mode 1: two calls give the same replicates, so calls can be compared
    d.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
    d.upload_sample(m.R, m.E, None)
    d.set_gene_map(gmap, ng)
    return m, gmap, ng


def usage_stats(reps, gmap, ng):
    """the definitions of include/emsar_hip.h on the replicates [B][n_tx]: usage per replicate, its Welford mean and sd, and the count
    of replicates in which a transcript is its gene's dominant isoform"""
    u, dom = hip.isoform_usage_host(gmap, ng, reps, want_dominant=True)
    mean, sd = welford(u) if len(reps) > 1 else (u[0].copy(), np.zeros(reps.shape[1]))
    t = np.arange(reps.shape[1])
    count = ((dom[:, np.maximum(gmap, 0)] == t[None, :]) & (gmap >= 0)[None, :]).sum(axis=0).astype(np.int32)
    return u, dom, mean, sd, count


def check_against_replicates(r, gmap, ng, what):
    u, dom, mean, sd, count = usage_stats(r["replicates"], gmap, ng)
    assert same(r["usage_mean"], mean) and same(r["usage_sd"], sd), what
    assert r["dominant_count"].dtype == np.int32 and np.array_equal(r["dominant_count"], count), what
    # every replicate with a positive gene sum has exactly one dominant isoform
    per_gene = np.bincount(gmap[gmap >= 0], weights=r["dominant_count"][gmap >= 0], minlength=ng)
    assert np.array_equal(per_gene, (dom >= 0).sum(axis=0)), what
    assert np.all(r["usage_mean"] >= 0) and np.all(r["usage_mean"] <= 1) and not r["usage_mean"][gmap < 0].any()
    return u


@pytest.mark.parametrize("set_mode", [0, 1], ids=["sets", "streaming"])
@pytest.mark.parametrize("name", ["family", "vicugna_pe"])
def test_bootstrap_against_its_own_replicates(name, set_mode):
    with EmsarHip(0) as d:
        m, gmap, ng = _boot_case(d, name)
        B, seed = 5, 21
        kw = solve_kw(set_mode)
        r = d.bootstrap_isoforms(B, seed, want_replicates=True, want_genes=True, set_mode=set_mode, **kw)
        assert "usage_q" not in r and "fpkm_q" not in r and r["stats"].n_replicates == B and r["stats"].reduce_ms > 0
        check_against_replicates(r, gmap, ng, (name, set_mode))
        assert r["usage_sd"].max() > 0 and 0 < r["dominant_count"].max() <= B
        g = d.bootstrap_genes(B, seed, want_replicates=True, set_mode=set_mode, **kw)
        for k in STATS:
            assert same(r[k], g[k]), (name, k)
        # without gene outputs and without replicates: the same isoform statistics
        plain = d.bootstrap_isoforms(B, seed, set_mode=set_mode, **kw)
        assert plain["replicates"] is None and "gene_fpkm_mean" not in plain
        for k in ISO + ("fpkm_mean", "fpkm_sd", "tpm_sd"):
            assert same(plain[k], r[k]) if k != "dominant_count" else np.array_equal(plain[k], r[k]), (name, k)


@pytest.mark.parametrize("B", [1, 5, 100])
def test_quantiles(B):
    with EmsarHip(0) as d:
        m, gmap, ng = _boot_case(d, "family")
        r = d.bootstrap_isoforms(B, 21, q=Q, want_replicates=True, want_genes=True, **SOLVE)
        assert r["qstats"].n_quantiles == len(Q) and r["qstats"].held_bytes == 8 * B * (m.n_tx + 1 + ng) and r["qstats"].quantile_ms > 0
        u = check_against_replicates(r, gmap, ng, B)
        assert same(r["usage_q"], hip.quantiles_host(u, Q))
        assert np.all(np.diff(r["usage_q"], axis=0) >= 0) and r["usage_q"].min() >= 0 and r["usage_q"].max() <= 1
        bq = d.bootstrap_quantiles(B, Q, 21, want_replicates=True, want_genes=True, **SOLVE)
        for k in STATS + QUANT:
            assert same(r[k], bq[k]), (B, k)
        if B == 1:
            assert same(r["usage_q"], np.repeat(u, len(Q), axis=0)) and not r["usage_sd"].any() and same(r["usage_mean"], u[0])
        else:
            assert (r["usage_q"][-1] > r["usage_q"][0]).any()
        # without gene outputs the usage quantiles are the same (the gene sums are computed either way)
        plain = d.bootstrap_isoforms(B, 21, q=Q, **SOLVE)
        assert same(plain["usage_q"], r["usage_q"]) and same(plain["fpkm_q"], r["fpkm_q"]) and "gene_fpkm_q" not in plain


@pytest.mark.parametrize("set_mode", [0, 1], ids=["sets", "streaming"])
def test_batch_invariance(set_mode, monkeypatch):
    with EmsarHip(0) as d:
        m, gmap, ng = _boot_case(d, "family")
        res = {}
        for batch in ("1", "3", None):
            if batch:
                monkeypatch.setenv("EMSAR_HIP_BOOT_BATCH", batch)
            else:
                monkeypatch.delenv("EMSAR_HIP_BOOT_BATCH")
            res[batch] = d.bootstrap_isoforms(7, 5, q=Q, want_replicates=True, want_genes=True, set_mode=set_mode, **solve_kw(set_mode))
            assert res[batch]["stats"].batch == (int(batch) if batch else 7)
        for batch in ("1", "3"):
            for k in STATS + QUANT + ISO + ("usage_q",):
                assert same(np.asarray(res[batch][k], dtype=np.float64), np.asarray(res[None][k], dtype=np.float64)), (batch, k)


def test_numbering_invariance(monkeypatch):
    """The shuffled family case of tests/test_bootq_gpu.py::test_numbering_invariance, the library's own numbering forced on and off:
    each numbering's isoform outputs are those of its own replicates, and where the replicates are the same bits so is every output."""
    m = _family(6)
    gmap = (np.arange(m.n_tx) // 3).astype(np.int32)
    gmap[7::13] = -1
    gmap[1:3] = -1                               # gene 0 keeps one transcript
    ng = int(gmap.max()) + 1
    res = []
    for renumber in ("2", "0"):
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
        with EmsarHip(0) as d:
            d.set_deterministic(True)
            d.upload_structure(m.n_tx, m.row_ptr, m.col_idx, layout=hip.LAYOUT_TILED)
            assert d.info()["renumbered"] == int(renumber == "2")
            d.upload_sample(m.R, m.E, host_den(m))
            d.set_gene_map(gmap, ng)
            r = d.bootstrap_isoforms(20, 3, q=Q, want_replicates=True, want_genes=True, **SOLVE)
            u = check_against_replicates(r, gmap, ng, renumber)
            assert same(r["usage_q"], hip.quantiles_host(u, Q)), renumber
            res.append(r)
    a, b = res
    if same(a["replicates"], b["replicates"]):
        for k in ISO + ("usage_q",) + QUANT:
            assert same(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), k


def test_context_is_left_as_it_was():
    with EmsarHip(0) as d:
        _boot_case(d, "family")
        for set_mode in (0, 1):
            kw = solve_kw(set_mode)
            th0, _ = d.solve(set_mode=set_mode, **kw)
            d.bootstrap_isoforms(4, 9, q=[0.5], set_mode=set_mode, **kw)
            d.bootstrap_isoforms(4, 9, set_mode=set_mode, **kw)
            th1, _ = d.solve(set_mode=set_mode, **kw)
            assert same(th0, th1), set_mode


def _call(d, n, q, outs=(1, 1, 1, 1, 1), genes=(0, 0, 0, 0, 0), iso=(1, 1, 1, 0), first=0, null_iso=False, n_q=None, max_iter=100000):
    """the C entry point itself: outs / genes = which of the five transcript / gene outputs are given (mean, sd, tpm_sd, fpkm_q, tpm_q),
    iso = which of usage_mean, usage_sd, dominant_count, usage_q"""
    T, G, K = d.n_tx, max(d.n_genes, 1), max(len(q), 1)
    f64p = C.POINTER(C.c_double)
    qa = np.ascontiguousarray(q, dtype=np.float64)
    p = hip.EmParams(max_iter, 1, 1e-10, 1e-6, 8, 0, 0.0, 0.0, 0.0, 0, 0)
    held = []

    def buf(given, size, dt=np.float64, ct=C.c_double):
        if not given:
            return None
        held.append(np.zeros(size, dtype=dt))
        return held[-1].ctypes.data_as(C.POINTER(ct))

    io = hip.IsoformOutputs(buf(iso[0], T), buf(iso[1], T), buf(iso[2], T, np.int32, C.c_int32), buf(iso[3], K * T))
    return d._L.emsar_hip_bootstrap_isoforms(
        d._h, C.byref(p), 1, first, n, len(q) if n_q is None else n_q, qa.ctypes.data_as(f64p) if len(q) else None,
        buf(outs[0], T), buf(outs[1], T), buf(outs[2], T), None, None, buf(outs[3], K * T), buf(outs[4], K * T),
        buf(genes[0], G), buf(genes[1], G), buf(genes[2], G), buf(genes[3], K * G), buf(genes[4], K * G), None, None,
        None if null_iso else C.byref(io))


def test_errors():
    ALL, NOQ = (1, 1, 1, 1, 1), (1, 1, 1, 0, 0)
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        with pytest.raises(hip.EmsarHipError) as e:
            d.isoform_usage(np.ones(3))                                   # no map
        assert e.value.status == -5
        d.set_gene_map([1, -1, 1], 2)
        assert _call(d, 5, []) == -5                                      # before upload_sample
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])                   # drops the map
        d.upload_sample([1, 2, 3], None, None)
        assert _call(d, 5, []) == -5 and _call(d, 5, [0.5], iso=(1, 1, 1, 1)) == -5     # no gene map
        d.set_gene_map([1, -1, 1], 2)
        # the point estimate
        u, k = d.isoform_usage(np.array([1.0, 2.0, 3.0]), want_dominant=True)
        assert same(u, np.array([0.25, 0.0, 0.75])) and k.tolist() == [-1, 2]
        f64p = C.POINTER(C.c_double)
        x, out = np.ones(3), np.zeros(3)
        assert d._L.emsar_hip_isoform_usage(d._h, 0, x.ctypes.data_as(f64p), out.ctypes.data_as(f64p), None) == -1
        assert d._L.emsar_hip_isoform_usage(d._h, 1, None, out.ctypes.data_as(f64p), None) == -1
        assert d._L.emsar_hip_isoform_usage(d._h, 1, x.ctypes.data_as(f64p), None, None) == -1
        assert d._L.emsar_hip_isoform_usage(None, 1, x.ctypes.data_as(f64p), out.ctypes.data_as(f64p), None) == -1
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(hip.EmsarHipError) as e:
                d.isoform_usage(np.array([1.0, bad, 3.0]))               # a transcript in no gene is checked as well
            assert e.value.status == -1, bad
        # the bootstrap: n_q == 0
        assert _call(d, 5, []) == 0 and _call(d, 5, [], outs=NOQ) == 0 and _call(d, 5, [], iso=(0, 0, 0, 0)) == 0
        assert _call(d, 5, [], null_iso=True) == -1
        assert _call(d, 5, [], iso=(1, 1, 1, 1)) == -1                   # usage_q without probabilities
        assert _call(d, 5, [], n_q=-1) == -1
        assert _call(d, 0, []) == -1 and _call(d, 2, [], first=-1) == -1
        for k in range(3):                                               # a transcript output missing
            assert _call(d, 5, [], outs=tuple(int(i != k) for i in range(3)) + (0, 0)) == -1
        assert _call(d, 5, [], genes=(1, 1, 1, 0, 0)) == 0 and _call(d, 5, [], genes=(1, 0, 1, 0, 0)) == -1
        assert _call(d, 5000, [], max_iter=50) == 0                      # nothing is held: no limit of 4096 replicates
        # n_q > 0: what bootstrap_quantiles rejects
        assert _call(d, 5, [0.5], iso=(1, 1, 1, 1)) == 0 and _call(d, 5, [0.5]) == 0
        assert _call(d, 5, [0.5], null_iso=True) == -1
        assert _call(d, 4096, [0.5], iso=(1, 1, 1, 1), max_iter=50) == 0 and _call(d, 4097, [0.5], max_iter=50) == -1
        assert _call(d, 5, [0.5], outs=NOQ) == -1 and _call(d, 5, [0.5], outs=(1, 1, 1, 1, 0)) == -1
        for bad in (float("nan"), float("inf"), -0.1, 1.5):
            assert _call(d, 5, [0.5, bad]) == -1, bad
        assert _call(d, 5, [0.5], genes=ALL) == 0
        for k in range(5):                                               # a gene output group only partly given
            assert _call(d, 5, [0.5], genes=tuple(int(i != k) for i in range(5))) == -1
        # closed form: theta_b = w_b, so the usage is that of the drawn weights
        r = d.bootstrap_isoforms(9, 1, q=[0.0, 0.5, 1.0], want_replicates=True)
        w = np.array([d.bootstrap_weights(1, b) for b in range(9)], dtype=np.float64)
        assert same(r["replicates"], w)
        tot = w[:, 0] + w[:, 2]
        u0 = np.where(tot > 0, w[:, 0] / np.where(tot > 0, tot, 1.0), 0.0)
        assert same(r["usage_q"][:, 0], np.sort(u0)[[0, 4, 8]]) and not r["usage_q"][:, 1].any()
        assert r["dominant_count"].tolist() == [int(((w[:, 0] >= w[:, 2]) & (tot > 0)).sum()), 0, int((w[:, 2] > w[:, 0]).sum())]


def test_non_finite_theta_is_err_numeric():
    """ERR_NUMERIC as solve (tests/test_hip_parity.py::test_non_finite_theta_is_reported_not_returned): effective lengths so small that
    theta_b = w_b / den leaves the double range in every replicate.  The call reports it, returns no statistics as if they were
    numbers, and leaves the context usable."""
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        d.set_gene_map([1, -1, 1], 2)
        d.upload_sample([100, 200, 300], None, np.full(3, 1e-308))        # w / den > 1.8e308
        for q in (None, [0.5]):
            with pytest.raises(hip.EmsarHipError) as e:
                d.bootstrap_isoforms(4, 1, q=q)
            assert e.value.status == -6
        d.upload_sample([100, 200, 300], None, np.ones(3))
        r = d.bootstrap_isoforms(4, 1, want_replicates=True)
        check_against_replicates(r, np.array([1, -1, 1], dtype=np.int32), 2, "after ERR_NUMERIC")


# ---- the command-line driver ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


HEAD = ["transcript_ID", "gene_ID", "FPKM", "usage", "dominant", "usage_mean", "usage_sd", "dominant_freq"]
QCLI = [0.025, 0.5, 0.975]
QHEAD = ["usage_q0.025000000000000001", "usage_q0.5", "usage_q0.97499999999999998"]


def _read_isoforms(path, head):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == head
    rows = [l.split("\t") for l in lines[1:]]
    assert all(len(r) == len(head) for r in rows)
    return rows


def _cli_sample_isoforms(fx, g2t, B, q, seed):
    """What emsar-hip does for a sample, through the Python bindings (tests/test_bootq_gpu.py::_cli_sample_quantiles): count, model,
    den in row order on the host, deterministic mode, the CLI's solver settings, the g2t file's gene map, solve, isoform_usage of the
    solve's FPKM, bootstrap_isoforms."""
    from emsar_amd import hostlib as HL
    opts = fx.meta["opts"]
    aln, fmt = aln_path(fx.dir)
    rsh = HL.HostRsh(os.path.join(fx.dir, "index.rsh"))
    cnt = rsh.count(aln, pe=int("-P" in opts), fmt=fmt, max_repeat=int(opts[opts.index("-k") + 1]) if "-k" in opts else 100,
                    strand=opts[opts.index("-s") + 1] if "-s" in opts else "ns")
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=200000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
    names, gmap = rsh.genes(g2t)
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        d.upload_structure(rsh.n_tx, rp, ci)
        d.upload_euma(rsh.euma)
        model = rsh.model(cnt, L=d.adj_euma(rsh.wf(cnt)))
        E = np.array(model.E_solver)
        den = np.zeros(rsh.n_tx)
        rows = np.repeat(np.arange(rsh.n_rows), np.diff(rp.astype(np.int64)))
        keep = E[rows] != 0.0
        np.add.at(den, ci[keep], E[rows][keep])             # in row order, one add at a time: the CLI's loop
        d.set_gene_map(gmap, len(names))
        d.upload_sample(np.array(cnt.R), E, den)
        th, _ = d.solve(**cli)
        usage, dom = d.isoform_usage(th, want_dominant=True)
        return usage, dom, d.bootstrap_isoforms(B, seed, q=q, **cli), names, np.asarray(gmap)


def test_cli_isoforms_file(tmp_path, _built):
    fx = get_fixture("vicugna_pe")
    g2t = os.path.join(fx.dir, "genes.g2t.gz")
    base = ["--bootstrap", "8", "--bootstrap-quantiles", "0.025,0.5,0.975", "--g2t", g2t]
    _run_cli(fx, tmp_path / "a", base)
    _run_cli(fx, tmp_path / "b", base + ["--isoforms"])
    _run_cli(fx, tmp_path / "c", base + ["--isoforms"])
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for ext in ("fpkm", "fraglength_effect", "segments", "gfpkm", "bootstrap", "gbootstrap", "bootq", "gbootq"):
        assert open(a / ("out.0." + ext), "rb").read() == open(b / ("out.0." + ext), "rb").read(), ext
    assert not (a / "out.0.isoforms").exists()
    assert open(b / "out.0.isoforms", "rb").read() == open(c / "out.0.isoforms", "rb").read()
    rows = _read_isoforms(str(b / "out.0.isoforms"), HEAD + QHEAD)
    usage, dom, r, names, gmap = _cli_sample_isoforms(fx, g2t, 8, QCLI, 1)
    text = [l.split("\t") for l in open(b / "out.0.fpkm").read().splitlines()[1:]]
    in_gene = np.nonzero(gmap >= 0)[0]
    # the order of .fpkm, its FPKM column, the gene of the map
    assert [row[0] for row in rows] == [text[t][0] for t in in_gene] and [row[2] for row in rows] == [text[t][1] for t in in_gene]
    assert [row[1] for row in rows] == [names[gmap[t]] for t in in_gene]
    # the library calls' values to the print quantum
    quantum = 1e-6
    cols = {3: usage, 5: r["usage_mean"], 6: r["usage_sd"], 7: r["dominant_count"] / 8.0, 8: r["usage_q"][0], 9: r["usage_q"][1], 10: r["usage_q"][2]}
    for j, want in cols.items():
        got = np.array([float(row[j]) for row in rows])
        assert np.all(np.abs(got - want[in_gene]) <= quantum), HEAD[j] if j < 8 else QHEAD[j - 8]
    assert [int(row[4]) for row in rows] == [int(dom[gmap[t]] == t) for t in in_gene]
    # one dominant isoform per expressed gene; a gene's usages add up to one (each is printed to half a quantum)
    per_gene = np.bincount(gmap[in_gene], weights=[float(row[4]) for row in rows], minlength=len(names))
    assert np.array_equal(per_gene, (dom >= 0).astype(float)) and 0 < per_gene.sum() <= len(names)
    n_iso = np.bincount(gmap[in_gene], minlength=len(names))
    tot = np.bincount(gmap[in_gene], weights=[float(row[3]) for row in rows], minlength=len(names))
    assert np.all(np.abs(tot - per_gene) <= (n_iso + 1) * 0.5 * quantum)
    assert max(float(row[6]) for row in rows) > 0 and max(float(row[10]) - float(row[8]) for row in rows) > 0


def test_cli_isoforms_columns_and_multisample(tmp_path, _built):
    fx = get_fixture("vicugna_pe")
    g2t = os.path.join(fx.dir, "genes.g2t.gz")
    # without a bootstrap: the base columns; with one and no quantiles: no usage_q columns
    _run_cli(fx, tmp_path / "p", ["--g2t", g2t, "--isoforms"])
    _run_cli(fx, tmp_path / "s", ["--g2t", g2t, "--isoforms", "--bootstrap", "8", "--bootstrap-seed", "2"])
    plain = _read_isoforms(str(tmp_path / "p" / "out.0.isoforms"), HEAD[:5])
    seed2 = _read_isoforms(str(tmp_path / "s" / "out.0.isoforms"), HEAD)
    assert [r[:5] for r in seed2] == plain
    assert not (tmp_path / "p" / "out.0.bootstrap").exists()
    # -M with two samples: a file each, seeds 1 and 2
    lst = tmp_path / "list.txt"
    aln = aln_path(fx.dir)[0]
    lst.write_text(aln + "\n" + aln + "\n")
    cmd = [CLI, "-q", "-M", "--gpus", "1", "--g2t", g2t, "--isoforms", "--bootstrap", "8"] + fx.meta["opts"] + [
        "-I", os.path.join(fx.dir, "index.rsh"), str(tmp_path / "m"), "out", str(lst)]
    subprocess.run(cmd, check=True, timeout=600)
    m0 = _read_isoforms(str(tmp_path / "m" / "out.0.isoforms"), HEAD)
    m1 = _read_isoforms(str(tmp_path / "m" / "out.1.isoforms"), HEAD)
    assert m1 == seed2 and [r[:5] for r in m0] == plain and m0 != m1
