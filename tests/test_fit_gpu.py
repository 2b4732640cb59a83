"""GPU: the model fit on the device (emsar_hip_model_fit) against the host function -- bit for bit except the deviance, which goes
through the device's log -- the same bits across layouts, merged rows and the library's numbering, repeatability and side effects,
the edge cases and errors of the ABI, and emsar-hip --fit."""
import os
import subprocess

import numpy as np
import pytest

from emsar_amd import EmsarHip, _build, hip
from tests.conftest import aln_path, get_fixture
from tests.test_fit_cpu import EPS, family_fit_problem, np_rows, staircase_reference
from tests.test_genes_gpu import vicugna_genes

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "emsar_amd", "emsar-hip")
SOLVE = dict(max_iter=200000, tol=1e-10)
TX = ("tx_chi2", "tx_dev", "tx_miss", "tx_df", "tx_worst_row")
ROWS = ("row_mu", "row_chi2", "row_dev")
GENES = ("gene_chi2", "gene_dev", "gene_miss", "gene_df")


def host_of(p, theta=None, E="own", genes=True):
    return hip.model_fit_host(p["n_tx"], p["rp"], p["ci"], p["theta"] if theta is None else theta, row_weight=p["R"],
                              E=p["E"] if isinstance(E, str) else E, rows=True, gene_of_tx=p["gene_of_tx"] if genes else None,
                              n_genes=p["n_genes"] if genes else 0)


def upload(d, p, layout=hip.LAYOUT_AUTO, merge=False, genes=True):
    d.upload_structure(p["n_tx"], p["rp"], p["ci"], layout=layout, merge_rows=merge)
    d.upload_sample(p["R"], p["E"], None)
    if genes:
        d.set_gene_map(p["gene_of_tx"], p["n_genes"])


def assert_device_equals_host(got, want, p, theta, E, what, genes=True):
    """Everything but dev bit for bit.  dev: per row |delta| <= 2^-52 (8 R |log(R / mu)| + 2 d) -- two logs within 1 ulp, the
    subtraction and the doubling, a margin of 2; per transcript, gene and for the total 1e-12 * sum p (2 R |log(R / mu)| + d)."""
    for k in ("tx_chi2", "tx_miss", "tx_df", "tx_worst_row", "row_mu", "row_chi2") + (("gene_chi2", "gene_miss", "gene_df") if genes else ()):
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:5])
    r = np_rows(p["rp"], p["ci"], p["R"], E, np.asarray(theta, dtype=np.float64))
    fin = np.isfinite(want["row_dev"])
    assert np.array_equal(np.isinf(got["row_dev"]), ~fin), what
    err = np.abs(got["row_dev"][fin] - want["row_dev"][fin])
    tol = EPS * (8.0 * r["L"][fin] + 2.0 * want["row_dev"][fin])
    print("%s: row dev max error %.3g, max error / tolerance %.3g" % (what, err.max(initial=0.0), (err / np.maximum(tol, 1e-300)).max(initial=0.0)))
    assert np.all(err <= tol), (what, "row_dev")
    # the scale of a transcript's deviance: sum over its entries of p (2 L + d)
    rp = np.asarray(p["rp"]).astype(np.int64)
    row_of = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    s = np.where(r["pos"], r["S"], 0.0)[row_of]
    with np.errstate(all="ignore"):
        w = np.where(s > 0, np.asarray(theta)[p["ci"]] / np.where(s > 0, s, 1.0) * (2.0 * r["L"] + np.where(r["pos"], r["d"], 0.0))[row_of], 0.0)
    scale = {"tx_dev": np.bincount(p["ci"], weights=w, minlength=p["n_tx"])}
    if genes:
        g = np.asarray(p["gene_of_tx"])
        scale["gene_dev"] = np.bincount(g[g >= 0], weights=scale["tx_dev"][g >= 0], minlength=p["n_genes"])
    for k, sc in scale.items():
        err = np.where(got[k] == want[k], 0.0, np.abs(got[k] - np.where(np.isinf(want[k]), 0.0, want[k])))
        print("%s: %s max error %.3g, max error / scale %.3g" % (what, k, err.max(initial=0.0), (err / np.maximum(sc, 1e-300)).max(initial=0.0)))
        assert np.all(err <= 1e-12 * sc), (what, k)
    a, b = got["stats"], want["stats"]
    for k in ("rows_inside", "rows_infeasible", "index_slots", "index_bytes", "sum_chi2", "sum_miss"):
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))
    assert abs(a.sum_dev - b.sum_dev) <= 1e-12 * (2.0 * r["L"][r["pos"]].sum() + r["d"][r["pos"]].sum()), what
    assert a.kernel_ms > 0 and a.total_ms >= a.kernel_ms * 0.5


def same_bits(a, b, keys, what="", dev_total=True):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    for k in ("rows_inside", "rows_infeasible", "index_slots", "sum_chi2", "sum_miss") + (("sum_dev",) if dev_total else ()):
        assert getattr(a["stats"], k) == getattr(b["stats"], k), (what, k)


@pytest.fixture(scope="module")
def dev():
    with EmsarHip(0) as d:
        yield d


# ---- device equals host -----------------------------------------------------------------------------------------------------------

def test_staircase_device_equals_host(dev):
    p, _ = staircase_reference()
    upload(dev, p)
    got = dev.model_fit(p["theta"], p["E"], rows=True, genes=True)
    assert_device_equals_host(got, host_of(p), p, p["theta"], p["E"], "staircase")
    st = got["stats"]
    assert len(p["ci"]) <= st.index_slots <= len(p["ci"]) + 64 * 255 and st.rows_infeasible > 0


def test_family_device_equals_host(dev):
    p = family_fit_problem()
    upload(dev, p)
    th, st = dev.solve(**SOLVE)
    assert st.converged == 1
    for theta, what in ((th, "family at the device's MLE"), (p["theta"], "family at the oracle's theta")):
        got = dev.model_fit(theta, p["E"], rows=True, genes=True)
        assert_device_equals_host(got, host_of(p, theta=theta), p, theta, p["E"], what)
    assert (np.bincount(p["gene_of_tx"][p["gene_of_tx"] >= 0]) >= 1000).any()


def test_vicugna_device_equals_host(dev):
    m = get_fixture("vicugna_pe").model
    names, gmap = vicugna_genes()
    p = dict(n_tx=m.n_tx, rp=m.row_ptr, ci=m.col_idx, R=m.R, E=m.E, gene_of_tx=np.asarray(gmap, dtype=np.int32), n_genes=len(names))
    upload(dev, p)
    th, st = dev.solve(**SOLVE)
    assert st.converged == 1
    got = dev.model_fit(th, m.E, rows=True, genes=True)
    assert_device_equals_host(got, host_of(p, theta=th), p, th, m.E, "vicugna_pe at its MLE")
    assert got["stats"].sum_dev > 0 and got["stats"].rows_infeasible == 0      # the MLE is feasible
    # another E for this call than the sample's: R stays the uploaded one
    E2 = np.where(np.arange(len(m.E)) % 3 == 0, 0.0, np.asarray(m.E) * 1.5)
    got = dev.model_fit(th, E2, rows=True, genes=True)
    assert_device_equals_host(got, host_of(p, theta=th, E=E2), p, th, E2, "vicugna_pe, another E")


# ---- invariance -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("renumber", ["2", "0"])
def test_same_bits_across_layouts_and_numbering(renumber, monkeypatch):
    monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
    p = family_fit_problem()
    want = host_of(p)
    first = None
    with EmsarHip(0) as d:
        for layout, merge in ((hip.LAYOUT_TILED, False), (hip.LAYOUT_TILED, True), (hip.LAYOUT_CSR, False)):
            upload(d, p, layout, merge)
            if layout == hip.LAYOUT_TILED:
                assert d.info()["renumbered"] == int(renumber == "2")
            got = d.model_fit(p["theta"], p["E"], rows=True, genes=True)
            first = first or got
            same_bits(got, first, TX + ROWS + GENES, (layout, merge))
            same_bits(got, want, ("tx_chi2", "tx_miss", "tx_df", "tx_worst_row", "gene_chi2", "gene_df", "row_mu", "row_chi2"), (layout, merge), dev_total=False)


def test_same_bits_staircase_merged_and_csr():
    p, _ = staircase_reference()
    res = []
    with EmsarHip(0) as d:
        for layout, merge in ((hip.LAYOUT_TILED, False), (hip.LAYOUT_TILED, True), (hip.LAYOUT_CSR, False)):
            upload(d, p, layout, merge)
            res.append(d.model_fit(p["theta"], p["E"], rows=True, genes=True))
    for r in res[1:]:
        same_bits(r, res[0], TX + ROWS + GENES)


# ---- repeatability and side effects -----------------------------------------------------------------------------------------------

def test_second_call_and_another_structure(dev):
    p, _ = staircase_reference()
    upload(dev, p)
    a = dev.model_fit(p["theta"], p["E"], rows=True, genes=True)
    b = dev.model_fit(p["theta"], p["E"], rows=True, genes=True)           # the index is there already
    same_bits(a, b, TX + ROWS + GENES)
    assert b["stats"].index_slots == a["stats"].index_slots > 0
    c = dev.model_fit(p["theta"] * 2.0, None, rows=True, genes=False)       # another theta, E = 1.0, no genes: the same index
    pe = dict(p, R=np.where(p["E"] == 0.0, 0, p["R"]))                      # R is the uploaded one: 0 where E was 0 at upload_sample
    assert_device_equals_host(c, host_of(pe, theta=p["theta"] * 2.0, E=None, genes=False), pe, p["theta"] * 2.0, None, "second theta", genes=False)
    q = family_fit_problem()                                               # another matrix: its own index
    upload(dev, q)
    got = dev.model_fit(q["theta"], q["E"], rows=True, genes=True)
    assert_device_equals_host(got, host_of(q), q, q["theta"], q["E"], "after another upload_structure")
    assert got["stats"].index_slots != a["stats"].index_slots
    # a new sample on the same structure: R follows it
    R2 = np.asarray(q["R"]) * 2 + 1
    dev.upload_sample(R2, q["E"], None)
    q2 = dict(q, R=R2)
    assert_device_equals_host(dev.model_fit(q["theta"], q["E"], rows=True, genes=True), host_of(q2), q2, q["theta"], q["E"], "after another upload_sample")


@pytest.mark.parametrize("set_mode", [0, 1], ids=["sets", "streaming"])
def test_solve_fit_solve(set_mode):
    p = family_fit_problem()
    # streaming only, this problem takes 10^4 passes to tol 1e-10: 300 passes are the same check (deterministic mode: the same bits)
    kw = SOLVE if set_mode == 0 else dict(max_iter=300, tol=1e-10)
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        upload(d, p)
        th1, _ = d.solve(set_mode=set_mode, **kw)
        d.model_fit(th1, p["E"], rows=True, genes=True)
        th2, _ = d.solve(set_mode=set_mode, **kw)
        assert np.array_equal(th1, th2)
        before = d.get_theta()
        d.model_fit(p["theta"], p["E"])
        assert np.array_equal(d.get_theta(), before)                       # the current point is not the fit's theta


# ---- edge cases and errors --------------------------------------------------------------------------------------------------------

def test_edge_cases(dev):
    p, _ = staircase_reference()
    upload(dev, p)
    # all-zero theta: every inside row with reads is infeasible, nothing reaches a transcript
    z = np.zeros(p["n_tx"])
    got = dev.model_fit(z, p["E"], rows=True, genes=True)
    assert_device_equals_host(got, host_of(p, theta=z), p, z, p["E"], "all-zero theta")
    assert got["stats"].rows_infeasible > 1000 and not got["tx_df"].any() and np.all(got["tx_worst_row"] == -1)
    assert (got["stats"].sum_chi2, got["stats"].sum_dev, got["stats"].sum_miss) == (0.0, 0.0, 0.0)
    # no inside rows: E = 0 everywhere at this call
    E0 = np.zeros(len(p["R"]))
    got = dev.model_fit(p["theta"], E0, rows=True, genes=True)
    assert got["stats"].rows_inside == 0 and got["stats"].rows_infeasible == 0
    for k in TX[:4] + ROWS + GENES:
        assert not got[k].any(), k
    assert np.all(got["tx_worst_row"] == -1)
    # a single row, a gene-less call
    dev.upload_structure(3, [0, 3], [2, 0, 2])
    dev.upload_sample([7], None, None)
    got = dev.model_fit([1.0, 5.0, 0.5], rows=True)
    want = hip.model_fit_host(3, [0, 3], [2, 0, 2], [1.0, 5.0, 0.5], row_weight=[7], rows=True)
    for k in ("tx_chi2", "tx_miss", "tx_df", "tx_worst_row", "row_mu", "row_chi2"):
        assert np.array_equal(got[k], want[k]), k
    assert np.all(np.abs(got["tx_dev"] - want["tx_dev"]) <= 1e-12 * want["tx_dev"]) and want["tx_dev"][0] > 0
    assert got["row_mu"].tolist() == [2.0] and got["tx_df"].tolist() == [0.5, 0.0, 0.5] and got["tx_worst_row"].tolist() == [0, -1, 0]
    assert "gene_chi2" not in got


def test_errors():
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        with pytest.raises(hip.EmsarHipError) as e:
            d.model_fit(np.ones(3))                                    # before upload_sample
        assert e.value.status == -5
        d.upload_sample([1, 2, 3], None, None)
        with pytest.raises(hip.EmsarHipError) as e:
            d.model_fit(np.ones(3), genes=True)                        # gene outputs without a map
        assert e.value.status == -5
        for bad in (np.nan, -1.0, np.inf):
            with pytest.raises(hip.EmsarHipError) as e:
                d.model_fit([1.0, bad, 1.0])
            assert e.value.status == -1
            with pytest.raises(hip.EmsarHipError) as e:
                d.model_fit(np.ones(3), E=[1.0, bad, 1.0])
            assert e.value.status == -1
        assert d._L.emsar_hip_model_fit(d._h, None, None, None, None) == -1          # NULL theta
        # the context stays usable
        got = d.model_fit([1.0, 2.0, 6.0], rows=True)
        assert got["row_mu"].tolist() == [1.0, 2.0, 6.0] and got["tx_miss"].tolist() == [0.0, 0.0, 3.0] and got["tx_worst_row"].tolist() == [-1, -1, 2]
        th, st = d.solve(**SOLVE)
        assert np.allclose(th, [1.0, 2.0, 3.0])
        d.set_gene_map([0, 0, -1], 1)
        assert d.model_fit(th, genes=True)["gene_df"].tolist() == [2.0]


# ---- the command-line driver ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


def _run_cli(fx, out, extra):
    cmd = [CLI, "-q", "-g"] + fx.meta["opts"] + extra + ["-I", os.path.join(fx.dir, "index.rsh"), str(out), "out", aln_path(fx.dir)[0]]
    subprocess.run(cmd, check=True, timeout=600)


def _cli_sample_fit(fx, g2t):
    """What emsar-hip --fit does for a sample, through the Python bindings: count, model, den in row order on the host, deterministic
    mode, the CLI's solver settings, solve, model_fit of the solve's FPKM with the E of the solve."""
    from emsar_amd import hostlib as HL
    opts = fx.meta["opts"]
    aln, fmt = aln_path(fx.dir)
    rsh = HL.HostRsh(os.path.join(fx.dir, "index.rsh"))
    cnt = rsh.count(aln, pe=int("-P" in opts), fmt=fmt, max_repeat=int(opts[opts.index("-k") + 1]) if "-k" in opts else 100,
                    strand=opts[opts.index("-s") + 1] if "-s" in opts else "ns")
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=200000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
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
        names = gmap = None
        if g2t:
            names, gmap = rsh.genes(g2t)
            d.set_gene_map(gmap, len(names))
        d.upload_sample(np.array(cnt.R), E, den)
        th, _ = d.solve(**cli)
        return th, den, d.model_fit(th, E, genes=bool(g2t)), names, gmap


FIT_HEAD = "transcriptID\tFPKM\teff_segments\tchi2\tdeviance\tmiss_reads\tmiss_fraction\tworst_segment"
GFIT_HEAD = "geneID\teff_segments\tchi2\tdeviance\tmiss_reads\tmiss_fraction"


def _fraction(miss, expected):
    with np.errstate(all="ignore"):
        return np.where(expected != 0.0, miss / np.where(expected != 0.0, expected, 1.0), 0.0)


@pytest.mark.parametrize("case,genes", [("toy5_pe", False), ("vicugna_pe", True)])
def test_cli_fit(case, genes, tmp_path, _built):
    fx = get_fixture(case)
    g2t = os.path.join(fx.dir, "genes.g2t.gz") if genes else None
    base = ["--g2t", g2t] if genes else []
    _run_cli(fx, tmp_path / "a", base)
    _run_cli(fx, tmp_path / "b", base + ["--fit"])
    a, b = tmp_path / "a", tmp_path / "b"
    for ext in ("fpkm", "fraglength_effect", "segments") + (("gfpkm",) if genes else ()):
        assert open(a / ("out.0." + ext), "rb").read() == open(b / ("out.0." + ext), "rb").read(), ext
    assert not (a / "out.0.fit").exists() and not (a / "out.0.gfit").exists() and (b / "out.0.gfit").exists() == genes
    th, den, fit, names, gmap = _cli_sample_fit(fx, g2t)
    quantum = 1e-6                                           # "%lf"
    lines = open(b / "out.0.fit").read().splitlines()
    assert lines[0] == FIT_HEAD
    rows = [l.split("\t") for l in lines[1:]]
    text = [l.split("\t") for l in open(b / "out.0.fpkm").read().splitlines()[1:]]
    assert len(rows) == fx.n_tx and all(len(r) == 8 for r in rows)
    assert [r[0] for r in rows] == [t[0] for t in text] and [r[1] for r in rows] == [t[1] for t in text]
    cols = {2: fit["tx_df"], 3: fit["tx_chi2"], 4: fit["tx_dev"], 5: fit["tx_miss"], 6: _fraction(fit["tx_miss"], th * den)}
    for j, want in cols.items():
        got = np.array([float(r[j]) for r in rows])
        assert np.all(np.abs(got - want) <= quantum + 1e-15 * np.abs(want)), FIT_HEAD.split("\t")[j]
    assert [r[7] for r in rows] == ["c%d" % w if w >= 0 else "-" for w in fit["tx_worst_row"]]
    seg_ids = {l.split("\t")[0] for l in open(b / "out.0.segments").read().splitlines()}
    assert {r[7] for r in rows} - {"-"} <= seg_ids
    # (toy5_pe is five single-transcript segments: the closed form fits them exactly and no segment misses)
    assert any(r[7] != "-" for r in rows) == bool((fit["tx_miss"] > 0).any()) == genes
    if genes:
        lines = open(b / "out.0.gfit").read().splitlines()
        assert lines[0] == GFIT_HEAD
        grows = [l.split("\t") for l in lines[1:]]
        assert [r[0] for r in grows] == list(names) and all(len(r) == 6 for r in grows)
        gmap = np.asarray(gmap)
        expected = np.zeros(len(names))
        np.add.at(expected, gmap[gmap >= 0], (th * den)[gmap >= 0])
        cols = {1: fit["gene_df"], 2: fit["gene_chi2"], 3: fit["gene_dev"], 4: fit["gene_miss"], 5: _fraction(fit["gene_miss"], expected)}
        for j, want in cols.items():
            got = np.array([float(r[j]) for r in grows])
            assert np.all(np.abs(got - want) <= quantum + 1e-15 * np.abs(want)), GFIT_HEAD.split("\t")[j]
