"""GPU: the asymptotic standard errors on the device (emsar_hip_asymptotic) against the host function, bit for bit in every output --
at the edges of the kernels' size classes, alone and packed together, in every forced class, over long entry walks, across layouts
and numberings, on the solved fixtures; side effects, errors, and emsar-hip --asymptotic."""
import os
import subprocess

import numpy as np
import pytest

from emsar_amd import EmsarHip, _build, hip
from tests import asym_problems as AP
from tests.conftest import aln_path, get_fixture

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "emsar_amd", "emsar-hip")
CLI_SOLVE = dict(max_iter=200000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
EDGES = (1, 2, 8, 9, 64, 65, 192, 193)
STATS = ("components", "components_too_large", "components_infeasible", "components_unidentifiable", "rows_infeasible", "max_n",
         "min_pivot_ratio", "theta_unestimated_share")


def edge_part(n):
    return AP.component(n, np.random.default_rng(1000 + n))


def with_genes(p, seed=3):
    rng = np.random.default_rng(seed)
    p["n_genes"] = max(2, p["n_tx"] // 3)
    p["gene"] = rng.integers(-1, p["n_genes"], size=p["n_tx"]).astype(np.int32)
    return p


def host_of(p, **kw):
    return hip.asymptotic_host(p["n_tx"], p["row_ptr"], p["col_idx"], p["theta"], row_weight=p["weight"], E=p.get("E"),
                               gene_of_tx=p.get("gene"), n_genes=p.get("n_genes", 0), **kw)


def upload(d, p, layout=hip.LAYOUT_AUTO, merge=False):
    d.upload_structure(p["n_tx"], p["row_ptr"], p["col_idx"], layout=layout, merge_rows=merge)
    d.upload_sample(p["weight"], p.get("E"), None)
    if "gene" in p:
        d.set_gene_map(p["gene"], p["n_genes"])


def device_of(d, p, **kw):
    return d.asymptotic(p["theta"], genes="gene" in p, **kw)


def assert_device_equals_host(got, want, what=""):
    assert set(got) == set(want), what
    for k in want:
        if k != "stats":
            assert AP.same_bits(np.asarray(got[k]), np.asarray(want[k])), (what, k)
    for k in STATS:
        assert getattr(got["stats"], k) == getattr(want["stats"], k), (what, k)
    assert list(got["stats"].n_status) == list(want["stats"].n_status), what
    assert got["stats"].total_ms > 0 and got["stats"].plan_ms > 0


@pytest.fixture(scope="module")
def dev():
    with EmsarHip(0) as d:
        yield d


@pytest.fixture(scope="module")
def together():
    """every edge size and 301 small components in one structure: every component behind non-zero record offsets, the 8-lane class
    with dozens of full waves and a last one that is partly filled"""
    rng = np.random.default_rng(77)
    small = [AP.component(int(n), rng) for n in rng.integers(1, 9, size=301)]
    parts = small[:150] + [edge_part(n) for n in EDGES] + small[150:]
    p = with_genes(AP.assemble(parts, rng))
    p["edge_tids"] = {n: p["comp_tids"][150 + k] for k, n in enumerate(EDGES)}
    return p, host_of(p)


# ---- the size classes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EDGES)
def test_class_edges_alone(dev, together, n):
    p = with_genes(AP.assemble([edge_part(n)]), seed=n)
    upload(dev, p)
    got = device_of(dev, p, block_tid=n // 2)
    want = host_of(p, block_tid=n // 2)
    assert_device_equals_host(got, want, n)
    st = got["stats"]
    if n > 192:
        assert (got["status"] == AP.BIG).all() and got["block_cov"].shape == (0, 0) and sum(st.components_class) == 0
    else:
        assert (got["status"] == AP.EST).all() and got["block_cov"].shape == (n, n) and st.sets_ms > 0 and st.rows_ms > 0
        assert list(st.components_class) == [int(lo < n <= hi) for lo, hi in ((0, 1), (1, 8), (8, 64), (64, 192))]
        # the same component inside the big structure: the same bits (the gene sums apart: the neighbours' genes differ)
        big, bw = together
        tids = big["edge_tids"][n]
        for k in ("var", "rowsum", "partner_cov", "sd_fpkm"):
            assert AP.same_bits(got[k], np.ascontiguousarray(bw[k][tids])), (n, k)
        assert np.array_equal(got["partner"], np.where(bw["partner"][tids] >= 0, bw["partner"][tids] - tids[0], -1))


@pytest.mark.parametrize("force", [None, "1", "2"])
def test_class_edges_together(dev, together, force, monkeypatch):
    p, want = together
    if force:
        monkeypatch.setenv("EMSAR_HIP_ASYM_CLASS", force)
    upload(dev, p)
    got = device_of(dev, p)
    assert_device_equals_host(got, want, force)
    cls = list(got["stats"].components_class)
    assert sum(cls) == 301 + 7 and got["stats"].components_too_large == 1
    if force is None:
        assert cls == list(want["stats"].components_class) and cls[1] % 8 != 0 and cls[1] > 200 and cls[2] == cls[3] == 2
    else:
        assert cls[:int(force) + 1] == [0] * (int(force) + 1)
    for n in (2, 9, 65):                                    # the block output of a tid in each class, behind non-zero offsets
        t = int(p["edge_tids"][n][-1])
        b, bw = device_of(dev, p, block_tid=t), host_of(p, block_tid=t)
        assert AP.same_bits(b["block_cov"], bw["block_cov"]) and list(b["block_tids"]) == list(p["edge_tids"][n]) == list(bw["block_tids"])


def test_long_walks(dev):
    p = with_genes(AP.assemble([AP.component(5, np.random.default_rng(9), long_walk=1000), AP.component(1, np.random.default_rng(10), long_walk=1000),
                                AP.component(70, np.random.default_rng(11), long_walk=1000)], np.random.default_rng(12)))
    assert np.bincount(p["col_idx"]).max() > 1000
    upload(dev, p)
    assert_device_equals_host(device_of(dev, p), host_of(p))


# ---- layouts and numberings ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("renumber", ["2", "0"])
def test_same_bits_across_layouts_and_numbering(renumber, monkeypatch):
    monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
    rng = np.random.default_rng(21)
    parts = [AP.component(int(n), rng) for n in rng.integers(1, 30, size=120)] + [AP.component(100, rng)]
    p = with_genes(AP.assemble(parts, rng, shuffle_tids=True))
    want = host_of(p, block_tid=5)
    with EmsarHip(0) as d:
        for layout, merge in ((hip.LAYOUT_TILED, False), (hip.LAYOUT_TILED, True), (hip.LAYOUT_CSR, False)):
            upload(d, p, layout, merge)
            if layout == hip.LAYOUT_TILED:
                assert d.info()["renumbered"] == int(renumber == "2")
            assert_device_equals_host(device_of(d, p, block_tid=5), want, (layout, merge))


# ---- the other statuses -------------------------------------------------------------------------------------------------------------

def test_unidentifiable_infeasible_boundary(dev):
    rng = np.random.default_rng(31)
    parts = [AP.component(6, rng), ([[0, 1], [1, 0], [1, 0, 2], [2]], np.array([3, 8, 2, 5]), np.array([2.0, 5.0, 1.0])),   # 0 and 1 confounded
             ([[0, 1], [0]], np.array([4, 0]), np.array([0.0, 0.0])),                                                     # reads over theta = 0
             ([[0]], np.array([0]), np.array([3.0])), AP.component(12, rng)]                                              # active, no reads
    p = with_genes(AP.assemble(parts, rng))
    upload(dev, p)
    for cut in (None, -1.0, 0.0, 2.5):
        got, want = device_of(dev, p, boundary_cut=cut), host_of(p, boundary_cut=cut)
        assert_device_equals_host(got, want, cut)
        assert got["stats"].rows_infeasible == 1 and got["stats"].components_unidentifiable >= 1 + (cut != 2.5)
    st = device_of(dev, p, boundary_cut=-1.0)["status"]
    assert sorted(set(st)) == [AP.EST, AP.UNI, AP.INF] and (st == AP.INF).sum() == 2
    st = device_of(dev, p)["status"]
    assert sorted(set(st)) == [AP.EST, AP.BND, AP.UNI] and (st == AP.BND).sum() == 2
    unid = p["comp_tids"][1]
    got = device_of(dev, p)
    assert (got["status"][unid] == AP.UNI).all() and (got["blocker"][unid] == unid[1]).all() and np.isinf(got["var"][unid]).all()
    assert np.isinf(got["gene_sd"][p["gene"][unid][p["gene"][unid] >= 0]]).all()


# ---- side effects -------------------------------------------------------------------------------------------------------------------

def test_context_untouched():
    m = get_fixture("syn300_k2").model
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        d.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
        d.upload_sample(m.R, m.E, None)
        th1, st = d.solve(**CLI_SOLVE)
        a = d.asymptotic(th1)                                # uploads the caller-order CSR the model fit shares
        before = d.get_theta()
        d.asymptotic(th1 * 0.5 + 1.0, block_tid=0)
        assert np.array_equal(d.get_theta(), before)
        th2, _ = d.solve(**CLI_SOLVE)
        assert np.array_equal(th1, th2)
        fit = d.model_fit(th1, m.E, rows=True)               # builds its index next to that CSR
        want = hip.model_fit_host(m.n_tx, m.row_ptr, m.col_idx, th1, row_weight=m.R, E=m.E, rows=True)
        for k in ("tx_chi2", "tx_miss", "tx_df", "tx_worst_row", "row_mu", "row_chi2"):
            assert np.array_equal(fit[k], want[k]), k
        b = d.asymptotic(th1)                                # and the other way round
        AP.assert_same_result(a, b)
        th3, _ = d.solve(**CLI_SOLVE)
        assert np.array_equal(th1, th3)


@pytest.mark.parametrize("case", ["syn2k_se", "vicugna_pe"])
def test_solved_fixtures(case):
    m = get_fixture(case).model
    with EmsarHip(0) as d:
        d.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
        d.upload_sample(m.R, m.E, None)
        th, st = d.solve(**CLI_SOLVE)
        got = d.asymptotic(th)
    want = hip.asymptotic_host(m.n_tx, m.row_ptr, m.col_idx, th, row_weight=m.R, E=m.E)
    assert_device_equals_host(got, want, case)
    s = got["stats"]
    print(case, s.as_dict())
    assert sum(s.n_status) == m.n_tx and s.n_status[AP.BIG] == 0 and s.components_too_large == 0
    est = got["status"] == AP.EST
    assert est.sum() > m.n_tx // 4 and np.isfinite(got["var"][est]).all() and (got["var"][est] > 0).all()


def test_errors():
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3, 5], [0, 1, 2, 0, 1])
        with pytest.raises(hip.EmsarHipError) as e:
            d.asymptotic(np.ones(3))                                   # before upload_sample
        assert e.value.status == -5
        d.upload_sample([1, 2, 3, 4], None, None)
        with pytest.raises(hip.EmsarHipError) as e:
            d.asymptotic(np.ones(3), genes=True)                       # gene outputs without a map
        assert e.value.status == -5
        for bad in (np.nan, -1.0, np.inf):
            with pytest.raises(hip.EmsarHipError) as e:
                d.asymptotic([1.0, bad, 1.0])
            assert e.value.status == -1
        for tid in (3, 100):
            with pytest.raises(hip.EmsarHipError) as e:
                d.asymptotic(np.ones(3), block_tid=tid)
            assert e.value.status == -1
        assert d._L.emsar_hip_asymptotic(d._h, None, None, None, None) == -1            # NULL theta
        import ctypes as C
        o, var, gsd = hip.AsymOutputs(), np.zeros(3), np.zeros(1)
        o.var, o.gene_sd = hip._p(var, C.c_double), hip._p(gsd, C.c_double)
        th = np.ones(3)
        assert d._L.emsar_hip_asymptotic(d._h, hip._p(th, C.c_double), None, C.byref(o), None) == -1     # a gene group partly given
        # the context stays usable
        got = d.asymptotic([1.0, 2.0, 3.0])
        assert (got["status"] == [AP.EST, AP.EST, AP.EST]).all() and got["partner"].tolist() == [1, 0, -1]
        th, st = d.solve(max_iter=200000, tol=1e-10)
        assert st.converged == 1 and abs(th[2] - 3.0) < 1e-9
        d.set_gene_map([0, 0, -1], 1)
        r = d.asymptotic(th, genes=True)
        assert r["gene_status"].tolist() == [AP.EST] and r["gene_sd"][0] > 0 and np.isnan(r["usage_sd"][2])


# ---- the command-line driver ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


def _run_cli(fx, out, extra):
    cmd = [CLI, "-q", "-g"] + fx.meta["opts"] + extra + ["-I", os.path.join(fx.dir, "index.rsh"), str(out), "out", aln_path(fx.dir)[0]]
    subprocess.run(cmd, check=True, timeout=600)


ASYM_HEAD = "tid\ttranscriptID\tFPKM\tsd_FPKM\tTPM\tsd_TPM\tstatus\tpartner\tpartner_corr"


@pytest.mark.parametrize("case,genes", [("syn300_se", False), ("vicugna_pe", True)])
def test_cli_asymptotic(case, genes, tmp_path, _built):
    fx = get_fixture(case)
    base = ["--g2t", os.path.join(fx.dir, "genes.g2t.gz")] if genes else []
    _run_cli(fx, tmp_path / "a", base)
    _run_cli(fx, tmp_path / "b", base + ["--asymptotic"])
    a, b = tmp_path / "a", tmp_path / "b"
    for ext in ("fpkm",) + (("gfpkm",) if genes else ()):
        assert open(a / ("out.0." + ext), "rb").read() == open(b / ("out.0." + ext), "rb").read(), ext
    assert not (a / "out.0.asym").exists() and (b / "out.0.gasym").exists() == genes
    lines = open(b / "out.0.asym").read().splitlines()
    assert lines[0] == ASYM_HEAD + ("\tusage_sd" if genes else "")
    rows = [l.split("\t") for l in lines[1:]]
    text = [l.split("\t") for l in open(b / "out.0.fpkm").read().splitlines()[1:]]
    assert len(rows) == fx.n_tx and all(len(r) == 9 + genes for r in rows)
    assert [r[1] for r in rows] == [t[0] for t in text] and [r[2] for r in rows] == [t[1] for t in text]      # the FPKM column is the .fpkm file's
    assert [int(r[0]) for r in rows] == list(range(fx.n_tx)) and {r[6] for r in rows} <= set(AP.STATUS)
    names = {r[1] for r in rows}
    for r in rows:
        if r[6] == "ESTIMATED":
            assert float(r[3]) > 0 or float(r[2]) == 0.0
            assert (r[7] == "-" and r[8] == "nan") or (r[7] in names and -1.000001 <= float(r[8]) <= 1.000001), r
        if r[6] == "BOUNDARY":
            assert float(r[3]) == 0.0 and r[7] == "-"
    assert sum(r[6] == "ESTIMATED" for r in rows) > fx.n_tx // 4
    if genes:
        g = [l.split("\t") for l in open(b / "out.0.gasym").read().splitlines()]
        gf = [l.split("\t") for l in open(b / "out.0.gfpkm").read().splitlines()]
        assert g[0] == ["geneID", "gFPKM", "sd", "status"] and len(g) == len(gf)              # one line per gene
        assert [r[0] for r in g[1:]] == [r[0] for r in gf[1:]] and [r[1] for r in g[1:]] == [r[1] for r in gf[1:]]
        assert {r[3] for r in g[1:]} <= set(AP.STATUS)
