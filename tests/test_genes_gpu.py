"""GPU: gene-level sums (emsar_hip_set_gene_map / gene_sums / bootstrap_genes) -- the fixed chunked order bit for bit across layouts,
renumbering and batch sizes, the bootstrap's gene statistics against its own replicates, the isoforms' negative covariance on
vicugna_pe, the ABI's errors, and emsar-hip --g2t against the reference's gene step."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from emsar_amd import EmsarHip, _build, hip, hostlib, synth
from tests.conftest import GOLDEN, aln_path, get_fixture
from tests.test_genes_cpu import fpkm_columns, read_gfpkm

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "emsar_amd", "emsar-hip")
VIC = os.path.join(GOLDEN, "vicugna_pe")
SOLVE = dict(max_iter=200000, tol=1e-10)
CHUNK = 256


def chunked_sums(X, gene_of_tx, n_genes):
    """The documented order (include/emsar_hip.h): a gene's transcripts by ascending tid, chunks of 256 added left to right, then the
    chunk sums left to right.  np.cumsum adds sequentially."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    out = np.zeros((X.shape[0], n_genes))
    order = np.argsort(gene_of_tx, kind="stable")
    g_sorted = gene_of_tx[order]
    starts = np.searchsorted(g_sorted, np.arange(n_genes + 1))
    for g in range(n_genes):
        idx = order[starts[g]:starts[g + 1]]
        if len(idx) == 0:
            continue
        parts = np.stack([X[:, idx[c:c + CHUNK]].cumsum(axis=1)[:, -1] for c in range(0, len(idx), CHUNK)], axis=1)
        out[:, g] = parts.cumsum(axis=1)[:, -1]
    return out


def welford(rows):
    """k_boot_accum's recurrence over rows [B][n] in order: mean and sample sd"""
    m = np.zeros(rows.shape[1])
    q = np.zeros(rows.shape[1])
    for k, x in enumerate(rows, start=1):
        d = x - m
        m = m + d / k
        q = q + d * (x - m)
    return m, np.sqrt(q / (len(rows) - 1))


def vicugna_genes():
    r = hostlib.HostRsh(os.path.join(VIC, "index.rsh"))
    return r.genes(os.path.join(VIC, "genes.g2t.gz"))


def family_problem(seed=3):
    """families of the generator as genes, plus one gene of >= 1000 transcripts drawn from across the matrix (several chunks)"""
    sizes = [2, 3, 5, 8, 13, 40, 1, 1, 4] * 60
    n_tx, rp, ci, R = synth.family_matrix(sizes, rows_per_tid=3, seed=seed)
    E = np.random.default_rng(seed).uniform(0.5, 2.0, size=len(R))
    fam = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    rng = np.random.default_rng(seed + 1)
    big = rng.choice(n_tx, size=1100, replace=False)
    gene_of_tx = fam.copy()
    gene_of_tx[big] = len(sizes)                       # the big gene
    gene_of_tx[rng.choice(n_tx, size=20, replace=False)] = -1
    n_genes = len(sizes) + 2                            # and one gene without transcripts
    return O.Csr(n_tx, rp, ci, R=R, E=E), gene_of_tx, n_genes


@pytest.fixture(scope="module")
def dev():
    with EmsarHip(0) as d:
        yield d


def test_gene_sums_vicugna_bit_identical(dev):
    names, gmap = vicugna_genes()
    m = get_fixture("vicugna_pe").model
    dev.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
    dev.set_gene_map(gmap, len(names))
    X = np.random.default_rng(1).lognormal(0.0, 3.0, size=(3, m.n_tx)) * (np.random.default_rng(2).random((3, m.n_tx)) < 0.8)
    got = dev.gene_sums(X)
    assert got.shape == (3, len(names))
    assert np.array_equal(got, chunked_sums(X, gmap, len(names)))
    assert np.array_equal(dev.gene_sums(X[1]), got[1])
    alone = np.nonzero((np.bincount(gmap) == 1)[gmap])[0]           # transcripts that are their gene's only one
    assert np.array_equal(got[:, gmap[alone]], X[:, alone])          # such a gene's sum is that transcript's value


@pytest.mark.parametrize("renumber", ["2", "0"])
def test_gene_sums_same_bits_across_layouts_and_numbering(renumber, monkeypatch):
    monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
    m, gmap, ng = family_problem()
    X = np.random.default_rng(7).lognormal(0.0, 2.0, size=(5, m.n_tx))
    want = chunked_sums(X, gmap, ng)
    assert (np.bincount(gmap[gmap >= 0], minlength=ng) >= 1000).any() and want[:, -1].tolist() == [0.0] * 5
    with EmsarHip(0) as d:
        for layout, merge in ((hip.LAYOUT_TILED, False), (hip.LAYOUT_TILED, True), (hip.LAYOUT_CSR, False)):
            d.upload_structure(m.n_tx, m.row_ptr, m.col_idx, layout=layout, merge_rows=merge)
            if layout == hip.LAYOUT_TILED:
                assert d.info()["renumbered"] == int(renumber == "2")
            d.set_gene_map(gmap, ng)
            assert np.array_equal(d.gene_sums(X), want), (layout, merge)


def _boot_case(d, name):
    if name == "vicugna_pe":
        m = get_fixture("vicugna_pe").model
        names, gmap = vicugna_genes()
        ng = len(names)
    else:
        m, gmap, ng = family_problem(5)
    d.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
    d.upload_sample(m.R, m.E, None)
    d.set_gene_map(gmap, ng)
    return m, gmap, ng


@pytest.mark.parametrize("set_mode", [0, 1], ids=["sets", "streaming"])
@pytest.mark.parametrize("name", ["vicugna_pe", "family"])
def test_bootstrap_genes(name, set_mode, monkeypatch):
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        m, gmap, ng = _boot_case(d, name)
        B, seed = 12, 21
        r = d.bootstrap_genes(B, seed, want_replicates=True, set_mode=set_mode, **SOLVE)
        mean, sd, tsd, reps, st = d.bootstrap(B, seed, want_replicates=True, set_mode=set_mode, **SOLVE)
        # the transcript outputs are bootstrap()'s bits
        for a, b in ((r["fpkm_mean"], mean), (r["fpkm_sd"], sd), (r["tpm_sd"], tsd), (r["replicates"], reps)):
            assert np.array_equal(a, b)
        # the gene statistics are those of the replicates' gene sums, in the documented order
        G = chunked_sums(reps, gmap, ng)
        S = reps.sum(axis=1)
        gm, gs = welford(G)
        _, gts = welford(np.where(S[:, None] > 0, G * 1e6 / S[:, None], 0.0))
        for got, want in ((r["gene_fpkm_mean"], gm), (r["gene_fpkm_sd"], gs), (r["gene_tpm_sd"], gts)):
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-300), name
        assert np.all(np.abs(r["gene_fpkm_mean"] - G.mean(axis=0)) <= 1e-12 * np.abs(G.mean(axis=0)) + 1e-300)
        assert r["gene_fpkm_sd"].max() > 0 and r["stats"].reduce_ms > 0
        # and do not depend on the batch size
        for batch in ("1", "7"):
            monkeypatch.setenv("EMSAR_HIP_BOOT_BATCH", batch)
            rb = d.bootstrap_genes(B, seed, want_replicates=True, set_mode=set_mode, **SOLVE)
            assert rb["stats"].batch == int(batch)
            for k in ("fpkm_mean", "fpkm_sd", "tpm_sd", "replicates", "gene_fpkm_mean", "gene_fpkm_sd", "gene_tpm_sd"):
                assert np.array_equal(rb[k], r[k]), (name, batch, k)
        monkeypatch.delenv("EMSAR_HIP_BOOT_BATCH")


def test_isoforms_covary_negatively_on_vicugna(dev):
    names, gmap = vicugna_genes()
    m = get_fixture("vicugna_pe").model
    dev.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
    dev.upload_sample(m.R, m.E, None)
    dev.set_gene_map(gmap, len(names))
    r = dev.bootstrap_genes(20, 1, **SOLVE)
    multi = np.nonzero(np.bincount(gmap) >= 2)[0]
    var_gene = r["gene_fpkm_sd"][multi] ** 2
    var_naive = np.array([(r["fpkm_sd"][gmap == g] ** 2).sum() for g in multi])
    for g, a, b in zip(multi, var_gene, var_naive):
        print("%s  n_iso=%d  var(gene)=%.6g  sum var(isoforms)=%.6g" % (names[g], (gmap == g).sum(), a, b))
    assert var_gene.sum() < var_naive.sum()


def test_errors():
    with EmsarHip(0) as d:
        with pytest.raises(hip.EmsarHipError) as e:
            d.set_gene_map([0, 0, 0], 1)                      # before upload_structure
        assert e.value.status == -5
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        with pytest.raises(hip.EmsarHipError) as e:
            d.gene_sums(np.ones(3))                           # no map
        assert e.value.status == -5
        for bad, ng in (([0, 1, 2], 2), ([0, -2, 0], 1), ([0, 0, 0], 0)):
            with pytest.raises(hip.EmsarHipError) as e:
                d.set_gene_map(bad, ng)
            assert e.value.status == -1
        d.set_gene_map([1, -1, 1], 2)
        assert np.array_equal(d.gene_sums(np.array([1.0, 2.0, 4.0])), [0.0, 5.0])
        d.upload_sample([1, 2, 3], None, None)
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap_genes(0, 1)
        assert e.value.status == -1
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])       # drops the map
        d.upload_sample([1, 2, 3], None, None)
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap_genes(2, 1)
        assert e.value.status == -5
        with pytest.raises(hip.EmsarHipError) as e:
            d.gene_sums(np.ones(3))
        assert e.value.status == -5


# ---- the command-line driver ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


def _run(out, extra, aln=None, check=True):
    fx = get_fixture("vicugna_pe")
    cmd = [CLI, "-q", "-g"] + fx.meta["opts"] + extra + ["-I", os.path.join(VIC, "index.rsh"), str(out), "out", aln or aln_path(VIC)[0]]
    return subprocess.run(cmd, check=check, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_cli_g2t_bootstrap(tmp_path, _built):
    g2t = os.path.join(VIC, "genes.g2t.gz")
    _run(tmp_path / "a", ["--bootstrap", "20"])
    _run(tmp_path / "b", ["--bootstrap", "20", "--g2t", g2t])
    a, b = tmp_path / "a", tmp_path / "b"
    for ext in ("fpkm", "fraglength_effect", "segments", "bootstrap"):
        assert open(a / ("out.0." + ext), "rb").read() == open(b / ("out.0." + ext), "rb").read(), ext
    assert not (a / "out.0.gfpkm").exists() and not (a / "out.0.gbootstrap").exists()
    names, gmap = vicugna_genes()
    n_iso = np.bincount(gmap)
    got = read_gfpkm(str(b / "out.0.gfpkm"))
    assert list(got) == names
    # FPKM2gFPKM.pl's rules on our own .fpkm: the script sums the printed values, we print the sums (one more print quantum)
    tx, cols = fpkm_columns(str(b / "out.0.fpkm"))
    perl = np.zeros((len(names), 3))
    for t in range(len(tx)):
        perl[gmap[t]] += cols[t]
    for k, g in enumerate(names):
        for j, c in ((0, 0), (1, 1), (2, 3)):
            assert abs(got[g][c] - perl[k, j]) <= (n_iso[k] + 1) * 5e-7 + 1e-9 * abs(perl[k, j]), (g, c)
    # against the reference's gene step on the reference's .fpkm: the transcript parity criteria (tests/conftest.py), summed per gene,
    # wherever the reference agrees with itself on every isoform
    fx = get_fixture("vicugna_pe")
    ref = read_gfpkm(os.path.join(VIC, "ref.run0.gfpkm.gz"))
    assert set(ref) == set(got)
    noisy = np.bincount(gmap, weights=fx.noise_mask().astype(float), minlength=len(names)) > 0
    checked = 0
    for k, g in enumerate(names):
        if noisy[k]:
            continue
        checked += 1
        assert abs(got[g][0] - ref[g][0]) <= 1e-5 * abs(ref[g][0]) + n_iso[k] * 2.5e-6, (g, got[g], ref[g])
        assert abs(got[g][1] - ref[g][1]) <= 1e-5 * abs(ref[g][1]) + n_iso[k] * 2e-3, (g, got[g], ref[g])
    assert checked > 0.9 * len(names)
    # .gbootstrap: a one-transcript gene's row is its transcript's .bootstrap row; FPKM as in .gfpkm
    brows = {l.split("\t")[0]: l.split("\t")[1:] for l in open(b / "out.0.bootstrap").read().splitlines()[1:]}
    glines = open(b / "out.0.gbootstrap").read().splitlines()
    assert glines[0] == "geneID\tFPKM\tboot.mean.FPKM\tboot.sd.FPKM\tTPM\tboot.sd.TPM"
    grows = [l.split("\t") for l in glines[1:]]
    assert [r[0] for r in grows] == names
    gf = [l.split("\t") for l in open(b / "out.0.gfpkm").read().splitlines()[1:]]
    assert [r[1] for r in gf] == [r[1] for r in grows] and [r[4] for r in gf] == [r[4] for r in grows]
    for k, r in enumerate(grows):
        if n_iso[k] == 1:
            t = int(np.nonzero(gmap == k)[0][0])
            assert r[1:] == brows[tx[t]], (names[k], r, brows[tx[t]])
    assert max(float(r[3]) for r in grows) > 0


def test_cli_g2t_multisample_and_bad_map(tmp_path, _built):
    g2t = os.path.join(VIC, "genes.g2t.gz")
    lst = tmp_path / "list.txt"
    a = aln_path(VIC)[0]
    lst.write_text(a + "\n" + a + "\n")
    out = tmp_path / "m"
    fx = get_fixture("vicugna_pe")
    cmd = [CLI, "-q", "-M", "--gpus", "1", "--g2t", g2t] + fx.meta["opts"] + ["-I", os.path.join(VIC, "index.rsh"), str(out), "out", str(lst)]
    subprocess.run(cmd, check=True, timeout=600)
    g0, g1 = open(out / "out.0.gfpkm").read(), open(out / "out.1.gfpkm").read()
    assert g0 == g1 and len(g0.splitlines()) == 12664
    # a g2t without a single gene/transcript line: an error before any sample is solved
    bad = tmp_path / "bad.g2t"
    bad.write_text("no tabs here\n")
    r = _run(tmp_path / "x", ["--g2t", str(bad)], check=False)
    assert r.returncode != 0 and b"g2t" in r.stderr
    assert not (tmp_path / "x" / "out.0.fpkm").exists()
    r = _run(tmp_path / "y", ["--g2t", str(tmp_path / "missing.g2t")], check=False)
    assert r.returncode != 0 and not (tmp_path / "y" / "out.0.fpkm").exists()
