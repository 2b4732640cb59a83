"""CPU: the isoform usage's definition (include/emsar_hip.h "isoform usage") -- emsar_hip_isoform_usage_host against a numpy restatement
bit for bit (gene sums in the documented chunked order, one division, first maximum on the tid-sorted list), its exact properties and
argument errors, the ABI struct and symbols, the .isoforms writer byte for byte and the CLI's argument check -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from emsar_amd import _build, hip, hostlib
from tests.test_genes_gpu import chunked_sums, family_problem


def restated(X, gene_of_tx, n_genes):
    """The definition in numpy: gene sums by chunked_sums, one division per transcript, np.argmax (the first maximum) over the gene's
    transcripts in ascending tid."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    G = chunked_sums(X, gene_of_tx, n_genes)
    Gt = G[:, np.maximum(gene_of_tx, 0)]
    ok = (gene_of_tx >= 0)[None, :] & (Gt > 0)
    usage = np.where(ok, X / np.where(ok, Gt, 1.0), 0.0)
    dom = np.full((X.shape[0], n_genes), -1, dtype=np.int32)
    order = np.argsort(gene_of_tx, kind="stable")                      # stable: ascending tid inside a gene
    starts = np.searchsorted(gene_of_tx[order], np.arange(n_genes + 1))
    for g in range(n_genes):
        idx = order[starts[g]:starts[g + 1]]
        if len(idx):
            dom[:, g] = np.where(G[:, g] > 0, idx[np.argmax(X[:, idx], axis=1)], -1)
    return usage, dom, G


def members(gene_of_tx, g):
    return np.nonzero(gene_of_tx == g)[0]


def tie_columns(gene_of_tx, n_genes, seed=0):
    """Columns full of equal maxima for any map: all ones (every gene ties, across its chunk boundaries too), small integers (ties
    and zeros), zeros except two equal values at the end of every gene's first chunk and the start of its second (positions 255 and
    256; the last two transcripts of a smaller gene; a tie between zeros in front of them), and all zeros."""
    n = len(gene_of_tx)
    rng = np.random.default_rng(seed)
    pair = np.zeros(n)
    for g in range(n_genes):
        idx = members(gene_of_tx, g)
        if len(idx) >= 257:
            pair[idx[255:257]] = 3.5
        elif len(idx) >= 2:
            pair[idx[-2:]] = 3.5
        elif len(idx) == 1:
            pair[idx] = 3.5
    return np.stack([np.ones(n), rng.integers(0, 3, n).astype(np.float64), pair, np.zeros(n)])


def lognormal_columns(n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.lognormal(0.0, 2.0, size=(k, n)) * (rng.random((k, n)) >= 0.2)


def small_problem(seed=4):
    """genes of 256, 257 and 300 transcripts, an all-zero gene, hand-made ties, a lone transcript, an empty gene and five transcripts
    in no gene, the tids dealt at random -> (gene_of_tx, n_genes, X [3 + 4][n_tx], the genes by name)"""
    sizes = {"g256": 256, "g257": 257, "g300": 300, "zero": 5, "two": 4, "three": 5, "zeros_tie": 4, "lone": 1, "empty": 0}
    names = list(sizes)
    gene_of_tx = np.concatenate([np.full(k, g, dtype=np.int32) for g, k in enumerate(sizes.values())] + [np.full(5, -1, dtype=np.int32)])
    gene_of_tx = gene_of_tx[np.random.default_rng(seed).permutation(len(gene_of_tx))]
    gid = {nm: g for g, nm in enumerate(names)}
    X = lognormal_columns(len(gene_of_tx), 3, seed + 1)
    X[:, members(gene_of_tx, gid["lone"])] = [[0.75], [1e-300], [3e300]]
    X[:, members(gene_of_tx, gid["zero"])] = 0.0
    X[:, members(gene_of_tx, gid["two"])] = [4.0, 7.0, 7.0, 1.0]                       # two equal positive maxima
    X[:, members(gene_of_tx, gid["three"])] = [2.0, 9.0, 9.0, 9.0, 0.0]                 # three
    X[:, members(gene_of_tx, gid["zeros_tie"])] = [0.0, 0.0, 2.5, 0.0]                  # zeros tie, the sum is positive
    big = members(gene_of_tx, gid["g300"])
    X[0, big] = np.minimum(X[0, big], 50.0)
    X[0, big[255:257]] = 60.0                                                           # a tie across the chunk boundary
    X[1, big[256]] = X[1, big].max() * 2                                                # the maximum in the second chunk alone
    return gene_of_tx, len(names), np.vstack([X, tie_columns(gene_of_tx, len(names))]), gid


def check_properties(X, gene_of_tx, n_genes, usage, dom, G):
    assert np.all(usage >= 0.0) and np.all(usage <= 1.0)
    assert not usage[:, gene_of_tx < 0].any()
    n_iso = np.bincount(gene_of_tx[gene_of_tx >= 0], minlength=n_genes)
    lone = np.nonzero((gene_of_tx >= 0) & (n_iso[np.maximum(gene_of_tx, 0)] == 1))[0]
    assert len(lone) > 0
    assert np.array_equal(usage[:, lone], (X[:, lone] > 0).astype(np.float64))          # exactly 1.0, or 0.0 for x == 0
    assert np.array_equal(dom == -1, ~(G > 0))
    for c in range(X.shape[0]):
        has = np.nonzero(dom[c] >= 0)[0]
        assert np.array_equal(gene_of_tx[dom[c, has]], has)                             # a transcript of its own gene
        assert np.all(X[c, dom[c, has]] > 0)


@pytest.fixture(scope="module")
def family():
    m, gene_of_tx, n_genes = family_problem()
    X = np.vstack([lognormal_columns(m.n_tx, 5, 7), tie_columns(gene_of_tx, n_genes)])
    return gene_of_tx, n_genes, X


def test_host_equals_the_restatement_on_the_family_map(family):
    gene_of_tx, n_genes, X = family
    n_iso = np.bincount(gene_of_tx[gene_of_tx >= 0], minlength=n_genes)
    assert n_iso.max() >= 1000 and n_iso.min() == 0 and (n_iso == 1).any() and (gene_of_tx < 0).sum() == 20
    usage, dom = hip.isoform_usage_host(gene_of_tx, n_genes, X, want_dominant=True)
    want_u, want_d, G = restated(X, gene_of_tx, n_genes)
    assert usage.shape == X.shape and dom.shape == (len(X), n_genes) and dom.dtype == np.int32
    assert np.array_equal(usage, want_u) and np.array_equal(dom, want_d)
    check_properties(X, gene_of_tx, n_genes, usage, dom, G)
    assert np.array_equal(hip.isoform_usage_host(gene_of_tx, n_genes, X), usage)         # without the dominant isoforms
    u1, d1 = hip.isoform_usage_host(gene_of_tx, n_genes, X[2], want_dominant=True)     # a single column
    assert np.array_equal(u1, usage[2]) and np.array_equal(d1, dom[2])


def test_host_equals_the_restatement_on_the_small_map():
    gene_of_tx, n_genes, X, gid = small_problem()
    usage, dom = hip.isoform_usage_host(gene_of_tx, n_genes, X, want_dominant=True)
    want_u, want_d, G = restated(X, gene_of_tx, n_genes)
    assert np.array_equal(usage, want_u) and np.array_equal(dom, want_d)
    check_properties(X, gene_of_tx, n_genes, usage, dom, G)
    m = lambda nm: members(gene_of_tx, gid[nm])
    # the smallest tid among equal maxima
    assert (dom[:3, gid["two"]] == m("two")[1]).all() and (dom[:3, gid["three"]] == m("three")[1]).all()
    assert (dom[:3, gid["zeros_tie"]] == m("zeros_tie")[2]).all() and np.array_equal(usage[0, m("zeros_tie")], [0.0, 0.0, 1.0, 0.0])
    assert dom[0, gid["g300"]] == m("g300")[255] and dom[1, gid["g300"]] == m("g300")[256]
    assert (dom[:3, gid["zero"]] == -1).all() and (dom[:, gid["empty"]] == -1).all() and not usage[:3, m("zero")].any()
    ones, pair, zeros = 3, 5, 6                                                          # rows of tie_columns behind the three columns
    for nm in ("g256", "g257", "g300", "two", "lone"):
        assert dom[ones, gid[nm]] == m(nm)[0], nm                                        # all equal: the first tid
    assert dom[pair, gid["g256"]] == m("g256")[254] and dom[pair, gid["g257"]] == m("g257")[255] and dom[pair, gid["g300"]] == m("g300")[255]
    assert (dom[zeros] == -1).all() and not usage[zeros].any()


def test_scaling_a_column_changes_nothing(family):
    gene_of_tx, n_genes, X = family
    for gmap, ng, cols in ((gene_of_tx, n_genes, X), small_problem()[:3]):
        cols = np.minimum(cols, 1e300)
        a = hip.isoform_usage_host(gmap, ng, cols, want_dominant=True)
        b = hip.isoform_usage_host(gmap, ng, 2.0 * cols, want_dominant=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_argument_errors():
    L = hip.load_library()
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    gmap = np.array([0, 1, -1, 1], dtype=np.int32)
    x = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]])
    u, d = np.zeros((2, 4)), np.zeros((2, 2), dtype=np.int32)
    call = lambda n_tx, ng, g, nc, v, uo, do: L.emsar_hip_isoform_usage_host(
        n_tx, ng, None if g is None else g.ctypes.data_as(i32p), nc, None if v is None else v.ctypes.data_as(f64p),
        None if uo is None else uo.ctypes.data_as(f64p), None if do is None else do.ctypes.data_as(i32p))
    assert call(4, 2, gmap, 2, x, u, d) == 0 and call(4, 2, gmap, 2, x, u, None) == 0
    assert np.array_equal(u, [[1.0, 1.0 / 3.0, 0.0, 2.0 / 3.0], [0.0] * 4]) and np.array_equal(d, [[0, 3], [-1, -1]])
    assert call(4, 0, gmap, 2, x, u, d) == -1 and call(-1, 2, gmap, 2, x, u, d) == -1
    assert call(4, 2, None, 2, x, u, d) == -1 and call(4, 2, gmap, 0, x, u, d) == -1
    assert call(4, 2, gmap, 2, None, u, d) == -1 and call(4, 2, gmap, 2, x, None, d) == -1
    for bad in ([0, 2, -1, 1], [0, -2, -1, 1]):
        assert call(4, 2, np.array(bad, dtype=np.int32), 2, x, u, d) == -1
    for bad in (-1e-300, float("nan"), float("inf"), -float("inf")):
        y = x.copy()
        y[1, 2] = bad                                                                   # a transcript in no gene is checked as well
        assert call(4, 2, gmap, 2, y, u, d) == -1, bad
        with pytest.raises(hip.EmsarHipError) as e:
            hip.isoform_usage_host(gmap, 2, y)
        assert e.value.status == -1
    assert call(4, 2, gmap, 1, np.array([0.0, -0.0, 0.0, 5.0]), u, d) == 0               # -0.0 is a zero


def test_abi_struct_and_symbols():
    hdr = open(os.path.join(os.path.dirname(_build.PKG), "include", "emsar_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} emsar_isoform_outputs;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [nm.strip().lstrip("*") for decl in body.split(";") if decl.strip() for nm in decl.strip().split(None, 1)[1].split(",")]
    assert [f for f, _ in hip.IsoformOutputs._fields_] == fields == ["usage_mean", "usage_sd", "dominant_count", "usage_q"]
    assert C.sizeof(hip.IsoformOutputs) == 4 * C.sizeof(C.c_void_p) == 32
    # additions only: the existing structs keep their size
    assert C.sizeof(hip.BootStats) == 64 and C.sizeof(hip.QuantileStats) == 24
    L = hip.load_library()
    for name in ("emsar_hip_isoform_usage", "emsar_hip_isoform_usage_host", "emsar_hip_bootstrap_isoforms"):
        assert name in hip.SYMBOLS and hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name


def test_writer_byte_for_byte(tmp_path):
    _build.build_all()
    tx = ["tA", "tB", "tC", "tD", "tE"]
    genes = ["g1", "", "g3"]
    gmap = [0, 2, -1, 0, 1]                                            # tC is in no gene: no line
    fpkm = [1.5, 0.0, 9.0, 4.5, 2.25]
    usage = [0.25, 0.0, 0.0, 0.75, 1.0]
    dom = [3, 4, -1]
    head = "transcript_ID\tgene_ID\tFPKM\tusage\tdominant"
    base = [("tA", "g1", "1.500000", "0.250000", "0"), ("tB", "g3", "0.000000", "0.000000", "0"), ("tD", "g1", "4.500000", "0.750000", "1"),
            ("tE", "", "2.250000", "1.000000", "1")]
    p = str(tmp_path / "a.isoforms")
    hostlib.write_isoforms(p, tx, genes, gmap, fpkm, usage, dom)
    assert open(p, "rb").read() == (head + "\n" + "".join("\t".join(r) + "\n" for r in base)).encode()
    mean, sd, cnt = [0.3, 0.0, 0.0, 0.7, 1.0], [0.125, 0.0, 0.0, 0.125, 0.0], [1, 0, 0, 7, 8]
    boot = [("0.300000", "0.125000", "0.125000"), ("0.000000", "0.000000", "0.000000"), ("0.700000", "0.125000", "0.875000"),
            ("1.000000", "0.000000", "1.000000")]
    hostlib.write_isoforms(p, tx, genes, gmap, fpkm, usage, dom, n_boot=8, usage_mean=mean, usage_sd=sd, dominant_count=cnt)
    want = head + "\tusage_mean\tusage_sd\tdominant_freq\n" + "".join("\t".join(r + b) + "\n" for r, b in zip(base, boot))
    assert open(p, "rb").read() == want.encode()
    uq = [[0.1, 0.0, 0.5, 0.6, 1.0], [0.4, 0.0, 0.5, 0.9, 1.0]]
    quant = [("0.100000", "0.400000"), ("0.000000", "0.000000"), ("0.600000", "0.900000"), ("1.000000", "1.000000")]
    hostlib.write_isoforms(p, tx, genes, gmap, fpkm, usage, dom, n_boot=8, usage_mean=mean, usage_sd=sd, dominant_count=cnt, q=[0.025, 0.5],
                           usage_q=uq)
    want = head + "\tusage_mean\tusage_sd\tdominant_freq\tusage_q0.025000000000000001\tusage_q0.5\n" + "".join(
        "\t".join(r + b + k) + "\n" for r, b, k in zip(base, boot, quant))
    assert open(p, "rb").read() == want.encode()


def _cli(args, tmp_path):
    _build.build_all()
    return subprocess.run([_build.CLI] + args + ["-P", "-I", str(tmp_path / "none.rsh"), str(tmp_path), "out", "none.bowtie"],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


@pytest.mark.parametrize("extra", [[], ["--bootstrap", "10"], ["--bootstrap", "10", "--bootstrap-quantiles", "0.5"]])
def test_cli_isoforms_need_a_gene_map(extra, tmp_path):
    r = _cli(["--isoforms"] + extra, tmp_path)
    assert r.returncode == 1
    assert "--isoforms needs --g2t" in r.stderr and "rsh" not in r.stderr              # before any input is opened
    assert not os.listdir(str(tmp_path))
    # with a map the pair gets as far as the index
    r = _cli(["--isoforms", "--g2t", str(tmp_path / "none.g2t")] + extra, tmp_path)
    assert r.returncode != 0 and "--isoforms" not in r.stderr


def test_cli_help_lists_the_flag(tmp_path):
    r = _cli(["--help"], tmp_path)
    assert "--isoforms" in r.stderr and "--g2t" in r.stderr
