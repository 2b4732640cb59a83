"""GPU: bootstrap quantiles (emsar_hip_bootstrap_quantiles) -- every quantile against quantiles_host of the call's own replicates bit
for bit (transcripts and genes, FPKM and TPM), the other outputs against bootstrap_genes, invariance under batching (fresh child
processes) and numbering, no side effects on the context, errors, and the CLI's .bootq / .gbootq files."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from emsar_amd import EmsarHip, _build, hip
from tests.conftest import aln_path, get_fixture
from tests.test_bootstrap_gpu import CLI, SOLVE, _family, _run_cli
from tests.test_genes_gpu import vicugna_genes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = [0.0, 0.025, 0.5, 0.975, 1.0]
CASES = [("vicugna_pe", 20, 0), ("vicugna_pe", 20, 1), ("syn300_se", 20, 0), ("syn300_se", 20, 1), ("toy5_pe", 7, 0), ("toy5_pe", 7, 1)]
STATS = ("fpkm_mean", "fpkm_sd", "tpm_sd", "replicates", "gene_fpkm_mean", "gene_fpkm_sd", "gene_tpm_sd")
QUANT = ("fpkm_q", "tpm_q", "gene_fpkm_q", "gene_tpm_q")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def gene_map(case, n_tx):
    """vicugna_pe: its g2t file.  The others: genes of 1, 2, 3, 1, 2, 3, .. neighbouring transcripts, every 11th transcript in no gene,
    and one gene without transcripts."""
    if case == "vicugna_pe":
        names, gmap = vicugna_genes()
        return np.asarray(gmap, dtype=np.int32), len(names)
    gmap = np.zeros(n_tx, dtype=np.int32)
    g = t = 0
    while t < n_tx:
        k = 1 + g % 3
        gmap[t:t + k] = g
        t += k
        g += 1
    gmap[5::11] = -1
    return gmap, g + 1


def host_den(m):
    """den_t = sum_c m_ct E_c added in row order on the host, as emsar-hip does: the device's own scatter adds with floating atomics,
    whose order -- and with it the last bits of den and of every theta -- changes from one context or process to the next"""
    rp = m.row_ptr.astype(np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    E = np.asarray(m.E, dtype=np.float64)
    keep = E[rows] != 0.0
    den = np.zeros(m.n_tx)
    np.add.at(den, np.asarray(m.col_idx)[keep], E[rows][keep])
    return den


def setup(d, case):
    m = get_fixture(case).model
    gmap, ng = gene_map(case, m.n_tx)
    d.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
    d.upload_sample(m.R, m.E, host_den(m))
    d.set_gene_map(gmap, ng)
    return m, gmap, ng


def tpm_of(x, S):
    """k_boot_accum's expression on rows x[b] with the returned denominators: S_b > 0 ? x_b * 1e6 / S_b : 0"""
    safe = np.where(S > 0, S, 1.0)[:, None]
    return np.where(S[:, None] > 0, x * 1e6 / safe, 0.0)


def check_against_host(d, r, gmap, ng, what):
    """the four quantile outputs are the library's definition applied to the call's own replicates and sums"""
    reps, S = r["replicates"], r["replicate_sums"]
    assert np.allclose(S, reps.sum(axis=1), rtol=1e-12, atol=0), what
    assert same(r["fpkm_q"], hip.quantiles_host(reps, Q)), what
    assert same(r["tpm_q"], hip.quantiles_host(tpm_of(reps, S), Q)), what
    G = d.gene_sums(reps)
    assert same(r["gene_fpkm_q"], hip.quantiles_host(G, Q)), what
    assert same(r["gene_tpm_q"], hip.quantiles_host(tpm_of(G, S), Q)), what
    # a one-transcript gene's quantiles are its transcript's
    alone = np.nonzero((np.bincount(gmap[gmap >= 0], minlength=ng) == 1)[np.maximum(gmap, 0)] & (gmap >= 0))[0]
    assert len(alone) > 0
    assert same(r["gene_fpkm_q"][:, gmap[alone]], r["fpkm_q"][:, alone]) and same(r["gene_tpm_q"][:, gmap[alone]], r["tpm_q"][:, alone]), what
    # sanity: ordered in q, and with q = 0 and 1 every replicate lies inside
    for key, vals in (("fpkm_q", reps), ("tpm_q", tpm_of(reps, S)), ("gene_fpkm_q", G), ("gene_tpm_q", tpm_of(G, S))):
        assert np.all(np.diff(r[key], axis=0) >= 0), (what, key)
        assert np.all(vals >= r[key][0]) and np.all(vals <= r[key][-1]), (what, key)
    assert np.all(r["fpkm_q"][1] <= r["fpkm_q"][2]) and np.all(r["fpkm_q"][2] <= r["fpkm_q"][3])


@pytest.mark.parametrize("case,B,set_mode", CASES, ids=["%s-B%d-mode%d" % c for c in CASES])
def test_quantiles_are_those_of_the_replicates(case, B, set_mode):
    with EmsarHip(0) as d:
        d.set_deterministic(True)          # set_mode 1: two calls then give the same replicates, so the calls below can be compared
        m, gmap, ng = setup(d, case)
        th0, _ = d.solve(set_mode=set_mode, **SOLVE)
        r = d.bootstrap_quantiles(B, Q, 21, want_replicates=True, want_genes=True, set_mode=set_mode, **SOLVE)
        assert r["qstats"].n_quantiles == len(Q) and r["qstats"].held_bytes == 8 * B * (m.n_tx + 1 + ng) and r["qstats"].quantile_ms > 0
        assert r["stats"].n_replicates == B
        check_against_host(d, r, gmap, ng, (case, set_mode))
        assert r["fpkm_q"][-1].max() > 0 and (r["fpkm_q"][-1] > r["fpkm_q"][0]).any()
        # mean, sd and replicates are bootstrap_genes' bits
        g = d.bootstrap_genes(B, 21, want_replicates=True, set_mode=set_mode, **SOLVE)
        for k in STATS:
            assert same(r[k], g[k]), (case, k)
        # without gene outputs and without replicates: the same transcript outputs
        plain = d.bootstrap_quantiles(B, Q, 21, set_mode=set_mode, **SOLVE)
        assert plain["replicates"] is None and "gene_fpkm_q" not in plain
        for k in ("fpkm_mean", "fpkm_sd", "tpm_sd", "fpkm_q", "tpm_q", "replicate_sums"):
            assert same(plain[k], r[k]), (case, k)
        # a window of replicates, other probabilities, a single q
        w = d.bootstrap_quantiles(3, [0.3], 21, first=4, want_replicates=True, set_mode=set_mode, **SOLVE)
        assert same(w["replicates"], r["replicates"][4:7])
        assert same(w["fpkm_q"], hip.quantiles_host(w["replicates"], [0.3]))
        one = d.bootstrap_quantiles(1, Q, 21, want_replicates=True, set_mode=set_mode, **SOLVE)
        assert same(one["fpkm_q"], np.repeat(one["replicates"], len(Q), axis=0))
        # the context is as it was
        th1, _ = d.solve(set_mode=set_mode, **SOLVE)
        assert same(th0, th1), case


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from emsar_amd import EmsarHip
from tests.test_bootq_gpu import Q, SOLVE, QUANT, STATS, setup
out = {}
with EmsarHip(0) as d:
    d.set_deterministic(True)
    setup(d, sys.argv[2])
    for set_mode in (0, 1):
        r = d.bootstrap_quantiles(int(sys.argv[3]), Q, 5, want_replicates=True, want_genes=True, set_mode=set_mode, **SOLVE)
        for k in QUANT + STATS + ("replicate_sums",):
            out["%s_%d" % (k, set_mode)] = r[k]
        out["batch_%d" % set_mode] = np.array([r["stats"].batch])
np.savez(sys.argv[4], **out)
"""


@pytest.mark.parametrize("case,B", [("vicugna_pe", 20), ("syn300_se", 20), ("toy5_pe", 7)])
def test_batch_invariance(case, B, tmp_path):
    """EMSAR_HIP_BOOT_BATCH = 1, 3 and unset, each in a fresh process: the same bits in every output."""
    res = {}
    for batch in ("1", "3", None):
        env = {k: v for k, v in os.environ.items() if k != "EMSAR_HIP_BOOT_BATCH"}
        if batch:
            env["EMSAR_HIP_BOOT_BATCH"] = batch
        path = str(tmp_path / ("b%s.npz" % batch))
        subprocess.run([sys.executable, "-c", CHILD, ROOT, case, str(B), path], check=True, timeout=600, env=env, cwd=ROOT)
        res[batch] = dict(np.load(path))
    for set_mode in (0, 1):
        assert res["1"]["batch_%d" % set_mode][0] == 1 and res["3"]["batch_%d" % set_mode][0] == 3
        assert res[None]["batch_%d" % set_mode][0] == B
    for batch in ("1", "3"):
        for k, v in res[None].items():
            if not k.startswith("batch_"):
                assert same(res[batch][k], v), (case, batch, k)


@pytest.mark.parametrize("case,B", [("family", 20), ("vicugna_pe", 20), ("syn300_se", 20), ("toy5_pe", 7)])
def test_numbering_invariance(case, B, monkeypatch):
    """The library's own transcript numbering forced on and off: every output of the call is the same bits.  (The resident sets are
    solved in the caller's order whatever the numbering, and den is given by the caller, so the replicates are the same bits; the
    quantile stage adds its TPM denominators in the caller's order too, k_quant_sums.  The sd of TPM keeps k_boot_sums' library-order
    denominators, as in bootstrap(), and is not compared here.)"""
    if case == "family":
        m = _family(6)
        gmap = (np.arange(m.n_tx) // 3).astype(np.int32)
        gmap[7::13] = -1
        gmap[1:3] = -1                               # gene 0 keeps one transcript
        ng = int(gmap.max()) + 1
    else:
        m = get_fixture(case).model
        gmap, ng = gene_map(case, m.n_tx)
    res = []
    for renumber in ("2", "0"):
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
        with EmsarHip(0) as d:
            d.set_deterministic(True)
            d.upload_structure(m.n_tx, m.row_ptr, m.col_idx, layout=hip.LAYOUT_TILED)
            if renumber == "0":
                assert d.info()["renumbered"] == 0
            elif m.n_tx >= 100:                      # (the five transcripts of toy5_pe leave the library nothing to renumber)
                assert d.info()["renumbered"] == 1
            d.upload_sample(m.R, m.E, host_den(m))
            d.set_gene_map(gmap, ng)
            r = d.bootstrap_quantiles(B, Q, 3, want_replicates=True, want_genes=True, **SOLVE)
            check_against_host(d, r, gmap, ng, (case, renumber))
            res.append(r)
    a, b = res
    for k in ("replicates", "replicate_sums", "fpkm_mean", "fpkm_sd", "gene_fpkm_mean", "gene_fpkm_sd") + QUANT:
        assert same(a[k], b[k]), (case, k)


def test_memory_rule():
    """Held replicates beyond half of the free device memory: ERR_OOM at once, and the context still works.  4096 replicates of 6.3 M
    transcripts are 206 GB, more than half of any free memory of a 288 GB card."""
    n_tx = 6 << 20
    with EmsarHip(0) as d:
        d.upload_structure(n_tx, [0, 1, 2, 3], [0, 1, n_tx - 1], layout=hip.LAYOUT_CSR)
        d.upload_sample([1, 2, 3], None, None)
        assert _call(d, 4096, [0.5], (1, 1, 1, 1, 1), (0, 0, 0, 0, 0)) == -3
        r = d.bootstrap_quantiles(3, [0.0, 1.0], 1, want_replicates=True)
        assert same(r["fpkm_q"], np.stack([r["replicates"].min(axis=0), r["replicates"].max(axis=0)]))


def _call(d, n, q, outs, genes, first=0):
    """the C entry point itself: outs / genes = which of the five transcript / gene outputs are given"""
    T, G, K = d.n_tx, max(d.n_genes, 1), max(len(q), 1)
    f64p = C.POINTER(C.c_double)
    qa = np.ascontiguousarray(q, dtype=np.float64)
    p = hip.EmParams(100000, 1, 1e-10, 1e-6, 8, 0, 0.0, 0.0, 0.0, 0, 0)
    held = []

    def buf(given, size):
        if not given:
            return None
        held.append(np.zeros(size))
        return held[-1].ctypes.data_as(f64p)

    return d._L.emsar_hip_bootstrap_quantiles(
        d._h, C.byref(p), 1, first, n, len(q), qa.ctypes.data_as(f64p) if len(q) else None,
        buf(outs[0], T), buf(outs[1], T), buf(outs[2], T), None, None, buf(outs[3], K * T), buf(outs[4], K * T),
        buf(genes[0], G), buf(genes[1], G), buf(genes[2], G), buf(genes[3], K * G), buf(genes[4], K * G), None, None)


def test_errors():
    ALL, NONE = (1, 1, 1, 1, 1), (0, 0, 0, 0, 0)
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        assert _call(d, 5, [0.5], ALL, NONE) == -5                       # before upload_sample
        d.upload_sample([1, 2, 3], None, None)
        assert _call(d, 5, [0.5], ALL, NONE) == 0
        assert _call(d, 4096, [0.5], ALL, NONE) == 0                     # the limit itself
        assert _call(d, 4097, [0.5], ALL, NONE) == -1
        assert _call(d, 0, [0.5], ALL, NONE) == -1 and _call(d, 2, [0.5], ALL, NONE, first=-1) == -1
        assert _call(d, 5, [], ALL, NONE) == -1
        for bad in (float("nan"), float("inf"), -0.1, 1.5, 1.0000000000000002):
            assert _call(d, 5, [0.5, bad], ALL, NONE) == -1, bad
            with pytest.raises(hip.EmsarHipError) as e:
                d.bootstrap_quantiles(5, [bad], 1)
            assert e.value.status == -1
        for k in range(5):                                               # a transcript output missing
            assert _call(d, 5, [0.5], tuple(int(i != k) for i in range(5)), NONE) == -1
        assert _call(d, 5, [0.5], ALL, ALL) == -5                        # gene outputs without a map
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap_quantiles(5, [0.5], 1, want_genes=True)
        assert e.value.status == -5
        d.set_gene_map([1, -1, 1], 2)
        assert _call(d, 5, [0.5], ALL, ALL) == 0
        for k in range(5):                                               # a gene output group only partly given
            assert _call(d, 5, [0.5], ALL, tuple(int(i != k) for i in range(5))) == -1
            assert _call(d, 5, [0.5], ALL, tuple(int(i == k) for i in range(5))) == -1
        # closed form: theta_b = w_b, so the quantiles are those of the drawn weights
        r = d.bootstrap_quantiles(9, [0.0, 0.5, 1.0], 1, want_replicates=True, want_genes=True)
        w = np.array([d.bootstrap_weights(1, b) for b in range(9)], dtype=np.float64)
        assert same(r["replicates"], w) and same(r["fpkm_q"], np.sort(w, axis=0)[[0, 4, 8]])
        assert same(r["gene_fpkm_q"][:, 1], np.sort(w[:, 0] + w[:, 2])[[0, 4, 8]]) and not r["gene_fpkm_q"][:, 0].any()


# ---- the command-line driver ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


def _read_bootq(path, id_col):
    lines = open(path).read().splitlines()
    cols = lines[0].split("\t")
    assert cols[0] == id_col
    rows = [l.split("\t") for l in lines[1:]]
    assert all(len(r) == len(cols) for r in rows)
    return cols, rows


def _cli_sample_quantiles(fx, g2t, B, q, seed):
    """What emsar-hip does for a sample, through the Python bindings: count, model (L on the device), den in row order on the host,
    deterministic mode, the CLI's solver settings, the gene map of the g2t file, solve, bootstrap_quantiles."""
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
        d.solve(**cli)
        return d.bootstrap_quantiles(B, q, seed, want_genes=True, **cli), names, np.asarray(gmap)


def test_cli_bootq_files(tmp_path, _built):
    fx = get_fixture("vicugna_pe")
    g2t = os.path.join(fx.dir, "genes.g2t.gz")
    base = ["--bootstrap", "10", "--g2t", g2t]
    _run_cli(fx, tmp_path / "a", base + ["--stats-json", str(tmp_path / "a.json")])
    _run_cli(fx, tmp_path / "b", base + ["--bootstrap-quantiles", "0.025,0.5,0.975", "--stats-json", str(tmp_path / "b.json")])
    a, b = tmp_path / "a", tmp_path / "b"
    for ext in ("fpkm", "fraglength_effect", "segments", "bootstrap", "gfpkm", "gbootstrap"):
        assert open(a / ("out.0." + ext), "rb").read() == open(b / ("out.0." + ext), "rb").read(), ext
    assert not (a / "out.0.bootq").exists() and not (a / "out.0.gbootq").exists()
    ja, jb = json.load(open(tmp_path / "a.json"))["per_sample"][0], json.load(open(tmp_path / "b.json"))["per_sample"][0]
    assert set(jb) - set(ja) == {"bootq_quantiles", "bootq_held_bytes", "bootq_ms"} and set(ja) <= set(jb)
    assert jb["bootq_quantiles"] == 3 and jb["bootq_held_bytes"] > 0
    head = ["FPKM@" + s for s in ("0.025000000000000001", "0.5", "0.97499999999999998")]
    head += [h.replace("FPKM", "TPM") for h in head]
    cols, rows = _read_bootq(str(b / "out.0.bootq"), "transcriptID")
    gcols, grows = _read_bootq(str(b / "out.0.gbootq"), "geneID")
    assert cols[1:] == head and gcols[1:] == head
    text = [l.split("\t") for l in open(b / "out.0.fpkm").read().splitlines()[1:]]
    gtext = [l.split("\t") for l in open(b / "out.0.gfpkm").read().splitlines()[1:]]
    assert [r[0] for r in rows] == [t[0] for t in text] and [r[0] for r in grows] == [t[0] for t in gtext]
    # the library call's values, printed the same way (seed 1 + sample 0)
    r, names, gmap = _cli_sample_quantiles(fx, g2t, 10, [0.025, 0.5, 0.975], 1)
    assert [row[0] for row in grows] == names
    for k in range(3):
        assert [row[1 + k] for row in rows] == ["%f" % x for x in r["fpkm_q"][k]], k
        assert [row[4 + k] for row in rows] == ["%f" % x for x in r["tpm_q"][k]], k
        assert [row[1 + k] for row in grows] == ["%f" % x for x in r["gene_fpkm_q"][k]], k
        assert [row[4 + k] for row in grows] == ["%f" % x for x in r["gene_tpm_q"][k]], k
    # a one-transcript gene's row is its transcript's row
    n_iso = np.bincount(gmap, minlength=len(names))
    trow = {row[0]: row[1:] for row in rows}
    tx = [t[0] for t in text]
    checked = 0
    for g, row in enumerate(grows):
        if n_iso[g] == 1:
            assert row[1:] == trow[tx[int(np.nonzero(gmap == g)[0][0])]], names[g]
            checked += 1
    assert checked > 0
    assert max(float(row[3]) - float(row[1]) for row in rows) > 0          # an interval with some width


def test_cli_multisample(tmp_path, _built):
    fx = get_fixture("vicugna_pe")
    lst = tmp_path / "list.txt"
    aln = aln_path(fx.dir)[0]
    lst.write_text(aln + "\n" + aln + "\n")
    cmd = [CLI, "-q", "-M", "--gpus", "1", "--bootstrap", "8", "--bootstrap-quantiles", "0,0.5,1"] + fx.meta["opts"] + [
        "-I", os.path.join(fx.dir, "index.rsh"), str(tmp_path), "out", str(lst)]
    subprocess.run(cmd, check=True, timeout=600)
    c0, r0 = _read_bootq(str(tmp_path / "out.0.bootq"), "transcriptID")
    c1, r1 = _read_bootq(str(tmp_path / "out.1.bootq"), "transcriptID")
    assert c0 == c1 == ["transcriptID", "FPKM@0", "FPKM@0.5", "FPKM@1", "TPM@0", "TPM@0.5", "TPM@1"]
    assert [r[0] for r in r0] == [r[0] for r in r1] and r0 != r1           # seeds 1 and 2
    assert not (tmp_path / "out.0.gbootq").exists()
    for rows in (r0, r1):
        assert all(float(r[1]) <= float(r[2]) <= float(r[3]) and float(r[4]) <= float(r[5]) <= float(r[6]) for r in rows)
