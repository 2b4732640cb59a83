"""GPU: the binomial depth subsampling (emsar_hip_subsample) -- device draws against the host's, every replicate against an independent
solve of its thinned sample, the depth normalisation, invariance under batching, the neighbouring fractions, layout and numbering, no
side effects on the context, the gene outputs, errors, and the CLI's .saturation file."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from emsar_amd import EmsarHip, _build, hip
from tests.conftest import CASES, aln_path, get_fixture
from tests.test_bootstrap_gpu import CLI, SOLVE, _check_same_mle, _eff_R, _family, _problems, _run_cli
from tests.test_genes_gpu import _boot_case, chunked_sums, welford
from tests.test_subsample_cpu import btrs_rows, is_inversion

pytestmark = pytest.mark.gpu
KEYS = ("fpkm_mean", "fpkm_sd", "tpm_mean", "tpm_sd", "depth_mean", "replicates")


@pytest.fixture(scope="module")
def dev():
    with EmsarHip(0) as d:
        yield d


def _upload(d, m, **kw):
    d.upload_structure(m.n_tx, m.row_ptr, m.col_idx, **kw)
    d.upload_sample(m.R, m.E, None)


def test_device_draws_equal_host_draws(dev):
    n_btrs = n_off = 0
    for case, m in _problems():                            # the fixtures and the family matrix
        _upload(dev, m)
        R = _eff_R(m.R, m.E)
        for f in (0.1, 0.5, 0.9, 1.0):
            inv = np.array([is_inversion(int(r), f) for r in R])
            for rep in (0, 7):
                got, want = dev.subsample_weights(11, rep, f), hip.subsample_draw_host(11, rep, f, R)
                assert np.array_equal(got[inv], want[inv]), (case, f)
                if f < 1.0 and (~inv).any():               # the BTRS rows: the bound of the large-count input below
                    n_btrs += int((~inv).sum())
                    n_off += int((got[~inv] != want[~inv]).sum())
                    assert (got[~inv] == want[~inv]).mean() >= 0.999, (case, f, rep)
                elif f == 1.0:
                    assert np.array_equal(got, R)
    print("fixtures and family: %d BTRS draws, %d differ from the host" % (n_btrs, n_off))
    assert n_btrs > 0
    # large counts: the BTRS path, where the device log may differ from the host's by an ulp at an acceptance edge
    n_tx, rp, ci, R = btrs_rows()
    dev.upload_structure(n_tx, rp, ci)
    dev.upload_sample(R, None, None)
    for f in (0.3, 0.5, 0.8):
        got, want = dev.subsample_weights(2, 3, f), hip.subsample_draw_host(2, 3, f, R)
        inv = R * min(f, 1.0 - f) < 10.0
        assert (~inv).sum() >= 10000
        print("f = %g: %d BTRS rows, %d differ from the host" % (f, (~inv).sum(), (got[~inv] != want[~inv]).sum()))
        assert np.array_equal(got[inv], want[inv]), f
        assert (got[~inv] == want[~inv]).mean() >= 0.999, f


@pytest.mark.parametrize("set_mode,tiled_multi", [(0, None), (1, None), (1, "5")], ids=["0", "1", "1-unit"])
def test_replicates_are_solves_of_their_draws(set_mode, tiled_multi, monkeypatch):
    if tiled_multi is not None:
        monkeypatch.setenv("EMSAR_HIP_TILED_MULTI", tiled_multi)
    fr, n, seed = [0.5, 0.25], 2, 9
    with EmsarHip(0) as a, EmsarHip(0) as b:
        for name, m in _problems():
            _upload(a, m)
            r = a.subsample(fr, n, seed, want_replicates=True, set_mode=set_mode, **SOLVE)
            reps = r["replicates"]
            assert reps.shape == (len(fr), n, m.n_tx) and r["stats"].n_replicates == n and r["stats"].n_fractions == len(fr)
            N_R = int(_eff_R(m.R, m.E).astype(np.int64).sum())
            b.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
            for k, f in enumerate(fr):
                assert np.allclose(r["fpkm_mean"][k], reps[k].mean(0), rtol=1e-12, atol=1e-12)
                assert np.allclose(r["fpkm_sd"][k], reps[k].std(0, ddof=1), rtol=1e-9, atol=1e-12)
                S = reps[k].sum(1)
                tpm = np.where(S[:, None] > 0, reps[k] * 1e6 / np.where(S > 0, S, 1.0)[:, None], 0.0)
                assert np.allclose(r["tpm_mean"][k], tpm.mean(0), rtol=1e-12, atol=1e-12)
                assert np.allclose(r["tpm_sd"][k], tpm.std(0, ddof=1), rtol=1e-9, atol=1e-9)
                depth = []
                for j in range(n):
                    w = a.subsample_weights(seed, j, f)
                    N_b = int(w.astype(np.int64).sum())
                    depth.append(N_b)
                    raw = reps[k, j] / (N_R / N_b) if N_b > 0 else reps[k, j]
                    if N_b == 0:
                        assert not reps[k, j].any()
                        continue
                    b.upload_sample(w, m.E, None)
                    th_b, _ = b.solve(set_mode=set_mode, **SOLVE)
                    _check_same_mle(m, w, raw, th_b, "%s f %g rep %d vs solve" % (name, f, j))
                    th_o, _ = O.Csr(m.n_tx, m.row_ptr, m.col_idx, R=w, E=m.E).em_solve(max_iter=200000, tol=1e-10)
                    _check_same_mle(m, w, raw, th_o, "%s f %g rep %d vs oracle" % (name, f, j))
                assert r["depth_mean"][k] == np.mean(depth), (name, f)


@pytest.mark.parametrize("set_mode", [0, 1])
def test_full_fraction_is_the_sample(set_mode):
    with EmsarHip(0) as d:
        # the streaming passes add with floating atomics unless the deterministic mode is on: two solves of the same weights then
        # differ in their last bits, and no sd over them is exactly 0
        d.set_deterministic(True)
        for name, m in _problems():
            _upload(d, m)
            R = _eff_R(m.R, m.E)
            assert np.array_equal(d.subsample_weights(4, 2, 1.0), R)
            th, _ = d.solve(set_mode=set_mode, **SOLVE)
            r = d.subsample([1.0], 3, 4, want_replicates=True, set_mode=set_mode, **SOLVE)
            assert r["depth_mean"][0] == R.astype(np.int64).sum()
            assert np.array_equal(r["replicates"][0][0], r["replicates"][0][2])
            assert not r["fpkm_sd"].any() and not r["tpm_sd"].any(), name
            _check_same_mle(m, R, r["fpkm_mean"][0], th, name + " f = 1")


@pytest.mark.parametrize("set_mode", [0, 1])
def test_batch_and_neighbour_invariance(set_mode, monkeypatch):
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        for name, m in [("vicugna_pe", get_fixture("vicugna_pe").model), ("family", _family(4))]:
            _upload(d, m)
            one = d.subsample([0.5, 0.25], 10, 5, want_replicates=True, set_mode=set_mode, **SOLVE)
            for batch in ("1", "3"):
                monkeypatch.setenv("EMSAR_HIP_BOOT_BATCH", batch)
                other = d.subsample([0.5, 0.25], 10, 5, want_replicates=True, set_mode=set_mode, **SOLVE)
                monkeypatch.delenv("EMSAR_HIP_BOOT_BATCH")
                assert other["stats"].batch == int(batch)
                for k in KEYS:
                    assert np.array_equal(one[k], other[k]), (name, batch, k)
            for i, f in enumerate([0.5, 0.25]):
                alone = d.subsample([f], 10, 5, want_replicates=True, set_mode=set_mode, **SOLVE)
                for k in KEYS:
                    assert np.array_equal(one[k][i], alone[k][0]), (name, f, k)


def test_draws_do_not_depend_on_layout_or_numbering(monkeypatch):
    m = _family(6)
    R = _eff_R(m.R, m.E)
    want = hip.subsample_draw_host(3, 1, 0.5, R)
    res = []
    for renumber in ("2", "0"):
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
        with EmsarHip(0) as d:
            for layout in (hip.LAYOUT_TILED, hip.LAYOUT_CSR):
                _upload(d, m, layout=layout)
                assert np.array_equal(d.subsample_weights(3, 1, 0.5), want), (renumber, layout)
                res.append(d.subsample([0.5], 3, 3, **SOLVE))
    for r in res[1:]:      # the same draws, so the same depth and, to the solver's tolerance, the same estimates
        assert np.array_equal(r["depth_mean"], res[0]["depth_mean"])
        assert np.allclose(r["fpkm_mean"], res[0]["fpkm_mean"], rtol=1e-9, atol=1e-12)


def test_no_side_effects(dev):
    m = get_fixture("syn2k_se").model
    _upload(dev, m)
    info = dev.info()
    th0, _ = dev.solve(**SOLVE)
    cur = dev.get_theta()
    b0 = dev.bootstrap(4, 77, **SOLVE)
    r1 = dev.subsample([0.3, 1.0], 4, 77, **SOLVE)
    assert np.array_equal(dev.get_theta(), cur)
    r2 = dev.subsample([0.3, 1.0], 4, 77, **SOLVE)
    for k in KEYS[:5]:
        assert np.array_equal(r1[k], r2[k])
    th1, _ = dev.solve(**SOLVE)
    assert np.array_equal(th0, th1)
    b1 = dev.bootstrap(4, 77, **SOLVE)
    for x, y in zip(b0[:3], b1[:3]):
        assert np.array_equal(x, y)
    assert dev.info() == info
    # streaming path too (set_mode 1 swaps the replicates' weights into the layout and back)
    dev.set_deterministic(True)
    s0, _ = dev.solve(set_mode=1, **SOLVE)
    c0 = dev.bootstrap(3, 1, set_mode=1, **SOLVE)
    dev.subsample([0.5], 3, 1, set_mode=1, **SOLVE)
    s1, _ = dev.solve(set_mode=1, **SOLVE)
    c1 = dev.bootstrap(3, 1, set_mode=1, **SOLVE)
    dev.set_deterministic(False)
    assert np.array_equal(s0, s1)
    for x, y in zip(c0[:3], c1[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("set_mode", [0, 1], ids=["sets", "streaming"])
@pytest.mark.parametrize("name", ["vicugna_pe", "family"])
def test_gene_outputs(name, set_mode):
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        m, gmap, ng = _boot_case(d, name)
        fr, B, seed = [0.5, 0.2], 8, 21
        r = d.subsample(fr, B, seed, want_replicates=True, want_genes=True, set_mode=set_mode, **SOLVE)
        plain = d.subsample(fr, B, seed, want_replicates=True, set_mode=set_mode, **SOLVE)
        for k in KEYS:
            assert np.array_equal(r[k], plain[k]), k
        alone = np.nonzero((np.bincount(gmap[gmap >= 0], minlength=ng) == 1)[np.maximum(gmap, 0)] & (gmap >= 0))[0]
        assert len(alone) > 0
        for i in range(len(fr)):
            reps = r["replicates"][i]
            G = chunked_sums(reps, gmap, ng)
            assert np.array_equal(d.gene_sums(reps), G)
            S = reps.sum(axis=1)
            gm, gs = welford(G)
            gtm, _ = welford(np.where(S[:, None] > 0, G * 1e6 / S[:, None], 0.0))
            for got, want in ((r["gene_fpkm_mean"][i], gm), (r["gene_fpkm_sd"][i], gs), (r["gene_tpm_mean"][i], gtm)):
                assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-300), (name, i)
            # a one-transcript gene's row is its transcript's row
            assert np.array_equal(r["gene_fpkm_mean"][i][gmap[alone]], r["fpkm_mean"][i][alone])
            assert np.array_equal(r["gene_fpkm_sd"][i][gmap[alone]], r["fpkm_sd"][i][alone])
            assert np.array_equal(r["gene_tpm_mean"][i][gmap[alone]], r["tpm_mean"][i][alone])
        assert r["gene_fpkm_sd"].max() > 0


@pytest.mark.parametrize("set_mode", [0, 1])
def test_nothing_drawn(set_mode):
    """N_b = 0: at f = 1e-9 no read of a small sample survives.  Every replicate is all zero (factor 0, TPM of a zero sum is 0),
    depth_mean is 0 and the call succeeds."""
    rp, ci, R = [0, 1, 3, 4, 6], [0, 0, 1, 2, 1, 2], [5, 7, 3, 4]
    with EmsarHip(0) as d:
        d.upload_structure(3, rp, ci)
        d.upload_sample(R, [1.0, 2.0, 0.5, 1.5], None)
        for j in range(3):
            assert not d.subsample_weights(1, j, 1e-9).any()
        r = d.subsample([1e-9, 1.0], 3, 1, want_replicates=True, set_mode=set_mode, **SOLVE)
        assert r["depth_mean"].tolist() == [0.0, float(sum(R))]
        assert not r["replicates"][0].any()
        for k in ("fpkm_mean", "fpkm_sd", "tpm_mean", "tpm_sd"):
            assert not r[k][0].any(), k
        assert r["fpkm_mean"][1].max() > 0 and np.isfinite(r["fpkm_mean"]).all()
        d.solve(set_mode=set_mode, **SOLVE)


def test_errors():
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        for call in (lambda: d.subsample([0.5], 5, 1), lambda: d.subsample_weights(1, 0, 0.5)):
            with pytest.raises(hip.EmsarHipError) as e:
                call()
            assert e.value.status == -5
        d.upload_sample([1, 2, 3], None, None)
        bad = [lambda: d.subsample([], 5, 1), lambda: d.subsample([0.5], 0, 1), lambda: d.subsample([0.5], -1, 1)]
        for f in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            bad.append(lambda f=f: d.subsample([0.5, f], 2, 1))
            bad.append(lambda f=f: d.subsample_weights(1, 0, f))
        bad.append(lambda: d.subsample_weights(1, -1, 0.5))
        for call in bad:
            with pytest.raises(hip.EmsarHipError) as e:
                call()
            assert e.value.status == -1
        with pytest.raises(hip.EmsarHipError) as e:          # gene outputs without a map
            d.subsample([0.5], 2, 1, want_genes=True)
        assert e.value.status == -5
        r = d.subsample([1.0, 0.5], 2, 1)
        assert np.array_equal(r["fpkm_mean"][0], [1.0, 2.0, 3.0]) and r["depth_mean"][0] == 6.0


@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


def _read_saturation(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# fractions=")
    head = dict(kv.split("=") for kv in lines[0][2:].split(" "))
    cols = lines[1].split("\t")
    rows = [l.split("\t") for l in lines[2:]]
    assert all(len(r) == len(cols) for r in rows)
    return head, cols, rows


@pytest.mark.parametrize("case", ["vicugna_pe", "toy5_pe", "syn300_k2", "syn2k_se"])
def test_cli_saturation_file(case, tmp_path, _built):
    fx = get_fixture(case)
    fr = [0.25, 0.5, 1.0]
    sub = ["--subsample", "0.25,0.5,1", "--subsample-reps", "4", "--subsample-seed", "6"]
    _run_cli(fx, tmp_path / "a", ["--bootstrap", "5"])
    _run_cli(fx, tmp_path / "b", ["--bootstrap", "5"] + sub + ["--stats-json", str(tmp_path / "s.json")])
    for ext in ("fpkm", "fraglength_effect", "segments", "bootstrap"):
        assert open(tmp_path / "a" / ("out.0." + ext), "rb").read() == open(tmp_path / "b" / ("out.0." + ext), "rb").read(), ext
    assert not (tmp_path / "a" / "out.0.saturation").exists()
    head, cols, rows = _read_saturation(str(tmp_path / "b" / "out.0.saturation"))
    assert [float(x) for x in head["fractions"].split(",")] == fr and head["replicates"] == "4" and head["seed"] == "6"
    assert cols[:3] == ["transcriptID", "FPKM", "TPM"] and len(cols) == 3 + 4 * len(fr)
    text = [l.split("\t") for l in open(tmp_path / "a" / "out.0.fpkm").read().splitlines()[1:]]
    assert [r[0] for r in rows] == [t[0] for t in text]
    assert [r[1] for r in rows] == [t[1] for t in text] and [r[2] for r in rows] == [t[6] for t in text]
    js = json.load(open(tmp_path / "s.json"))["per_sample"][0]
    assert js["sub_fractions"] == 3 and js["sub_replicates"] == 4 and js["sub_draws"] > 0
    # the same numbers from the Python binding, printed the same way
    r, tpm = _cli_sample_subsample(fx, fr, 4, 6)
    assert head["depth_mean"] == ",".join("%f" % x for x in r["depth_mean"])
    assert [row[2] for row in rows] == ["%f" % x for x in tpm]
    for k in range(len(fr)):
        for j, key in enumerate(("fpkm_mean", "fpkm_sd", "tpm_mean", "tpm_sd")):
            assert [row[3 + 4 * k + j] for row in rows] == ["%f" % x for x in r[key][k]], (fr[k], key)
    assert not r["fpkm_sd"][2].any() and not r["tpm_sd"][2].any()                          # f = 1: sd 0
    assert r["fpkm_sd"][0].max() > 0


def _cli_sample_subsample(fx, fractions, n, seed):
    """What emsar-hip does for a sample, through the Python bindings: count, model (L on the device), den in row order on the host,
    deterministic mode, the CLI's solver settings, solve, subsample."""
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
        d.upload_sample(np.array(cnt.R), E, den)
        th, _ = d.solve(**cli)
        tpm, _, _ = d.normalise(th, np.zeros(rsh.n_tx), cnt.total_reads)
        return d.subsample(fractions, n, seed, **cli), tpm


def test_cli_multisample_seeds_differ_and_genes(tmp_path, _built):
    fx = get_fixture("vicugna_pe")
    lst = tmp_path / "list.txt"
    a = aln_path(fx.dir)[0]
    lst.write_text(a + "\n" + a + "\n")
    g2t = os.path.join(fx.dir, "genes.g2t.gz")
    cmd = [CLI, "-q", "-M", "--gpus", "1", "--subsample", "0.5", "--g2t", g2t] + fx.meta["opts"] + ["-I", os.path.join(fx.dir, "index.rsh"), str(tmp_path), "out", str(lst)]
    subprocess.run(cmd, check=True, timeout=600)
    h0, _, r0 = _read_saturation(str(tmp_path / "out.0.saturation"))
    h1, _, r1 = _read_saturation(str(tmp_path / "out.1.saturation"))
    assert h0["seed"] == "1" and h1["seed"] == "2" and h0["replicates"] == "10"
    assert [r[1] for r in r0] == [r[1] for r in r1]                   # same sample, same FPKM
    assert [r[3] for r in r0] != [r[3] for r in r1]                   # seeds 1 and 2
    gh, gcols, grows = _read_saturation(str(tmp_path / "out.0.gsaturation"))
    assert gcols[0] == "geneID" and len(gcols) == 3 + 3 and gh == h0
    gtext = [l.split("\t") for l in open(tmp_path / "out.0.gfpkm").read().splitlines()[1:]]
    assert [r[0] for r in grows] == [t[0] for t in gtext] and [r[1] for r in grows] == [t[1] for t in gtext]
    assert [r[2] for r in grows] == [t[4] for t in gtext]


def test_thinner_samples_are_noisier(dev):
    """Binomial thinning: the relative sd of TPM grows as the depth falls (about 3x between f = 0.5 and 0.1), and vanishes at f = 1."""
    m = get_fixture("vicugna_pe").model
    dev.set_deterministic(True)          # f = 1: the streamed part of every replicate is then the same bits
    _upload(dev, m)
    th, _ = dev.solve(**SOLVE)
    tpm = th * 1e6 / th.sum()
    r = dev.subsample([0.1, 0.5, 1.0], 10, 1, **SOLVE)
    dev.set_deterministic(False)
    sel = tpm >= 1
    assert sel.sum() > 10
    med = [np.median(r["tpm_sd"][k][sel] / tpm[sel]) for k in range(3)]
    print("median sd_TPM / TPM at f = 0.1, 0.5, 1.0:", med)
    assert med[0] > med[1] > 0
    assert med[2] == 0
