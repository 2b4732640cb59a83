"""GPU: the Poisson bootstrap (emsar_hip_bootstrap) -- device draws against the host's, every replicate against an independent solve of
its drawn sample, invariance under batching and splitting, no side effects on the context, the closed form, errors, and the CLI's
.bootstrap file."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from emsar_amd import EmsarHip, _build, hip, synth
from tests.conftest import CASES, aln_path, get_fixture

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "emsar_amd", "emsar-hip")
SOLVE = dict(max_iter=200000, tol=1e-10)


@pytest.fixture(scope="module")
def dev():
    with EmsarHip(0) as d:
        yield d


def _eff_R(R, E):
    return np.where(np.asarray(E) != 0, np.asarray(R, dtype=np.int64), 0).astype(np.int32)


def _family(seed=3):
    n_tx, rp, ci, R = synth.family_matrix([2, 3, 5, 8, 13, 40] * 8, rows_per_tid=3, seed=seed)
    E = np.random.default_rng(seed).uniform(0.5, 2.0, size=len(R))
    return O.Csr(n_tx, rp, ci, R=R, E=E)


def _problems():
    out = [(c, get_fixture(c).model) for c in CASES]
    out.append(("family", _family()))
    return out


def _check_same_mle(m, R_b, theta, want, what):
    """The parity criteria of the golden tests, on the drawn sample: the likelihood of theta is at least that of the independent solve
    (to 1e-9 relative), and every row's expected count E_c S_c agrees."""
    mb = O.Csr(m.n_tx, m.row_ptr, m.col_idx, R=R_b, E=m.E)
    F, F_w = mb.loglik(theta), mb.loglik(want)
    assert F >= F_w - 1e-9 * abs(F_w) - 1e-9, (what, F, F_w)
    rp = m.row_ptr.astype(np.int64)
    lam = lambda th: m.E * np.add.reduceat(np.append(th[m.col_idx], 0.0), rp[:-1])[: m.n_rows] * (np.diff(rp) > 0)
    a, b = lam(theta), lam(want)
    assert np.all(np.abs(a - b) <= 1e-5 * np.abs(b) + 2e-3), (what, np.max(np.abs(a - b)))


def test_device_draws_equal_host_draws(dev):
    for case in CASES:
        m = get_fixture(case).model
        dev.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
        dev.upload_sample(m.R, m.E, None)
        R = _eff_R(m.R, m.E)
        for rep in (0, 7):
            assert np.array_equal(dev.bootstrap_weights(11, rep), hip.bootstrap_draw_host(11, rep, R)), case
    # large counts: the PTRS path, where the device log may differ from the host's by an ulp at an acceptance edge
    rng = np.random.default_rng(5)
    n_rows, n_tx = 40000, 500
    rp = np.arange(n_rows + 1, dtype=np.uint64)
    ci = rng.integers(0, n_tx, size=n_rows).astype(np.int32)
    R = np.minimum(rng.lognormal(3.0, 2.5, size=n_rows), 1e5).astype(np.int32)
    dev.upload_structure(n_tx, rp, ci)
    dev.upload_sample(R, None, None)
    got, want = dev.bootstrap_weights(2, 3), hip.bootstrap_draw_host(2, 3, R)
    small = R <= 16
    assert np.array_equal(got[small], want[small])
    assert (got[~small] == want[~small]).mean() >= 0.999


@pytest.mark.parametrize("set_mode,tiled_multi", [(0, None), (1, None), (1, "5")], ids=["0", "1", "1-unit"])
def test_replicates_are_solves_of_their_draws(set_mode, tiled_multi, monkeypatch):
    """1-unit: the streaming solves with the unit kernel forced (EMSAR_HIP_TILED_MULTI=5), so that the replicates' swapped-in
    weights go through k_pass_tiled_unit<true, MODE_EM> as well."""
    if tiled_multi is not None:
        monkeypatch.setenv("EMSAR_HIP_TILED_MULTI", tiled_multi)
    with EmsarHip(0) as a, EmsarHip(0) as b:
        for name, m in _problems():
            a.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
            a.upload_sample(m.R, m.E, None)
            seed, first, n = 9, 2, 3
            mean, sd, tsd, reps, st = a.bootstrap(n, seed, first=first, want_replicates=True, set_mode=set_mode, **SOLVE)
            assert reps.shape == (n, m.n_tx) and st.n_replicates == n
            assert np.allclose(mean, reps.mean(0), rtol=1e-12, atol=1e-12)
            assert np.allclose(sd, reps.std(0, ddof=1), rtol=1e-9, atol=1e-12)
            b.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
            for k in range(n):
                w = a.bootstrap_weights(seed, first + k)
                b.upload_sample(w, m.E, None)
                th_b, _ = b.solve(set_mode=set_mode, **SOLVE)
                _check_same_mle(m, w, reps[k], th_b, "%s rep %d vs solve" % (name, k))
                th_o, _ = O.Csr(m.n_tx, m.row_ptr, m.col_idx, R=w, E=m.E).em_solve(max_iter=200000, tol=1e-10)
                _check_same_mle(m, w, reps[k], th_o, "%s rep %d vs oracle" % (name, k))


@pytest.mark.parametrize("set_mode", [0, 1])
def test_batch_and_split_invariance(set_mode, monkeypatch):
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        for name, m in [("vicugna_pe", get_fixture("vicugna_pe").model), ("family", _family(4))]:
            d.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
            d.upload_sample(m.R, m.E, None)
            one = d.bootstrap(10, 5, want_replicates=True, set_mode=set_mode, **SOLVE)
            p1 = d.bootstrap(3, 5, first=0, want_replicates=True, set_mode=set_mode, **SOLVE)
            p2 = d.bootstrap(7, 5, first=3, want_replicates=True, set_mode=set_mode, **SOLVE)
            assert np.array_equal(one[3], np.vstack([p1[3], p2[3]])), name
            monkeypatch.setenv("EMSAR_HIP_BOOT_BATCH", "1")
            single = d.bootstrap(10, 5, want_replicates=True, set_mode=set_mode, **SOLVE)
            monkeypatch.delenv("EMSAR_HIP_BOOT_BATCH")
            assert single[4].batch == 1
            for x, y in zip(one[:4], single[:4]):
                assert np.array_equal(x, y), name


def test_reproducible_and_no_side_effects(dev):
    m = get_fixture("syn2k_se").model
    dev.upload_structure(m.n_tx, m.row_ptr, m.col_idx)
    dev.upload_sample(m.R, m.E, None)
    info = dev.info()
    th0, _ = dev.solve(**SOLVE)
    cur = dev.get_theta()
    r1 = dev.bootstrap(6, 77, **SOLVE)
    assert np.array_equal(dev.get_theta(), cur)
    r2 = dev.bootstrap(6, 77, **SOLVE)
    for x, y in zip(r1[:3], r2[:3]):
        assert np.array_equal(x, y)
    assert (r1[1] >= 0).all() and (r1[2] >= 0).all() and r1[1].max() > 0
    th1, _ = dev.solve(**SOLVE)
    assert np.array_equal(th0, th1)
    assert dev.info() == info
    # streaming path too (set_mode 1 swaps the replicates' weights into the layout and back)
    dev.set_deterministic(True)
    s0, _ = dev.solve(set_mode=1, **SOLVE)
    dev.bootstrap(3, 1, set_mode=1, **SOLVE)
    s1, _ = dev.solve(set_mode=1, **SOLVE)
    dev.set_deterministic(False)
    assert np.array_equal(s0, s1)


@pytest.mark.parametrize("layout", [hip.LAYOUT_CSR, hip.LAYOUT_TILED], ids=["csr", "tiled"])
def test_unweighted_sample_is_restored(layout):
    """A sample uploaded without weights has no weight arrays on the device: the streamed replicates allocate them, and the call frees
    them again and leaves the sample unweighted (stored_bytes_per_pass counts 4 bytes per row only while it is weighted)."""
    m = _family()
    with EmsarHip(0) as d:
        d.set_deterministic(True)
        d.upload_structure(m.n_tx, m.row_ptr, m.col_idx, layout=layout)
        d.upload_sample(np.ones(m.n_rows, dtype=np.int32), None, None)
        weighted_bytes = d.info()["stored_bytes_per_pass"]
        d.upload_sample(None, None, None)
        info = d.info()
        assert info["stored_bytes_per_pass"] < weighted_bytes      # the sample really starts without weight arrays (no merged rows)
        th0, st0 = d.solve(set_mode=1, **SOLVE)
        d.bootstrap(3, 1, set_mode=1, **SOLVE)
        d.subsample([0.5], 2, 1, set_mode=1, **SOLVE)
        th1, st1 = d.solve(set_mode=1, **SOLVE)
        assert np.array_equal(th0, th1)
        assert st1.stored_bytes_per_pass == st0.stored_bytes_per_pass
        assert d.info() == info
        d.run_passes(2)


def test_closed_form(dev):
    n_tx = 50
    rng = np.random.default_rng(1)
    R = rng.integers(1, 400, size=n_tx).astype(np.int32)
    rp = np.arange(n_tx + 1, dtype=np.uint64)
    ci = np.arange(n_tx, dtype=np.int32)
    E = rng.uniform(0.5, 2.0, size=n_tx)
    dev.upload_structure(n_tx, rp, ci)
    dev.upload_sample(R, E, None)
    mean, sd, tsd, reps, st = dev.bootstrap(2000, 3, want_replicates=True)
    w0 = dev.bootstrap_weights(3, 0)
    assert np.array_equal(reps[0], w0 / E)
    w5 = dev.bootstrap_weights(3, 5)
    assert np.array_equal(reps[5], w5 / E)
    assert np.all(np.abs(sd - np.sqrt(R) / E) <= 0.05 * np.sqrt(R) / E)


def test_errors():
    with EmsarHip(0) as d:
        d.upload_structure(3, [0, 1, 2, 3], [0, 1, 2])
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap(5, 1)
        assert e.value.status == -5
        d.upload_sample([1, 2, 3], None, None)
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap(0, 1)
        assert e.value.status == -1
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap(2, 1, first=-1)
        assert e.value.status == -1


def _run_cli(fx, out, extra, aln=None):
    cmd = [CLI, "-q", "-g"] + fx.meta["opts"] + extra + ["-I", os.path.join(fx.dir, "index.rsh"), str(out), "out", aln or aln_path(fx.dir)[0]]
    subprocess.run(cmd, check=True, timeout=600)


def _read_boot(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "transcriptID\tFPKM\tboot.mean.FPKM\tboot.sd.FPKM\tTPM\tboot.sd.TPM"
    rows = [l.split("\t") for l in lines[1:]]
    return [r[0] for r in rows], np.array([[float(x) for x in r[1:]] for r in rows])


@pytest.fixture(scope="module")
def _built():
    _build.build_all()
    assert os.path.exists(CLI)


@pytest.mark.parametrize("case", ["vicugna_pe", "toy5_pe", "syn300_k2", "syn2k_se"])
def test_cli_bootstrap_file(case, tmp_path, _built):
    fx = get_fixture(case)
    _run_cli(fx, tmp_path / "a", [])
    _run_cli(fx, tmp_path / "b", ["--bootstrap", "50"])
    _run_cli(fx, tmp_path / "c", ["--bootstrap", "50", "--stats-json", str(tmp_path / "s.json")])
    for ext in ("fpkm", "fraglength_effect", "segments"):
        assert open(tmp_path / "a" / ("out.0." + ext), "rb").read() == open(tmp_path / "b" / ("out.0." + ext), "rb").read(), ext
    assert not (tmp_path / "a" / "out.0.bootstrap").exists()
    boot = open(tmp_path / "b" / "out.0.bootstrap", "rb").read()
    assert boot == open(tmp_path / "c" / "out.0.bootstrap", "rb").read()
    names, v = _read_boot(str(tmp_path / "b" / "out.0.bootstrap"))
    f = O.read_fpkm(str(tmp_path / "a" / "out.0.fpkm"))
    assert names == f["names"]
    text = [l.split("\t") for l in open(tmp_path / "a" / "out.0.fpkm").read().splitlines()[1:]]
    btext = [l.split("\t") for l in boot.decode().splitlines()[1:]]
    assert [r[1] for r in text] == [r[1] for r in btext] and [r[6] for r in text] == [r[4] for r in btext]
    assert (v[:, 2] >= 0).all() and (v[:, 4] >= 0).all() and v[:, 2].max() > 0
    import json
    js = json.load(open(tmp_path / "s.json"))["per_sample"][0]
    assert js["boot_replicates"] == 50 and js["boot_draws"] > 0


def test_cli_multisample_seeds_differ(tmp_path, _built):
    fx = get_fixture("vicugna_pe")
    lst = tmp_path / "list.txt"
    a = aln_path(fx.dir)[0]
    lst.write_text(a + "\n" + a + "\n")
    cmd = [CLI, "-q", "-M", "--gpus", "1", "--bootstrap", "20"] + fx.meta["opts"] + ["-I", os.path.join(fx.dir, "index.rsh"), str(tmp_path), "out", str(lst)]
    subprocess.run(cmd, check=True, timeout=600)
    _, v0 = _read_boot(str(tmp_path / "out.0.bootstrap"))
    _, v1 = _read_boot(str(tmp_path / "out.1.bootstrap"))
    assert np.array_equal(v0[:, 0], v1[:, 0])            # same sample, same FPKM
    assert not np.array_equal(v0[:, 2], v1[:, 2])        # seeds 1 and 2
