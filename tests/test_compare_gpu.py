"""GPU: the two-sample likelihood-ratio test (emsar_hip_compare, include/emsar_hip.h "two-sample test") against an independent numpy
reference (tests/compare_problems.py: two plain EMs for F1, one plain EM on the stacked problem for F0, no multiplier in it), on
identical samples, with a size factor, across size classes, on the closed-form paths, at the boundary, on the paths that are not
searched, for bit-identity under everything a result must not depend on, under a swap of the samples, and through the CLI.

The tolerance of the reference comparison is dev_tol + 8 e_F: the reported dual value lies within dev_tol of the device's own statistic,
and four F values enter Lambda with a factor 2 each.  e_F is NOT taken from the kernel under test: it is 4 x the largest
|F of the existing set solver - F of the numpy EM| measured once on an MI355X on exactly the class problems below (DESIGN.md
"Two-sample test" has the figures and how they were taken: F is no output of any entry point, so it was measured (a) as numpy's F at
solve's theta against numpy's F at its own optimum and (b) through the presence test's Lambda, whose two F values come from
k_solve_sets_drop, against the numpy EM with the transcript dropped).

Every call passes max_iter <= 20000 and at most the default 40 evaluations: no workgroup can run long."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import compare_problems as CP
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED = range(5)
DEV_TOL = 1e-4                   # the default of emsar_compare_params.dev_tol
E_F_MEASURED = 9.4e-10           # the largest |F device - F numpy| on the class problems (DESIGN.md "Two-sample test"), one MI355X
E_F = 4 * E_F_MEASURED
TOL = DEV_TOL + 8 * E_F
CUT95 = 3.841458820694124
CAPS = dict(max_iter=20000)
OUTPUTS = H.COMPARE_OUTPUTS + ("status", "evals")


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b:
        yield a, b


def load(dev, prob, R, den=None, layout=H.LAYOUT_AUTO, merge_rows=False):
    n_tx, rp, ci, _, E = prob
    dev.upload_structure(n_tx, rp, ci, layout, merge_rows)
    dev.upload_sample(R, E, den)


def same_bits(x, y, keys=OUTPUTS):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def classes_of(prob, R):
    n_tx, rp, ci, _, E = prob
    return H.sets_selfcheck(n_tx, rp, ci, np.where(E > 0, R, 0))["sets_resident"]


@pytest.mark.parametrize("threads", [64, 256, 512])
def test_independent_reference(devs, threads):
    """a transcript whose set is of the class in both samples (256, 512: at the class's upper edge): Lambda against numpy"""
    a, b = devs
    prob, RA, RB, tids = CP.class_problem(threads)
    want = [0, 0, 0]
    want[(64, 256, 512).index(threads)] = 1
    assert classes_of(prob, RA) == want and classes_of(prob, RB) == want
    den = CP.den_of(prob)
    load(a, prob, RA, den)
    load(b, prob, RB, den)
    r = a.compare(b, tids, tol=1e-12, **CAPS)
    for i, t in enumerate(tids):
        ref = CP.reference(prob, RA, RB, t)
        print(threads, t, "Lambda", r["lambda"][i], "ref", ref["lam"], "diff", r["lambda"][i] - ref["lam"], "evals", r["evals"][i], "gap", r["gap"][i],
              "mult", r["multiplier"][i], "ref passes", ref["passes"])
        assert r["status"][i] == TESTED
        assert abs(r["lambda"][i] - ref["lam"]) <= TOL, (threads, t, r["lambda"][i], ref["lam"])
        assert abs(r["theta_a"][i] - ref["theta_a"]) <= 1e-6 * ref["theta_a"] and abs(r["theta_b"][i] - ref["theta_b"]) <= 1e-6 * ref["theta_b"]
        assert abs(r["theta_null"][i] - ref["theta_null"]) <= 1e-3 * ref["theta_null"]
        assert r["pvalue"][i] == H.compare_pvalue_host(r["lambda"][i])
        assert abs(r["log2fc"][i] - math.log2(ref["theta_a"] / ref["theta_b"])) <= 1e-5
    st = r["stats"].as_dict()
    print(st)
    assert st["items_launched"] == len(tids) and st["evals_sum"] == int(r["evals"].sum()) and st["n_status"]["TESTED"] == len(tids)


def test_identical_samples(devs):
    """compare(A, A') with A' a second context holding the same sample: Lambda exactly 0.0 after one evaluation, for every transcript"""
    a, b = devs
    prob = SP.all_resident_problem()
    den = CP.den_of(prob)
    load(a, prob, prob[3], den)
    load(b, prob, prob[3], den)
    r = a.compare(b, max_iter=4000)
    given = ~np.isin(r["status"], (OUTSIDE, NOT_RESIDENT))
    print(r["stats"].as_dict())
    assert given.sum() > 0.9 * prob[0]
    assert np.all(r["lambda"][given] == 0.0) and np.all(r["evals"][given] == 1) and np.all(r["pvalue"][given] == 1.0)
    assert np.all(r["raw_lambda"][given] == 0.0) and np.all(r["gap"][given] == 0.0) and np.all(r["multiplier"][given] == 0.0)
    assert r["theta_a"][given].tobytes() == r["theta_b"][given].tobytes()
    assert np.all(np.isin(r["status"][given], (TESTED, BOTH_ABSENT, UNCONVERGED)))
    assert np.all((r["status"][given] == BOTH_ABSENT) == (r["theta_a"][given] == 0.0))


def test_size_factor(devs):
    """B = A with every weight doubled: at ratio 1/2 nothing differs; at ratio 1 a transcript with >= 50 reads does"""
    a, b = devs
    prob, RA, _, _ = CP.class_problem(64)
    den = CP.den_of(prob)
    load(a, prob, RA, den)
    load(b, prob, 2 * RA, den)
    half = a.compare(b, ratio=0.5, tol=1e-12, **CAPS)
    given = ~np.isin(half["status"], (OUTSIDE, NOT_RESIDENT))
    print("ratio 1/2: max Lambda", half["lambda"][given].max(), "evals max", half["evals"].max())
    assert given.all() and np.all(half["lambda"] <= TOL) and np.all(np.isin(half["status"], (TESTED, BOTH_ABSENT)))
    assert np.all(np.abs(half["log2fc"][half["status"] == TESTED]) <= 1e-6)
    one = a.compare(b, ratio=1.0, tol=1e-12, **CAPS)
    reads = one["theta_a"] * den
    big = np.flatnonzero(reads >= 50)
    print("ratio 1: transcripts with >= 50 reads", len(big), "min Lambda among them", one["lambda"][big].min())
    assert len(big) >= 10 and np.all(one["lambda"][big] > CUT95) and np.all(one["status"][big] == TESTED)
    assert np.all(np.abs(one["log2fc"][big] + 1.0) <= 1e-6)


def test_different_classes(devs):
    """A has reads on ten chain rows only: t's component is 64-class in A and 512-class in B; the launch takes the larger class"""
    a, b = devs
    prob, RA, RB, tids = CP.split_problem()
    assert classes_of(prob, RA) == [1, 0, 0] and classes_of(prob, RB) == [0, 0, 1]
    den = CP.den_of(prob)
    load(a, prob, RA, den)
    load(b, prob, RB, den)
    r = a.compare(b, tids, tol=1e-12, **CAPS)
    s = b.compare(a, tids, tol=1e-12, **CAPS)
    for i, t in enumerate(tids):
        ref = CP.reference(prob, RA, RB, t)
        print("split", t, "Lambda", r["lambda"][i], s["lambda"][i], "ref", ref["lam"], "evals", r["evals"][i], s["evals"][i], "theta", r["theta_a"][i], r["theta_b"][i])
        assert r["status"][i] == TESTED and s["status"][i] == TESTED
        assert abs(r["lambda"][i] - ref["lam"]) <= TOL, (t, r["lambda"][i], ref["lam"])
        assert abs(s["lambda"][i] - ref["lam"]) <= TOL, (t, s["lambda"][i], ref["lam"])
    assert r["stats"].items_launched == len(tids)


def small(devs, **kw):
    a, b = devs
    prob, RA, RB, den_a, den_b = CP.small_problem()
    load(a, prob, RA, den_a)
    load(b, prob, RB, den_b)
    return prob, RA, RB, den_a, den_b, a.compare(b, tol=1e-12, **CAPS, **kw)


def test_closed_form_paths_boundary_and_outside(devs):
    prob, RA, RB, den_a, den_b, r = small(devs)
    print({k: r[k] for k in OUTPUTS})
    # both closed form: the host's search, the bits of the diagnostic entry the CPU test checks against the closed form
    for t in (0, 1):
        want = H.debug_compare_closed(float(RA[t]), den_a[t], float(RB[t]), den_b[t])
        for k in OUTPUTS:
            assert np.array([r[k][t]]).tobytes() == np.array([want[k]], dtype=r[k].dtype).tobytes(), (t, k, r[k][t], want[k])
    assert r["lambda"][1] == 0.0 and r["evals"][1] == 1
    # one side closed form (2: alone in A, in a set in B), a family in both (3, 4, 5), 7 next to the boundary case
    for t in (2, 3, 4, 5, 7):
        ref = CP.reference(prob, RA, RB, t, 1.0, den_a, den_b)
        print(t, r["lambda"][t], ref["lam"], r["evals"][t])
        assert r["status"][t] == TESTED and abs(r["lambda"][t] - ref["lam"]) <= TOL, (t, r["lambda"][t], ref["lam"])
    # boundary: 6 has 30 reads of its own in A and not one read in B
    ref = CP.reference(prob, RA, RB, 6, 1.0, den_a, den_b)
    print(6, r["lambda"][6], ref["lam"], r["evals"][6], r["theta_a"][6], r["theta_b"][6])
    assert r["theta_b"][6] == 0.0 and r["theta_a"][6] * den_a[6] >= 20 and r["status"][6] == TESTED and r["log2fc"][6] == math.inf
    assert np.isfinite(r["lambda"][6]) and abs(r["lambda"][6] - ref["lam"]) <= TOL, (r["lambda"][6], ref["lam"])
    # absent in both; den = 0 in one sample
    for t in (8, 9):
        assert r["status"][t] == BOTH_ABSENT and r["lambda"][t] == 0.0 and r["pvalue"][t] == 1.0 and r["evals"][t] == 1 and math.isnan(r["log2fc"][t])
    assert r["status"][10] == OUTSIDE and r["evals"][10] == 0
    for k in H.COMPARE_OUTPUTS:
        assert math.isnan(r[k][10]), k
    st = r["stats"].as_dict()
    assert sum(st["n_status"].values()) == prob[0] and st["n_status"]["OUTSIDE"] == 1 and st["n_status"]["BOTH_ABSENT"] == 2
    assert st["items_launched"] == 6                          # 2 .. 7: the rest never reaches the device


def test_boundary_inside_a_set(devs):
    """theta_hat_t = 0 in B although a row of t has reads there (its sibling explains them better), 35 reads of t alone in A"""
    a, b = devs
    rows = [[0], [0, 1], [1], [1, 2], [2]]
    n_tx, rp, ci = CP.csr(rows, 3)
    E = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    RA = np.array([35, 10, 20, 8, 15], dtype=np.int32)
    RB = np.array([0, 6, 90, 8, 15], dtype=np.int32)
    prob = (n_tx, rp, ci, RA, E)
    load(a, prob, RA)
    load(b, prob, RB)
    r = a.compare(b, tol=1e-12, **CAPS)
    ref = CP.reference(prob, RA, RB, 0)
    print({k: r[k] for k in OUTPUTS}, ref)
    assert ref["theta_b"] < 1e-6                                  # the reference agrees that B's estimate sits on the boundary
    assert r["theta_b"][0] <= 1e-6 and r["status"][0] == TESTED and abs(r["lambda"][0] - ref["lam"]) <= TOL, (r["lambda"][0], ref["lam"])
    if r["theta_b"][0] == 0.0:
        assert r["log2fc"][0] == math.inf


def test_other_statuses_and_errors(devs):
    a, b = devs
    prob, RA, RB, den_a, den_b, r1 = small(devs, set_mode=1)
    assert np.all(r1["status"] == NOT_RESIDENT) and r1["stats"].items_launched == 0 and np.all(r1["evals"] == 0)
    for k in H.COMPARE_OUTPUTS:
        assert np.all(np.isnan(r1[k])), k
    r = a.compare(b, max_evals=1, **CAPS)
    full = a.compare(b, **CAPS)
    moved = np.flatnonzero((full["status"] == TESTED) & (full["evals"] > 1))
    assert len(moved) >= 6
    assert np.all(r["status"][moved] == UNCONVERGED) and np.all(r["evals"][moved] == 1) and np.all(r["lambda"][moved] == 0.0)
    assert r["theta_a"][moved].tobytes() == full["theta_a"][moved].tobytes() and r["theta_b"][moved].tobytes() == full["theta_b"][moved].tobytes()
    for bad in (dict(query=[0, 11]), dict(query=[-1]), dict(ratio=-1.0), dict(ratio=math.nan), dict(ratio=math.inf), dict(dev_tol=math.inf),
                dict(set_mode=2), dict(count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare(b, **bad, **CAPS)
        assert e.value.status == -1, bad
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare(a, **CAPS)
    assert e.value.status == -1
    with emsar_amd.EmsarHip(0) as d:
        d.upload_structure(prob[0], prob[1], prob[2])
        for x, y in ((a, d), (d, a)):
            with pytest.raises(emsar_amd.EmsarHipError) as e:
                x.compare(y, **CAPS)
            assert e.value.status == -5                           # before upload_sample
        n_tx, rp, ci = CP.csr([[0, 1], [1, 2]], prob[0])
        d.upload_structure(n_tx, rp, ci)
        d.upload_sample()
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare(d, **CAPS)
        assert e.value.status == -1                               # another structure
    # a ratio of 0 is the default 1
    assert not same_bits(a.compare(b, ratio=0.0, **CAPS), full)


def invariance_problem():
    """five 64-class sets side by side (two edge shapes between small families) under two fitted samples that differ in every third transcript"""
    sets = [SP.family(3, 1), SP.edge_set(*SP.EDGES[0][0], seed=SP.SEEDS[0]), SP.family(2, 2), SP.edge_set(*SP.EDGES[2][0], seed=SP.SEEDS[2]), SP.family(5, 3)]
    prob = SP.compose(sets, seed=31)
    return prob, CP.fitted_weights(prob, 41), CP.fitted_weights(prob, 42, apart=range(0, prob[0], 3))


def test_invariance_bit_for_bit(devs, monkeypatch):
    a, b = devs
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    kw = dict(max_iter=3000)
    load(a, prob, RA, den, H.LAYOUT_CSR)
    load(b, prob, RB, den, H.LAYOUT_CSR)
    before = [a.solve(**kw)[0], b.solve(**kw)[0]]
    whole = a.compare(b, **kw)
    after = [a.solve(**kw)[0], b.solve(**kw)[0]]
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    st = whole["stats"].as_dict()
    print(st)
    assert st["n_status"]["TESTED"] >= 30 and st["n_status"]["TESTED"] + st["n_status"]["UNCONVERGED"] == prob[0] and st["evals_max"] <= 40
    q = np.random.default_rng(5).permutation(prob[0]).astype(np.int32)
    shuffled = a.compare(b, q, **kw)
    twice = a.compare(b, np.concatenate([q[:30], q[:30], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_COMPARE_BATCH", "1")           # one item per class and launch
    single = a.compare(b, **kw)
    monkeypatch.delenv("EMSAR_HIP_COMPARE_BATCH")
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][60:].tobytes() == shuffled[k].tobytes() and twice[k][:30].tobytes() == twice[k][30:60].tobytes() == shuffled[k][:30].tobytes(), k
        assert single[k].tobytes() == whole[k].tobytes(), k
    assert sum(twice["stats"].as_dict()["n_status"].values()) == prob[0]
    for layout, merge in ((H.LAYOUT_TILED, False), (H.LAYOUT_TILED, True)):
        load(a, prob, RA, den, layout, merge)
        load(b, prob, RB, den, layout, merge)
        assert not same_bits(a.compare(b, **kw), whole), (layout, merge)
    load(b, prob, RB, den, H.LAYOUT_CSR)                         # the two contexts need not share a layout
    assert not same_bits(a.compare(b, **kw), whole)


def test_swap(devs):
    """compare(B, A) at ratio 1 / r: the same Lambda within 2 dev_tol, the same status, log2fc negated"""
    a, b = devs
    prob, RA, RB, _ = CP.class_problem(64)
    den = CP.den_of(prob)
    load(a, prob, RA, den)
    load(b, prob, RB, den)
    for ratio in (1.0, 1.6):
        ab, ba = a.compare(b, ratio=ratio, **CAPS), b.compare(a, ratio=1.0 / ratio, **CAPS)
        ok = ab["status"] == TESTED
        print(ratio, "tested", ok.sum(), "max |dLambda|", np.abs(ab["lambda"][ok] - ba["lambda"][ok]).max(), "max Lambda", ab["lambda"][ok].max())
        assert np.array_equal(ab["status"], ba["status"])
        assert ok.sum() >= 30 and np.all(np.abs(ab["lambda"][ok] - ba["lambda"][ok]) <= 2 * DEV_TOL)
        assert np.all(np.abs(ab["log2fc"][ok] + ba["log2fc"][ok]) <= 1e-9)
        assert ab["theta_a"].tobytes() == ba["theta_b"].tobytes() and ab["theta_b"].tobytes() == ba["theta_a"].tobytes()


def test_cli_compare_file(tmp_path):
    """-M --compare on the syn300_se fixture and on every second read of it (the fixtures' indices differ in their fragment lengths, so a
    second sample over the same index is cut from the first): out.1.compare has one line per transcript and its columns are the Python
    call's as printed; sample 0 writes no .compare; without -M, or with one sample, --compare is a usage error"""
    import gzip

    from emsar_amd import _build
    from emsar_amd import hostlib as HL
    from tests.conftest import aln_path, get_fixture
    _build.build_all()
    fx = get_fixture("syn300_se")
    aln, fmt = aln_path(fx.dir)
    rsh_path = os.path.join(fx.dir, "index.rsh")
    lines = gzip.open(aln, "rt").read().splitlines(True)
    names = []
    for l in lines:
        if not names or names[-1] != l.split("\t")[0]:
            names.append(l.split("\t")[0])
    keep = set(names[::2])
    alns = [tmp_path / "full.bowtie.gz", tmp_path / "half.bowtie.gz"]
    with gzip.open(alns[0], "wt") as f:
        f.write("".join(lines))
    with gzip.open(alns[1], "wt") as f:
        f.write("".join(l for l in lines if l.split("\t")[0] in keep))
    lst = tmp_path / "samples.list"
    lst.write_text("".join(str(p) + "\n" for p in alns))
    base = [_build.CLI, "-q", "-i", "20000"] + fx.meta["opts"]
    subprocess.run(base + ["-M", "--gpus", "1", "--compare", "-I", rsh_path, str(tmp_path / "o"), "out", str(lst)], check=True, timeout=300)
    assert not (tmp_path / "o" / "out.0.compare").exists()
    got = [l.split("\t") for l in (tmp_path / "o" / "out.1.compare").read_text().splitlines()]
    assert got[0] == ["tid", "transcriptID", "FPKM", "FPKM_ref", "log2FC", "Lambda", "p", "status", "evals"]
    got = got[1:]
    rsh = HL.HostRsh(rsh_path)
    assert len(got) == rsh.n_tx and all(len(r) == 9 for r in got) and [int(r[0]) for r in got] == list(range(rsh.n_tx))
    assert [r[1] for r in got] == list(rsh.names)
    # what the CLI does for the two samples, through the Python bindings
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=20000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
    rows = np.repeat(np.arange(rsh.n_rows), np.diff(rp.astype(np.int64)))
    with emsar_amd.EmsarHip(0) as d0, emsar_amd.EmsarHip(0) as d1:
        for d, path in ((d0, alns[0]), (d1, alns[1])):
            cnt = rsh.count(str(path), fmt=fmt)
            d.set_deterministic(True)
            d.upload_structure(rsh.n_tx, rp, ci)
            d.upload_euma(rsh.euma)
            E = np.array(rsh.model(cnt, L=d.adj_euma(rsh.wf(cnt))).E_solver)
            den = np.zeros(rsh.n_tx)
            keep_e = E[rows] != 0.0
            np.add.at(den, ci[keep_e], E[rows][keep_e])
            d.upload_sample(np.array(cnt.R), E, den)
        p = d1.compare(d0, **cli)
    assert [r[7] for r in got] == [H.COMPARE_STATUS[k] for k in p["status"]]
    assert [int(r[8]) for r in got] == list(p["evals"])
    for col, key in ((2, "theta_a"), (3, "theta_b"), (4, "log2fc"), (5, "lambda")):
        v = np.array([float(r[col]) for r in got])
        fin = np.isfinite(p[key])
        assert np.array_equal(np.isnan(v), np.isnan(p[key])) and np.array_equal(v[~fin & ~np.isnan(v)], p[key][~fin & ~np.isnan(p[key])]), key
        assert np.all(np.abs(v[fin] - p[key][fin]) <= 1e-6 + 1e-15 * np.abs(p[key][fin])), key          # "%lf"
    assert [r[5] for r in got] == ["nan" if math.isnan(x) else "inf" if math.isinf(x) else "%f" % x for x in p["lambda"]]
    print(p["stats"].as_dict())
    assert np.sum(p["status"] == TESTED) >= 10
    one = tmp_path / "one.list"
    one.write_text(str(alns[0]) + "\n")
    for cmd in (base + ["--compare", "-I", rsh_path, str(tmp_path / "e"), "out", str(alns[0])],
                base + ["-M", "--compare", "-I", rsh_path, str(tmp_path / "e"), "out", str(one)]):
        res = subprocess.run(cmd, capture_output=True, timeout=300)
        assert res.returncode != 0 and b"--compare needs -M" in res.stderr and b"Usage" in res.stderr
