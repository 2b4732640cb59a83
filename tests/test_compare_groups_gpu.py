"""GPU: the K-sample test across replicate groups (emsar_hip_compare_groups, include/emsar_hip.h "K-sample test") against the independent
numpy reference of tests/compare_groups_problems.py (plain EMs only; recorded in tests/golden/compare_groups_refs.json), against
emsar_hip_compare at K = 2, on identical samples, for bit-identity under everything a result must not depend on, on the paths that are
not searched or searched on the host, on its argument errors, and through the CLI.

The tolerance on a Lambda is derived as test_compare_usage_gpu.py derives its own.  Every searched item (the all-samples search, the
search of a group of two or more) that enters the Lambda is granted (|S| + 1) dev_tol: each of its |S| inner searches and its outer
search dev_tol -- their stopping rules bound it.  Every F value that enters adds 2 e_F, e_F = 4 x 9.4e-10 being test_compare_gpu.py's
figure, measured on the existing set solver and not on this code: Lambda_between = 2 (sum_g C(S_g) - C(all)) holds 2 K of them,
Lambda_within = 2 (sum_k F_hat^k - sum_g C(S_g)) two per sample of a group of two or more (a group of one cancels exactly).  w_ref, the
reference's own bound, comes on top.  The common values are compared at 1e-3 relative, test_compare_gpu.py's figure for theta_null,
plus 1e-6 of the outer bracket's width max_k theta_hat^k / s_k - min_k theta_hat^k / s_k: where the maximum lies AT an end of the
bracket (a sample with theta_hat = 0 that pulls the common value to 0) the search closes in on the end and never evaluates it, and 1e-6
of the width is twenty halvings.  theta_hat is compared at 1e-6 relative plus the solver's abs_floor (1e-6), the unit of its stopping
rule: an estimate that decays to 0 is only known to be small.

Every call passes max_iter <= 20000 and the default caps: no workgroup can run long."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import compare_groups_problems as GP
from tests import compare_problems as CP
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TESTED, ALL_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED = range(5)
DEV_TOL = 1e-4
E_F = 4 * 9.4e-10
CAPS = dict(max_iter=20000)
OUTPUTS = H.GROUPS_OUTPUTS + ("theta_group", "theta_hat") + H.GROUPS_COUNTS


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b, emsar_amd.EmsarHip(0) as c, emsar_amd.EmsarHip(0) as d:
        yield a, b, c, d


def load(dev, prob, R, den=None, layout=H.LAYOUT_AUTO, merge_rows=False):
    n_tx, rp, ci, _, E = prob
    dev.upload_structure(n_tx, rp, ci, layout, merge_rows)
    dev.upload_sample(R, E, den)


def same_bits(x, y, keys=OUTPUTS):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def tolerances(groups, w_between, w_within):
    K, G = len(groups), max(groups) + 1
    sizes = [list(groups).count(g) for g in range(G)]
    multi = [n for n in sizes if n >= 2]
    within = sum(n + 1 for n in multi) * DEV_TOL + 2 * E_F * 2 * sum(multi) + w_within
    between = 0.0 if G == 1 else ((K + 1) + sum(n + 1 for n in multi)) * DEV_TOL + 2 * E_F * 2 * K + w_between
    return between, within


def check_against(r, i, ref, groups, what, sizes=None):
    tb, tw = tolerances(groups, ref["w_between"], ref["w_within"])
    print(what, "between", r["lambda_between"][i], "ref", ref["lam_between"], "residual", r["lambda_between"][i] - ref["lam_between"], "tol", tb,
          "| within", r["lambda_within"][i], "ref", ref["lam_within"], "residual", r["lambda_within"][i] - ref["lam_within"], "tol", tw,
          "| common", r["theta_common"][i], ref["theta_common"], "group", r["theta_group"][i], ref["theta_group"],
          "| outer", r["outer"][i], "evals", r["evals"][i], "slope", r["slope"][i])
    assert ref["w_between"] <= GP.W_REF_MAX and ref["w_within"] <= GP.W_REF_MAX
    assert r["status"][i] == TESTED, (what, r["status"][i])
    assert abs(r["lambda_between"][i] - ref["lam_between"]) <= tb, (what, r["lambda_between"][i], ref["lam_between"], tb)
    assert abs(r["lambda_within"][i] - ref["lam_within"]) <= tw, (what, r["lambda_within"][i], ref["lam_within"], tw)
    ends = [x / s for x, s in zip(ref["theta_hat"], sizes or [1.0] * len(groups))]
    width = 1e-6 * (max(ends) - min(ends))
    assert abs(r["theta_common"][i] - ref["theta_common"]) <= 1e-3 * ref["theta_common"] + width, (what, r["theta_common"][i], ref["theta_common"])
    for g, x in enumerate(ref["theta_group"]):
        assert abs(r["theta_group"][i][g] - x) <= 1e-3 * x + width, (what, g, r["theta_group"][i][g], x)
    for k, x in enumerate(ref["theta_hat"]):
        assert abs(r["theta_hat"][i][k] - x) <= 1e-6 * x + 1e-6, (what, k, r["theta_hat"][i][k], x)
    df = (max(groups) + 1 - 1, len(groups) - max(groups) - 1)
    assert r["p_between"][i] == H.compare_groups_pvalue_host([r["lambda_between"][i]], df[0])[0]
    assert r["p_within"][i] == H.compare_groups_pvalue_host([r["lambda_within"][i]], df[1])[0]


@pytest.mark.parametrize("name", GP.CASE_NAMES)
def test_independent_reference(devs, name):
    """every class with K = 3 in two groups, K = 4 in two groups with size factors, K = 3 in three groups; and the split problem, where
    t's set lies in the 64 class in one sample and in the 512 class in the others"""
    prob, Rs, groups, sizes, tids = GP.case_inputs(name)
    den = CP.den_of(prob)
    for dev, R in zip(devs, Rs):
        load(dev, prob, R, den)
    r = devs[0].compare_groups(devs[1:len(Rs)], groups, sizes, tids, tol=1e-12, **CAPS)
    for i, t in enumerate(tids):
        check_against(r, i, GP.recorded()["%s:%d" % (name, t)], groups, (name, t), sizes)
    st = r["stats"].as_dict()
    print(st)
    per_t = 1 + sum(1 for g in range(max(groups) + 1) if 2 <= list(groups).count(g) < len(groups))
    assert st["items_launched"] == per_t * len(tids) and st["evals_sum"] == int(r["evals"].sum()) and st["n_status"]["TESTED"] == len(tids)
    assert st["df_between"] == max(groups) and st["df_within"] == len(groups) - max(groups) - 1


@pytest.mark.parametrize("threads", [64, 256, 512])
def test_two_samples_are_the_compare_statistic(devs, threads):
    """K = 2: groups (0, 1) with sizes (r, 1) is emsar_hip_compare at ratio r reached by another search -- within 3 dev_tol (the two
    inner searches and the outer one here) + dev_tol (the search there); theta_hat has compare's bits; groups (0, 0) puts the same
    statistic into lambda_within"""
    a, b = devs[:2]
    prob, RA, RB, tids = CP.class_problem(threads)
    den = CP.den_of(prob)
    load(a, prob, RA, den)
    load(b, prob, RB, den)
    q = np.unique(np.concatenate([np.array(tids), np.arange(0, prob[0], max(1, prob[0] // 6))])).astype(np.int32)
    for ratio in (1.0, 1.6):
        cmp_ = a.compare(b, q, ratio=ratio, tol=1e-12, **CAPS)
        two = a.compare_groups([b], (0, 1), (ratio, 1.0), q, tol=1e-12, **CAPS)
        one = a.compare_groups([b], (0, 0), (ratio, 1.0), q, tol=1e-12, **CAPS)
        ok = (cmp_["status"] == 0) & (two["status"] == TESTED)
        print(threads, ratio, "tested", ok.sum(), "of", len(q), "max |between - compare|", np.abs(two["lambda_between"][ok] - cmp_["lambda"][ok]).max(),
              "outer max", two["outer"].max(), "evals max", two["evals"].max())
        assert ok.sum() >= len(tids) and np.all(ok[np.isin(q, tids)])
        assert np.all(np.abs(two["lambda_between"][ok] - cmp_["lambda"][ok]) <= 3 * DEV_TOL + DEV_TOL)
        assert two["theta_hat"][:, 0].tobytes() == cmp_["theta_a"].tobytes() and two["theta_hat"][:, 1].tobytes() == cmp_["theta_b"].tobytes()
        assert np.all(two["lambda_within"] == 0.0) and np.all(two["p_within"] == 1.0)
        assert two["stats"].df_between == 1 and two["stats"].df_within == 0
        assert one["lambda_within"].tobytes() == two["lambda_between"].tobytes() and np.all(one["lambda_between"] == 0.0)
        assert one["stats"].df_between == 0 and one["stats"].df_within == 1 and np.all(one["p_between"] == 1.0)
        assert one["theta_common"].tobytes() == two["theta_common"].tobytes() and one["theta_group"][:, 0].tobytes() == one["theta_common"].tobytes()


def test_identical_samples(devs):
    """three contexts holding one sample: both Lambdas exactly 0.0, one outer point, for every transcript"""
    a, b, c = devs[:3]
    prob = SP.all_resident_problem()
    den = CP.den_of(prob)
    for d in (a, b, c):
        load(d, prob, prob[3], den)
    r = a.compare_groups([b, c], (0, 0, 1), max_iter=4000)
    given = ~np.isin(r["status"], (OUTSIDE, NOT_RESIDENT))
    print(r["stats"].as_dict())
    assert given.sum() > 0.9 * prob[0]
    for k in ("lambda_between", "lambda_within", "raw_between", "raw_within", "slope"):
        assert np.all(r[k][given] == 0.0), k
    assert np.all(r["outer"][given] == 1) and np.all(r["p_between"][given] == 1.0) and np.all(r["p_within"][given] == 1.0)
    assert r["theta_hat"][given, 0].tobytes() == r["theta_hat"][given, 1].tobytes() == r["theta_hat"][given, 2].tobytes()
    assert r["theta_common"][given].tobytes() == r["theta_hat"][given, 0].tobytes()
    assert np.all(np.isin(r["status"][given], (TESTED, ALL_ABSENT, UNCONVERGED)))
    assert np.all((r["status"][given] == ALL_ABSENT) == (r["theta_hat"][given, 0] == 0.0))
    assert np.sum(r["status"] == TESTED) > 0.5 * prob[0]


def invariance_samples():
    from tests.test_compare_genes_gpu import invariance_problem
    prob, RA, RB = invariance_problem()
    return prob, [RA, CP.fitted_weights(prob, 43), RB, CP.fitted_weights(prob, 44, apart=range(0, prob[0], 3))]


def test_invariance_bit_for_bit(devs, monkeypatch):
    prob, Rs = invariance_samples()
    den = CP.den_of(prob)
    kw = dict(max_iter=3000)
    groups = (0, 0, 1, 1)
    tids = np.arange(0, prob[0], 7, dtype=np.int32)

    def config(layout, merge, mode):
        if mode is None:
            monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
        else:
            monkeypatch.setenv("EMSAR_HIP_RENUMBER", mode)
        for dev, R in zip(devs, Rs):
            load(dev, prob, R, den, layout, merge)
    config(H.LAYOUT_CSR, False, None)
    a = devs[0]
    before = [d.solve(**kw)[0] for d in devs] + [a.compare(devs[2], tids, **kw)]
    whole = a.compare_groups(devs[1:], groups, **kw)
    after = [d.solve(**kw)[0] for d in devs] + [a.compare(devs[2], tids, **kw)]
    for x, y in zip(before[:4], after[:4]):
        assert x.tobytes() == y.tobytes()
    assert not [k for k in H.COMPARE_OUTPUTS + ("status", "evals") if before[4][k].tobytes() != after[4][k].tobytes()]
    st = whole["stats"].as_dict()
    print(st)
    assert st["n_status"]["TESTED"] >= 30 and st["n_status"]["TESTED"] + st["n_status"]["UNCONVERGED"] == prob[0]
    assert st["evals_max"] <= 4 * 12 * 40 and st["outer_max"] <= 12 and st["items_launched"] <= 3 * prob[0]
    q = np.random.default_rng(5).permutation(prob[0]).astype(np.int32)
    shuffled = a.compare_groups(devs[1:], groups, None, q, **kw)
    twice = a.compare_groups(devs[1:], groups, None, np.concatenate([q[:30], q[:30], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_GROUPS_BATCH", "1")            # one item per class and launch
    single = a.compare_groups(devs[1:], groups, None, q[:25], **kw)
    monkeypatch.delenv("EMSAR_HIP_GROUPS_BATCH")
    swapped = a.compare_groups(devs[1:], (1, 1, 0, 0), **kw)
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][60:].tobytes() == shuffled[k].tobytes() and twice[k][:30].tobytes() == twice[k][30:60].tobytes() == shuffled[k][:30].tobytes(), k
        assert single[k].tobytes() == shuffled[k][:25].tobytes(), k
        if k != "theta_group":
            assert swapped[k].tobytes() == whole[k].tobytes(), k
    assert swapped["theta_group"][:, ::-1].tobytes() == whole["theta_group"].tobytes()
    assert sum(twice["stats"].as_dict()["n_status"].values()) == prob[0]
    for layout, merge, mode in ((H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"), (H.LAYOUT_TILED, True, "2")):
        config(layout, merge, mode)
        assert not same_bits(a.compare_groups(devs[1:], groups, **kw), whole), (layout, merge, mode)
    monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
    load(devs[1], prob, Rs[1], den, H.LAYOUT_CSR)                 # the contexts need not share a layout
    assert not same_bits(a.compare_groups(devs[1:], groups, **kw), whole)


def test_statuses_and_host_paths(devs):
    a, b, c = devs[:3]
    prob, Rs, dens = GP.small_samples()
    for d, R, den in zip((a, b, c), Rs, dens):
        load(d, prob, R, den)
    groups = (0, 0, 1)
    r = a.compare_groups([b, c], groups, tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    # closed form in every sample: the host's searches, the bits of the diagnostic entry the CPU test checks against the closed form
    for t in (0, 1, 8, 9):
        want = H.debug_compare_groups_closed([float(R[t]) if t < 2 else 0.0 for R in Rs], [d[t] for d in dens], groups)    # rows 0, 1 hold 0, 1 alone
        for k in OUTPUTS:
            assert np.asarray(r[k][t]).tobytes() == np.asarray(want[k], dtype=r[k].dtype).tobytes(), (t, k, r[k][t], want[k])
    assert r["status"][0] == TESTED and r["lambda_between"][0] > 0.0
    assert r["status"][1] == TESTED and r["lambda_between"][1] == 0.0 and r["lambda_within"][1] == 0.0 and r["outer"][1] == 1
    for t in (8, 9):
        assert r["status"][t] == ALL_ABSENT and r["lambda_between"][t] == 0.0 and r["lambda_within"][t] == 0.0
        assert r["p_between"][t] == 1.0 and r["p_within"][t] == 1.0 and r["outer"][t] == 1
    # 2: theta_hat = 0 in exactly one sample (closed form without a read in C, closed form in A, in a set in B): the root of C's inner
    # search is the end of its range; 6: theta_hat = 0 inside a set in B; 3, 4, 5, 7: families
    for t in (2, 3, 4, 5, 6, 7):
        ref = GP.reference(prob, Rs, dens, groups, None, t)
        assert ref["ended_by_step"]
        check_against(r, t, ref, groups, ("small", t))
    assert r["theta_hat"][2][2] == 0.0 and r["theta_hat"][2][0] > 0.0 and r["theta_hat"][2][1] > 0.0
    assert r["theta_hat"][6][1] == 0.0 and r["theta_hat"][6][0] * dens[0][6] >= 20
    # den = 0 in one sample
    assert r["status"][10] == OUTSIDE and r["outer"][10] == 0 and r["evals"][10] == 0
    for k in H.GROUPS_OUTPUTS:
        assert math.isnan(r[k][10]), k
    assert np.all(np.isnan(r["theta_group"][10])) and np.all(np.isnan(r["theta_hat"][10]))
    st = r["stats"].as_dict()
    print(st)
    dev = np.array([2, 3, 4, 5, 6, 7])
    assert sum(st["n_status"].values()) == prob[0] and st["n_status"]["OUTSIDE"] == 1 and st["n_status"]["ALL_ABSENT"] == 2
    assert st["items_launched"] == 2 * len(dev)                   # the all-samples search and group 0's; the rest never reaches the device
    assert st["evals_sum"] == int(r["evals"][dev].sum()) and st["outer_sum"] >= int(r["outer"][dev].sum())
    assert st["outer_max"] >= int(r["outer"][dev].max()) and st["evals_max"] <= int(r["evals"][dev].max()) and st["passes_max"] <= st["passes_sum"]
    only = a.compare_groups([b, c], groups, None, [3], tol=1e-12, **CAPS)
    more = a.compare_groups([b, c], groups, None, [3, 0, 1, 8, 10], tol=1e-12, **CAPS)
    assert only["stats"].items_launched == more["stats"].items_launched == 2 and not same_bits({k: v[:1] for k, v in more.items() if k != "stats"}, only)
    # the caps: two outer points are not enough where the samples differ
    capped = a.compare_groups([b, c], groups, max_outer=2, tol=1e-12, **CAPS)
    moved = np.flatnonzero((r["status"] == TESTED) & (r["outer"] > 2))
    assert len(moved) >= 4 and np.all(capped["status"][moved] == UNCONVERGED) and np.all(capped["outer"][moved] == 2)
    assert capped["theta_hat"].tobytes() == r["theta_hat"].tobytes()
    # not resident
    nr = a.compare_groups([b, c], groups, set_mode=1, **CAPS)
    assert np.all(nr["status"] == NOT_RESIDENT) and nr["stats"].items_launched == 0 and np.all(nr["evals"] == 0)
    for k in H.GROUPS_OUTPUTS:
        assert np.all(np.isnan(nr[k])), k


def test_argument_errors(devs):
    a, b, c = devs[:3]
    prob, Rs, dens = GP.small_samples()
    for d, R, den in zip((a, b, c), Rs, dens):
        load(d, prob, R, den)
    ok = dict(groups=(0, 0, 1))
    for bad in (dict(groups=(0, 0, 2)), dict(groups=(0, -1, 1)), dict(groups=(1, 1, 1)), dict(groups=(0, 1, 3)), dict(ok, sizes=(1.0, 0.0, 1.0)),
                dict(ok, sizes=(1.0, -2.0, 1.0)), dict(ok, sizes=(1.0, math.inf, 1.0)), dict(ok, sizes=(1.0, math.nan, 1.0)), dict(ok, query=[0, 11]),
                dict(ok, query=[-1]), dict(ok, dev_tol=math.inf), dict(ok, dev_tol=math.nan), dict(ok, set_mode=2), dict(ok, count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups([b, c], **bad, **CAPS)
        assert e.value.status == -1, bad
    for others, groups in (([b, a], (0, 0, 1)), ([b, b], (0, 0, 1)), ([b, None], (0, 0, 1)), ([], (0,))):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups(others, groups, **CAPS)
        assert e.value.status == -1, (others, groups)
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_groups([b] * 32, [0] * 33, **CAPS)              # K = 33 (and contexts given twice)
    assert e.value.status == -1
    with emsar_amd.EmsarHip(0) as d:
        d.upload_structure(prob[0], prob[1], prob[2])
        for first, others in ((a, [b, d]), (d, [a, b])):
            with pytest.raises(emsar_amd.EmsarHipError) as e:
                first.compare_groups(others, (0, 0, 1), **CAPS)
            assert e.value.status == -5                           # before upload_sample
        n_tx, rp, ci = CP.csr([[0, 1], [1, 2]], prob[0])
        d.upload_structure(n_tx, rp, ci)
        d.upload_sample()
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups([b, d], (0, 0, 1), **CAPS)
        assert e.value.status == -1                               # another structure


def test_cli_groups_file(tmp_path):
    """-M --compare-groups 0,0,1 on the syn300_se fixture, every second and every third read of it: out.groups has one line per
    transcript and its columns are the Python call's as printed; every other file has the bytes of a run without the switch"""
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
    alns = [tmp_path / "full.bowtie.gz", tmp_path / "half.bowtie.gz", tmp_path / "third.bowtie.gz"]
    for path, keep in zip(alns, (set(names), set(names[::2]), set(names[::3]))):
        with gzip.open(path, "wt") as f:
            f.write("".join(l for l in lines if l.split("\t")[0] in keep))
    lst = tmp_path / "samples.list"
    lst.write_text("".join(str(p) + "\n" for p in alns))
    groups, sizes = (0, 0, 1), (1.0, 0.5, 0.4)
    base = [_build.CLI, "-q", "-i", "20000"] + fx.meta["opts"] + ["-M", "--gpus", "1"]
    subprocess.run(base + ["-I", rsh_path, str(tmp_path / "p"), "out", str(lst)], check=True, timeout=300)
    subprocess.run(base + ["--compare-groups", "0,0,1", "--compare-sizes", "1,0.5,0.4", "-I", rsh_path, str(tmp_path / "o"), "out", str(lst)], check=True,
                   timeout=300)
    plain, with_groups = sorted(os.listdir(tmp_path / "p")), sorted(os.listdir(tmp_path / "o"))
    assert with_groups == sorted(plain + ["out.groups"]) and len(plain) >= 6
    for name in plain:
        assert (tmp_path / "o" / name).read_bytes() == (tmp_path / "p" / name).read_bytes(), name
    text = (tmp_path / "o" / "out.groups").read_text().splitlines()
    assert text[0] == "# samples=3 groups=0,0,1 sizes=1,0.5,0.4 df_between=1 df_within=1"
    assert text[1].split("\t") == ["transcript", "FPKM_common", "FPKM_g0", "FPKM_g1", "Lambda_between", "df", "p_between", "Lambda_within", "df", "p_within",
                                   "status", "outer", "evals"]
    got = [l.split("\t") for l in text[2:]]
    rsh = HL.HostRsh(rsh_path)
    assert len(got) == rsh.n_tx and all(len(r) == 13 for r in got) and [r[0] for r in got] == list(rsh.names)
    # what the CLI does for the three samples, through the Python bindings
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=20000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
    rows = np.repeat(np.arange(rsh.n_rows), np.diff(rp.astype(np.int64)))
    with emsar_amd.EmsarHip(0) as d0, emsar_amd.EmsarHip(0) as d1, emsar_amd.EmsarHip(0) as d2:
        for d, path in ((d0, alns[0]), (d1, alns[1]), (d2, alns[2])):
            cnt = rsh.count(str(path), fmt=fmt)
            d.set_deterministic(True)
            d.upload_structure(rsh.n_tx, rp, ci)
            d.upload_euma(rsh.euma)
            E = np.array(rsh.model(cnt, L=d.adj_euma(rsh.wf(cnt))).E_solver)
            den = np.zeros(rsh.n_tx)
            keep_e = E[rows] != 0.0
            np.add.at(den, ci[keep_e], E[rows][keep_e])
            d.upload_sample(np.array(cnt.R), E, den)
        p = d0.compare_groups([d1, d2], groups, sizes, **cli)
    print(p["stats"].as_dict())
    assert [r[10] for r in got] == [H.GROUPS_STATUS[k] for k in p["status"]]
    assert [int(r[11]) for r in got] == list(p["outer"]) and [int(r[12]) for r in got] == list(p["evals"])
    assert all(r[5] == "1" and r[8] == "1" for r in got)
    show = lambda x, fmt: "nan" if math.isnan(x) else ("-inf" if x < 0 else "inf") if math.isinf(x) else fmt % x
    for col, key, fmt_ in ((1, "theta_common", "%f"), (4, "lambda_between", "%f"), (6, "p_between", "%.6g"), (7, "lambda_within", "%f"), (9, "p_within", "%.6g")):
        assert [r[col] for r in got] == [show(x, fmt_) for x in p[key]], key
    for g in (0, 1):
        assert [r[2 + g] for r in got] == [show(x, "%f") for x in p["theta_group"][:, g]], g
    assert np.sum(p["status"] == TESTED) >= 10
