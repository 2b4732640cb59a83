"""GPU: the profile-likelihood intervals (emsar_hip_profile, include/emsar_hip.h "profile-likelihood intervals") against closed-form
profiles, against a pinned EM on the CPU oracle (tests/profile_problems.py: no multiplier in it), against solve and the presence test for
bit-identity and side effects, for independence of the query's shape, for nesting in the level, on the paths that are not searched, and
through the CLI.

The deviance tolerance of the oracle comparison (test_against_the_oracle) is derived, not tuned: the pinned reference's own deviance,
computed at tol 1e-10 and at 1e-13 on exactly these problems, queries and (its own) limits at level 0.95, disagrees by at most
3.87e-15 * (|F_full| + |F_pinned|) (measured on the CPU by `python -m tests.profile_problems` over 215 limits; the worst case is the
900-transcript set, a few ulp of F as two sums of ~10^3 terms give).  The test allows 100 x that spread, LAMBDA_REL = 3.9e-13 of
(|F_full| + |F_pinned|), plus 1e-7 * q for the solver's stopping rule.  Level 0.95 alone gives the reference 69 TWO_SIDED and 77 LOWER_ZERO queries
on these problems, so no second level is run.

Every call passes max_iter <= 20000 and max_evals <= 30: no workgroup can run long."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import profile_problems as PP
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED = range(5)
LAMBDA_SPREAD = 3.9e-15          # the pinned reference against itself, tol 1e-10 vs 1e-13, relative to |F_full| + |F_pinned| (3.87e-15 measured)
LAMBDA_REL = 100 * LAMBDA_SPREAD
DEV_TOL = 1e-4                   # the default of emsar_profile_params.dev_tol
LEVEL = 0.95
CAPS = dict(max_iter=20000, max_evals=30)
OUTPUTS = ("lower", "upper", "dev_lower", "dev_upper", "lambda", "theta_hat", "status", "evals")


def csr(rows, n_tx):
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return n_tx, rp, np.concatenate([np.array(r, dtype=np.int32) for r in rows]).astype(np.int32)


@pytest.fixture(scope="module")
def dev():
    with emsar_amd.EmsarHip(0) as d:
        yield d


def load(dev, prob, den=None):
    n_tx, rp, ci, R, E = prob
    dev.upload_structure(n_tx, rp, ci)
    dev.upload_sample(R, E, den)


def on_the_cut(dev_value, q):
    return abs(dev_value - q) <= DEV_TOL * q


def test_closed_form_components(dev):
    """one-transcript components: F(x) = u log x - x den, searched on the host; u = 0 gives (0, q / (2 den))"""
    n_tx, rp, ci = csr([[0], [1], [2, 3]], 4)
    load(dev, (n_tx, rp, ci, np.array([100, 0, 5], dtype=np.int32), np.ones(3)), np.array([2.0, 0.5, 1.0, 1.0]))
    r = dev.profile(level=LEVEL, **CAPS)
    q = H.profile_cut_host(LEVEL)
    assert r["stats"].cut == q
    print({k: r[k] for k in OUTPUTS})
    assert r["status"][1] == LOWER_ZERO and r["lower"][1] == 0.0 and r["lambda"][1] == 0.0 and r["dev_lower"][1] == 0.0
    assert abs(r["upper"][1] - q / (2 * 0.5)) <= DEV_TOL * q / (2 * 0.5)
    assert r["status"][0] == TWO_SIDED and r["lambda"][0] == np.inf and r["theta_hat"][0] == 50.0
    D = lambda x: 2 * (100 * math.log(50 / x) - 2 * (50 - x))
    assert 0 < r["lower"][0] < 50 < r["upper"][0]
    for k in ("lower", "upper"):
        assert on_the_cut(D(r[k][0]), q), (k, r[k][0], D(r[k][0]), q)
        assert abs(D(r[k][0]) - r["dev_" + k][0]) <= 1e-9, (k, D(r[k][0]), r["dev_" + k][0])
    # the pair {2,3} shares its only row: each can be absent, each can hold all five reads and more
    assert list(r["status"][2:]) == [LOWER_ZERO, LOWER_ZERO] and np.all(r["upper"][2:] > 5.0) and np.all(r["lower"][2:] == 0.0)


@pytest.mark.parametrize("level", [0.95, 0.99])
def test_two_transcripts_closed_form_profile(dev, level):
    """rows {a}: 30 and {a,b}: 50 with E = 1: den = (2, 1), theta_hat = (30, 20).  With b pinned at x the best a solves
    2 a^2 - (80 - 2 x) a - 30 x = 0; with a pinned at x the best b is max(50 - x, 0)"""
    n_tx, rp, ci = csr([[0], [0, 1]], 2)
    load(dev, (n_tx, rp, ci, np.array([30, 50], dtype=np.int32), np.ones(2)))
    r = dev.profile(level=level, tol=1e-13, **CAPS)
    q = H.profile_cut_host(level)
    F = lambda a, b: 30 * math.log(a) + 50 * math.log(a + b) - 2 * a - b
    F_hat = F(30.0, 20.0)
    D_b = lambda x: 2 * (F_hat - F(((80 - 2 * x) + math.sqrt((2 * x - 80) ** 2 + 240 * x)) / 4, x))
    D_a = lambda x: 2 * (F_hat - F(x, max(50 - x, 0.0)))
    lam_b = 2 * (30 * math.log(30) + 50 * math.log(50) - 80 * math.log(40))
    print(level, {k: r[k] for k in OUTPUTS}, "Lambda_b", lam_b)
    np.testing.assert_allclose(r["theta_hat"], [30.0, 20.0], rtol=1e-9)
    assert r["lambda"][0] == np.inf and abs(r["lambda"][1] - lam_b) <= 1e-9 * lam_b
    searched = [(0, "lower", D_a), (0, "upper", D_a), (1, "upper", D_b)]
    if level == 0.95:
        assert list(r["status"]) == [TWO_SIDED, TWO_SIDED]
        searched.append((1, "lower", D_b))
    else:
        assert q > lam_b and list(r["status"]) == [TWO_SIDED, LOWER_ZERO]
        assert r["lower"][1] == 0.0 and r["dev_lower"][1] == r["lambda"][1]
    for t, k, D in searched:
        x, dv = r[k][t], r["dev_" + k][t]
        assert x > 0 and on_the_cut(dv, q), (t, k, x, dv, q)
        assert abs(D(x) - dv) <= 1e-9 * max(1.0, dv), (t, k, x, D(x), dv)
    assert np.all(r["lower"] <= r["theta_hat"]) and np.all(r["theta_hat"] <= r["upper"])
    assert r["stats"].evals_sum == int(np.sum(r["evals"])) and r["stats"].evals_max <= 30


def excluded(lam, scale, q):
    """a reference Lambda too close to the cut for the status to be the reference's to decide"""
    return abs(lam - q) <= LAMBDA_REL * scale + 1e-7 * q


@pytest.mark.parametrize("name", list(PP.ORACLE_CASES))
def test_against_the_oracle(dev, name):
    """statuses exactly; every searched limit lies on the reference's profile curve within LAMBDA_REL * (|F_full| + |F_pinned|) + 1e-7 q
    (module docstring) and on the cut within dev_tol; lower <= theta_hat <= upper"""
    prob, ref, tids, lam = PP.oracle_case(name)
    load(dev, prob)
    r = dev.profile(tids, level=LEVEL, tol=1e-12, **CAPS)
    q = H.profile_cut_host(LEVEL)
    worst = 0.0
    for i, (t, (lm, scale)) in enumerate(zip(tids, lam)):
        if lm != lm:
            assert r["status"][i] == OUTSIDE, (name, int(t))
            continue
        if excluded(lm, scale, q):
            continue
        want = LOWER_ZERO if lm <= q else TWO_SIDED
        assert r["status"][i] == want, (name, int(t), int(r["status"][i]), lm, r["lambda"][i])
        assert r["lower"][i] <= r["theta_hat"][i] <= r["upper"][i], (name, int(t))
        if want == LOWER_ZERO:
            assert r["lower"][i] == 0.0 and r["dev_lower"][i] == r["lambda"][i]
        for k in (("lower", "upper") if want == TWO_SIDED else ("upper",)):
            x, dv = r[k][i], r["dev_" + k][i]
            d_ref, sc = ref.deviance(int(t), float(x))
            bound = LAMBDA_REL * sc + 1e-7 * q
            worst = max(worst, abs(d_ref - dv) / bound)
            assert on_the_cut(dv, q), (name, int(t), k, x, dv, q)
            assert abs(d_ref - dv) <= bound, (name, int(t), k, x, d_ref, dv, bound)
    st = r["stats"].as_dict()
    print(name, "queried", len(tids), "worst |dD| / bound", worst, "evals mean", st["evals_sum"] / max(1, np.sum(r["evals"] > 0)), "max", st["evals_max"],
          "passes max", st["passes_max"], st["n_status"])


def test_the_reference_decides_both_kinds_and_few_queries_are_excluded():
    """the reference alone, at LEVEL: at least 5 TWO_SIDED and 5 LOWER_ZERO queries, and at most 1 query in 20 so close to the cut that
    it is left out"""
    q = PP.cut(LEVEL)
    two = zero = out = total = 0
    for name in PP.ORACLE_CASES:
        for lm, scale in PP.oracle_case(name)[3]:
            if lm != lm:
                continue
            total += 1
            if excluded(lm, scale, q):
                out += 1
            elif lm > q:
                two += 1
            else:
                zero += 1
    print("two-sided", two, "lower-zero", zero, "excluded", out, "of", total)
    assert two >= 5 and zero >= 5 and 20 * out <= total, (two, zero, out, total)


def test_consistency_with_solve_and_presence(dev):
    prob = SP.all_resident_problem()
    load(dev, prob)
    kw = dict(max_iter=4000)
    before, _ = dev.solve(**kw)
    theta0 = dev.get_theta()
    q = np.random.default_rng(11).choice(prob[0], size=120, replace=False).astype(np.int32)
    pres0 = dev.presence(q, **kw)
    r = dev.profile(q, level=LEVEL, max_evals=30, **kw)
    assert dev.get_theta().tobytes() == theta0.tobytes()
    after, _ = dev.solve(**kw)
    assert after.tobytes() == before.tobytes()
    pres1 = dev.presence(q, **kw)
    for k in ("lambda", "pvalue", "heir", "heir_share", "status", "theta_hat"):
        assert pres1[k].tobytes() == pres0[k].tobytes(), k
    known = np.isin(pres0["status"], (0, 1, 2))            # TESTED, ABSENT, ESSENTIAL
    assert known.sum() > 60
    assert r["lambda"][known].tobytes() == pres0["lambda"][known].tobytes()
    given = ~np.isin(r["status"], (OUTSIDE, NOT_RESIDENT))
    assert given.sum() > 60 and r["theta_hat"][given].tobytes() == before[q][given].tobytes()
    st = r["stats"].as_dict()
    print(st)
    assert st["n_status"]["TWO_SIDED"] > 0 and st["n_status"]["LOWER_ZERO"] > 0 and sum(st["n_status"].values()) == len(q)
    assert st["evals_max"] <= 30 and st["evals_sum"] == int(np.sum(r["evals"])) and st["passes_sum"] >= st["passes_max"] > 0
    assert st["items_launched"] > pres0["stats"].items_launched


def test_independence_of_the_query(dev, monkeypatch):
    prob = SP.all_resident_problem()
    load(dev, prob)
    kw = dict(level=LEVEL, max_iter=4000, max_evals=30)
    q = np.random.default_rng(11).choice(prob[0], size=120, replace=False).astype(np.int32)
    whole = dev.profile(q, **kw)
    halves = [dev.profile(q[:60], **kw), dev.profile(q[60:], **kw)]
    rev = dev.profile(q[::-1].copy(), **kw)
    twice = dev.profile(np.concatenate([q[:40], q[:40], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_PROFILE_BATCH", "7")           # many launches per class instead of one
    small = dev.profile(q, **kw)
    monkeypatch.delenv("EMSAR_HIP_PROFILE_BATCH")
    for k in OUTPUTS:
        assert np.concatenate([h[k] for h in halves]).tobytes() == whole[k].tobytes(), k
        assert rev[k][::-1].tobytes() == whole[k].tobytes(), k
        assert twice[k][80:].tobytes() == whole[k].tobytes() and twice[k][:40].tobytes() == twice[k][40:80].tobytes() == whole[k][:40].tobytes(), k
        assert small[k].tobytes() == whole[k].tobytes(), k
    assert sum(twice["stats"].as_dict()["n_status"].values()) == len(q)


def test_intervals_nest_in_the_level(dev):
    """the wider level's interval contains the narrower one's, up to a relative 1e-3 of its width (dev_tol seen through the curve)"""
    prob = SP.ragged_problem()
    load(dev, prob)
    rs = [dev.profile(level=lv, **CAPS) for lv in (0.8, 0.95, 0.99)]
    for narrow, wide in zip(rs, rs[1:]):
        ok = ~np.isin(narrow["status"], (OUTSIDE, NOT_RESIDENT))
        assert ok.sum() >= 50 and not np.any(narrow["status"] == UNCONVERGED) and not np.any(wide["status"] == UNCONVERGED)
        margin = 1e-3 * (wide["upper"] - wide["lower"])[ok]
        assert np.all(wide["lower"][ok] <= narrow["lower"][ok] + margin)
        assert np.all(wide["upper"][ok] >= narrow["upper"][ok] - margin)
        assert np.all(wide["upper"][ok] > wide["lower"][ok])


def test_other_paths_and_errors(dev):
    prob = SP.everything_problem()
    n_tx, rp, ci, R, E = prob
    load(dev, prob)
    info = H.sets_selfcheck(n_tx, rp, ci, np.where(E > 0, R, 0))
    assert info["sets_streamed"] == 1
    q = np.random.default_rng(3).choice(n_tx, size=200, replace=False).astype(np.int32)
    r = dev.profile(q, max_iter=3000, max_evals=30)
    pres = dev.presence(q, max_iter=3000)
    nr = r["status"] == NOT_RESIDENT
    assert 0 < nr.sum() < len(q) and np.array_equal(nr, pres["status"] == 4)
    for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda", "theta_hat"):
        assert np.all(np.isnan(r[k][nr])), k
    assert np.all(r["evals"][nr] == 0)
    r1 = dev.profile(q[:20], set_mode=1, **CAPS)
    assert np.all(r1["status"] == NOT_RESIDENT) and r1["stats"].items_launched == 0 and np.all(np.isnan(r1["upper"]))
    # den = 0: outside the likelihood; one evaluation per search: unconverged, with values
    rows = [[0, 1], [0, 0], [2, 3], [2, 8], [4, 5], [5, 6], [4, 6], [4, 5, 6], [7], [8, 2, 3]]
    Rw = np.array([9, 4, 6, 5, 7, 0, 3, 11, 2, 3], dtype=np.int32)
    n_tx, rp, ci = csr(rows, 9)
    den = np.array([2.0, 1.0, 2.0, 0.0, 3.0, 3.0, 3.0, 0.0, 0.5])
    load(dev, (n_tx, rp, ci, Rw, np.ones(len(rows))), den)
    r = dev.profile(**CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert r["status"][3] == OUTSIDE and r["status"][7] == OUTSIDE
    for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda", "theta_hat"):
        assert np.all(np.isnan(r[k][[3, 7]])), k
    inside = [0, 1, 2, 4, 5, 6, 8]
    assert np.all(np.isin(r["status"][inside], (TWO_SIDED, LOWER_ZERO)))
    assert r["status"][0] == TWO_SIDED and r["lambda"][0] == np.inf and r["status"][2] == TWO_SIDED and r["lambda"][2] == np.inf
    q = H.profile_cut_host(0.95)
    for t in inside:
        assert on_the_cut(r["dev_upper"][t], q) and (r["status"][t] == LOWER_ZERO or on_the_cut(r["dev_lower"][t], q)), t
    r = dev.profile(max_iter=20000, max_evals=1)
    assert np.all(r["status"][inside] == UNCONVERGED) and np.all(r["evals"][inside] >= 1) and np.all(r["evals"][inside] <= 2)
    for k in ("upper", "dev_upper", "theta_hat"):
        assert np.all(np.isfinite(r[k][inside])), k
    assert np.all(np.isfinite(r["lower"][inside])) and np.all(r["upper"][inside] >= r["theta_hat"][inside])
    for bad in (dict(query=[0, 9]), dict(query=[-1]), dict(level=0.0), dict(level=1.0), dict(level=math.nan), dict(dev_tol=math.inf)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            dev.profile(**bad, **CAPS)
        assert e.value.status == -1, bad
    with emsar_amd.EmsarHip(0) as d:
        d.upload_structure(*csr([[0, 1]], 2))
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            d.profile(**CAPS)
        assert e.value.status == -5


def test_cli_profile_file(tmp_path):
    """--profile on a golden fixture: the .profile file's columns are the Python call's, the other files do not change"""
    from emsar_amd import _build
    from emsar_amd import hostlib as HL
    from tests.conftest import aln_path, get_fixture
    _build.build_all()
    fx = get_fixture("syn300_se")
    aln, fmt = aln_path(fx.dir)
    rsh_path = os.path.join(fx.dir, "index.rsh")
    for tag, extra in (("a", []), ("b", ["--profile", "--profile-evals", "30"])):
        subprocess.run([_build.CLI, "-q", "-g", "-i", "20000"] + fx.meta["opts"] + extra + ["-I", rsh_path, str(tmp_path / tag), "out", aln], check=True, timeout=300)
    a, b = tmp_path / "a", tmp_path / "b"
    for ext in ("fpkm", "fraglength_effect", "segments"):
        assert (a / ("out.0." + ext)).read_bytes() == (b / ("out.0." + ext)).read_bytes(), ext
    assert not (a / "out.0.profile").exists()
    # what the CLI does for the sample, through the Python bindings: count, model, den in row order on the host, its solver settings
    rsh = HL.HostRsh(rsh_path)
    cnt = rsh.count(aln, fmt=fmt)
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=20000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
    with emsar_amd.EmsarHip(0) as d:
        d.set_deterministic(True)
        d.upload_structure(rsh.n_tx, rp, ci)
        d.upload_euma(rsh.euma)
        E = np.array(rsh.model(cnt, L=d.adj_euma(rsh.wf(cnt))).E_solver)
        den = np.zeros(rsh.n_tx)
        rows = np.repeat(np.arange(rsh.n_rows), np.diff(rp.astype(np.int64)))
        keep = E[rows] != 0.0
        np.add.at(den, ci[keep], E[rows][keep])
        d.upload_sample(np.array(cnt.R), E, den)
        p = d.profile(max_evals=30, **cli)
    lines = (b / "out.0.profile").read_text().splitlines()
    assert lines[0].split("\t") == ["tid", "transcriptID", "FPKM", "lower", "upper", "Lambda", "status"]
    got = [l.split("\t") for l in lines[1:]]
    text = [l.split("\t") for l in (b / "out.0.fpkm").read_text().splitlines()[1:]]
    assert len(got) == rsh.n_tx and all(len(r) == 7 for r in got)
    assert [int(r[0]) for r in got] == list(range(rsh.n_tx)) and [r[1:3] for r in got] == [t[:2] for t in text]
    assert [r[6] for r in got] == [H.PROFILE_STATUS[k] for k in p["status"]]
    for col, key in ((3, "lower"), (4, "upper"), (5, "lambda")):
        v = np.array([float(r[col]) for r in got])
        fin = np.isfinite(p[key])
        assert np.array_equal(np.isinf(v), np.isinf(p[key])) and np.array_equal(np.isnan(v), np.isnan(p[key])), key
        assert np.all(np.abs(v[fin] - p[key][fin]) <= 1e-6 + 1e-15 * np.abs(p[key][fin])), key          # "%lf"
    assert np.sum(p["status"] == TWO_SIDED) >= 10 and np.sum(p["status"] == LOWER_ZERO) >= 10
    # a list: the named transcripts only, in the list's order
    lst = tmp_path / "names.txt"
    pick = [int(t) for t in np.flatnonzero(p["status"] == TWO_SIDED)[:3][::-1]]
    lst.write_text("".join(rsh.names[t] + "\n" for t in pick))
    subprocess.run([_build.CLI, "-q", "-i", "20000"] + fx.meta["opts"] + ["--profile", "--profile-evals", "30", "--profile-list", str(lst), "-I", rsh_path, str(tmp_path / "c"), "out", aln],
                   check=True, timeout=300)
    short = [l.split("\t") for l in (tmp_path / "c" / "out.0.profile").read_text().splitlines()[1:]]
    assert short == [got[t] for t in pick]
