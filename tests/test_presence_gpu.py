"""GPU: the presence test (emsar_hip_presence, include/emsar_hip.h "presence test") -- a likelihood-ratio test of every transcript on
its own connected set -- against a closed-form answer, against the CPU oracle solving the matrix with the transcript's entries
deleted, on hand-made edge rows, for independence of the query's shape, for side effects on the context, and through the CLI.

The Lambda tolerance of the oracle comparison (test_against_the_oracle) is derived, not tuned: the oracle's own Lambda, computed with
em_solve at tol 1e-10 and at 1e-13 on exactly these problems and queries, disagrees by at most 4.26e-15 * (|F_full| + |F_drop|)
(measured on the CPU over 214 tested transcripts, |F_full| + |F_drop| up to 1.5e5, i.e. 6.4e-10 in Lambda; the worst case is the
900-transcript set).  The test allows 100 x that spread, LAMBDA_REL = 4.3e-13 of (|F_full| + |F_drop|), plus 1e-7 * Lambda for the
solver's stopping rule.  The oracle's EM at tol 1e-12 is what the two large cases cost: about 0.7 s per solve of the 250- and the
900-transcript set, ten solves each."""
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
import oracle
from emsar_amd import hip as H
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TESTED, ABSENT, ESSENTIAL, OUTSIDE, NOT_RESIDENT, UNCONVERGED = range(6)
LAMBDA_SPREAD = 4.3e-15          # the oracle against itself, tol 1e-10 vs 1e-13, relative to |F_full| + |F_drop| (4.26e-15 measured)
LAMBDA_REL = 100 * LAMBDA_SPREAD
QUERY_SEED = 5                   # with it the reference's heirs are clear in 188 of the 214 tested queries (checked on the CPU; 3/4 are asked for)
# problems of the oracle comparison: name -> (problem, how many transcripts to query: None = all of them)
ORACLE_CASES = {
    "ragged60": (SP.ragged_problem, None),
    "edge0_c0": (lambda: SP.edge_problem(0), None), "edge2_c0": (lambda: SP.edge_problem(2), None),
    "edge1_c1": (lambda: SP.edge_problem(1), None), "edge3_c1": (lambda: SP.edge_problem(3), None),
    "edge6_c1": (lambda: SP.edge_problem(6), None), "edge4_c1_250": (lambda: SP.edge_problem(4), 8),
    "edge8_c2_900": (lambda: SP.edge_problem(8), 8),
}


def csr(rows, n_tx):
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return n_tx, rp, np.concatenate([np.array(r, dtype=np.int32) for r in rows]).astype(np.int32)


def drop_matrix(rp, ci, R, E, t):
    """the CSR with t's entries deleted, and whether a row inside the likelihood with reads has no entry left"""
    keep = ci != t
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp).astype(np.int64))
    cnt = np.bincount(rows[keep], minlength=len(rp) - 1)
    had = np.diff(rp).astype(np.int64) > 0
    rp2 = np.zeros(len(rp), dtype=np.uint64)
    rp2[1:] = np.cumsum(cnt)
    stranded = bool(np.any(had & (cnt == 0) & (np.asarray(R) > 0) & (np.asarray(E) > 0)))
    return rp2, ci[keep], stranded


def full_solve(prob, tol=1e-12):
    n_tx, rp, ci, R, E = prob
    full = oracle.Csr(n_tx, rp, ci, R=R, E=E)
    th, _ = full.em_solve(tol=tol)
    return th, full.loglik(th), full.den()


def reference(prob, tids, base, tol=1e-12):
    """per queried transcript: status, Lambda, |F_full| + |F_drop|, heir, whether the heir is clear (the best gain exceeds the
    runner-up by 1 % of theta_t den_t), from oracle.Csr on the full matrix (base = full_solve at the same tol) and on the matrix with
    the transcript's entries deleted"""
    n_tx, rp, ci, R, E = prob
    th, F, den = base
    out = []
    for t in tids:
        reads = th[t] * den[t]
        if den[t] == 0:
            out.append(dict(status=OUTSIDE))
            continue
        if reads < 1e-9:
            out.append(dict(status=ABSENT, lam=0.0))
            continue
        rp2, ci2, stranded = drop_matrix(rp, ci, R, E, t)
        if stranded:
            out.append(dict(status=ESSENTIAL, lam=np.inf))
            continue
        sub = oracle.Csr(n_tx, rp2, ci2, R=R, E=E)
        th2, _ = sub.em_solve(tol=tol)
        F2 = sub.loglik(th2)
        gain = (th2 - th) * den
        gain[t] = -np.inf
        order = np.argsort(-gain, kind="stable")
        best, second = gain[order[0]], gain[order[1]] if n_tx > 2 else -np.inf
        out.append(dict(status=TESTED, lam=max(0.0, 2 * (F - F2)), scale=abs(F) + abs(F2), heir=int(order[0]) if best > 0 else -1,
                        share=best / reads, clear=bool(best > 0 and best - max(second, 0.0) > 0.01 * reads)))
    return out


def queries(prob, count, base):
    """all transcripts, or `count` of those with theta_hat > 0 (base = full_solve) chosen by QUERY_SEED"""
    if count is None:
        return np.arange(prob[0], dtype=np.int32)
    th, _, den = base
    alive = np.flatnonzero(th * den >= 1e-9)
    return np.sort(np.random.default_rng(QUERY_SEED).choice(alive, size=count, replace=False)).astype(np.int32)


_ref_cache = {}


def oracle_case(name):
    """problem, queried tids and their reference, computed once per session"""
    if name not in _ref_cache:
        make, count = ORACLE_CASES[name]
        prob = make()
        base = full_solve(prob)
        q = queries(prob, count, base)
        _ref_cache[name] = (prob, q, reference(prob, q, base))
    return _ref_cache[name]


@pytest.fixture(scope="module")
def dev():
    with emsar_amd.EmsarHip(0) as d:
        yield d


def load(dev, prob, den=None):
    n_tx, rp, ci, R, E = prob
    dev.upload_structure(n_tx, rp, ci)
    dev.upload_sample(R, E, den)


def test_closed_form_answer(dev):
    """rows {a}: 30 and {a,b}: 50 with E = 1: theta_hat = (30, 20); without b, a takes all 80 reads at den 2, theta = 40; the {a} row
    is folded into u_a, so F carries the u log theta term; a cannot be dropped"""
    n_tx, rp, ci = csr([[0], [0, 1]], 2)
    load(dev, (n_tx, rp, ci, np.array([30, 50], dtype=np.int32), np.ones(2)))
    r = dev.presence(tol=1e-13)
    want = 2 * (30 * np.log(30) + 50 * np.log(50) - 80 * np.log(40))
    assert list(r["status"]) == [ESSENTIAL, TESTED]
    np.testing.assert_allclose(r["theta_hat"], [30.0, 20.0], rtol=1e-9)
    print("Lambda_b", r["lambda"][1], "closed form", want)
    assert abs(r["lambda"][1] - want) <= 1e-9 * want
    assert r["lambda"][0] == np.inf and r["pvalue"][0] == 0.0
    assert r["pvalue"][1] == H.presence_pvalue_host(r["lambda"][1])
    assert r["heir"][1] == 0 and abs(r["heir_share"][1] - 1.0) < 1e-8 and r["heir"][0] == -1 and np.isnan(r["heir_share"][0])
    st = r["stats"].as_dict()
    assert st["n_status"]["TESTED"] == 1 and st["n_status"]["ESSENTIAL"] == 1 and st["items_launched"] == 2
    # R = (50, 30): the a-only row explains more than a's share of the pair row could: theta_hat_b = 0
    # (theta_a = 40).  ABSENT asks for exactly 0, which is where a projected Newton step puts b; with the default newton_after this set
    # of two meets the relative stopping rule at theta_b ~ 1e-17 before its first Newton step at pass 60, and b is then tested: Lambda 0, p 1
    load(dev, (n_tx, rp, ci, np.array([50, 30], dtype=np.int32), np.ones(2)))
    r = dev.presence()
    assert r["status"][1] in (ABSENT, TESTED) and r["lambda"][1] <= 1e-12 and abs(r["pvalue"][1] - 1.0) <= 1e-6 and r["theta_hat"][1] < 1e-12
    r = dev.presence(newton_after=1)
    assert list(r["status"]) == [ESSENTIAL, ABSENT]
    assert r["theta_hat"][1] == 0.0 and r["lambda"][1] == 0.0 and r["pvalue"][1] == 1.0 and r["heir"][1] == -1
    assert r["stats"].items_launched == 1            # the baseline alone


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_against_the_oracle(dev, name):
    """statuses exactly; Lambda within LAMBDA_REL * (|F_full| + |F_drop|) + 1e-7 * Lambda (module docstring: 100 x the oracle's own
    spread of 4.26e-15); the heir wherever the reference's is clear"""
    prob, q, ref = oracle_case(name)
    load(dev, prob)
    r = dev.presence(q, tol=1e-12)
    worst = 0.0
    for i, (t, w) in enumerate(zip(q, ref)):
        assert r["status"][i] == w["status"], (name, int(t), int(r["status"][i]), w)
        if w["status"] == TESTED:
            bound = LAMBDA_REL * w["scale"] + 1e-7 * w["lam"]
            worst = max(worst, abs(r["lambda"][i] - w["lam"]) / bound)
            assert abs(r["lambda"][i] - w["lam"]) <= bound, (name, int(t), r["lambda"][i], w["lam"], bound)
            if w["clear"]:
                assert r["heir"][i] == w["heir"], (name, int(t), int(r["heir"][i]), w)
                assert abs(r["heir_share"][i] - w["share"]) <= 1e-6 * max(1.0, w["share"]), (name, int(t), r["heir_share"][i], w["share"])
        if w["status"] in (ABSENT, ESSENTIAL):
            assert r["lambda"][i] == w["lam"]
    print(name, "queried", len(q), "worst |dLambda| / bound", worst, "min raw Lambda", r["stats"].min_raw_lambda)


def test_the_heir_is_checked_in_three_quarters_of_the_queries():
    """the reference alone: of all TESTED queries of the oracle comparison at least 3/4 have a clear heir"""
    tested = clear = 0
    for name in ORACLE_CASES:
        for w in oracle_case(name)[2]:
            tested += w["status"] == TESTED
            clear += w["status"] == TESTED and w["clear"]
    assert tested > 0 and 4 * clear >= 3 * tested, (clear, tested)


def test_edge_semantics(dev):
    # tids: 0,1 a pair with a {t,t} row on 0; 2,3: 3 has den 0, so the row {2,3} hangs on 2 alone; 4,5,6 a family with an R = 0 row;
    # 7 has den 0 and stands alone
    rows = [[0, 1], [0, 0], [2, 3], [2, 8], [4, 5], [5, 6], [4, 6], [4, 5, 6], [7], [8, 2, 3]]
    R = np.array([9, 4, 6, 5, 7, 0, 3, 11, 2, 3], dtype=np.int32)
    n_tx, rp, ci = csr(rows, 9)
    den = np.array([2.0, 1.0, 2.0, 0.0, 3.0, 3.0, 3.0, 0.0, 0.5])          # 8 is cheap: theta_hat = (.., 2: 4, 8: 12)
    load(dev, (n_tx, rp, ci, R, np.ones(len(rows))), den)
    r = dev.presence()
    s = list(r["status"])
    assert s[0] == ESSENTIAL                       # the {0,0} row is a single-transcript row with reads
    assert s[1] in (TESTED, ABSENT)
    # {2,3} + {2,8} + {8,2,3}: without 2, 8 explains {2,8} and {8,2,3} but nothing explains {2,3} (3 has den 0): found by the drop
    # solve's epilogue, no single-transcript row says so; 8 can go
    assert s[2] == ESSENTIAL and r["lambda"][2] == np.inf and r["pvalue"][2] == 0.0 and s[8] == TESTED
    assert r["stats"].items_launched > 3           # 2 was solved for, not decided beforehand
    assert s[3] == OUTSIDE and s[7] == OUTSIDE and np.isnan(r["lambda"][3]) and np.isnan(r["pvalue"][7]) and r["heir"][3] == -1
    assert all(x in (TESTED, ABSENT) for x in s[4:7])
    assert np.all(np.isfinite(r["lambda"][4:7])) and np.all(r["lambda"][4:7] >= 0)
    # make {2,3} the only row of 2 next to a row that 8 shares: dropping 2 strands {2,3} (its other member has den 0): the epilogue's count
    rows2 = [[2, 3], [2, 8], [8, 0], [0, 1]]
    n_tx, rp, ci = csr(rows2, 9)
    load(dev, (n_tx, rp, ci, np.array([6, 5, 4, 3], dtype=np.int32), np.ones(4)), np.array([1.0, 1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5]))
    r = dev.presence([2, 8, 3])
    assert list(r["status"]) == [ESSENTIAL, TESTED, OUTSIDE]
    assert r["lambda"][0] == np.inf and r["pvalue"][0] == 0.0
    # repeats and non-monotone order: a transcript's answer is the same wherever it stands
    q = [8, 2, 8, 0, 2, 1, 8]
    rq = dev.presence(q)
    one = {t: dev.presence([t]) for t in set(q)}
    for i, t in enumerate(q):
        for k in ("lambda", "pvalue", "heir_share", "theta_hat"):
            assert rq[k][i].tobytes() == one[t][k][0].tobytes(), (k, i, t)
        assert rq["status"][i] == one[t]["status"][0] and rq["heir"][i] == one[t]["heir"][0]
    assert sum(rq["stats"].as_dict()["n_status"].values()) == len(set(q))
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        dev.presence([0, 9])
    assert e.value.status == -1
    with pytest.raises(emsar_amd.EmsarHipError):
        dev.presence([-1])


def test_streamed_sets_and_streaming_mode_are_not_resident(dev):
    prob = SP.everything_problem()
    n_tx, rp, ci, R, E = prob
    load(dev, prob)
    info = H.sets_selfcheck(n_tx, rp, ci, np.where(E > 0, R, 0))
    assert info["sets_streamed"] == 1
    rng = np.random.default_rng(3)
    q = rng.choice(n_tx, size=200, replace=False).astype(np.int32)
    r = dev.presence(q, max_iter=3000)
    n_nr = int(np.sum(r["status"] == NOT_RESIDENT))
    assert 0 < n_nr < len(q)
    assert np.all(np.isnan(r["lambda"][r["status"] == NOT_RESIDENT])) and np.all(np.isnan(r["theta_hat"][r["status"] == NOT_RESIDENT]))
    # the streamed set is the 900-transcript shape one entry over the cap: its transcripts, and only they
    fpkm, st = dev.solve(max_iter=3000)
    assert st.sets_streamed == 1
    r1 = dev.presence(q[:20], set_mode=1)
    assert np.all(r1["status"] == NOT_RESIDENT) and r1["stats"].items_launched == 0


def test_independence_and_no_side_effects(dev, monkeypatch):
    prob = SP.all_resident_problem()
    n_tx = prob[0]
    load(dev, prob)
    kw = dict(max_iter=4000)
    before, _ = dev.solve(**kw)
    theta0 = dev.get_theta()
    rng = np.random.default_rng(11)
    q = rng.choice(n_tx, size=120, replace=False).astype(np.int32)
    whole = dev.presence(q, **kw)
    assert dev.get_theta().tobytes() == theta0.tobytes()
    after, _ = dev.solve(**kw)
    assert after.tobytes() == before.tobytes()
    halves = [dev.presence(q[:60], **kw), dev.presence(q[60:], **kw)]
    rev = dev.presence(q[::-1].copy(), **kw)
    monkeypatch.setenv("EMSAR_HIP_PRESENCE_BATCH", "7")          # many launches per class instead of one
    small = dev.presence(q, **kw)
    monkeypatch.delenv("EMSAR_HIP_PRESENCE_BATCH")
    for k in ("lambda", "pvalue", "heir", "heir_share", "status", "theta_hat"):
        assert np.concatenate([h[k] for h in halves]).tobytes() == whole[k].tobytes(), k
        assert rev[k][::-1].tobytes() == whole[k].tobytes(), k
        assert small[k].tobytes() == whole[k].tobytes(), k
    assert whole["theta_hat"].tobytes() == before[q].tobytes()       # the baseline is solve's result, bit for bit
    assert np.any(whole["status"] == TESTED)
    st = whole["stats"].as_dict()
    assert st["drop_passes_max"] > 0 and st["drop_passes_sum"] >= st["drop_passes_max"] and st["min_raw_lambda"] <= 0.0
    assert st["items_launched"] > st["n_status"]["TESTED"]


def test_needs_a_sample():
    with emsar_amd.EmsarHip(0) as d:
        n_tx, rp, ci = csr([[0, 1]], 2)
        d.upload_structure(n_tx, rp, ci)
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            d.presence()
        assert e.value.status == -5


def test_cli_presence_file(tmp_path):
    """--presence on a golden fixture: the .presence file's Lambda column is the Python call's, the .fpkm does not change"""
    from emsar_amd import _build
    from emsar_amd import hostlib as HL
    from tests.conftest import aln_path, get_fixture
    _build.build_all()
    fx = get_fixture("syn300_se")
    aln, fmt = aln_path(fx.dir)
    rsh_path = os.path.join(fx.dir, "index.rsh")
    for tag, extra in (("a", []), ("b", ["--presence"])):
        subprocess.run([_build.CLI, "-q", "-g"] + fx.meta["opts"] + extra + ["-I", rsh_path, str(tmp_path / tag), "out", aln], check=True, timeout=300)
    a, b = tmp_path / "a", tmp_path / "b"
    for ext in ("fpkm", "fraglength_effect", "segments"):
        assert (a / ("out.0." + ext)).read_bytes() == (b / ("out.0." + ext)).read_bytes(), ext
    assert not (a / "out.0.presence").exists()
    # what the CLI does for the sample, through the Python bindings: count, model, den in row order on the host, its solver settings
    rsh = HL.HostRsh(rsh_path)
    cnt = rsh.count(aln, fmt=fmt)
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=200000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13)
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
        p = d.presence(**cli)
    lines = (b / "out.0.presence").read_text().splitlines()
    assert lines[0].split("\t") == ["tid", "transcriptID", "FPKM", "Lambda", "p", "status", "heir", "heir_share"]
    got = [l.split("\t") for l in lines[1:]]
    text = [l.split("\t") for l in (b / "out.0.fpkm").read_text().splitlines()[1:]]
    assert len(got) == rsh.n_tx and all(len(r) == 8 for r in got)
    assert [int(r[0]) for r in got] == list(range(rsh.n_tx)) and [r[1:3] for r in got] == [t[:2] for t in text]
    assert [r[5] for r in got] == [H.PRESENCE_STATUS[k] for k in p["status"]]
    assert [r[6] for r in got] == [rsh.names[h] if h >= 0 else "-" for h in p["heir"]]
    lam = np.array([float(r[3]) for r in got])
    fin = np.isfinite(p["lambda"])
    assert np.array_equal(np.isinf(lam), np.isinf(p["lambda"])) and np.array_equal(np.isnan(lam), np.isnan(p["lambda"]))
    assert np.all(np.abs(lam[fin] - p["lambda"][fin]) <= 1e-6 + 1e-15 * p["lambda"][fin])          # "%lf"
    assert np.sum(p["status"] == TESTED) >= 10 and np.sum(p["status"] == ESSENTIAL) >= 10
    # a list: the named transcripts only, in the list's order
    lst = tmp_path / "names.txt"
    pick = [int(t) for t in np.flatnonzero(p["status"] == TESTED)[:3][::-1]]
    lst.write_text("".join(rsh.names[t] + "\n" for t in pick))
    subprocess.run([_build.CLI, "-q"] + fx.meta["opts"] + ["--presence", "--presence-list", str(lst), "-I", rsh_path, str(tmp_path / "c"), "out", aln],
                   check=True, timeout=300)
    short = [l.split("\t") for l in (tmp_path / "c" / "out.0.presence").read_text().splitlines()[1:]]
    assert short == [got[t] for t in pick]
