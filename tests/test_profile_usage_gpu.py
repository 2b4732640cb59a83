"""GPU: the profile-likelihood intervals of isoform usage (emsar_hip_profile_usage, include/emsar_hip.h "profile-likelihood intervals of
isoform usage") against the independent numpy reference of tests/profile_usage_problems.py (roots of the dual deviance over bracketed
multiplier searches over plain EMs, recorded in tests/golden/profile_usage_refs.json with the reference's own error w_ref), inside one
set of each size class, over several parts with closed-form parts, with mixed classes in one gene, at the boundary statuses, against
the presence test and isoform_usage, for bit-identity under everything a result must not depend on, on the paths that are not searched,
on the host's closed-form path and through the CLI.

The tolerance at a limit the device reports is  |limit - limit_ref| |slope_ref| <= dev_tol q + 2 dev_tol + 4 P e_F + w_ref + 1e-9:  the
outer rule is granted dev_tol q, the inner search's bound on the device and in the reference dev_tol each, each of the P parts enters D
with two F values and a factor 2 each.  e_F = 4 x 9.4e-10 is test_compare_gpu.py's figure, measured on the existing set solver, not on
the code under test.

Every call passes max_iter <= 20000, tol = 1e-12 where a reference is compared and the default caps of the two searches, and den is
computed on the host (CP.den_of)."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import compare_gene_problems as GP
from tests import compare_problems as CP
from tests import compare_usage_problems as UP
from tests import profile_usage_problems as PU
from tests.test_compare_genes_gpu import config, drawn_genes, invariance_problem, load

pytestmark = pytest.mark.gpu

TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE, UPPER_ONE, UNIT, UNDEFINED, SINGLE = range(10)
DEV_TOL = 1e-4
TIGHT = 1e-9
E_F = 4 * 9.4e-10
W_REF_MAX = 1e-7
CAPS = dict(max_iter=20000)
OUTPUTS = H.PROFILE_USAGE_OUTPUTS + H.PROFILE_USAGE_COUNTS
STATS = ("n_status", "items_launched", "evals_sum", "passes_sum", "outer_sum", "evals_max", "passes_max", "parts_max", "outer_max", "min_raw_lambda", "cut")
SMALL = [[0, 3, 6], [8, 9], [4, 10], [1, 2], [5], [7]]


@pytest.fixture(scope="module")
def dev():
    with emsar_amd.EmsarHip(0) as d:
        yield d


def same_bits(x, y, keys=OUTPUTS):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def stats_of(r):
    d = r["stats"].as_dict()
    return {k: d[k] for k in STATS}


def tol_of(ref, dev_tol):
    q = ref["q"]
    return lambda side: dev_tol * q + 2 * dev_tol + 4 * ref["parts"] * E_F + abs(ref["w_" + side]) + 1e-9


def check_against(r, i, ref, what, dev_tol=DEV_TOL):
    """every check of a searched (gene, t) against its recorded reference -> the two residuals in units of D"""
    q, tol = ref["q"], tol_of(ref, dev_tol)
    assert abs(ref["w_lower"]) <= W_REF_MAX and abs(ref["w_upper"]) <= W_REF_MAX, (what, ref["w_lower"], ref["w_upper"])
    res = {}
    for side in ("lower", "upper"):
        res[side] = abs(r[side][i] - ref[side + "_ref"]) * abs(ref["slope_" + side])
    print(what, "dev_tol", dev_tol, "usage", r["usage"][i], "ref", ref["usage"], "lower", r["lower"][i], "ref", ref["lower_ref"], "upper", r["upper"][i],
          "ref", ref["upper_ref"], "residuals", res, "tol", tol("lower"), tol("upper"), "dev", r["dev_lower"][i], r["dev_upper"][i], "Lambdas",
          r["lambda_zero"][i], r["lambda_one"][i], "ref D0 D1", ref["D0"], ref["D1"], "status", r["status"][i], "outer", r["outer_evals"][i], "evals",
          r["evals"][i])
    assert r["parts"][i] == ref["parts"] and r["members"][i] == ref["members"], (what, r["parts"][i], r["members"][i])
    assert abs(r["usage"][i] - ref["usage"]) <= 1e-6 * max(ref["usage"], 1e-3), (what, r["usage"][i], ref["usage"])
    zero, one = ref["lower_ref"] == 0.0, ref["upper_ref"] == 1.0
    assert r["status"][i] == (UNIT if zero and one else LOWER_ZERO if zero else UPPER_ONE if one else TWO_SIDED), (what, r["status"][i])
    for side, at_end, end, lam in (("lower", zero, 0.0, "lambda_zero"), ("upper", one, 1.0, "lambda_one")):
        if at_end:
            assert r[side][i] == end and r["dev_" + side][i] == r[lam][i] <= q, (what, side, r[side][i], r["dev_" + side][i])
        else:
            assert abs(r["dev_" + side][i] - q) <= dev_tol * q, (what, side, r["dev_" + side][i])
            assert res[side] <= tol(side), (what, side, r[side][i], ref[side + "_ref"], res[side], tol(side))
            assert r[lam][i] > q
    assert r["lower"][i] <= r["usage"][i] <= r["upper"][i] and r["lower"][i] < r["upper"][i]
    if not zero and not one:
        assert r["lower"][i] < r["usage"][i] < r["upper"][i]
    # the ends: +inf by the host's rule exactly where the reference's rule says so; else no smaller than the dual D next to the end
    for lam, D in (("lambda_zero", ref["D0"]), ("lambda_one", ref["D1"])):
        if math.isinf(D):
            assert r[lam][i] == math.inf, (what, lam, r[lam][i])
        else:
            assert r[lam][i] >= D - tol("lower") and math.isfinite(r[lam][i]), (what, lam, r[lam][i], D)
    return res


def run_case(dev, name, which, genes=None, **kw):
    """sample `which` of the case `name` of UP.CASES on the device -> (result, index of t in the query, reference)"""
    prob, R, den, members, t = PU.sample_of(name, which)
    load(dev, prob, R, den, [members] if genes is None else genes)
    return dev.profile_usage(np.array([t], dtype=np.int32), tol=1e-12, **CAPS, **kw), 0, PU.tested_reference(name, which)


def genes_of(name):
    return GP.class_genes(int(name[5:].partition("-")[0])) if name.startswith("class") else None


# ---- 1. every recorded case against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", list(UP.CASES))
def test_against_the_reference(dev, name, which):
    """inside one set of each class (class64-*, class256, class512), over the parts loop with closed-form parts (small-*: 0 is itself a
    closed-form part), mixed classes in one gene (mixed), a share of exactly 0 (small-0-3-6:6 B, split A) and awkward row forms"""
    r, i, ref = run_case(dev, name, which, genes=genes_of(name), dev_tol=DEV_TOL)
    check_against(r, i, ref, (name, which))
    st = r["stats"].as_dict()
    searched = int(ref["lower_ref"] != 0.0) + int(ref["upper_ref"] != 1.0)
    assert st["items_launched"] == 1 + searched and st["evals_sum"] == r["evals"][0] and st["outer_sum"] == r["outer_evals"][0]
    assert st["outer_max"] <= 24 and st["evals_max"] <= 24 * 40 and st["parts_max"] == ref["parts"] and abs(st["cut"] - ref["q"]) <= 1e-14


@pytest.mark.parametrize("name,which", [("class64-0", "A"), ("class64-1", "B"), ("small-0-3-6:0", "A"), ("small-0-3-6:3", "B"), ("mixed", "A"),
                                        ("class256", "A")])
def test_residual_shrinks_with_dev_tol(dev, name, which):
    """dev_tol = 1e-9: every search of every recorded case still ends within the default caps (24 outer points of 40 inner evaluations
    each) at tol = 1e-12 for dev_tol = 1e-4, 1e-5, ... 1e-9 -- at most 9 outer points and 69 inner evaluations per limit, residuals of at most
    3.7e-9 at 1e-9 --, and 1e-9 is the smallest value worth asking for: F_hat is about 2.1e6 in the class256 and class512 problems, where D
    moves in steps of 2 ulp(F) = 9.3e-10, so a rule |D - q| <= 1e-10 q could be met by luck alone.  The tolerance shrinks with dev_tol to the
    floor 4 P e_F + w_ref + 1e-9 that the set solver's own F leaves, and the residual must lie a hundred times below the bound of the
    run at 1e-4"""
    r, i, ref = run_case(dev, name, which, genes=genes_of(name), dev_tol=TIGHT)
    tight = check_against(r, i, ref, (name, which), dev_tol=TIGHT)
    assert r["status"][i] == TWO_SIDED
    loose = tol_of(ref, DEV_TOL)
    assert max(tight.values()) <= 0.01 * loose("lower")


# ---- 2. the boundary statuses ------------------------------------------------------------------------------------------------------------
def two_transcripts(rows, R):
    n_tx, rp, ci = CP.csr(rows, 2)
    R = np.asarray(R, dtype=np.int32)
    return (n_tx, rp, ci, R, np.ones(len(rows))), R


def test_boundary_statuses(dev):
    """rows {t, s} with 6 reads and {s} with 2, E = 1, den = (1, 2): theta_hat = (4, 2), usage 2/3; without t the 8 reads go to s,
    Lambda_zero = 2 (6 ln 6 + 2 ln 2 - 8 ln 4) <= q; s has reads only it explains: Lambda_one = +inf.  s mirrors t: UPPER_ONE, lower = 1 - upper_t"""
    prob, R = two_transcripts([[0, 1], [1]], [6, 2])
    den = CP.den_of(prob)
    assert list(den) == [1.0, 2.0]
    load(dev, prob, R, den, [[0, 1]])
    r = dev.profile_usage(tol=1e-12, **CAPS)
    # PU.reference(prob, R, den, [0, 1], 0), three seconds of plain EM next to the boundary: recorded here
    ref = dict(q=PU.Q95, lower_ref=0.0, upper_ref=0.9511456220353456, slope_upper=66.62123958456434, w_upper=5.4e-15)
    q = ref["q"]
    lam = 2.0 * (6 * math.log(6) + 2 * math.log(2) - 8 * math.log(4))
    print({k: r[k] for k in OUTPUTS}, ref, lam)
    assert abs(lam - 2.0929925709) <= 1e-8 and abs(ref["upper_ref"] - 0.95114562) <= 1e-7 and ref["lower_ref"] == 0.0
    tol = (DEV_TOL * q + 2 * DEV_TOL + 4 * E_F + abs(ref["w_upper"]) + 1e-9) / abs(ref["slope_upper"])
    assert list(r["status"]) == [LOWER_ZERO, UPPER_ONE] and np.all(np.abs(r["usage"] - [2 / 3, 1 / 3]) <= 1e-12)
    assert r["lower"][0] == 0.0 and abs(r["lambda_zero"][0] - lam) <= 1e-9 and r["dev_lower"][0] == r["lambda_zero"][0] and r["lambda_one"][0] == math.inf
    assert abs(r["upper"][0] - ref["upper_ref"]) <= tol and abs(r["dev_upper"][0] - q) <= DEV_TOL * q
    assert r["upper"][1] == 1.0 and abs(r["lambda_one"][1] - lam) <= 1e-9 and r["dev_upper"][1] == r["lambda_one"][1] and r["lambda_zero"][1] == math.inf
    assert abs(r["lower"][1] - (1.0 - ref["upper_ref"])) <= tol and abs(r["dev_lower"][1] - q) <= DEV_TOL * q
    assert list(r["parts"]) == [1, 1] and list(r["members"]) == [2, 2] and r["stats"].items_launched == 4
    # one row {t, s} with 3 reads, den = (1, 1): the reads cannot tell the two apart
    prob, R = two_transcripts([[0, 1]], [3])
    load(dev, prob, R, CP.den_of(prob), [[0, 1]])
    r = dev.profile_usage(tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert list(r["status"]) == [UNIT, UNIT] and np.all(np.abs(r["usage"] - 0.5) <= 1e-12)
    assert np.all(r["lower"] == 0.0) and np.all(r["upper"] == 1.0) and np.all(r["lambda_zero"] <= 1e-9) and np.all(r["lambda_one"] <= 1e-9)
    assert np.all(r["dev_lower"] == r["lambda_zero"]) and np.all(r["dev_upper"] == r["lambda_one"]) and np.all(r["evals"] == 0)
    assert r["stats"].items_launched == 2 and r["stats"].as_dict()["n_status"]["UNIT"] == 2


# ---- 3. the two members of a two-member gene mirror each other ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
def test_two_member_gene_is_symmetric(dev, which):
    prob, R, den, members, t = PU.sample_of("mixed", which)
    ref = PU.tested_reference("mixed", which)
    assert len(members) == 2 and t == members[0]
    load(dev, prob, R, den, [members])
    r = dev.profile_usage(np.array(members, dtype=np.int32), tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert list(r["status"]) == [TWO_SIDED, TWO_SIDED] and abs(r["usage"].sum() - 1.0) <= 1e-12
    assert abs(r["lower"][1] - (1.0 - r["upper"][0])) <= 2 * DEV_TOL * ref["q"] / abs(ref["slope_upper"])
    assert abs(r["upper"][1] - (1.0 - r["lower"][0])) <= 2 * DEV_TOL * ref["q"] / abs(ref["slope_lower"])
    assert abs(r["lambda_zero"][1] - r["lambda_one"][0]) <= 1e-9 * r["lambda_one"][0] and abs(r["lambda_one"][1] - r["lambda_zero"][0]) <= 1e-9 * r["lambda_zero"][0]


# ---- 4. Lambda_zero is the presence statistic, usage is isoform_usage -------------------------------------------------------------------
def test_presence_and_isoform_usage(dev):
    """lambda_zero and the presence test's Lambda are the same difference of two F values, summed over the gene's parts here and over t's
    set there: 1e-9 relative wherever both are finite (two Lambdas of exactly 0 agree)"""
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    for R in (RA, RB):
        load(dev, prob, R, den, genes)
        r = dev.profile_usage(tol=1e-12, **CAPS)
        pres = dev.presence(tol=1e-12, **CAPS)
        usage = dev.isoform_usage(dev.solve(tol=1e-12, **CAPS)[0])
        given = np.isin(r["status"], (TWO_SIDED, LOWER_ZERO, UPPER_ONE, UNIT, UNCONVERGED))
        print(r["stats"].as_dict(), "given", given.sum())
        assert given.sum() >= 30          # two of them UNCONVERGED: twins with equal columns, whose solves at tol = 1e-12 run into max_iter
        assert np.all(np.abs(r["usage"][given] - usage[given]) <= 1e-12 * np.maximum(usage[given], 1e-300))
        essential = pres["status"] == H.PRESENCE_STATUS.index("ESSENTIAL")
        assert np.array_equal(np.isinf(r["lambda_zero"][given]), essential[given])
        both = given & np.isfinite(r["lambda_zero"]) & np.isfinite(pres["lambda"])
        diff = np.abs(r["lambda_zero"][both] - pres["lambda"][both])
        scale = np.maximum(r["lambda_zero"][both], pres["lambda"][both])
        print("both finite", both.sum(), "max |d Lambda|", diff.max(), "max relative", (diff / np.where(scale > 0, scale, 1.0)).max(), "smallest Lambda",
              scale.min(), "Lambdas", np.sort(scale)[:8])
        assert both.sum() >= 10 and np.all(diff <= 1e-9 * scale)
        inner = given & (r["status"] != UNCONVERGED)
        assert np.all(r["lower"][inner] <= r["usage"][inner]) and np.all(r["usage"][inner] <= r["upper"][inner])
        assert np.all((r["lower"][inner] >= 0.0) & (r["upper"][inner] <= 1.0))


# ---- 5. bit-for-bit invariance, the context untouched -------------------------------------------------------------------------------------
def test_invariance_bit_for_bit(dev, monkeypatch):
    prob, RA, _ = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    n = prob[0]
    kw = dict(max_iter=3000)
    config(monkeypatch, dev, prob, RA, den, genes, H.LAYOUT_CSR, False, None)
    before = dev.solve(**kw)[0]
    whole = dev.profile_usage(**kw)
    assert before.tobytes() == dev.solve(**kw)[0].tobytes()
    st = whole["stats"].as_dict()
    print(st)
    assert st["n_status"]["TWO_SIDED"] + st["n_status"]["LOWER_ZERO"] + st["n_status"]["UPPER_ONE"] + st["n_status"]["UNIT"] >= 20
    assert st["parts_max"] >= 2 and np.sum(whole["parts"] > 1) >= 5 and st["outer_max"] <= 24
    q = np.random.default_rng(5).permutation(n).astype(np.int32)
    shuffled = dev.profile_usage(q, **kw)
    twice = dev.profile_usage(np.concatenate([q[:10], q[:10], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_PROFILE_USAGE_BATCH", "1")     # one item per class and launch
    single = dev.profile_usage(**kw)
    monkeypatch.delenv("EMSAR_HIP_PROFILE_USAGE_BATCH")
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][20:].tobytes() == shuffled[k].tobytes() and twice[k][:10].tobytes() == twice[k][10:20].tobytes() == shuffled[k][:10].tobytes(), k
        assert single[k].tobytes() == whole[k].tobytes(), k
    assert stats_of(shuffled) == stats_of(whole) == stats_of(twice) == stats_of(single)
    part = dev.profile_usage(q[:7], **kw)                       # a part of the query alone
    assert not [k for k in OUTPUTS if part[k].tobytes() != shuffled[k][:7].tobytes()]
    for layout, merge, mode in ((H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"), (H.LAYOUT_TILED, True, "2")):
        config(monkeypatch, dev, prob, RA, den, genes, layout, merge, mode)
        got = dev.profile_usage(**kw)
        assert not same_bits(got, whole) and stats_of(got) == stats_of(whole), (layout, merge, mode)


# ---- 6. the paths that are not searched, and the errors ------------------------------------------------------------------------------------
def test_statuses_without_a_search(dev):
    prob, RA, RB, den_a, den_b = CP.small_problem()
    load(dev, prob, RB, den_b, SMALL)
    r = dev.profile_usage(tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    nan_out = lambda t: all(math.isnan(r[k][t]) for k in H.PROFILE_USAGE_OUTPUTS)
    # {8, 9}: no reads; {4, 10}: 10 has den = 0 here, which leaves 4 alone; {5}, {7}: one member
    assert r["status"][8] == r["status"][9] == UNDEFINED and nan_out(8) and r["parts"][8] == 2 and r["members"][8] == 2 and r["evals"][8] == 0
    assert r["status"][10] == OUTSIDE and r["status"][4] == SINGLE and r["status"][5] == SINGLE and r["status"][7] == SINGLE
    for t in (10, 4, 5, 7):
        assert nan_out(t) and r["outer_evals"][t] == r["evals"][t] == r["parts"][t] == r["members"][t] == 0, t
    assert r["status"][6] == LOWER_ZERO and r["usage"][6] == 0.0 and r["lower"][6] == 0.0 and r["lambda_zero"][6] == 0.0
    assert abs(r["usage"][[0, 3, 6]].sum() - 1.0) <= 1e-12 and r["parts"][0] == r["parts"][3] == r["parts"][6] == 3
    st = r["stats"].as_dict()
    assert sum(st["n_status"].values()) == 11 and st["n_status"]["SINGLE"] == 3 and st["n_status"]["UNDEFINED"] == 2 and st["n_status"]["OUTSIDE"] == 1
    g = np.full(prob[0], -1, dtype=np.int32)
    g[[0, 3]] = 0
    dev.set_gene_map(g, 1)
    o = dev.profile_usage([6, 0], tol=1e-12, **CAPS)
    assert o["status"][0] == OUTSIDE and o["status"][1] in (TWO_SIDED, LOWER_ZERO, UPPER_ONE, UNIT)          # 6 has no gene


def test_not_resident_too_large_and_errors(dev):
    prob, RA, _, _ = CP.class_problem(64)
    genes = GP.class_genes(64)
    den = CP.den_of(prob)
    load(dev, prob, RA, den, genes)
    q = np.array([g[0] for g in genes], dtype=np.int32)
    full = dev.profile_usage(q, **CAPS)
    assert np.all(full["status"] == TWO_SIDED)
    capped = dev.profile_usage(q, max_outer=1, max_evals=2, **CAPS)
    assert np.all(capped["status"] == UNCONVERGED) and np.all(capped["outer_evals"] == 2) and np.all(capped["evals"] <= 4)
    assert capped["usage"].tobytes() == full["usage"].tobytes() and capped["lambda_zero"].tobytes() == full["lambda_zero"].tobytes()
    assert np.all(np.isfinite(capped["lower"])) and np.all(np.isfinite(capped["upper"]))
    off = dev.profile_usage(q, set_mode=1, **CAPS)
    assert np.all(off["status"] == NOT_RESIDENT) and off["stats"].items_launched == 0 and np.all(off["evals"] == 0) and np.all(np.isnan(off["usage"]))
    for bad in (dict(query=[0, prob[0]]), dict(query=[-1]), dict(dev_tol=math.inf), dict(dev_tol=math.nan), dict(level=0.0), dict(level=1.0),
                dict(level=math.nan), dict(set_mode=2), dict(count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            dev.profile_usage(**bad, **CAPS)
        assert e.value.status == -1, bad
    assert not same_bits(dev.profile_usage(q, **CAPS), full)
    load(dev, prob, RA, den)                                  # a new structure drops the gene map
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        dev.profile_usage(**CAPS)
    assert e.value.status == -5
    # 65 one-transcript rows in one gene: TOO_LARGE; 64: searched on the host
    n = 65 + 64
    rows = [[t] for t in range(n)]
    n_tx, rp, ci = CP.csr(rows, n)
    R = np.random.default_rng(3).integers(1, 40, size=n).astype(np.int32)
    g = np.zeros(n, dtype=np.int32)
    g[65:] = 1
    load(dev, (n_tx, rp, ci, R, np.ones(n)), R, None, (g, 2))
    r = dev.profile_usage([3, 70], **CAPS)
    assert r["status"][0] == TOO_LARGE and r["evals"][0] == r["parts"][0] == r["members"][0] == 0 and all(math.isnan(r[k][0]) for k in H.PROFILE_USAGE_OUTPUTS)
    assert r["status"][1] == TWO_SIDED and r["parts"][1] == r["members"][1] == 64 and r["stats"].items_launched == 0


# ---- 7. the host's closed-form path ----------------------------------------------------------------------------------------------------
def test_closed_form_genes_are_the_hosts(dev):
    prob, RA, RB, den_a, den_b = CP.small_problem()
    load(dev, prob, RA, den_a, [[0, 1]])
    for kw in (dict(), dict(dev_tol=1e-8, level=0.9, max_evals=50, max_outer=30)):
        h = dev.profile_usage([1, 0, 5], tol=1e-12, **CAPS, **kw)
        assert h["stats"].items_launched == 0 and h["status"][2] == OUTSIDE          # 5 has no gene
        for i, t in enumerate((1, 0)):
            want = H.debug_profile_usage_closed(RA[[0, 1]].astype(float), den_a[[0, 1]], t=t, **kw)
            for k in OUTPUTS:
                assert np.array([h[k][i]]).tobytes() == np.array([want[k]], dtype=h[k].dtype).tobytes(), (t, k, h[k][i], want[k])
        assert h["status"][0] == TWO_SIDED and h["outer_evals"][0] > 1 and abs(h["lower"][0] + h["upper"][1] - 1.0) <= 1e-3


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_uprofile_file(tmp_path):
    """--profile-usage --g2t on the syn300_se fixture: out.0.uprofile has one line per transcript and its columns are the Python call's
    as printed; --profile --g2t alone writes no .uprofile; with --profile-usage every other file keeps its bytes; --profile-list filters"""
    from emsar_amd import _build
    from emsar_amd import hostlib as HL
    from tests.conftest import aln_path, get_fixture
    _build.build_all()
    fx = get_fixture("syn300_se")
    aln, fmt = aln_path(fx.dir)
    rsh_path = os.path.join(fx.dir, "index.rsh")
    rsh = HL.HostRsh(rsh_path)
    g2t = tmp_path / "genes.g2t"
    g2t.write_text("".join("gene%04d\t%s\n" % (t // 3, name) for t, name in enumerate(rsh.names)))
    n_genes = (rsh.n_tx + 2) // 3
    lst = tmp_path / "some.list"
    lst.write_text("".join(name + "\n" for name in rsh.names[:5]))
    base = [_build.CLI, "-q", "-i", "20000", "--gpus", "1", "--g2t", str(g2t), "--profile-evals", "30"] + fx.meta["opts"]
    tail = lambda d: ["-I", rsh_path, str(tmp_path / d), "out", aln]
    subprocess.run(base + ["--profile"] + tail("p"), check=True, timeout=300)
    subprocess.run(base + ["--profile", "--profile-usage"] + tail("o"), check=True, timeout=300)
    subprocess.run(base + ["--profile-usage", "--profile-list", str(lst)] + tail("l"), check=True, timeout=300)
    assert not [f for f in os.listdir(tmp_path / "p") if f.endswith(".uprofile")]
    assert sorted(os.listdir(tmp_path / "o")) == sorted(os.listdir(tmp_path / "p") + ["out.0.uprofile"])
    for f in os.listdir(tmp_path / "p"):
        assert (tmp_path / "o" / f).read_bytes() == (tmp_path / "p" / f).read_bytes(), f
    assert not [f for f in os.listdir(tmp_path / "l") if f.endswith("profile") and f != "out.0.uprofile"]
    got = [l.split("\t") for l in (tmp_path / "o" / "out.0.uprofile").read_text().splitlines()]
    assert got[0] == ["transcript", "gene", "usage", "lower", "upper", "Lambda_zero", "Lambda_one", "status", "outer", "evals"]
    assert (tmp_path / "l" / "out.0.uprofile").read_text().splitlines() == ["\t".join(r) for r in got[:6]]
    got = got[1:]
    assert len(got) == rsh.n_tx and all(len(r) == 10 for r in got)
    assert [r[0] for r in got] == list(rsh.names) and [r[1] for r in got] == ["gene%04d" % (t // 3) for t in range(rsh.n_tx)]
    gene_of = np.arange(rsh.n_tx, dtype=np.int32) // 3
    rp, ci = np.asarray(rsh.row_ptr), np.asarray(rsh.col_idx)
    cli = dict(max_iter=20000, accel=1, tol=1e-10, abs_floor=0.0, check_every=0, zero_cut=2.5e-7, abs_step=1e-13, max_evals=30)
    rows = np.repeat(np.arange(rsh.n_rows), np.diff(rp.astype(np.int64)))
    with emsar_amd.EmsarHip(0) as d:
        cnt = rsh.count(str(aln), fmt=fmt)
        d.set_deterministic(True)
        d.upload_structure(rsh.n_tx, rp, ci)
        d.upload_euma(rsh.euma)
        E = np.array(rsh.model(cnt, L=d.adj_euma(rsh.wf(cnt))).E_solver)
        den = np.zeros(rsh.n_tx)
        keep_e = E[rows] != 0.0
        np.add.at(den, ci[keep_e], E[rows][keep_e])
        d.upload_sample(np.array(cnt.R), E, den)
        d.set_gene_map(gene_of, n_genes)
        p = d.profile_usage(**cli)
    assert [r[7] for r in got] == [H.PROFILE_USAGE_STATUS[k] for k in p["status"]]
    assert [int(r[8]) for r in got] == list(p["outer_evals"]) and [int(r[9]) for r in got] == list(p["evals"])
    for col, key in ((2, "usage"), (3, "lower"), (4, "upper"), (5, "lambda_zero"), (6, "lambda_one")):
        v = np.array([float(r[col]) for r in got])
        fin = np.isfinite(p[key])
        assert np.array_equal(np.isnan(v), np.isnan(p[key])) and np.array_equal(v[~fin & ~np.isnan(v)], p[key][~fin & ~np.isnan(p[key])]), key
        assert np.all(np.abs(v[fin] - p[key][fin]) <= 1e-6 + 1e-15 * np.abs(p[key][fin])), key          # "%lf"
    print(p["stats"].as_dict())
    assert np.sum(np.isin(p["status"], (TWO_SIDED, LOWER_ZERO, UPPER_ONE, UNIT))) >= 30
