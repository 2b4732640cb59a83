"""GPU: the gene-level profile intervals and the gene presence test (emsar_hip_profile_genes, include/emsar_hip.h "gene-level profile
intervals") against an analytic gene, against scalar root finds on the host path, against the independent pinned-sum EM of
tests/profile_gene_problems.py in each size class and over several parts, for one-member genes against emsar_hip_profile, for
bit-identity under everything a result must not depend on, on the paths that are not searched, and through the CLI.

The tolerance against the reference, at a limit the device reports: D_ref(limit) lies within
    100 x SPREAD x (|F_hat| + |F_pinned|)  +  1e-7 q  +  4 P E_F
of dev_*.  SPREAD = 2.3e-16 is the reference against itself (relative step 1e-10 against 1e-13; 2.22e-16 measured by
`python -m tests.profile_gene_problems`), 1e-7 q is test_profile_gpu.py's figure for the solver's stopping rule, E_F = 4 x 9.4e-10
test_compare_genes_gpu.py's figure for one F of one part (each of the P parts enters a deviance with two F values and a factor 2 each).
None of the three was measured on the code under test.

Every call passes max_iter <= 20000 and max_evals <= 30, and den is computed on the host (CP.den_of)."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import compare_gene_problems as GP
from tests import compare_problems as CP
from tests import profile_gene_problems as PG
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE = range(6)
DEV_TOL = 1e-4
E_F = 4 * 9.4e-10
CAPS = dict(max_iter=20000, max_evals=30)
OUTPUTS = H.PROFILE_GENE_OUTPUTS + ("status", "evals", "parts", "members")
SMALL_X = [[0, 3, 6], [8, 9], [10], [1], [2], [5], [7]]
SMALL_Y = [[0, 1], [4, 10], [8, 9]]


def q_of(level):
    return H.profile_cut_host(level)


@pytest.fixture(scope="module")
def dev():
    with emsar_amd.EmsarHip(0) as d:
        yield d


def load(dev, prob, R, den=None, genes=None, layout=H.LAYOUT_AUTO, merge_rows=False):
    """structure, sample and (genes: a list of member lists, or a gene_of_tx vector with its n_genes) the gene map, which a new structure drops"""
    n_tx, rp, ci, _, E = prob
    dev.upload_structure(n_tx, rp, ci, layout, merge_rows)
    dev.upload_sample(R, E, den)
    if genes is not None:
        if isinstance(genes, tuple):
            dev.set_gene_map(*genes)
        else:
            dev.set_gene_map(GP.gene_map(n_tx, genes), len(genes))


def same_bits(x, y, keys=OUTPUTS):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def on_the_cut(dev_value, q):
    return abs(dev_value - q) <= DEV_TOL * q


def check_against(r, i, gene, q, what):
    """status, parts, members; D_ref(reported limit) within the tolerance of dev_*; lambda against the reference's drop"""
    xh, F_hat, _ = gene.em()
    X_hat = float(xh[gene.is_member].sum())
    _, F_drop, _ = gene.em(pin=0.0)
    lam_ref = 2.0 * (F_hat - F_drop)
    assert r["parts"][i] == gene.n_parts and r["members"][i] == gene.members, (what, r["parts"][i], r["members"][i])
    assert r["status"][i] == (TWO_SIDED if lam_ref > q else LOWER_ZERO), (what, r["status"][i], lam_ref)
    assert abs(r["gene_hat"][i] - X_hat) <= 1e-6 * X_hat, (what, r["gene_hat"][i], X_hat)
    if math.isinf(lam_ref):
        assert math.isinf(r["lambda"][i]) and r["pvalue"][i] == 0.0, (what, r["lambda"][i])
    else:
        tol = 100 * PG.SPREAD * (abs(F_hat) + abs(F_drop)) + 4 * gene.n_parts * E_F
        print(what, "Lambda", r["lambda"][i], "ref", lam_ref, "residual", r["lambda"][i] - lam_ref, "tol", tol)
        assert abs(r["lambda"][i] - lam_ref) <= tol, (what, r["lambda"][i], lam_ref, tol)
        assert r["pvalue"][i] == H.gene_presence_pvalue_host([r["lambda"][i]], [r["members"][i]])[0]
    for side in ("lower", "upper"):
        if side == "lower" and r["status"][i] == LOWER_ZERO:
            assert r["lower"][i] == 0.0 and r["dev_lower"][i] == r["lambda"][i]
            continue
        x, d = float(r[side][i]), float(r["dev_" + side][i])
        D_ref, F_pin = gene.deviance(x, F_hat)
        tol = 100 * PG.SPREAD * (abs(F_hat) + abs(F_pin)) + 1e-7 * q + 4 * gene.n_parts * E_F
        print(what, side, x, "dev", d, "D_ref", D_ref, "residual", d - D_ref, "tol", tol, "evals", r["evals"][i])
        assert on_the_cut(d, q), (what, side, d, q)
        assert abs(d - D_ref) <= tol, (what, side, d, D_ref, tol)
    assert r["lower"][i] <= r["gene_hat"][i] <= r["upper"][i]


# ---- 1. the analytic gene --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.95, 0.99])
def test_analytic_gene(dev, level):
    """rows {a}: 30, {a, b}: 50, gene {a, b}: D(x) = 2 (50 log(50 / x) - (50 - x)) for x >= 30"""
    prob, R, members = PG.analytic_problem()
    load(dev, prob, R, CP.den_of(prob), [members])
    q = q_of(level)
    r = dev.profile_genes(level=level, tol=1e-13, **CAPS)
    print({k: r[k] for k in OUTPUTS}, r["stats"].as_dict())
    assert r["status"][0] == TWO_SIDED and r["parts"][0] == 1 and r["members"][0] == 2
    assert math.isinf(r["lambda"][0]) and r["lambda"][0] > 0 and r["pvalue"][0] == 0.0         # a has reads of its own
    assert abs(r["gene_hat"][0] - 50.0) <= 1e-9 * 50.0
    for side in ("lower", "upper"):
        x, d = r[side][0], r["dev_" + side][0]
        assert on_the_cut(d, q), (side, d, q)
        assert x >= 30.0 and abs(d - float(PG.analytic_D(x))) <= 1e-9, (side, x, d, float(PG.analytic_D(x)))
    assert r["lower"][0] < 50.0 < r["upper"][0]
    st = r["stats"].as_dict()
    assert st["cut"] == q and st["items_launched"] == 3 and st["n_status"]["TWO_SIDED"] == 1 and st["evals_sum"] == r["evals"][0] <= 60


# ---- 2. closed-form genes: the host path -------------------------------------------------------------------------------------------
def test_closed_form_genes(dev):
    """lone transcripts only: nothing is launched; the bits are the diagnostic entry's"""
    rows = [[t] for t in range(8)]
    n_tx, rp, ci = CP.csr(rows, 8)
    R = np.array([30, 20, 0, 40, 0, 40, 0, 0], dtype=np.int32)
    E = np.array([2.0, 3.0, 1.0, 30.0, 30.0, 30.0, 3.0, 2.0])
    genes = [[0, 1], [2, 3], [4, 5], [6, 7]]
    load(dev, (n_tx, rp, ci, R, E), R, None, genes)
    q = q_of(0.95)
    r = dev.profile_genes(**CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert r["stats"].items_launched == 0 and np.all(r["parts"] == 2) and np.all(r["members"] == 2)
    for k, members in enumerate(genes):
        want = H.debug_profile_genes_closed(R[members].astype(float), E[members], max_evals=30)
        for key in H.PROFILE_GENE_OUTPUTS + ("status", "evals"):
            assert np.array([r[key][k]]).tobytes() == np.array([want[key]], dtype=r[key].dtype).tobytes(), (k, key, r[key][k], want[key])
    # two lone transcripts with reads against a scalar root find
    lower, upper, X_hat = PG.closed_limits([30.0, 20.0], [2.0, 3.0], q)
    assert r["status"][0] == TWO_SIDED and math.isinf(r["lambda"][0])
    assert abs(r["lower"][0] - lower) <= DEV_TOL * (X_hat - lower) and abs(r["upper"][0] - upper) <= DEV_TOL * (upper - X_hat)
    # the end of the range: the zero-read member has the strictly smallest den
    x_hat, x_end = 40.0 / 30.0, 40.0 / 29.0
    F = lambda x: 40.0 * math.log(x) - 30.0 * x
    D_end = 2.0 * (F(x_hat) - F(x_end))
    lone = H.debug_profile_genes_closed([40.0], [30.0], max_evals=30)
    assert abs(r["upper"][1] - (x_end + (q - D_end) / 2.0)) <= 1e-12 * r["upper"][1] and r["dev_upper"][1] == q
    assert H.debug_profile_genes_closed([0.0, 40.0], [1.0, 30.0], max_evals=30)["evals_upper"] == 1         # and r has its evals, above
    # tied dens: the ordinary search
    assert r["evals"][2] == lone["evals"] and r["upper"][2] == lone["upper"] and on_the_cut(r["dev_upper"][2], q)
    # no reads at all
    assert r["status"][3] == LOWER_ZERO and r["lambda"][3] == 0.0 and r["pvalue"][3] == 1.0 and r["lower"][3] == 0.0
    assert r["upper"][3] == q / (2.0 * 2.0) and r["dev_upper"][3] == q and r["gene_hat"][3] == 0.0 and r["evals"][3] == 0


def test_end_of_range_on_the_device(dev):
    """The end rule in the kernel: a zero-read lone member (den e0) with the smallest den in a gene with a set part.  Rows {1}: 30,
    {1, 2}: 50, {2}: 12 with den 2 each: along the path both scale alike, X = 46 c, D(X) = 2 (92 log(46 / X) - 2 (46 - X)), and the end
    s = 0 lies at c = 2 / (2 - e0)."""
    n_tx, rp, ci = CP.csr([[0], [1], [1, 2], [2]], 3)
    R = np.array([0, 30, 50, 12], dtype=np.int32)
    D = lambda x: 2.0 * (92.0 * math.log(46.0 / x) - 2.0 * (46.0 - x))
    q = q_of(0.95)
    out = {}
    for e0 in (0.5, 0.05):
        prob = (n_tx, rp, ci, R, np.array([e0, 1.0, 1.0, 1.0]))
        load(dev, prob, R, CP.den_of(prob), [[0, 1, 2]])
        r = out[e0] = dev.profile_genes(tol=1e-13, **CAPS)
        print(e0, {k: r[k] for k in OUTPUTS}, r["stats"].as_dict())
        assert r["status"][0] == TWO_SIDED and r["parts"][0] == 2 and r["members"][0] == 3 and math.isinf(r["lambda"][0])
        assert abs(r["gene_hat"][0] - 46.0) <= 1e-9 * 46.0
        assert on_the_cut(r["dev_lower"][0], q) and abs(r["dev_lower"][0] - D(r["lower"][0])) <= 1e-8
        assert r["stats"].items_launched == 3 and r["stats"].evals_sum == r["evals"][0]
    # e0 = 0.5: D_end = D(46 * 4 / 3) = 8.4 lies beyond the cut, the ordinary search follows the end evaluation
    r = out[0.5]
    assert D(46.0 * 2.0 / 1.5) > q
    assert on_the_cut(r["dev_upper"][0], q) and abs(r["dev_upper"][0] - D(r["upper"][0])) <= 1e-8 and 46.0 < r["upper"][0] < 46.0 * 2.0 / 1.5
    # e0 = 0.05: D_end = 0.06 < q, one evaluation and the line; the lower search is the record with the most evaluations
    r = out[0.05]
    X_end = 46.0 * 2.0 / 1.95
    assert D(X_end) < q
    want = X_end + (q - D(X_end)) / (2.0 * 0.05)
    assert r["dev_upper"][0] == q and abs(r["upper"][0] - want) <= 1e-8 * want
    assert r["stats"].evals_max >= 2 and r["evals"][0] - r["stats"].evals_max == 1


# ---- 3. against the reference in each class ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [64, 256, 512])
def test_against_the_reference(dev, threads):
    prob, RA, _, _ = CP.class_problem(threads)
    genes = GP.class_genes(threads)
    den = CP.den_of(prob)
    load(dev, prob, RA, den, genes)
    q = q_of(0.95)
    r = dev.profile_genes(tol=1e-12, **CAPS)
    for k, members in enumerate(genes):
        check_against(r, k, PG.Gene(prob, RA, members, den), q, (threads, members))
    st = r["stats"].as_dict()
    print(st)
    assert st["n_status"]["TWO_SIDED"] == len(genes) and st["parts_max"] == 1 and st["items_launched"] == 3 * len(genes)
    assert st["evals_sum"] == int(r["evals"].sum()) and st["evals_max"] <= 30 and st["cut"] == q


# ---- 4. several parts, the statuses decided on the host -----------------------------------------------------------------------------
def test_parts_loop_and_host_statuses(dev):
    prob, RA, RB, den_a, den_b = CP.small_problem()
    q95, q99 = q_of(0.95), q_of(0.99)
    load(dev, prob, RA, den_a, SMALL_X)
    r = dev.profile_genes(tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    # {0, 3, 6}: a member in no set (0, closed form) and two set parts
    check_against(r, 0, PG.Gene(prob, RA, SMALL_X[0], den_a), q95, "small A {0, 3, 6}")
    assert r["parts"][0] == 3 and r["members"][0] == 3
    # {8, 9}: no reads anywhere
    assert r["status"][1] == LOWER_ZERO and r["lambda"][1] == 0.0 and r["upper"][1] == q95 / (2.0 * min(den_a[8], den_a[9])) and r["evals"][1] == 0
    wide = dev.profile_genes(level=0.99, tol=1e-12, **CAPS)
    given = np.isin(r["status"], (TWO_SIDED, LOWER_ZERO))
    assert given.sum() == len(SMALL_X)
    assert np.all(wide["lower"][given] <= r["lower"][given]) and np.all(wide["upper"][given] >= r["upper"][given])
    assert np.all(r["lower"][given] <= r["gene_hat"][given]) and np.all(r["gene_hat"][given] <= r["upper"][given])
    assert r["gene_hat"].tobytes() == wide["gene_hat"].tobytes() and r["lambda"].tobytes() == wide["lambda"].tobytes()
    theta = dev.solve(tol=1e-12, max_iter=20000)[0]
    sums = dev.gene_sums(theta)
    assert np.all(np.abs(r["gene_hat"] - sums) <= 1e-12 * sums)
    # sample B: 10 has den = 0 -> {10} is OUTSIDE; 6 has no read to its name there
    load(dev, prob, RB, den_b, SMALL_X)
    b = dev.profile_genes(tol=1e-12, **CAPS)
    print({k: b[k] for k in OUTPUTS})
    assert b["status"][2] == OUTSIDE and b["evals"][2] == 0 and b["parts"][2] == 0 and b["members"][2] == 0
    for k in H.PROFILE_GENE_OUTPUTS:
        assert math.isnan(b[k][2]), k
    check_against(b, 0, PG.Gene(prob, RB, SMALL_X[0], den_b), q95, "small B {0, 3, 6}")
    load(dev, prob, RB, den_b, SMALL_Y)
    y = dev.profile_genes(tol=1e-12, **CAPS)
    check_against(y, 1, PG.Gene(prob, RB, SMALL_Y[1], den_b), q95, "small B {4, 10}")
    assert y["members"][1] == 1 and y["parts"][1] == 1       # 10 takes no part
    st = y["stats"].as_dict()
    assert sum(st["n_status"].values()) == len(SMALL_Y)


# ---- 5. one-member genes are the transcript profile -----------------------------------------------------------------------------------
def invariance_problem():
    from tests.test_compare_gpu import invariance_problem as ip
    prob, RA, _ = ip()
    return prob, RA


def test_one_member_genes_are_the_transcript_profile(dev):
    prob, R = invariance_problem()
    den = CP.den_of(prob)
    kw = dict(max_iter=3000, max_evals=30)
    load(dev, prob, R, den, (np.arange(prob[0], dtype=np.int32), prob[0]), H.LAYOUT_CSR)
    g, t = dev.profile_genes(**kw), dev.profile(**kw)
    print(g["stats"].as_dict(), t["stats"].as_dict())
    assert np.array_equal(g["status"], t["status"])
    given = np.isin(t["status"], (TWO_SIDED, LOWER_ZERO, UNCONVERGED))
    assert given.sum() >= 30 and np.all(g["members"][given] == 1)
    fin = given & np.isfinite(t["lambda"])
    assert np.array_equal(np.isinf(g["lambda"]), np.isinf(t["lambda"]))
    print("max rel dLambda", np.max(np.abs(g["lambda"][fin] - t["lambda"][fin]) / np.maximum(t["lambda"][fin], 1e-300)) if fin.any() else None)
    assert np.all(np.abs(g["lambda"][fin] - t["lambda"][fin]) <= 1e-9 * t["lambda"][fin])
    # both lie within dev_tol q of the cut, and the slope of D at a limit is about 2 q / half-width
    width = t["upper"][given] - t["lower"][given]
    assert np.all(np.abs(g["lower"][given] - t["lower"][given]) <= 2 * DEV_TOL * width)
    assert np.all(np.abs(g["upper"][given] - t["upper"][given]) <= 2 * DEV_TOL * width)
    assert g["gene_hat"].tobytes() == t["theta_hat"].tobytes()


# ---- 6. bit-for-bit invariance ------------------------------------------------------------------------------------------------------
def drawn_genes(n_tx, seed=9):
    """genes of 1 .. 4 members drawn over all transcripts: many span two sets"""
    rng = np.random.default_rng(seed)
    order, genes, at = rng.permutation(n_tx), [], 0
    while at < n_tx:
        k = int(rng.integers(1, 5))
        genes.append([int(x) for x in order[at:at + k]])
        at += k
    return genes


def config(monkeypatch, dev, prob, R, den, genes, layout, merge, mode):
    if mode is None:
        monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
    else:
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", mode)
    load(dev, prob, R, den, genes, layout, merge)
    if mode is not None:
        assert dev.info()["renumbered"] == int(mode == "2")


def test_invariance_bit_for_bit(dev, monkeypatch):
    prob, R = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    ng = len(genes)
    kw = dict(max_iter=3000, max_evals=30)
    tids = np.arange(0, prob[0], 7, dtype=np.int32)
    config(monkeypatch, dev, prob, R, den, genes, H.LAYOUT_CSR, False, None)
    before = [dev.solve(max_iter=3000)[0], dev.profile(tids, **kw)]
    whole = dev.profile_genes(**kw)
    after = [dev.solve(max_iter=3000)[0], dev.profile(tids, **kw)]
    assert before[0].tobytes() == after[0].tobytes()
    assert not [k for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda", "theta_hat", "status", "evals") if before[1][k].tobytes() != after[1][k].tobytes()]
    st = whole["stats"].as_dict()
    print(st)
    searched = st["n_status"]["TWO_SIDED"] + st["n_status"]["LOWER_ZERO"]
    assert searched >= 20 and searched + st["n_status"]["UNCONVERGED"] == ng and st["evals_max"] <= 30
    assert st["parts_max"] >= 2 and np.sum(whole["parts"] > 1) >= 5               # genes that span sets
    q = np.random.default_rng(5).permutation(ng).astype(np.int32)
    shuffled = dev.profile_genes(q, **kw)
    twice = dev.profile_genes(np.concatenate([q[:10], q[:10], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_PROFILE_GENES_BATCH", "1")      # one item per class and launch
    single = dev.profile_genes(**kw)
    monkeypatch.delenv("EMSAR_HIP_PROFILE_GENES_BATCH")
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][20:].tobytes() == shuffled[k].tobytes() and twice[k][:10].tobytes() == twice[k][10:20].tobytes() == shuffled[k][:10].tobytes(), k
        assert single[k].tobytes() == whole[k].tobytes(), k
    assert sum(twice["stats"].as_dict()["n_status"].values()) == ng
    for layout, merge, mode in ((H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"), (H.LAYOUT_TILED, True, "2")):
        config(monkeypatch, dev, prob, R, den, genes, layout, merge, mode)
        assert not same_bits(dev.profile_genes(**kw), whole), (layout, merge, mode)


# ---- 7. statuses and errors ---------------------------------------------------------------------------------------------------------
def test_statuses_and_errors(dev):
    prob, RA, RB, den_a, den_b = CP.small_problem()
    load(dev, prob, RA, den_a, SMALL_X)
    r1 = dev.profile_genes(set_mode=1, **CAPS)
    assert np.all(r1["status"] == NOT_RESIDENT) and r1["stats"].items_launched == 0
    assert np.all(r1["evals"] == 0) and np.all(r1["parts"] == 0) and np.all(r1["members"] == 0)
    for k in H.PROFILE_GENE_OUTPUTS:
        assert np.all(np.isnan(r1[k])), k
    full = dev.profile_genes(**CAPS)
    capped = dev.profile_genes(max_iter=20000, max_evals=1)
    moved = np.flatnonzero(np.isin(full["status"], (TWO_SIDED, LOWER_ZERO)) & (full["evals"] > 2))
    assert len(moved) >= 3
    assert np.all(capped["status"][moved] == UNCONVERGED) and np.all(capped["evals"][moved] <= 2)
    assert capped["gene_hat"].tobytes() == full["gene_hat"].tobytes() and capped["lambda"].tobytes() == full["lambda"].tobytes()
    for bad in (dict(query=[0, len(SMALL_X)]), dict(query=[-1]), dict(level=0.0), dict(level=1.0), dict(level=math.nan), dict(dev_tol=math.inf),
                dict(dev_tol=math.nan), dict(set_mode=2), dict(count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            dev.profile_genes(**bad, **CAPS)
        assert e.value.status == -1, bad
    L = H.load_library()
    assert L.emsar_hip_profile_genes(dev._h, None, None, -1, np.zeros(1, dtype=np.int32).ctypes.data_as(H.C.POINTER(H.C.c_int32)), None, None) == -1
    assert L.emsar_hip_profile_genes(None, None, None, 0, None, None, None) == -1
    assert not same_bits(dev.profile_genes(**CAPS), full)
    with emsar_amd.EmsarHip(0) as d:
        n_tx, rp, ci, _, E = prob
        d.upload_structure(n_tx, rp, ci)
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            d.profile_genes(**CAPS)                           # before upload_sample
        assert e.value.status == -5
        d.upload_sample(RA, E, den_a)
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            d.profile_genes(**CAPS)                           # no gene map
        assert e.value.status == -5
        d.set_gene_map(GP.gene_map(n_tx, SMALL_X), len(SMALL_X))
        assert not same_bits(d.profile_genes(**CAPS), full)
        # a lone transcript with reads and an infinite den given by the caller: x = 0, F_hat is not finite
        bad_den = den_a.copy()
        bad_den[1] = math.inf
        d.upload_sample(RA, E, bad_den)
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            d.profile_genes([3], **CAPS)                      # gene {1}: on the host, nothing is launched
        assert e.value.status == -6


def test_streamed_member(dev):
    """everything_problem: a gene with a member in the streamed set is NOT_RESIDENT, its neighbours in the query are not touched by it"""
    prob = SP.everything_problem()
    n_tx, R = prob[0], prob[3]
    den = CP.den_of(prob)
    genes = (np.arange(n_tx, dtype=np.int32) // 3, (n_tx + 2) // 3)
    load(dev, prob, R, den, genes)
    kw = dict(max_iter=2000, max_evals=30)
    r = dev.profile_genes(**kw)
    st = r["stats"].as_dict()
    print(st)
    assert st["n_status"]["NOT_RESIDENT"] >= 1 and st["n_status"]["TWO_SIDED"] + st["n_status"]["LOWER_ZERO"] + st["n_status"]["UNCONVERGED"] >= 20
    off = np.flatnonzero(r["status"] == NOT_RESIDENT)
    assert np.all(r["evals"][off] == 0) and np.all(np.isnan(r["lambda"][off])) and np.all(r["members"][off] == 0)
    on = np.flatnonzero(r["status"] != NOT_RESIDENT).astype(np.int32)
    alone = dev.profile_genes(on, **kw)
    for k in OUTPUTS:
        assert alone[k].tobytes() == r[k][on].tobytes(), k


def test_too_large(dev):
    """65 one-transcript rows in one gene: TOO_LARGE; 64: searched on the host; 63 closed-form parts and a set part: one launched gene"""
    n = 65 + 64 + 2
    rows = [[t] for t in range(n)] + [[n - 2, n - 1]]
    n_tx, rp, ci = CP.csr(rows, n)
    R = np.random.default_rng(3).integers(1, 40, size=len(rows)).astype(np.int32)
    prob = (n_tx, rp, ci, R, np.ones(len(rows)))
    g = np.full(n, -1, dtype=np.int32)
    g[:65] = 0
    g[65:129] = 1
    load(dev, prob, R, None, (g, 2))
    r = dev.profile_genes(**CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert r["status"][0] == TOO_LARGE and r["evals"][0] == 0 and r["parts"][0] == 0 and r["members"][0] == 0
    assert all(math.isnan(r[k][0]) for k in H.PROFILE_GENE_OUTPUTS)
    assert r["status"][1] == TWO_SIDED and r["parts"][1] == 64 and r["members"][1] == 64 and r["stats"].items_launched == 0
    den = CP.den_of(prob)
    lower, upper, X_hat = PG.closed_limits(R[65:129].astype(float), den[65:129], q_of(0.95))
    assert abs(r["lower"][1] - lower) <= DEV_TOL * (X_hat - lower) and abs(r["upper"][1] - upper) <= DEV_TOL * (upper - X_hat)
    g2 = np.full(n, -1, dtype=np.int32)
    g2[list(range(1, 64)) + [n - 1]] = 0
    dev.set_gene_map(g2, 1)
    r = dev.profile_genes(**CAPS)
    assert r["status"][0] == TWO_SIDED and r["parts"][0] == 64 and r["stats"].items_launched == 3 and r["stats"].parts_max == 64


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------
def test_cli_gprofile_file(tmp_path):
    """--profile --g2t on the syn300_se fixture: out.0.gprofile has one line per gene in the order of .gfpkm and its columns are the Python
    call's as printed; out.0.profile keeps its bytes; without --g2t no .gprofile; --profile-list filters transcripts only"""
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
    base = [_build.CLI, "-q", "-i", "20000", "--gpus", "1", "--profile", "--profile-evals", "30"] + fx.meta["opts"]
    subprocess.run(base + ["-I", rsh_path, str(tmp_path / "p"), "out", aln], check=True, timeout=300)
    subprocess.run(base + ["--g2t", str(g2t), "-I", rsh_path, str(tmp_path / "o"), "out", aln], check=True, timeout=300)
    subprocess.run(base + ["--g2t", str(g2t), "--profile-list", str(lst), "-I", rsh_path, str(tmp_path / "l"), "out", aln], check=True, timeout=300)
    assert (tmp_path / "o" / "out.0.profile").read_bytes() == (tmp_path / "p" / "out.0.profile").read_bytes()
    assert not (tmp_path / "p" / "out.0.gprofile").exists()
    assert (tmp_path / "l" / "out.0.gprofile").read_bytes() == (tmp_path / "o" / "out.0.gprofile").read_bytes()
    assert len((tmp_path / "l" / "out.0.profile").read_text().splitlines()) == 6
    got = [l.split("\t") for l in (tmp_path / "o" / "out.0.gprofile").read_text().splitlines()]
    assert got[0] == ["gene", "gFPKM", "lower", "upper", "Lambda", "p", "members", "status"]
    got = got[1:]
    gfpkm = [l.split("\t") for l in (tmp_path / "o" / "out.0.gfpkm").read_text().splitlines()][-n_genes:]
    assert len(got) == n_genes and all(len(r) == 8 for r in got)
    assert [r[0] for r in got] == [r[0] for r in gfpkm] and [r[1] for r in got] == [r[1] for r in gfpkm]
    order = {name: k for k, name in enumerate(r[0] for r in got)}
    gene_of = np.array([order["gene%04d" % (t // 3)] for t in range(rsh.n_tx)], dtype=np.int32)
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
        p = d.profile_genes(**cli)
    assert [r[7] for r in got] == [H.PROFILE_GENE_STATUS[k] for k in p["status"]]
    assert [int(r[6]) for r in got] == list(p["members"])
    for col, key in ((2, "lower"), (3, "upper"), (4, "lambda")):
        v = np.array([float(r[col]) for r in got])
        fin = np.isfinite(p[key])
        assert np.array_equal(np.isnan(v), np.isnan(p[key])) and np.array_equal(v[~fin & ~np.isnan(v)], p[key][~fin & ~np.isnan(p[key])]), key
        assert np.all(np.abs(v[fin] - p[key][fin]) <= 1e-6 + 1e-15 * np.abs(p[key][fin])), key          # "%lf"
    assert [r[5] for r in got] == ["nan" if math.isnan(x) else "%.6g" % x for x in p["pvalue"]]
    print(p["stats"].as_dict())
    assert np.sum(np.isin(p["status"], (TWO_SIDED, LOWER_ZERO))) >= 10
