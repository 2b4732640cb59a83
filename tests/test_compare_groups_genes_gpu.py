"""GPU: the gene-level K-sample test across replicate groups (emsar_hip_compare_groups_genes, include/emsar_hip.h "gene-level K-sample
test") against the independent numpy reference of tests/compare_groups_gene_problems.py (a sandwich of a dual and a primal bound made of
plain EMs; the long cases recorded in tests/golden/compare_groups_gene_refs.json), against emsar_hip_compare_genes at K = 2 and
emsar_hip_compare_groups on one-member genes, on identical samples, at the end of the multiplier's range, for bit-identity under
everything a result must not depend on, on the paths that are not searched or searched on the host, on its argument errors, and through
the CLI.

The tolerance on a Lambda is derived as test_compare_groups_gpu.py and test_compare_genes_gpu.py derive theirs, from figures the project
already holds: DEV_TOL = 1e-4 and E_F = 4 x 9.4e-10 (test_compare_gpu.py's figure, measured on the existing set solver and not on this
code).  Every searched item (the all-samples search, the search of a group of two or more) that enters a Lambda is granted
(|S| + 1) dev_tol: each of its |S| inner searches and its outer search dev_tol -- their stopping rules bound it.  Every part's F that
enters adds 2 e_F, twice over for the two sums of a Lambda: Lambda_between 4 P_all e_F (P_all = the parts of all samples),
Lambda_within 4 e_F x the parts of the samples in groups of two or more (a group of one cancels exactly).  The reference's own width
comes on top.  The common values are compared at 1e-3 relative plus 1e-6 of the outer bracket's width, gene_hat at 1e-6 relative plus
1e-6 (the solver's abs_floor) per member.

Every call passes max_iter <= 20000 and the default caps, K <= 4: no workgroup can run long."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import compare_gene_problems as GP
from tests import compare_groups_gene_problems as CGG
from tests import compare_groups_problems as CGP
from tests import compare_problems as CP
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TESTED, ALL_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE = range(6)
DEV_TOL = 1e-4
E_F = 4 * 9.4e-10
CAPS = dict(max_iter=20000)
OUTPUTS = H.GROUPS_GENE_OUTPUTS + ("gene_group", "gene_hat") + H.GROUPS_GENE_COUNTS


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b, emsar_amd.EmsarHip(0) as c, emsar_amd.EmsarHip(0) as d:
        yield a, b, c, d


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


def load_all(devs, prob, Rs, dens, genes, **kw):
    """sample k into context k, the gene map on the first one"""
    for k, (dev, R, den) in enumerate(zip(devs, Rs, dens)):
        load(dev, prob, R, den, genes if k == 0 else None, **kw)


def same_bits(x, y, keys=OUTPUTS):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def searched_groups(groups):
    return [n for n in (list(groups).count(g) for g in range(max(groups) + 1)) if 2 <= n]


def tolerances(groups, parts, w_between, w_within):
    """parts: per sample"""
    K, G = len(groups), max(groups) + 1
    multi = searched_groups(groups)
    in_multi = sum(p for k, p in enumerate(parts) if list(groups).count(groups[k]) >= 2)
    within = sum(n + 1 for n in multi) * DEV_TOL + 4 * E_F * in_multi + w_within
    between = 0.0 if G == 1 else ((K + 1) + sum(n + 1 for n in multi)) * DEV_TOL + 4 * sum(parts) * E_F + w_between
    return between, within


def items_per_gene(groups):
    return 1 + sum(1 for n in searched_groups(groups) if n < len(groups))


def check_against(r, i, ref, groups, what, sizes=None):
    tb, tw = tolerances(groups, ref["parts"], ref["w_between"], ref["w_within"])
    print(what, "between", r["lambda_between"][i], "ref", ref["lam_between"], "residual", r["lambda_between"][i] - ref["lam_between"], "tol", tb,
          "| within", r["lambda_within"][i], "ref", ref["lam_within"], "residual", r["lambda_within"][i] - ref["lam_within"], "tol", tw,
          "| common", r["gene_common"][i], ref["gene_common"], "group", r["gene_group"][i], ref["gene_group"], "hat", r["gene_hat"][i], ref["gene_hat"],
          "| outer", r["outer"][i], "evals", r["evals"][i], "parts", r["parts"][i], "slope", r["slope"][i])
    assert ref["w_between"] <= CGG.W_REF_MAX and ref["w_within"] <= CGG.W_REF_MAX and ref["ended_by_step"]
    assert r["status"][i] == TESTED, (what, r["status"][i])
    assert abs(r["lambda_between"][i] - ref["lam_between"]) <= tb, (what, r["lambda_between"][i], ref["lam_between"], tb)
    assert abs(r["lambda_within"][i] - ref["lam_within"]) <= tw, (what, r["lambda_within"][i], ref["lam_within"], tw)
    ends = [x / s for x, s in zip(ref["gene_hat"], sizes or [1.0] * len(groups))]
    width = 1e-6 * (max(ends) - min(ends))
    assert abs(r["gene_common"][i] - ref["gene_common"]) <= 1e-3 * ref["gene_common"] + width, (what, r["gene_common"][i], ref["gene_common"])
    for g, x in enumerate(ref["gene_group"]):
        assert abs(r["gene_group"][i][g] - x) <= 1e-3 * x + width, (what, g, r["gene_group"][i][g], x)
    for k, x in enumerate(ref["gene_hat"]):
        assert abs(r["gene_hat"][i][k] - x) <= 1e-6 * x + 1e-6 * ref["n_members"], (what, k, r["gene_hat"][i][k], x)
    assert r["parts"][i] == sum(ref["parts"]), (what, r["parts"][i], ref["parts"])
    df = (max(groups), len(groups) - max(groups) - 1)
    assert r["p_between"][i] == H.compare_groups_pvalue_host([r["lambda_between"][i]], df[0])[0]
    assert r["p_within"][i] == H.compare_groups_pvalue_host([r["lambda_within"][i]], df[1])[0]


def check_stats(r, groups, n_device):
    """n_device genes went to the device, all of them TESTED"""
    st = r["stats"].as_dict()
    print(st)
    assert st["items_launched"] == items_per_gene(groups) * n_device
    assert st["df_between"] == max(groups) and st["df_within"] == len(groups) - max(groups) - 1
    return st


# ---- 1. the independent reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in CGP.CLASS_CASES])
def test_reference_class64(devs, case):
    """three genes of three members inside one 64-class set: K = 3 in two groups, K = 4 in two groups with size factors, K = 3 in three"""
    prob, Rs, dens, _, groups, sizes = CGG.class_case(64, case)
    genes = GP.class_genes(64)
    load_all(devs, prob, Rs, dens, genes)
    r = devs[0].compare_groups_genes(devs[1:len(Rs)], groups, sizes, tol=1e-12, **CAPS)
    for i in range(len(genes)):
        check_against(r, i, CGG.recorded()["class64-%d/%s" % (i, case)], groups, ("class64", i, case), sizes)
    st = check_stats(r, groups, len(genes))
    assert st["evals_sum"] == int(r["evals"].sum()) and st["n_status"]["TESTED"] == len(genes) and st["parts_max"] == len(Rs)


@pytest.mark.parametrize("name", ["class256/k3_001", "class512/k3_001", "mixed", "split"])
def test_reference_large_classes(devs, name):
    """one gene in the 256 and in the 512 class; a 64-class and a 256-class part in one gene (the launch class is the largest part's);
    the gene's set in the 64 class in one sample and in the 512 class in the others"""
    prob, Rs, dens, members, groups, sizes = CGG.case_inputs(name)
    load_all(devs, prob, Rs, dens, [members])
    r = devs[0].compare_groups_genes(devs[1:len(Rs)], groups, sizes, tol=1e-12, **CAPS)
    check_against(r, 0, CGG.recorded()[name], groups, name, sizes)
    st = check_stats(r, groups, 1)
    assert st["evals_sum"] == int(r["evals"][0]) and st["parts_max"] == r["parts"][0] == (6 if name == "mixed" else 3)


def test_reference_small_and_awkward(devs):
    """closed-form and set parts mixed, a member without reads, a member with den = 0 in one sample; then the awkward gene: a den = 0
    member, a transcript twice in a row, one alone in its row"""
    prob, Rs, dens = CGP.small_samples()
    groups = (0, 0, 1)
    load_all(devs, prob, Rs, dens, [[0, 3, 6], [4, 10]])
    r = devs[0].compare_groups_genes(devs[1:3], groups, tol=1e-12, **CAPS)
    check_against(r, 0, CGG.live_reference("small-0-3-6"), groups, "small-0-3-6")
    check_against(r, 1, CGG.live_reference("small-4-10"), groups, "small-4-10")
    st = check_stats(r, groups, 2)
    assert st["evals_sum"] == int(r["evals"].sum()) and r["parts"][0] == 9 and r["parts"][1] == 3
    prob, Rs, dens, gene, groups, _ = CGG.awkward_case()
    from tests import awkward_problems as AP
    outside = int(AP.awkward_members()[1]["outside"])
    assert dens[0][outside] == 0.0 and outside in gene
    load_all(devs, prob, Rs, dens, [gene, [outside]])
    r = devs[0].compare_groups_genes(devs[1:3], groups, tol=1e-12, **CAPS)
    check_against(r, 0, CGG.live_reference("awkward"), groups, "awkward")
    assert r["status"][1] == OUTSIDE and r["parts"][1] == 0
    check_stats(r, groups, 1)


# ---- 2. K = 2 is the two-sample gene test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [64, 256, 512])
def test_two_samples_are_the_gene_compare_statistic(devs, threads):
    """groups (0, 1) with sizes (r, 1) is emsar_hip_compare_genes at ratio r reached by another search -- within 3 dev_tol (the two inner
    searches and the outer one here) + dev_tol (the search there); gene_hat has its bits; groups (0, 0) puts the same bits into
    lambda_within"""
    a, b = devs[:2]
    prob, RA, RB, _ = CP.class_problem(threads)
    den = CP.den_of(prob)
    genes = GP.class_genes(threads)
    load(a, prob, RA, den, genes)
    load(b, prob, RB, den)
    for ratio in (1.0, 1.6):
        cmp_ = a.compare_genes(b, ratio=ratio, tol=1e-12, **CAPS)
        two = a.compare_groups_genes([b], (0, 1), (ratio, 1.0), tol=1e-12, **CAPS)
        one = a.compare_groups_genes([b], (0, 0), (ratio, 1.0), tol=1e-12, **CAPS)
        print(threads, ratio, "between", two["lambda_between"], "compare_genes", cmp_["lambda"], "outer", two["outer"], "evals", two["evals"])
        assert np.all(cmp_["status"] == 0) and np.all(two["status"] == TESTED)
        assert np.all(np.abs(two["lambda_between"] - cmp_["lambda"]) <= 3 * DEV_TOL + DEV_TOL)
        assert two["gene_hat"][:, 0].tobytes() == cmp_["gene_a"].tobytes() and two["gene_hat"][:, 1].tobytes() == cmp_["gene_b"].tobytes()
        assert np.array_equal(two["parts"], cmp_["parts"])
        assert np.all(two["lambda_within"] == 0.0) and np.all(two["p_within"] == 1.0)
        assert two["stats"].df_between == 1 and two["stats"].df_within == 0 and two["stats"].items_launched == len(genes)
        assert one["lambda_within"].tobytes() == two["lambda_between"].tobytes() and np.all(one["lambda_between"] == 0.0)
        assert one["stats"].df_between == 0 and one["stats"].df_within == 1 and np.all(one["p_between"] == 1.0)
        assert one["gene_common"].tobytes() == two["gene_common"].tobytes() and one["gene_group"][:, 0].tobytes() == one["gene_common"].tobytes()


# ---- 3. a one-member gene is the transcript test ---------------------------------------------------------------------------------------
def invariance_samples():
    from tests.test_compare_gpu import invariance_problem
    prob, RA, RB = invariance_problem()
    return prob, [RA, CP.fitted_weights(prob, 43), RB, CP.fitted_weights(prob, 44, apart=range(0, prob[0], 3))]


def test_one_member_genes_are_the_transcript_test(devs):
    """the identity map: every gene is one transcript.  Both calls stop by the same rules at points of their own: the allowance is the
    sum of both calls' stopping allowances; gene_hat is theta_hat within the solver's floor"""
    prob, Rs = invariance_samples()
    den = CP.den_of(prob)
    groups = (0, 0, 1)
    kw = dict(max_iter=3000)
    load_all(devs, prob, Rs[:3], [den] * 3, (np.arange(prob[0], dtype=np.int32), prob[0]), layout=H.LAYOUT_CSR)
    g = devs[0].compare_groups_genes(devs[1:3], groups, **kw)
    t = devs[0].compare_groups(devs[1:3], groups, **kw)
    ok = np.isin(t["status"], (TESTED, UNCONVERGED))
    tb, tw = 2 * ((3 + 1) + (2 + 1)) * DEV_TOL, 2 * (2 + 1) * DEV_TOL
    print("tested", ok.sum(), "max |d between|", np.abs(g["lambda_between"][ok] - t["lambda_between"][ok]).max(), "tol", tb,
          "max |d within|", np.abs(g["lambda_within"][ok] - t["lambda_within"][ok]).max(), "tol", tw)
    assert np.array_equal(g["status"], t["status"]) and ok.sum() >= 30
    assert np.all(np.abs(g["lambda_between"][ok] - t["lambda_between"][ok]) <= tb) and np.all(np.abs(g["lambda_within"][ok] - t["lambda_within"][ok]) <= tw)
    assert np.all(np.abs(g["gene_hat"][ok] - t["theta_hat"][ok]) <= 1e-6 * t["theta_hat"][ok] + 1e-6)
    assert np.all(g["parts"][ok] == 3)


# ---- 4. identical samples --------------------------------------------------------------------------------------------------------------
def test_identical_samples(devs):
    """three contexts holding one sample: both Lambdas, both raw values and the slope exactly 0.0, one outer point, p = 1"""
    a, b, c = devs[:3]
    prob = SP.all_resident_problem()
    genes = (np.arange(prob[0], dtype=np.int32) // 3, (prob[0] + 2) // 3)
    den = CP.den_of(prob)
    load_all((a, b, c), prob, [prob[3]] * 3, [den] * 3, genes)
    r = a.compare_groups_genes([b, c], (0, 0, 1), max_iter=4000)
    given = ~np.isin(r["status"], (OUTSIDE, NOT_RESIDENT, TOO_LARGE))
    print(r["stats"].as_dict())
    assert given.sum() > 0.9 * genes[1]
    for k in ("lambda_between", "lambda_within", "raw_between", "raw_within", "slope"):
        assert np.all(r[k][given] == 0.0), k
    assert np.all(r["outer"][given] == 1) and np.all(r["p_between"][given] == 1.0) and np.all(r["p_within"][given] == 1.0)
    assert r["gene_hat"][given, 0].tobytes() == r["gene_hat"][given, 1].tobytes() == r["gene_hat"][given, 2].tobytes()
    assert r["gene_common"][given].tobytes() == r["gene_hat"][given, 0].tobytes()
    assert np.all((r["status"][given] == ALL_ABSENT) == (r["gene_hat"][given, 0] == 0.0))
    assert np.sum(r["status"] == TESTED) > 0.5 * genes[1]


# ---- 5. a sample in which the gene has no reads ----------------------------------------------------------------------------------------
def test_a_sample_without_reads_is_the_end_of_the_range(devs):
    """X_hat^B = 0 and the member at the smallest den has no reads: B's inner searches run to the end of the multiplier's range, where
    P_B(y) = -mn y in closed form; the gene is a set part in the other samples, so the searches run on the device"""
    prob, Rs, dens, members, groups, _ = CGG.no_reads_case()
    load_all(devs, prob, Rs, dens, [members])
    r = devs[0].compare_groups_genes(devs[1:3], groups, tol=1e-12, **CAPS)
    check_against(r, 0, CGG.live_reference("no-reads"), groups, "no-reads")
    assert r["gene_hat"][0][1] == 0.0 and r["stats"].items_launched == 2 and r["parts"][0] == 4


# ---- 6. bit-for-bit invariance ---------------------------------------------------------------------------------------------------------
def drawn_genes(n_tx, seed=9):
    """genes of 1 .. 4 members drawn over all transcripts: many span two sets"""
    rng = np.random.default_rng(seed)
    order, genes, at = rng.permutation(n_tx), [], 0
    while at < n_tx:
        k = int(rng.integers(1, 5))
        genes.append([int(x) for x in order[at:at + k]])
        at += k
    return genes


def test_invariance_bit_for_bit(devs, monkeypatch):
    prob, Rs = invariance_samples()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    ng = len(genes)
    kw = dict(max_iter=3000)
    groups = (0, 0, 1, 1)
    tids = np.arange(0, prob[0], 7, dtype=np.int32)

    def config(layout, merge, mode, maps=(True, False, False, False)):
        if mode is None:
            monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
        else:
            monkeypatch.setenv("EMSAR_HIP_RENUMBER", mode)
        for dev, R, m in zip(devs, Rs, maps):
            load(dev, prob, R, den, genes if m else None, layout, merge)
    config(H.LAYOUT_CSR, False, None, (True, False, True, False))
    a = devs[0]

    def others():
        return [d.solve(**kw)[0] for d in devs], a.compare_groups(devs[1:], groups, None, tids, **kw), a.compare_genes(devs[2], **kw)
    before = others()
    whole = a.compare_groups_genes(devs[1:], groups, **kw)
    after = others()
    for x, y in zip(before[0], after[0]):
        assert x.tobytes() == y.tobytes()
    assert not [k for k in H.GROUPS_OUTPUTS + ("theta_group", "theta_hat") + H.GROUPS_COUNTS if before[1][k].tobytes() != after[1][k].tobytes()]
    assert not [k for k in H.COMPARE_GENE_OUTPUTS + ("status", "evals", "parts") if before[2][k].tobytes() != after[2][k].tobytes()]
    st = whole["stats"].as_dict()
    print(st)
    assert st["n_status"]["TESTED"] >= 20 and st["n_status"]["TESTED"] + st["n_status"]["UNCONVERGED"] == ng
    assert st["outer_max"] <= 12 and st["items_launched"] <= 3 * ng and st["parts_max"] >= 8 and np.sum(whole["parts"] > 4) >= 5   # genes that span sets
    q = np.random.default_rng(5).permutation(ng).astype(np.int32)
    shuffled = a.compare_groups_genes(devs[1:], groups, None, q, **kw)
    twice = a.compare_groups_genes(devs[1:], groups, None, np.concatenate([q[:10], q[:10], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_GROUPS_GENES_BATCH", "1")      # one item per class and launch
    single = a.compare_groups_genes(devs[1:], groups, None, q[:12], **kw)
    monkeypatch.delenv("EMSAR_HIP_GROUPS_GENES_BATCH")
    swapped = a.compare_groups_genes(devs[1:], (1, 1, 0, 0), **kw)
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][20:].tobytes() == shuffled[k].tobytes() and twice[k][:10].tobytes() == twice[k][10:20].tobytes() == shuffled[k][:10].tobytes(), k
        assert single[k].tobytes() == shuffled[k][:12].tobytes(), k
        if k != "gene_group":
            assert swapped[k].tobytes() == whole[k].tobytes(), k
    assert swapped["gene_group"][:, ::-1].tobytes() == whole["gene_group"].tobytes()
    assert sum(twice["stats"].as_dict()["n_status"].values()) == ng
    # the map on every context, and on the first alone
    for maps in ((True, True, True, True), (True, False, False, False)):
        config(H.LAYOUT_CSR, False, None, maps)
        assert not same_bits(a.compare_groups_genes(devs[1:], groups, **kw), whole), maps
    for layout, merge, mode in ((H.LAYOUT_AUTO, False, None), (H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"),
                                (H.LAYOUT_TILED, True, "2")):
        config(layout, merge, mode)
        assert not same_bits(a.compare_groups_genes(devs[1:], groups, **kw), whole), (layout, merge, mode)
    monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
    load(devs[1], prob, Rs[1], den, None, H.LAYOUT_CSR)          # the contexts need not share a layout or a numbering
    assert not same_bits(a.compare_groups_genes(devs[1:], groups, **kw), whole)


# ---- 7. statuses and host paths --------------------------------------------------------------------------------------------------------
SMALL_GENES = [[3, 6], [4], [8, 9], [10], [0, 1], [2], [5, 7]]       # disjoint: a transcript has one gene


def test_statuses_and_host_paths(devs):
    a, b, c = devs[:3]
    prob, Rs, dens = CGP.small_samples()
    groups = (0, 0, 1)
    load_all((a, b, c), prob, Rs, dens, SMALL_GENES + [[]])       # the last gene has no transcript
    r = a.compare_groups_genes([b, c], groups, tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    # all parts closed form in every sample: the host's searches, the bits of the diagnostic entry the CPU tests check
    for i, gene in ((4, [0, 1]), (2, [8, 9])):
        want = H.debug_compare_groups_genes_closed([[(float(R[t]) if t < 2 else 0.0, d[t]) for t in gene] for R, d in zip(Rs, dens)], groups)   # rows 0, 1 hold 0, 1 alone
        for k in OUTPUTS:
            assert np.asarray(r[k][i]).tobytes() == np.asarray(want[k], dtype=r[k].dtype).tobytes(), (gene, k, r[k][i], want[k])
    assert r["status"][4] == TESTED and r["lambda_between"][4] > 0.0 and r["parts"][4] == 6
    assert r["status"][2] == ALL_ABSENT and r["lambda_between"][2] == 0.0 and r["lambda_within"][2] == 0.0 and r["p_between"][2] == 1.0 and r["outer"][2] == 1
    # den = 0 in one sample for the only member; no transcript at all
    for i in (3, 7):
        assert r["status"][i] == OUTSIDE and r["outer"][i] == 0 and r["evals"][i] == 0 and r["parts"][i] == 0
        for k in H.GROUPS_GENE_OUTPUTS:
            assert math.isnan(r[k][i]), (i, k)
        assert np.all(np.isnan(r["gene_group"][i])) and np.all(np.isnan(r["gene_hat"][i]))
    dev = np.array([0, 1, 5, 6])
    assert np.all(r["status"][dev] == TESTED)
    st = r["stats"].as_dict()
    print(st)
    assert sum(st["n_status"].values()) == len(SMALL_GENES) + 1 and st["n_status"]["OUTSIDE"] == 2 and st["n_status"]["ALL_ABSENT"] == 1
    assert st["items_launched"] == 2 * len(dev)                   # the all-samples search and group 0's; the rest never reaches the device
    assert st["evals_sum"] == int(r["evals"][dev].sum()) and st["outer_sum"] >= int(r["outer"][dev].sum()) and st["parts_max"] == 6
    only = a.compare_groups_genes([b, c], groups, None, [0], tol=1e-12, **CAPS)
    more = a.compare_groups_genes([b, c], groups, None, [0, 4, 2, 3, 7], tol=1e-12, **CAPS)
    assert only["stats"].items_launched == more["stats"].items_launched == 2 and not same_bits({k: v[:1] for k, v in more.items() if k != "stats"}, only)
    # the caps: two outer points are not enough where the samples differ
    capped = a.compare_groups_genes([b, c], groups, max_outer=2, tol=1e-12, **CAPS)
    moved = np.flatnonzero((r["status"] == TESTED) & (r["outer"] > 2))
    assert len(moved) >= 3 and np.all(capped["status"][moved] == UNCONVERGED) and np.all(capped["outer"][moved] == 2)
    assert capped["gene_hat"].tobytes() == r["gene_hat"].tobytes()
    # not resident
    nr = a.compare_groups_genes([b, c], groups, set_mode=1, **CAPS)
    assert np.all(nr["status"] == NOT_RESIDENT) and nr["stats"].items_launched == 0 and np.all(nr["evals"] == 0) and np.all(nr["parts"] == 0)
    for k in H.GROUPS_GENE_OUTPUTS:
        assert np.all(np.isnan(nr[k])), k


def test_streamed_member(devs):
    """everything_problem: a gene with a member in the streamed set is NOT_RESIDENT, its neighbours in the query are not touched by it"""
    a, b, c = devs[:3]
    prob = SP.everything_problem()
    n_tx, R = prob[0], prob[3]
    den = CP.den_of(prob)
    genes = (np.arange(n_tx, dtype=np.int32) // 3, (n_tx + 2) // 3)
    Rs = [R, np.where(np.arange(len(R)) % 2 == 0, R, 2 * R).astype(np.int32), np.where(np.arange(len(R)) % 3 == 0, 2 * R, R).astype(np.int32)]
    load_all((a, b, c), prob, Rs, [den] * 3, genes)
    r = a.compare_groups_genes([b, c], (0, 0, 1), max_iter=2000)
    st = r["stats"].as_dict()
    print(st)
    assert st["n_status"]["NOT_RESIDENT"] >= 1 and st["n_status"]["TESTED"] + st["n_status"]["UNCONVERGED"] >= 20
    off = np.flatnonzero(r["status"] == NOT_RESIDENT)
    assert np.all(r["evals"][off] == 0) and np.all(np.isnan(r["lambda_between"][off])) and np.all(r["parts"][off] == 0)
    on = np.flatnonzero(r["status"] != NOT_RESIDENT).astype(np.int32)
    alone = a.compare_groups_genes([b, c], (0, 0, 1), None, on, max_iter=2000)
    for k in OUTPUTS:
        assert alone[k].tobytes() == r[k][on].tobytes(), k


def test_too_large(devs):
    """65 one-transcript rows in one gene: TOO_LARGE; 64: TESTED (searched on the host: every part is closed form)"""
    a, b, c = devs[:3]
    n = 65 + 64 + 2
    rows = [[t] for t in range(n)] + [[n - 2, n - 1]]
    n_tx, rp, ci = CP.csr(rows, n)
    rng = np.random.default_rng(3)
    Rs = [rng.integers(1, 40, size=len(rows)).astype(np.int32) for _ in range(3)]
    prob = (n_tx, rp, ci, Rs[0], np.ones(len(rows)))
    g = np.full(n, -1, dtype=np.int32)
    g[:65] = 0
    g[65:129] = 1
    load_all((a, b, c), prob, Rs, [None] * 3, (g, 2))
    groups = (0, 0, 1)
    r = a.compare_groups_genes([b, c], groups, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert r["status"][0] == TOO_LARGE and r["evals"][0] == 0 and r["parts"][0] == 0 and all(math.isnan(r[k][0]) for k in H.GROUPS_GENE_OUTPUTS)
    assert r["status"][1] == TESTED and r["parts"][1] == 192 and r["stats"].items_launched == 0 and r["stats"].n_status[TOO_LARGE] == 1
    den = CP.den_of(prob)
    want = CGG.closed_gene_groups([[(float(R[t]), den[t]) for t in range(65, 129)] for R in Rs], groups)
    assert abs(r["lambda_between"][1] - want["lam_between"]) <= 7 * DEV_TOL + 1e-9 and abs(r["lambda_within"][1] - want["lam_within"]) <= 3 * DEV_TOL + 1e-9
    # 63 closed-form parts and one set part per sample: the most a launched item may hold
    g2 = np.full(n, -1, dtype=np.int32)
    g2[list(range(1, 64)) + [n - 1]] = 0
    a.set_gene_map(g2, 1)
    r = a.compare_groups_genes([b, c], groups, **CAPS)
    assert r["status"][0] == TESTED and r["parts"][0] == 192 and r["stats"].items_launched == 2 and r["stats"].parts_max == 192


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(devs):
    a, b, c = devs[:3]
    prob, Rs, dens = CGP.small_samples()
    load_all((a, b, c), prob, Rs, dens, SMALL_GENES)
    ok = dict(groups=(0, 0, 1))
    full = a.compare_groups_genes([b, c], **ok, **CAPS)
    for bad in (dict(groups=(0, 0, 2)), dict(groups=(0, -1, 1)), dict(groups=(1, 1, 1)), dict(groups=(0, 1, 3)), dict(ok, sizes=(1.0, 0.0, 1.0)),
                dict(ok, sizes=(1.0, -2.0, 1.0)), dict(ok, sizes=(1.0, math.inf, 1.0)), dict(ok, sizes=(1.0, math.nan, 1.0)),
                dict(ok, genes=[0, len(SMALL_GENES)]), dict(ok, genes=[-1]), dict(ok, dev_tol=math.inf), dict(ok, dev_tol=math.nan), dict(ok, set_mode=2),
                dict(ok, count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups_genes([b, c], **bad, **CAPS)
        assert e.value.status == -1, bad
    for others, groups in (([b, a], (0, 0, 1)), ([b, b], (0, 0, 1)), ([b, None], (0, 0, 1)), ([], (0,))):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups_genes(others, groups, **CAPS)
        assert e.value.status == -1, (others, groups)
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_groups_genes([b] * 32, [0] * 33, **CAPS)        # K = 33 (and contexts given twice)
    assert e.value.status == -1
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        b.compare_groups_genes([a, c], (0, 0, 1), **CAPS)         # no map on the first context
    assert e.value.status == -5
    c.set_gene_map(GP.gene_map(prob[0], [[0, 1], [4, 10], [8, 9]] + [[2]] * 4), len(SMALL_GENES))
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_groups_genes([b, c], **ok, **CAPS)              # another map on a later context
    assert e.value.status == -1
    c.set_gene_map(GP.gene_map(prob[0], SMALL_GENES), len(SMALL_GENES) + 1)
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_groups_genes([b, c], **ok, **CAPS)              # the same entries under another n_genes
    assert e.value.status == -1
    c.set_gene_map(GP.gene_map(prob[0], SMALL_GENES), len(SMALL_GENES))
    assert not same_bits(a.compare_groups_genes([b, c], **ok, **CAPS), full)
    with emsar_amd.EmsarHip(0) as d:
        d.upload_structure(prob[0], prob[1], prob[2])
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups_genes([b, d], (0, 0, 1), **CAPS)
        assert e.value.status == -5                               # before upload_sample
        n_tx, rp, ci = CP.csr([[0, 1], [1, 2]], prob[0])
        d.upload_structure(n_tx, rp, ci)
        d.upload_sample()
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_groups_genes([b, d], (0, 0, 1), **CAPS)
        assert e.value.status == -1                               # another structure


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_ggroups_file(tmp_path):
    """-M --compare-groups 0,0,1 --g2t on the syn300_se fixture, every second and every third read of it: exactly the files of the run
    with --g2t alone plus out.groups and out.ggroups; out.groups has the bytes of a run without --g2t, every other file keeps its bytes;
    out.ggroups has one line per gene in the order of .gfpkm and its columns are the Python call's as printed"""
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
    rsh = HL.HostRsh(rsh_path)
    g2t = tmp_path / "genes.g2t"
    g2t.write_text("".join("gene%04d\t%s\n" % (t // 3, name) for t, name in enumerate(rsh.names)))
    n_genes = (rsh.n_tx + 2) // 3
    groups, sizes = (0, 0, 1), (1.0, 0.5, 0.4)
    base = [_build.CLI, "-q", "-i", "20000"] + fx.meta["opts"] + ["-M", "--gpus", "1"]
    tail = ["-I", rsh_path]
    switch = ["--compare-groups", "0,0,1", "--compare-sizes", "1,0.5,0.4"]
    subprocess.run(base + ["--g2t", str(g2t)] + tail + [str(tmp_path / "p"), "out", str(lst)], check=True, timeout=300)
    subprocess.run(base + switch + tail + [str(tmp_path / "n"), "out", str(lst)], check=True, timeout=300)
    subprocess.run(base + switch + ["--g2t", str(g2t)] + tail + [str(tmp_path / "o"), "out", str(lst)], check=True, timeout=300)
    plain, both = sorted(os.listdir(tmp_path / "p")), sorted(os.listdir(tmp_path / "o"))
    assert both == sorted(plain + ["out.groups", "out.ggroups"]) and len(plain) >= 9
    for name in plain:
        assert (tmp_path / "o" / name).read_bytes() == (tmp_path / "p" / name).read_bytes(), name
    assert (tmp_path / "o" / "out.groups").read_bytes() == (tmp_path / "n" / "out.groups").read_bytes()
    assert not (tmp_path / "n" / "out.ggroups").exists()
    text = (tmp_path / "o" / "out.ggroups").read_text().splitlines()
    assert text[0] == "# samples=3 groups=0,0,1 sizes=1,0.5,0.4 df_between=1 df_within=1" == (tmp_path / "o" / "out.groups").read_text().splitlines()[0]
    assert text[1].split("\t") == ["gene", "gFPKM_common", "gFPKM_g0", "gFPKM_g1", "Lambda_between", "df", "p_between", "Lambda_within", "df", "p_within",
                                   "status", "outer", "evals", "parts"]
    got = [l.split("\t") for l in text[2:]]
    gfpkm = [l.split("\t")[0] for l in (tmp_path / "o" / "out.0.gfpkm").read_text().splitlines()]
    assert len(got) == n_genes and all(len(r) == 14 for r in got) and [r[0] for r in got] == gfpkm[-n_genes:]
    # what the CLI does for the three samples, through the Python bindings
    order = {name: k for k, name in enumerate(r[0] for r in got)}
    gene_of = np.array([order["gene%04d" % (t // 3)] for t in range(rsh.n_tx)], dtype=np.int32)
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
        d0.set_gene_map(gene_of, n_genes)
        p = d0.compare_groups_genes([d1, d2], groups, sizes, **cli)
    print(p["stats"].as_dict())
    assert [r[10] for r in got] == [H.GROUPS_GENE_STATUS[k] for k in p["status"]]
    assert [int(r[11]) for r in got] == list(p["outer"]) and [int(r[12]) for r in got] == list(p["evals"]) and [int(r[13]) for r in got] == list(p["parts"])
    assert all(r[5] == "1" and r[8] == "1" for r in got)
    show = lambda x, fmt: "nan" if math.isnan(x) else ("-inf" if x < 0 else "inf") if math.isinf(x) else fmt % x
    for col, key, fmt_ in ((1, "gene_common", "%f"), (4, "lambda_between", "%f"), (6, "p_between", "%.6g"), (7, "lambda_within", "%f"), (9, "p_within", "%.6g")):
        assert [r[col] for r in got] == [show(x, fmt_) for x in p[key]], key
    for g in (0, 1):
        assert [r[2 + g] for r in got] == [show(x, "%f") for x in p["gene_group"][:, g]], g
    assert np.sum(p["status"] == TESTED) >= 10
