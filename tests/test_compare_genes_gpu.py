"""GPU: the gene-level two-sample likelihood-ratio test (emsar_hip_compare_genes, include/emsar_hip.h "gene-level two-sample test")
against the independent numpy reference of tests/compare_gene_problems.py (a bracketed dual search over plain EMs with a primal feasible
point: its own error is the width w_ref), inside one set, over several parts, across size classes and samples, for one-member genes
against the transcript test, on identical samples, with a size factor, for bit-identity under everything a result must not depend on,
on awkward row forms, on the paths that are not searched, and through the CLI.

The tolerance against the reference is dev_tol + 4 P e_F + w_ref: the reported dual value lies within dev_tol of the device's own
statistic, and each of the P parts of both samples enters Lambda with two F values (at lambda = 0 and at the last multiplier) and a
factor 2 each.  e_F = 4 x 9.4e-10 is test_compare_gpu.py's figure, measured on the existing set solver on these class problems, not on
the code under test.

Every call passes max_iter <= 20000 and at most the default 40 evaluations, and den is computed on the host (CP.den_of)."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import awkward_problems as AP
from tests import compare_gene_problems as GP
from tests import compare_problems as CP
from tests import set_problems as SP

pytestmark = pytest.mark.gpu

TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE = range(6)
DEV_TOL = 1e-4
E_F = 4 * 9.4e-10
W_REF_MAX = 1e-7
CUT95 = 3.841458820694124
CAPS = dict(max_iter=20000)
OUTPUTS = H.COMPARE_GENE_OUTPUTS + ("status", "evals", "parts")


def tol_of(ref):
    return DEV_TOL + 4 * ref["parts"] * E_F + ref["w_ref"]


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b:
        yield a, b


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


def classes_of(prob, R):
    n_tx, rp, ci, _, E = prob
    return H.sets_selfcheck(n_tx, rp, ci, np.where(E > 0, R, 0))["sets_resident"]


def check_against(r, i, ref, what):
    tol = tol_of(ref)
    print(what, "Lambda", r["lambda"][i], "ref", ref["lam"], "residual", r["lambda"][i] - ref["lam"], "tol", tol, "w_ref", ref["w_ref"], "evals", r["evals"][i],
          "parts", r["parts"][i], "gap", r["gap"][i], "mult", r["multiplier"][i], "ref mult", ref["multiplier"])
    assert ref["w_ref"] <= W_REF_MAX, (what, ref["w_ref"])
    assert r["status"][i] == TESTED and r["parts"][i] == ref["parts"], (what, r["status"][i], r["parts"][i], ref["parts"])
    assert abs(r["lambda"][i] - ref["lam"]) <= tol, (what, r["lambda"][i], ref["lam"], tol)
    for k in ("gene_a", "gene_b"):
        assert abs(r[k][i] - ref[k]) <= 1e-6 * ref[k], (what, k, r[k][i], ref[k])
    assert r["pvalue"][i] == H.compare_pvalue_host(r["lambda"][i])


# ---- 1. two or three members inside one set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [64, 256, 512])
def test_members_inside_one_set(devs, threads):
    a, b = devs
    prob, RA, RB, _ = CP.class_problem(threads)
    genes = GP.class_genes(threads)
    den = CP.den_of(prob)
    load(a, prob, RA, den, genes)
    load(b, prob, RB, den)
    r = a.compare_genes(b, tol=1e-12, **CAPS)
    for k, members in enumerate(genes):
        ref, _ = GP.tested_reference("class%d-%d" % (threads, k) if threads == 64 else "class%d" % threads)
        check_against(r, k, ref, (threads, members))
        assert abs(r["gene_null"][k] - ref["gene_null"]) <= 1e-3 * ref["gene_null"]
        assert abs(r["log2fc"][k] - math.log2(ref["gene_a"] / ref["gene_b"])) <= 1e-5
    st = r["stats"].as_dict()
    print(st)
    assert st["items_launched"] == len(genes) and st["evals_sum"] == int(r["evals"].sum()) and st["n_status"]["TESTED"] == len(genes)
    assert st["parts_max"] == 2


# ---- 2. the loop over parts, closed-form parts, the host path, the statuses decided on the host ----------------------------------------
# two maps: the genes {0, 3, 6} / {0, 1} and {10} / {4, 10} share a transcript
SMALL_X = [[0, 3, 6], [8, 9], [10], [1], [2], [5], [7]]
SMALL_Y = [[0, 1], [4, 10], [8, 9]]


def small(devs, genes, **kw):
    a, b = devs
    prob, RA, RB, den_a, den_b = CP.small_problem()
    load(a, prob, RA, den_a, genes)
    load(b, prob, RB, den_b)
    return prob, RA, RB, den_a, den_b, a.compare_genes(b, tol=1e-12, **CAPS, **kw)


def test_parts_loop_and_host_paths(devs):
    a, b = devs
    prob, RA, RB, den_a, den_b, r = small(devs, SMALL_X)
    print({k: r[k] for k in OUTPUTS})
    # one closed-form part and two set parts in A; in B transcript 6 is on the boundary (no read of its own, none shared)
    ref, _ = GP.tested_reference("small-0-3-6")
    check_against(r, 0, ref, "small {0, 3, 6}")
    assert r["parts"][0] == 6
    assert r["status"][1] == BOTH_ABSENT and r["lambda"][1] == 0.0 and r["pvalue"][1] == 1.0 and r["evals"][1] == 1 and math.isnan(r["log2fc"][1])
    assert r["status"][2] == OUTSIDE and r["evals"][2] == 0 and r["parts"][2] == 0
    for k in H.COMPARE_GENE_OUTPUTS:
        assert math.isnan(r[k][2]), k
    st = r["stats"].as_dict()
    assert sum(st["n_status"].values()) == len(SMALL_X) and st["n_status"]["OUTSIDE"] == 1 and st["n_status"]["BOTH_ABSENT"] == 1
    assert st["parts_max"] == 6 and st["items_launched"] == 4      # {0, 3, 6}, {2}, {5}, {7}; {1} and {8, 9} are the host's
    prob, RA, RB, den_a, den_b, r = small(devs, SMALL_Y)
    print({k: r[k] for k in OUTPUTS})
    # all closed form: the host's search, the bits of the diagnostic entry, nothing launched for it
    want = H.debug_compare_genes_closed(RA[[0, 1]].astype(float), den_a[[0, 1]], RB[[0, 1]].astype(float), den_b[[0, 1]])
    for k in H.COMPARE_GENE_OUTPUTS + ("status", "evals"):
        assert np.array([r[k][0]]).tobytes() == np.array([want[k]], dtype=r[k].dtype).tobytes(), (k, r[k][0], want[k])
    assert r["parts"][0] == 4 and r["status"][0] == TESTED and r["evals"][0] > 1
    without = a.compare_genes(b, [1, 2], tol=1e-12, **CAPS)
    assert without["stats"].items_launched == r["stats"].items_launched == 1         # {4, 10} alone reaches the device
    assert not [k for k in OUTPUTS if without[k].tobytes() != r[k][1:].tobytes()]
    # 10 has den = 0 in B: held at 0 there, and still a member in A
    ref, _ = GP.tested_reference("small-4-10")
    check_against(r, 1, ref, "small {4, 10}")
    theta_a = a.solve(tol=1e-12, **CAPS)[0]
    assert abs(r["gene_a"][1] - (theta_a[4] + theta_a[10])) <= 1e-9 * r["gene_a"][1] and theta_a[10] > 0
    assert r["status"][2] == BOTH_ABSENT


# ---- 3. mixed classes in one gene and across the samples -------------------------------------------------------------------------------
def test_mixed_classes_in_one_gene(devs):
    a, b = devs
    prob, RA, RB, gene = GP.mixed_problem()
    assert classes_of(prob, RA) == [1, 1, 0] and classes_of(prob, RB) == [1, 1, 0]
    den = CP.den_of(prob)
    load(a, prob, RA, den, [gene])
    load(b, prob, RB, den)
    r = a.compare_genes(b, tol=1e-12, **CAPS)
    ref, _ = GP.tested_reference("mixed")
    check_against(r, 0, ref, ("mixed", gene))
    assert r["parts"][0] == 4 and r["stats"].items_launched == 1


def test_different_classes_across_samples(devs):
    """split_problem: the gene's two transcripts lie in one 64-class chain in A and in the 512-class set in B; H0 at ratio 1 is symmetric,
    so (B, A) has the same reference"""
    a, b = devs
    prob, RA, RB, tids = CP.split_problem()
    assert classes_of(prob, RA) == [1, 0, 0] and classes_of(prob, RB) == [0, 0, 1]
    den = CP.den_of(prob)
    load(a, prob, RA, den, [tids])
    load(b, prob, RB, den, [tids])
    ref, _ = GP.tested_reference("split")
    r = a.compare_genes(b, tol=1e-12, **CAPS)
    s = b.compare_genes(a, tol=1e-12, **CAPS)
    check_against(r, 0, ref, "split A, B")
    check_against(s, 0, dict(ref, gene_a=ref["gene_b"], gene_b=ref["gene_a"]), "split B, A")
    assert r["gene_a"].tobytes() == s["gene_b"].tobytes() and r["gene_b"].tobytes() == s["gene_a"].tobytes()
    assert r["stats"].items_launched == 1 and r["parts"][0] == 2


# ---- 4. 7. 8. one-member genes, gene sums, bit-for-bit invariance --------------------------------------------------------------------
def invariance_problem():
    from tests.test_compare_gpu import invariance_problem as ip
    return ip()


def test_one_member_genes_are_the_transcript_test(devs):
    a, b = devs
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    kw = dict(max_iter=3000)
    ident = (np.arange(prob[0], dtype=np.int32), prob[0])
    load(a, prob, RA, den, ident, H.LAYOUT_CSR)
    load(b, prob, RB, den, None, H.LAYOUT_CSR)
    g, t = a.compare_genes(b, **kw), a.compare(b, **kw)
    ok = np.isin(t["status"], (TESTED, UNCONVERGED))
    print("tested", ok.sum(), "max |dLambda|", np.abs(g["lambda"][ok] - t["lambda"][ok]).max())
    assert np.array_equal(g["status"], t["status"]) and ok.sum() >= 30
    assert np.all(np.abs(g["lambda"][ok] - t["lambda"][ok]) <= 2 * DEV_TOL)
    assert g["gene_a"].tobytes() == t["theta_a"].tobytes() and g["gene_b"].tobytes() == t["theta_b"].tobytes()


def drawn_genes(n_tx, seed=9):
    """genes of 1 .. 4 members drawn over all transcripts: many span two sets"""
    rng = np.random.default_rng(seed)
    order, genes, at = rng.permutation(n_tx), [], 0
    while at < n_tx:
        k = int(rng.integers(1, 5))
        genes.append([int(x) for x in order[at:at + k]])
        at += k
    return genes


def test_gene_sum_at_lambda_zero(devs):
    a, b = devs
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    load(a, prob, RA, den, genes)
    load(b, prob, RB, den, genes)
    r = a.compare_genes(b, tol=1e-12, **CAPS)
    ga, gb = a.gene_sums(a.solve(tol=1e-12, **CAPS)[0]), b.gene_sums(b.solve(tol=1e-12, **CAPS)[0])
    given = np.isin(r["status"], (TESTED, UNCONVERGED, BOTH_ABSENT))
    assert given.sum() >= 20                                  # of the 29 genes drawn
    assert np.all(np.abs(r["gene_a"][given] - ga[given]) <= 1e-12 * ga[given]) and np.all(np.abs(r["gene_b"][given] - gb[given]) <= 1e-12 * gb[given])


def config(monkeypatch, dev, prob, R, den, genes, layout, merge, mode):
    if mode is None:
        monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
    else:
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", mode)
    load(dev, prob, R, den, genes, layout, merge)
    if mode is not None:
        assert dev.info()["renumbered"] == int(mode == "2")


def test_invariance_bit_for_bit(devs, monkeypatch):
    a, b = devs
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    ng = len(genes)
    kw = dict(max_iter=3000)
    tids = np.arange(0, prob[0], 7, dtype=np.int32)
    config(monkeypatch, a, prob, RA, den, genes, H.LAYOUT_CSR, False, None)
    config(monkeypatch, b, prob, RB, den, genes, H.LAYOUT_CSR, False, None)
    before = [a.solve(**kw)[0], b.solve(**kw)[0], a.compare(b, tids, **kw)]
    whole = a.compare_genes(b, **kw)
    after = [a.solve(**kw)[0], b.solve(**kw)[0], a.compare(b, tids, **kw)]
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert not [k for k in H.COMPARE_OUTPUTS + ("status", "evals") if before[2][k].tobytes() != after[2][k].tobytes()]
    st = whole["stats"].as_dict()
    print(st)
    assert st["n_status"]["TESTED"] >= 20 and st["n_status"]["TESTED"] + st["n_status"]["UNCONVERGED"] == ng and st["evals_max"] <= 40
    assert st["parts_max"] >= 4 and np.sum(whole["parts"] > 2) >= 5              # genes that span sets
    q = np.random.default_rng(5).permutation(ng).astype(np.int32)
    shuffled = a.compare_genes(b, q, **kw)
    twice = a.compare_genes(b, np.concatenate([q[:10], q[:10], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_COMPARE_GENES_BATCH", "1")     # one item per class and launch
    single = a.compare_genes(b, **kw)
    monkeypatch.delenv("EMSAR_HIP_COMPARE_GENES_BATCH")
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][20:].tobytes() == shuffled[k].tobytes() and twice[k][:10].tobytes() == twice[k][10:20].tobytes() == shuffled[k][:10].tobytes(), k
        assert single[k].tobytes() == whole[k].tobytes(), k
    assert sum(twice["stats"].as_dict()["n_status"].values()) == ng
    # without a map on ctx_b: ctx_a's map is used for both
    load(b, prob, RB, den, None, H.LAYOUT_CSR)
    assert not same_bits(a.compare_genes(b, **kw), whole)
    for layout, merge, mode in ((H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"), (H.LAYOUT_TILED, True, "2")):
        config(monkeypatch, a, prob, RA, den, genes, layout, merge, mode)
        config(monkeypatch, b, prob, RB, den, genes, layout, merge, mode)
        assert not same_bits(a.compare_genes(b, **kw), whole), (layout, merge, mode)
    # the two contexts in different configurations: a TILED, merged, library numbering; b CSR, then TILED in the caller's numbering without a map
    config(monkeypatch, b, prob, RB, den, genes, H.LAYOUT_CSR, False, None)
    assert not same_bits(a.compare_genes(b, **kw), whole)
    config(monkeypatch, b, prob, RB, den, None, H.LAYOUT_TILED, False, "0")
    assert not same_bits(a.compare_genes(b, **kw), whole)
    config(monkeypatch, a, prob, RA, den, genes, H.LAYOUT_CSR, False, None)
    config(monkeypatch, b, prob, RB, den, None, H.LAYOUT_TILED, True, "2")
    assert not same_bits(a.compare_genes(b, **kw), whole)


# ---- 5. 6. identical samples, a size factor ------------------------------------------------------------------------------------------
def family_genes():
    """the sets of all_resident_problem's small shapes as genes: consecutive caller tids in threes"""
    prob = SP.all_resident_problem()
    return prob, (np.arange(prob[0], dtype=np.int32) // 3, (prob[0] + 2) // 3)


def test_identical_samples(devs):
    a, b = devs
    prob, genes = family_genes()
    den = CP.den_of(prob)
    load(a, prob, prob[3], den, genes)
    load(b, prob, prob[3], den, genes)
    r = a.compare_genes(b, max_iter=4000)
    given = ~np.isin(r["status"], (OUTSIDE, NOT_RESIDENT, TOO_LARGE))
    print(r["stats"].as_dict())
    assert given.sum() > 0.9 * genes[1]
    assert np.all(r["lambda"][given] == 0.0) and np.all(r["evals"][given] == 1) and np.all(r["gap"][given] == 0.0) and np.all(r["pvalue"][given] == 1.0)
    assert r["gene_a"][given].tobytes() == r["gene_b"][given].tobytes()


def test_size_factor(devs):
    a, b = devs
    prob, RA, _, _ = CP.class_problem(64)
    den = CP.den_of(prob)
    genes = (np.arange(prob[0], dtype=np.int32) // 3, (prob[0] + 2) // 3)
    load(a, prob, RA, den, genes)
    load(b, prob, 2 * RA, den, genes)
    half = a.compare_genes(b, ratio=0.5, tol=1e-12, **CAPS)
    tol = DEV_TOL + 4 * int(half["parts"].max()) * E_F
    print("ratio 1/2: max Lambda", half["lambda"].max(), "evals max", half["evals"].max(), "tol", tol)
    assert np.all(np.isin(half["status"], (TESTED, BOTH_ABSENT))) and np.all(half["lambda"] <= tol)
    one = a.compare_genes(b, ratio=1.0, tol=1e-12, **CAPS)
    reads = a.gene_sums(a.solve(tol=1e-12, **CAPS)[0] * den)
    big = np.flatnonzero(reads >= 50)
    print("ratio 1: genes with >= 50 reads", len(big), "min Lambda among them", one["lambda"][big].min())
    assert len(big) >= 5 and np.all(one["lambda"][big] > CUT95) and np.all(one["status"][big] == TESTED)
    assert np.all(np.abs(one["log2fc"][big] + 1.0) <= 1e-6)


# ---- 9. row forms ----------------------------------------------------------------------------------------------------------------------
def test_row_forms(devs):
    """a gene of a transcript that occurs twice in a row, the den = 0 transcript and the one alone in its row"""
    a, b = devs
    prob, notes = AP.awkward_members()
    RA, RB = AP.awkward_samples()
    den = CP.den_of(prob)
    gene = GP.awkward_gene()
    assert den[notes["outside"]] == 0.0
    load(a, prob, RA, den, [gene, [int(notes["outside"])]])
    load(b, prob, RB, den)
    r = a.compare_genes(b, tol=1e-12, **CAPS)
    ref, _ = GP.tested_reference("awkward")
    check_against(r, 0, ref, ("awkward", gene))
    assert r["parts"][0] == 4 and r["status"][1] == OUTSIDE


# ---- 10. statuses and errors -----------------------------------------------------------------------------------------------------------
def test_statuses_and_errors(devs):
    a, b = devs
    prob, RA, RB, den_a, den_b, r1 = small(devs, SMALL_X, set_mode=1)
    assert np.all(r1["status"] == NOT_RESIDENT) and r1["stats"].items_launched == 0 and np.all(r1["evals"] == 0)
    for k in H.COMPARE_GENE_OUTPUTS:
        assert np.all(np.isnan(r1[k])), k
    full = a.compare_genes(b, **CAPS)
    capped = a.compare_genes(b, max_evals=1, **CAPS)
    moved = np.flatnonzero((full["status"] == TESTED) & (full["evals"] > 1))
    assert len(moved) >= 3
    assert np.all(capped["status"][moved] == UNCONVERGED) and np.all(capped["evals"][moved] == 1) and np.all(capped["lambda"][moved] == 0.0)
    assert capped["gene_a"][moved].tobytes() == full["gene_a"][moved].tobytes() and capped["gene_b"][moved].tobytes() == full["gene_b"][moved].tobytes()
    for bad in (dict(query=[0, len(SMALL_X)]), dict(query=[-1]), dict(ratio=-1.0), dict(ratio=math.nan), dict(ratio=math.inf), dict(dev_tol=math.inf),
                dict(set_mode=2), dict(count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_genes(b, **bad, **CAPS)
        assert e.value.status == -1, bad
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_genes(a, **CAPS)
    assert e.value.status == -1
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        b.compare_genes(a, **CAPS)                            # no map on the context that holds sample A
    assert e.value.status == -5
    b.set_gene_map(GP.gene_map(prob[0], SMALL_Y + [[1]] * 4), len(SMALL_X))
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_genes(b, **CAPS)                            # another map on ctx_b
    assert e.value.status == -1
    b.set_gene_map(GP.gene_map(prob[0], SMALL_X), len(SMALL_X) + 1)
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_genes(b, **CAPS)                            # the same entries under another n_genes
    assert e.value.status == -1
    b.set_gene_map(GP.gene_map(prob[0], SMALL_X), len(SMALL_X))
    assert not same_bits(a.compare_genes(b, **CAPS), full)
    with emsar_amd.EmsarHip(0) as d:
        n_tx, rp, ci = CP.csr([[0, 1], [1, 2]], prob[0])
        d.upload_structure(n_tx, rp, ci)
        d.upload_sample()
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_genes(d, **CAPS)
        assert e.value.status == -1                           # another structure
    assert not same_bits(a.compare_genes(b, ratio=0.0, **CAPS), full)          # a ratio of 0 is the default 1


def test_streamed_member(devs):
    """everything_problem: a gene with a member in the streamed set is NOT_RESIDENT, its neighbours in the query are not touched by it"""
    a, b = devs
    prob = SP.everything_problem()
    n_tx, R = prob[0], prob[3]
    den = CP.den_of(prob)
    n_genes = (n_tx + 2) // 3
    genes = (np.arange(n_tx, dtype=np.int32) // 3, n_genes)
    load(a, prob, R, den, genes)
    load(b, prob, np.where(np.arange(len(R)) % 2 == 0, R, 2 * R).astype(np.int32), den, genes)
    r = a.compare_genes(b, max_iter=2000)
    st = r["stats"].as_dict()
    print(st)
    assert st["n_status"]["NOT_RESIDENT"] >= 1 and st["n_status"]["TESTED"] + st["n_status"]["UNCONVERGED"] >= 20
    off = np.flatnonzero(r["status"] == NOT_RESIDENT)
    assert np.all(r["evals"][off] == 0) and np.all(np.isnan(r["lambda"][off]))
    on = np.flatnonzero(r["status"] != NOT_RESIDENT).astype(np.int32)
    alone = a.compare_genes(b, on, max_iter=2000)
    for k in OUTPUTS:
        assert alone[k].tobytes() == r[k][on].tobytes(), k


def test_too_large(devs):
    """65 one-transcript rows in one gene: TOO_LARGE; 64: TESTED (searched on the host: every part is closed form)"""
    a, b = devs
    n = 65 + 64 + 2
    rows = [[t] for t in range(n)] + [[n - 2, n - 1]]
    n_tx, rp, ci = CP.csr(rows, n)
    rng = np.random.default_rng(3)
    RA, RB = rng.integers(1, 40, size=len(rows)).astype(np.int32), rng.integers(1, 40, size=len(rows)).astype(np.int32)
    prob = (n_tx, rp, ci, RA, np.ones(len(rows)))
    g = np.full(n, -1, dtype=np.int32)
    g[:65] = 0
    g[65:129] = 1
    load(a, prob, RA, None, (g, 2))
    load(b, prob, RB, None)
    r = a.compare_genes(b, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    assert r["status"][0] == TOO_LARGE and r["evals"][0] == 0 and r["parts"][0] == 0 and all(math.isnan(r[k][0]) for k in H.COMPARE_GENE_OUTPUTS)
    assert r["status"][1] == TESTED and r["parts"][1] == 128 and r["stats"].items_launched == 0
    den = CP.den_of(prob)
    want, _ = GP.closed_gene_lambda(RA[65:129].astype(float), den[65:129], RB[65:129].astype(float), den[65:129])
    assert abs(r["lambda"][1] - want) <= DEV_TOL
    # 63 closed-form parts and one set part per sample: the most a launched item may hold
    g2 = np.full(n, -1, dtype=np.int32)
    g2[list(range(1, 64)) + [n - 1]] = 0
    a.set_gene_map(g2, 1)
    r = a.compare_genes(b, **CAPS)
    assert r["status"][0] == TESTED and r["parts"][0] == 128 and r["stats"].items_launched == 1 and r["stats"].parts_max == 128


# ---- 11. the command line --------------------------------------------------------------------------------------------------------------
def test_cli_gcompare_file(tmp_path):
    """-M --compare --g2t on the syn300_se fixture and on every second read of it: out.1.gcompare has one line per gene in the order of
    .gfpkm and its columns are the Python call's as printed; out.1.compare keeps its bytes; sample 0 writes no .gcompare"""
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
    rsh = HL.HostRsh(rsh_path)
    g2t = tmp_path / "genes.g2t"
    g2t.write_text("".join("gene%04d\t%s\n" % (t // 3, name) for t, name in enumerate(rsh.names)))
    n_genes = (rsh.n_tx + 2) // 3
    base = [_build.CLI, "-q", "-i", "20000"] + fx.meta["opts"]
    subprocess.run(base + ["-M", "--gpus", "1", "--compare", "-I", rsh_path, str(tmp_path / "p"), "out", str(lst)], check=True, timeout=300)
    subprocess.run(base + ["-M", "--gpus", "1", "--compare", "--g2t", str(g2t), "-I", rsh_path, str(tmp_path / "o"), "out", str(lst)], check=True, timeout=300)
    assert (tmp_path / "o" / "out.1.compare").read_bytes() == (tmp_path / "p" / "out.1.compare").read_bytes()
    assert not (tmp_path / "o" / "out.0.gcompare").exists() and not (tmp_path / "p" / "out.1.gcompare").exists()
    got = [l.split("\t") for l in (tmp_path / "o" / "out.1.gcompare").read_text().splitlines()]
    assert got[0] == ["gene", "gFPKM", "gFPKM_ref", "log2FC", "Lambda", "p", "status", "evals", "parts"]
    got = got[1:]
    gfpkm = [l.split("\t")[0] for l in (tmp_path / "o" / "out.1.gfpkm").read_text().splitlines()]
    assert len(got) == n_genes and all(len(r) == 9 for r in got)
    assert [r[0] for r in got] == gfpkm[-n_genes:]
    # what the CLI does for the two samples, through the Python bindings
    order = {name: k for k, name in enumerate(r[0] for r in got)}
    gene_of = np.array([order["gene%04d" % (t // 3)] for t in range(rsh.n_tx)], dtype=np.int32)
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
            d.set_gene_map(gene_of, n_genes)
        p = d1.compare_genes(d0, **cli)
    assert [r[6] for r in got] == [H.COMPARE_GENE_STATUS[k] for k in p["status"]]
    assert [int(r[7]) for r in got] == list(p["evals"]) and [int(r[8]) for r in got] == list(p["parts"])
    for col, key in ((1, "gene_a"), (2, "gene_b"), (3, "log2fc"), (4, "lambda")):
        v = np.array([float(r[col]) for r in got])
        fin = np.isfinite(p[key])
        assert np.array_equal(np.isnan(v), np.isnan(p[key])) and np.array_equal(v[~fin & ~np.isnan(v)], p[key][~fin & ~np.isnan(p[key])]), key
        assert np.all(np.abs(v[fin] - p[key][fin]) <= 1e-6 + 1e-15 * np.abs(p[key][fin])), key          # "%lf"
    assert [r[4] for r in got] == ["nan" if math.isnan(x) else "inf" if math.isinf(x) else "%f" % x for x in p["lambda"]]
    print(p["stats"].as_dict())
    assert np.sum(p["status"] == TESTED) >= 10
