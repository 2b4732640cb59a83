"""GPU: the two-sample test of isoform usage (emsar_hip_compare_usage, include/emsar_hip.h "two-sample test of isoform usage") against
the independent numpy reference of tests/compare_usage_problems.py (a 201-point grid with refinement over bracketed dual searches over
plain EMs, recorded in tests/golden/compare_usage_refs.json; its own error is the width w_ref), inside one set of each size class, over
several parts, across classes and samples, against isoform_usage at lambda = 0, for bit-identity under everything a result must not
depend on, on awkward row forms, on the paths that are not searched, and through the CLI.

The tolerance against the reference is 3 dev_tol + 4 P e_F + w_ref: each of the two inner searches and the outer search is granted
dev_tol (their stopping rules bound it), each of the P parts of both samples enters Lambda with two F values (at lambda = 0 and at the
reported outer point) and a factor 2 each.  e_F = 4 x 9.4e-10 is test_compare_gpu.py's figure, measured on the existing set solver on
these class problems, not on the code under test.

Every call passes max_iter <= 20000 and the default caps of the two searches, and den is computed on the host (CP.den_of)."""
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
from tests import compare_usage_problems as UP
from tests.test_compare_genes_gpu import classes_of, config, drawn_genes, invariance_problem, load

pytestmark = pytest.mark.gpu

TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE, UNDEFINED, SINGLE = range(8)
DEV_TOL = 1e-4
E_F = 4 * 9.4e-10
W_REF_MAX = 1e-7
CAPS = dict(max_iter=20000)
OUTPUTS = H.USAGE_OUTPUTS + H.USAGE_COUNTS
STATS = ("n_status", "items_launched", "evals_sum", "passes_sum", "outer_sum", "evals_max", "passes_max", "parts_max", "outer_max", "min_raw_lambda")


def tol_of(ref):
    return 3 * DEV_TOL + 4 * ref["parts"] * E_F + ref["w_ref"]


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b:
        yield a, b


def same_bits(x, y, keys=OUTPUTS):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def check_against(r, i, ref, what):
    tol = tol_of(ref)
    print(what, "Lambda", r["lambda"][i], "ref", ref["lam"], "residual", r["lambda"][i] - ref["lam"], "tol", tol, "w_ref", ref["w_ref"], "outer",
          r["outer_evals"][i], "evals", r["evals"][i], "parts", r["parts"][i], "usage", r["usage_a"][i], r["usage_b"][i], "null", r["usage_null"][i],
          "ref null", ref["usage_null"], "slope", r["slope"][i])
    assert ref["w_ref"] <= W_REF_MAX and ref["peaks"] == 1, (what, ref["w_ref"], ref["peaks"])
    assert r["status"][i] == TESTED and r["parts"][i] == ref["parts"], (what, r["status"][i], r["parts"][i], ref["parts"])
    assert abs(r["lambda"][i] - ref["lam"]) <= tol, (what, r["lambda"][i], ref["lam"], tol)
    for k in ("usage_a", "usage_b"):
        assert abs(r[k][i] - ref[k]) <= 1e-6 * max(ref[k], 1e-3), (what, k, r[k][i], ref[k])
    lo, hi = min(r["usage_a"][i], r["usage_b"][i]), max(r["usage_a"][i], r["usage_b"][i])
    assert lo < r["usage_null"][i] < hi and r["slope"][i] <= DEV_TOL and 2 <= r["outer_evals"][i] <= 12
    assert r["pvalue"][i] == H.compare_pvalue_host(r["lambda"][i]) and r["raw_lambda"][i] == r["lambda"][i]
    want = math.log(r["usage_a"][i] / (1 - r["usage_a"][i])) - math.log(r["usage_b"][i] / (1 - r["usage_b"][i])) if lo > 0 and hi < 1 else None
    assert want is None or abs(r["dlogit"][i] - want) <= 1e-12 * max(1.0, abs(want))


def run_case(devs, name, genes=None, swap=False, **kw):
    """the case `name` of UP.CASES on the device -> (result, index of t in the query, reference)"""
    a, b = devs
    prob, RA, RB, den_a, den_b, members, t = UP.case(name)
    genes = [members] if genes is None else genes
    if swap:
        RA, RB, den_a, den_b = RB, RA, den_b, den_a
    load(a, prob, RA, den_a, genes)
    load(b, prob, RB, den_b)
    query = np.array([t], dtype=np.int32)
    return a.compare_usage(b, query, tol=1e-12, **CAPS, **kw), 0, UP.tested_reference(name)


# ---- 1. inside one set of each size class --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["class64-0", "class64-1", "class64-2", "class256", "class512"])
def test_inside_one_set(devs, name):
    threads = int(name[5:].partition("-")[0])
    r, i, ref = run_case(devs, name, genes=GP.class_genes(threads))
    check_against(r, i, ref, name)
    st = r["stats"].as_dict()
    print(st)
    assert st["items_launched"] == 1 and st["evals_sum"] == r["evals"][0] and st["outer_sum"] == st["outer_max"] == r["outer_evals"][0]
    assert st["n_status"]["TESTED"] == 1 and st["parts_max"] == 2 and st["evals_max"] <= 40 * 2 * 12


# ---- 2. the loop over parts, closed-form parts, a share at the boundary, the host path and the host's statuses ------------------------
SMALL = [[0, 3, 6], [8, 9], [4, 10], [1, 2], [5], [7]]


def test_parts_loop_boundary_and_host_paths(devs):
    a, b = devs
    prob, RA, RB, den_a, den_b = CP.small_problem()
    load(a, prob, RA, den_a, SMALL)
    load(b, prob, RB, den_b)
    r = a.compare_usage(b, tol=1e-12, **CAPS)
    print({k: r[k] for k in OUTPUTS})
    # {0, 3, 6}: one closed-form part and two set parts per sample; 6 has share 0 in B (no read of its own, none shared)
    check_against(r, 0, UP.tested_reference("small-0-3-6:0"), "small {0, 3, 6}: 0")          # t itself a closed-form part on the device
    check_against(r, 3, UP.tested_reference("small-0-3-6:3"), "small {0, 3, 6}: 3")
    check_against(r, 6, UP.tested_reference("small-0-3-6:6"), "small {0, 3, 6}: 6")
    assert r["usage_b"][6] == 0.0 and r["dlogit"][6] == math.inf and r["parts"][0] == r["parts"][3] == r["parts"][6] == 6
    assert r["status"][0] == TESTED and abs(r["usage_a"][[0, 3, 6]].sum() - 1.0) <= 1e-12
    # {8, 9}: no reads in either sample; {4, 10}: 10 has den = 0 in B, which leaves 4 alone there; {5}, {7}: one member
    assert r["status"][8] == r["status"][9] == UNDEFINED and r["outer_evals"][8] == 1 and math.isnan(r["lambda"][8]) and math.isnan(r["usage_a"][8])
    assert r["status"][10] == OUTSIDE and r["status"][4] == SINGLE and r["status"][5] == SINGLE and r["status"][7] == SINGLE
    for t in (10, 4, 5, 7):
        assert all(math.isnan(r[k][t]) for k in H.USAGE_OUTPUTS) and r["outer_evals"][t] == r["evals"][t] == r["parts"][t] == 0, t
    # {1, 2}: closed form in A; 2 lies in a set in B
    assert r["status"][1] == r["status"][2] == TESTED and r["parts"][1] == 4
    st = r["stats"].as_dict()
    assert sum(st["n_status"].values()) == 11 and st["n_status"]["SINGLE"] == 3 and st["n_status"]["UNDEFINED"] == 2 and st["n_status"]["OUTSIDE"] == 1
    assert st["items_launched"] == 5 and st["parts_max"] == 6            # 0, 3, 6 and 1, 2; {8, 9} is the host's
    # all parts closed form in both samples: the host's search, the bits of the diagnostic entry, nothing launched
    a.set_gene_map(GP.gene_map(prob[0], [[0, 1]]), 1)
    h = a.compare_usage(b, [1, 0, 5], tol=1e-12, **CAPS)
    assert h["stats"].items_launched == 0 and h["status"][2] == OUTSIDE          # 5 has no gene
    for i, t in enumerate((1, 0)):
        want = H.debug_compare_usage_closed(RA[[0, 1]].astype(float), den_a[[0, 1]], RB[[0, 1]].astype(float), den_b[[0, 1]], t=t)
        for k in OUTPUTS:
            assert np.array([h[k][i]]).tobytes() == np.array([want[k]], dtype=h[k].dtype).tobytes(), (t, k, h[k][i], want[k])
    assert h["status"][0] == TESTED and h["outer_evals"][0] > 1 and abs(h["lambda"][0] - h["lambda"][1]) <= 3 * DEV_TOL


# ---- 3. mixed classes in one gene and across the samples -------------------------------------------------------------------------------
def test_mixed_classes_in_one_gene(devs):
    prob, RA, RB, gene = GP.mixed_problem()
    assert classes_of(prob, RA) == [1, 1, 0] and classes_of(prob, RB) == [1, 1, 0]
    r, i, ref = run_case(devs, "mixed")
    check_against(r, i, ref, ("mixed", gene))
    assert r["parts"][0] == 4 and r["stats"].items_launched == 1


def test_different_classes_across_samples(devs):
    """split_problem: the gene's two transcripts lie in one 64-class chain in A and in the 512-class set in B, and the launch class is
    B's; the null is symmetric, so (B, A) has the same reference with the shares exchanged.  Sample A has reads on chain rows of two
    transcripts each only: the share of the tested transcript is at the boundary there (the EM of the reference leaves it at 1e-187,
    the device at exactly 0), and under the null the whole gene leaves A -- X = 0 satisfies theta_t = u X -- so the maximum lies at the
    end of the bracket, B's estimated share."""
    prob, RA, RB, tids = CP.split_problem()
    assert classes_of(prob, RA) == [1, 0, 0] and classes_of(prob, RB) == [0, 0, 1]
    ref = UP.tested_reference("split")
    r, i, _ = run_case(devs, "split")
    s, _, _ = run_case(devs, "split", swap=True)
    check_against(r, i, ref, "split A, B")
    check_against(s, i, dict(ref, usage_a=ref["usage_b"], usage_b=ref["usage_a"]), "split B, A")
    assert r["usage_a"].tobytes() == s["usage_b"].tobytes() and r["usage_b"].tobytes() == s["usage_a"].tobytes() and r["dlogit"][0] == -s["dlogit"][0]
    assert r["usage_a"][0] == 0.0 and r["stats"].items_launched == 1 and r["parts"][0] == 2


# ---- 4. row forms ----------------------------------------------------------------------------------------------------------------------
def test_row_forms(devs):
    """a gene of a transcript that occurs twice in a row, the den = 0 transcript and the one alone in its row"""
    a, b = devs
    prob, notes = AP.awkward_members()
    gene = GP.awkward_gene()
    r, i, ref = run_case(devs, "awkward", genes=[gene, [int(notes["outside"])]])
    check_against(r, i, ref, ("awkward", gene))
    o = a.compare_usage(b, [int(notes["outside"]), gene[2]], tol=1e-12, **CAPS)
    assert o["status"][0] == OUTSIDE and o["status"][1] == TESTED and abs(o["usage_a"][1] + r["usage_a"][0] - 1.0) <= 1e-12
    assert abs(o["lambda"][1] - r["lambda"][0]) <= 2 * tol_of(ref)          # two members take part: the complement's null is the same


# ---- 5. the shares at lambda = 0, bit-for-bit invariance, contexts untouched -----------------------------------------------------------
def test_usage_is_isoform_usage_of_the_solve(devs):
    a, b = devs
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    load(a, prob, RA, den, genes)
    load(b, prob, RB, den, genes)
    r = a.compare_usage(b, tol=1e-12, **CAPS)
    ua, ub = a.isoform_usage(a.solve(tol=1e-12, **CAPS)[0]), b.isoform_usage(b.solve(tol=1e-12, **CAPS)[0])
    given = np.isin(r["status"], (TESTED, UNCONVERGED, BOTH_ABSENT))
    print(r["stats"].as_dict(), "given", given.sum())
    assert given.sum() >= 30
    assert np.all(np.abs(r["usage_a"][given] - ua[given]) <= 1e-12 * ua[given]) and np.all(np.abs(r["usage_b"][given] - ub[given]) <= 1e-12 * ub[given])
    assert np.all((r["lambda"][given] >= 0.0) & np.isfinite(r["lambda"][given]))


def stats_of(r):
    d = r["stats"].as_dict()
    return {k: d[k] for k in STATS}


def test_invariance_bit_for_bit(devs, monkeypatch):
    a, b = devs
    prob, RA, RB = invariance_problem()
    den = CP.den_of(prob)
    genes = drawn_genes(prob[0])
    n = prob[0]
    kw = dict(max_iter=3000)
    config(monkeypatch, a, prob, RA, den, genes, H.LAYOUT_CSR, False, None)
    config(monkeypatch, b, prob, RB, den, genes, H.LAYOUT_CSR, False, None)
    before = [a.solve(**kw)[0], b.solve(**kw)[0], a.compare_genes(b, **kw), b.compare_genes(a, **kw)]
    whole = a.compare_usage(b, **kw)
    after = [a.solve(**kw)[0], b.solve(**kw)[0], a.compare_genes(b, **kw), b.compare_genes(a, **kw)]
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    for x, y in zip(before[2:], after[2:]):
        assert not [k for k in H.COMPARE_GENE_OUTPUTS + ("status", "evals", "parts") if x[k].tobytes() != y[k].tobytes()]
    st = whole["stats"].as_dict()
    print(st)
    assert st["n_status"]["TESTED"] >= 20 and st["outer_max"] <= 12 and st["parts_max"] >= 4 and np.sum(whole["parts"] > 2) >= 5
    assert st["outer_sum"] <= int(whole["outer_evals"].sum()) and st["evals_sum"] <= int(whole["evals"].sum())          # the host's searches are not counted
    q = np.random.default_rng(5).permutation(n).astype(np.int32)
    shuffled = a.compare_usage(b, q, **kw)
    twice = a.compare_usage(b, np.concatenate([q[:10], q[:10], q]), **kw)
    monkeypatch.setenv("EMSAR_HIP_COMPARE_USAGE_BATCH", "1")     # one item per class and launch
    single = a.compare_usage(b, **kw)
    monkeypatch.delenv("EMSAR_HIP_COMPARE_USAGE_BATCH")
    for k in OUTPUTS:
        assert shuffled[k].tobytes() == whole[k][q].tobytes(), k
        assert twice[k][20:].tobytes() == shuffled[k].tobytes() and twice[k][:10].tobytes() == twice[k][10:20].tobytes() == shuffled[k][:10].tobytes(), k
        assert single[k].tobytes() == whole[k].tobytes(), k
    assert stats_of(shuffled) == stats_of(whole) == stats_of(twice) == stats_of(single)
    # a part of the query alone
    part = a.compare_usage(b, q[:7], **kw)
    assert not [k for k in OUTPUTS if part[k].tobytes() != shuffled[k][:7].tobytes()]
    # without a map on ctx_b: ctx_a's map is used for both
    load(b, prob, RB, den, None, H.LAYOUT_CSR)
    assert not same_bits(a.compare_usage(b, **kw), whole)
    for layout, merge, mode in ((H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"), (H.LAYOUT_TILED, True, "2")):
        config(monkeypatch, a, prob, RA, den, genes, layout, merge, mode)
        config(monkeypatch, b, prob, RB, den, genes, layout, merge, mode)
        got = a.compare_usage(b, **kw)
        assert not same_bits(got, whole) and stats_of(got) == stats_of(whole), (layout, merge, mode)
    # the two contexts in different configurations
    config(monkeypatch, b, prob, RB, den, None, H.LAYOUT_CSR, False, None)
    assert not same_bits(a.compare_usage(b, **kw), whole)
    config(monkeypatch, a, prob, RA, den, genes, H.LAYOUT_CSR, False, None)
    config(monkeypatch, b, prob, RB, den, None, H.LAYOUT_TILED, True, "2")
    assert not same_bits(a.compare_usage(b, **kw), whole)


# ---- 6. caps, statuses and errors -------------------------------------------------------------------------------------------------------
def test_unconverged_and_errors(devs):
    a, b = devs
    prob, RA, RB, _ = CP.class_problem(64)
    genes = GP.class_genes(64)
    den = CP.den_of(prob)
    load(a, prob, RA, den, genes)
    load(b, prob, RB, den)
    q = np.array([g[0] for g in genes], dtype=np.int32)
    full = a.compare_usage(b, q, **CAPS)
    capped = a.compare_usage(b, q, max_outer=1, max_evals=2, **CAPS)
    print({k: capped[k] for k in OUTPUTS})
    assert np.all(full["status"] == TESTED) and np.all(capped["status"] == UNCONVERGED)
    assert np.all(capped["outer_evals"] == 2) and np.all(capped["evals"] <= 2 + 4) and np.all(np.isfinite(capped["lambda"])) and np.all(capped["lambda"] >= 0)
    assert capped["usage_a"].tobytes() == full["usage_a"].tobytes() and capped["usage_b"].tobytes() == full["usage_b"].tobytes()
    assert np.all(np.isfinite(capped["usage_null"])) and np.all(np.isfinite(capped["slope"]))
    off = a.compare_usage(b, q, set_mode=1, **CAPS)
    assert np.all(off["status"] == NOT_RESIDENT) and off["stats"].items_launched == 0 and np.all(off["evals"] == 0) and np.all(np.isnan(off["lambda"]))
    for bad in (dict(query=[0, prob[0]]), dict(query=[-1]), dict(dev_tol=math.inf), dict(dev_tol=math.nan), dict(set_mode=2), dict(count_floor=-1.0)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            a.compare_usage(b, **bad, **CAPS)
        assert e.value.status == -1, bad
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_usage(a, **CAPS)
    assert e.value.status == -1
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        b.compare_usage(a, **CAPS)                            # no map on the context that holds sample A
    assert e.value.status == -5
    b.set_gene_map(GP.gene_map(prob[0], genes[::-1]), len(genes))
    with pytest.raises(emsar_amd.EmsarHipError) as e:
        a.compare_usage(b, **CAPS)                            # another map on ctx_b
    assert e.value.status == -1
    b.set_gene_map(GP.gene_map(prob[0], genes), len(genes))
    assert not same_bits(a.compare_usage(b, q, **CAPS), full)


def test_too_large(devs):
    """65 one-transcript rows in one gene: TOO_LARGE; 64: searched on the host; 63 and a set part per sample: the most an item may hold"""
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
    r = a.compare_usage(b, [3, 70], **CAPS)
    assert r["status"][0] == TOO_LARGE and r["evals"][0] == 0 and r["parts"][0] == 0 and all(math.isnan(r[k][0]) for k in H.USAGE_OUTPUTS)
    assert r["status"][1] == TESTED and r["parts"][1] == 128 and r["stats"].items_launched == 0
    g2 = np.full(n, -1, dtype=np.int32)
    g2[list(range(1, 64)) + [n - 1]] = 0
    a.set_gene_map(g2, 1)
    r = a.compare_usage(b, [n - 1, 5], **CAPS)
    assert np.all(r["status"] == TESTED) and np.all(r["parts"] == 128) and r["stats"].items_launched == 2 and r["stats"].parts_max == 128


# ---- 7. the command line --------------------------------------------------------------------------------------------------------------
def test_cli_ucompare_file(tmp_path):
    """-M --compare --g2t with and without --compare-usage on the syn300_se fixture and on every second read of it: out.1.ucompare has one
    line per transcript and its columns are the Python call's as printed; .compare and .gcompare keep their bytes; sample 0 writes none"""
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
    base = [_build.CLI, "-q", "-i", "20000"] + fx.meta["opts"] + ["-M", "--gpus", "1", "--g2t", str(g2t)]
    tail = lambda d: ["-I", rsh_path, str(tmp_path / d), "out", str(lst)]
    subprocess.run(base + ["--compare"] + tail("p"), check=True, timeout=300)
    subprocess.run(base + ["--compare", "--compare-usage"] + tail("o"), check=True, timeout=300)
    for ext in ("compare", "gcompare", "fpkm", "gfpkm"):
        assert (tmp_path / "o" / ("out.1." + ext)).read_bytes() == (tmp_path / "p" / ("out.1." + ext)).read_bytes(), ext
    assert not (tmp_path / "o" / "out.0.ucompare").exists() and not (tmp_path / "p" / "out.1.ucompare").exists()
    # --compare-usage on its own: the same .ucompare, and neither .compare nor .gcompare
    subprocess.run(base + ["--compare-usage"] + tail("u"), check=True, timeout=300)
    assert (tmp_path / "u" / "out.1.ucompare").read_bytes() == (tmp_path / "o" / "out.1.ucompare").read_bytes()
    assert (tmp_path / "u" / "out.1.fpkm").read_bytes() == (tmp_path / "p" / "out.1.fpkm").read_bytes()
    assert not [f for f in os.listdir(tmp_path / "u") if f.endswith(".compare") or f.endswith(".gcompare")] and not (tmp_path / "u" / "out.0.ucompare").exists()
    got = [l.split("\t") for l in (tmp_path / "o" / "out.1.ucompare").read_text().splitlines()]
    assert got[0] == ["transcript", "gene", "usage", "usage_ref", "dlogit", "Lambda", "p", "status", "outer", "evals"]
    got = got[1:]
    assert len(got) == rsh.n_tx and all(len(r) == 10 for r in got)
    assert [r[0] for r in got] == list(rsh.names) and [r[1] for r in got] == ["gene%04d" % (t // 3) for t in range(rsh.n_tx)]
    # usage errors: no --g2t, no -M
    for args in (base[:-2] + ["--compare-usage"] + tail("e"), [_build.CLI, "-q"] + fx.meta["opts"] + ["--g2t", str(g2t), "--compare-usage", "-I", rsh_path,
                                                                                                    str(tmp_path / "e"), "out", str(alns[0])]):
        bad = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and "--compare-usage needs" in bad.stderr, bad.stderr
    # what the CLI does for the two samples, through the Python bindings
    gene_of = np.arange(rsh.n_tx, dtype=np.int32) // 3
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
        p = d1.compare_usage(d0, **cli)
    assert [r[7] for r in got] == [H.USAGE_STATUS[k] for k in p["status"]]
    assert [int(r[8]) for r in got] == list(p["outer_evals"]) and [int(r[9]) for r in got] == list(p["evals"])
    for col, key in ((2, "usage_a"), (3, "usage_b"), (4, "dlogit"), (5, "lambda")):
        v = np.array([float(r[col]) for r in got])
        fin = np.isfinite(p[key])
        assert np.array_equal(np.isnan(v), np.isnan(p[key])) and np.array_equal(v[~fin & ~np.isnan(v)], p[key][~fin & ~np.isnan(p[key])]), key
        assert np.all(np.abs(v[fin] - p[key][fin]) <= 1e-6 + 1e-15 * np.abs(p[key][fin])), key          # "%lf"
    assert [r[5] for r in got] == ["nan" if math.isnan(x) else "inf" if math.isinf(x) else "%f" % x for x in p["lambda"]]
    print(p["stats"].as_dict())
    assert np.sum(p["status"] == TESTED) >= 30
