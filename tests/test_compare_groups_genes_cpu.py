"""CPU: the gene-level K-sample test across replicate groups (include/emsar_hip.h "gene-level K-sample test").  The host's searches
through the diagnostic entry (genes whose parts are all closed form, which emsar_hip_compare_groups_genes answers on the host by the
same code) against closed-form references that know nothing of the library's search, the end of the multiplier's range, identical
samples, the p-values, the numpy reference's own sandwich, the header and the bindings, the .ggroups writer and the CLI's usage text.

The allowance on a Lambda is that of test_compare_groups_genes_gpu.py without its solver terms (a closed form has no solver error):
every searched item is granted (|S| + 1) dev_tol, and 1e-9 stands for the references' own bisections."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from emsar_amd import _build, hip as H, hostlib
from tests import compare_groups_gene_problems as CGG
from tests import compare_groups_problems as CGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTED, ALL_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE = range(6)
DEV_TOL = 1e-4
W_CLOSED = 1e-9


@pytest.fixture(scope="module", autouse=True)
def built():
    _build.build_all()


def allowances(groups):
    K, G = len(groups), max(groups) + 1
    multi = [n for n in (list(groups).count(g) for g in range(G)) if n >= 2]
    within = sum(n + 1 for n in multi) * DEV_TOL + W_CLOSED
    between = 0.0 if G == 1 else ((K + 1) + sum(n + 1 for n in multi)) * DEV_TOL + W_CLOSED
    return between, within


def check(got, ref, groups, sizes, what):
    tb, tw = allowances(groups)
    print(what, "between", got["lambda_between"], ref["lam_between"], "residual", got["lambda_between"] - ref["lam_between"], "tol", tb,
          "| within", got["lambda_within"], ref["lam_within"], "residual", got["lambda_within"] - ref["lam_within"], "tol", tw,
          "| common", got["gene_common"], ref["gene_common"], "outer", got["outer"], "evals", got["evals"])
    assert got["status"] == TESTED, what
    assert abs(got["lambda_between"] - ref["lam_between"]) <= tb and abs(got["lambda_within"] - ref["lam_within"]) <= tw, what
    s = sizes or [1.0] * len(groups)
    ends = [x / k for x, k in zip(ref["gene_hat"], s)]
    width = 1e-6 * (max(ends) - min(ends))
    assert abs(got["gene_common"] - ref["gene_common"]) <= 1e-3 * ref["gene_common"] + width, what
    for g, x in enumerate(ref["gene_group"]):
        assert abs(got["gene_group"][g] - x) <= 1e-3 * x + width, (what, g)
    assert np.all(np.abs(got["gene_hat"] - np.array(ref["gene_hat"])) <= 1e-14 * np.array(ref["gene_hat"])), what
    G = max(groups) + 1
    assert got["p_between"] == H.compare_groups_pvalue_host([got["lambda_between"]], G - 1)[0]
    assert got["p_within"] == H.compare_groups_pvalue_host([got["lambda_within"]], len(groups) - G)[0]


ONE = [(40.0, 2.0), (25.0, 3.0), (60.0, 2.5), (11.0, 1.5)]
SEVERAL = [
    [(30.0, 3.0), (10.0, 5.0)],
    [(20.0, 3.0), (15.0, 5.0), (4.0, 2.0)],
    [(50.0, 3.5), (9.0, 5.0)],
    [(12.0, 3.0), (0.0, 4.0), (33.0, 6.0)],
]


@pytest.mark.parametrize("K, groups, sizes", [(3, (0, 0, 1), None), (4, (0, 0, 1, 1), (1.0, 1.25, 0.8, 1.0)), (3, (0, 1, 2), None), (2, (0, 1), (1.6, 1.0)),
                                              (3, (0, 0, 0), None)])
def test_one_member_genes_against_the_closed_form(K, groups, sizes):
    """a gene of one lone transcript per sample is the transcript test's closed form, x_S = sum u / sum s den, and has the bits of the
    transcript test's own host search"""
    members = [[m] for m in ONE[:K]]
    got = H.debug_compare_groups_genes_closed(members, groups, sizes)
    ref = CGP.closed_groups([m[0] for m in ONE[:K]], [m[1] for m in ONE[:K]], groups, sizes)
    check(got, dict(ref, gene_common=ref["theta_common"], gene_group=ref["theta_group"], gene_hat=ref["theta_hat"]), groups, sizes, ("one", groups))
    tx = H.debug_compare_groups_closed([m[0] for m in ONE[:K]], [m[1] for m in ONE[:K]], groups, sizes)
    for a, b in zip(H.GROUPS_GENE_OUTPUTS, H.GROUPS_OUTPUTS):
        assert got[a] == tx[b], a
    assert got["gene_group"].tobytes() == tx["theta_group"].tobytes() and got["gene_hat"].tobytes() == tx["theta_hat"].tobytes()
    assert (got["status"], got["outer"], got["evals"], got["parts"]) == (tx["status"], tx["outer"], tx["evals"], K)


@pytest.mark.parametrize("K, groups, sizes", [(3, (0, 0, 1), None), (4, (0, 0, 1, 1), (1.0, 1.25, 0.8, 1.0)), (4, (0, 1, 1, 2), None), (3, (0, 1, 2), None),
                                              (2, (0, 0), (0.7, 1.0))])
def test_several_members_against_nested_bisection(K, groups, sizes):
    """genes of several lone transcripts, other members in every sample: 200-halving bisections on lambda_k inside one on x"""
    members = SEVERAL[:K]
    got = H.debug_compare_groups_genes_closed(members, groups, sizes)
    check(got, CGG.closed_gene_groups(members, groups, sizes), groups, sizes, ("several", groups))
    assert got["parts"] == sum(len(m) for m in members) and got["outer"] >= 2
    if max(groups) + 1 == K:
        assert got["lambda_within"] == 0.0 and got["p_within"] == 1.0


def test_a_sample_without_reads_is_the_end_of_the_range():
    """X_hat = 0 in one sample and the member at the smallest den has no reads: no multiplier inside the range raises X there, the
    root is the end of the range and P_k(y) = -mn y"""
    members = [[(30.0, 3.0), (10.0, 5.0)], [(0.0, 2.0), (0.0, 5.0)], [(50.0, 3.0), (9.0, 5.0)]]
    for groups in ((0, 0, 1), (0, 1, 1), (0, 1, 2)):
        got = H.debug_compare_groups_genes_closed(members, groups)
        check(got, CGG.closed_gene_groups(members, groups), groups, None, ("no reads", groups))
        assert got["gene_hat"][1] == 0.0 and got["lambda_between"] + got["lambda_within"] > 10.0       # 40 reads against none
    # the pair (reads, none) alone: C = max_x [P_0(x) - mn x], in closed form sum u log(den / (den + mn)) below F_hat
    got = H.debug_compare_groups_genes_closed(members[:2], (0, 0))
    u, d = np.array([30.0, 10.0]), np.array([3.0, 5.0])
    want = 2.0 * float(np.sum(u * np.log((d + 2.0) / d)))
    print("pair", got["lambda_within"], want)
    assert got["status"] == TESTED and abs(got["lambda_within"] - want) <= 3 * DEV_TOL and got["lambda_between"] == 0.0


def test_identical_and_absent_samples():
    members = [[(30.0, 3.0), (10.0, 5.0), (0.0, 2.0)]] * 3
    got = H.debug_compare_groups_genes_closed(members, (0, 0, 1))
    for k in ("lambda_between", "lambda_within", "raw_between", "raw_within", "slope"):
        assert got[k] == 0.0, k
    assert got["outer"] == 1 and got["p_between"] == 1.0 and got["p_within"] == 1.0 and got["status"] == TESTED and got["evals"] == 3 + 2
    assert got["gene_common"] == got["gene_hat"][0] == 12.0
    got = H.debug_compare_groups_genes_closed([[(0.0, 3.0), (0.0, 5.0)]] * 3, (0, 0, 1))
    assert got["status"] == ALL_ABSENT and got["lambda_between"] == 0.0 and got["lambda_within"] == 0.0 and got["p_between"] == 1.0
    # size factors that make the samples agree: x_k / s_k equal
    got = H.debug_compare_groups_genes_closed([[(30.0, 3.0), (10.0, 5.0)], [(60.0, 3.0), (20.0, 5.0)]], (0, 1), (1.0, 2.0))
    assert got["lambda_between"] == 0.0 and got["outer"] == 1
    # the caps
    capped = H.debug_compare_groups_genes_closed(SEVERAL[:3], (0, 0, 1), max_outer=2)
    assert capped["status"] == UNCONVERGED and capped["outer"] == 2
    for bad in (dict(members=[[(1.0, 0.0)], [(1.0, 1.0)]], groups=(0, 1)), dict(members=[[(-1.0, 1.0)], [(1.0, 1.0)]], groups=(0, 1)),
                dict(members=[[], [(1.0, 1.0)]], groups=(0, 1)), dict(members=[[(1.0, 1.0)], [(1.0, 1.0)]], groups=(0, 2)),
                dict(members=[[(1.0, 1.0)], [(1.0, 1.0)]], groups=(0, 1), sizes=(1.0, 0.0)), dict(members=[[(1.0, 1.0)]], groups=(0,)),
                dict(members=[[(1.0, 1.0)] * 65, [(1.0, 1.0)]], groups=(0, 1))):
        with pytest.raises(H.EmsarHipError) as e:
            H.debug_compare_groups_genes_closed(**bad)
        assert e.value.status == -1, bad


def test_pvalues_are_the_groups_tail():
    got = H.debug_compare_groups_genes_closed(SEVERAL, (0, 1, 1, 2))
    p = H.compare_groups_pvalue_host([got["lambda_between"], got["lambda_within"]], [2, 1])
    assert got["p_between"] == p[0] and got["p_within"] == p[1] and 0.0 < p[0] < 1.0
    assert abs(p[0] - math.exp(-got["lambda_between"] / 2.0)) <= 1e-13 * p[0]
    assert abs(p[1] - math.erfc(math.sqrt(got["lambda_within"] / 2.0))) <= 1e-13 * p[1]


@pytest.mark.parametrize("name", ["small-0-3-6", "small-4-10"])
def test_reference_sandwich_on_the_small_problem(name):
    """the numpy reference bounds every C_g(S) from both sides: U >= L up to the EMs' own bounds, and narrower than W_REF_MAX"""
    prob, Rs, dens, members, groups, sizes = CGG.case_inputs(name)
    samples = [CGG.Sample(prob, Rs[k], dens[k], sorted(members), 1.0) for k in range(3)]
    for S in ([0, 1, 2], [0, 1], [1, 2]):
        c = CGG.common_fit(samples, S)
        free = sum(samples[k].hat["F"] for k in S)
        print(name, S, "U", c["U"], "L", c["L"], "U - L", c["U"] - c["L"], "sum F_hat", free, "x", c["x"])
        assert c["U"] - c["L"] >= -1e-12 and c["width"] <= CGG.W_REF_MAX
        assert c["L"] <= free + 1e-9                       # a common value cannot beat the free fits
        xs = [samples[k].hat["X"] for k in S]
        assert min(xs) <= c["x"] <= max(xs)
    r = CGG.live_reference(name)
    assert r["w_between"] <= CGG.W_REF_MAX and r["w_within"] <= CGG.W_REF_MAX and r["lam_between"] > -1e-9 and r["lam_within"] > -1e-9
    assert r["searched"] == [3, 2]


def test_header_and_bindings():
    text = open(os.path.join(ROOT, "include", "emsar_hip.h")).read()
    assert re.search(r"EMSAR_GENE_GROUPS_TOO_LARGE = (\d)", text).group(1) == str(H.GROUPS_GENE_STATUS.index("TOO_LARGE")) == "5"
    assert H.GROUPS_GENE_STATUS[:5] == H.GROUPS_STATUS
    block = text[text.index("gene-level K-sample test across replicate groups"):text.index("EMSAR_GENE_GROUPS_TOO_LARGE = 5")]
    for word in ("NOT_RESIDENT", "OUTSIDE", "TOO_LARGE", "ALL_ABSENT", "UNCONVERGED", "EMSAR_HIP_GROUPS_GENES_BATCH", "end of the range", "ERR_STATE"):
        assert word in block, word
    for field in H.GROUPS_GENE_OUTPUTS + ("gene_group", "gene_hat") + H.GROUPS_GENE_COUNTS:
        assert re.search(r"\b%s\b[^}]*\} emsar_groups_gene_outputs;" % field, text, re.S), field
    for field, _ in H.GroupsGeneStats._fields_:
        assert re.search(r"\b%s\b[^}]*\} emsar_groups_gene_stats;" % field, text, re.S), field
    assert C.sizeof(H.GroupsGeneStats) == 8 * 6 + 8 * 4 + 4 * 6 + 8 * 3 and C.sizeof(H.GroupsGeneOutputs) == 8 * 14
    assert "emsar_hip_compare_groups_genes" in H.SYMBOLS and "emsar_hip_debug_compare_groups_genes_closed" not in text
    assert set(H.GroupsGeneStats().as_dict()["n_status"]) == set(H.GROUPS_GENE_STATUS)
    assert hasattr(H.EmsarHip, "compare_groups_genes")


def test_ggroups_writer(tmp_path):
    names = ["gA", "gB", "gC", "gD", "gE", "gF", "gG", "gH", "gI"]
    n = len(names)
    status = np.array([0, 1, 2, 3, 4, 5, 6, -1, 2 ** 31 - 1], dtype=np.int32)
    common = np.array([1.5, 0.0, math.nan, math.nan, 2.25, math.nan, 1.0, 1.0, 1.0])
    group = np.column_stack([common + 1.0, common + 2.0])
    lb = np.array([3.25, 0.0, math.nan, math.nan, math.inf, math.nan, 1.0, 1.0, 1.0])
    lw = np.array([0.5, 0.0, math.nan, math.nan, 7.0, math.nan, 1.0, 1.0, 1.0])
    pb, pw = H.compare_groups_pvalue_host(lb, 1), H.compare_groups_pvalue_host(lw, 2)
    outer, evals, parts = np.arange(n, dtype=np.int32), 10 * np.arange(n, dtype=np.int32), 3 + np.arange(n, dtype=np.int32)
    path = str(tmp_path / "a.ggroups")
    hostlib.write_ggroups(path, names, (0, 0, 1, 1), (1.0, 1.25, 0.8, 1.0), common, group, lb, pb, lw, pw, status, outer, evals, parts)
    lines = open(path).read().splitlines()
    assert lines[0] == "# samples=4 groups=0,0,1,1 sizes=1,1.25,0.8,1 df_between=1 df_within=2"
    assert lines[1].split("\t") == ["gene", "gFPKM_common", "gFPKM_g0", "gFPKM_g1", "Lambda_between", "df", "p_between", "Lambda_within", "df", "p_within",
                                    "status", "outer", "evals", "parts"]
    rows = [l.split("\t") for l in lines[2:]]
    assert len(rows) == n and all(len(r) == 14 for r in rows) and [r[0] for r in rows] == names
    assert [r[10] for r in rows] == list(H.GROUPS_GENE_STATUS) + ["?"] * 3
    assert rows[0][1:10] == ["1.500000", "2.500000", "3.500000", "3.250000", "1", "%.6g" % pb[0], "0.500000", "2", "%.6g" % pw[0]]
    assert rows[1][4:10] == ["0.000000", "1", "1", "0.000000", "2", "1"]
    assert rows[2][1:10] == ["nan", "nan", "nan", "nan", "1", "nan", "nan", "2", "nan"]
    assert rows[4][4] == "inf" and rows[4][6] == "0"
    assert [int(r[11]) for r in rows] == list(outer) and [int(r[12]) for r in rows] == list(evals) and [int(r[13]) for r in rows] == list(parts)
    # the "#" line and the shared columns are .groups' own
    tpath = str(tmp_path / "a.groups")
    hostlib.write_groups(tpath, names, (0, 0, 1, 1), (1.0, 1.25, 0.8, 1.0), common, group, lb, pb, lw, pw, np.minimum(status, 4), outer, evals)
    tlines = open(tpath).read().splitlines()
    assert tlines[0] == lines[0] and [l.split("\t")[1:10] for l in tlines[2:]] == [r[1:10] for r in rows]
    # no size factors, three groups
    hostlib.write_ggroups(path, names[:2], (0, 1, 2), None, common[:2], np.column_stack([common[:2]] * 3), lb[:2], pb[:2], lw[:2], pw[:2], status[:2],
                          outer[:2], evals[:2], parts[:2])
    lines = open(path).read().splitlines()
    assert lines[0] == "# samples=3 groups=0,1,2 sizes=1,1,1 df_between=2 df_within=0" and lines[1].split("\t")[1:5] == ["gFPKM_common", "gFPKM_g0", "gFPKM_g1", "gFPKM_g2"]
    assert len(lines) == 4 and lines[2].split("\t")[6] == "2" and lines[2].split("\t")[9] == "0"


def test_cli_usage(tmp_path):
    """the gene file needs no switch of its own: the usage text names it under --compare-groups, and the wrong uses of --compare-groups
    end as they did, with or without --g2t, before anything is read or written"""
    lst = tmp_path / "s3.list"
    lst.write_text("".join("sample%d.bowtie\n" % k for k in range(3)))
    rsh, out, g2t = str(tmp_path / "no.rsh"), str(tmp_path / "o"), str(tmp_path / "no.g2t")
    three = ["-M", "-I", rsh, out, "out", str(lst)]
    for extra in ([], ["--g2t", g2t]):
        for args, msg in ((["--compare-groups", "0,1"] + three, b"one group id per sample"), (["--compare-groups", "0,0,2"] + three, b"0 .. G-1"),
                          (["--compare-groups", "0,0,1", "-I", rsh, out, "out", "one.bowtie"], b"--compare-groups needs -M"),
                          (["--compare-sizes", "1,1,1"] + three, b"--compare-sizes needs --compare-groups")):
            res = subprocess.run([_build.CLI, "-q"] + extra + args, capture_output=True, timeout=60)
            assert res.returncode == 1 and msg in res.stderr and b"Usage" in res.stderr and not os.path.exists(out), (extra, args, res.stderr[:300])
    res = subprocess.run([_build.CLI, "--help"], capture_output=True, timeout=60)
    assert b"<prefix>.ggroups" in res.stderr and b"<prefix>.groups" in res.stderr
    src = open(os.path.join(ROOT, "emsar_amd", "csrc", "host", "emsar_hip_main.c")).read()
    assert "gFPKM_common" not in src and "ALL_ABSENT\"" not in src and "emsar_write_ggroups(" in src       # writer and status words stay in output.c
