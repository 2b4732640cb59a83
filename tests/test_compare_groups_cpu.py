"""CPU: the K-sample test across replicate groups (include/emsar_hip.h "K-sample test") without a device -- the numpy reference against the
two-sample reference and against itself, the host's two-level search on one-transcript components against the closed form, the p-value,
the header and the bindings, the CLI's usage errors and the .groups writer."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from emsar_amd import _build, hip as H, hostlib
from tests import compare_groups_problems as GP
from tests import compare_problems as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTED, ALL_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED = range(5)
DEV_TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def built():
    _build.build_all()


@pytest.mark.parametrize("ratio", [1.0, 1.6])
def test_reference_at_two_samples_is_the_two_sample_reference(ratio):
    """K = 2, groups (0, 1), sizes (r, 1): C(all) is CP.reference's F0 and Lambda_between its Lambda, to 1e-9"""
    prob, RA, RB, tids = CP.class_problem(64)
    den = CP.den_of(prob)
    for t in tids:
        two = CP.reference(prob, RA, RB, t, ratio)
        r = GP.reference(prob, [RA, RB], [den, den], (0, 1), (ratio, 1.0), t)
        print(t, r["lam_between"], two["lam"], r["w_between"])
        assert abs(r["lam_between"] - two["lam"]) <= 1e-9 and r["lam_within"] == 0.0 and r["ended_by_step"]
        assert abs(r["theta_common"] * ratio - two["theta_null"]) <= 1e-9 * two["theta_null"]
        one = GP.reference(prob, [RA, RB], [den, den], (0, 0), (ratio, 1.0), t)
        assert abs(one["lam_within"] - two["lam"]) <= 1e-9 and one["lam_between"] == 0.0


def test_reference_lambdas_add_up():
    """Lambda_between + Lambda_within = 2 (sum F_hat - C(all)): live on the smallest class, and in every recorded case; the recording's
    conditions on its inputs hold for what is in the file"""
    prob, Rs, groups, sizes, tids = GP.case_inputs("64/k4_0011")
    den = CP.den_of(prob)
    r = GP.reference(prob, Rs, [den] * len(Rs), groups, sizes, tids[0])
    rec = GP.recorded()
    assert set(rec) == {"%s:%d" % (name, t) for name in GP.CASE_NAMES for t in GP.case_inputs(name)[4]}
    for key, x in list(rec.items()) + [("live", r)]:
        total = 2.0 * (sum(x["F_hat"]) - x["C_all"])
        assert abs(x["lam_between"] + x["lam_within"] - total) <= 1e-9 * max(1.0, abs(total)), key
        assert x["w_between"] <= GP.W_REF_MAX and x["w_within"] <= GP.W_REF_MAX and x["ended_by_step"], key
        assert x["lam_between"] >= -x["w_between"] and x["lam_within"] >= -x["w_within"], key
    live = rec["64/k4_0011:%d" % tids[0]]
    assert abs(live["lam_between"] - r["lam_between"]) <= 1e-9 and abs(live["lam_within"] - r["lam_within"]) <= 1e-9


CLOSED = [
    ([30, 50, 80], [10, 10, 10], (0, 0, 1), None),
    ([30, 50, 80], [10, 12, 9], (0, 1, 2), None),
    ([30, 0, 80, 20, 5], [10, 12, 9, 10, 3], (0, 0, 1, 1, 2), None),                  # a sample without a read
    ([30, 7, 80, 20, 5], [10, 12, 9, 10, 3], (0, 0, 1, 1, 2), (1.0, 1.3, 0.7, 1.0, 2.0)),
    ([30, 0, 80, 20, 5], [10, 12, 9, 10, 3], (1, 0, 1, 0, 0), (1.0, 1.3, 0.7, 1.0, 2.0)),
    ([12, 40, 9], [4, 4, 2], (0, 0, 0), (1.0, 2.0, 0.5)),
]


@pytest.mark.parametrize("u,den,groups,sizes", CLOSED)
def test_closed_components_against_the_closed_form(u, den, groups, sizes):
    """K one-transcript components: x_S = sum u_k / sum s_k den_k.  Every searched item is granted (|S| + 1) dev_tol, as on the device"""
    r = H.debug_compare_groups_closed(u, den, groups, sizes)
    c = GP.closed_groups(u, den, groups, sizes)
    K, G = len(u), max(groups) + 1
    multi = [n for n in (list(groups).count(g) for g in range(G)) if n >= 2]
    tol_within = sum(n + 1 for n in multi) * DEV_TOL
    tol_between = 0.0 if G == 1 else (K + 1) * DEV_TOL + tol_within
    print(r, c)
    assert r["status"] == TESTED and 2 <= r["outer"] <= 12 and r["slope"] <= DEV_TOL
    assert abs(r["lambda_between"] - c["lam_between"]) <= tol_between + 1e-9 and abs(r["lambda_within"] - c["lam_within"]) <= tol_within + 1e-9
    assert r["lambda_between"] == max(r["raw_between"], 0.0) and r["lambda_within"] == max(r["raw_within"], 0.0)
    if G == 1:
        assert r["raw_between"] == 0.0 and r["theta_group"][0] == r["theta_common"]
    assert abs(r["theta_common"] - c["theta_common"]) <= 1e-3 * c["theta_common"]
    assert np.all(np.abs(r["theta_group"] - np.array(c["theta_group"])) <= 1e-3 * np.array(c["theta_group"]))
    assert r["theta_hat"].tobytes() == (np.array(u, dtype=np.float64) / np.array(den, dtype=np.float64)).tobytes()
    assert r["p_between"] == H.compare_groups_pvalue_host([r["lambda_between"]], G - 1)[0]
    assert r["p_within"] == H.compare_groups_pvalue_host([r["lambda_within"]], K - G)[0]


def test_closed_components_absent_identical_and_capped():
    r = H.debug_compare_groups_closed([0, 0, 0], [1, 2, 3], (0, 1, 1))
    assert r["status"] == ALL_ABSENT and r["lambda_between"] == 0.0 and r["lambda_within"] == 0.0 and r["p_between"] == 1.0 and r["outer"] == 1
    r = H.debug_compare_groups_closed([20, 20, 20], [5, 5, 5], (0, 0, 1))
    assert r["status"] == TESTED and r["raw_between"] == 0.0 and r["raw_within"] == 0.0 and r["outer"] == 1 and r["evals"] == 5
    assert r["theta_common"] == 4.0 and np.all(r["theta_group"] == 4.0)
    r = H.debug_compare_groups_closed([20, 32, 10], [5, 8, 2], (0, 1, 1), (1.0, 1.0, 1.25))     # equal once the size factors are applied
    assert r["status"] == TESTED and r["raw_between"] == 0.0 and r["raw_within"] == 0.0 and r["outer"] == 1
    full = H.debug_compare_groups_closed([30, 50, 80], [10, 10, 10], (0, 0, 1))
    for caps in (dict(max_outer=2), dict(max_evals=1)):
        r = H.debug_compare_groups_closed([30, 50, 80], [10, 10, 10], (0, 0, 1), **caps)
        assert r["status"] == UNCONVERGED and r["theta_hat"].tobytes() == full["theta_hat"].tobytes()
    assert H.debug_compare_groups_closed([30, 50, 80], [10, 10, 10], (0, 0, 1), max_outer=2)["outer"] == 2
    for bad in (dict(groups=(0, 2, 2)), dict(groups=(0, -1, 1)), dict(groups=(1, 1, 1)), dict(sizes=(1.0, 0.0, 1.0)), dict(sizes=(1.0, math.nan, 1.0)),
                dict(u=[1, -1, 2]), dict(den=[1, 0, 2]), dict(dev_tol=math.inf)):
        kw = dict(u=[30, 50, 80], den=[10, 10, 10], groups=(0, 0, 1))
        kw.update(bad)
        with pytest.raises(H.EmsarHipError) as e:
            H.debug_compare_groups_closed(**kw)
        assert e.value.status == -1, bad
    with pytest.raises(H.EmsarHipError):
        H.debug_compare_groups_closed([1.0], [1.0], (0,))
    with pytest.raises(H.EmsarHipError):
        H.debug_compare_groups_closed([1.0] * 33, [1.0] * 33, [0] * 33)


def test_pvalue():
    lam = np.array([0.5, 1.0, 3.841458820694124, 10.0, 40.0])
    p1 = H.compare_groups_pvalue_host(lam, 1)
    assert np.all(np.abs(p1 - np.array([math.erfc(math.sqrt(x / 2.0)) for x in lam])) <= 1e-15 + 1e-13 * p1)
    assert abs(p1[2] - 0.05) <= 1e-12 and p1.tobytes() == H.compare_pvalue_host(lam).tobytes()
    p2 = H.compare_groups_pvalue_host(lam, 2)
    assert np.all(np.abs(p2 - np.exp(-lam / 2.0)) <= 1e-13 * p2)
    assert H.compare_groups_pvalue_host(lam, [1, 2, 3, 4, 5]).tobytes() == H.gene_presence_pvalue_host(lam, [1, 2, 3, 4, 5]).tobytes()
    p = H.compare_groups_pvalue_host([0.0, -1.0, math.inf, math.nan, 0.0, -2.0, 3.0, math.inf, math.nan, 3.0], [3, 3, 3, 3, 0, 0, 0, 0, 0, -1])
    assert list(p[:3]) == [1.0, 1.0, 0.0] and math.isnan(p[3])
    assert list(p[4:8]) == [1.0, 1.0, 0.0, 0.0] and math.isnan(p[8]) and math.isnan(p[9])
    assert len(H.compare_groups_pvalue_host([], [])) == 0


def test_header_and_bindings():
    text = open(os.path.join(ROOT, "include", "emsar_hip.h")).read()
    enum = dict(re.findall(r"EMSAR_GROUPS_([A-Z_]+) = (\d)", text))
    assert [k for k, _ in sorted(enum.items(), key=lambda kv: int(kv[1]))] == list(H.GROUPS_STATUS)
    assert re.search(r"#define EMSAR_COMPARE_GROUPS_MAX (\d+)", text).group(1) == str(H.GROUPS_MAX)
    block = text[text.index("K-sample test across replicate groups"):text.index("EMSAR_GROUPS_TESTED")]
    assert "OVER-DISPERSION" in block and "ANTI-CONSERVATIVE" in block and "CONSERVATIVE WHERE" in block
    for field in ("dev_tol", "max_evals", "max_outer"):
        assert re.search(r"typedef struct \{[^}]*\b%s\b[^}]*\} emsar_groups_params;" % field, text), field
    for field in H.GROUPS_OUTPUTS + ("theta_group", "theta_hat") + H.GROUPS_COUNTS:
        assert re.search(r"\b%s\b[^}]*\} emsar_groups_outputs;" % field, text, re.S), field
    for field, _ in H.GroupsStats._fields_:
        assert re.search(r"\b%s\b[^}]*\} emsar_groups_stats;" % field, text, re.S), field
    assert C.sizeof(H.GroupsStats) == 8 * 5 + 8 * 4 + 4 * 6 + 8 * 3 and C.sizeof(H.GroupsParams) == 16 and C.sizeof(H.GroupsOutputs) == 8 * 13
    assert "emsar_hip_compare_groups" in H.SYMBOLS and "emsar_hip_compare_groups_pvalue_host" in H.SYMBOLS
    assert set(H.GroupsStats().as_dict()["n_status"]) == set(H.GROUPS_STATUS)


def test_cli_usage_errors(tmp_path):
    """every wrong use ends before anything is read or written: the message and the usage text, status 1"""
    lst = {n: tmp_path / ("s%d.list" % n) for n in (1, 3, 33)}
    for n, path in lst.items():
        path.write_text("".join("sample%d.bowtie\n" % k for k in range(n)))
    rsh = str(tmp_path / "no.rsh")
    out = str(tmp_path / "o")
    three = ["-M", "-I", rsh, out, "out", str(lst[3])]
    cases = [
        (["--compare-groups", "0,0,1", "-I", rsh, out, "out", "one.bowtie"], b"--compare-groups needs -M"),
        (["--compare-groups", "0", "-M", "-I", rsh, out, "out", str(lst[1])], b"--compare-groups needs -M and at least two samples"),
        (["--compare-groups", "0,1"] + three, b"one group id per sample"),
        (["--compare-groups", "0,0,1,1"] + three, b"one group id per sample"),
        (["--compare-groups", "0,0,2"] + three, b"0 .. G-1"),
        (["--compare-groups", "1,1,1"] + three, b"0 .. G-1"),
        (["--compare-groups", "0,0,1", "--compare-sizes", "1,2"] + three, b"one size factor per sample"),
        (["--compare-sizes", "1,1,1"] + three, b"--compare-sizes needs --compare-groups"),
        (["--compare-groups", ",".join("0" for _ in range(33)), "-M", "-I", rsh, out, "out", str(lst[33])], b"at most 32 samples"),
    ]
    for args, msg in cases:
        res = subprocess.run([_build.CLI, "-q"] + args, capture_output=True, timeout=60)
        assert res.returncode == 1 and msg in res.stderr and b"Usage" in res.stderr, (args, res.stderr[:300])
        assert not os.path.exists(out)
    for args, msg in ((["--compare-groups", "0,0,1", "--compare-sizes", "1,0,1"] + three, b"positive size factors"),
                      (["--compare-groups", "0,0,1", "--compare-sizes", "1,-2,1"] + three, b"positive size factors"),
                      (["--compare-groups", "0,x,1"] + three, b"list of group ids"), (["--compare-groups", "0,-1,1"] + three, b"list of group ids")):
        res = subprocess.run([_build.CLI, "-q"] + args, capture_output=True, timeout=60)
        assert res.returncode == 1 and msg in res.stderr and not os.path.exists(out), (args, res.stderr[:300])
    res = subprocess.run([_build.CLI, "--help"], capture_output=True, timeout=60)
    assert b"--compare-groups" in res.stderr and b"--compare-sizes" in res.stderr


def test_groups_writer(tmp_path):
    names = ["tA", "tB", "tC", "tD", "tE", "tF", "tG", "tH", "tI"]
    n = len(names)
    status = np.array([0, 1, 2, 3, 4, 5, -1, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    common = np.array([1.5, 0.0, math.nan, math.nan, 2.25, 1.0, 1.0, 1.0, 1.0])
    group = np.column_stack([common + 1.0, common + 2.0])
    lb = np.array([3.25, 0.0, math.nan, math.nan, math.inf, 1.0, 1.0, 1.0, 1.0])
    lw = np.array([0.5, 0.0, math.nan, math.nan, 7.0, 1.0, 1.0, 1.0, 1.0])
    pb, pw = H.compare_groups_pvalue_host(lb, 1), H.compare_groups_pvalue_host(lw, 2)
    outer, evals = np.arange(n, dtype=np.int32), 10 * np.arange(n, dtype=np.int32)
    path = str(tmp_path / "a.groups")
    hostlib.write_groups(path, names, (0, 0, 1, 1), (1.0, 1.25, 0.8, 1.0), common, group, lb, pb, lw, pw, status, outer, evals)
    lines = open(path).read().splitlines()
    assert lines[0] == "# samples=4 groups=0,0,1,1 sizes=1,1.25,0.8,1 df_between=1 df_within=2"
    assert lines[1].split("\t") == ["transcript", "FPKM_common", "FPKM_g0", "FPKM_g1", "Lambda_between", "df", "p_between", "Lambda_within", "df", "p_within",
                                    "status", "outer", "evals"]
    rows = [l.split("\t") for l in lines[2:]]
    assert len(rows) == n and all(len(r) == 13 for r in rows) and [r[0] for r in rows] == names
    assert [r[10] for r in rows] == list(H.GROUPS_STATUS) + ["?"] * 4
    assert rows[0][1:10] == ["1.500000", "2.500000", "3.500000", "3.250000", "1", "%.6g" % pb[0], "0.500000", "2", "%.6g" % pw[0]]
    assert rows[1][4:10] == ["0.000000", "1", "1", "0.000000", "2", "1"]
    assert rows[2][1:10] == ["nan", "nan", "nan", "nan", "1", "nan", "nan", "2", "nan"]
    assert rows[4][4] == "inf" and rows[4][6] == "0"
    assert [int(r[11]) for r in rows] == list(outer) and [int(r[12]) for r in rows] == list(evals)
    # a query and no size factors
    q = [7, 2]
    hostlib.write_groups(path, names, (0, 1), None, common[:2], group[:2], lb[:2], pb[:2], lw[:2], pw[:2], status[:2], outer[:2], evals[:2], query=q)
    lines = open(path).read().splitlines()
    assert lines[0] == "# samples=2 groups=0,1 sizes=1,1 df_between=1 df_within=0" and [l.split("\t")[0] for l in lines[2:]] == ["tH", "tC"]
