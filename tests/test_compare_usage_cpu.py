"""CPU: the two-sample test of isoform usage (include/emsar_hip.h "two-sample test of isoform usage") on the host path -- the two-level
search the library runs for a gene whose parts are all closed form, through emsar_hip_debug_compare_usage_closed, which makes no HIP
call -- against closed formulas, SLSQP and the numpy reference of tests/compare_usage_problems.py; the header, the bindings and the
recorded references the GPU tests compare with.

The tolerance against an exact value is 3 dev_tol: each of the two inner searches and the outer search is granted dev_tol, and their
stopping rules bound it (closed forms have no solver residual)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from emsar_amd import hip as H
from tests import compare_usage_problems as UP

TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE, UNDEFINED, SINGLE = range(8)
DEV_TOL = 1e-4
TOL = 3 * DEV_TOL

# two members, both lone in both samples, t first: (u_a, den_a, u_b, den_b)
PAIRS = [
    ([30, 50], [2.0, 3.0], [70, 20], [2.0, 3.0]),
    ([5, 400], [0.7, 11.0], [9, 380], [0.9, 10.0]),
    ([1200, 900], [40.0, 55.0], [1000, 1100], [38.0, 61.0]),
    ([3, 2], [1.0, 1.0], [1, 6], [1.0, 1.0]),
    ([0, 50], [2.0, 3.0], [70, 20], [2.0, 3.0]),          # the share 0 in A
    ([64, 0], [2.0, 3.0], [70, 20], [2.0, 3.0]),          # the share 1 in A
]


@pytest.mark.parametrize("k", range(len(PAIRS)))
def test_lone_two_member_gene(k):
    ua, da, ub, db = PAIRS[k]
    want, share = UP.lone_pair_lambda(ua, da, ub, db)
    r = H.debug_compare_usage_closed(ua, da, ub, db)
    print(k, r, "formula", want, share, "residual", r["lambda"] - want)
    assert r["status"] == TESTED and r["parts"] == 4
    assert abs(r["lambda"] - want) <= TOL
    assert r["raw_lambda"] == r["lambda"] and r["pvalue"] == H.compare_pvalue_host(r["lambda"])
    ea, eb = (ua[0] / da[0]) / (ua[0] / da[0] + ua[1] / da[1]), (ub[0] / db[0]) / (ub[0] / db[0] + ub[1] / db[1])
    assert abs(r["usage_a"] - ea) <= 1e-15 and abs(r["usage_b"] - eb) <= 1e-15
    assert min(ea, eb) <= r["usage_null"] <= max(ea, eb) and abs(r["usage_null"] - share) <= 1e-3
    assert 2 <= r["outer_evals"] <= 12 and r["evals"] > 2
    assert r["slope"] <= DEV_TOL
    # the second member's share is the complement: the same null, the same statistic
    s = H.debug_compare_usage_closed(ua, da, ub, db, t=1)
    assert abs(s["lambda"] - want) <= TOL and abs(s["usage_a"] + r["usage_a"] - 1.0) <= 1e-15


def slsqp_lambda(ua, da, ub, db, t):
    """max F^A + F^B under theta_t^A X^B = theta_t^B X^A, from several starts"""
    from scipy.optimize import minimize
    ua, da, ub, db = (np.asarray(x, dtype=np.float64) for x in (ua, da, ub, db))
    n = len(ua)
    u, d = np.concatenate([ua, ub]), np.concatenate([da, db])

    def negF(z):
        x = np.exp(z)
        return -(float(np.dot(u, z)) - float(np.dot(x, d)))

    def grad(z):
        return -(u - np.exp(z) * d)

    def con(z):
        x = np.exp(z)
        return x[t] * x[n:].sum() - x[n + t] * x[:n].sum()
    F1 = float(np.sum(u * np.log(u / d))) - float(u.sum())
    best = np.inf
    for share in (0.2, 0.5, 0.8):
        xa, xb = ua / da, ub / db
        for x in (xa, xb):
            O = x.sum() - x[t]
            x[t] = share * O / (1.0 - share)
        r = minimize(negF, np.log(np.concatenate([xa, xb])), jac=grad, constraints=[dict(type="eq", fun=con)], method="SLSQP",
                     options=dict(ftol=1e-14, maxiter=500))
        if r.success and abs(con(r.x)) <= 1e-8:
            best = min(best, r.fun)
    return 2.0 * (F1 + best)


TRIPLES = [
    ([30, 50, 10], [2.0, 3.0, 1.5], [70, 20, 40], [2.0, 3.0, 1.5], 1),
    ([30, 50, 10], [2.0, 3.0, 1.5], [70, 20, 40], [2.0, 3.0, 1.5], 0),
    ([300, 500, 100], [20.0, 33.0, 15.0], [350, 420, 160], [22.0, 30.0, 14.0], 2),
]


@pytest.mark.parametrize("k", range(len(TRIPLES)))
def test_lone_three_member_gene_against_slsqp(k):
    pytest.importorskip("scipy")
    ua, da, ub, db, t = TRIPLES[k]
    want = slsqp_lambda(ua, da, ub, db, t)
    r = H.debug_compare_usage_closed(ua, da, ub, db, t=t)
    print(k, r, "slsqp", want, "residual", r["lambda"] - want)
    assert r["status"] == TESTED and r["parts"] == 6
    assert abs(r["lambda"] - want) <= TOL + 1e-7          # SLSQP's own ftol on F ~ 1e3


def test_reference_agrees_on_a_lone_gene():
    """the numpy reference (grid and refinement over plain EMs) against the closed formula: it is what the GPU tests trust"""
    ua, da, ub, db = PAIRS[0]
    prob, RA, RB, den_a, den_b = UP.lone_problem(ua, da, ub, db)
    ref = UP.reference(prob, RA, RB, [0, 1], 0, den_a, den_b, grid=41)
    want, share = UP.lone_pair_lambda(ua, da, ub, db)
    print(ref["lam"], want, ref["w_ref"], ref["usage_null"], share, ref["peaks"])
    assert abs(ref["lam"] - want) <= 1e-7 and ref["w_ref"] <= 1e-7 and ref["peaks"] == 1
    r = H.debug_compare_usage_closed(ua, da, ub, db)
    assert abs(r["lambda"] - ref["lam"]) <= TOL + ref["w_ref"]


def test_symmetry():
    for ua, da, ub, db in PAIRS:
        r, s = H.debug_compare_usage_closed(ua, da, ub, db), H.debug_compare_usage_closed(ub, db, ua, da)
        assert abs(r["lambda"] - s["lambda"]) <= TOL, (r, s)
        assert r["usage_a"] == s["usage_b"] and r["usage_b"] == s["usage_a"]
        assert r["dlogit"] == -s["dlogit"]
    for ua, da, ub, db, t in TRIPLES:
        r, s = H.debug_compare_usage_closed(ua, da, ub, db, t=t), H.debug_compare_usage_closed(ub, db, ua, da, t=t)
        assert abs(r["lambda"] - s["lambda"]) <= TOL and r["dlogit"] == -s["dlogit"]


def test_scaling():
    """The share is scale-free, so no ratio parameter is needed.  A depth factor on B -- theta_B seven times larger or smaller at the
    same reads, which is den_B scaled -- moves F^B by a constant under H1 and H0 alike: Lambda stays within the tolerance and the shares
    keep their values.  B's read weights times 7 at the same den is seven times the information in B, not a depth factor: the shares
    stay, equal shares still give exactly 0, and Lambda is the closed formula's of the scaled reads (it grows)."""
    for ua, da, ub, db in PAIRS[:5]:
        base = H.debug_compare_usage_closed(ua, da, ub, db)
        for f in (7.0, 1.0 / 7.0):
            r = H.debug_compare_usage_closed(ua, da, ub, [x * f for x in db])
            assert abs(r["lambda"] - base["lambda"]) <= 2 * TOL, (f, r, base)
            assert abs(r["usage_b"] - base["usage_b"]) <= 1e-15 and r["usage_a"] == base["usage_a"]
        ub7 = [7 * x for x in ub]
        want, _ = UP.lone_pair_lambda(ua, da, ub7, db)
        r = H.debug_compare_usage_closed(ua, da, ub7, db)
        assert abs(r["lambda"] - want) <= TOL and abs(r["usage_b"] - base["usage_b"]) <= 1e-15 and r["lambda"] >= base["lambda"] - TOL
    r = H.debug_compare_usage_closed([30, 50], [2.0, 3.0], [7 * 30, 7 * 50], [2.0, 3.0])
    assert r["lambda"] <= TOL and abs(r["usage_a"] - r["usage_b"]) <= 1e-15


def test_equal_shares():
    r = H.debug_compare_usage_closed([30, 50, 10], [2.0, 3.0, 1.5], [60, 100, 20], [2.0, 3.0, 1.5], t=1)
    assert r["status"] == TESTED and r["lambda"] == 0.0 and r["raw_lambda"] == 0.0 and r["pvalue"] == 1.0
    assert r["outer_evals"] == 1 and r["evals"] == 2 and r["usage_a"] == r["usage_b"] == r["usage_null"] and r["dlogit"] == 0.0
    # depth differs by a power of two: the shares are the same bits
    r = H.debug_compare_usage_closed([30, 50], [2.0, 3.0], [120, 200], [2.0, 3.0])
    assert r["lambda"] == 0.0 and r["outer_evals"] == 1


def test_share_at_the_boundary():
    ua, da, ub, db = PAIRS[4]
    r = H.debug_compare_usage_closed(ua, da, ub, db)
    print(r)
    assert r["status"] == TESTED and math.isfinite(r["lambda"]) and r["lambda"] > 50 and r["usage_a"] == 0.0
    assert r["dlogit"] == -math.inf and 0.0 < r["usage_null"] < r["usage_b"]
    want, _ = UP.lone_pair_lambda(ua, da, ub, db)
    assert abs(r["lambda"] - want) <= TOL
    # the closed limit: sample A has no read on t, so P_A(u) = u_s log(u_s / (d_s + d_t u / (1 - u))) - u_s
    ua, da, ub, db = PAIRS[5]
    r = H.debug_compare_usage_closed(ua, da, ub, db)
    assert r["status"] == TESTED and r["usage_a"] == 1.0 and r["dlogit"] == math.inf and math.isfinite(r["lambda"])
    # both at the same end
    r = H.debug_compare_usage_closed([0, 50, 4], [2.0, 3.0, 1.0], [0, 20, 9], [2.0, 3.0, 1.0])
    assert r["status"] == BOTH_ABSENT and r["lambda"] == 0.0 and r["pvalue"] == 1.0 and math.isnan(r["dlogit"]) and r["outer_evals"] == 1


def test_statuses_the_host_decides():
    nan_out = lambda r: all(math.isnan(r[k]) for k in H.USAGE_OUTPUTS) and r["outer_evals"] == 0 and r["evals"] == 0 and r["parts"] == 0
    r = H.debug_compare_usage_closed([30, 50], [0.0, 3.0], [70, 20], [2.0, 3.0])          # den_t == 0 in A
    assert r["status"] == OUTSIDE and nan_out(r)
    r = H.debug_compare_usage_closed([30, 50], [2.0, 3.0], [70, 20], [0.0, 3.0])          # den_t == 0 in B
    assert r["status"] == OUTSIDE and nan_out(r)
    r = H.debug_compare_usage_closed([30, 50], [2.0, 0.0], [70, 20], [2.0, 3.0])          # t alone takes part in A
    assert r["status"] == SINGLE and nan_out(r)
    r = H.debug_compare_usage_closed([30], [2.0], [70], [2.0])
    assert r["status"] == SINGLE and nan_out(r)
    rng = np.random.default_rng(4)
    u, d = rng.integers(1, 50, size=65).astype(float), rng.uniform(1.0, 3.0, size=65)
    r = H.debug_compare_usage_closed(u, d, u[::-1].copy(), d)
    assert r["status"] == TOO_LARGE and nan_out(r)
    r = H.debug_compare_usage_closed(u[:64], d[:64], u[:64][::-1].copy(), d[:64], t=5)
    assert r["status"] == TESTED and r["parts"] == 128
    # a member with den == 0 takes no part: the same bits as without it; t_b names t's place in B's list
    r3 = H.debug_compare_usage_closed([30, 50, 9], [2.0, 3.0, 0.0], [8, 70, 20], [0.0, 2.0, 3.0], t=0, t_b=1)
    r2 = H.debug_compare_usage_closed([30, 50], [2.0, 3.0], [70, 20], [2.0, 3.0])
    assert r3 == r2
    r = H.debug_compare_usage_closed([0, 0], [2.0, 3.0], [70, 20], [2.0, 3.0])            # the gene sum of A is 0
    assert r["status"] == UNDEFINED and math.isnan(r["lambda"]) and math.isnan(r["usage_a"]) and r["outer_evals"] == 1 and r["evals"] == 2
    ua, da, ub, db = PAIRS[0]
    r = H.debug_compare_usage_closed(ua, da, ub, db, max_outer=1, max_evals=2)
    full = H.debug_compare_usage_closed(ua, da, ub, db)
    assert r["status"] == UNCONVERGED and r["outer_evals"] == 2 and r["evals"] == 2 + 4 and math.isfinite(r["lambda"]) and r["lambda"] > 0
    assert r["usage_a"] == full["usage_a"] and r["usage_b"] == full["usage_b"]
    r = H.debug_compare_usage_closed(ua, da, ub, db, max_outer=2)
    assert r["status"] == UNCONVERGED and r["outer_evals"] == 2
    for bad in (dict(dev_tol=math.inf), dict(dev_tol=math.nan), dict(t=2), dict(t=-1)):
        with pytest.raises(H.EmsarHipError) as e:
            H.debug_compare_usage_closed(ua, da, ub, db, **bad)
        assert e.value.status == -1, bad
    with pytest.raises(H.EmsarHipError):
        H.debug_compare_usage_closed([-1, 5], da, ub, db)


def test_tolerance_scales_the_work():
    ua, da, ub, db = PAIRS[2]
    want, _ = UP.lone_pair_lambda(ua, da, ub, db)
    loose, tight = H.debug_compare_usage_closed(ua, da, ub, db, dev_tol=1e-2), H.debug_compare_usage_closed(ua, da, ub, db, dev_tol=1e-8, max_outer=40)
    assert abs(loose["lambda"] - want) <= 3e-2 and abs(tight["lambda"] - want) <= 3e-8 + 1e-9 and tight["evals"] > loose["evals"]
    assert tight["status"] == TESTED


def test_header_and_bindings():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emsar_hip.h")).read()
    enum = dict(re.findall(r"EMSAR_USAGE_([A-Z_]+) = (\d)", text))
    assert {k: int(v) for k, v in enum.items()} == {name: i for i, name in enumerate(H.USAGE_STATUS)}
    assert H.USAGE_STATUS == ("TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE", "UNDEFINED", "SINGLE")
    assert C.sizeof(H.UsageParams) == 16
    assert C.sizeof(H.UsageOutputs) == 12 * C.sizeof(C.c_void_p)
    assert C.sizeof(H.UsageStats) == 8 * 8 + 8 * 4 + 4 * 4 + 8 * 3
    assert H.USAGE_OUTPUTS == ("lambda", "raw_lambda", "pvalue", "usage_a", "usage_b", "usage_null", "dlogit", "slope")
    assert "emsar_hip_compare_usage" in H.SYMBOLS
    for field in ("dev_tol", "max_evals", "max_outer"):
        assert re.search(r"typedef struct \{[^}]*\b%s\b[^}]*\} emsar_usage_params;" % field, text), field
    for field in ("outer_sum", "outer_max"):
        assert re.search(r"\b%s\b[^}]*\} emsar_usage_stats;" % field, text, re.S), field


def test_recorded_references():
    """what the GPU tests compare with: every recorded gene has one local maximum on the reference's grid and a narrow reference"""
    rec = UP.recorded()
    for name, ref in rec.items():
        print(name, ref)
        assert name in UP.CASES and ref["peaks"] == 1 and ref["w_ref"] <= 1e-7 and ref["lam"] > 0.0, name
    assert set(rec) == set(UP.CASES)
    # one of them again, from a coarser grid: the refinement reaches the same maximum when there is one peak
    prob, RA, RB, den_a, den_b, members, t = UP.case("small-0-3-6:3")
    again = UP.reference(prob, RA, RB, members, t, den_a, den_b, grid=11)
    assert abs(again["lam"] - rec["small-0-3-6:3"]["lam"]) <= 1e-7 and again["parts"] == rec["small-0-3-6:3"]["parts"] and again["peaks"] == 1
    # and one at the full grid, a share at the boundary: the file is what the code computes, its count of peaks included
    prob, RA, RB, den_a, den_b, members, t = UP.case("small-0-3-6:6")
    full = UP.reference(prob, RA, RB, members, t, den_a, den_b)
    for k in UP.KEPT:
        assert full[k] == rec["small-0-3-6:6"][k], (k, full[k], rec["small-0-3-6:6"][k])
    assert full["peaks"] == 1 and len(full["grid_u"]) == UP.GRID


def test_writer_byte_for_byte(tmp_path):
    """.ucompare (emsar_write_ucompare): five transcripts, one in no gene (an empty gene field, as for the gene with the empty name), a query list
    out of order with repeats, every status and one outside the range, and nan, +inf and -inf in each of the five number columns -- the
    sign of an infinity is printed"""
    from emsar_amd import _build, hostlib
    _build.build_all()
    nan, inf = float("nan"), float("inf")
    p = str(tmp_path / "a.ucompare")
    hostlib.write_ucompare(p, ["tA", "tB", "tC", "tD", "tE"], ["g1", "", "g3"], [0, 2, -1, 0, 1],
                           [0.25, nan, inf, -inf, 0.0, 1.0, 1e-7, 0.5, 0.5], [0.75, nan, inf, -inf, 1.0, 0.0, 0.999999, 0.5, 0.5],
                           [-2.197225, nan, inf, -inf, -4e-7, 30.5, 0.0, 0.0, 0.0], [3.25, nan, inf, -inf, 0.0, 10.0, 0.125, 0.0, 0.0],
                           [0.0714, nan, inf, -inf, 1.0, 1e-300, 0.123456789, 1.0, 1.0], [0, 1, 2, 3, 4, 5, 6, 7, 8], [5, 0, 1, 12, 3, 0, 0, 0, 2],
                           [120, 0, 1, 480, 7, 3, 0, 0, 2], query=[3, 0, 4, 0, 1, 2, 4, 2, 1])
    assert open(p, "rb").read() == (b"transcript\tgene\tusage\tusage_ref\tdlogit\tLambda\tp\tstatus\touter\tevals\n"
                                    b"tD\tg1\t0.250000\t0.750000\t-2.197225\t3.250000\t0.0714\tTESTED\t5\t120\n"
                                    b"tA\tg1\tnan\tnan\tnan\tnan\tnan\tBOTH_ABSENT\t0\t0\n"
                                    b"tE\t\tinf\tinf\tinf\tinf\tinf\tOUTSIDE\t1\t1\n"
                                    b"tA\tg1\t-inf\t-inf\t-inf\t-inf\t-inf\tNOT_RESIDENT\t12\t480\n"
                                    b"tB\tg3\t0.000000\t1.000000\t-0.000000\t0.000000\t1\tUNCONVERGED\t3\t7\n"
                                    b"tC\t\t1.000000\t0.000000\t30.500000\t10.000000\t1e-300\tTOO_LARGE\t0\t3\n"
                                    b"tE\t\t0.000000\t0.999999\t0.000000\t0.125000\t0.123457\tUNDEFINED\t0\t0\n"
                                    b"tC\t\t0.500000\t0.500000\t0.000000\t0.000000\t1\tSINGLE\t0\t0\n"
                                    b"tB\tg3\t0.500000\t0.500000\t0.000000\t0.000000\t1\t?\t2\t2\n")
