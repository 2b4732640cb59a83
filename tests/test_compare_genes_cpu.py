"""CPU: the gene-level two-sample test's host side (include/emsar_hip.h "gene-level two-sample test") -- the search the host runs for a
gene whose parts are all closed form (emsar_hip_debug_compare_genes_closed) against an independent solution of its equation, the
numpy reference of tests/compare_gene_problems.py against the per-transcript reference and against a constrained optimiser, and the
argument errors that need no device."""
import math

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import compare_gene_problems as GP
from tests import compare_problems as CP

TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE = range(6)
DEV_TOL = 1e-4
W_REF_MAX = 1e-7                 # what the reference may be wrong by on any gene a test uses


def test_names():
    import ctypes as C
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emsar_hip.h")).read()
    assert re.search(r"EMSAR_GENE_COMPARE_TOO_LARGE = 5\b", text) and TOO_LARGE == 5
    assert C.sizeof(H.CompareGeneOutputs) == 12 * C.sizeof(C.c_void_p)
    assert C.sizeof(H.CompareGeneStats) == 8 * 6 + 8 * 3 + 4 * 4 + 8 * 3
    assert H.COMPARE_GENE_STATUS == ("TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE")
    assert H.COMPARE_GENE_OUTPUTS == ("lambda", "pvalue", "log2fc", "gene_a", "gene_b", "gene_null", "multiplier", "gap", "raw_lambda")


CLOSED = [
    ("1+1", [30.0], [2.0], [10.0], [3.0], 1.0),
    ("3+2", [30.0, 5.0, 0.0], [2.0, 1.5, 4.0], [10.0, 1.0], [3.0, 0.5], 1.0),
    ("1+4", [12.0], [0.7], [40.0, 3.0, 9.0, 1.0], [2.5, 2.5, 0.9, 6.0], 1.0),
    ("3+2 ratio 0.7", [30.0, 5.0, 0.0], [2.0, 1.5, 4.0], [10.0, 1.0], [3.0, 0.5], 0.7),
    ("1+4 ratio 0.7", [12.0], [0.7], [40.0, 3.0, 9.0, 1.0], [2.5, 2.5, 0.9, 6.0], 0.7),
    ("down", [3.0, 2.0], [2.0, 2.0], [40.0, 9.0], [2.5, 0.9], 1.0),
]


@pytest.mark.parametrize("name,u_a,d_a,u_b,d_b,ratio", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_gene_against_bisection(name, u_a, d_a, u_b, d_b, ratio):
    r = H.debug_compare_genes_closed(u_a, d_a, u_b, d_b, ratio=ratio)
    want, lam = GP.closed_gene_lambda(u_a, d_a, u_b, d_b, ratio)
    print(name, r, want, lam)
    assert r["status"] == TESTED and 1 < r["evals"] <= 40
    assert abs(r["lambda"] - want) <= DEV_TOL
    assert r["lambda"] <= want + 1e-9                        # the dual value is a lower bound of the statistic
    assert r["gene_a"] == pytest.approx(sum(u / d for u, d in zip(u_a, d_a)), rel=1e-14)
    assert r["gene_b"] == pytest.approx(sum(u / d for u, d in zip(u_b, d_b)), rel=1e-14)
    assert r["log2fc"] == pytest.approx(math.log2(r["gene_a"] / (ratio * r["gene_b"])), abs=1e-12)
    assert r["pvalue"] == H.compare_pvalue_host(r["lambda"])
    assert abs(r["multiplier"] - lam) <= 1e-2 * abs(lam)


def test_closed_gene_one_member_is_the_transcript_test():
    """the two paths shift den differently (den + lambda against den * scale): not the same bits, the same Lambda within dev_tol"""
    for ratio in (1.0, 0.7):
        g = H.debug_compare_genes_closed([30.0], [2.0], [10.0], [3.0], ratio=ratio)
        t = H.debug_compare_closed(30.0, 2.0, 10.0, 3.0, ratio=ratio)
        assert g["status"] == t["status"] == TESTED and abs(g["lambda"] - t["lambda"]) <= DEV_TOL
        assert g["gene_a"] == t["theta_a"] and g["gene_b"] == t["theta_b"]
        assert abs(g["lambda"] - CP.closed_pair_lambda(30.0, 2.0, 10.0, 3.0, ratio)[0]) <= DEV_TOL


def test_closed_gene_boundaries():
    # no read in A: the root is the end of the range, Lambda finite, ended by the bracket-width rule
    for u_a, d_a, u_b, d_b in (([0.0, 0.0], [2.0, 1.5], [10.0, 1.0], [3.0, 0.5]), ([10.0, 1.0], [3.0, 0.5], [0.0, 0.0], [2.0, 1.5])):
        r = H.debug_compare_genes_closed(u_a, d_a, u_b, d_b)
        want, _ = GP.closed_gene_lambda(u_a, d_a, u_b, d_b)
        print(r, want)
        assert r["status"] == TESTED and math.isfinite(r["lambda"]) and abs(r["lambda"] - want) <= DEV_TOL
        assert math.isinf(r["log2fc"]) and (r["log2fc"] < 0) == (sum(u_a) == 0)
    r = H.debug_compare_genes_closed([0.0, 0.0], [2.0, 1.5], [0.0], [3.0])
    assert r["status"] == BOTH_ABSENT and r["lambda"] == 0.0 and r["pvalue"] == 1.0 and r["evals"] == 1 and math.isnan(r["log2fc"])
    # equal sums: one evaluation
    r = H.debug_compare_genes_closed([4.0, 4.0], [2.0, 2.0], [8.0], [2.0])
    assert r["status"] == TESTED and r["lambda"] == 0.0 and r["evals"] == 1
    # the cap
    r = H.debug_compare_genes_closed([30.0, 5.0], [2.0, 1.5], [10.0], [3.0], max_evals=1)
    assert r["status"] == UNCONVERGED and r["evals"] == 1 and r["lambda"] == 0.0


def test_closed_gene_stays_in_range_next_to_the_end():
    """members whose den differ by one ulp on the side that shrinks to the end of its range: every den' stays positive, so nothing is NaN"""
    d = 3.0
    r = H.debug_compare_genes_closed([50.0, 20.0], [2.0, 2.5], [0.0, 0.0, 0.0], [d, np.nextafter(d, 4.0), d], dev_tol=1e-12, max_evals=200)
    assert all(math.isfinite(r[k]) for k in ("lambda", "gene_null", "multiplier", "gap", "raw_lambda")), r


def test_argument_errors():
    for bad in (dict(u_a=[], den_a=[]), dict(den_a=[0.0]), dict(u_a=[-1.0]), dict(u_b=[math.nan]), dict(den_b=[-2.0]), dict(ratio=-1.0),
                dict(ratio=math.inf), dict(dev_tol=math.nan)):
        kw = dict(u_a=[1.0], den_a=[1.0], u_b=[1.0], den_b=[1.0])
        kw.update(bad)
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            H.debug_compare_genes_closed(**kw)
        assert e.value.status == -1, bad
    with pytest.raises(ValueError):
        H.debug_compare_genes_closed([1.0, 2.0], [1.0], [1.0], [1.0])
    L = H.load_library()
    assert L.emsar_hip_compare_genes(None, None, None, None, 0, None, None, None) == -1


# ---- the reference checks itself ----------------------------------------------------------------------------------------------------
def test_reference_one_member_gene_is_the_stacked_reference():
    prob, RA, RB, tids = CP.class_problem(64)
    for t in tids:
        g, c = GP.reference(prob, RA, RB, [t]), CP.reference(prob, RA, RB, t)
        print(t, g["lam"], c["lam"], g["w_ref"])
        assert g["w_ref"] <= W_REF_MAX and abs(g["lam"] - c["lam"]) <= g["w_ref"] + 1e-7
    prob, RA, RB, den_a, den_b = CP.small_problem()
    for t in (3, 6):                                          # 6: no read in B, the root is the end of the range
        g, c = GP.reference(prob, RA, RB, [t], 1.0, den_a, den_b), CP.reference(prob, RA, RB, t, 1.0, den_a, den_b)
        print(t, g["lam"], c["lam"], g["w_ref"])
        assert g["w_ref"] <= W_REF_MAX and abs(g["lam"] - c["lam"]) <= g["w_ref"] + 1e-7


@pytest.mark.parametrize("name", GP.TESTED_GENES)
def test_reference_width_on_the_tested_genes(name):
    """w_ref <= 1e-7 on every gene the GPU tests compare against"""
    r, members = GP.tested_reference(name)
    print(name, members, r["lam"], r["w_ref"], r["multiplier"], r["parts"], r["evals"])
    assert r["w_ref"] <= W_REF_MAX


def test_reference_gives_none_without_a_part():
    prob, RA, RB, den_a, den_b = CP.small_problem()
    assert GP.reference(prob, RA, RB, [10], 1.0, den_a, den_b) is None           # den = 0 in B: no part there


def test_reference_two_member_gene_against_slsqp():
    """small_problem (11 transcripts), gene {3, 4}: maximise F_A + F_B over every transcript of the two components under the linear
    equality sum_members x_A = r sum_members x_B"""
    opt = pytest.importorskip("scipy.optimize")
    prob, RA, RB, den_a, den_b = CP.small_problem()
    members, ratio = [3, 4], 1.0
    pa, pb = GP.parts_of(prob, RA, den_a, members), GP.parts_of(prob, RB, den_b, members)
    assert len(pa) == 1 and len(pb) == 1
    a, b = pa[0], pb[0]
    live_a, live_b = np.flatnonzero(a.den > 0), np.flatnonzero(b.den > 0)
    na = len(live_a)

    def split(z):
        xa, xb = np.zeros(len(a.tids)), np.zeros(len(b.tids))
        xa[live_a], xb[live_b] = z[:na], z[na:]
        return xa, xb

    def neg(z):
        xa, xb = split(z)
        return -(a.F_at(xa) + b.F_at(xb))
    con = np.concatenate([a.is_member[live_a].astype(float), -ratio * b.is_member[live_b].astype(float)])
    xa0, _, Fa = a.solve(0.0)
    xb0, _, Fb = b.solve(0.0)
    z0 = np.concatenate([xa0[live_a], xb0[live_b]])
    res = opt.minimize(neg, z0, method="SLSQP", bounds=[(1e-9, None)] * len(z0), constraints=[dict(type="eq", fun=lambda z: float(con @ z), jac=lambda z: con)],
                       options=dict(ftol=1e-15, maxiter=500))
    lam_slsqp = 2.0 * (Fa + Fb + res.fun)
    ref = GP.reference(prob, RA, RB, members, ratio, den_a, den_b)
    print(lam_slsqp, ref["lam"], ref["w_ref"], res.message, abs(float(con @ res.x)))
    assert res.success and abs(float(con @ res.x)) <= 1e-9
    assert ref["w_ref"] <= W_REF_MAX and abs(ref["lam"] - lam_slsqp) <= ref["w_ref"] + 1e-7


def test_writer_byte_for_byte(tmp_path):
    """.gcompare (emsar_write_gcompare): three genes, one with an empty name, written three times -- every status and two outside the range,
    and nan, +inf and -inf in each of the five number columns; the sign of an infinity is printed"""
    from emsar_amd import _build, hostlib
    _build.build_all()
    nan, inf = float("nan"), float("inf")
    genes = ["g1", "", "g3"]
    head = b"gene\tgFPKM\tgFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\tparts\n"
    p = str(tmp_path / "a.gcompare")
    hostlib.write_gcompare(p, genes, [1.5, nan, inf], [0.75, nan, inf], [1.0, nan, inf], [3.25, nan, inf], [0.0714, nan, inf], [0, 1, 2], [12, 0, 1], [2, 0, 64])
    assert open(p, "rb").read() == head + (b"g1\t1.500000\t0.750000\t1.000000\t3.250000\t0.0714\tTESTED\t12\t2\n"
                                           b"\tnan\tnan\tnan\tnan\tnan\tBOTH_ABSENT\t0\t0\n"
                                           b"g3\tinf\tinf\tinf\tinf\tinf\tOUTSIDE\t1\t64\n")
    hostlib.write_gcompare(p, genes, [-inf, 0.0, 2.25], [-inf, 4.5, 0.0], [-inf, -2.5, 0.5], [-inf, 0.0, 10.0], [-inf, 1.0, 1e-300], [3, 4, 5], [40, 7, 3], [1, 3, 65])
    assert open(p, "rb").read() == head + (b"g1\t-inf\t-inf\t-inf\t-inf\t-inf\tNOT_RESIDENT\t40\t1\n"
                                           b"\t0.000000\t4.500000\t-2.500000\t0.000000\t1\tUNCONVERGED\t7\t3\n"
                                           b"g3\t2.250000\t0.000000\t0.500000\t10.000000\t1e-300\tTOO_LARGE\t3\t65\n")
    hostlib.write_gcompare(p, genes, [1e-7, 1.0, 2.0], [12345678.5, 1.0, 2.0], [-4e-7, 0.0, 0.0], [0.125, 0.0, 0.0], [0.123456789, 1.0, 1.0], [6, -1, 7], [2, 1, 1],
                           [2, 1, 1])
    assert open(p, "rb").read() == head + (b"g1\t0.000000\t12345678.500000\t-0.000000\t0.125000\t0.123457\t?\t2\t2\n"
                                           b"\t1.000000\t1.000000\t0.000000\t0.000000\t1\t?\t1\t1\n"
                                           b"g3\t2.000000\t2.000000\t0.000000\t0.000000\t1\t?\t1\t1\n")
