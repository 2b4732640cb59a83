"""CPU: what the two-sample test (include/emsar_hip.h "two-sample test") defines on the host -- the chi2_1 p-value, the ABI's structs and
names, the argument checks that need no device, the multiplier search on a pair of one-transcript components against the closed-form
answer, the numpy reference of tests/compare_problems.py against that same closed form, and the generated code of the new kernels."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from emsar_amd import _build
from emsar_amd import hip as H
from tests import compare_problems as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_TOL = 1e-4          # the default of emsar_compare_params.dev_tol


@pytest.fixture(scope="module", autouse=True)
def _built():
    _build.build_all()


def test_pvalue_helper():
    lam = np.array([0.0, -1.0, -0.0, math.inf, math.nan, 1e-12, 0.5, 1.0, 3.841458820694124, 10.0, 50.0, 1400.0])
    p = H.compare_pvalue_host(lam)
    assert p[0] == 1.0 and p[1] == 1.0 and p[2] == 1.0 and p[3] == 0.0 and math.isnan(p[4])
    for x, got in zip(lam[5:], p[5:]):
        want = math.erfc(math.sqrt(x / 2.0))
        assert abs(got - want) <= 4e-16 * want + 1e-300, (x, got, want)
    assert abs(p[8] - 0.05) <= 1e-12
    assert H.compare_pvalue_host(0.0) == 1.0 and H.compare_pvalue_host(math.inf) == 0.0
    # twice the presence test's boundary-mixture value
    assert H.compare_pvalue_host(2.5) == 2.0 * H.presence_pvalue_host(2.5)
    L = H.load_library()
    assert L.emsar_hip_compare_pvalue_host(-1, None, None) == -1
    assert L.emsar_hip_compare_pvalue_host(2, None, None) == -1
    assert L.emsar_hip_compare_pvalue_host(0, None, None) == 0


def test_abi_structs_and_names():
    L = H.load_library()
    for name in ("emsar_hip_compare", "emsar_hip_compare_pvalue_host"):
        assert name in H.SYMBOLS and hasattr(L, name)
    assert C.sizeof(H.CompareParams) == 8 + 8 + 4 + 4
    assert C.sizeof(H.CompareOutputs) == 11 * C.sizeof(C.c_void_p)
    assert C.sizeof(H.CompareStats) == 8 * 5 + 8 * 3 + 4 * 2 + 8 * 3
    text = open(os.path.join(ROOT, "include", "emsar_hip.h")).read()
    enum = dict(re.findall(r"EMSAR_COMPARE_([A-Z_]+) = (\d)", text))
    assert [k for k, _ in sorted(enum.items(), key=lambda kv: int(kv[1]))] == list(H.COMPARE_STATUS)
    assert list(H.COMPARE_STATUS) == ["TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED"]
    for struct, mirror in (("emsar_compare_params", H.CompareParams), ("emsar_compare_outputs", H.CompareOutputs),
                           ("emsar_compare_stats", H.CompareStats)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if f.strip()]
        fields = [re.sub(r"\[\d+\]", "", f) for f in fields]
        assert fields == [k.rstrip("_") for k, _ in mirror._fields_], struct
    assert [k.rstrip("_") for k, _ in H.CompareOutputs._fields_][:9] == list(H.COMPARE_OUTPUTS)
    assert "CONSERVATIVE" in text[text.index("two-sample test"):text.index("EMSAR_COMPARE_TESTED")]


def test_argument_checks_without_a_device():
    """no context, one context twice: ERR_ARG before anything else; without a GPU no context can be made, so there is no host path"""
    import torch

    import emsar_amd
    L = H.load_library()
    assert L.emsar_hip_compare(None, None, None, None, 0, None, None, None) == -1
    fake = C.c_void_p(16)
    assert L.emsar_hip_compare(fake, None, None, None, 0, None, None, None) == -1
    assert L.emsar_hip_compare(None, fake, None, None, 0, None, None, None) == -1
    assert L.emsar_hip_compare(fake, fake, None, None, 0, None, None, None) == -1       # the same context twice: not looked into
    if not torch.cuda.is_available():
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            emsar_amd.EmsarHip(0)
        assert e.value.status == -2
    for bad in (dict(ratio=-1.0), dict(ratio=math.nan), dict(ratio=math.inf), dict(dev_tol=math.inf), dict(dev_tol=math.nan)):
        with pytest.raises(H.EmsarHipError) as e:
            H.debug_compare_closed(10, 1.0, 20, 1.0, **bad)
        assert e.value.status == -1, bad
    for bad in ((-1, 1.0, 2, 1.0), (1, 0.0, 2, 1.0), (1, 1.0, 2, math.nan)):
        with pytest.raises(H.EmsarHipError):
            H.debug_compare_closed(*bad)


CLOSED = [(40, 2.0, 55, 2.0, 1.0), (100, 1.5, 30, 0.7, 1.0), (30, 1.0, 0, 1.0, 1.0), (0, 1.0, 12, 3.0, 1.0), (25, 1.0, 50, 1.0, 0.5),
          (25, 1.0, 50, 1.0, 2.0), (25, 1.0, 61, 1.0, 0.5), (7, 0.3, 900, 4.0, 1.7), (100000, 1.0, 100500, 1.0, 1.0), (3, 2.0, 1, 5.0, 0.25)]


@pytest.mark.parametrize("u_a,d_a,u_b,d_b,ratio", CLOSED)
def test_closed_pair_search_against_the_closed_form(u_a, d_a, u_b, d_b, ratio):
    """two singletons: the null MLE is x = (u_A + u_B) / (d_A + d_B / r) on the A scale; Lambda in one line of numpy.  The reported dual
    value lies below the statistic by at most the stopping rule's dev_tol (plus the rounding of four F values of this size)"""
    want, x_null = CP.closed_pair_lambda(u_a, d_a, u_b, d_b, ratio)
    r = H.debug_compare_closed(u_a, d_a, u_b, d_b, ratio=ratio)
    eps = 8 * 2.3e-16 * (abs(u_a * math.log(max(u_a / d_a, 1e-300))) + abs(u_b * math.log(max(u_b / d_b, 1e-300))) + u_a + u_b + 1)
    print(r, want, x_null)
    assert r["status"] == 0 and (1 if want == 0.0 else 2) <= r["evals"] <= 40
    assert r["theta_a"] == u_a / d_a and r["theta_b"] == u_b / d_b
    assert want - DEV_TOL - eps <= r["lambda"] <= want + eps, (r["lambda"], want)
    assert r["raw_lambda"] == r["lambda"] or (r["raw_lambda"] < 0 and r["lambda"] == 0.0)
    if u_a > 0:                                                  # the last x_A; without a read of t in A it stays 0 (the null value is r x_B then)
        assert abs(r["theta_null"] - x_null) <= 1e-3 * x_null
    assert r["pvalue"] == H.compare_pvalue_host(r["lambda"])
    if u_a > 0 and u_b > 0:
        assert abs(r["log2fc"] - math.log2((u_a / d_a) / (ratio * u_b / d_b))) <= 1e-12
    else:
        assert r["log2fc"] == (math.inf if u_b == 0 else -math.inf)
    # a tighter rule tightens it
    tight = H.debug_compare_closed(u_a, d_a, u_b, d_b, ratio=ratio, dev_tol=1e-9, max_evals=60)
    assert tight["status"] == 0 and want - 1e-9 - eps <= tight["lambda"] <= want + eps, (tight, want)


def test_closed_pair_special_cases():
    same = H.debug_compare_closed(40, 2.0, 40, 2.0)
    assert same["lambda"] == 0.0 and same["raw_lambda"] == 0.0 and same["evals"] == 1 and same["status"] == 0 and same["pvalue"] == 1.0
    assert same["multiplier"] == 0.0 and same["gap"] == 0.0 and same["log2fc"] == 0.0
    scaled = H.debug_compare_closed(40, 2.0, 80, 2.0, ratio=0.5)          # a size factor: twice the reads, tested at r = 1/2
    assert scaled["lambda"] == 0.0 and scaled["evals"] == 1
    none = H.debug_compare_closed(0, 2.0, 0, 1.0)
    assert none["status"] == 1 and none["lambda"] == 0.0 and none["pvalue"] == 1.0 and none["evals"] == 1 and math.isnan(none["log2fc"])
    capped = H.debug_compare_closed(40, 2.0, 55, 2.0, max_evals=1)
    assert capped["status"] == 4 and capped["evals"] == 1 and capped["lambda"] == 0.0 and capped["theta_a"] == 20.0 and capped["theta_b"] == 27.5
    capped = H.debug_compare_closed(40, 2.0, 55, 2.0, max_evals=2)
    assert capped["status"] == 4 and capped["evals"] == 2 and np.isfinite(capped["lambda"])
    # a ratio of 0 is the default 1
    assert H.debug_compare_closed(40, 2.0, 55, 2.0, ratio=0.0) == H.debug_compare_closed(40, 2.0, 55, 2.0, ratio=1.0)
    # swapping the samples at 1 / r: the same statistic within the two stopping rules, log2fc negated
    a, b = H.debug_compare_closed(25, 1.0, 50, 3.0, ratio=2.0), H.debug_compare_closed(50, 3.0, 25, 1.0, ratio=0.5)
    assert abs(a["lambda"] - b["lambda"]) <= 2 * DEV_TOL and abs(a["log2fc"] + b["log2fc"]) <= 1e-15


def test_closed_pair_search_point_by_point():
    """(40 reads, den 2) against (55, 2) capped after 1, 2 and 3 evaluations: the points of the search, which kernel and host take from
    one step function.  Plain arithmetic, no libm call enters these three fields: the first point is v = (7.5 / 47.5) / (1 + 7.5 / 47.5)
    = 3 / 22 of lambda_end = -den_A, multiplier -3 / 11; the values are those of the build before the step was shared."""
    want = {1: ("0x0.0p+0", "0x1.4000000000000p+4", "-0x1.e000000000000p+2"),
            2: ("-0x1.1745d1745d174p-2", "0x1.7286bca1af287p+4", "-0x1.0ac7691840ad0p+0"),
            3: ("-0x1.3d5af9a723f79p-2", "0x1.7aae0140782d1p+4", "-0x1.24a59d21cb400p-3")}
    for max_evals, bits in want.items():
        r = H.debug_compare_closed(40, 2.0, 55, 2.0, max_evals=max_evals)
        assert r["evals"] == max_evals and r["status"] == 4
        assert tuple(float(r[k]).hex() for k in ("multiplier", "theta_null", "gap")) == bits, (max_evals, r)
        assert r["theta_a"] == 20.0 and r["theta_b"] == 27.5
    assert abs(float.fromhex(want[2][0]) + 3.0 / 11.0) <= 1e-16


def test_the_numpy_reference_agrees_with_the_closed_form():
    """the stacked EM of tests/compare_problems.py on two singletons, and on the hand-made problem's closed-form pair"""
    prob, RA, RB, den_a, den_b = CP.small_problem()
    for t in (0, 1):
        for ratio in (1.0, 0.5, 3.0):
            ref = CP.reference(prob, RA, RB, t, ratio, den_a, den_b)
            want, x = CP.closed_pair_lambda(float(RA[t]), den_a[t], float(RB[t]), den_b[t], ratio)
            assert abs(ref["lam"] - want) <= 1e-10 * max(1.0, want), (t, ratio, ref["lam"], want)
            assert abs(ref["theta_null"] - x) <= 1e-10 * x
    ref = CP.reference(prob, RA, RB, 1, 1.0, den_a, den_b)
    assert abs(ref["lam"]) <= 1e-10                              # 25 reads over den 1 in both samples
    # a family: Lambda >= 0 and the null value lies between the two free estimates
    ref = CP.reference(prob, RA, RB, 4, 1.0, den_a, den_b)
    assert ref["lam"] >= -1e-10 and min(ref["theta_a"], ref["theta_b"]) <= ref["theta_null"] <= max(ref["theta_a"], ref["theta_b"])


def test_compare_kernels_use_no_scratch():
    """the ISA listing of the build (absent where build/ is not shipped): the three k_compare_sets instantiations use no scratch memory
    and spill no vector register"""
    asm = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        pytest.skip("no ISA listing (build/ is not shipped)")
    meta = {}
    for blk in open(asm).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    for threads in (64, 256, 512):
        names = [n for n in meta if n and "k_compare_setsILi%dE" % threads in n]
        assert len(names) == 1, (threads, names)
        print(names[0], meta[names[0]])
        assert meta[names[0]]["vgpr_spill_count"] == 0 and meta[names[0]]["private_segment_fixed_size"] == 0, (names[0], meta[names[0]])


def test_writer_byte_for_byte(tmp_path):
    """.compare (emsar_write_compare): a query list out of order with repeats, every status and two outside the range, and nan, +inf and -inf
    in each of the five number columns -- the sign of an infinity is printed"""
    from emsar_amd import hostlib
    _build.build_all()
    nan, inf = float("nan"), float("inf")
    p = str(tmp_path / "a.compare")
    hostlib.write_compare(p, ["tA", "tB", "tC", "tD", "tE"],
                          [1.5, nan, inf, -inf, 0.0, 2.25, 1e-7], [0.75, nan, inf, -inf, 4.5, 0.0, 12345678.5], [1.0, nan, inf, -inf, -2.5, 0.5, -4e-7],
                          [3.25, nan, inf, -inf, 0.0, 10.0, 0.125], [0.0714, nan, inf, -inf, 1.0, 1e-300, 0.123456789], [0, 1, 2, 3, 4, 5, -1],
                          [12, 0, 1, 40, 7, 3, 2], query=[3, 0, 4, 0, 1, 2, 4])
    assert open(p, "rb").read() == (b"tid\ttranscriptID\tFPKM\tFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\n"
                                    b"3\ttD\t1.500000\t0.750000\t1.000000\t3.250000\t0.0714\tTESTED\t12\n"
                                    b"0\ttA\tnan\tnan\tnan\tnan\tnan\tBOTH_ABSENT\t0\n"
                                    b"4\ttE\tinf\tinf\tinf\tinf\tinf\tOUTSIDE\t1\n"
                                    b"0\ttA\t-inf\t-inf\t-inf\t-inf\t-inf\tNOT_RESIDENT\t40\n"
                                    b"1\ttB\t0.000000\t4.500000\t-2.500000\t0.000000\t1\tUNCONVERGED\t7\n"
                                    b"2\ttC\t2.250000\t0.000000\t0.500000\t10.000000\t1e-300\t?\t3\n"
                                    b"4\ttE\t0.000000\t12345678.500000\t-0.000000\t0.125000\t0.123457\t?\t2\n")
    hostlib.write_compare(p, ["tA", "tB"], [1.0, 2.0], [3.0, 4.0], [-1.5, -1.0], [0.5, 0.25], [0.5, 0.625], [0, 4], [9, 8])          # no query: all, in order
    assert open(p, "rb").read() == (b"tid\ttranscriptID\tFPKM\tFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\n"
                                    b"0\ttA\t1.000000\t3.000000\t-1.500000\t0.500000\t0.5\tTESTED\t9\n"
                                    b"1\ttB\t2.000000\t4.000000\t-1.000000\t0.250000\t0.625\tUNCONVERGED\t8\n")
