"""CPU: what the gene-level profile intervals (include/emsar_hip.h "gene-level profile intervals") compute without a device -- the
independent reference of tests/profile_gene_problems.py against analytic cases, the host's search of genes whose parts are all closed
form (emsar_hip_debug_profile_genes_closed), the end-of-range rule, the p-value bound and the sizes of the new structs."""
import ctypes as C
import math

import numpy as np
import pytest

from emsar_amd import hip as H
from tests import compare_problems as CP
from tests import profile_gene_problems as PG

TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE = range(6)
DEV_TOL = 1e-4


def q_of(level):
    return H.profile_cut_host(level)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_analytic_gene():
    """rows {a}: 30, {a, b}: 50, gene {a, b}: D(x) = 2 (50 log(50 / x) - (50 - x)) for x >= 30, to 1e-13 of |F_hat| + |F_pinned|"""
    prob, R, members = PG.analytic_problem()
    g = PG.Gene(prob, R, members)
    assert g.n_parts == 1 and g.members == 2
    xh, F_hat, _ = g.em()
    X_hat, F_want = PG.analytic_fit()
    assert abs(float(xh[g.is_member].sum()) - X_hat) <= 1e-10 and abs(F_hat - F_want) <= 1e-12 * abs(F_want)
    for x in (31.0, 37.5, 50.0, 64.0, 90.0):
        D, F = g.deviance(x, F_hat)
        print(x, D, float(PG.analytic_D(x)))
        assert abs(D - float(PG.analytic_D(x))) <= 1e-13 * (abs(F_hat) + abs(F))
    _, F_drop, _ = g.em(pin=0.0)
    assert F_drop == -math.inf                                # a has reads of its own: the gene is essential


def test_reference_on_lone_transcripts():
    """two one-transcript components in one gene: the pinned EM against the closed form x_i = u_i / (den_i + lam)"""
    n_tx, rp, ci = CP.csr([[0], [1]], 2)
    R = np.array([30, 20], dtype=np.int32)
    E = np.array([2.0, 3.0])
    g = PG.Gene((n_tx, rp, ci, R, E), R, [0, 1])
    assert g.n_parts == 2
    _, F_hat, _ = g.em()
    q = q_of(0.95)
    lower, upper, X_hat = PG.closed_limits([30, 20], [2.0, 3.0], q)
    for x in (lower, upper):
        D, F = g.deviance(x, F_hat)
        assert abs(D - q) <= 1e-12 * (abs(F_hat) + abs(F)), (x, D)


def test_pinned_mstep_meets_its_constraint():
    rng = np.random.default_rng(1)
    for _ in range(20):
        k = int(rng.integers(1, 6))
        n, den, x = rng.uniform(0.0, 50.0, k), rng.uniform(0.5, 4.0, k), float(rng.uniform(0.1, 100.0))
        n[rng.integers(0, k)] += 1.0
        y = PG.pinned_mstep(list(n), list(den), x)
        assert abs(sum(y) - x) <= 1e-12 * x and min(y) >= 0.0
    assert PG.pinned_mstep([3.0, 4.0], [1.0, 2.0], 0.0) == [0.0, 0.0]


# ---- the host's search: genes whose parts are all closed form --------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.95, 0.99])
def test_closed_gene_against_a_scalar_root_find(level):
    q = q_of(level)
    u, den = [30.0, 20.0, 7.0], [2.0, 3.0, 0.75]
    r = H.debug_profile_genes_closed(u, den, level=level)
    lower, upper, X_hat = PG.closed_limits(u, den, q)
    print(r, lower, upper)
    assert r["status"] == TWO_SIDED and math.isinf(r["lambda"]) and r["pvalue"] == 0.0
    assert abs(r["gene_hat"] - X_hat) <= 1e-14 * X_hat
    assert abs(r["dev_lower"] - q) <= DEV_TOL * q and abs(r["dev_upper"] - q) <= DEV_TOL * q
    # both lie within dev_tol q of the cut and the slope of D at a limit is about 2 q / half-width
    assert abs(r["lower"] - lower) <= DEV_TOL * (X_hat - lower) and abs(r["upper"] - upper) <= DEV_TOL * (upper - X_hat)
    assert r["lower"] < r["gene_hat"] < r["upper"] and 2 <= r["evals"] <= 80


def test_end_of_range_rule():
    """a zero-read lone member with the strictly smallest den next to a member with 40 reads: one evaluation at s = 0, then the line"""
    q = q_of(0.95)
    r = H.debug_profile_genes_closed([0.0, 40.0], [1.0, 30.0])
    x_hat, x_end = 40.0 / 30.0, 40.0 / 29.0
    F = lambda x: 40.0 * math.log(x) - 30.0 * x
    D_end = 2.0 * (F(x_hat) - F(x_end))
    assert D_end < q
    assert r["evals_upper"] == 1 and r["dev_upper"] == q and r["evals"] > 2
    assert abs(r["upper"] - (x_end + (q - D_end) / 2.0)) <= 1e-12 * r["upper"]
    assert r["status"] == TWO_SIDED and abs(r["dev_lower"] - q) <= DEV_TOL * q and r["gene_hat"] == x_hat
    lone = H.debug_profile_genes_closed([40.0], [30.0])
    # the end lies beyond the cut (at s = 0 the member with reads has den 1: D_end >= q): the ordinary search runs and lands on the cut
    far = H.debug_profile_genes_closed([0.0, 40.0], [29.0, 30.0])
    assert 2.0 * (F(x_hat) - F(40.0 / 1.0)) > q
    assert far["evals_upper"] > 1 and abs(far["dev_upper"] - q) <= DEV_TOL * q
    assert abs(far["upper"] - lone["upper"]) <= 2 * DEV_TOL * (lone["upper"] - x_hat)        # short of the end the zero-read member adds nothing
    # tied dens: no reachable end, the ordinary search
    tied = H.debug_profile_genes_closed([0.0, 40.0], [30.0, 30.0])
    assert tied["evals_upper"] > 1 and abs(tied["dev_upper"] - q) <= DEV_TOL * q
    assert tied["upper"] == lone["upper"] and tied["lower"] == lone["lower"]                 # the same path, point for point
    # a zero-read member that is not the smallest: the member with reads is, and the ordinary search brackets
    above = H.debug_profile_genes_closed([0.0, 40.0], [31.0, 30.0])
    assert above["evals_upper"] > 1 and above["upper"] == lone["upper"]


def test_gene_without_reads():
    q = q_of(0.95)
    r = H.debug_profile_genes_closed([0.0, 0.0, 0.0], [3.0, 2.0, 5.0])
    assert r["status"] == LOWER_ZERO and r["lambda"] == 0.0 and r["pvalue"] == 1.0 and r["evals"] == 0
    assert r["lower"] == 0.0 and r["dev_lower"] == 0.0 and r["upper"] == q / (2.0 * 2.0) and r["dev_upper"] == q and r["gene_hat"] == 0.0


def test_closed_unconverged_and_errors():
    r = H.debug_profile_genes_closed([30.0, 20.0], [2.0, 3.0], max_evals=1)
    assert r["status"] == UNCONVERGED and r["evals"] == 2
    r = H.debug_profile_genes_closed([0.0, 40.0], [29.0, 30.0], max_evals=1)          # the end evaluation is the one evaluation
    assert r["status"] == UNCONVERGED
    for bad in (dict(level=0.0), dict(level=1.0), dict(level=math.nan), dict(dev_tol=math.inf)):
        with pytest.raises(H.EmsarHipError) as e:
            H.debug_profile_genes_closed([1.0], [1.0], **bad)
        assert e.value.status == -1
    for u, den in (([-1.0], [1.0]), ([1.0], [0.0]), ([math.nan], [1.0])):
        with pytest.raises(H.EmsarHipError):
            H.debug_profile_genes_closed(u, den)


# ---- the p-value bound -----------------------------------------------------------------------------------------------------------
def test_pvalue_closed_forms():
    lam = np.array([1e-6, 0.3, 1.0, 3.841458820694124, 10.0, 50.0, 400.0, 1400.0, 1600.0])
    x = lam / 2
    p1, p2, p4 = (H.gene_presence_pvalue_host(lam, k) for k in (1, 2, 4))
    for i in range(len(lam)):
        assert abs(p1[i] - math.erfc(math.sqrt(x[i]))) <= 4e-16 * p1[i] + 1e-320
        assert abs(p2[i] - math.exp(-x[i])) <= 1e-13 * p2[i] + 1e-320
        assert abs(p4[i] - math.exp(-x[i]) * (1.0 + x[i])) <= 1e-13 * p4[i] + 1e-320
    p3 = H.gene_presence_pvalue_host(lam, 3)
    for i in range(len(lam)):
        want = math.erfc(math.sqrt(x[i])) + 2.0 * math.sqrt(x[i] / math.pi) * math.exp(-x[i])
        assert abs(p3[i] - want) <= 1e-13 * want + 1e-320
    assert abs(H.gene_presence_pvalue_host([3.841458820694124], [1])[0] - 0.05) <= 1e-12


def test_pvalue_monotone_in_k_and_special_values():
    lam = np.array([0.1, 2.0, 9.0, 60.0, 1500.0])
    prev = np.zeros(len(lam))
    for k in range(1, 40):
        p = H.gene_presence_pvalue_host(lam, k)
        # up to the rounding of a sum of at most 20 terms: at Lambda = 0.1 the odd and the even formula both round to about 1
        assert np.all(p >= prev * (1.0 - 1e-14)) and np.all(p <= 1.0) and np.all(p >= 0.0), k
        if k <= 8:                                            # beyond, p at Lambda = 0.1 rounds to 1
            assert np.all(p[:4] > prev[:4]), k
        prev = p
    big = H.gene_presence_pvalue_host([50.0], [5000])
    assert big[0] == 1.0 or abs(big[0] - 1.0) <= 1e-12
    p = H.gene_presence_pvalue_host([0.0, -1.0, math.inf, math.nan, 3.0, 3.0], [3, 3, 3, 3, 0, -2])
    assert p[0] == 1.0 and p[1] == 1.0 and p[2] == 0.0 and math.isnan(p[3]) and math.isnan(p[4]) and math.isnan(p[5])
    assert len(H.gene_presence_pvalue_host([], [])) == 0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_sizes():
    assert C.sizeof(H.ProfileGeneOutputs) == 11 * 8
    assert C.sizeof(H.ProfileGeneStats) == 6 * 8 + 3 * 8 + 4 * 4 + 5 * 8 == 128
    assert H.ProfileGeneStats.cut.offset == 96 and H.ProfileGeneStats.total_ms.offset == 120
    assert H.PROFILE_GENE_STATUS == ("TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE")
    assert "emsar_hip_profile_genes" in H.SYMBOLS and "emsar_hip_gene_presence_pvalue_host" in H.SYMBOLS


# ---- the .gprofile file --------------------------------------------------------------------------------------------------------------
def test_writer_byte_for_byte(tmp_path):
    """.gprofile (emsar_write_gprofile): three genes, one with an empty name, written three times -- every status and two outside the range,
    and nan, +inf and -inf in each of the four columns that can carry them (gFPKM is a sum of printed FPKM); the sign of an infinity is
    printed"""
    from emsar_amd import _build, hostlib
    _build.build_all()
    nan, inf = float("nan"), float("inf")
    genes = ["g1", "", "g3"]
    head = b"gene\tgFPKM\tlower\tupper\tLambda\tp\tmembers\tstatus\n"
    p = str(tmp_path / "a.gprofile")
    hostlib.write_gprofile(p, genes, [1.5, 0.0, 9.0], [0.75, nan, inf], [2.25, nan, inf], [3.25, nan, inf], [0.0714, nan, inf], [3, 0, 1], [0, 1, 2])
    assert open(p, "rb").read() == head + (b"g1\t1.500000\t0.750000\t2.250000\t3.250000\t0.0714\t3\tTWO_SIDED\n"
                                           b"\t0.000000\tnan\tnan\tnan\tnan\t0\tLOWER_ZERO\n"
                                           b"g3\t9.000000\tinf\tinf\tinf\tinf\t1\tOUTSIDE\n")
    hostlib.write_gprofile(p, genes, [1e-7, 4.5, 12345678.5], [-inf, 0.0, 1.0], [-inf, 6.5, 2.0], [-inf, 0.0, 10.0], [-inf, 1.0, 1e-300], [2, 64, 65], [3, 4, 5])
    assert open(p, "rb").read() == head + (b"g1\t0.000000\t-inf\t-inf\t-inf\t-inf\t2\tNOT_RESIDENT\n"
                                           b"\t4.500000\t0.000000\t6.500000\t0.000000\t1\t64\tUNCONVERGED\n"
                                           b"g3\t12345678.500000\t1.000000\t2.000000\t10.000000\t1e-300\t65\tTOO_LARGE\n")
    hostlib.write_gprofile(p, genes, [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [2.0, 2.0, 2.0], [0.125, 0.125, 0.125], [0.123456789, 1.0, 1.0], [1, 1, 1], [6, -1, 0])
    assert open(p, "rb").read() == head + (b"g1\t1.000000\t0.500000\t2.000000\t0.125000\t0.123457\t1\t?\n"
                                           b"\t1.000000\t0.500000\t2.000000\t0.125000\t1\t1\t?\n"
                                           b"g3\t1.000000\t0.500000\t2.000000\t0.125000\t1\t1\tTWO_SIDED\n")
