"""CPU: the profile-likelihood intervals of isoform usage (emsar_hip_profile_usage, include/emsar_hip.h "profile-likelihood intervals of
isoform usage") where no device is needed: the host's search on genes of one-transcript components through the diagnostic entry, against
the analytic curve of a gene of two lone transcripts; the host's statuses and argument checks; the .uprofile writer; the command line's
messages.

A gene of two lone transcripts t, s with u_t, u_s reads and den d_t, d_s: under theta_t = o theta_s (o = u / (1 - u)) the maximum is at
theta_s = n / (o d_t + d_s), n = u_t + u_s, so  D(u) = 2 (F_hat - u_t ln o - n ln(n / (o d_t + d_s)) + n),  F_hat = sum u ln(u / d) - n.
The device code reports the dual value of an inner search, a lower bound of D whose error the inner rule keeps below the outer one:
|D(limit) - q| <= dev_tol q + 1e-9 is asked of the analytic curve at the reported limit."""
import math
import os
import subprocess

import numpy as np
import pytest

import emsar_amd
from emsar_amd import _build
from emsar_amd import hip as H

Q95 = 3.841458820694124
TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED, TOO_LARGE, UPPER_ONE, UNIT, UNDEFINED, SINGLE = range(10)


def curve(u_t, u_s, d_t, d_s):
    n = u_t + u_s
    F_hat = sum(a * math.log(a / d) for a, d in ((u_t, d_t), (u_s, d_s)) if a > 0) - n

    def D(u):
        o = u / (1.0 - u)
        return 2.0 * (F_hat - (u_t * math.log(o) if u_t > 0 else 0.0) - n * math.log(n / (o * d_t + d_s)) + n)
    return D


def test_symbols_and_tables():
    L = emsar_amd.load_library()
    assert hasattr(L, "emsar_hip_profile_usage") and hasattr(L, "emsar_hip_debug_profile_usage_closed")
    assert "emsar_hip_profile_usage" in H.SYMBOLS
    assert H.PROFILE_USAGE_STATUS == ("TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE", "UPPER_ONE", "UNIT", "UNDEFINED",
                                      "SINGLE")
    assert H.PROFILE_USAGE_OUTPUTS == ("usage", "lower", "upper", "dev_lower", "dev_upper", "lambda_zero", "lambda_one")
    assert H.PROFILE_USAGE_COUNTS == ("status", "outer_evals", "evals", "parts", "members")
    cut = H.profile_cut_host(0.95)
    assert abs(cut - Q95) <= 1e-14


@pytest.mark.parametrize("u_t,u_s,d_t,d_s", [(30, 50, 1.0, 2.0), (3, 500, 1.0, 2.0), (500, 3, 0.25, 7.0), (1, 1, 1.0, 1.0), (40000, 90000, 3.0, 0.5)])
@pytest.mark.parametrize("dev_tol", [1e-4, 1e-8])
def test_lone_pair_against_the_analytic_curve(u_t, u_s, d_t, d_s, dev_tol):
    D = curve(u_t, u_s, d_t, d_s)
    for t, (ut, us, dt, ds) in enumerate(((u_t, u_s, d_t, d_s), (u_s, u_t, d_s, d_t))):
        r = H.debug_profile_usage_closed([u_t, u_s], [d_t, d_s], t=t, dev_tol=dev_tol)
        Dt = curve(ut, us, dt, ds)
        print(t, r, Dt(r["lower"]) - Q95, Dt(r["upper"]) - Q95)
        assert r["status"] == TWO_SIDED and r["parts"] == r["members"] == 2
        assert abs(r["usage"] - (ut / dt) / (ut / dt + us / ds)) <= 1e-15 and 0.0 < r["lower"] < r["usage"] < r["upper"] < 1.0
        assert r["lambda_zero"] == math.inf and r["lambda_one"] == math.inf             # both have reads only they explain
        for lim, dev in ((r["lower"], r["dev_lower"]), (r["upper"], r["dev_upper"])):
            assert abs(Dt(lim) - Q95) <= dev_tol * Q95 + 1e-9 and abs(dev - Q95) <= dev_tol * Q95
            assert dev <= Dt(lim) + 1e-9                                                 # the dual value: a lower bound of D
        assert 2 <= r["outer_evals"] <= 2 * 24 and r["evals"] >= r["outer_evals"]
    # the two members of a two-member gene mirror each other
    a, b = (H.debug_profile_usage_closed([u_t, u_s], [d_t, d_s], t=t, dev_tol=1e-10) for t in (0, 1))
    slope = abs(D(a["upper"] + 1e-7) - D(a["upper"] - 1e-7)) / 2e-7
    assert abs(a["lower"] + b["upper"] - 1.0) * slope <= 1e-6 and abs(a["upper"] + b["lower"] - 1.0) * slope <= 1e-6


@pytest.mark.parametrize("u_s,d_t,d_s", [(50, 1.0, 2.0), (7, 3.0, 0.5), (100000, 1.0, 1.0)])
def test_no_reads_of_its_own(u_s, d_t, d_s):
    """u_t = 0: usage 0, LOWER_ZERO, and the upper limit in closed form: o* = (d_s / d_t) (exp(q / 2n) - 1); the sibling's interval is
    its mirror image with UPPER_ONE"""
    r = H.debug_profile_usage_closed([0, u_s], [d_t, d_s], t=0)
    o = (d_s / d_t) * math.expm1(Q95 / (2.0 * u_s))
    want = o / (1.0 + o)
    D = curve(0, u_s, d_t, d_s)
    print(r, want, D(r["upper"]) - Q95)
    assert r["status"] == LOWER_ZERO and r["usage"] == 0.0 and r["lower"] == 0.0 and r["dev_lower"] == 0.0 and r["lambda_zero"] == 0.0
    assert r["lambda_one"] == math.inf and abs(D(r["upper"]) - Q95) <= 1e-4 * Q95 + 1e-9
    slope = 2.0 * u_s * d_t / d_s                            # dD/du at 0, and D is convex: a lower bound of the slope at the limit
    assert abs(r["upper"] - want) * slope <= 1e-4 * Q95 + 1e-9
    s = H.debug_profile_usage_closed([0, u_s], [d_t, d_s], t=1)
    assert s["status"] == UPPER_ONE and s["usage"] == 1.0 and s["upper"] == 1.0 and s["dev_upper"] == 0.0 and s["lambda_one"] == 0.0
    assert s["lambda_zero"] == math.inf and abs((1.0 - s["lower"]) - want) * slope <= 1e-4 * Q95 + 1e-9


def test_host_statuses_and_arguments():
    nan_out = lambda r: all(math.isnan(r[k]) for k in H.PROFILE_USAGE_OUTPUTS)
    zero_counts = lambda r: r["outer_evals"] == r["evals"] == r["parts"] == r["members"] == 0
    r = H.debug_profile_usage_closed([3, 5], [0.0, 1.0], t=0)                            # den_t = 0
    assert r["status"] == OUTSIDE and nan_out(r) and zero_counts(r)
    r = H.debug_profile_usage_closed([3, 5], [1.0, 0.0], t=0)                            # the sibling takes no part
    assert r["status"] == SINGLE and nan_out(r) and zero_counts(r)
    r = H.debug_profile_usage_closed([3], [1.0], t=0)
    assert r["status"] == SINGLE and nan_out(r) and zero_counts(r)
    r = H.debug_profile_usage_closed(np.arange(65) + 1, np.ones(65), t=3)
    assert r["status"] == TOO_LARGE and nan_out(r) and zero_counts(r)
    r = H.debug_profile_usage_closed(np.arange(64) + 1, np.ones(64), t=3)
    assert r["status"] == TWO_SIDED and r["parts"] == r["members"] == 64 and r["lower"] < r["usage"] == 4.0 / (64 * 65 / 2) < r["upper"]
    r = H.debug_profile_usage_closed([0, 0, 0], [1.0, 2.0, 3.0], t=1)                    # no reads at all: the gene sum is 0
    assert r["status"] == UNDEFINED and nan_out(r) and r["parts"] == r["members"] == 3 and r["evals"] == 0
    r = H.debug_profile_usage_closed([30, 50, 0], [1.0, 2.0, 0.5], t=0, max_outer=1)
    full = H.debug_profile_usage_closed([30, 50, 0], [1.0, 2.0, 0.5], t=0)
    assert r["status"] == UNCONVERGED and r["outer_evals"] == 2 and r["usage"] == full["usage"] and 0.0 < r["lower"] < r["usage"] < r["upper"] < 1.0
    assert full["status"] == TWO_SIDED and full["members"] == 3
    # a member without reads widens nothing here: it cannot take reads from the others (no shared row)
    pair = H.debug_profile_usage_closed([30, 50], [1.0, 2.0], t=0)
    assert abs(full["lower"] - pair["lower"]) <= 1e-5 and abs(full["upper"] - pair["upper"]) <= 1e-5
    # levels: a higher level is a wider interval
    wide = H.debug_profile_usage_closed([30, 50], [1.0, 2.0], t=0, level=0.99)
    assert wide["lower"] < pair["lower"] and wide["upper"] > pair["upper"]
    for bad in (dict(level=0.0), dict(level=1.0), dict(level=math.nan), dict(dev_tol=math.inf), dict(dev_tol=math.nan), dict(t=2), dict(t=-1)):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            H.debug_profile_usage_closed([30, 50], [1.0, 2.0], **bad)
        assert e.value.status == -1, bad
    for u, den in (([-1, 5], [1.0, 1.0]), ([1, 5], [-1.0, 1.0]), ([math.nan, 5], [1.0, 1.0]), ([1, 5], [math.inf, 1.0])):
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            H.debug_profile_usage_closed(u, den)
        assert e.value.status == -1, (u, den)


def test_writer_byte_for_byte(tmp_path):
    """.uprofile (emsar_write_uprofile): five transcripts, one in no gene (an empty gene field, as for the gene with the empty name), a query
    list out of order with repeats, every status and two outside the range, nan and inf in each of the five number columns"""
    from emsar_amd import hostlib
    _build.build_all()
    nan, inf = float("nan"), float("inf")
    p = str(tmp_path / "a.uprofile")
    n = 12
    status = list(range(10)) + [10, -1]
    query = [3, 0, 4, 0, 1, 2, 4, 2, 1, 0, 3, 3]
    hostlib.write_uprofile(p, ["tA", "tB", "tC", "tD", "tE"], ["g1", "", "g3"], [0, 2, -1, 0, 1],
                           [0.25, nan, inf] + [0.5] * (n - 3), [0.125, nan, inf] + [0.0] * (n - 3), [0.75, nan, inf] + [1.0] * (n - 3),
                           [12.5, nan, inf] + [1e-7] * (n - 3), [inf, nan, inf] + [3.25] * (n - 3), status, list(range(n)), [7 * k for k in range(n)], query=query)
    lines = open(p, "rb").read().split(b"\n")
    assert lines[0] == b"transcript\tgene\tusage\tlower\tupper\tLambda_zero\tLambda_one\tstatus\touter\tevals" and lines[-1] == b"" and len(lines) == n + 2
    assert lines[1] == b"tD\tg1\t0.250000\t0.125000\t0.750000\t12.500000\tinf\tTWO_SIDED\t0\t0"
    assert lines[2] == b"tA\tg1\tnan\tnan\tnan\tnan\tnan\tLOWER_ZERO\t1\t7"
    assert lines[3] == b"tE\t\tinf\tinf\tinf\tinf\tinf\tOUTSIDE\t2\t14"
    assert lines[6] == b"tC\t\t0.500000\t0.000000\t1.000000\t0.000000\t3.250000\tTOO_LARGE\t5\t35"
    words = [l.split(b"\t")[7].decode() for l in lines[1:-1]]
    assert words == list(H.PROFILE_USAGE_STATUS) + ["?", "?"]
    # every transcript in order without a query
    hostlib.write_uprofile(p, ["tA", "tB"], ["g"], [0, 0], [0.5, 0.5], [0.25, 0.0], [0.75, 1.0], [9.0, 0.0], [8.0, 0.5], [0, 7], [4, 0], [20, 0])
    assert open(p, "rb").read() == (b"transcript\tgene\tusage\tlower\tupper\tLambda_zero\tLambda_one\tstatus\touter\tevals\n"
                                    b"tA\tg\t0.500000\t0.250000\t0.750000\t9.000000\t8.000000\tTWO_SIDED\t4\t20\n"
                                    b"tB\tg\t0.500000\t0.000000\t1.000000\t0.000000\t0.500000\tUNIT\t0\t0\n")


PROF_NEEDS = "--profile-list, --profile-level and --profile-evals need --profile."
USAGE_G2T = "--profile-usage needs --g2t FILE."
LEVEL_RANGE = "--profile-level must lie in (0, 1)."
MESSAGES = [
    (["--profile-usage"], USAGE_G2T, True),
    (["--profile", "--profile-usage"], USAGE_G2T, True),
    (["--profile-usage", "--profile-level", "0.9"], USAGE_G2T, True),
    (["--profile-list", "none.list"], PROF_NEEDS, False),                                  # unchanged, byte for byte
    (["--profile-level", "0.9"], PROF_NEEDS, False),
    (["--profile-evals", "30"], PROF_NEEDS, False),
    (["--profile-evals", "30", "--g2t", "none.g2t"], PROF_NEEDS, False),
    (["--profile-usage", "--g2t", "none.g2t", "--profile-level", "2"], LEVEL_RANGE, False),   # accepted with --profile-usage: the range check speaks
    (["--profile-usage", "--g2t", "none.g2t", "--profile-evals", "0"], "--profile-evals must be positive.", False),
]


@pytest.mark.parametrize("args,message,usage", MESSAGES, ids=[" ".join(a) for a, _, _ in MESSAGES])
def test_cli_messages(args, message, usage, tmp_path):
    _build.build_all()
    r = subprocess.run([_build.CLI] + args + ["-P", "-I", str(tmp_path / "none.rsh"), str(tmp_path / "o"), "out", "none.bowtie"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    head, sep, _ = r.stderr.partition("Usage : ")
    assert r.returncode == 1 and head == message + "\n" and bool(sep) == usage, r.stderr
    assert not (tmp_path / "o").exists() and r.stdout == ""


def test_cli_accepts_the_profile_options_with_profile_usage(tmp_path):
    """with --profile-usage and a gene map the three --profile-* options pass the option checks: the run ends at the index that does not exist"""
    _build.build_all()
    r = subprocess.run([_build.CLI, "--profile-usage", "--g2t", "none.g2t", "--profile-level", "0.9", "--profile-evals", "30", "--profile-list", "l", "-P",
                        "-I", str(tmp_path / "none.rsh"), str(tmp_path / "o"), "out", "none.bowtie"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0 and "need --profile" not in r.stderr and "needs --g2t" not in r.stderr and "Usage : " not in r.stderr, r.stderr
