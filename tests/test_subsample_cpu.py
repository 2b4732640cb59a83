"""CPU: the binomial draws of the depth subsampling (boot_binomial, emsar_amd/csrc/boot_rng.hpp) pinned against an independent
restatement, their distribution and keying, the ABI struct, the new kernels' code, and the CLI's argument checks -- no GPU needed
(subsample_draw_host)."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from emsar_amd import _build, hip
from tests.test_bootstrap_cpu import inversion as poisson_inversion
from tests.test_bootstrap_cpu import loggam, philox4x64_10, ptrs

FRACTIONS = [0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99]


# ---- an independent restatement of boot_binomial -----------------------------------------------------------------------------------
def f_bits(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def uniforms(seed, rep, row, f):
    j = 0
    while True:
        for w in philox4x64_10([row, j, 1, f_bits(f)], [seed, rep]):
            yield (w >> 11) * 2.0 ** -53
        j += 1


def is_inversion(R, f):
    return R * min(f, 1.0 - f) < 10.0


def binomial(seed, rep, row, R, f):
    if R <= 0:
        return 0
    if f >= 1.0:
        return R
    U = uniforms(seed, rep, row, f)
    flip = f > 0.5
    p = 1.0 - f if flip else f
    q = 1.0 - p
    n = float(R)
    if n * p < 10.0:
        pr, sq, e = 1.0, q, R
        while e:
            if e & 1:
                pr = pr * sq
            sq = sq * sq
            e >>= 1
        u = next(U)
        s = p / q
        F, k = pr, 0
        while u >= F and k < R:
            k += 1
            pr = pr * s * float(R - k + 1) / float(k)
            F = F + pr
        return R - k if flip else k
    spq = math.sqrt(n * p * q)
    b = 1.15 + 2.53 * spq
    a = -0.0873 + 0.0248 * b + 0.01 * p
    c = n * p + 0.5
    vr = 0.92 - 4.2 / b
    alpha = (2.83 + 5.1 / b) * spq
    lpq = math.log(p / q)
    m = math.floor((n + 1.0) * p)
    h = loggam(m + 1.0) + loggam(n - m + 1.0)
    while True:
        u = next(U) - 0.5
        v = next(U)
        us = 0.5 - abs(u)
        k = math.floor((2.0 * a / us + b) * u + c) if us > 0.0 else -1
        if not (us >= 0.07 and v <= vr):
            if k < 0 or k > n:
                continue
            lv = math.log(v * alpha / (a / (us * us) + b)) if v > 0.0 else -math.inf
            if not (lv <= h - loggam(k + 1.0) - loggam(n - k + 1.0) + (k - m) * lpq):
                continue
        return R - int(k) if flip else int(k)


def test_draws_match_the_restatement_on_a_grid():
    """R = 1 .. 2000 for every fraction: the inversion branch (only *, /, +, - and compares) and the BTRS branch (the same libm)."""
    R = np.arange(1, 2001, dtype=np.int32)
    n_inv = n_btrs = 0
    for f in FRACTIONS:
        got = hip.subsample_draw_host(7, 2, f, R)
        want = [binomial(7, 2, i, int(r), f) for i, r in enumerate(R)]
        inv = np.array([is_inversion(int(r), f) for r in R])
        assert got[inv].tolist() == [w for w, i in zip(want, inv) if i], f
        assert got[~inv].tolist() == [w for w, i in zip(want, inv) if not i], f
        n_inv += inv.sum()
        n_btrs += (~inv).sum()
    assert n_inv > 2000 and n_btrs > 2000


def test_large_counts_match_the_restatement():
    R = np.array([17, 40, 99, 1000, 12345, 100000, 2 ** 30, 2 ** 31 - 1] * 40, dtype=np.int32)
    for seed, rep, f in [(1, 0, 0.3), (5, 9, 0.8), (987654321987, 11, 1e-7)]:
        got = hip.subsample_draw_host(seed, rep, f, R)
        assert got.tolist() == [binomial(seed, rep, i, int(r), f) for i, r in enumerate(R)]


def btrs_rows():
    """The large-count input of the GPU test's device-against-host comparison: lognormal R up to 1e5, one transcript per row."""
    rng = np.random.default_rng(5)
    n_rows, n_tx = 40000, 500
    rp = np.arange(n_rows + 1, dtype=np.uint64)
    ci = rng.integers(0, n_tx, size=n_rows).astype(np.int32)
    R = np.minimum(rng.lognormal(3.0, 2.5, size=n_rows), 1e5).astype(np.int32)
    return n_tx, rp, ci, R


def test_host_draws_match_the_restatement_on_the_gpu_tests_rows():
    """The GPU test allows the device 0.1 % of the BTRS rows off the host's draws (an ulp of log at an acceptance edge).  Host against
    restatement there is the same code with the same libm: no row may differ, and there are enough BTRS rows for 0.1 % to mean something."""
    _, _, _, R = btrs_rows()
    for f in (0.3, 0.5, 0.8):
        got = hip.subsample_draw_host(2, 3, f, R)
        want = np.array([binomial(2, 3, i, int(r), f) for i, r in enumerate(R)])
        btrs = ~(R * min(f, 1.0 - f) < 10.0)
        assert btrs.sum() >= 10000
        assert (got != want).sum() == 0, f


def test_edges_and_range():
    rng = np.random.default_rng(2)
    R = np.minimum(rng.lognormal(2.0, 2.5, size=50000), 1e6).astype(np.int32)
    R[::7] = 0
    assert np.array_equal(hip.subsample_draw_host(3, 1, 1.0, R), R)                   # f = 1: R itself
    for f in (1e-9, 0.01, 0.3, 0.5, 0.9, 0.999999):                                    # 0.9 and 0.999999: the symmetry branch
        w = hip.subsample_draw_host(3, 1, f, R)
        assert (w >= 0).all() and (w <= R).all(), f
        assert not w[R == 0].any()
    assert np.array_equal(hip.subsample_draw_host(3, 1, 0.4, None, n_rows=777), hip.subsample_draw_host(3, 1, 0.4, np.ones(777, np.int32)))
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(hip.EmsarHipError) as e:
            hip.subsample_draw_host(1, 0, bad, R)
        assert e.value.status == -1
    with pytest.raises(hip.EmsarHipError):
        hip.subsample_draw_host(1, -1, 0.5, R)
    with pytest.raises(hip.EmsarHipError):
        hip.subsample_draw_host(1, 0, 0.5, np.array([1, -2], np.int32))


def _log_pmf(k, R, f):
    return math.lgamma(R + 1) - math.lgamma(k + 1) - math.lgamma(R - k + 1) + k * math.log(f) + (R - k) * math.log1p(-f)


@pytest.mark.parametrize("f", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("R", [1, 2, 5, 16, 40, 1000, 100000])
def test_distribution(R, f):
    """Judged like the Poisson draws (tests/test_bootstrap_cpu.py::test_distribution): mean and variance within 5 standard errors, the
    histogram against the exact pmf by a chi-square test with sparse bins pooled, p > 1e-4."""
    from scipy import stats
    n = 200000
    d = hip.subsample_draw_host(12345, 0, f, np.full(n, R, dtype=np.int32)).astype(np.float64)
    var = R * f * (1 - f)
    assert abs(d.mean() - R * f) <= 5 * math.sqrt(var / n)
    # var of the sample variance, exactly: (mu4 - sigma^4 (n - 3) / (n - 1)) / n, mu4 = npq (1 + 3 (n - 2) pq) for a binomial (the
    # Poisson test's (mu4 - sigma^4) / n drops the (n - 3) / (n - 1), which matters only where mu4 = sigma^4: one fair coin)
    mu4 = var * (1 + 3 * (R - 2) * f * (1 - f))
    assert abs(d.var(ddof=1) - var) <= 5 * math.sqrt((mu4 - var * var * (n - 3) / (n - 1)) / n)
    lo, hi = int(max(0, R * f - 6 * math.sqrt(var))), int(min(R, R * f + 6 * math.sqrt(var)))
    edges = np.arange(lo, hi + 1)
    pmf = np.array([math.exp(_log_pmf(int(k), R, f)) for k in edges])
    below = sum(math.exp(_log_pmf(k, R, f)) for k in range(max(0, lo - 200), lo))
    above = max(0.0, 1.0 - pmf.sum() - below)
    obs = np.array([(d < lo).sum()] + [(d == k).sum() for k in edges] + [(d > hi).sum()], dtype=np.float64)
    exp = np.concatenate([[below], pmf, [above]]) * n
    # pool sparse bins (expected < 5) into their neighbours
    o2, e2, ao, ae = [], [], 0.0, 0.0
    for o, e in zip(obs, exp):
        ao += o; ae += e
        if ae >= 5:
            o2.append(ao); e2.append(ae); ao = ae = 0.0
    o2[-1] += ao; e2[-1] += ae
    e2 = np.array(e2) * (sum(o2) / sum(e2))
    assert len(o2) >= 2
    assert stats.chisquare(o2, e2).pvalue > 1e-4


def test_keying():
    R = np.random.default_rng(0).integers(0, 60, size=5000).astype(np.int32)
    full = hip.subsample_draw_host(1, 3, 0.5, R)
    assert np.array_equal(hip.subsample_draw_host(1, 3, 0.5, R), full)
    # a row's draw does not depend on the other rows
    assert np.array_equal(hip.subsample_draw_host(1, 3, 0.5, R[:1234]), full[:1234])
    R2 = R.copy()
    R2[::2] += 5
    assert np.array_equal(hip.subsample_draw_host(1, 3, 0.5, R2)[1::2], full[1::2])
    # it changes with the seed, the replicate, the row and the fraction
    assert not np.array_equal(full, hip.subsample_draw_host(2, 3, 0.5, R))
    assert not np.array_equal(full, hip.subsample_draw_host(1, 4, 0.5, R))
    same = np.full(5000, 30, dtype=np.int32)
    d = hip.subsample_draw_host(1, 3, 0.5, same)
    assert len(set(d.tolist())) > 5
    # two fractions a hair apart draw from different streams (the uniforms are keyed by the bits of f, not only scaled by it)
    e = hip.subsample_draw_host(1, 3, math.nextafter(0.5, 0.0), same)
    assert (d != e).mean() > 0.5


def test_bootstrap_draws_are_unchanged_and_independent():
    R = np.tile(np.arange(0, 17, dtype=np.int32), 100)
    got = hip.bootstrap_draw_host(1, 3, R)
    assert got.tolist() == [0 if r == 0 else poisson_inversion(1, 3, i, int(r)) for i, r in enumerate(R)]
    big = np.array([17, 40, 1000, 100000] * 50, dtype=np.int32)
    assert hip.bootstrap_draw_host(5, 9, big).tolist() == [ptrs(5, 9, i, int(r)) for i, r in enumerate(big)]
    n = 200000
    for Rc, f in [(8, 0.5), (40, 0.5), (1000, 0.25)]:
        same = np.full(n, Rc, dtype=np.int32)
        a = hip.bootstrap_draw_host(1, 3, same).astype(np.float64)
        b = hip.subsample_draw_host(1, 3, f, same).astype(np.float64)
        assert abs(np.corrcoef(a, b)[0, 1]) < 5 / math.sqrt(n), (Rc, f)


def test_subsample_stats_struct_matches_header():
    hdr = open(os.path.join(os.path.dirname(_build.PKG), "include", "emsar_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} emsar_subsample_stats;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int32_t": 4, "int64_t": 8, "double": 8}
    off = 0
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        for nm in names.split(","):
            s = size[ty]
            off = (off + s - 1) // s * s
            fields.append(nm.strip())
            off += s
    assert [f for f, _ in hip.SubsampleStats._fields_] == fields
    assert C.sizeof(hip.SubsampleStats) == (off + 7) // 8 * 8 == 64


ASM = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")


def test_new_kernels_use_no_scratch():
    _build.build_hip()
    if not os.path.exists(ASM):                   # a library built earlier without its listing: build again, the recipe leaves one
        _build.build_hip(force=True)
    assert os.path.exists(ASM), "build_hip() left no ISA listing"
    meta = {}
    for blk in open(ASM).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    for kern, vmax in (("10k_sub_draw", 128), ("11k_sub_scale", 16), ("11k_boot_draw", 128)):
        names = [n for n in meta if n.startswith("_ZN12_GLOBAL__N_1" + kern)]
        assert len(names) == 1, (kern, names)
        m = meta[names[0]]
        assert m["vgpr_spill_count"] == m["sgpr_spill_count"] == m["private_segment_fixed_size"] == 0, (kern, m)
        assert m["vgpr_count"] <= vmax, (kern, m)


BAD_LISTS = ["", "0.5,", ",0.5", "0.1,,0.5", "0", "0.5,0", "-0.5", "1.5", "0.5,1.0000001", "x", "0.5x", "nan", "inf", ",".join(["0.5"] * 65)]


@pytest.mark.parametrize("arg", BAD_LISTS)
def test_cli_rejects_bad_subsample_lists(arg, tmp_path):
    _build.build_all()
    r = subprocess.run([_build.CLI, "--subsample", arg, "-P", "1", str(tmp_path / "none.rsh"), str(tmp_path), "out", "none.bowtie"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0
    assert "--subsample" in r.stderr and "rsh" not in r.stderr


@pytest.mark.parametrize("opt,arg", [("--subsample-reps", "0"), ("--subsample-reps", "x"), ("--subsample-reps", "-3"), ("--subsample-seed", "abc"),
                                     ("--subsample-seed", "-1")])
def test_cli_rejects_bad_subsample_counts(opt, arg, tmp_path):
    _build.build_all()
    r = subprocess.run([_build.CLI, "--subsample", "0.5", opt, arg, str(tmp_path / "none.rsh"), str(tmp_path), "out", "none.bowtie"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0 and opt in r.stderr
