"""CPU: the Poisson bootstrap's draws (emsar_amd/csrc/boot_rng.hpp) pinned against independent restatements, their distribution and
keying, the ABI struct, the batched set kernel's code, and the CLI's argument checks -- no GPU needed (bootstrap_draw_host)."""
import ctypes as C
import math
import os
import re
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

from emsar_amd import _build, hip

M64 = (1 << 64) - 1


# ---- an independent restatement of the generator ---------------------------------------------------------------------------------
def philox4x64_10(ctr, key):
    """Philox4x64-10 (Salmon et al. 2011): one block of four 64-bit words."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B97F4A7C15) & M64, (k1 + 0xBB67AE8584CAA73B) & M64
        p0, p1 = 0xD2E7470EE14C6C93 * c0, 0xCA5A826395121157 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & M64, (p0 >> 64) ^ c3 ^ k1, p0 & M64
    return [c0, c1, c2, c3]


def uniforms(seed, rep, row):
    j = 0
    while True:
        for w in philox4x64_10([row, j, 0, 0], [seed, rep]):
            yield (w >> 11) * 2.0 ** -53
        j += 1


getcontext().prec = 50
EXP_NEG = [float((-Decimal(n)).exp()) for n in range(17)]


def inversion(seed, rep, row, R):
    u = next(uniforms(seed, rep, row))
    p = EXP_NEG[R]
    F, k = p, 0
    while u >= F and k < 64:
        k += 1
        p = p * R / k
        F = F + p
    return k


def loggam(x):
    c = [8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04,
         -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e+00]
    if x == 1.0 or x == 2.0:
        return 0.0
    n = int(7.0 - x) if x < 7.0 else 0
    x0 = x + n
    x2 = 1.0 / (x0 * x0)
    g = c[9]
    for k in range(8, -1, -1):
        g = g * x2
        g = g + c[k]
    gl = g / x0 + 0.5 * math.log(2.0 * 3.141592653589793) + (x0 - 0.5) * math.log(x0) - x0
    for _ in range(n):
        gl = gl - math.log(x0 - 1.0)
        x0 = x0 - 1.0
    return gl


def ptrs(seed, rep, row, R):
    U = uniforms(seed, rep, row)
    lam = float(R)
    slam, loglam = math.sqrt(lam), math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    while True:
        u = next(U) - 0.5
        v = next(U)
        us = 0.5 - abs(u)
        k = math.floor((2.0 * a / us + b) * u + lam + 0.43)
        if us >= 0.07 and v <= vr:
            return k
        if k < 0 or (us < 0.013 and v > us):
            continue
        if (math.log(v) + math.log(invalpha) - math.log(a / (us * us) + b)) <= (-lam + k * loglam - loggam(k + 1.0)):
            return k


def test_python_philox_is_numpys():
    for key, ctr in [((1, 3), (5, 0, 0, 0)), ((2, 4), (17, 5, 0, 0)), ((M64, 123456789), (99999, 1, 0, 0)), ((0, 0), (1, 2, 3, 4))]:
        # numpy increments the counter before a block (c0 >= 1 here: no borrow into c1)
        g = np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array([(ctr[0] - 1) & M64, ctr[1], ctr[2], ctr[3]], dtype=np.uint64))
        assert [int(x) for x in g.random_raw(4)] == philox4x64_10(list(ctr), list(key))


def test_inversion_draws_match_the_restatement():
    R = np.tile(np.arange(0, 17, dtype=np.int32), 300)
    for seed, rep in [(1, 0), (1, 3), (987654321987, 11)]:
        got = hip.bootstrap_draw_host(seed, rep, R)
        want = [0 if r == 0 else inversion(seed, rep, i, int(r)) for i, r in enumerate(R)]
        assert got.tolist() == want


def test_ptrs_draws_match_the_restatement():
    R = np.array([17, 18, 25, 40, 99, 1000, 12345, 100000, 2 ** 30] * 60, dtype=np.int32)
    for seed, rep in [(1, 0), (5, 9)]:
        got = hip.bootstrap_draw_host(seed, rep, R)
        want = [ptrs(seed, rep, i, int(r)) for i, r in enumerate(R)]
        assert got.tolist() == want


@pytest.mark.parametrize("R", [0, 1, 2, 5, 16, 17, 40, 1000, 100000])
def test_distribution(R):
    n = 200000
    d = hip.bootstrap_draw_host(12345, 0, np.full(n, R, dtype=np.int32)).astype(np.float64)
    if R == 0:
        assert not d.any()
        return
    # mean and variance within 5 standard errors (var of the sample variance of a Poisson: (mu4 - sigma^4) / n, mu4 = R(1 + 3R))
    assert abs(d.mean() - R) <= 5 * math.sqrt(R / n)
    assert abs(d.var(ddof=1) - R) <= 5 * math.sqrt((R * (1 + 3 * R) - R * R) / n)
    if R in (5, 17, 40, 1000):
        from scipy import stats
        lo, hi = int(max(0, R - 6 * math.sqrt(R))), int(R + 6 * math.sqrt(R))
        edges = np.arange(lo, hi + 1)
        obs = np.array([(d < lo).sum()] + [(d == k).sum() for k in edges] + [(d > hi).sum()], dtype=np.float64)
        pmf = stats.poisson.pmf(edges, R)
        exp = np.concatenate([[stats.poisson.cdf(lo - 1, R)], pmf, [stats.poisson.sf(hi, R)]]) * n
        # pool sparse bins (expected < 5) into their neighbours
        o2, e2, ao, ae = [], [], 0.0, 0.0
        for o, e in zip(obs, exp):
            ao += o; ae += e
            if ae >= 5:
                o2.append(ao); e2.append(ae); ao = ae = 0.0
        o2[-1] += ao; e2[-1] += ae
        e2 = np.array(e2) * (sum(o2) / sum(e2))
        assert stats.chisquare(o2, e2).pvalue > 1e-4


def test_keying():
    R = np.random.default_rng(0).integers(0, 60, size=5000).astype(np.int32)
    full = hip.bootstrap_draw_host(1, 3, R)
    assert np.array_equal(hip.bootstrap_draw_host(1, 3, R[:1234]), full[:1234])
    assert not np.array_equal(full, hip.bootstrap_draw_host(1, 4, R))
    assert not np.array_equal(full, hip.bootstrap_draw_host(2, 3, R))
    assert np.array_equal(hip.bootstrap_draw_host(1, 3, None, n_rows=777), hip.bootstrap_draw_host(1, 3, np.ones(777, np.int32)))
    with pytest.raises(hip.EmsarHipError):
        hip.bootstrap_draw_host(1, -1, R)
    with pytest.raises(hip.EmsarHipError):
        hip.bootstrap_draw_host(1, 0, np.array([1, -2], np.int32))


def test_boot_stats_struct_matches_header():
    hdr = open(os.path.join(os.path.dirname(_build.PKG), "include", "emsar_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} emsar_boot_stats;", hdr).group(1)
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
    assert [f for f, _ in hip.BootStats._fields_] == fields
    assert C.sizeof(hip.BootStats) == (off + 7) // 8 * 8 == 64


ASM = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")


def test_batched_set_kernel_keeps_the_registers_of_the_set_kernel():
    _build.build_hip()
    if not os.path.exists(ASM):
        pytest.skip("no ISA listing (build/ is not shipped)")
    meta = {}
    for blk in open(ASM).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    for th in (64, 256, 512):
        base = [n for n in meta if n.startswith("_ZN12_GLOBAL__N_112k_solve_setsILi%dEE" % th)]
        boot = [n for n in meta if n.startswith("_ZN12_GLOBAL__N_117k_solve_sets_bootILi%dEE" % th)]
        assert len(base) == 1 and len(boot) == 1, (base, boot)
        a, b = meta[base[0]], meta[boot[0]]
        assert b["vgpr_count"] == a["vgpr_count"], (th, a, b)
        assert b["vgpr_spill_count"] == b["sgpr_spill_count"] == b["private_segment_fixed_size"] == 0, (th, b)


@pytest.mark.parametrize("arg", ["-1", "x", "3x", ""])
def test_cli_rejects_bad_bootstrap_counts(arg, tmp_path):
    _build.build_all()
    r = subprocess.run([_build.CLI, "--bootstrap", arg, "-P", "1", str(tmp_path / "none.rsh"), str(tmp_path), "out", "none.bowtie"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0
    assert "--bootstrap" in r.stderr


def test_cli_rejects_bad_bootstrap_seed(tmp_path):
    _build.build_all()
    r = subprocess.run([_build.CLI, "--bootstrap", "5", "--bootstrap-seed", "abc", str(tmp_path / "none.rsh"), str(tmp_path), "out", "none.bowtie"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode != 0 and "--bootstrap-seed" in r.stderr
