"""CPU: the bootstrap quantiles' definition (include/emsar_hip.h "bootstrap quantiles") -- quantiles_host against a pure-Python
restatement bit for bit, against numpy.quantile within the derived rounding bound, its exact properties and argument errors, the ABI
struct, the CLI's argument checks and the new kernel's code -- no GPU needed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from emsar_amd import _build, hip

BS = [1, 2, 3, 10, 99, 100, 1000, 4096]
QS = [0.0, 0.025, 0.25, 0.5, 0.975, 1.0]


def restated(column, q):
    """The definition, operation for operation: Python floats are IEEE doubles and every operator rounds once."""
    x = sorted(column)
    B = len(x)
    h = q * float(B - 1)
    i = int(math.floor(h))
    g = h - float(i)
    if g == 0.0 or i == B - 1:
        return x[i]
    d = x[i + 1] - x[i]
    s = g * d
    return x[i] + s


def columns(B, seed):
    """[B][8]: lognormal, uniform, many zeros plus a tail, all zeros, all equal, two values, small integers (ties), wide range"""
    rng = np.random.default_rng(seed)
    c = [rng.lognormal(0.0, 3.0, B), rng.random(B), rng.lognormal(1.0, 1.0, B) * (rng.random(B) < 0.3), np.zeros(B), np.full(B, 3.25),
         rng.integers(0, 2, B) * 7.5, rng.integers(0, 5, B).astype(np.float64), 10.0 ** rng.uniform(-300, 300, B)]
    return np.ascontiguousarray(np.stack(c, axis=1))


def all_q(seed):
    return np.array(QS + np.random.default_rng(seed).random(7).tolist())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("B", BS)
def test_host_equals_the_restatement_bit_for_bit(B):
    v, q = columns(B, B), all_q(B + 1)
    got = hip.quantiles_host(v, q)
    assert got.shape == (len(q), v.shape[1])
    want = np.array([[restated(v[:, t].tolist(), float(qk)) for t in range(v.shape[1])] for qk in q])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(hip.quantiles_host(v[:, 0], q), got[:, 0])               # a single column


@pytest.mark.parametrize("B", BS)
def test_host_against_numpy(B):
    """numpy's "linear" method is the same formula up to rounding.  The position h = q (B - 1) is one multiplication on both sides.  The
    library rounds three times (the subtraction, the product, the sum), numpy at most four (for g >= 0.5 it takes x_(i+1) - d (1 - g), and
    1 - g is rounded as well).  Every one of these errors is at most half an ulp of a quantity no larger than m = max(|x_(i)|, |x_(i+1)|):
    0 <= g < 1, and the values here are non-negative, so |d| = |x_(i+1) - x_(i)| <= m.  That is 1.5 ulp(m) on one side and 2 on the
    other: the two differ by at most 3.5 ulp(m), 4 are allowed."""
    v, q = columns(B, 100 + B), all_q(B + 2)
    got = hip.quantiles_host(v, q)
    want = np.quantile(v, q, axis=0)
    s = np.sort(v, axis=0)
    for k, qk in enumerate(q):
        i = int(math.floor(qk * float(B - 1)))
        big = np.maximum(s[i], s[min(i + 1, B - 1)])
        assert np.all(np.abs(got[k] - want[k]) <= 4 * np.spacing(big)), (B, qk)


@pytest.mark.parametrize("B", BS)
def test_exact_properties(B):
    v = columns(B, 200 + B)
    q = np.sort(all_q(B + 3))
    got = hip.quantiles_host(v, q)
    assert np.all(np.diff(got, axis=0) >= 0)                                       # non-decreasing in q
    assert np.array_equal(bits(got[0]), bits(v.min(axis=0))) and np.array_equal(bits(got[-1]), bits(v.max(axis=0)))
    if B % 2 == 1:
        assert np.array_equal(bits(hip.quantiles_host(v, [0.5])[0]), bits(np.sort(v, axis=0)[B // 2]))
    if B == 1:
        assert np.array_equal(bits(got), bits(np.repeat(v, len(q), axis=0)))
    rng = np.random.default_rng(B)
    for _ in range(3):                                                             # any order of the replicates
        assert np.array_equal(bits(hip.quantiles_host(v[rng.permutation(B)], q)), bits(got))


def test_argument_errors():
    L = hip.load_library()
    v = np.arange(12.0).reshape(4, 3)
    out = np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    q = np.array([0.5, 0.9])
    assert L.emsar_hip_quantiles_host(4, 3, p(v), 2, p(q), p(out)) == 0
    assert L.emsar_hip_quantiles_host(4, 3, p(v), 0, p(q), p(out)) == -1
    assert L.emsar_hip_quantiles_host(4, 3, p(v), -1, p(q), p(out)) == -1
    assert L.emsar_hip_quantiles_host(0, 3, p(v), 2, p(q), p(out)) == -1
    assert L.emsar_hip_quantiles_host(4, 3, p(v), 2, None, p(out)) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, 1.0000000000000002, 2.0):
        with pytest.raises(hip.EmsarHipError) as e:
            hip.quantiles_host(v, [0.5, bad])
        assert e.value.status == -1, bad
    with pytest.raises(hip.EmsarHipError) as e:
        hip.quantiles_host(v, [])
    assert e.value.status == -1


def test_quantile_stats_struct_matches_header():
    hdr = open(os.path.join(os.path.dirname(_build.PKG), "include", "emsar_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} emsar_quantile_stats;", hdr).group(1)
    size = {"int32_t": 4, "int64_t": 8, "double": 8}
    off, fields = 0, []
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
    assert [f for f, _ in hip.QuantileStats._fields_] == fields
    assert C.sizeof(hip.QuantileStats) == off == 24
    # additions only: the existing structs keep their size
    assert C.sizeof(hip.BootStats) == 64 and C.sizeof(hip.SubsampleStats) == 64


ASM = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")


def test_quantile_kernel_uses_no_scratch():
    _build.build_hip()
    if not os.path.exists(ASM):                   # a library built earlier without its listing: build again, the recipe leaves one
        _build.build_hip(force=True)
    assert os.path.exists(ASM), "build_hip() left no ISA listing"
    meta = {}
    for blk in open(ASM).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                                  "group_segment_fixed_size")}
    for kern, lds in (("16k_boot_quantiles", 0), ("12k_quant_sums", 128)):
        names = [n for n in meta if n.startswith("_ZN12_GLOBAL__N_1" + kern)]
        assert len(names) == 1, (kern, names)
        m = meta[names[0]]
        assert m["vgpr_spill_count"] == m["sgpr_spill_count"] == m["private_segment_fixed_size"] == 0, (kern, m)
        assert m["vgpr_count"] <= 64, (kern, m)        # eight waves to a SIMD: the LDS, not the registers, bounds the occupancy
        # k_boot_quantiles: the tile is dynamic LDS, sized by the launch (16 KiB up to B = 2048, 32 KiB above); k_quant_sums: 16 doubles
        assert m["group_segment_fixed_size"] == lds, (kern, m)


def _cli(args, tmp_path):
    _build.build_all()
    return subprocess.run([_build.CLI] + args + ["-P", "-I", str(tmp_path / "none.rsh"), str(tmp_path), "out", "none.bowtie"],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


BAD_LISTS = ["", "0.5,", ",0.5", "0.1,,0.5", "-0.5", "1.5", "0.5,1.0000001", "0.5,-1e-9", "x", "0.5x", "nan", "inf", "0.5;0.9",
             ",".join(["0.5"] * 65)]


@pytest.mark.parametrize("arg", BAD_LISTS)
def test_cli_rejects_bad_quantile_lists(arg, tmp_path):
    r = _cli(["--bootstrap", "10", "--bootstrap-quantiles", arg], tmp_path)
    assert r.returncode != 0
    assert "--bootstrap-quantiles" in r.stderr and "rsh" not in r.stderr


@pytest.mark.parametrize("boot", [[], ["--bootstrap", "0"], ["--bootstrap", "4097"]])
def test_cli_quantiles_need_a_bootstrap(boot, tmp_path):
    r = _cli(boot + ["--bootstrap-quantiles", "0.025,0.5,0.975"], tmp_path)
    assert r.returncode != 0
    assert "--bootstrap-quantiles" in r.stderr and "--bootstrap B" in r.stderr and "rsh" not in r.stderr
    # the order of the two options does not matter, and a good pair gets as far as the index
    r = _cli(["--bootstrap-quantiles", "0,0.5,1", "--bootstrap", "10"], tmp_path)
    assert r.returncode != 0 and "--bootstrap-quantiles" not in r.stderr
