"""CPU: what the presence test (include/emsar_hip.h "presence test") defines on the host -- the p-value of the boundary mixture, the
ABI's structs and names, and the .presence writer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from emsar_amd import _build
from emsar_amd import hip as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    _build.build_all()


def _ulps(a, b):
    if a == b:
        return 0
    ia, ib = np.array([a, b], dtype=np.float64).view(np.int64)
    return abs(int(ia) - int(ib))


def test_pvalue_of_the_boundary_mixture():
    lam = [0.0, 1e-300, 1e-12, 0.5, 3.84, 50.0, 1e4, math.inf]
    got = H.presence_pvalue_host(np.array(lam))
    want = [1.0] + [0.5 * math.erfc(math.sqrt(x / 2)) for x in lam[1:-1]] + [0.0]
    for x, g, w in zip(lam, got, want):
        assert _ulps(float(g), w) <= 4, (x, g, w)
    assert got[0] == 1.0 and got[-1] == 0.0 and got[-2] == 0.0               # Lambda = 1e4: erfc underflows
    assert abs(got[1] - 0.5) < 1e-12 and abs(got[2] - 0.5) < 1e-6 and 0.0249 < got[4] < 0.0251      # 3.84: the 5 % point of chi2_1, halved
    assert math.isnan(H.presence_pvalue_host(math.nan)) and H.presence_pvalue_host(2.0) == 0.5 * math.erfc(1.0)
    assert H.presence_pvalue_host(-1e-9) == 1.0                               # below 0 only by rounding: reported as Lambda = 0
    assert H.presence_pvalue_host(np.zeros(0)).shape == (0,)
    L = H.load_library()
    assert L.emsar_hip_presence_pvalue_host(3, None, None) == -1 and L.emsar_hip_presence_pvalue_host(-1, None, None) == -1
    assert L.emsar_hip_presence_pvalue_host(0, None, None) == 0


def test_abi_structs_and_names():
    L = H.load_library()
    for name in ("emsar_hip_presence", "emsar_hip_presence_pvalue_host"):
        assert name in H.SYMBOLS and hasattr(L, name)
    assert C.sizeof(H.PresenceOutputs) == 6 * C.sizeof(C.c_void_p)
    assert C.sizeof(H.PresenceStats) == 8 * 6 + 8 + 8 + 4 + 4 + 8 * 4
    text = open(os.path.join(ROOT, "include", "emsar_hip.h")).read()
    enum = dict(re.findall(r"EMSAR_PRESENCE_([A-Z_]+) = (\d)", text))
    assert [k for k, _ in sorted(enum.items(), key=lambda kv: int(kv[1]))] == list(H.PRESENCE_STATUS)
    # the fields of the header's structs, in order, against the ctypes mirrors
    for struct, mirror in (("emsar_presence_outputs", H.PresenceOutputs), ("emsar_presence_stats", H.PresenceStats)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if f.strip()]
        fields = [re.sub(r"\[\d+\]", "", f) for f in fields]
        assert fields == [k.rstrip("_") for k, _ in mirror._fields_], struct
    assert L.emsar_hip_presence(None, None, 0, None, None, None) == -1           # no context


def test_presence_file(tmp_path):
    from emsar_amd import hostlib
    names = ["tA", "tB", "tC", "tD"]
    fpkm = [3.1, 0.0, 12.5, 1e-7]
    path = str(tmp_path / "x.presence")
    hostlib.write_presence(path, names, fpkm, [2.5, 0.0, math.inf, math.nan], [0.05692344, 1.0, 0.0, math.nan], [0, 1, 2, 4], [2, -1, -1, -1],
                           [0.75, math.nan, math.nan, math.nan])
    lines = open(path).read().splitlines()
    assert lines[0] == "tid\ttranscriptID\tFPKM\tLambda\tp\tstatus\their\their_share"
    assert lines[1:] == ["0\ttA\t3.100000\t2.500000\t0.0569234\tTESTED\ttC\t0.750000",
                         "1\ttB\t0.000000\t0.000000\t1\tABSENT\t-\tnan",
                         "2\ttC\t12.500000\tinf\t0\tESSENTIAL\t-\tnan",
                         "3\ttD\t0.000000\tnan\tnan\tNOT_RESIDENT\t-\tnan"]
    # a query list: its order, repeats kept; FPKM by tid
    hostlib.write_presence(path, names, fpkm, [1.0, 4.0, 1.0], [0.1, 0.02, 0.1], [0, 5, 0], [0, 3, 0], [0.5, 1.0, 0.5], query=[2, 0, 2])
    lines = open(path).read().splitlines()
    assert [l.split("\t")[:3] for l in lines[1:]] == [["2", "tC", "12.500000"], ["0", "tA", "3.100000"], ["2", "tC", "12.500000"]]
    assert lines[2].split("\t")[5:] == ["UNCONVERGED", "tD", "1.000000"]
    with pytest.raises(hostlib.HostError):
        hostlib.write_presence(str(tmp_path / "no" / "dir.presence"), names, fpkm, [0.0] * 4, [1.0] * 4, [1] * 4, [-1] * 4, [math.nan] * 4)


def test_set_kernels_use_no_scratch():
    """the ISA listing of the build (absent where build/ is not shipped): the three k_solve_sets_drop instantiations, like the set kernels
    they share solve_one_set with, spill nothing and use no scratch, and stay inside the register budget of their workgroup size
    (512 threads = 8 waves on 4 SIMDs = at most 128 VGPRs)"""
    asm = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        pytest.skip("no ISA listing (build/ is not shipped)")
    meta = {}
    for blk in open(asm).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    for kernel in ("k_solve_setsILi", "k_solve_sets_bootILi", "k_solve_sets_dropILi"):
        for threads in (64, 256, 512):
            names = [n for n in meta if n and "%s%dE" % (kernel, threads) in n]
            assert len(names) == 1, (kernel, threads, names)
            m = meta[names[0]]
            assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (names[0], m)
            assert m["vgpr_count"] <= 128, (names[0], m)
