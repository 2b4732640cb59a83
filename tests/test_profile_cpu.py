"""CPU: what the profile-likelihood intervals (include/emsar_hip.h "profile-likelihood intervals") define on the host -- the chi2_1 cut,
the ABI's structs and names, the .profile writer, and that the device entry point does not run without a device."""
import ctypes as C
import math
import os
import re

import pytest

from emsar_amd import _build
from emsar_amd import hip as H
from tests import profile_problems as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    _build.build_all()


def test_cut_is_the_chi2_quantile():
    """against 2 erfinv(level)^2 from a bisection on math.erf in Python, to 1e-12 relative; two values written out"""
    for level in (0.5, 0.6826894921370859, 0.9, 0.95, 0.99, 0.999):
        got, want = H.profile_cut_host(level), PP.cut(level)
        assert abs(got - want) <= 1e-12 * want, (level, got, want)
    assert abs(H.profile_cut_host(0.95) - 3.841458820694124) <= 1e-12 * 3.841458820694124
    assert abs(H.profile_cut_host(0.99) - 6.634896601021214) <= 1e-12 * 6.634896601021214
    assert abs(H.profile_cut_host(math.erf(1 / math.sqrt(2))) - 1.0) <= 1e-12
    L = H.load_library()
    out = C.c_double(-1.0)
    for bad in (0.0, 1.0, math.nan, -0.5, 1.5):
        assert L.emsar_hip_profile_cut_host(bad, C.byref(out)) == -1 and out.value == -1.0, bad
        with pytest.raises(H.EmsarHipError) as e:
            H.profile_cut_host(bad)
        assert e.value.status == -1
    assert L.emsar_hip_profile_cut_host(0.95, None) == -1


def test_abi_structs_and_names():
    L = H.load_library()
    for name in ("emsar_hip_profile", "emsar_hip_profile_cut_host"):
        assert name in H.SYMBOLS and hasattr(L, name)
    assert C.sizeof(H.ProfileParams) == 8 + 8 + 4 + 4
    assert C.sizeof(H.ProfileOutputs) == 8 * C.sizeof(C.c_void_p)
    assert C.sizeof(H.ProfileStats) == 8 * 5 + 8 * 3 + 4 * 2 + 8 * 5
    text = open(os.path.join(ROOT, "include", "emsar_hip.h")).read()
    enum = dict(re.findall(r"EMSAR_PROFILE_([A-Z_]+) = (\d)", text))
    assert [k for k, _ in sorted(enum.items(), key=lambda kv: int(kv[1]))] == list(H.PROFILE_STATUS)
    assert list(H.PROFILE_STATUS) == ["TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED"]
    # the fields of the header's structs, in order, against the ctypes mirrors
    for struct, mirror in (("emsar_profile_params", H.ProfileParams), ("emsar_profile_outputs", H.ProfileOutputs),
                           ("emsar_profile_stats", H.ProfileStats)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if f.strip()]
        fields = [re.sub(r"\[\d+\]", "", f) for f in fields]
        assert fields == [k.rstrip("_") for k, _ in mirror._fields_], struct
    types = {"double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64}
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} emsar_profile_stats;", text).group(1), flags=re.S)
    want = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            for f in m.group(2).split(","):
                n = re.search(r"\[(\d+)\]", f)
                want.append(types[m.group(1)] * int(n.group(1)) if n else types[m.group(1)])
    assert [C.sizeof(t) for t in want] == [C.sizeof(t) for _, t in H.ProfileStats._fields_]


def test_no_device_no_answer():
    """no context: ERR_ARG; and without a GPU no context can be made (ERR_NO_DEVICE), so there is no host path to fall back to"""
    import torch

    import emsar_amd
    L = H.load_library()
    assert L.emsar_hip_profile(None, None, None, 0, None, None, None) == -1
    if not torch.cuda.is_available():
        with pytest.raises(emsar_amd.EmsarHipError) as e:
            emsar_amd.EmsarHip(0)
        assert e.value.status == -2


def test_profile_file(tmp_path):
    from emsar_amd import hostlib
    names = ["tA", "tB", "tC", "tD"]
    fpkm = [3.1, 0.0, 12.5, 1e-7]
    path = str(tmp_path / "x.profile")
    hostlib.write_profile(path, names, fpkm, [1.25, 0.0, 9.0, math.nan], [6.5, 3.841459, 17.25, math.nan], [7.5, 0.0, math.inf, math.nan], [0, 1, 4, 3])
    lines = open(path).read().splitlines()
    assert lines[0] == "tid\ttranscriptID\tFPKM\tlower\tupper\tLambda\tstatus"
    assert lines[1:] == ["0\ttA\t3.100000\t1.250000\t6.500000\t7.500000\tTWO_SIDED",
                         "1\ttB\t0.000000\t0.000000\t3.841459\t0.000000\tLOWER_ZERO",
                         "2\ttC\t12.500000\t9.000000\t17.250000\tinf\tUNCONVERGED",
                         "3\ttD\t0.000000\tnan\tnan\tnan\tNOT_RESIDENT"]
    # a query list: its order, repeats kept; FPKM by tid
    hostlib.write_profile(path, names, fpkm, [1.0, 0.0, 1.0], [2.0, 5.0, 2.0], [9.0, 1.0, 9.0], [0, 2, 0], query=[2, 0, 2])
    lines = open(path).read().splitlines()
    assert [l.split("\t")[:3] for l in lines[1:]] == [["2", "tC", "12.500000"], ["0", "tA", "3.100000"], ["2", "tC", "12.500000"]]
    assert lines[2].split("\t")[3:] == ["0.000000", "5.000000", "1.000000", "OUTSIDE"]
    with pytest.raises(hostlib.HostError):
        hostlib.write_profile(str(tmp_path / "no" / "dir.profile"), names, fpkm, [0.0] * 4, [1.0] * 4, [0.0] * 4, [1] * 4)


def test_profile_kernels_use_no_scratch():
    """the ISA listing of the build (absent where build/ is not shipped): the three k_profile_sets instantiations use no scratch memory
    -- the search's state is a handful of uniform scalars on top of the set solver's registers"""
    asm = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        pytest.skip("no ISA listing (build/ is not shipped)")
    meta = {}
    for blk in open(asm).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_spill_count", "private_segment_fixed_size")}
    for threads in (64, 256, 512):
        names = [n for n in meta if n and "k_profile_setsILi%dE" % threads in n]
        assert len(names) == 1, (threads, names)
        assert meta[names[0]]["vgpr_spill_count"] == 0 and meta[names[0]]["private_segment_fixed_size"] == 0, (names[0], meta[names[0]])
