"""CPU: the asymptotic standard errors (include/emsar_hip.h "asymptotic standard errors") as emsar_hip_asymptotic_host computes them --
against a pure-Python restatement of the definition bit for bit, against known answers, against numpy's inverse, and the ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from emsar_amd import _build
from emsar_amd import hip as H

from . import asym_problems as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = 5e-7


@pytest.fixture(scope="module", autouse=True)
def _built():
    _build.build_all()


def _host(p, **kw):
    return H.asymptotic_host(p["n_tx"], p["row_ptr"], p["col_idx"], p["theta"], row_weight=p["weight"], **kw)


def _edge_problem(n, seed):
    """a component of n, a second one of 3 that only an inactive transcript ties to it, a row with E == 0 between the two, a transcript
    at theta == boundary_cut and one at the next double above it, and a gene map with a gene across both components"""
    rng = np.random.default_rng(seed)
    a, b = AP.component(n, rng), AP.component(3, rng)
    p = AP.assemble([a, b], rng)
    z, eq, nx = p["n_tx"], p["n_tx"] + 1, p["n_tx"] + 2
    rows = [list(p["col_idx"][int(p["row_ptr"][c]):int(p["row_ptr"][c + 1])]) for c in range(len(p["row_ptr"]) - 1)]
    w = list(p["weight"])
    a0, b0 = int(p["comp_tids"][0][0]), int(p["comp_tids"][1][0])
    extra = [([a0, z], 7), ([z, b0], 9), ([z], 3), ([a0, b0], 11), ([eq, nx], 5), ([eq], 2), ([nx], 4), ([nx, eq, nx], 6)]
    for r, x in extra:
        at = int(rng.integers(0, len(rows) + 1))
        rows.insert(at, r)
        w.insert(at, x)
    theta = np.concatenate([p["theta"], [1e-9, CUT, np.nextafter(CUT, 1.0)]])
    q = AP.from_rows(p["n_tx"] + 3, rows, w, theta)
    q["E"] = np.array([0.0 if r == [a0, b0] else 1.5 for r in rows])
    q["n_genes"] = 4
    q["gene"] = rng.integers(-1, 3, size=q["n_tx"]).astype(np.int32)          # gene 3 stays empty
    q["gene"][[a0, b0]] = 0
    q["ids"] = dict(a0=a0, b0=b0, z=z, eq=eq, nx=nx, n=n)
    return q


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9, 17])
def test_equals_the_restatement(n):
    p = _edge_problem(n, 100 + n)
    got = _host(p, E=p["E"], gene_of_tx=p["gene"], n_genes=p["n_genes"])
    want = AP.restate(p, E=p["E"], gene_of_tx=list(p["gene"]), n_genes=p["n_genes"])
    AP.assert_equals_restatement(got, want, genes=True)
    i = p["ids"]
    st = got["status"]
    assert st[i["z"]] == AP.BND and st[i["eq"]] == AP.BND and st[i["nx"]] == AP.EST
    assert (st[p["col_idx"]] != AP.BND).sum() > 0 and got["stats"].components == 3 and got["stats"].max_n == max(n, 3)
    assert got["stats"].n_status[AP.EST] == n + 3 + 1                              # nothing ties the two components together
    assert got["partner"][i["nx"]] == -1 and math.isnan(got["partner_cov"][i["nx"]])
    assert got["stats"].min_pivot_ratio == want["stats"]["min_pivot_ratio"]
    assert got["stats"].theta_unestimated_share == want["stats"]["theta_unestimated_share"] == 0.0
    # the block of each component equals the restatement's Sigma
    for t0 in (i["a0"], i["b0"], i["nx"]):
        blk = _host(p, E=p["E"], block_tid=t0)
        tids, Sg = want["blocks"][min(t for t in want["blocks"] if t0 in want["blocks"][t][0])]
        assert list(blk["block_tids"]) == tids and AP.same_bits(blk["block_cov"], np.array(Sg))
    assert _host(p, E=p["E"], block_tid=i["z"])["block_cov"].shape == (0, 0)


def test_known_answers():
    # one transcript, only single-tid rows: var = 1 / sum R / (theta * theta), one operation at a time
    th = 3.7
    p = AP.from_rows(1, [[0], [0], [0]], [5, 1, 12], [th])
    J = 0.0
    for R in (5.0, 1.0, 12.0):
        J = J + R / (th * th)
    r = _host(p)
    assert r["var"][0] == (1.0 * 1.0) / J and r["status"][0] == AP.EST and r["sd_fpkm"][0] == math.sqrt(r["var"][0])
    assert r["stats"].min_pivot_ratio == 1.0 and r["stats"].components_class[0] == 1
    # two transcripts that only ever occur together
    p = AP.from_rows(3, [[0, 2], [2, 0], [1]], [4, 9, 2], [1.5, 2.0, 0.7])
    r = _host(p)
    assert list(r["status"]) == [AP.UNI, AP.EST, AP.UNI] and list(r["blocker"]) == [2, -1, 2]
    assert r["var"][0] == r["var"][2] == math.inf and r["sd_tpm"][0] == math.inf and r["stats"].components_unidentifiable == 1
    assert r["stats"].theta_unestimated_share == (1.5 + 0.7) / ((1.5 + 2.0) + 0.7)
    AP.assert_equals_restatement(r, AP.restate(p))
    # an active transcript that no row with reads contains
    p = AP.from_rows(2, [[0], [1]], [3, 0], [1.0, 2.0])
    r = _host(p)
    assert list(r["status"]) == [AP.EST, AP.UNI] and r["blocker"][1] == 1
    # a row with reads over theta = 0 transcripts
    p = AP.from_rows(3, [[0, 1], [2]], [6, 3], [0.0, 0.0, 1.0])
    r = _host(p)                             # the default cut: the row is counted and marks no component
    assert list(r["status"]) == [AP.BND, AP.BND, AP.EST] and r["stats"].rows_infeasible == 1 and r["stats"].components == 1
    r = _host(p, boundary_cut=-1.0)          # theta = 0 is then active
    assert list(r["status"]) == [AP.INF, AP.INF, AP.EST] and r["stats"].rows_infeasible == 1 and r["stats"].components_infeasible == 1
    assert np.isnan(r["var"][:2]).all() and np.isnan(r["sd_tpm"][:2]).all() and r["var"][2] > 0
    AP.assert_equals_restatement(r, AP.restate(p, boundary_cut=-1.0))
    assert (_host(p, boundary_cut=0.0)["status"] == [AP.BND, AP.BND, AP.EST]).all()


@pytest.mark.parametrize("n,status", [(192, AP.EST), (193, AP.BIG)])
def test_too_large(n, status):
    p = AP.single(n, 7)
    r = _host(p)
    assert (r["status"] == status).all() and r["stats"].max_n == n
    if status == AP.BIG:
        for k in ("var", "rowsum", "sd_fpkm", "sd_tpm", "partner_cov"):
            assert np.isnan(r[k]).all(), k
        assert (r["partner"] == -1).all() and r["stats"].components_too_large == 1 and r["stats"].theta_unestimated_share == 1.0
    else:
        assert np.isfinite(r["var"]).all() and (r["var"] > 0).all() and r["stats"].components_class[3] == 1


def _numpy_J(p):
    rp, col, th = p["row_ptr"].astype(np.int64), p["col_idx"], p["theta"]
    J = np.zeros((p["n_tx"], p["n_tx"]))
    for c in range(len(rp) - 1):
        m = np.bincount(col[rp[c]:rp[c + 1]], minlength=p["n_tx"]).astype(np.float64)
        J += p["weight"][c] / (m @ th) ** 2 * np.outer(m, m)
    return J


# Measured for emsar_hip_asymptotic_host on the builder problems below (seed 11), x86-64, numpy on OpenBLAS:
#     n      cond(J)     max |block_cov - inv(J)|     max |J @ block_cov - I|
#     8      30.5        2.84e-14                     5.55e-16
#     64     1.77e+03    7.11e-14                     8.88e-16
#     192    1.04e+04    1.99e-13                     1.78e-15
# The bounds are 64 x these: the margin covers the difference between LAPACK's order of operations and the definition's, nothing else
# (the device equals the host bit for bit).
NUMPY_BOUNDS = {8: (64 * 2.84e-14, 64 * 5.55e-16), 64: (64 * 7.11e-14, 64 * 8.88e-16), 192: (64 * 1.99e-13, 64 * 1.78e-15)}


@pytest.mark.parametrize("n", [8, 64, 192])
def test_against_numpy(n):
    p = AP.single(n, 11)
    r = _host(p, block_tid=0)
    assert list(r["block_tids"]) == list(range(n)) and np.array_equal(r["block_cov"], r["block_cov"].T)
    J = _numpy_J(p)
    d_inv = np.abs(r["block_cov"] - np.linalg.inv(J)).max()
    d_id = np.abs(J @ r["block_cov"] - np.eye(n)).max()
    print("n = %d: cond(J) = %.3g, max |cov - inv(J)| = %.3g, max |J cov - I| = %.3g" % (n, np.linalg.cond(J), d_inv, d_id))
    assert d_inv <= NUMPY_BOUNDS[n][0] and d_id <= NUMPY_BOUNDS[n][1]
    assert AP.same_bits(r["var"], np.ascontiguousarray(np.diag(r["block_cov"])))


def test_finish_with_genes():
    """sd_tpm, gene_sd and usage_sd against the restated finish: a gene across two components, a gene with an UNIDENTIFIABLE member, a
    gene of boundary transcripts only, an empty gene, transcripts without a gene"""
    rng = np.random.default_rng(5)
    parts = [AP.component(4, rng), AP.component(6, rng), AP.component(1, rng)]
    parts.append(([[0, 1], [1, 0]], np.array([3, 8]), np.array([2.0, 5.0])))          # confounded: UNIDENTIFIABLE
    parts.append(([[0]], np.array([2]), np.array([0.0])))                            # boundary
    p = AP.assemble(parts, rng)
    gene = np.array([0, 0, 1, 1] + [1, 1, 2, 2, -1, -1] + [2] + [3, 3] + [4], dtype=np.int32)
    gene[int(p["comp_tids"][1][5])] = 3                                              # an estimated member next to the confounded pair
    r = _host(p, gene_of_tx=gene, n_genes=6)
    want = AP.restate(p, gene_of_tx=list(gene), n_genes=6)
    AP.assert_equals_restatement(r, want, genes=True)
    assert list(r["gene_status"]) == [AP.EST, AP.EST, AP.EST, AP.UNI, AP.BND, AP.BND]
    assert r["gene_sd"][3] == math.inf and r["gene_sd"][4] == 0.0 and r["gene_sd"][5] == 0.0 and (r["gene_sd"][:3] > 0).all()
    assert np.isnan(r["usage_sd"][gene == -1]).all() and (r["usage_sd"][gene == 3] == math.inf).all()
    assert 0 < r["stats"].theta_unestimated_share == want["stats"]["theta_unestimated_share"] < 1
    # a gene across two components adds their variances: the covariance between components is 0
    g1 = np.flatnonzero(gene == 1)
    blocks = [_host(p, block_tid=int(t)) for t in (g1[0], g1[-1])]
    v = 0.0
    for b in blocks:
        idx = [k for k, t in enumerate(b["block_tids"]) if gene[t] == 1]
        v += b["block_cov"][np.ix_(idx, idx)].sum()
    assert abs(r["gene_sd"][1] ** 2 - v) <= 1e-12 * v


def test_abi_structs_and_errors():
    L = H.load_library()
    for name in ("emsar_hip_asymptotic", "emsar_hip_asymptotic_host"):
        assert name in H.SYMBOLS and hasattr(L, name)
    assert C.sizeof(H.AsymParams) == 8 + 8 + 4 + 4
    assert C.sizeof(H.AsymOutputs) == 14 * C.sizeof(C.c_void_p)
    assert C.sizeof(H.AsymStats) == 8 * 3 + 8 * 4 + 8 + 8 * 5 + 8 + 4 + 4 + 8 * 7
    text = open(os.path.join(ROOT, "include", "emsar_hip.h")).read()
    enum = dict(re.findall(r"EMSAR_ASYM_([A-Z_]+) = (\d)", text))
    assert [k for k, _ in sorted(enum.items(), key=lambda kv: int(kv[1]))] == list(H.ASYM_STATUS) == list(AP.STATUS)
    assert int(re.search(r"#define EMSAR_ASYM_MAX_N (\d+)", text).group(1)) == H.ASYM_MAX_N
    for struct, mirror in (("emsar_asym_params", H.AsymParams), ("emsar_asym_outputs", H.AsymOutputs), ("emsar_asym_stats", H.AsymStats)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if f.strip()]
        fields = [re.sub(r"\[\d+\]", "", f) for f in fields]
        assert fields == [k for k, _ in mirror._fields_], struct
    assert L.emsar_hip_asymptotic(None, None, None, None, None) == -1            # no context
    p = AP.single(3, 1)
    for bad in (np.array([1.0, -1.0, 1.0]), np.array([1.0, math.nan, 1.0]), np.array([1.0, math.inf, 1.0])):
        with pytest.raises(H.EmsarHipError) as e:
            _host(dict(p, theta=bad))
        assert e.value.status == -1
    for tid in (3, -2):
        with pytest.raises(H.EmsarHipError) as e:
            _host(p, block_tid=tid) if tid >= 0 else H.asymptotic_host(3, p["row_ptr"], p["col_idx"], p["theta"], block_tid=tid)
        assert e.value.status == -1
    # a gene group only partly given; gene outputs without a map
    var, gsd = np.zeros(3), np.zeros(1)
    o = H.AsymOutputs()
    o.var, o.gene_sd = H._p(var, C.c_double), H._p(gsd, C.c_double)
    args = (len(p["row_ptr"]) - 1, 3, H._p(p["row_ptr"], C.c_uint64), H._p(p["col_idx"], C.c_int32), None, None, H._p(p["theta"], C.c_double), 0, None, None)
    assert L.emsar_hip_asymptotic_host(*args, C.byref(o), None) == -1
    gst = np.zeros(1, dtype=np.int32)
    o.gene_status = H._p(gst, C.c_int32)
    assert L.emsar_hip_asymptotic_host(*args, C.byref(o), None) == -5           # ERR_STATE: no gene map
    o = H.AsymOutputs()
    o.var = H._p(var, C.c_double)
    assert L.emsar_hip_asymptotic_host(*args, C.byref(o), None) == 0 and (var > 0).all()
    assert L.emsar_hip_asymptotic_host(*args, None, None) == 0                  # nothing asked for


def test_asym_kernels_use_no_scratch():
    """the ISA listing of the build (absent where build/ is not shipped), its metadata block only: every k_asym_* kernel spills nothing
    and uses no scratch; the 256-thread class stays inside the register budget of its workgroup size (4 waves on 4 SIMDs: up to
    512 VGPRs each, but 128 keeps four workgroups' worth of waves per SIMD free for the smaller classes next to it)"""
    asm = os.path.join(_build.BUILD, "emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        pytest.skip("no ISA listing (build/ is not shipped)")
    meta = {}
    for blk in open(asm).read().split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, None])[1]
        meta[g("name")] = {k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    names = [n for n in meta if n and "k_asym_" in n]
    assert len(names) == 5, names                    # rows, single, three classes
    for n in names:
        m = meta[n]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (n, m)
    big = [n for n in names if "k_asym_setsILi256ELi256E" in n]
    assert len(big) == 1 and meta[big[0]]["vgpr_count"] <= 128, big


def test_asym_files(tmp_path):
    from emsar_amd import hostlib
    names = ["tA", "tB", "tC", "tD", "tE"]
    path = str(tmp_path / "x.asym")
    args = dict(fpkm=[3.1, 0.0, 12.5, 2.0, 7.0], tpm=[100.0, 0.0, 400.0, 64.5, 225.8], sd_fpkm=[0.5, 0.0, 2.0, math.inf, math.nan],
                sd_tpm=[16.25, 0.0, 60.0, math.inf, math.nan], var=[0.25, 0.0, 4.0, math.inf, math.nan], status=[0, 1, 0, 2, 3],
                partner=[2, -1, 0, -1, -1], partner_cov=[-0.5, math.nan, -0.5, math.nan, math.nan])
    hostlib.write_asym(path, names, **args)
    lines = open(path).read().splitlines()
    assert lines[0] == "tid\ttranscriptID\tFPKM\tsd_FPKM\tTPM\tsd_TPM\tstatus\tpartner\tpartner_corr"
    assert lines[1:] == ["0\ttA\t3.100000\t0.5\t100.000000\t16.25\tESTIMATED\ttC\t-0.5",
                         "1\ttB\t0.000000\t0\t0.000000\t0\tBOUNDARY\t-\tnan",
                         "2\ttC\t12.500000\t2\t400.000000\t60\tESTIMATED\ttA\t-0.5",
                         "3\ttD\t2.000000\tinf\t64.500000\tinf\tUNIDENTIFIABLE\t-\tnan",
                         "4\ttE\t7.000000\tnan\t225.800000\tnan\tTOO_LARGE\t-\tnan"]
    hostlib.write_asym(path, names, usage_sd=[0.125, 0.0, 0.125, math.inf, math.nan], **args)
    lines = open(path).read().splitlines()
    assert lines[0].endswith("partner_corr\tusage_sd") and [l.split("\t")[9] for l in lines[1:]] == ["0.125", "0", "0.125", "inf", "nan"]
    gpath = str(tmp_path / "x.gasym")
    hostlib.write_gasym(gpath, ["g1", "g2", "g3", "g4"], [15.6, 2.0, 7.0, 0.0], [1.75, math.inf, math.nan, 0.0], [0, 2, 4, 1])
    assert open(gpath).read().splitlines() == ["geneID\tgFPKM\tsd\tstatus", "g1\t15.600000\t1.75\tESTIMATED", "g2\t2.000000\tinf\tUNIDENTIFIABLE",
                                               "g3\t7.000000\tnan\tINFEASIBLE", "g4\t0.000000\t0\tBOUNDARY"]
    with pytest.raises(hostlib.HostError):
        hostlib.write_asym(str(tmp_path / "no" / "dir.asym"), names, **args)
