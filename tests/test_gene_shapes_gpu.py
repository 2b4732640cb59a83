"""GPU: emsar_hip_compare, emsar_hip_compare_genes, emsar_hip_profile_genes and emsar_hip_compare_usage against their numpy references
off the diagonal of the size classes (tests/gene_shape_problems.py): a small set in a large launch (EDGES[1], [2], [3], [5], [6], [7]),
the ragged set, a 256 launch that goes over 300 transcripts twice with members of the gene on either side of local id 256, a 512 launch
that solves a 256-class part, a gene with parts in all three classes and a lone transcript, a gene with nine set parts per sample, a 256
launch with two 64-class parts, and a gene whose class-2 member has den = 0 in one sample only -- in both sample orders, under CSR
against TILED with the library's numbering and merged rows, with one item per launch, and with the contexts untouched by each call.

The loading and checking are those of the three gene GPU tests, unchanged (load, config, check_against), and so are their tolerances:
    compare         dev_tol + 8 e_F                                       (test_compare_gpu.TOL)
    compare_genes   dev_tol + 4 P e_F + w_ref                             (test_compare_genes_gpu.tol_of)
    profile_genes   100 SPREAD (|F_hat| + |F_pinned|) + 1e-7 q + 4 P e_F  (test_profile_genes_gpu.check_against)
    compare_usage   3 dev_tol + 4 P e_F + w_ref                           (test_compare_usage_gpu.tol_of)
e_F = 4 x 9.4e-10 was measured on the three class problems; on the problems of this file the largest |F(solve's theta) - F_ref| over
the parts, F in numpy at the theta of emsar_hip_solve (tol 1e-12) against the plain EM at 1e-13, is E_F_HERE below (DESIGN.md "Pinned
since" has the figure per problem): not above 9.4e-10, so the constant is kept.

The statistics of the calls count launched items, not launches per class: the launch class that was meant is pinned on the host
(test_gene_shapes_cpu.py: the classes of every gene's parts as the library packs them), and here by items_launched and parts.

Every call passes max_iter <= 20000 and the default search caps, and den is computed on the host (CP.den_of)."""
import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import gene_shape_problems as SH
from tests import test_compare_genes_gpu as TG
from tests import test_compare_gpu as TC
from tests import test_compare_usage_gpu as TU
from tests import test_profile_genes_gpu as TPG
from tests.test_compare_genes_gpu import config, load

pytestmark = pytest.mark.gpu

E_F_HERE = 4.7e-10           # measured (4.66e-10, EDGES[5] under sample A); <= test_compare_gpu.E_F_MEASURED: the shared constants hold here
CAPS = dict(max_iter=20000)
assert E_F_HERE <= TC.E_F_MEASURED


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b:
        yield a, b


def genes_of(name):
    """the gene map a case is loaded with and the case's gene id in it: the problem's genes in a fixed order"""
    p = SH.problem(name)
    order = list(SH.MIX_GENES) if "g_many" in p["genes"] else ["gene"]
    return [p["genes"][g] for g in order], order.index(name.partition(":")[2] or "gene")


def load_pair(devs, name, swap=False):
    a, b = devs
    prob, RA, RB, den_a, den_b, members, t = SH.case(name)
    genes, g = genes_of(name)
    if swap:
        RA, RB, den_a, den_b = RB, RA, den_b, den_a
    load(a, prob, RA, den_a, genes)
    load(b, prob, RB, den_b)
    return g, t


# ---- 1. the transcript test --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SH.COMPARE_CASES)
def test_compare_against_the_reference(devs, name):
    a, b = devs
    load_pair(devs, name)
    tids = SH.problem(name)["tids"]
    r = a.compare(b, tids, tol=1e-12, **CAPS)
    for i, t in enumerate(tids):
        ref = SH.compare_reference(name, t)
        print(name, t, "Lambda", r["lambda"][i], "ref", ref["lam"], "residual", r["lambda"][i] - ref["lam"], "tol", TC.TOL, "evals", r["evals"][i])
        assert ref["lam"] > 0.0
        assert r["status"][i] == TC.TESTED, (name, t, r["status"][i])
        assert abs(r["lambda"][i] - ref["lam"]) <= TC.TOL, (name, t, r["lambda"][i], ref["lam"])
    st = r["stats"].as_dict()
    assert st["items_launched"] == len(tids) and st["n_status"]["TESTED"] == len(tids)


# ---- 2. the gene-level two-sample test -----------------------------------------------------------------------------------------------------
def swapped(ref):
    """H0 at ratio 1 is symmetric: (B, A) has the reference of (A, B) with the gene sums exchanged"""
    return dict(ref, gene_a=ref["gene_b"], gene_b=ref["gene_a"], multiplier=-ref["multiplier"])


@pytest.mark.parametrize("swap", [False, True], ids=["A,B", "B,A"])
@pytest.mark.parametrize("name", SH.GENE_CASES)
def test_compare_genes_against_the_reference(devs, name, swap):
    a, b = devs
    g, _ = load_pair(devs, name, swap)
    ref = SH.recorded()["gene"][name]
    r = a.compare_genes(b, [g], tol=1e-12, **CAPS)
    TG.check_against(r, 0, swapped(ref) if swap else ref, (name, "B, A" if swap else "A, B"))
    st = r["stats"].as_dict()
    print(st)
    assert st["items_launched"] == 1 and st["parts_max"] == ref["parts"] and st["n_status"]["TESTED"] == 1


# ---- 3. the gene profile and the gene presence test ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SH.PROFILE_CASES)
def test_profile_genes_against_the_reference(devs, name):
    a, _ = devs
    prob, R, den, members = SH.profile_case(name)
    genes, g = genes_of(name)
    load(a, prob, R, den, genes)
    r = a.profile_genes([g], level=0.95, tol=1e-12, **CAPS)
    print(name, {k: r[k] for k in TPG.OUTPUTS})
    TPG.check_against(r, 0, SH.profile_gene(name), TPG.q_of(0.95), name)
    st = r["stats"].as_dict()
    assert st["items_launched"] == (3 if r["status"][0] == TPG.TWO_SIDED else 2) and st["parts_max"] == SH.profile_gene(name).n_parts


# ---- 4. the usage test -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SH.USAGE_CASES)
def test_compare_usage_against_the_reference(devs, name):
    a, b = devs
    _, t = load_pair(devs, name)
    ref = SH.recorded()["usage"][name]
    r = a.compare_usage(b, [t], tol=1e-12, **CAPS)
    TU.check_against(r, 0, ref, name)
    st = r["stats"].as_dict()
    print(st)
    assert st["items_launched"] == 1 and st["parts_max"] == ref["parts"]


# ---- 5. 6. bit-identity on the class mix, the contexts untouched ---------------------------------------------------------------------------------
CALLS = {
    "compare_genes": (lambda a, b, q: a.compare_genes(b, **CAPS), "EMSAR_HIP_COMPARE_GENES_BATCH", TG.OUTPUTS),
    "profile_genes": (lambda a, b, q: a.profile_genes(**CAPS), "EMSAR_HIP_PROFILE_GENES_BATCH", TPG.OUTPUTS),
    "compare_usage": (lambda a, b, q: a.compare_usage(b, q, **CAPS), "EMSAR_HIP_COMPARE_USAGE_BATCH", TU.OUTPUTS),
}


@pytest.mark.parametrize("call", list(CALLS))
def test_class_mix_bit_for_bit(devs, monkeypatch, call):
    """every gene of the class mix queried (the usage test: every member of every gene): CSR against TILED in the library's numbering
    with merged rows, against one item per class and launch; a solve of either context returns the same bits before and after"""
    a, b = devs
    run, batch_var, outputs = CALLS[call]
    p = SH.mix_problem()
    prob, genes = p["prob"], [p["genes"][g] for g in SH.MIX_GENES]
    q = np.array(sorted(t for g in genes for t in g), dtype=np.int32)
    config(monkeypatch, a, prob, p["RA"], p["den_a"], genes, H.LAYOUT_CSR, False, None)
    config(monkeypatch, b, prob, p["RB"], p["den_b2"], genes, H.LAYOUT_CSR, False, None)
    before = [a.solve(**CAPS)[0], b.solve(**CAPS)[0]]
    whole = run(a, b, q)
    after = [a.solve(**CAPS)[0], b.solve(**CAPS)[0]]
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    st = whole["stats"].as_dict()
    print(call, st)
    assert st["parts_max"] >= (9 if call == "profile_genes" else 18) and st["items_launched"] >= len(genes)
    monkeypatch.setenv(batch_var, "1")
    single = run(a, b, q)
    monkeypatch.delenv(batch_var)
    assert not [k for k in outputs if single[k].tobytes() != whole[k].tobytes()]
    config(monkeypatch, a, prob, p["RA"], p["den_a"], genes, H.LAYOUT_TILED, True, "2")      # asserts info().renumbered == 1
    config(monkeypatch, b, prob, p["RB"], p["den_b2"], genes, H.LAYOUT_TILED, True, "2")
    tiled = run(a, b, q)
    assert not [k for k in outputs if tiled[k].tobytes() != whole[k].tobytes()]
