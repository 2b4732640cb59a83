"""CPU: what the problems of tests/gene_shape_problems.py hold, pinned on the host -- the class of every set as the library packs it, the
stored rows, that nothing is streamed, the footprint of the two-trip shape, for every gene the set parts per sample and their classes as
GP.parts_of finds them (and with them the launch class that test_gene_shapes_gpu.py means: the largest), and the conditions every
reference has to meet before the device is compared with it: w_ref <= 1e-7, one peak, Lambda > 0, and both statuses of the gene profile
among its cases.  No case is left out for failing one."""
import math

import numpy as np
import pytest

from emsar_amd.hip import sets_selfcheck
from tests import compare_gene_problems as GP
from tests import gene_shape_problems as SH
from tests import set_problems as SP

CUT95 = 3.841458820694124


def selfcheck(prob, R):
    n_tx, rp, ci, _, E = prob
    d = sets_selfcheck(n_tx, rp, ci, np.where(E != 0, R, 0).astype(np.int32))
    assert d["tids_closed"] + d["tids_resident"] + d["tids_streamed"] == n_tx and d["sets_cluster"] == 0
    return d


def one_hot(cls):
    return [int(c == cls) for c in range(3)]


@pytest.mark.parametrize("k", SH.A_EDGES)
def test_edge_problems(k):
    (n_t, n_r, nnz), bytes_, cls = SP.EDGES[k]
    p = SH.edge_problem(k)
    assert p["prob"][0] == n_t and [int(t) for t in p["local"][[0, 7, 3]]] == p["genes"]["gene"] and p["tids"] == p["genes"]["gene"][:2]
    assert p["t"]["gene"] == p["tids"][0]
    for R in (p["RA"], p["RB"]):
        d = selfcheck(p["prob"], R)
        assert d["sets_resident"] == one_hot(cls) and d["sets_streamed"] == 0 and d["rows_stored"] == n_r and d["tids_resident"] == n_t
        assert d["max_lds_bytes"] == [bytes_ * x for x in one_hot(cls)]
    # a small set in a large launch: most threads of the launch hold no transcript, or the class comes from the rows alone
    assert n_t < (64, 256, 512)[cls]


def test_ragged_problem():
    p = SH.ragged_problem()
    assert p["prob"][0] == SP.RAGGED_T and len(p["genes"]["gene"]) == 3 and p["tids"] == p["genes"]["gene"][:2] and p["t"]["gene"] == p["tids"][0]
    rows = SH.AP.rows_of(p["prob"])
    for t in p["genes"]["gene"]:                      # each member has a row of its own with E > 0: its estimate is unique
        assert any(r == (t,) and e > 0 for r, e in zip(rows, p["prob"][4]))
    for R in (p["RA"], p["RB"]):
        d = selfcheck(p["prob"], R)
        assert d["sets_resident"] == [1, 0, 0] and d["sets_streamed"] == 0 and d["rows_stored"] == 26
        assert d["max_lds_bytes"] == [SP.lds_bytes(60, 26, 230), 0, 0]


def test_two_trips_problem():
    n_t, n_r, nnz = SH.TWO_TRIPS_SHAPE
    assert SP.lds_bytes(n_t, n_r, nnz) == 30944 and 6144 < 30944 <= 49152 and 256 < n_t <= 512 and n_r <= 512
    p = SH.two_trips_problem()
    # one set of all the tids: the library's local id of a transcript (ascending tid within its set) is its tid
    assert p["prob"][0] == n_t and p["genes"]["gene"] == list(SH.TWO_TRIPS_GENE) and p["tids"] == list(SH.TWO_TRIPS_TESTED)
    assert min(p["genes"]["gene"]) < 256 < max(p["genes"]["gene"]) and sum(t >= 256 for t in p["genes"]["gene"]) == 2
    assert p["tids"][1] >= 256 and p["t"]["gene"] == p["tids"][1] and set(p["tids"]) <= set(p["genes"]["gene"])
    for R in (p["RA"], p["RB"]):
        d = selfcheck(p["prob"], R)
        assert d["sets_resident"] == [0, 1, 0] and d["sets_streamed"] == 0 and d["rows_stored"] == n_r and d["tids_resident"] == n_t
        assert d["max_lds_bytes"] == [0, 30944, 0]


def test_mix_problem():
    p = SH.mix_problem()
    sets = SH.mix_sets()
    assert len(sets) == len(SH.MIX_SETS) == len(SH.MIX_CLASSES)
    counts = [SH.MIX_CLASSES.count(c) for c in range(3)]
    assert counts == [6, 2, 1]
    caps = [max(SP.lds_bytes(*s.shape) for s, c in zip(sets, SH.MIX_CLASSES) if c == cls) for cls in range(3)]
    assert caps == [SP.EDGES[0][1], SP.EDGES[1][1], SP.EDGES[7][1]]
    for R in (p["RA"], p["RB"], p["RL"]):
        d = selfcheck(p["prob"], R)
        assert d["sets_resident"] == counts and d["sets_streamed"] == 0 and d["tids_closed"] == 1 and d["n_components"] == len(sets)
        assert d["rows_stored"] == sum(len(s.rows) for s in sets) and d["max_lds_bytes"] == caps
    members = [t for g in p["genes"].values() for t in g]
    assert len(set(members)) == len(members)             # a transcript has one gene
    home = {int(t): k for k, (tids, _) in enumerate(p["members"]) for t in tids}
    assert [SH.MIX_CLASSES[home[t]] for t in p["genes"]["g512_256"]] == [2, 1]
    assert [SH.MIX_CLASSES[home[t]] for t in p["genes"]["g_three"][:3]] == [0, 1, 2] and p["genes"]["g_three"][3] == p["alone"]
    assert sorted(home[t] for t in p["genes"]["g_many"]) == list(range(len(sets)))
    assert [SH.MIX_SETS[home[t]] for t in p["genes"]["g256_64x2"]] == ["edge0", "edge2", "edge1"]
    # the second pair: den = 0 in sample B for g_three's class-2 member alone
    off = np.flatnonzero(p["den_b2"] != p["den_a"])
    assert list(off) == [p["genes"]["g_three"][2]] and p["den_b2"][off[0]] == 0.0 and p["den_b"] is p["den_a"]


# the classes of the set parts of every gene per sample (sorted), and the closed-form parts per sample
PARTS = {
    "edge1": ([1], [1], 0), "edge2": ([0], [0], 0), "edge3": ([1], [1], 0), "edge5": ([2], [2], 0), "edge6": ([1], [1], 0), "edge7": ([2], [2], 0),
    "ragged": ([0], [0], 0), "two_trips": ([1], [1], 0),
    "mix:g512_256": ([1, 2], [1, 2], 0),
    "mix:g_three": ([0, 1, 2], [0, 1, 2], 1),
    "mix:g_many": ([0] * 6 + [1, 1, 2], [0] * 6 + [1, 1, 2], 0),
    "mix:g256_64x2": ([0, 0, 1], [0, 0, 1], 0),
    "mix2:g_three": ([0, 1, 2], [0, 1], 1),
}


@pytest.mark.parametrize("name", SH.GENE_CASES)
def test_parts_and_classes_of_every_gene(name):
    prob, RA, RB, den_a, den_b, members, t = SH.case(name)
    want_a, want_b, closed = PARTS[name]
    total = 0
    for R, den, want in ((RA, den_a, want_a), (RB, den_b, want_b)):
        assert sorted(SH.part_classes(prob, R, den, members)) == want, name
        parts = GP.parts_of(prob, R, den, members)
        assert len(parts) == len(want) + closed and sum(len(p.tids) == 1 for p in parts) == closed
        total += len(parts)
    assert total == SH.recorded()["gene"][name]["parts"]
    assert t in members and den_a[t] > 0 and den_b[t] > 0


def test_the_matrix_is_covered():
    """every (launch class, part class) cell at or below the diagonal holds a gene case, two-sample and single-sample alike"""
    two, one = set(), set()
    for name in SH.GENE_CASES:
        a, b, _ = PARTS[name]
        two |= {(max(a + b), c) for c in a + b}
        one |= {(max(s), c) for s in (a, b) for c in s}
    cells = {(l, c) for l in range(3) for c in range(l + 1)}
    assert two == cells and one == cells
    assert max(len(PARTS[n][0]) for n in SH.GENE_CASES) >= 8
    assert set(SH.USAGE_CASES) <= set(SH.GENE_CASES) and {"edge1", "edge3", "edge6", "ragged", "two_trips", "mix:g512_256", "mix:g_three", "mix:g_many",
                                                             "mix2:g_three"} <= set(SH.USAGE_CASES)


def test_recorded_references():
    """what the GPU tests compare with: every named case is there and meets its conditions; one entry of each kind again, bit for bit"""
    rec = SH.recorded()
    assert set(rec["gene"]) == set(SH.GENE_CASES) and set(rec["usage"]) == set(SH.USAGE_CASES)
    for name, ref in rec["gene"].items():
        print("gene", name, ref)
        assert ref["w_ref"] <= SH.W_REF_MAX and ref["lam"] > 0.0 and math.isfinite(ref["lam"]), name
    for name, ref in rec["usage"].items():
        print("usage", name, ref)
        assert ref["w_ref"] <= SH.W_REF_MAX and ref["peaks"] == 1 and ref["lam"] > 0.0 and math.isfinite(ref["lam"]), name
    assert rec["gene"]["two_trips"]["lam"] > CUT95
    for name in ("edge3", "mix:g256_64x2"):
        again = SH.kept("gene", SH.gene_reference(name))
        assert again == rec["gene"][name], (name, again, rec["gene"][name])
    again = SH.kept("usage", SH.usage_reference("edge3"))
    assert again == rec["usage"]["edge3"], (again, rec["usage"]["edge3"])


def test_transcript_references():
    """CP.reference of the two queried transcripts of every problem of the transcript test: Lambda > 0"""
    for name in SH.COMPARE_CASES:
        for t in SH.problem(name)["tids"]:
            ref = SH.compare_reference(name, t)
            print(name, t, ref["lam"], ref["passes"])
            assert ref["lam"] > 0.0 and math.isfinite(ref["lam"]) and max(ref["passes"]) < 200000


def test_both_profile_statuses_occur():
    """the reference's gene presence Lambda on either side of the 0.95 cut: TWO_SIDED and LOWER_ZERO are both judged on the device"""
    lams = {name: SH.presence_lambda(name) for name in SH.PROFILE_CASES}
    print(lams)
    assert all(v > 0.0 for v in lams.values())
    assert lams["mixlow:g256_64x2"] < CUT95 and sum(v > CUT95 for v in lams.values()) >= 10
    assert any(math.isinf(v) for v in lams.values()) and any(CUT95 < v < math.inf for v in lams.values())
