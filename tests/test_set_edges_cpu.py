"""CPU: the shapes of tests/set_problems.py sit where test_set_edges_gpu.py needs them -- each at its edge of a size class of the
set-resident solver (sets.hpp: set_lds_bytes against 6 / 48 / 156 KiB, max(n_t, n_r) against 128 and 512), number for number.
A change to set_lds_bytes or to the class rule that moves an edge fails here, not silently in the interior of a class on the GPU."""
import numpy as np
import pytest

from emsar_amd.hip import sets_selfcheck
from tests import set_problems as SP


def selfcheck(problem):
    n_tx, rp, ci, R, E = problem
    d = sets_selfcheck(n_tx, rp, ci, np.where(E != 0, R, 0).astype(np.int32))     # upload_sample's rule: E = 0 rows weigh 0
    assert d["tids_closed"] + d["tids_resident"] + d["tids_streamed"] == n_tx and d["sets_cluster"] == 0
    return d


def test_the_formula_is_the_one_of_the_table():
    for (n_t, n_r, nnz), bytes_, _ in SP.EDGES:
        assert SP.lds_bytes(n_t, n_r, nnz) == bytes_


@pytest.mark.parametrize("k", range(len(SP.EDGES)), ids=["%dx%dx%d" % e[0] for e in SP.EDGES])
def test_each_edge_shape_alone(k):
    (n_t, n_r, nnz), bytes_, cls = SP.EDGES[k]
    n_tx, rp, ci, R, E = SP.edge_problem(k)
    assert n_tx == n_t
    d = selfcheck(SP.edge_problem(k))
    assert d["n_components"] == 1 and d["tids_closed"] == 0
    if cls == SP.STREAMED:
        assert d["sets_resident"] == [0, 0, 0] and d["sets_streamed"] == 1 and d["tids_streamed"] == n_t
        assert d["max_lds_bytes"] == [0, 0, 0] and d["rows_stored"] == 0
    else:
        want = [0, 0, 0]
        want[cls] = 1
        assert d["sets_resident"] == want and d["sets_streamed"] == 0 and d["tids_resident"] == n_t
        assert d["max_lds_bytes"] == [bytes_ if c == cls else 0 for c in range(3)]
        assert d["rows_stored"] == n_r
        assert d["rows_in"] == n_r                       # the E = 0 copies and the single-transcript rows are no rows of the set


def test_ragged_set():
    s = SP.ragged_set()
    n_t, n_r, nnz = s.shape
    assert (n_t, n_r, nnz) == (60, 26, 230)
    lens = sorted(len(r) for r in s.rows)
    assert all(lens.count(L) >= 2 for L in range(2, 14)) and 17 in lens and 33 in lens
    deg = np.bincount(np.concatenate([np.array(r) for r in s.rows]), minlength=n_t)
    assert set(deg) == set(range(1, 10))
    # both gathers: every tail length 0 .. 3 after at least one full trip of four
    assert {L % 4 for L in lens if L >= 4} == {0, 1, 2, 3} and {int(x) % 4 for x in deg if x >= 4} == {0, 1, 2, 3}
    d = selfcheck(SP.ragged_problem())
    assert d["sets_resident"] == [1, 0, 0] and d["rows_stored"] == n_r and d["tids_resident"] == n_t
    assert d["max_lds_bytes"] == [SP.lds_bytes(n_t, n_r, nnz), 0, 0]


def test_composed_problems():
    counts = [sum(1 for e in SP.EDGES if e[2] == c) for c in range(3)]
    assert counts == [2, 4, 3]
    caps = [max(e[1] for e in SP.EDGES if e[2] == c) for c in range(3)]
    assert caps == [6144, 49152, 159744]
    # every edge shape and the ragged set
    d = selfcheck(SP.everything_problem())
    assert d["sets_resident"] == [counts[0] + 1, counts[1], counts[2]] and d["sets_streamed"] == 1
    assert d["max_lds_bytes"] == caps
    assert d["tids_streamed"] == 900 and d["tids_closed"] == 0
    assert d["rows_stored"] == sum(e[0][1] for e in SP.EDGES if e[2] != SP.STREAMED) + 26
    # the resident shapes with small families before and between them (what test_set_edges_gpu.py solves and resamples)
    sets = SP.resident_sets()
    fam = [s for s in sets if s.n_t <= 5]
    assert len(fam) >= 5 and {s.n_t for s in fam} == {2, 3, 4, 5}
    d = selfcheck(SP.all_resident_problem())
    assert d["sets_resident"] == [counts[0] + 1 + len(fam), counts[1], counts[2]] and d["sets_streamed"] == 0
    assert d["max_lds_bytes"] == caps and d["tids_closed"] == 0
    assert d["n_components"] == len(sets) and d["rows_stored"] == sum(len(s.rows) for s in sets)
