"""CPU: the recipe of tests/quant_shape_problems.py holds -- the replicate counts reach every tile shape of the quantile kernels and
both LDS sizes, the lattice's 71 transcripts and 27 genes leave a partial last tile at every C > 1, and at every B the predicted
replicates (bootstrap_draw_host and the closed form) contain what tests/test_quant_shapes_gpu.py relies on: replicates that draw nothing,
all-zero columns, ties and no ties around the median, genes whose sum is zero in some replicates only.  No GPU needed."""
import numpy as np
import pytest

from tests import quant_shape_problems as P
from tests.test_bootstrap_cpu import inversion
from tests.test_genes_gpu import chunked_sums


def test_tile_rule_reaches_every_shape():
    tiles = {B: P.tile_of(B) for B in P.BS}
    assert {C for _, C, _ in tiles.values()} == {32, 16, 8, 4, 2, 1}
    assert {lds for _, _, lds in tiles.values()} == {16384, 32768}
    assert set(P.B_EDGES) <= set(P.BS) and {100, 1000} <= set(P.BS) and max(P.BS) == 4096
    for B, (Bp, C, lds) in tiles.items():
        assert Bp >= B > Bp // 2 and Bp & (Bp - 1) == 0 and lds == 8 * Bp * C <= 32768
    # both edges of every padded size from 64 to 4096, and the rule at the sizes the existing tests use
    assert sorted({Bp for Bp, _, _ in tiles.values()}) == [64, 128, 256, 512, 1024, 2048, 4096]
    for Bp in (64, 128, 256, 512, 1024, 2048):
        assert P.tile_of(Bp)[0] == Bp and P.tile_of(Bp + 1)[0] == 2 * Bp and Bp in P.BS and Bp + 1 in P.BS
    assert P.tile_of(1) == (1, 32, 256) and P.tile_of(20) == (32, 32, 8192) and P.tile_of(100) == (128, 16, 16384)
    assert P.tile_of(2048) == (2048, 1, 16384) and P.tile_of(4096) == (4096, 1, 32768)


def test_probabilities():
    from tests.test_bootq_gpu import Q
    assert P.Q5 == Q
    q = P.Q67
    assert len(P.Q1) == 1 and len(q) == 67 and len(set(q.tolist())) == 67 and np.all(np.diff(q) > 0)
    assert q[0] == 0.0 and q[1] == np.nextafter(0.0, 1.0) and q[-2] == np.nextafter(1.0, 0.0) and q[-1] == 1.0
    assert set(Q + [0.25, 0.75]) <= set(q.tolist())
    for C in (32, 16, 8, 4, 2, 1):                  # the read-out loop ends inside a round of 256 lanes at every shape
        assert (len(q) * C) % 256 != 0 and (len(P.Q1) * C) % 256 != 0


def test_lattice_is_as_described():
    p = P.lattice()
    assert p.n_tx == 71 and p.ng == 27 and p.n_rows == 100 and set(p.R.tolist()) == set(P.CYCLE) and p.R.max() <= 16
    rows_of = np.bincount(p.col_idx, minlength=p.n_tx)
    assert set(rows_of[:67].tolist()) == {1, 2} and not rows_of[67:].any()
    assert np.all(np.diff(p.row_ptr.astype(np.int64)) == 1)
    assert p.E.min() >= 0.5 and p.E.max() <= 2.0 and np.all(p.den[:67] > 0) and not p.den[67:].any()
    for C in (32, 16, 8, 4, 2):
        assert p.n_tx % C != 0 and p.ng % C != 0, C
    n_iso = np.bincount(p.gmap[p.gmap >= 0], minlength=p.ng)
    assert set(n_iso.tolist()) == {0, 1, 2, 3} and (n_iso == 0).sum() == 1 and n_iso[26] == 0
    assert np.all(p.gmap[5:67:11] == -1) and (p.gmap < 0).sum() == 7
    reads = np.bincount(p.col_idx, weights=p.R, minlength=p.n_tx)
    per_gene = np.bincount(p.gmap[p.gmap >= 0], weights=reads[p.gmap >= 0], minlength=p.ng)
    # genes of zero-read transcripts only: 25 (three transcripts in no row) and 0 (transcript 0 alone: a row, no reads)
    assert per_gene[25] == 0 and n_iso[25] == 3 and per_gene[0] == 0 and n_iso[0] == 1 and (per_gene[1:25] > 0).all()
    assert ((reads[:67] == 0) & (rows_of[:67] > 0)).sum() == 10                       # transcripts with rows and no reads
    assert sorted(P.LATTICE_SEED) == list(P.BS)


def test_sparse_draws_by_the_python_restatement():
    """Every draw of `sparse` (R = 1) from the pure-Python Philox and inversion of tests/test_bootstrap_cpu.py: the replicates that
    draw nothing, counted."""
    p = P.sparse()
    assert p.n_tx == 5 and p.R.tolist() == [1, 1, 1] and p.col_idx.tolist() == [0, 1, 2] and p.gmap.tolist() == [0, 0, 1, -1, 2]
    assert p.den.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]
    want = np.array([[inversion(21, b, row, 1) for row in range(3)] for b in range(4096)], dtype=np.int32)
    assert np.array_equal(P.draws("sparse", 21, 4096), want)
    empty = ~want.any(axis=1)
    assert empty[:33].sum() == 2 and empty[:100].sum() == 9 and empty.sum() == 200
    first = np.array([[inversion(1, b, row, 1) for row in range(3)] for b in range(33)], dtype=np.int32)
    assert np.array_equal(P.draws("sparse", 1, 33), first) and (~first.any(axis=1)).any()


@pytest.mark.parametrize("B", P.BS)
def test_sparse_has_empty_and_non_empty_replicates(B):
    for seed in (1, 21):
        d = P.draws("sparse", seed, B)
        assert d.shape == (B, 3)
        empty = ~d.any(axis=1)
        assert empty.any() and not empty.all(), (B, seed)
        reps = P.predicted_replicates("sparse", seed, B)
        assert np.array_equal(reps[:, :3], d.astype(np.float64)) and not reps[:, 3:].any()
        assert np.array_equal(reps.sum(axis=1) == 0, empty)
        G = chunked_sums(reps, P.sparse().gmap, 3)
        assert (G[:, 0] == 0).any() and (G[:, 0] > 0).any() and not G[:, 2].any()       # G = 0 usage in some replicates; always


@pytest.mark.parametrize("B", P.BS)
def test_lattice_columns(B):
    p = P.lattice()
    reps = P.predicted_replicates("lattice", P.LATTICE_SEED[B], B)
    assert reps.shape == (B, 71) and np.isfinite(reps).all() and reps.min() == 0.0
    d = P.draws("lattice", P.LATTICE_SEED[B], B)
    t = 13                                                  # two rows of R = 16
    rows = np.nonzero(p.col_idx == t)[0]
    assert len(rows) == 2 and np.array_equal(reps[:, t], (d[:, rows[0]].astype(np.float64) + d[:, rows[1]]) / p.den[t])
    assert (~reps.any(axis=0)).any()                        # an all-zero column
    lo, hi = P.median_pair(reps)
    assert ((lo == hi) & (hi > 0)).any()                    # a column whose two order statistics around the median are equal (and not 0)
    assert (lo != hi).any()                                 # and one where they differ
    G = chunked_sums(reps, p.gmap, p.ng)
    zero = G == 0
    assert (zero.any(axis=0) & ~zero.all(axis=0)).any()     # a gene whose sum is 0 in some replicates and not in others
    assert zero[:, 25].all() and zero[:, 26].all()
