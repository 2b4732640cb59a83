"""Connected sets of an exact packed shape (n_t transcripts, n_r distinct rows, nnz entries) for the set-resident solver, shared
by test_set_edges_cpu.py (which pins every shape to its class and LDS footprint through sets_selfcheck) and test_set_edges_gpu.py
(which solves them).  sets.hpp: set_lds_bytes = 66 n_t + 26 n_r + 4 nnz + 516 rounded up to 16, classes at 6 / 48 / 156 KiB of it
and at max(n_t, n_r) of 128 / 512."""
import numpy as np


def lds_bytes(n_t, n_r, nnz):
    """set_lds_bytes of sets.hpp, restated"""
    return (66 * n_t + 26 * n_r + 4 * nnz + 516 + 15) // 16 * 16


# (n_t, n_r, nnz) -> footprint, class (3 = not resident: left to the streaming passes); pairs on either side of an edge
EDGES = [
    ((40, 80, 227), 6144, 0), ((40, 80, 228), 6160, 1),                # the 6 KiB cap
    ((18, 128, 258), 6064, 0), ((18, 129, 258), 6096, 1),              # 128 / 129 rows: raised by the one-wave limit, not by bytes
    ((250, 500, 4784), 49152, 1), ((250, 500, 4785), 49168, 2),        # the 48 KiB cap
    ((100, 512, 1100), 24832, 1), ((100, 513, 1100), 24864, 2),        # 512 / 513 rows
    ((900, 2000, 11957), 159744, 2), ((900, 2000, 11958), 159760, 3),  # the 156 KiB cap: the largest launch there is / streamed
]
STREAMED = 3
# The seed of each shape: of eight tried (100 + k + 10 j), the one whose problem the CPU oracle's EM finishes in the fewest passes --
# random weights make some of these sets boundary optima that take 10^5 passes, and the tests have to stay quick.  Nothing the device
# computes entered the choice.
SEEDS = [130, 131, 122, 113, 104, 175, 146, 107, 178, 119]


class EdgeSet:
    """One connected set: rows (tuples of distinct local ids, no two rows the same set of ids) and their weights (> 0)."""

    def __init__(self, n_t, rows, weights):
        self.n_t, self.rows, self.weights = int(n_t), [tuple(int(x) for x in r) for r in rows], [int(w) for w in weights]
        assert len(set(frozenset(r) for r in self.rows)) == len(self.rows), "rows must differ (identical rows are merged)"
        assert all(len(set(r)) == len(r) >= 2 for r in self.rows) and min(self.weights) > 0
        seen = _component(self.n_t, self.rows)
        assert seen == self.n_t, "the set must be connected"

    @property
    def shape(self):
        return self.n_t, len(self.rows), sum(len(r) for r in self.rows)


def _component(n_t, rows):
    """transcripts reachable from transcript 0 through the rows"""
    parent = list(range(n_t))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for r in rows:
        for t in r[1:]:
            parent[find(t)] = find(r[0])
    return sum(find(t) == find(0) for t in range(n_t))


def edge_set(n_t, n_r, nnz, seed):
    """Chain rows {i, i+1} (connected whatever follows), then n_r - (n_t - 1) further distinct rows of distinct ids whose lengths
    start at 2 and share the rest of nnz round-robin; weights in 1 .. 39."""
    rng = np.random.default_rng(seed)
    rows = [(i, i + 1) for i in range(n_t - 1)]
    extra = n_r - len(rows)
    rest = nnz - 2 * len(rows) - 2 * extra
    assert extra > 0 and rest >= 0
    lens = [2 + rest // extra + (1 if k < rest % extra else 0) for k in range(extra)]
    assert max(lens) <= n_t
    have = set(frozenset(r) for r in rows)
    for L in lens:
        while True:
            r = rng.choice(n_t, size=L, replace=False)
            if frozenset(int(x) for x in r) not in have:
                break
        have.add(frozenset(int(x) for x in r))
        rows.append(tuple(r))
    s = EdgeSet(n_t, rows, rng.integers(1, 40, size=len(rows)))
    assert s.shape == (n_t, n_r, nnz)
    return s


RAGGED_T = 60
RAGGED_LENS = sorted([L for L in range(2, 14) for _ in range(2)] + [17, 33], reverse=True)
# how many transcripts occur in 1, 2, .. 9 rows: 60 transcripts, 230 entries = sum(RAGGED_LENS)
RAGGED_DEGREES = {1: 8, 2: 11, 3: 11, 4: 10, 5: 7, 6: 5, 7: 4, 8: 2, 9: 2}


def ragged_set(seed=1):
    """60 transcripts, rows of every length 2 .. 13 twice plus one of 17 and one of 33, transcripts in exactly 1, 2, .. 9 rows: the
    4-way unrolled gathers of set_em_estep (over a row) and set_em_acc (over a transcript's rows) take every tail length 0 .. 3 after
    one or more full trips.  Rows are filled longest first, each from the transcripts with the most rows still to come (ties at random)."""
    rng = np.random.default_rng(seed)
    left = np.concatenate([[d] * c for d, c in RAGGED_DEGREES.items()])
    assert len(left) == RAGGED_T and left.sum() == sum(RAGGED_LENS)
    left = left[rng.permutation(RAGGED_T)]
    rows = []
    for L in RAGGED_LENS:
        order = np.lexsort((rng.random(RAGGED_T), -left))
        pick = order[:L]
        assert left[pick].min() > 0
        left[pick] -= 1
        rows.append(tuple(pick[rng.permutation(L)]))
    assert not left.any()
    s = EdgeSet(RAGGED_T, rows, rng.integers(1, 40, size=len(rows)))
    deg = np.bincount(np.concatenate([np.array(r) for r in s.rows]), minlength=RAGGED_T)
    assert sorted(set(deg)) == list(range(1, 10)) and sorted(len(r) for r in s.rows) == sorted(RAGGED_LENS)
    return s


def family(n_t, seed):
    """a small family of 2 .. 5 transcripts: the chain and one row of them all (n_t >= 3)"""
    rng = np.random.default_rng(seed)
    rows = [(i, i + 1) for i in range(n_t - 1)] + ([tuple(range(n_t))] if n_t >= 3 else [])
    return EdgeSet(n_t, rows, rng.integers(1, 40, size=len(rows)))


def compose(sets, seed=0):
    """The sets side by side under disjoint tid ranges, the caller's tids and the order of the rows shuffled -> (n_tx, rp, ci, R, E).
    Added on top of the requested shapes, so that these stay exact: copies of about 5 % of the rows with E = 0 (outside the
    likelihood: no part of any set) and, for about 10 % of the transcripts, a single-transcript row (folded into the transcript's own
    count, no row of a set).  E is uniform in [0.5, 2] elsewhere."""
    return compose_members(sets, seed)[:5]


def compose_members(sets, seed=0):
    """compose, and the membership: -> (n_tx, rp, ci, R, E, members), members[k] = (tids, rows) of sets[k] in the caller's numbering --
    its transcripts in the order of the set's local ids, and every row that holds one of them (ascending): the rows of the shape, their
    E = 0 copies and the single-transcript rows."""
    rng = np.random.default_rng(seed)
    rows, R, base, bases = [], [], 0, []
    for s in sets:
        rows += [tuple(base + t for t in r) for r in s.rows]
        R += s.weights
        bases.append(base)
        base += s.n_t
    n_tx, n_shape = base, len(rows)
    E = list(rng.uniform(0.5, 2.0, size=n_shape))
    for k in rng.choice(n_shape, size=max(1, n_shape // 20), replace=False):
        rows.append(rows[k])
        R.append(int(rng.integers(1, 40)))
        E.append(0.0)
    for t in rng.choice(n_tx, size=max(1, n_tx // 10), replace=False):
        rows.append((int(t),))
        R.append(int(rng.integers(1, 40)))
        E.append(float(rng.uniform(0.5, 2.0)))
    shuffle = rng.permutation(n_tx)
    order = rng.permutation(len(rows))
    rows = [rows[k] for k in order]
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = shuffle[np.concatenate([np.array(r, dtype=np.int64) for r in rows])].astype(np.int32)
    set_of_row = np.searchsorted(np.array(bases + [n_tx]), np.array([r[0] for r in rows]), side="right") - 1
    members = [(shuffle[b:b + s.n_t].astype(np.int64), np.flatnonzero(set_of_row == k)) for k, (s, b) in enumerate(zip(sets, bases))]
    return n_tx, rp, ci, np.array(R, dtype=np.int32)[order], np.array(E)[order], members


_cache = {}


def edge_problem(k):
    """EDGES[k] alone, as compose returns it"""
    if ("edge", k) not in _cache:
        _cache["edge", k] = compose([edge_set(*EDGES[k][0], seed=SEEDS[k])], seed=200 + k)
    return _cache["edge", k]


def ragged_problem():
    if "ragged" not in _cache:
        _cache["ragged"] = compose([ragged_set()], seed=7)
    return _cache["ragged"]


def resident_sets():
    """every resident edge shape and the ragged set, small families before and between them (no descriptor offset is 0 but the first)"""
    out = [family(3, 1), family(2, 2)]
    for k, (shape, _, cls) in enumerate(EDGES):
        if cls != STREAMED:
            out += [edge_set(*shape, seed=SEEDS[k]), family(2 + k % 4, 10 + k)]
    return out + [ragged_set(), family(5, 3)]


def all_resident_problem():
    if "resident" not in _cache:
        _cache["resident"] = compose(resident_sets(), seed=16)      # of seeds 11 .. 30 the quickest for the oracle solving it as one problem
    return _cache["resident"]


def all_resident_members():
    """all_resident_problem() with the membership of its sets (compose_members)"""
    if "resident_members" not in _cache:
        _cache["resident_members"] = compose_members(resident_sets(), seed=16)
    return _cache["resident_members"]


def everything_problem():
    """all ten edge shapes (the streamed one too) and the ragged set"""
    if "everything" not in _cache:
        _cache["everything"] = compose([edge_set(*shape, seed=SEEDS[k]) for k, (shape, _, _) in enumerate(EDGES)] + [ragged_set()], seed=12)
    return _cache["everything"]
