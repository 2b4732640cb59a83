"""Matrices and layout-knob settings shared by the TILED pass-kernel tests (test_pass_kernel_shapes.py on the CPU,
test_pass_kernels_gpu.py on the GPU).  Small: each is laid out in well under a second."""
import numpy as np

from emsar_amd import synth

KFARMAX = 3 * (256 - 960 // 16)        # layout_tiled.hpp kFarMax with 4-slot blocks: far entries one dictionary can hold
KMAXROWLEN = 4 * 60 - 3                # layout_tiled.hpp kMaxRowLen: longer rows go to the leftover CSR
LAYOUT_KNOBS = ("TILED_MULTI", "WEIGHTED_UNIT", "TILE_BLOCK", "SHORT_ECNT", "SHORT_BLOCK", "TILE_ROWS", "UNIT_TILES", "UNIT_TILES_MAX",
                "UNIT_FAR_SOFT", "UNIT_SORT", "UNIT_LPT", "TILE_CUT", "TILE_ANCHOR", "TILE_DENSE", "TAIL_SPLIT")

# The TILED branch of launch_pass as data: variant -> knobs -> which of R / E the sample carries, merged rows -> the kernel of a
# plain pass and of a likelihood pass (MODE_EM = 0, MODE_EM_LL = 1).  Below 2048 tiles (every matrix here) TILED_MULTI = 1, the
# default, picks what 0 picks; above, what 5 picks (test_pass_kernels_gpu.py: test_production_dispatch_above_the_pair_threshold).
# test_pass_dispatch_cpu.py holds the last two columns against the library's own chooser.
VARIANTS = {
    "tiled":        (dict(TILED_MULTI="0"), "", False, "k_pass_tiled<false, 0>", "k_pass_tiled<false, 1>"),
    "multi2":       (dict(TILED_MULTI="2"), "", False, "k_pass_tiled_multi<false, 0, 2>", "k_pass_tiled_multi<false, 1, 2>"),
    "multi3":       (dict(TILED_MULTI="3"), "", False, "k_pass_tiled_multi<false, 0, 3>", "k_pass_tiled_multi<false, 1, 3>"),
    "multi4":       (dict(TILED_MULTI="4"), "", False, "k_pass_tiled_multi<false, 0, 4>", "k_pass_tiled_multi<false, 1, 4>"),
    "unit":         (dict(TILED_MULTI="5"), "", False, "k_pass_tiled_unit<false, 0>", "k_pass_tiled_unit<false, 1>"),
    "tiled_R":      (dict(TILED_MULTI="0"), "R", False, "k_pass_tiled<true, 0>", "k_pass_tiled<true, 1>"),
    "tiled_E":      (dict(TILED_MULTI="0"), "E", False, "k_pass_tiled<true, 0>", "k_pass_tiled<true, 1>"),
    "tiled_RE":     (dict(TILED_MULTI="0"), "RE", False, "k_pass_tiled<true, 0>", "k_pass_tiled<true, 1>"),
    "unit_wu0":     (dict(TILED_MULTI="5", WEIGHTED_UNIT="0"), "RE", False, "k_pass_tiled<true, 0>", "k_pass_tiled<true, 1>"),
    "unit_wu1":     (dict(TILED_MULTI="5", WEIGHTED_UNIT="1"), "RE", False, "k_pass_tiled_unit<true, 0>", "k_pass_tiled<true, 1>"),
    "unit_wu2":     (dict(TILED_MULTI="5", WEIGHTED_UNIT="2"), "RE", False, "k_pass_tiled_unit<true, 0>", "k_pass_tiled_unit<true, 1>"),
    "merged_tiled": (dict(TILED_MULTI="0"), "RE", True, "k_pass_tiled<true, 0>", "k_pass_tiled<true, 1>"),
    "merged_unit":  (dict(TILED_MULTI="5"), "RE", True, "k_pass_tiled_unit<true, 0>", "k_pass_tiled<true, 1>"),
}


class Problem:
    """A CSR with a sample: R (int32 counts), E (row lengths, 0 = outside the likelihood), den (None = the E-scatter)."""

    def __init__(self, name, n_tx, rp, ci, R, E, den=None):
        self.name, self.n_tx = name, int(n_tx)
        self.rp, self.ci = np.ascontiguousarray(rp, dtype=np.uint64), np.ascontiguousarray(ci, dtype=np.int32)
        self.R, self.E = np.ascontiguousarray(R, dtype=np.int32), np.ascontiguousarray(E, dtype=np.float64)
        self.den = None if den is None else np.ascontiguousarray(den, dtype=np.float64)

    @property
    def n_rows(self):
        return len(self.rp) - 1


def _sample(rng, n_rows, R=None):
    """Counts R (given, or 1 + Poisson) with about 3 % set to 0; lengths E with about 5 % at 0."""
    R = (1 + rng.poisson(2.0, size=n_rows)) if R is None else np.array(R)
    R = R.astype(np.int32)
    R[rng.random(n_rows) < 0.03] = 0
    E = rng.uniform(0.5, 2.0, size=n_rows)
    E[rng.random(n_rows) < 0.05] = 0.0
    return R, E


def segments():
    """Segment-level input, the form the reference solves: read-level rows of the human law collapsed to counts."""
    s = synth.make_matrix(n_tx=3000, n_reads=200000, law="human", xfam=0.02, seed=21)
    rp, ci, cnt = synth.collapse(s["row_ptr"], s["col_idx"])
    R, E = _sample(np.random.default_rng(31), len(cnt), cnt)
    return Problem("segments", s["n_tx"], rp, ci, R, E)


def cfg5_reads():
    """Config 5's window law at 1/2000: 20 ids per row on average, 10 % of the rows with 50-100 (repeats allowed)."""
    s = synth.make_config("cfg5", 0.0005)
    R, E = _sample(np.random.default_rng(32), len(s["row_ptr"]) - 1)
    return Problem("cfg5_reads", s["n_tx"], s["row_ptr"], s["col_idx"], R, E)


def cfg5_segments():
    s = synth.make_config("cfg5", 0.0005)
    rp, ci, cnt = synth.collapse(s["row_ptr"], s["col_idx"])
    R, E = _sample(np.random.default_rng(33), len(cnt), cnt)
    return Problem("cfg5_segments", s["n_tx"], rp, ci, R, E)


def ugly(seed=7):
    """Empty rows, repeated ids, single-id rows (folded), rows longer than kMaxRowLen (leftover CSR), cross-family hits,
    and rows whose ids all have theta = 0 (den = 0 given by the caller: S = 0 with R > 0 and E > 0)."""
    rng = np.random.default_rng(seed)
    n_tx, n_rows, fam = 2500, 9000, 30
    zero = np.arange(0, n_tx, 50)                                 # the transcripts with den = 0, hence theta = 0
    rows = []
    for _ in range(n_rows):
        u = rng.random()
        k = 0 if u < 0.03 else 1 if u < 0.30 else int(rng.integers(2, 14)) if u < 0.96 else \
            int(rng.integers(14, 120)) if u < 0.99 else int(rng.integers(KMAXROWLEN + 1, 3 * KMAXROWLEN))
        base = int(rng.integers(0, n_tx))
        t = (base + rng.integers(0, fam, size=k)) % n_tx            # in-family ids, repeats allowed
        if k >= 2 and rng.random() < 0.1:
            t[rng.integers(0, k)] = rng.integers(0, n_tx)          # a cross-family hit
        rows.append(t)
    for _ in range(60):                                            # rows on den = 0 transcripts only
        rows.append(rng.choice(zero, size=int(rng.integers(1, 6))))
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate(rows).astype(np.int32)
    R, E = _sample(rng, len(rows), rng.integers(0, 30, size=len(rows)))
    R[-60:] = np.maximum(R[-60:], 1)
    E[-60:] = 1.0
    E[np.diff(rp.astype(np.int64)) == 0] = 0.0                     # an empty row has no EUMA
    den = np.zeros(n_tx)
    np.add.at(den, ci, np.repeat(E, np.diff(rp.astype(np.int64))))
    den[zero] = 0.0
    return Problem("ugly", n_tx, rp, ci, R, E, den)


def big_segments(n_rows=6_600_000, seed=11):
    """A segment matrix above the production threshold of the unit kernel (more than 2048 tiles of 3072 rows): 2-6 ids per
    row inside families of 24, numpy-generated."""
    rng = np.random.default_rng(seed)
    n_tx = 400_000
    k = rng.integers(2, 7, size=n_rows)
    rp = np.zeros(n_rows + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(k)
    base = np.repeat((rng.integers(0, n_tx // 24, size=n_rows) * 24), k)
    ci = (base + rng.integers(0, 24, size=int(rp[-1]))).astype(np.int32)
    R = (1 + rng.poisson(3.0, size=n_rows)).astype(np.int32)
    E = rng.uniform(0.5, 2.0, size=n_rows)
    return Problem("big_segments", n_tx, rp, ci, R, E)


PROBLEMS = {"segments": segments, "cfg5_reads": cfg5_reads, "cfg5_segments": cfg5_segments, "ugly": ugly}
_cache = {}


def problem(name):
    if name not in _cache:
        _cache[name] = PROBLEMS[name]()
    return _cache[name]


# Unit shapes: layout knobs (EMSAR_HIP_<name>) -> the matrix they are run on -> what the layout must then contain
# (test_pass_kernel_shapes.py checks the facts on the host; test_pass_kernels_gpu.py runs the unit kernel on each).
#   stride      the most tiles of any unit (units with fewer have absent tiles in utiles)
#   few_slices  some unit has fewer than 4 slices (waves without a slice)
#   m16         share of slices with more than 16 backward segments per lane, in %, at least
#   far_mean    far slots per unit on average, at least (a lower bound on the longest far list)
SHAPES = [
    ("unit_tiles_1", dict(UNIT_TILES="1"), "segments", dict(stride=1, few_slices=True)),
    ("unit_tiles_max_3", dict(UNIT_TILES_MAX="3"), "cfg5_segments", dict(stride=3, m16=10)),
    ("unit_tiles_max_4", dict(UNIT_TILES_MAX="4", UNIT_FAR_SOFT=str(KFARMAX)), "cfg5_reads", dict(stride=4, m16=5)),
    ("unit_tiles_max_4_seg", dict(UNIT_TILES_MAX="4", UNIT_FAR_SOFT=str(KFARMAX)), "cfg5_segments", dict(stride=3, m16=10)),
    ("far_soft_0", dict(UNIT_FAR_SOFT="0"), "cfg5_reads", dict(stride=4, m16=5)),
    ("lpt_0", dict(UNIT_LPT="0"), "cfg5_reads", dict(stride=3)),
    ("tile_rows_768", dict(TILE_ROWS="768"), "segments", dict(few_slices=True)),
    ("tile_rows_1536", dict(TILE_ROWS="1536"), "segments", dict(stride=1, few_slices=True)),
    ("anchor_0", dict(TILE_ANCHOR="0"), "segments", dict(few_slices=True, far_mean=KFARMAX // 2, m16=5)),
    ("unit_sort_0", dict(UNIT_SORT="0"), "cfg5_segments", dict(m16=10)),
    ("tile_cut_0", dict(TILE_CUT="0"), "cfg5_reads", dict(stride=4)),
    ("short_ecnt_4", dict(SHORT_ECNT="4"), "segments", dict(few_slices=True, far_mean=KFARMAX // 2, m16=20)),
    ("tile_block_16", dict(TILE_BLOCK="16"), "segments", dict(few_slices=True, m16=10)),
    ("tile_block_96", dict(TILE_BLOCK="96"), "cfg5_segments", dict(m16=30)),
]
