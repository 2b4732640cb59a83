"""Problems for the quantile kernels' tile shapes (emsar_amd/csrc/kernels_quant.hpp, k_iso_quantiles): three small samples, the replicate
counts at both edges of every padded size, the probabilities, and the host-side prediction of every replicate of the closed-form
samples.  Shared by tests/test_quant_shapes_cpu.py (the recipe holds) and tests/test_quant_shapes_gpu.py (the device against it).

The tile rule (kernels_quant.hpp): Bp = B rounded up to a power of two, C = 2048 / Bp clamped to 1 .. 32 columns, Bp * C doubles of LDS.

      B           Bp     C    LDS bytes
      33 ..  64    64   32    16384
      65 .. 128   128   16    16384
     129 .. 256   256    8    16384
     257 .. 512   512    4    16384
     513 .. 1024 1024    2    16384
    1025 .. 2048 2048    1    16384
    2049 .. 4096 4096    1    32768
"""
import functools
from types import SimpleNamespace

import numpy as np

from emsar_amd import hip

B_EDGES = (33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
BS = tuple(sorted(B_EDGES + (100, 1000)))
CYCLE = (0, 1, 1, 2, 3, 7, 16)             # all <= 16: the inversion path of the Poisson draw, where device and host draw the same bits
SPARSE_SEED = 21
# lattice: one seed per B, the first (from 1 up) at which every condition of tests/test_quant_shapes_cpu.py holds for that B.  On a
# lattice of at most 33 distinct values the two order statistics around the median of 4096 replicates differ only when a value's
# count lands exactly on the median's index, so most seeds have no such column at the larger B.
LATTICE_SEED = {33: 1, 64: 1, 65: 1, 100: 1, 128: 1, 129: 1, 256: 1, 257: 1, 512: 10, 513: 1, 1000: 23, 1024: 1, 1025: 1, 2048: 216, 2049: 216,
                4096: 3372}


def tile_of(B):
    """-> (Bp, C, LDS bytes) of the quantile kernels' tile for B replicates: the documented rule, restated"""
    Bp = 1
    while Bp < B:
        Bp *= 2
    C = min(32, max(1, 2048 // Bp))
    return Bp, C, 8 * Bp * C


def den_in_row_order(p):
    """den_t = sum_c m_ct E_c added one row at a time in row order (tests/test_bootq_gpu.py::host_den)"""
    rp = np.asarray(p.row_ptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    E = np.ones(len(rp) - 1) if p.E is None else np.asarray(p.E, dtype=np.float64)
    den = np.zeros(p.n_tx)
    np.add.at(den, np.asarray(p.col_idx), E[rows])
    return den


def _single_rows(n_tx, tx_of_row, R, E, gmap, ng):
    """a sample whose every row names one transcript: theta_b,t = (the draws of t's rows, added) / den_t, no EM"""
    n_rows = len(tx_of_row)
    p = SimpleNamespace(n_tx=n_tx, n_rows=n_rows, row_ptr=np.arange(n_rows + 1, dtype=np.uint64), col_idx=np.asarray(tx_of_row, dtype=np.int32),
                        R=np.asarray(R, dtype=np.int32), E=E, gmap=np.asarray(gmap, dtype=np.int32), ng=ng)
    p.den = den_in_row_order(p)
    return p


LATTICE_GENE_SIZES = (1, 2, 3, 3, 3, 3, 2, 3, 3, 3, 1, 3, 3, 3, 2, 3, 3, 3, 3, 2, 3, 3, 3, 3, 3)       # 25 genes over transcripts 0 .. 66


@functools.lru_cache(maxsize=None)
def lattice():
    """71 transcripts, 27 genes.  Transcript t < 67 has 1 + t % 2 rows [t] of its own, each with R = CYCLE[t % 7] (so every seventh
    transcript has rows and no reads); 67 .. 70 are in no row.  E uniform in [0.5, 2].  Genes 0 .. 24: 1, 2 or 3 neighbours of
    0 .. 66; every 11th transcript (5, 16, ..) and 67 in no gene; gene 25 = {68, 69, 70} and gene 0 = {0}: zero reads in every replicate; gene 26: no
    transcripts.  71 and 27 leave a partial last tile at every C > 1."""
    n_tx, tx_of_row, R = 71, [], []
    for t in range(67):
        for _ in range(1 + t % 2):
            tx_of_row.append(t)
            R.append(CYCLE[t % 7])
    E = np.random.default_rng(71).uniform(0.5, 2.0, size=len(R))
    gmap = np.full(n_tx, -1, dtype=np.int32)
    gmap[:67] = np.repeat(np.arange(len(LATTICE_GENE_SIZES)), LATTICE_GENE_SIZES)
    gmap[5::11] = -1
    gmap[67] = -1
    gmap[68:] = 25
    return _single_rows(n_tx, tx_of_row, R, E, gmap, 27)


@functools.lru_cache(maxsize=None)
def sparse():
    """5 transcripts, rows [0], [1], [2] with R = 1 and E = 1: one replicate in twenty (e^-3) draws nothing at all, S_b = 0"""
    return _single_rows(5, [0, 1, 2], [1, 1, 1], None, [0, 0, 1, -1, 2], 3)


@functools.lru_cache(maxsize=None)
def family():
    """_family(6) of tests/test_bootstrap_gpu.py under the gene map of tests/test_bootq_gpu.py::test_numbering_invariance: connected
    sets of 2 .. 40 transcripts, solved by EM in the resident sets -- values off any lattice"""
    from tests.test_bootstrap_gpu import _family
    m = _family(6)
    gmap = (np.arange(m.n_tx) // 3).astype(np.int32)
    gmap[7::13] = -1
    gmap[1:3] = -1
    p = SimpleNamespace(n_tx=m.n_tx, n_rows=m.n_rows, row_ptr=m.row_ptr, col_idx=m.col_idx, R=np.asarray(m.R, dtype=np.int32),
                        E=np.asarray(m.E, dtype=np.float64), gmap=gmap, ng=int(gmap.max()) + 1)
    p.den = den_in_row_order(p)
    return p


PROBLEMS = {"lattice": lattice, "sparse": sparse, "family": family}


def seed_of(name, B):
    return LATTICE_SEED[B] if name == "lattice" else SPARSE_SEED


@functools.lru_cache(maxsize=None)
def _draws(name, seed, B):
    p = PROBLEMS[name]()
    return np.stack([hip.bootstrap_draw_host(seed, b, p.R) for b in range(B)])


def draws(name, seed, B):
    """[B][n_rows] int32: the Poisson draws of replicates 0 .. B-1 on the host (4096 drawn once per seed where several B share it)"""
    full = _draws(name, seed, B if name == "lattice" else max(BS))
    full.setflags(write=False)
    return full[:B]


def predicted_replicates(name, seed, B):
    """[B][n_tx]: theta_b,t = u_b,t / den_t with u the exact integer sum of the draws of t's rows, 0 where den_t = 0 -- the closed
    form's one division (k_boot_closed), for the two samples whose rows name one transcript each"""
    p = PROBLEMS[name]()
    u = np.zeros((B, p.n_tx))
    np.add.at(u, (slice(None), p.col_idx), draws(name, seed, B).astype(np.float64))
    return np.where(p.den > 0, u / np.where(p.den > 0, p.den, 1.0), 0.0)


def median_pair(x):
    """the two order statistics the q = 0.5 interpolation reads, per column of x [B][n]: x_(i), x_(i+1), i = floor((B - 1) / 2)"""
    s = np.sort(x, axis=0)
    i = (len(x) - 1) // 2
    return s[i], s[i + 1]


Q5 = [0.0, 0.025, 0.5, 0.975, 1.0]         # Q of tests/test_bootq_gpu.py (asserted there to be the same list)
Q1 = np.array([0.975])


def _q67():
    q = Q5 + [0.25, 0.75, float(np.nextafter(1.0, 0.0)), float(np.nextafter(0.0, 1.0))]
    q += np.random.default_rng(67).random(67 - len(q)).tolist()
    return np.sort(np.array(q))


Q67 = _q67()                                # ascending: 0, nextafter(0, 1), .., nextafter(1, 0), 1.  67 * C is a multiple of 256 at no C
