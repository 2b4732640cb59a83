"""GPU: the bootstrap quantile sort (k_boot_quantiles, k_iso_quantiles) in every tile shape.  quant_tile_shift turns the replicate
count B into an LDS tile [Bp][C], Bp = B rounded up to a power of two and C = 2048 / Bp clamped to 1 .. 32; the B here cover every
(Bp, C) from (64, 32) to (4096, 1), the only 32 KiB shape, each at its smallest B (Bp / 2 + 1: nearly half the tile is padding) and
at its full size.  The problem is in closed form -- one single-transcript row per transcript, theta_b = w_b / E -- so that
thousands of replicates cost nothing, and it has fewer columns (37 transcripts, 20 genes) than the widest tile and no multiple of
any tile width: every C leaves a partial last tile.  Sorting does not round, so every comparison is bit for bit."""
import numpy as np
import pytest

from emsar_amd import EmsarHip, hip
from tests.test_bootq_gpu import Q, check_against_host, gene_map, same, tpm_of

pytestmark = pytest.mark.gpu
N_TX, SEED = 37, 13
# (Bp, C): (64, 32) (128, 16) | (256, 8) (512, 4) | (1024, 2) (2048, 1) | (4096, 1)
GROUPS = [(33, 64, 65, 128), (129, 256, 257, 512), (513, 1024, 1025, 2048), (2049, 4096)]
ISO_B = [129, 257, 1025, 4096]


class Problem:
    def __init__(self):
        rng = np.random.default_rng(4)
        # an all-zero column, heavy ties (counts of 1: a draw is 0, 1 or 2 most of the time), both draw paths (direct up to 16, PTRS above)
        self.R = np.resize(np.array([0, 1, 1, 3, 50, 100000, 2, 17, 1, 4000], dtype=np.int32), N_TX)
        self.E = rng.uniform(0.5, 2.0, size=N_TX)
        self.rp, self.ci = np.arange(N_TX + 1, dtype=np.uint64), np.arange(N_TX, dtype=np.int32)
        self.gmap, self.ng = gene_map("closed-form", N_TX)     # genes of 1, 2, 3 transcripts, transcripts in no gene, one empty gene
        assert self.ng == 20 and (self.gmap < 0).any() and set(np.bincount(self.gmap[self.gmap >= 0], minlength=self.ng)) == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def ctx():
    p = Problem()
    with EmsarHip(0) as d:
        d.upload_structure(N_TX, p.rp, p.ci)
        d.upload_sample(p.R, p.E, None)
        d.set_gene_map(p.gmap, p.ng)
        # the draws of replicate b do not depend on how many replicates a call asks for: drawn once for every B below
        W = np.array([d.bootstrap_weights(SEED, b) for b in range(4096)], dtype=np.float64)
        assert not W[:, p.R == 0].any() and W[:, p.R == 100000].min() > 90000
        W.setflags(write=False)
        yield d, p, W


def check_order_statistics(out, vals, B, what):
    """independent of quantile_sorted, which host and device share: q = 0 and q = 1 are the smallest and the largest of a column, and for
    odd B q = 0.5 is the middle one"""
    srt = np.sort(vals, axis=0)
    assert Q[0] == 0.0 and Q[2] == 0.5 and Q[4] == 1.0
    assert same(out[0], srt[0]) and same(out[4], srt[B - 1]), what
    if B % 2:
        assert same(out[2], srt[(B - 1) // 2]), what


@pytest.mark.parametrize("group", GROUPS, ids=["B" + "_".join(str(b) for b in g) for g in GROUPS])
def test_quantiles_in_every_tile_shape(ctx, group):
    d, p, W = ctx
    for B in group:
        r = d.bootstrap_quantiles(B, Q, SEED, want_replicates=True, want_genes=True)
        reps, S = r["replicates"], r["replicate_sums"]
        assert same(reps, W[:B] / p.E), B                    # the closed form: theta_b = w_b / E exactly
        check_against_host(d, r, p.gmap, p.ng, B)
        G = d.gene_sums(reps)
        for key, vals in (("fpkm_q", reps), ("tpm_q", tpm_of(reps, S)), ("gene_fpkm_q", G), ("gene_tpm_q", tpm_of(G, S))):
            check_order_statistics(r[key], vals, B, (B, key))
        assert not r["fpkm_q"][:, p.R == 0].any() and not r["gene_fpkm_q"][:, p.ng - 1].any()      # the all-zero column, the empty gene
        assert (r["fpkm_q"][4] > r["fpkm_q"][0])[p.R > 0].all()


@pytest.mark.parametrize("B", ISO_B)
def test_isoform_usage_quantiles_in_the_narrow_tiles(ctx, B):
    d, p, W = ctx
    r = d.bootstrap_isoforms(B, SEED, q=Q, want_replicates=True, want_genes=True)
    reps = r["replicates"]
    assert same(reps, W[:B] / p.E), B
    usage = hip.isoform_usage_host(p.gmap, p.ng, reps)
    assert same(r["usage_q"], hip.quantiles_host(usage, Q)), B
    check_order_statistics(r["usage_q"], usage, B, (B, "usage_q"))
    assert same(r["fpkm_q"], hip.quantiles_host(reps, Q)), B
    assert r["usage_q"][4].max() == 1.0 and (r["usage_q"][4] > r["usage_q"][0]).any()
