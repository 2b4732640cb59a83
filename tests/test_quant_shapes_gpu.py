"""GPU: k_boot_quantiles and k_iso_quantiles at every tile shape [Bp][C] -- C = 32, 16, 8, 4, 2, 1, both edges of every padded size
up to the limit B = 4096 (the 32 KiB tile), 100 and 1000 -- against references that no device code touches: the replicates predicted on
the host from bootstrap_draw_host (tests/quant_shape_problems.py), gene sums, usage and TPM restated in numpy, and the quantile
definition both in pure Python (tests/test_bootq_cpu.py::restated) and by quantiles_host.  Every comparison is bit for bit: sorting
does not round and the interpolation is three separately rounded operations.

tests/test_quant_tiles_gpu.py runs the same shapes with the device's own draws and gene sums and five probabilities.  Added here: the
host-side prediction, 67 probabilities (the read-out loop goes round more than once; 67 C is a multiple of 256 at no C) and a single
one, replicates with S_b = 0, transcripts of two rows and of none, usage quantiles at every B, values off a lattice, held batches,
numbering, and the limit."""
import math

import numpy as np
import pytest

from emsar_amd import EmsarHip, hip
from tests import quant_shape_problems as P
from tests.test_bootq_cpu import restated
from tests.test_bootq_gpu import same, tpm_of
from tests.test_bootstrap_gpu import SOLVE
from tests.test_genes_gpu import chunked_sums
from tests.test_isoforms_cpu import restated as usage_restated

pytestmark = pytest.mark.gpu
SHARED = ("fpkm_q", "tpm_q", "gene_fpkm_q", "gene_tpm_q")          # what bootstrap_quantiles returns as well
QUANT = SHARED + ("usage_q",)


def upload(d, p, layout=hip.LAYOUT_AUTO):
    d.set_deterministic(True)              # two calls give the same replicates, so calls can be compared
    d.upload_structure(p.n_tx, p.row_ptr, p.col_idx, layout=layout)
    d.upload_sample(p.R, p.E, p.den)
    d.set_gene_map(p.gmap, p.ng)


def references(p, reps, S):
    """the five arrays [B][n] the quantile stage sorts, from the replicates and the TPM denominators, in numpy"""
    usage, _, G = usage_restated(reps, p.gmap, p.ng)
    assert same(G, chunked_sums(reps, p.gmap, p.ng))
    return {"fpkm_q": reps, "tpm_q": tpm_of(reps, S), "gene_fpkm_q": G, "gene_tpm_q": tpm_of(G, S), "usage_q": usage}


def restated_quantiles(x, q):
    """tests/test_bootq_cpu.py::restated column by column (each column handed over sorted: its own sort is then one linear pass)"""
    out = np.zeros((len(q), x.shape[1]))
    for t in range(x.shape[1]):
        col = sorted(x[:, t].tolist())
        out[:, t] = [restated(col, float(qk)) for qk in q]
    return out


def check_quantiles(r, ref, q, what, keys=QUANT):
    for k in keys:
        assert r[k].shape == (len(q), ref[k].shape[1]) and np.isfinite(r[k]).all(), (what, k)
        assert same(r[k], restated_quantiles(ref[k], q)), (what, k)
        assert same(r[k], hip.quantiles_host(ref[k], q)), (what, k)


def check_edges(r, ref, what):
    """Q67 is ascending: row 0 is q = 0, row 1 nextafter(0, 1), row -2 nextafter(1, 0), row -1 q = 1"""
    for k in QUANT:
        assert same(r[k][0], ref[k].min(axis=0)) and same(r[k][-1], ref[k].max(axis=0)), (what, k)
        assert np.all(r[k][0] <= r[k][1]) and np.all(r[k][1] <= r[k][2]), (what, k)
        assert np.all(r[k][-3] <= r[k][-2]) and np.all(r[k][-2] <= r[k][-1]), (what, k)


def check_sums(S, reps, what):
    """exactly 0 for a replicate that drew nothing; elsewhere the row's sum to the existing criterion (rtol 1e-12 of math.fsum)"""
    empty = ~reps.any(axis=1)
    assert not S[empty].any() and not np.signbit(S[empty]).any(), what
    want = np.array([math.fsum(row) for row in reps])
    assert np.allclose(S, want, rtol=1e-12, atol=0), what
    return empty


def run_and_check(d, p, B, seed, reps, what, **kw):
    """bootstrap_isoforms with the 67 probabilities against the references of `reps` (None: the call's own replicates), then the
    single probability, then bootstrap_quantiles' four shared outputs"""
    r = d.bootstrap_isoforms(B, seed, q=P.Q67, want_replicates=True, want_genes=True, **kw)
    assert r["stats"].n_replicates == B and r["qstats"].n_quantiles == 67 and r["qstats"].held_bytes == 8 * B * (p.n_tx + 1 + p.ng)
    if reps is None:
        reps = r["replicates"]
    else:
        assert same(r["replicates"], reps), what       # the held buffer is filled at the right rows, batch after batch
    S = r["replicate_sums"]
    empty = check_sums(S, reps, what)
    ref = references(p, reps, S)
    check_quantiles(r, ref, P.Q67, what)
    check_edges(r, ref, what)
    one = d.bootstrap_isoforms(B, seed, q=P.Q1, want_genes=True, **kw)
    assert same(one["replicate_sums"], S), what
    check_quantiles(one, ref, P.Q1, what)
    bq = d.bootstrap_quantiles(B, P.Q67, seed, want_replicates=True, want_genes=True, **kw)
    for k in SHARED + ("replicates", "replicate_sums"):
        assert same(bq[k], r[k]), (what, k)
    return r, ref, empty


@pytest.mark.parametrize("B", P.BS)
def test_lattice(B):
    p = P.lattice()
    seed = P.seed_of("lattice", B)
    with EmsarHip(0) as d:
        upload(d, p)
        r, ref, empty = run_and_check(d, p, B, seed, P.predicted_replicates("lattice", seed, B), ("lattice", B))
    assert not r["fpkm_q"][:, 67:].any() and not r["gene_fpkm_q"][:, 25:].any() and not r["usage_q"][:, p.gmap < 0].any()
    assert (r["fpkm_q"][-1] > r["fpkm_q"][0]).any() and (r["usage_q"][-1] > r["usage_q"][0]).any()


@pytest.mark.parametrize("B", P.BS)
def test_sparse(B):
    """Replicates that draw nothing: S_b = 0, so TPM_b = 0 by the guard of the TPM load (not 0 / 0), every gene sum is 0 and with it the
    usage, and the replicate's columns all tie at 0."""
    p = P.sparse()
    with EmsarHip(0) as d:
        upload(d, p)
        r, ref, empty = run_and_check(d, p, B, P.SPARSE_SEED, P.predicted_replicates("sparse", P.SPARSE_SEED, B), ("sparse", B))
    assert empty.any() and not empty.all()
    for k in QUANT:
        assert not ref[k][empty].any() and not r[k][0].any(), k            # the empty replicates are every column's minimum: 0
    assert r["tpm_q"][-1, :3].max() == 1e6 and r["usage_q"][-1].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("B", [129, 1025])
def test_family(B):
    """EM through the resident sets: values off any lattice.  The quantile stage is judged on its own input, the returned replicates."""
    p = P.family()
    with EmsarHip(0) as d:
        upload(d, p)
        r, ref, empty = run_and_check(d, p, B, 21, None, ("family", B), set_mode=0, **SOLVE)
    assert not empty.any() and r["stats"].sets_ms > 0
    lo, hi = P.median_pair(r["replicates"])
    assert (lo != hi).mean() > 0.5                                            # mostly no ties: the interpolation has something to add


def test_batch_offsets(monkeypatch):
    """129 replicates in batches of 50, 50 and 29: every batch writes its own rows of the held buffers"""
    p, B = P.lattice(), 129
    seed = P.seed_of("lattice", B)
    with EmsarHip(0) as d:
        upload(d, p)
        whole = d.bootstrap_isoforms(B, seed, q=P.Q67, want_replicates=True, want_genes=True)
        assert whole["stats"].batch == B
        monkeypatch.setenv("EMSAR_HIP_BOOT_BATCH", "50")
        split = d.bootstrap_isoforms(B, seed, q=P.Q67, want_replicates=True, want_genes=True)
        monkeypatch.delenv("EMSAR_HIP_BOOT_BATCH")
    assert split["stats"].batch == 50
    assert same(split["replicates"], P.predicted_replicates("lattice", seed, B))
    for k in QUANT + ("replicates", "replicate_sums"):
        assert same(split[k], whole[k]), k


@pytest.mark.parametrize("name,B", [("lattice", 257), ("family", 129)])
def test_numbering(name, B, monkeypatch):
    """EMSAR_HIP_RENUMBER 2 and 0 under LAYOUT_TILED: the same bits in every quantile output.  (The lattice has no row of two
    transcripts, so the library finds nothing to renumber there and both runs keep the caller's order; the family problem is
    renumbered, and its quantile stage then goes through the caller -> library map.)"""
    p = P.PROBLEMS[name]()
    seed = P.seed_of(name, B)
    kw = dict(set_mode=0, **SOLVE) if name == "family" else {}
    res = []
    for renumber in ("2", "0"):
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", renumber)
        with EmsarHip(0) as d:
            upload(d, p, layout=hip.LAYOUT_TILED)
            assert d.info()["renumbered"] == int(renumber == "2" and name == "family")
            r = d.bootstrap_isoforms(B, seed, q=P.Q67, want_replicates=True, want_genes=True, **kw)
        ref = references(p, r["replicates"], r["replicate_sums"])
        for k in QUANT:
            assert same(r[k], hip.quantiles_host(ref[k], P.Q67)), (name, renumber, k)
        res.append(r)
    if name == "lattice":
        assert same(res[0]["replicates"], P.predicted_replicates(name, seed, B))
    for k in QUANT + ("replicates", "replicate_sums"):
        assert same(res[0][k], res[1][k]), (name, k)


def test_the_limit():
    p = P.lattice()
    seed = P.seed_of("lattice", 33)
    with EmsarHip(0) as d:
        upload(d, p)
        with pytest.raises(hip.EmsarHipError) as e:
            d.bootstrap_isoforms(4097, seed, q=[0.5])
        assert e.value.status == -1
        reps = P.predicted_replicates("lattice", seed, 33)
        r = d.bootstrap_isoforms(33, seed, q=P.Q67, want_replicates=True, want_genes=True)
    assert same(r["replicates"], reps)
    check_quantiles(r, references(p, reps, r["replicate_sums"]), P.Q67, "after the rejected call")
