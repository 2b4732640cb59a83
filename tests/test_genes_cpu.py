"""CPU: the g2t reader (genes.c) and the gene writers against util/FPKM2gFPKM.pl -- its own output on the reference's .fpkm of
vicugna_pe, and a Python restatement of the script's rules on g2t files written here."""
import gzip
import os

import numpy as np
import pytest

from emsar_amd import _build, hostlib
from tests.conftest import GOLDEN

VIC = os.path.join(GOLDEN, "vicugna_pe")


@pytest.fixture(scope="module")
def rsh():
    _build.build_host()
    return hostlib.HostRsh(os.path.join(VIC, "index.rsh"))


@pytest.fixture(scope="module")
def syn():
    _build.build_host()
    return hostlib.HostRsh(os.path.join(GOLDEN, "syn2k_se", "index.rsh"))


def read_gfpkm(path):
    """FPKM2gFPKM.pl output (rows in any order; plain or gzipped) -> {gene: (fpkm, ireadcount, ireadcount_int, tpm)}"""
    lines = (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read().splitlines()
    assert lines[0] == "geneID\tFPKM\tiReadcount\tiReadcount.int\tTPM"
    out = {}
    for l in lines[1:]:
        f = l.split("\t")
        assert len(f) == 5 and f[0] not in out
        out[f[0]] = (float(f[1]), float(f[2]), int(f[3]), float(f[4]))
    return out


def fpkm_columns(path):
    """names and columns 1, 4, 6 of a .fpkm, as the script reads them"""
    rows = [l.split("\t") for l in open(path).read().splitlines()[1:]]
    return [r[0] for r in rows], np.array([[float(r[1]), float(r[4]), float(r[6])] for r in rows])


def perl_roundoff(x):
    i = float(int(x))
    return int(i) + (1 if x - i >= 0.5 else 0)


def test_vicugna_reproduces_the_reference_gene_step(rsh, tmp_path):
    names, gene_of_tx = rsh.genes(os.path.join(VIC, "genes.g2t.gz"))
    assert len(names) == 12663 and gene_of_tx.shape == (12704,) and rsh.g2t_counts == (0, 0)
    assert "" not in names                                   # every index transcript is listed
    tx, cols = fpkm_columns(os.path.join(VIC, "ref.run0.fpkm"))
    assert tx == rsh.names
    sums = np.zeros((len(names), 3))
    for t in range(len(tx)):                                 # sequential, in file order, like the script
        sums[gene_of_tx[t]] += cols[t]
    n_iso = np.bincount(gene_of_tx, minlength=len(names))
    assert (n_iso >= 1).all() and (n_iso >= 2).sum() == 37
    ref = read_gfpkm(os.path.join(VIC, "ref.run0.gfpkm.gz"))
    assert set(ref) == set(names)
    want = np.array([ref[g][:2] + ref[g][3:] for g in names])
    tol = n_iso[:, None] * 5e-7 + 1e-9 * np.abs(want)
    assert np.all(np.abs(sums - want) <= tol)
    # the writer: the script's header, its roundoff of the gene's iReadcount, values to six decimals
    path = str(tmp_path / "g.gfpkm")
    rsh.write_gfpkm(path, names, sums[:, 0], sums[:, 1], sums[:, 2])
    got = read_gfpkm(path)
    assert list(got) == names
    for k, g in enumerate(names):
        assert got[g][2] == ref[g][2], g
        for j, c in ((0, 0), (1, 1), (2, 3)):
            assert abs(got[g][c] - want[k, j]) <= (n_iso[k] + 1) * 5e-7 + 1e-9 * abs(want[k, j]), (g, c)


def restate_fpkm2gfpkm(g2t_text, index_names):
    """FPKM2gFPKM.pl's map on text (chomp, split on tabs, last line wins, unlisted transcripts under the undef key), with this project's
    two documented deviations: a trailing CR is stripped and tab-less lines are skipped.  Genes in order of first appearance, the
    empty-ID gene last."""
    t2g, order = {}, []
    for line in g2t_text.split("\n"):
        line = line[:-1] if line.endswith("\r") else line
        if "\t" not in line:
            continue
        f = line.split("\t")
        g, t = f[0], f[1]
        if g and g not in order:
            order.append(g)
        t2g[t] = g
    genes = [t2g.get(t, "") for t in index_names]
    used = set(genes)
    names = [g for g in order if g in used] + ([""] if "" in used else [])
    ix = {g: k for k, g in enumerate(names)}
    unknown = sum(1 for line in g2t_text.split("\n") if "\t" in line and line.rstrip("\r").split("\t")[1] not in set(index_names))
    return names, np.array([ix[g] for g in genes], dtype=np.int32), unknown


def _quirky_g2t(names):
    t = names
    lines = [
        "GX\tNOT_IN_INDEX_1",                  # GX appears first with an unknown transcript ...
        "GA\t%s" % t[0],
        "GA\t%s\textra\tcolumns" % t[1],       # extra fields are ignored
        "GB\t%s" % t[2],                       # GB loses its only transcript below: it disappears
        "GC\t%s\r" % t[3],                     # CRLF
        "GB_only_unknown\tNOT_IN_INDEX_2",
        "no tab on this line",
        "",
        "GC\t%s" % t[2],                       # t2 listed twice: the last gene wins
        "GX\t%s" % t[4],                       # ... and keeps its first-appearance place
        "\t%s" % t[5],                         # an empty gene field: the empty-ID gene, as the script's undef key
    ]
    lines += ["G%03d\t%s" % (k // 3, t[k]) for k in range(10, 400)]
    return "\n".join(lines) + "\r\n"


def test_quirks_against_a_restatement_of_the_script(syn, tmp_path):
    text = _quirky_g2t(syn.names)
    p = tmp_path / "q.g2t"
    p.write_bytes(text.encode())
    names, gene_of_tx = syn.genes(str(p))
    want_names, want_map, unknown = restate_fpkm2gfpkm(text, syn.names)
    assert names == want_names
    assert np.array_equal(gene_of_tx, want_map)
    assert syn.g2t_counts == (unknown, int((want_map == len(want_names) - 1).sum()))
    # the rules, spelled out
    assert names[:3] == ["GX", "GA", "GC"] and "GB" not in names and "GB_only_unknown" not in names
    assert names[-1] == "" and gene_of_tx[2] == gene_of_tx[3] == names.index("GC")
    assert gene_of_tx[5] == len(names) - 1 and (gene_of_tx[400:] == len(names) - 1).all()
    assert unknown == 2
    # gzipped: the same map
    pz = tmp_path / "q.g2t.gz"
    pz.write_bytes(gzip.compress(text.encode()))
    names_z, map_z = syn.genes(str(pz))
    assert names_z == names and np.array_equal(map_z, gene_of_tx)


def test_no_empty_gene_when_every_transcript_is_listed(syn, tmp_path):
    p = tmp_path / "all.g2t"
    p.write_text("".join("G%d\t%s\n" % (k % 7, n) for k, n in enumerate(syn.names)))
    names, gene_of_tx = syn.genes(str(p))
    assert names == ["G%d" % k for k in range(7)]
    assert np.array_equal(gene_of_tx, np.arange(len(syn.names)) % 7)


def test_errors(syn, tmp_path):
    with pytest.raises(hostlib.HostError):
        syn.genes(str(tmp_path / "missing.g2t"))
    (tmp_path / "empty.g2t").write_text("")
    with pytest.raises(hostlib.HostError):
        syn.genes(str(tmp_path / "empty.g2t"))
    (tmp_path / "notab.g2t").write_text("gene transcript\nanother line\n")
    with pytest.raises(hostlib.HostError):
        syn.genes(str(tmp_path / "notab.g2t"))


def test_writers_byte_for_byte(syn, tmp_path):
    names = ["GA", "GB", "GC", ""]
    fpkm = np.array([1.5, 0.0, 123456.1234567, 2e-7])
    ir = np.array([2.5, 2.4999999, 0.5, 7.0])
    tpm = np.array([10.0, 0.0, 3.25, 1e-9])
    p = str(tmp_path / "x.gfpkm")
    syn.write_gfpkm(p, names, fpkm, ir, tpm)
    assert open(p, "rb").read() == (b"geneID\tFPKM\tiReadcount\tiReadcount.int\tTPM\n"
                                    b"GA\t1.500000\t2.500000\t3\t10.000000\n"
                                    b"GB\t0.000000\t2.500000\t2\t0.000000\n"
                                    b"GC\t123456.123457\t0.500000\t1\t3.250000\n"
                                    b"\t0.000000\t7.000000\t7\t0.000000\n")
    assert [perl_roundoff(x) for x in ir] == [3, 2, 1, 7]
    p = str(tmp_path / "x.gbootstrap")
    syn.write_gbootstrap(p, names[:2], fpkm[:2], [1.25, 0.0], [0.5, 0.0], tpm[:2], [0.125, 0.0])
    assert open(p, "rb").read() == (b"geneID\tFPKM\tboot.mean.FPKM\tboot.sd.FPKM\tTPM\tboot.sd.TPM\n"
                                    b"GA\t1.500000\t1.250000\t0.500000\t10.000000\t0.125000\n"
                                    b"GB\t0.000000\t0.000000\t0.000000\t0.000000\t0.000000\n")
