"""CPU: the layout knobs of the unit-shape GPU tests (test_pass_kernels_gpu.py) do produce the shapes those tests are meant to
reach.  The layout does not depend on the device or on the host thread count, so the host self-check of the same matrix
under the same knobs shows it; the facts are read from the statistics the builder prints under EMSAR_HIP_DEBUG."""
import re

import numpy as np
import pytest

from emsar_amd import EmsarHipError, layout_selfcheck_tiled
from tests import pass_problems as P


def layout_stats(monkeypatch, capfd, knobs, prob, merge_rows=False):
    """Lay `prob` out under `knobs` and return the builder's statistics: stride, far slots, units by slice count, % of slices
    with more than 8 / 16 / 24 backward segments per lane."""
    for k in P.LAYOUT_KNOBS:
        monkeypatch.delenv("EMSAR_HIP_" + k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("EMSAR_HIP_" + k, v)
    monkeypatch.setenv("EMSAR_HIP_DEBUG", "1")
    capfd.readouterr()
    info = layout_selfcheck_tiled(prob.n_tx, prob.rp, prob.ci, merge_rows=merge_rows)
    err = capfd.readouterr().err
    u = re.search(r"unit tables: (\d+) units, stride (\d+), (\d+) far slots", err)
    h = re.search(r"units by number of slices 1\.\.12:((?: \d+){12})", err)
    m = re.search(r"backward segments per lane \((\d+) % > 8, (\d+) % > 16, (\d+) % > 24\)", err)
    assert u and h and m, err
    return dict(units=int(u.group(1)), stride=int(u.group(2)), far_slots=int(u.group(3)), hist=[int(x) for x in h.group(1).split()],
                m8=int(m.group(1)), m16=int(m.group(2)), m24=int(m.group(3)), info=info)


@pytest.mark.parametrize("name,knobs,matrix,facts", P.SHAPES, ids=[s[0] for s in P.SHAPES])
def test_unit_shape_is_reached(monkeypatch, capfd, name, knobs, matrix, facts):
    st = layout_stats(monkeypatch, capfd, knobs, P.problem(matrix))
    assert st["units"] == st["info"]["n_units"] and sum(st["hist"]) == st["units"], st
    if "stride" in facts:
        assert st["stride"] == facts["stride"], st
    if facts.get("few_slices"):
        assert sum(st["hist"][:3]) > 0, st                     # a unit with 1-3 slices: some of its four waves have none
    if "m16" in facts:
        assert st["m16"] >= facts["m16"], st                   # tile_m_step's third branch (> 16 segments), as well as the second
    if "far_mean" in facts:
        assert st["far_slots"] >= facts["far_mean"] * st["units"], st


def test_default_layouts_have_the_shapes_of_the_pass_matrices(monkeypatch, capfd):
    """The matrices of the dispatch-table tests without knobs: config 5's rows form units of more than two tiles (absent tiles
    pad the unit tables), the segment sample has long far lists and slices with more than 16 backward segments."""
    st = layout_stats(monkeypatch, capfd, {}, P.problem("cfg5_reads"))
    assert st["stride"] == 4 and st["m16"] >= 5
    st = layout_stats(monkeypatch, capfd, {}, P.problem("cfg5_segments"))
    assert st["stride"] == 3 and st["m16"] >= 10 and sum(st["hist"][:3]) > 0
    st = layout_stats(monkeypatch, capfd, {}, P.problem("segments"))
    assert st["stride"] == 2 and st["m16"] >= 20 and sum(st["hist"][:3]) > 0 and st["far_slots"] >= P.KFARMAX // 2 * st["units"]
    ug = P.problem("ugly")
    st = layout_stats(monkeypatch, capfd, {}, ug)
    assert st["info"]["folded_single_rows"] > 0 and st["units"] > 0
    lens = np.diff(ug.rp.astype(np.int64))
    assert (lens > P.KMAXROWLEN).any() and (lens == 0).any()


def test_dense_coo_lists_are_refused(monkeypatch):
    """TILE_DENSE > 1 builds COO lists that check_tiled_extents refuses: the host self-check reports it instead of laying out."""
    monkeypatch.setenv("EMSAR_HIP_TILE_DENSE", "2")
    p = P.problem("segments")
    with pytest.raises(EmsarHipError) as e:
        layout_selfcheck_tiled(p.n_tx, p.rp, p.ci)
    assert e.value.status == -1                               # EMSAR_HIP_ERR_ARG
