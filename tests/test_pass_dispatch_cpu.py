"""CPU: which TILED pass kernel launch_pass picks, asked of the library's own chooser (choose_pass_kernel in emsar_hip.hip through the
diagnostic entry emsar_hip_debug_pass_kernel; no device).  The table VARIANTS that test_pass_kernels_gpu.py runs on the GPU names the
kernel of every variant: here those names are held against the code, and the default's switch at 2048 tiles against the knobs it
stands for."""
import itertools

import pytest

from emsar_amd.hip import debug_pass_kernel as kernel
from tests.pass_problems import VARIANTS

EM, EM_LL, SCATTER = 0, 1, 2
PAIR_MIN_TILES = 2048                      # kPairMinTiles


def _row(variant):
    """A VARIANTS row as the chooser's arguments: weighted, tiled_multi, weighted_unit (the knobs' defaults are 1)."""
    knobs, weights, merged, k_em, k_ll = VARIANTS[variant]
    weighted = bool(weights) or merged     # upload_sample: a sample with R or E, or merged rows
    return weighted, int(knobs.get("TILED_MULTI", "1")), int(knobs.get("WEIGHTED_UNIT", "1")), k_em, k_ll


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_table_names_the_kernel_the_chooser_returns(variant):
    weighted, tm, wu, k_em, k_ll = _row(variant)
    assert kernel(weighted, EM, 100, tm, wu) == k_em
    assert kernel(weighted, EM_LL, 100, tm, wu) == k_ll


@pytest.mark.parametrize("weighted", [False, True])
def test_no_knobs_at_the_threshold_is_one_tile_per_workgroup(weighted):
    for mode in (EM, EM_LL):
        assert kernel(weighted, mode, PAIR_MIN_TILES) == kernel(weighted, mode, PAIR_MIN_TILES, tiled_multi=0)
        assert kernel(weighted, mode, PAIR_MIN_TILES) == "k_pass_tiled<%s, %d>" % ("true" if weighted else "false", mode)


def test_no_knobs_above_the_threshold_is_the_unit_kernel():
    n = PAIR_MIN_TILES + 1
    assert kernel(False, EM, n) == "k_pass_tiled_unit<false, 0>"
    assert kernel(False, EM_LL, n) == "k_pass_tiled_unit<false, 1>"
    assert kernel(True, EM, n) == "k_pass_tiled_unit<true, 0>"
    assert kernel(True, EM_LL, n) == "k_pass_tiled<true, 1>"      # the likelihood passes of weighted rows stay with the one-tile kernel


def test_scatter_is_always_the_unweighted_one_tile_kernel():
    for weighted, tm, wu, n in itertools.product((False, True), range(6), range(3), (100, 5000)):
        assert kernel(weighted, SCATTER, n, tm, wu) == "k_pass_tiled<false, 2>", (weighted, tm, wu, n)


def test_knob_values_outside_the_named_ones():
    for mode, n in itertools.product((EM, EM_LL), (100, 5000)):
        assert kernel(False, mode, n, tiled_multi=6) == kernel(False, mode, n, tiled_multi=2) == "k_pass_tiled_multi<false, %d, 2>" % mode
        for weighted in (False, True):
            assert kernel(weighted, mode, n, tiled_multi=-1) == kernel(weighted, mode, n, tiled_multi=0)


def test_a_mode_that_does_not_exist_is_refused():
    from emsar_amd import EmsarHipError
    with pytest.raises(EmsarHipError):
        kernel(False, 3, 100)
