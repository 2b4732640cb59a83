"""CPU: bench.py's workload and arguments.  The threaded generator of the headline matrix returns synth.make_matrix's arrays (so
the benchmark times the same matrix as before, and its inputs are the same from run to run); a plain run's options."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from emsar_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("law,xfam,threads", [("human", 0.02, 3), ("human", 0.0, 1), ("repeats", 0.05, 4), ("poisson2", 0.02, 2)])
def test_threaded_family_matrix_is_synths(law, xfam, threads):
    kw = dict(n_tx=3000, n_reads=70_000, law=law, xfam=xfam, seed=7, block=16_000)       # five blocks, the last one short
    want = synth.make_matrix(structure="family", **kw)
    got = bench.family_matrix_threaded(threads=threads, **kw)
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.dtype == b.dtype and np.array_equal(a, b), k


def test_make_workload_of_the_headline_config_at_small_scale():
    cfg = dict(synth.CONFIGS["cfg3"], n_tx=2000, n_reads=300_000, structure="family")
    want = synth.make_matrix(**cfg)
    got = bench.make_workload(cfg)
    for k in ("row_ptr", "col_idx", "den"):
        assert np.array_equal(want[k], got[k]), k
    w = bench.make_workload(dict(cfg, structure="window"))
    assert np.array_equal(w["col_idx"], synth.make_matrix(**dict(cfg, structure="window"))["col_idx"])


def test_options_of_a_plain_run():
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    for bad in (["--steps", "0"], ["--warmup", "-1"]):                 # refused before anything touches a device
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, (bad, r.stderr[-300:])
