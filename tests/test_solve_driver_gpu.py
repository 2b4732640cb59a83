"""GPU: the pass accounting of the streaming solve's driver (solve.hpp: SolveRun::stream), the part of the loop that a restructuring
can shift without any result changing much.

The rule, as the header states it: a cycle is pc = 1 pass (plain EM) or 3 (SQUAREM); the first 4 x check_every cycles are launched
one by one; from then on, at every multiple of check_every cycles, check_every cycles are replayed from one hipGraph while
iters + pc x check_every <= max_iter, and single cycles follow.  The graph is not used for plain EM with an odd check_every (the
host's swap of th0 / th1 would not be restored) nor with EMSAR_HIP_GRAPH=0.  With a rule that cannot fire (tol = 1e-300; tol <= 0
would mean the default) the solve therefore runs
    iters   = ceil(max_iter / pc) x pc
    replays = max(0, floor((max_iter - 4 pc ce) / (pc ce)))    when the graph is allowed, else 0.
The replays are read from the line the solve prints under EMSAR_HIP_DEBUG."""
import re

import numpy as np
import pytest

from emsar_amd import EmsarHip, synth
from emsar_amd.hip import LAYOUT_TILED

pytestmark = pytest.mark.gpu

_problem = []


def problem():
    if not _problem:
        _problem.append(synth.make_config("cfg3", 0.004))      # a few dozen tiles
    return _problem[0]


def solve(monkeypatch, capfd, accel, check_every, max_iter, graph):
    """(theta, stats, streaming passes, graph replays, cycles per replay) of one deterministic streaming solve that cannot converge"""
    s = problem()
    monkeypatch.setenv("EMSAR_HIP_DEBUG", "1")
    if graph:
        monkeypatch.delenv("EMSAR_HIP_GRAPH", raising=False)
    else:
        monkeypatch.setenv("EMSAR_HIP_GRAPH", "0")              # read when the context is created
    with EmsarHip(0) as ctx:
        ctx.set_deterministic(True)
        ctx.upload_structure(s["n_tx"], s["row_ptr"], s["col_idx"], LAYOUT_TILED)
        ctx.upload_sample(None, None, s["den"])
        capfd.readouterr()
        th, st = ctx.solve(max_iter=max_iter, accel=accel, tol=1e-300, check_every=check_every, set_mode=1)
        err = capfd.readouterr().err
    m = re.search(r"emsar_hip_solve: (\d+) streaming passes, (\d+) graph replays of (\d+) cycles", err)
    assert m, err
    return th, st, int(m.group(1)), int(m.group(2)), int(m.group(3))


def expected(accel, check_every, max_iter, graph_allowed):
    pc = 3 if accel else 1
    iters = -(-max_iter // pc) * pc
    replays = max(0, (max_iter - 4 * pc * check_every) // (pc * check_every)) if graph_allowed else 0
    return iters, replays


# accel, check_every, max_iter, graph on, iters, replays
CASES = [(1, 8, 129, True, 129, 1),
         (1, 8, 129, False, 129, 0),
         (1, 8, 200, True, 201, 4),
         (1, 5, 100, True, 102, 2),
         (0, 8, 50, True, 50, 2),
         (0, 5, 50, True, 50, 0)]        # plain EM, odd count: no graph


@pytest.mark.parametrize("accel,check_every,max_iter,graph,iters,replays", CASES,
                         ids=["accel%d-ce%d-max%d-%s" % (c[0], c[1], c[2], "graph" if c[3] else "nograph") for c in CASES])
def test_pass_accounting(monkeypatch, capfd, accel, check_every, max_iter, graph, iters, replays):
    allowed = graph and (accel == 1 or check_every % 2 == 0)
    assert expected(accel, check_every, max_iter, allowed) == (iters, replays)     # the table is the rule's
    _, st, passes, got_replays, per_replay = solve(monkeypatch, capfd, accel, check_every, max_iter, graph)
    print("iters %d, streaming passes %d, replays %d of %d cycles, converged %d" % (st.iters, passes, got_replays, per_replay, st.converged))
    assert st.converged == 0                                   # a surprise convergence would hide the case
    assert st.iters == iters and passes == iters
    assert got_replays == replays and per_replay == check_every


def test_graph_replay_does_not_change_the_bits(monkeypatch, capfd):
    """The 129-pass SQUAREM solve with one replay and with every kernel launched: theta, loglik and final_delta bit for bit."""
    th_g, st_g, _, replays_g, _ = solve(monkeypatch, capfd, 1, 8, 129, True)
    th_n, st_n, _, replays_n, _ = solve(monkeypatch, capfd, 1, 8, 129, False)
    assert (replays_g, replays_n) == (1, 0)
    assert st_g.converged == 0 and st_n.converged == 0
    np.testing.assert_array_equal(th_g, th_n)
    assert st_g.iters == st_n.iters == 129
    assert st_g.loglik == st_n.loglik and st_g.final_delta == st_n.final_delta
