"""CPU: what tests/awkward_problems.py has to hold for test_per_transcript_configs_gpu.py to mean anything -- the row forms (a repeated
tid in a multi-transcript row, the same multiset in another order, a verbatim repeat), the standings (den = 0, a one-transcript
component, resident sets of two size classes), the merge of rows in the packed sets, the TILED numbering under EMSAR_HIP_RENUMBER 0 and
2, and, from the references alone, enough queries of every status.  Nothing here is a tolerance on the device: a change to the
generator, to set_problems.py or to the numbering rule that loses one of these fails here instead of leaving the GPU tests empty."""
import collections

import numpy as np
import pytest

from emsar_amd import hip as H
from tests import awkward_problems as AP
from tests import compare_problems as CP
from tests import profile_problems as PP
from tests import set_problems as SP
from tests import test_presence_gpu as TP
from tests import test_profile_gpu as TF


def selfcheck(prob):
    n_tx, rp, ci, R, E = prob
    return H.sets_selfcheck(n_tx, rp, ci, np.where(E > 0, R, 0).astype(np.int32))


def test_row_forms():
    prob, notes = AP.awkward_members()
    n_tx, rp, ci, R, E = prob
    rows = AP.rows_of(prob)
    assert n_tx == 54 and len(rows) == 118 and sorted(set(int(t) for t in ci)) == list(range(n_tx))
    assert not np.array_equal(np.sort(ci[:20]), ci[:20])                     # the caller's tids are shuffled
    inside = [r for r, e in zip(rows, E) if e > 0]
    repeated = [r for r in inside if len(set(r)) >= 2 and len(set(r)) < len(r)]
    assert sum(max(r.count(t) for t in r) == 2 for r in repeated) >= 4 and sum(max(r.count(t) for t in r) == 3 for r in repeated) >= 4
    assert len(AP.twice_in_a_row(prob)) >= 4
    by_multiset = collections.defaultdict(set)
    for r in inside:
        by_multiset[tuple(sorted(r))].add(r)
    assert sum(len(v) >= 2 for v in by_multiset.values()) >= 4                # the same multiset in another order
    assert sum(c >= 2 for c in collections.Counter(inside).values()) >= 3    # verbatim
    assert [form for form, _, _ in notes["added"]] == list(AP.FORMS) * 4
    for form, old, new in notes["added"]:
        assert old in rows and new in rows and set(old) == set(new) and len(new) - len(old) == {"first_twice": 1, "last_thrice": 2, "reversed": 0}[form]


def test_standings_and_classes():
    prob, notes = AP.awkward_members()
    n_tx, rp, ci, R, E = prob
    rows = AP.rows_of(prob)
    den = CP.den_of(prob)
    assert list(np.flatnonzero(den == 0)) == [notes["outside"]]
    mine = [k for k, r in enumerate(rows) if notes["outside"] in r]
    assert len(mine) == 1 and E[mine[0]] == 0 and R[mine[0]] > 0 and any(den[t] > 0 for t in rows[mine[0]])
    mine = [k for k, r in enumerate(rows) if notes["alone"] in r]
    assert len(mine) == 1 and rows[mine[0]] == (notes["alone"],) and E[mine[0]] > 0 and R[mine[0]] > 0
    d = selfcheck(prob)
    print(d)
    assert d["tids_closed"] == 2 and d["sets_streamed"] == 0 and d["tids_resident"] == n_tx - 2     # the den = 0 one and the one alone
    assert sum(x > 0 for x in d["sets_resident"]) >= 2 and d["sets_resident"][0] >= 1 and d["sets_resident"][1] >= 1
    assert d["max_lds_bytes"][0] <= 6144 < d["max_lds_bytes"][1]
    assert d["rows_stored"] < d["rows_in"]
    RA, RB = AP.awkward_samples()
    for Rs in (RA, RB):                                                       # the two samples of the two-sample test: the same sets
        ds = selfcheck((n_tx, rp, ci, Rs, E))
        assert ds["sets_resident"] == d["sets_resident"] and ds["rows_stored"] == d["rows_stored"] and ds["tids_closed"] == 2


@pytest.mark.parametrize("name", ["awkward", "everything"])
@pytest.mark.parametrize("merge", [False, True])
def test_the_numbering_is_forced_either_way(monkeypatch, name, merge):
    n_tx, rp, ci = (AP.awkward_problem() if name == "awkward" else SP.everything_problem())[:3]
    for mode, want in (("0", 0), ("2", 1)):
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", mode)
        assert H.layout_selfcheck_tiled(n_tx, rp, ci, merge)["renumbered"] == want, (name, merge, mode)


def test_the_subset_covers_what_it_has_to():
    prob, notes = AP.awkward_members()
    q = AP.query_subset()
    assert len(q) == AP.N_QUERY == len(set(q.tolist())) and not np.array_equal(np.sort(q), q)
    assert set(AP.twice_in_a_row(prob)) <= set(q.tolist()) and notes["outside"] in q and notes["alone"] in q
    rows = AP.rows_of(prob)
    merged = {t for r in rows for t in r if sum(sorted(o) == sorted(r) for o in rows) >= 2}
    assert merged & set(q.tolist())


def test_the_presence_reference_has_every_status():
    prob, notes = AP.awkward_members()
    base = TP.full_solve(prob)
    ref = TP.reference(prob, np.arange(prob[0]), base)
    n = collections.Counter(w["status"] for w in ref)
    clear = sum(w["status"] == TP.TESTED and w["clear"] for w in ref)
    print(dict(n), "clear", clear)
    assert n[TP.TESTED] >= 20 and n[TP.ABSENT] >= 3 and n[TP.ESSENTIAL] >= 3 and n[TP.OUTSIDE] == 1
    assert 4 * clear >= 3 * n[TP.TESTED]
    assert ref[notes["outside"]]["status"] == TP.OUTSIDE and ref[notes["alone"]]["status"] == TP.ESSENTIAL
    # the subset: the picks are what their names say, by the rule written next to them, and every status is asked for
    twice = AP.twice_in_a_row(prob)
    for pick, status in ((AP.ABSENT_PICK, TP.ABSENT), (AP.ESSENTIAL_PICK, TP.ESSENTIAL)):
        assert list(pick) == [t for t, w in enumerate(ref) if w["status"] == status and t not in twice and t != notes["alone"]][:2]
    q, sub = AP.presence_reference()
    ns = collections.Counter(w["status"] for w in sub)
    clear = sum(w["status"] == TP.TESTED and w["clear"] for w in sub)
    print("subset", dict(ns), "clear", clear)
    assert ns[TP.TESTED] >= 8 and ns[TP.ABSENT] >= 3 and ns[TP.ESSENTIAL] >= 3 and ns[TP.OUTSIDE] == 1 and 4 * clear >= 3 * ns[TP.TESTED]
    for t, w in zip(q, sub):
        assert w["status"] == ref[t]["status"]


def test_the_profile_reference_decides_both_kinds_and_few_queries_are_excluded():
    """at LEVEL over the subset: at least 3 TWO_SIDED and 3 LOWER_ZERO, at most 1 in 20 too close to the cut (test_profile_gpu's cap)"""
    _, q, lam = AP.profile_reference()
    cut = PP.cut(TF.LEVEL)
    two = zero = out = total = 0
    for lm, scale in lam:
        if lm != lm:
            continue
        total += 1
        if TF.excluded(lm, scale, cut):
            out += 1
        elif lm > cut:
            two += 1
        else:
            zero += 1
    print("two-sided", two, "lower-zero", zero, "excluded", out, "of", total)
    assert two >= 3 and zero >= 3 and 20 * out <= total and total == len(q) - 1


def test_the_compare_reference_runs_on_every_form():
    """the stacked EM of compare_problems takes rows with repeated ids as they stand: it converges for every query, and the two fitted
    samples differ enough for some Lambda to pass the 5 % cut and for some not to"""
    q, ref = AP.compare_reference()
    lam = np.array([r["lam"] for r in ref if r is not None])
    assert sum(r is None for r in ref) == 1 and max(max(r["passes"]) for r in ref if r is not None) < CP.MAX_PASSES
    print("Lambda", np.sort(lam))
    assert np.all(lam > -1e-9) and np.sum(lam > 3.84) >= 3 and np.sum(lam < 3.84) >= 3
