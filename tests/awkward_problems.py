"""A small problem with the row forms that tests/set_problems.py leaves out, shared by test_per_transcript_configs_cpu.py (which pins
what it holds, on the host) and test_per_transcript_configs_gpu.py (which runs presence, profile and compare on it under every layout
and numbering).  EdgeSet promises rows of distinct ids, no two rows the same set; here, on top of four such sets side by side:

    a row with one of its ids repeated           {a, a, b, ..} and {.., y, z, z, z}: the transcript counts twice (three times) in the row's sum
    a row that is another row in another order   the same multiset: build_sets and merge_rows fold the two into one stored row
    a verbatim repeat of a row                   likewise
    a transcript with den = 0                    its only row has E = 0 and is shared with a live transcript: outside the likelihood
    a transcript alone in its only row           a one-transcript component with reads: the closed form, never a member of a packed set

The caller's tids are shuffled (compose), so the TILED layout's own numbering differs from the caller's wherever it is switched on."""
import numpy as np

from tests import compare_problems as CP
from tests import set_problems as SP

SEED = 3                # the generator of the added rows: the first seed tried; test_per_transcript_configs_cpu.py holds what it has to give
N_PICKED = 12
FORMS = ("first_twice", "last_thrice", "reversed")


def rows_of(prob):
    _, rp, ci = prob[:3]
    rp = rp.astype(np.int64)
    return [tuple(int(x) for x in ci[rp[c]:rp[c + 1]]) for c in range(len(rp) - 1)]


def csr_of(rows, n_tx):
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return n_tx, rp, np.concatenate([np.array(r, dtype=np.int32) for r in rows]).astype(np.int32)


_cache = {}


def awkward_members():
    """-> (prob, notes): prob = (n_tx, rp, ci, R, E); notes = dict(outside: the den = 0 transcript, alone: the closed-form one,
    added: [(form, picked row, new row)] with the rows as tuples of caller tids, repeats: [row] repeated verbatim)"""
    if "awkward" not in _cache:
        sets = [SP.family(4, 1), SP.edge_set(*SP.EDGES[0][0], seed=SP.SEEDS[0]), SP.family(3, 2), SP.family(5, 3)]
        n_tx, rp, ci, R, E = SP.compose(sets, seed=17)
        rows, R, E = rows_of((n_tx, rp, ci)), [int(x) for x in R], [float(x) for x in E]
        rng = np.random.default_rng(SEED)
        multi = [k for k, r in enumerate(rows) if len(set(r)) >= 2 and E[k] > 0]
        picked = [int(k) for k in rng.choice(multi, size=N_PICKED, replace=False)]
        added = []
        for j, k in enumerate(picked):
            r, form = rows[k], FORMS[j % 3]
            new = (r[0],) + r if form == "first_twice" else r + (r[-1], r[-1]) if form == "last_thrice" else r[::-1]
            added.append((form, r, new))
            rows.append(new)
            R.append(int(rng.integers(1, 30)))
            E.append(E[k])
        repeats = []
        for k in picked[:3]:
            repeats.append(rows[k])
            rows.append(rows[k])
            R.append(int(rng.integers(1, 30)))
            E.append(E[k])
        live = rows[picked[3]][0]
        outside, alone = n_tx, n_tx + 1
        rows.append((live, outside))             # E = 0: outside the likelihood, and the only row of `outside`
        R.append(int(rng.integers(1, 30)))
        E.append(0.0)
        rows.append((alone,))
        R.append(int(rng.integers(1, 30)))
        E.append(float(rng.uniform(0.5, 2.0)))
        n_tx += 2
        order = rng.permutation(len(rows))
        n_tx, rp, ci = csr_of([rows[k] for k in order], n_tx)
        prob = (n_tx, rp, ci, np.array(R, dtype=np.int32)[order], np.array(E)[order])
        _cache["awkward"] = (prob, dict(outside=outside, alone=alone, added=added, repeats=repeats))
    return _cache["awkward"]


def awkward_problem():
    return awkward_members()[0]


def awkward_samples():
    """two fitted samples over awkward_problem() for the two-sample test, apart in every third transcript -> (RA, RB)"""
    if "samples" not in _cache:
        prob = awkward_problem()
        _cache["samples"] = (CP.fitted_weights(prob, 41), CP.fitted_weights(prob, 42, apart=range(0, prob[0], 3)))
    return _cache["samples"]


def twice_in_a_row(prob):
    """the transcripts that occur more than once in some row of two or more distinct transcripts"""
    out = set()
    for r in rows_of(prob):
        if len(set(r)) >= 2:
            out |= {t for t in r if r.count(t) > 1}
    return sorted(out)


N_QUERY = 20
# the first two transcripts by tid, outside those twice_in_a_row names, that the presence reference calls ABSENT and ESSENTIAL inside a
# set (test_per_transcript_configs_cpu.py holds the reference to it)
ABSENT_PICK = (7, 10)
ESSENTIAL_PICK = (25, 42)


def query_subset():
    """The N_QUERY transcripts that the device is compared with the references on, in a fixed shuffled order: every transcript that
    occurs twice in some row, the first member of a reversed row and of a verbatim repeat, the den = 0 transcript, the one alone in its
    row, ABSENT_PICK and ESSENTIAL_PICK, and others drawn by the seed up to N_QUERY."""
    prob, notes = awkward_members()
    need = set(twice_in_a_row(prob)) | {notes["outside"], notes["alone"]} | set(ABSENT_PICK) | set(ESSENTIAL_PICK)
    need |= {[new for form, _, new in notes["added"] if form == "reversed"][0][0], notes["repeats"][0][0]}
    rng = np.random.default_rng(SEED + 1)
    rest = [t for t in range(prob[0]) if t not in need]
    q = sorted(need) + [int(t) for t in rng.choice(rest, size=N_QUERY - len(need), replace=False)]
    return np.array(q, dtype=np.int32)[rng.permutation(len(q))]


def presence_reference(tol=1e-12):
    """tests.test_presence_gpu.reference over query_subset() -> (tids, per-tid dicts)"""
    from tests import test_presence_gpu as TP
    if ("presence", tol) not in _cache:
        prob, q = awkward_problem(), query_subset()
        _cache["presence", tol] = (q, TP.reference(prob, q, TP.full_solve(prob, tol), tol))
    return _cache["presence", tol]


def profile_reference():
    """tests.profile_problems.Reference of the problem and, over query_subset(), the reference's Lambda and |F_full| + |F_drop| as
    profile_problems.oracle_case gives them -> (Reference, tids, [(Lambda, scale)])"""
    from tests import profile_problems as PP
    if "profile" not in _cache:
        ref, q = PP.Reference(awkward_problem()), query_subset()
        lam = []
        for t in q:
            if ref.den[t] == 0:
                lam.append((np.nan, np.nan))
            elif ref.theta[t] * ref.den[t] < 1e-9:
                lam.append((0.0, 2 * abs(ref.F)))
            else:
                d, scale = ref.deviance(int(t), 0.0)
                lam.append((max(d, 0.0), scale))
        _cache["profile"] = (ref, q, lam)
    return _cache["profile"]


def compare_reference():
    """compare_problems.reference of awkward_samples() over query_subset() -> (tids, per-tid dicts; None where den = 0)"""
    if "compare" not in _cache:
        prob, q, (RA, RB) = awkward_problem(), query_subset(), awkward_samples()
        den = CP.den_of(prob)
        _cache["compare"] = (q, [CP.reference(prob, RA, RB, int(t)) if den[t] > 0 else None for t in q])
    return _cache["compare"]


def measure_spreads(level=0.95):
    """the two references against themselves on this problem, tol 1e-10 against 1e-13, over EVERY transcript (query_subset() is among
    them): presence as max |dLambda| / (|F_full| + |F_drop|) over the TESTED ones, profile as max |dD| / (|F_full| + |F_pinned|) at the
    reference's own limits (profile_problems.measure_spread, on this problem)"""
    from tests import profile_problems as PP
    from tests import test_presence_gpu as TP
    prob = awkward_problem()
    q = np.arange(prob[0])
    a, b = (TP.reference(prob, q, TP.full_solve(prob, tol), tol) for tol in (1e-10, 1e-13))
    assert [x["status"] for x in a] == [y["status"] for y in b]
    pres = max(abs(x["lam"] - y["lam"]) / x["scale"] for x, y in zip(a, b) if x["status"] == TP.TESTED)
    print("presence: max |dLambda| / scale", pres, flush=True)
    ref, c, prof = PP.Reference(prob), PP.cut(level), 0.0
    for t in q:
        if ref.den[t] == 0:
            continue
        lm = 0.0 if ref.theta[t] * ref.den[t] < 1e-9 else max(ref.deviance(int(t), 0.0)[0], 0.0)
        for side in ((0, 1) if lm > c else (1,)):
            x = ref.limit(int(t), side, c)
            d10, scale = ref.deviance(int(t), x, 1e-10)
            d13, _ = ref.deviance(int(t), x, 1e-13)
            prof = max(prof, abs(d10 - d13) / scale)
            print("profile", int(t), side, "x", x, "D", d10, "spread / scale", abs(d10 - d13) / scale, "worst", prof, flush=True)
    return pres, prof


if __name__ == "__main__":
    print("presence, profile spread", measure_spreads())
