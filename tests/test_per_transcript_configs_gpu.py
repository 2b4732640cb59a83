"""GPU: the three per-transcript calls (emsar_hip_presence, emsar_hip_profile, emsar_hip_compare) under every layout and numbering, and
on the row forms that tests/set_problems.py leaves out.

Configurations (CONFIGS): CSR; TILED in the caller's numbering and in the library's own (EMSAR_HIP_RENUMBER 0 and 2, asserted through
info() after every upload), each with and without MERGE_ROWS.  The sets are found and packed on the caller's CSR and only their tid lists
are mapped, so every output of the three calls is the SAME BYTES in all five, whichever configuration each of the two contexts of a
compare is in: a difference is a bug in one of the caller/library translations (SetQuery::lib_of, cand_of_lib, kind / den / theta by
library index, the heir's way back), not noise.  den is passed from the host everywhere: summed on the device it comes from floating
atomics and differs from process to process, which is not what is tested here.

Problems: tests/awkward_problems.py (54 transcripts: repeated tids inside multi-transcript rows, rows that are other rows reordered or
repeated, a den = 0 transcript, a one-transcript component; test_per_transcript_configs_cpu.py pins all that) with every transcript
queried, and set_problems.everything_problem() (all three classes and a streamed set) with fixed subsets.

Against the references (tests.test_presence_gpu.reference, profile_problems.Reference, compare_problems.reference) the device is judged
as test_presence_gpu / test_profile_gpu::test_against_the_oracle and test_compare_gpu::test_independent_reference judge, with their
constants.  Those constants are 100 x the references' own spread (tol 1e-10 against 1e-13) on the problems of those modules: 4.26e-15
and 3.87e-15 of |F_full| + |F_other|.  On awkward_problem() the same measurement (`python -m tests.awkward_problems`, every transcript,
the 20 queried ones among them) gives 5.6e-16 for presence (39 tested transcripts) and 7.8e-16 for profile (89 limits): inside the
recorded spreads, so LAMBDA_REL of either module is reused as it stands.  compare reuses TOL = dev_tol + 8 e_F, e_F having been measured
on larger |F| than this problem has.

Every call passes max_iter <= 20000 and at most 30 (profile) or the default 40 (compare) evaluations: no workgroup can run long."""
import math

import numpy as np
import pytest

import emsar_amd
from emsar_amd import hip as H
from tests import awkward_problems as AP
from tests import compare_problems as CP
from tests import set_problems as SP
from tests import test_compare_gpu as TC
from tests import test_presence_gpu as TP
from tests import test_profile_gpu as TF

pytestmark = pytest.mark.gpu

# (layout, merge_rows, EMSAR_HIP_RENUMBER; None = unset)
CONFIGS = [(H.LAYOUT_CSR, False, None), (H.LAYOUT_TILED, False, "0"), (H.LAYOUT_TILED, False, "2"), (H.LAYOUT_TILED, True, "0"),
           (H.LAYOUT_TILED, True, "2")]
IDS = ["csr", "tiled-caller", "tiled-library", "tiled-merged-caller", "tiled-merged-library"]
CSR, TILED_CALLER, TILED_LIBRARY, MERGED_CALLER, MERGED_LIBRARY = range(5)
MIXED = [(CSR, TILED_LIBRARY), (MERGED_LIBRARY, TILED_CALLER), (TILED_CALLER, MERGED_LIBRARY)]
PRESENCE_OUTPUTS = ("lambda", "pvalue", "heir", "heir_share", "status", "theta_hat")
STATS = {"presence": ("n_status", "items_launched", "drop_passes_sum", "drop_passes_max", "min_raw_lambda"),
         "profile": ("n_status", "items_launched", "evals_sum", "evals_max", "passes_sum", "passes_max", "cut"),
         "compare": ("n_status", "items_launched", "evals_sum", "evals_max", "passes_sum", "passes_max", "min_raw_lambda")}
OUTPUTS = {"presence": PRESENCE_OUTPUTS, "profile": TF.OUTPUTS, "compare": TC.OUTPUTS}


class Case:
    """a problem, two further samples over it for compare, the queries of each call and the iteration caps"""

    def __init__(self, name):
        self.name = name
        if name == "awkward":
            self.prob = AP.awkward_problem()
            self.RA, self.RB = AP.awkward_samples()
            self.streamed = np.zeros(self.prob[0], dtype=bool)
            self.q = dict.fromkeys(("presence", "profile", "compare"), np.arange(self.prob[0], dtype=np.int32))
            self.cap = 20000
        else:
            # the caps of test_presence_gpu / test_profile_gpu on this problem; a seeded subset in drawn (non-monotone) order with one
            # tid asked for twice; about a third of it lies in the streamed set (asserted where the results are compared)
            self.prob = SP.everything_problem()
            sets = [SP.edge_set(*shape, seed=SP.SEEDS[k]) for k, (shape, _, _) in enumerate(SP.EDGES)] + [SP.ragged_set()]
            again = SP.compose_members(sets, seed=12)                      # everything_problem() once more, for the membership
            assert all(np.array_equal(x, y) for x, y in zip(self.prob[1:], again[1:5]))
            self.streamed = np.zeros(self.prob[0], dtype=bool)            # the transcripts of the set that is left to the streaming passes
            self.streamed[again[5][[e[2] for e in SP.EDGES].index(SP.STREAMED)][0]] = True
            self.RA, self.RB = CP.fitted_weights(self.prob, 41), CP.fitted_weights(self.prob, 42, apart=range(0, self.prob[0], 3))
            rng = np.random.default_rng(3)
            self.q = {}
            for call, count in (("presence", 200), ("profile", 60), ("compare", 60)):
                q = rng.choice(self.prob[0], size=count - 1, replace=False).astype(np.int32)
                self.q[call] = np.concatenate([q, q[:1]])
                assert not np.array_equal(np.sort(q), q)
            self.cap = 3000
        self.den = CP.den_of(self.prob)
        n_tx, rp, ci, R, E = self.prob
        for x in (rp, ci, R, E, self.den, self.RA, self.RB):
            x.setflags(write=False)
        # the label of every transcript's connected set, in numpy on the caller's CSR (rows inside the likelihood with reads)
        parent = np.arange(n_tx)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        rp64 = rp.astype(np.int64)
        for c in np.flatnonzero((R > 0) & (E > 0)):
            r0 = find(ci[rp64[c]])
            for k in range(rp64[c] + 1, rp64[c + 1]):
                parent[find(ci[k])] = r0
        self.label = np.array([find(t) for t in range(n_tx)])


_cases, _results = {}, {}


def case_of(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module")
def devs():
    with emsar_amd.EmsarHip(0) as a, emsar_amd.EmsarHip(0) as b:
        yield a, b


def upload(dev, case, R, config, monkeypatch):
    layout, merge, mode = CONFIGS[config]
    if mode is None:
        monkeypatch.delenv("EMSAR_HIP_RENUMBER", raising=False)
    else:
        monkeypatch.setenv("EMSAR_HIP_RENUMBER", mode)
    n_tx, rp, ci, _, E = case.prob
    dev.upload_structure(n_tx, rp, ci, layout, merge)
    dev.upload_sample(R, E, case.den)
    info = dev.info()
    assert info["layout"] & 0xFF == layout
    if layout == H.LAYOUT_TILED:
        assert info["renumbered"] == int(mode == "2"), (IDS[config], info)


def run(devs, monkeypatch, name, cfg_a, cfg_b=None):
    """the three calls (compare alone where the two contexts differ in their configuration) on a case, once per session"""
    key = (name, cfg_a, cfg_b)
    if key not in _results:
        a, b = devs
        case, out = case_of(name), {}
        kw = dict(max_iter=case.cap)
        if cfg_b is None:
            upload(a, case, case.prob[3], cfg_a, monkeypatch)
            out["solve"] = a.solve(**kw)[0]
            out["presence"] = a.presence(case.q["presence"], **kw)
            out["profile"] = a.profile(case.q["profile"], level=TF.LEVEL, max_evals=30, **kw)
            out["solve_after"] = a.solve(**kw)[0]
        upload(a, case, case.RA, cfg_a, monkeypatch)
        upload(b, case, case.RB, cfg_a if cfg_b is None else cfg_b, monkeypatch)
        out["compare"] = a.compare(b, case.q["compare"], **kw)
        _results[key] = out
    return _results[key]


def differences(call, got, want):
    """the outputs and the stats fields of one call that are not the same bytes in two runs"""
    bad = [k for k in OUTPUTS[call] if got[k].tobytes() != want[k].tobytes()]
    g, w = got["stats"].as_dict(), want["stats"].as_dict()
    return bad + ["stats." + k for k in STATS[call] if repr(g[k]) != repr(w[k])]


def check_one_run(case, out):
    """what a run has to satisfy by itself, whatever its configuration: theta_hat is solve's, the heir is a caller tid of the queried
    transcript's own connected set, nothing the calls did shows in a following solve, and every kind of answer occurs"""
    pres, prof, cmp_ = out["presence"], out["profile"], out["compare"]
    resident = ~case.streamed                              # the streamed set adds with floating atomics: no two solves of it agree
    assert out["solve_after"][resident].tobytes() == out["solve"][resident].tobytes()
    for call, r, word in (("presence", pres, TP.NOT_RESIDENT), ("profile", prof, TF.NOT_RESIDENT), ("compare", cmp_, TC.NOT_RESIDENT)):
        assert np.array_equal(r["status"] == word, case.streamed[case.q[call]]), call
    q = case.q["presence"]
    given = pres["status"] != TP.NOT_RESIDENT
    assert pres["theta_hat"][given].tobytes() == out["solve"][q][given].tobytes()
    tested = pres["status"] == TP.TESTED
    heir = pres["heir"]
    assert np.all(heir[~tested & (pres["status"] != TP.UNCONVERGED)] == -1) and np.all((heir >= -1) & (heir < case.prob[0]))
    has = tested & (heir >= 0)
    assert has.sum() >= 20 and np.all(heir[has] != q[has]) and np.array_equal(case.label[heir[has]], case.label[q[has]])
    q = case.q["profile"]
    given = ~np.isin(prof["status"], (TF.OUTSIDE, TF.NOT_RESIDENT))
    assert given.sum() >= 20 and prof["theta_hat"][given].tobytes() == out["solve"][q][given].tobytes()
    ns = [pres["stats"].as_dict()["n_status"], prof["stats"].as_dict()["n_status"], cmp_["stats"].as_dict()["n_status"]]
    print(case.name, ns)
    assert ns[0]["TESTED"] >= 20 and ns[0]["ABSENT"] >= 1 and ns[0]["ESSENTIAL"] >= 3 and ns[1]["TWO_SIDED"] >= 3 and ns[1]["LOWER_ZERO"] >= 3
    assert ns[2]["TESTED"] >= 10
    if case.name == "awkward":
        assert ns[0]["OUTSIDE"] == ns[1]["OUTSIDE"] == ns[2]["OUTSIDE"] == 1 and ns[0]["NOT_RESIDENT"] == 0 and ns[0]["ABSENT"] >= 3
        return
    for n, call in zip(ns, ("presence", "profile", "compare")):
        assert 5 <= n["NOT_RESIDENT"] < len(set(case.q[call].tolist())) - 20, call                  # streamed transcripts are asked for
    for call, r in (("presence", pres), ("profile", prof), ("compare", cmp_)):                      # the tid asked for twice
        for k in OUTPUTS[call]:
            assert r[k][-1:].tobytes() == r[k][:1].tobytes(), (call, k)


@pytest.mark.parametrize("name", ["awkward", "everything"])
@pytest.mark.parametrize("config", range(len(CONFIGS)), ids=IDS)
def test_same_bits_in_every_configuration(devs, monkeypatch, name, config):
    case = case_of(name)
    want = run(devs, monkeypatch, name, CSR)
    got = run(devs, monkeypatch, name, config)
    check_one_run(case, got)
    for call in ("presence", "profile", "compare"):
        assert not differences(call, got[call], want[call]), (name, IDS[config], call)
    assert got["solve"][~case.streamed].tobytes() == want["solve"][~case.streamed].tobytes()


@pytest.mark.parametrize("name", ["awkward", "everything"])
@pytest.mark.parametrize("pair", MIXED, ids=["%s+%s" % (IDS[x], IDS[y]) for x, y in MIXED])
def test_mixed_contexts_in_one_compare(devs, monkeypatch, name, pair):
    """sample A and sample B live in contexts of different layouts and numberings: the bytes of both under CSR"""
    want = run(devs, monkeypatch, name, CSR)["compare"]
    got = run(devs, monkeypatch, name, *pair)["compare"]
    assert not differences("compare", got, want), (name, pair)
    assert got["stats"].as_dict()["n_status"]["TESTED"] >= 10


REFERENCE_CONFIGS = [CSR, MERGED_LIBRARY]
REFERENCE_IDS = [IDS[c] for c in REFERENCE_CONFIGS]


@pytest.mark.parametrize("config", REFERENCE_CONFIGS, ids=REFERENCE_IDS)
def test_presence_against_the_oracle(devs, monkeypatch, config):
    """as test_presence_gpu.test_against_the_oracle: statuses exactly; Lambda within LAMBDA_REL * (|F_full| + |F_drop|) + 1e-7 * Lambda;
    the heir and its share wherever the reference's heir is clear"""
    a, _ = devs
    case = case_of("awkward")
    q, ref = AP.presence_reference()
    upload(a, case, case.prob[3], config, monkeypatch)
    r = a.presence(q, tol=1e-12, max_iter=case.cap)
    worst = 0.0
    for i, (t, w) in enumerate(zip(q, ref)):
        assert r["status"][i] == w["status"], (int(t), int(r["status"][i]), w)
        if w["status"] == TP.TESTED:
            bound = TP.LAMBDA_REL * w["scale"] + 1e-7 * w["lam"]
            worst = max(worst, abs(r["lambda"][i] - w["lam"]) / bound)
            assert abs(r["lambda"][i] - w["lam"]) <= bound, (int(t), r["lambda"][i], w["lam"], bound)
            if w["clear"]:
                assert r["heir"][i] == w["heir"], (int(t), int(r["heir"][i]), w)
                assert abs(r["heir_share"][i] - w["share"]) <= 1e-6 * max(1.0, w["share"]), (int(t), r["heir_share"][i], w["share"])
        if w["status"] in (TP.ABSENT, TP.ESSENTIAL):
            assert r["lambda"][i] == w["lam"]
    print(IDS[config], "queried", len(q), "worst |dLambda| / bound", worst, "min raw Lambda", r["stats"].min_raw_lambda)


@pytest.mark.parametrize("config", REFERENCE_CONFIGS, ids=REFERENCE_IDS)
def test_profile_against_the_oracle(devs, monkeypatch, config):
    """as test_profile_gpu.test_against_the_oracle: statuses exactly; every searched limit on the reference's profile curve within
    LAMBDA_REL * (|F_full| + |F_pinned|) + 1e-7 q and on the cut within dev_tol; lower <= theta_hat <= upper"""
    a, _ = devs
    case = case_of("awkward")
    ref, tids, lam = AP.profile_reference()
    upload(a, case, case.prob[3], config, monkeypatch)
    r = a.profile(tids, level=TF.LEVEL, tol=1e-12, **TF.CAPS)
    q = H.profile_cut_host(TF.LEVEL)
    worst = 0.0
    for i, (t, (lm, scale)) in enumerate(zip(tids, lam)):
        if lm != lm:
            assert r["status"][i] == TF.OUTSIDE, int(t)
            continue
        if TF.excluded(lm, scale, q):
            continue
        want = TF.LOWER_ZERO if lm <= q else TF.TWO_SIDED
        assert r["status"][i] == want, (int(t), int(r["status"][i]), lm, r["lambda"][i])
        assert r["lower"][i] <= r["theta_hat"][i] <= r["upper"][i], int(t)
        if want == TF.LOWER_ZERO:
            assert r["lower"][i] == 0.0 and r["dev_lower"][i] == r["lambda"][i]
        for k in (("lower", "upper") if want == TF.TWO_SIDED else ("upper",)):
            x, dv = r[k][i], r["dev_" + k][i]
            d_ref, sc = ref.deviance(int(t), float(x))
            bound = TF.LAMBDA_REL * sc + 1e-7 * q
            worst = max(worst, abs(d_ref - dv) / bound)
            assert TF.on_the_cut(dv, q), (int(t), k, x, dv, q)
            assert abs(d_ref - dv) <= bound, (int(t), k, x, d_ref, dv, bound)
    st = r["stats"].as_dict()
    print(IDS[config], "queried", len(tids), "worst |dD| / bound", worst, "evals max", st["evals_max"], "passes max", st["passes_max"], st["n_status"])


@pytest.mark.parametrize("config", REFERENCE_CONFIGS, ids=REFERENCE_IDS)
def test_compare_against_the_reference(devs, monkeypatch, config):
    """as test_compare_gpu.test_independent_reference: TESTED, Lambda within TOL = dev_tol + 8 e_F of numpy's, the three estimates, p and
    the fold change; the den = 0 transcript OUTSIDE"""
    a, b = devs
    case = case_of("awkward")
    tids, ref = AP.compare_reference()
    upload(a, case, case.RA, config, monkeypatch)
    upload(b, case, case.RB, config, monkeypatch)
    r = a.compare(b, tids, tol=1e-12, **TC.CAPS)
    for i, (t, w) in enumerate(zip(tids, ref)):
        if w is None:
            assert r["status"][i] == TC.OUTSIDE and math.isnan(r["lambda"][i])
            continue
        print(IDS[config], int(t), "Lambda", r["lambda"][i], "ref", w["lam"], "diff", r["lambda"][i] - w["lam"], "evals", r["evals"][i], "n", w["n"])
        assert r["status"][i] == TC.TESTED
        assert abs(r["lambda"][i] - w["lam"]) <= TC.TOL, (int(t), r["lambda"][i], w["lam"])
        assert abs(r["theta_a"][i] - w["theta_a"]) <= 1e-6 * w["theta_a"] and abs(r["theta_b"][i] - w["theta_b"]) <= 1e-6 * w["theta_b"]
        assert abs(r["theta_null"][i] - w["theta_null"]) <= 1e-3 * w["theta_null"]
        assert r["pvalue"][i] == H.compare_pvalue_host(r["lambda"][i])
        assert abs(r["log2fc"][i] - math.log2(w["theta_a"] / w["theta_b"])) <= 1e-5
    st = r["stats"].as_dict()
    on_device = tids != AP.awkward_members()[1]["alone"]                # the one-transcript component is searched on the host
    assert st["evals_sum"] == int(r["evals"][on_device].sum()) and st["items_launched"] == len(tids) - 2
    assert st["n_status"]["TESTED"] == len(tids) - 1 and st["n_status"]["OUTSIDE"] == 1
