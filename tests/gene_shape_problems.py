"""Problems, samples, genes and references for the two-sample and gene-level set kernels off the diagonal of their size classes, shared by
test_gene_shapes_cpu.py (which pins what they hold, on the host) and test_gene_shapes_gpu.py (which compares the device with the
references).  The shapes are those of tests/set_problems.py, the samples CP.fitted_weights at its scale of 30, the references
CP.reference, GP.reference, PG.Gene and UP.reference unchanged; nothing the device computes enters anything here.

    A  one set per problem: EDGES[k] for k in A_EDGES and the ragged set (k = RAGGED, its gene: ragged_problem), each under RA = fitted_weights(1000 + k) and
       RB = fitted_weights(2000 + k, apart = local 0 and 7).  The gene is local 0, 7 and 3; the usage test queries local 0.
    B  "two_trips": edge_set(300, 310, 640): 30 944 bytes, the 256 class with 300 transcripts -- a 256 launch goes over the transcripts
       twice.  The gene holds the local ids 3, 130, 262 and 290, the queried transcripts are 3 and 290.
    C  "mix": four families, EDGES[0] and [2] (class 0), [1] and [3] (class 1), [7] (class 2) side by side and one lone transcript with
       reads.  Genes g512_256, g_three, g_many (a member in each of the nine sets), g256_64x2.  "mix2" is the same pair of samples with
       den = 0 in sample B for g_three's class-2 member: the launch class comes from sample A alone.  "mixlow" is a third sample in
       which g256_64x2's members are all but absent (the LOWER_ZERO case of the gene profile).

The gene and usage references are recorded in tests/golden/gene_shape_refs.json (`python -m tests.gene_shape_problems --write [NAME ..]`
computes them: from a tenth of a second to ten minutes per entry); test_gene_shapes_cpu.py recomputes one of each kind and holds every entry to its
conditions."""
import json
import os

import numpy as np

from tests import awkward_problems as AP
from tests import compare_gene_problems as GP
from tests import compare_problems as CP
from tests import compare_usage_problems as UP
from tests import set_problems as SP

A_EDGES = (1, 2, 3, 5, 6, 7)
RAGGED = 10                                   # the ragged set's place in the numbering of the seeds: EDGES ends at 9
TWO_TRIPS_SHAPE = (300, 310, 640)
# Of the eight seeds 300 + 10 j the one whose two samples CP.em fits freely in the fewest passes (python -m tests.gene_shape_problems
# --pick-seed prints them), as SP.SEEDS was picked; nothing the device computes entered the choice.
TWO_TRIPS_SEED = 300
TWO_TRIPS_FACTOR = 1.6
# Caller tids: the problem is one set of tids 0 .. 299 and the library numbers a set's transcripts by ascending tid, so these ARE the
# local ids of the kernels (under CSR and every layout in the caller's numbering), on either side of 256.
TWO_TRIPS_GENE = (3, 130, 262, 290)
TWO_TRIPS_TESTED = (3, 290)
MIX_SETS = ("family3", "edge0", "family5", "edge2", "edge1", "family5b", "edge3", "family3b", "edge7")
MIX_CLASSES = (0, 0, 0, 0, 1, 0, 1, 0, 2)
LOW_FACTOR = 0.02                             # presence Lambda 1.2: below the 0.95 cut, and an interior optimum that the EM reaches quickly

_cache = {}


def _one_set(s, compose_seed, k, locals_gene, locals_tested, usage_local=0, apart_gene=False, factor=1.6, by_tid=False):
    """one set alone under RA = fitted_weights(1000 + k) and RB = fitted_weights(2000 + k, apart = the tested transcripts, or the gene)"""
    n_tx, rp, ci, R, E, members = SP.compose_members([s], seed=compose_seed)
    prob = (n_tx, rp, ci, R, E)
    loc = np.arange(n_tx) if by_tid else members[0][0]
    tids = [int(loc[i]) for i in locals_tested]
    gene = [int(loc[i]) for i in locals_gene]
    den = CP.den_of(prob)
    return dict(prob=prob, RA=CP.fitted_weights(prob, 1000 + k), RB=CP.fitted_weights(prob, 2000 + k, apart=gene if apart_gene else tids, factor=factor),
                den_a=den, den_b=den, tids=tids, genes={"gene": gene}, t={"gene": int(loc[usage_local])}, local=loc)


def edge_problem(k):
    """problem A for EDGES[k] -> dict(prob, RA, RB, den_a, den_b, tids, genes, t, local)"""
    if ("edge", k) not in _cache:
        _cache["edge", k] = _one_set(SP.edge_set(*SP.EDGES[k][0], seed=SP.SEEDS[k]), 200 + k, k, (0, 7, 3), (0, 7))
    return _cache["edge", k]


def ragged_problem():
    """The ragged set has 60 transcripts in 26 rows: the sum of three arbitrary transcripts is not identified (GP.reference finds Lambda =
    8e-9 for local 0, 7, 3 whose sums differ by a tenth: a ridge, on which no two solvers need agree).  A transcript with a row of its
    own has a strictly concave term u log x and a unique estimate, so the gene is the first three of those by local id and the tested
    transcripts the first two."""
    if "ragged" not in _cache:
        n_tx, rp, ci, R, E, members = SP.compose_members([SP.ragged_set()], seed=7)
        own = {r[0] for r, e in zip(AP.rows_of((n_tx, rp, ci)), E) if len(r) == 1 and e > 0}
        locs = [i for i, t in enumerate(members[0][0]) if int(t) in own]
        _cache["ragged"] = _one_set(SP.ragged_set(), 7, RAGGED, locs[:3], locs[:2], usage_local=locs[0])
    return _cache["ragged"]


def two_trips_problem(seed=TWO_TRIPS_SEED):
    """problem B: samples 1300 and 2300; the whole gene lies apart in sample B"""
    if ("two_trips", seed) not in _cache:
        _cache["two_trips", seed] = _one_set(SP.edge_set(*TWO_TRIPS_SHAPE, seed=seed), 211, 300, TWO_TRIPS_GENE, TWO_TRIPS_TESTED,
                                             usage_local=TWO_TRIPS_TESTED[1], apart_gene=True, by_tid=True, factor=TWO_TRIPS_FACTOR)
    return _cache["two_trips", seed]


def mix_sets():
    E = lambda k: SP.edge_set(*SP.EDGES[k][0], seed=SP.SEEDS[k])
    return [SP.family(3, 21), E(0), SP.family(5, 22), E(2), E(1), SP.family(5, 23), E(3), SP.family(3, 24), E(7)]


def mix_problem():
    """problem C -> dict(prob, RA, RB, RL, den_a, den_b, den_b2, genes, t, members, alone)"""
    if "mix" not in _cache:
        n_tx, rp, ci, R, E, members = SP.compose_members(mix_sets(), seed=31)
        rows, R, E = AP.rows_of((n_tx, rp, ci)), [int(x) for x in R], [float(x) for x in E]
        rng = np.random.default_rng(32)
        alone = n_tx                               # a transcript alone in its only row, as awkward_members appends one: a closed-form part
        rows.append((alone,))
        R.append(int(rng.integers(1, 30)))
        E.append(float(rng.uniform(0.5, 2.0)))
        order = rng.permutation(len(rows))
        n_tx, rp, ci = AP.csr_of([rows[k] for k in order], n_tx + 1)
        prob = (n_tx, rp, ci, np.array(R, dtype=np.int32)[order], np.array(E)[order])
        loc = lambda k, i: int(members[k][0][i])
        genes = {
            "g512_256": [loc(8, 5), loc(4, 5)],
            "g_three": [loc(1, 3), loc(6, 4), loc(8, 20), alone],
            "g_many": [loc(k, 1) for k in range(len(MIX_SETS))],
            "g256_64x2": [loc(1, 10), loc(3, 2), loc(4, 12)],
        }
        t = {"g512_256": loc(8, 5), "g_three": loc(1, 3), "g_many": loc(4, 1), "g256_64x2": loc(1, 10)}
        den = CP.den_of(prob)
        den_b2 = den.copy()
        den_b2[loc(8, 20)] = 0.0
        _cache["mix"] = dict(prob=prob, RA=CP.fitted_weights(prob, 1500), RB=CP.fitted_weights(prob, 2500, apart=sorted(t.values())),
                             RL=CP.fitted_weights(prob, 3500, apart=genes["g256_64x2"], factor=LOW_FACTOR), den_a=den, den_b=den, den_b2=den_b2,
                             genes=genes, t=t, members=members, alone=alone, tids=[t["g512_256"], t["g_three"]])
    return _cache["mix"]


MIX_GENES = ("g512_256", "g_three", "g_many", "g256_64x2")
EDGE_CASES = tuple("edge%d" % k for k in A_EDGES)
# every gene the GPU tests compare with GP.reference and PG.Gene, by name
GENE_CASES = EDGE_CASES + ("ragged", "two_trips") + tuple("mix:" + g for g in MIX_GENES) + ("mix2:g_three",)
# every (gene, t) they compare with UP.reference
USAGE_CASES = ("edge1", "edge3", "edge6", "ragged", "two_trips", "mix:g512_256", "mix:g_three", "mix:g_many", "mix2:g_three")
# the single-sample cases of the gene profile: sample A of every gene case ("mix2:g_three": sample B, where the class-2 member has den = 0)
# and the sample in which g256_64x2 is all but absent
PROFILE_CASES = GENE_CASES + ("mixlow:g256_64x2",)
# the problems of the transcript test: (name, its two queried transcripts)
COMPARE_CASES = EDGE_CASES + ("ragged", "two_trips")


def problem(name):
    """the problem dict behind a case name"""
    head = name.partition(":")[0]
    if head.startswith("edge"):
        return edge_problem(int(head[4:]))
    return ragged_problem() if head == "ragged" else two_trips_problem() if head == "two_trips" else mix_problem()


def case(name):
    """-> (prob, RA, RB, den_a, den_b, members, t) as UP.case returns it"""
    p = problem(name)
    head, _, g = name.partition(":")
    g = g or "gene"
    return p["prob"], p["RA"], p["RB"], p["den_a"], p["den_b2"] if head == "mix2" else p["den_b"], p["genes"][g], p["t"][g]


def profile_case(name):
    """-> (prob, R, den, members) of a PROFILE_CASES name"""
    prob, RA, RB, den_a, den_b, members, _ = case(name)
    head = name.partition(":")[0]
    if head == "mixlow":
        return prob, mix_problem()["RL"], den_a, members
    return (prob, RB, den_b, members) if head == "mix2" else (prob, RA, den_a, members)


def part_classes(prob, R, den, members):
    """the size classes of the set parts of a gene in one sample, in GP.parts_of's order, by the library's own packing of each part's rows
    alone (H.sets_selfcheck); a closed-form part (one transcript) is left out -> list of 0 / 1 / 2"""
    from emsar_amd import hip as H
    n_tx, rp, ci, _, E = prob
    out = []
    for t in sorted(int(m) for m in members):
        if not den[t] > 0 or any(t in seen for seen, _ in out):
            continue
        tids, rows = CP.component(prob, R, t)
        w = np.zeros(len(R), dtype=np.int32)
        w[rows] = R[rows]
        d = H.sets_selfcheck(n_tx, rp, ci, w)
        assert sum(d["sets_resident"]) + d["sets_streamed"] <= 1
        out.append((set(int(x) for x in tids), d["sets_resident"].index(1) if sum(d["sets_resident"]) else None))
    return [c for _, c in out if c is not None]


# ---- the references ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gene_shape_refs.json")
GENE_KEPT = ("lam", "w_ref", "lo", "hi", "F1", "gene_a", "gene_b", "gene_null", "multiplier", "parts", "evals")
W_REF_MAX = 1e-7
# the searches of GP.reference in the order they are tried until w_ref <= W_REF_MAX
GENE_SEARCHES = (("secant", 14), ("secant", 24), ("bisect", 50))


def gene_reference(name):
    """GP.reference of a GENE_CASES name, by the first of GENE_SEARCHES that is narrow enough -> dict of GP.reference"""
    prob, RA, RB, den_a, den_b, members, _ = case(name)
    for method, evals in GENE_SEARCHES:
        r = GP.reference(prob, RA, RB, members, 1.0, den_a, den_b, method=method, evals=evals)
        if r["w_ref"] <= W_REF_MAX:
            break
    return r


def usage_reference(name, **kw):
    prob, RA, RB, den_a, den_b, members, t = case(name)
    return UP.reference(prob, RA, RB, members, t, den_a, den_b, **kw)


def kept(kind, r):
    keys, ints = (GENE_KEPT, ("parts", "evals")) if kind == "gene" else (UP.KEPT, ("peaks", "parts", "solves"))
    return {k: (int(r[k]) if k in ints else float(r[k])) for k in keys}


def recorded():
    """tests/golden/gene_shape_refs.json -> dict(gene: {name: GENE_KEPT}, usage: {name: UP.KEPT})"""
    if "recorded" not in _cache:
        with open(GOLDEN) as f:
            _cache["recorded"] = json.load(f)
    return _cache["recorded"]


def compare_reference(name, t):
    """CP.reference of a queried transcript of a COMPARE_CASES problem, computed once per session"""
    if ("cmp", name, t) not in _cache:
        p = problem(name)
        _cache["cmp", name, t] = CP.reference(p["prob"], p["RA"], p["RB"], t, 1.0, p["den_a"], p["den_b"])
    return _cache["cmp", name, t]


def profile_gene(name):
    """PG.Gene of a PROFILE_CASES name, built once per session"""
    from tests import profile_gene_problems as PG
    if ("pg", name) not in _cache:
        prob, R, den, members = profile_case(name)
        _cache["pg", name] = PG.Gene(prob, R, members, den)
    return _cache["pg", name]


def presence_lambda(name):
    """the reference's gene presence Lambda = 2 (F_hat - F_drop) of a PROFILE_CASES name"""
    g = profile_gene(name)
    return 2.0 * (g.em()[1] - g.em(pin=0.0)[1])


if __name__ == "__main__":
    import sys
    import time
    args = sys.argv[1:]
    if "--pick-seed" in args:
        for j in range(8):
            p = two_trips_problem(300 + 10 * j)
            fits = [CP.sample_fit(p["prob"], R, p["tids"][0], p["den_a"])["passes"] for R in (p["RA"], p["RB"])]
            print("seed", 300 + 10 * j, "passes", fits, sum(fits), flush=True)
        sys.exit(0)
    write = "--write" in args
    out = args[args.index("--out") + 1] if "--out" in args else GOLDEN
    kinds = [k for k in ("gene", "usage") if "--" + k in args] or ["gene", "usage"]
    for kind in kinds:
        names = [a for a in args if a in (GENE_CASES if kind == "gene" else USAGE_CASES)] or list(GENE_CASES if kind == "gene" else USAGE_CASES)
        for name in names:
            t0 = time.time()
            r = kept(kind, gene_reference(name) if kind == "gene" else usage_reference(name))
            print(kind, name, r, "%.1f s" % (time.time() - t0), flush=True)
            if write:
                have = json.load(open(out)) if os.path.exists(out) else {}
                have.setdefault(kind, {})[name] = r
                with open(out, "w") as f:
                    json.dump(have, f, indent=1, sort_keys=True)
                    f.write("\n")
