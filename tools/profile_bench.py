"""Cost of the profile-likelihood intervals (emsar_hip_profile) on bench.py's time_to_mle segment problem; prints one JSON object.

    python tools/profile_bench.py [--genes | --usage] [--rounds 3] [--level 0.95] [--max-iter 20000] [--max-evals 40] [--out FILE]

The problem (same seeds, 100 k transcripts in families) is uploaded and solved (the first solve finds and packs the sets); then every
transcript's interval is computed, --rounds times, and the presence test is run on the same input in the same process.  Reported: wall
and device ms per call (baseline_ms + drop_ms + search_ms: HIP events), transcripts per status, set solves per search item (mean, max),
the ratio of the wall time to emsar_hip_presence's, and -- for the transcripts the asymptotic standard errors call ESTIMATED with at
least 50 expected reads -- the median and the 5 % and 95 % points of (upper - lower) / (2 sqrt(q) sd_fpkm): 1 where the likelihood is
quadratic over the interval.
--genes: after that, in the same process, emsar_hip_profile_genes with the generator's families as genes (boot_bench.family_sizes), all
genes in one call: after one warm-up call, --rounds calls; wall and device ms (baseline_ms + search_ms: HIP events) as best / median /
worst over the rounds, genes per status, the searches of the genes that converged (two for TWO_SIDED, one for LOWER_ZERO; device and
host), evaluations per search, the most parts, and next to them the two yardsticks from this run: emsar_hip_profile over all transcripts (above) and one solve (wall, best
of --rounds).
--usage: instead of all that, emsar_hip_profile_usage over every transcript of a family of two or more (the families as genes) in one call:
the median of 5 calls after a warm-up call, wall and device ms (baseline_ms + search_ms: HIP events), transcripts per status, the limits
searched, outer points per search, inner evaluations per outer point, and the yardsticks from the same run, each the median of 5 after a
warm-up: emsar_hip_compare_usage on the same transcripts (against a Poisson redraw of the counts, seed 5, in a second context),
emsar_hip_profile on the same transcripts and one solve.
A record, never a test threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def genes_part(dev, a, solve, sizes, transcripts):
    """emsar_hip_profile_genes over all family genes in one call (module docstring); `transcripts` = the best transcript-profile run"""
    spread = lambda v: {"best": float(np.min(v)), "median": float(np.median(v)), "worst": float(np.max(v))}
    dev.set_gene_map(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes), len(sizes))
    one = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        dev.solve(**solve)
        one.append(1e3 * (time.perf_counter() - t0))
    dev.profile_genes(level=a.level, max_evals=a.max_evals, **solve)          # warm-up: the kernels' first launch
    runs = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        r = dev.profile_genes(level=a.level, max_evals=a.max_evals, **solve)
        d = r["stats"].as_dict()
        d["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        runs.append(d)
    d = runs[0]
    ok = np.isin(r["status"], (0, 1)) & (r["evals"] > 0)       # searched and converged, on the device or on the host
    n_search = int(np.sum(np.where(r["status"][ok] == 0, 2, 1)))
    return {"n_genes": int(len(sizes)), "status": d["n_status"], "wall_ms": spread([x["wall_ms"] for x in runs]),
            "device_ms": spread([x["baseline_ms"] + x["search_ms"] for x in runs]), "baseline_ms": spread([x["baseline_ms"] for x in runs]),
            "search_ms": spread([x["search_ms"] for x in runs]), "items_launched": d["items_launched"], "searches": n_search,
            "evals_per_search": float(r["evals"][ok].sum()) / max(1, n_search), "device_evals_sum": d["evals_sum"], "evals_max": d["evals_max"],
            "passes_max": d["passes_max"], "parts_max": d["parts_max"], "members_max": int(r["members"].max()),
            "min_raw_lambda": d["min_raw_lambda"], "one_solve_wall_ms": spread(one), "transcript_profile_wall_ms": 1e3 * transcripts["wall_s"],
            "transcript_profile_device_ms": transcripts["baseline_ms"] + transcripts["drop_ms"] + transcripts["search_ms"]}


def usage_part(a, solve, calls=5):
    """--usage (module docstring)"""
    from boot_bench import family_sizes, segment_problem
    from emsar_amd import EmsarHip
    n_tx, rp, ci, R, E = segment_problem()
    sizes = family_sizes(n_tx)
    gene_of = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    q = np.flatnonzero(np.asarray(sizes)[gene_of] >= 2).astype(np.int32)

    def timed(f):
        f()                                                    # warm-up
        runs = []
        for _ in range(calls):
            t0 = time.perf_counter()
            r = f()
            runs.append((time.perf_counter() - t0, r))
        runs.sort(key=lambda x: x[0])
        return runs[len(runs) // 2]
    with EmsarHip(0) as dev, EmsarHip(0) as other:
        for d, w in ((dev, R), (other, np.random.default_rng(5).poisson(R).astype(np.int32))):
            d.upload_structure(n_tx, rp, ci)
            d.upload_sample(w, E, None)
            d.solve(**solve)                                   # finds and packs the sets, warms up
        dev.set_gene_map(gene_of, len(sizes))
        th, _ = dev.solve(**solve)
        wall_u, r = timed(lambda: dev.profile_usage(q, level=a.level, max_evals=a.max_evals, **solve))
        wall_c, c = timed(lambda: dev.compare_usage(other, q, **solve))
        wall_p, p = timed(lambda: dev.profile(q, level=a.level, max_evals=a.max_evals, **solve))
        wall_s, _ = timed(lambda: dev.solve(**solve))
        unchanged = bool(dev.solve(**solve)[0].tobytes() == th.tobytes())
    d, dc, dp = r["stats"].as_dict(), c["stats"].as_dict(), p["stats"].as_dict()
    # the limits found by search, on the device or on the host: two for TWO_SIDED, one for LOWER_ZERO and UPPER_ONE; an UNCONVERGED
    # transcript is counted with two, which is one too many where one of its limits lay at an end
    limits = int(np.sum(np.isin(r["status"], (0, 4)) * 2 + np.isin(r["status"], (1, 6))))
    return dict(call="profile_usage", n_genes=int(len(sizes)), n_query=int(len(q)), calls=calls, status=d["n_status"], items_launched=d["items_launched"],
                wall_ms=1e3 * wall_u, device_ms=d["baseline_ms"] + d["search_ms"], baseline_ms=d["baseline_ms"], search_ms=d["search_ms"],
                limits_searched=limits, unconverged=d["n_status"]["UNCONVERGED"], outer_per_search=float(r["outer_evals"].sum()) / max(1, limits),
                outer_sum=d["outer_sum"], outer_max=d["outer_max"], inner_evals_per_outer_point=d["evals_sum"] / max(1, d["outer_sum"]),
                evals_sum=d["evals_sum"], evals_max=d["evals_max"], passes_sum=d["passes_sum"], passes_max=d["passes_max"], parts_max=d["parts_max"],
                min_raw_lambda=d["min_raw_lambda"], compare_usage_wall_ms=1e3 * wall_c, compare_usage_device_ms=dc["device_ms"],
                profile_wall_ms=1e3 * wall_p, profile_device_ms=dp["baseline_ms"] + dp["drop_ms"] + dp["search_ms"], solve_wall_ms=1e3 * wall_s,
                wall_over_compare_usage=wall_u / wall_c, wall_over_profile=wall_u / wall_p, solve_unchanged=unchanged)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--max-evals", type=int, default=40)
    ap.add_argument("--genes", action="store_true")
    ap.add_argument("--usage", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.usage:
        out = usage_part(a, dict(max_iter=a.max_iter, tol=1e-10))
        out.update(level=a.level, max_iter=a.max_iter, max_evals=a.max_evals)
        txt = json.dumps(out, indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    from boot_bench import family_sizes, segment_problem
    from emsar_amd import EmsarHip
    n_tx, rp, ci, R, E = segment_problem()
    solve = dict(max_iter=a.max_iter, tol=1e-10)
    out = {"n_tx": int(n_tx), "rows": int(len(rp) - 1), "level": a.level, "max_iter": a.max_iter, "max_evals": a.max_evals}
    with EmsarHip(0) as dev:
        dev.upload_structure(n_tx, rp, ci)
        dev.upload_sample(R, E, None)
        th, st = dev.solve(**solve)                        # finds and packs the sets, warms up
        pres = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            dev.presence(**solve)
            pres.append(time.perf_counter() - t0)
        runs = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            r = dev.profile(level=a.level, max_evals=a.max_evals, **solve)
            d = r["stats"].as_dict()
            d["wall_s"] = time.perf_counter() - t0
            runs.append(d)
        best = min(runs, key=lambda d: d["wall_s"])
        searches = int(np.sum(r["status"] == 0) * 2 + np.sum(np.isin(r["status"], (1, 4))))          # a lower bound: UNCONVERGED counts one
        asym = dev.asymptotic(th)
        den = np.zeros(n_tx)
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))
        np.add.at(den, ci, E[rows])
        pick = (asym["status"] == 0) & (th * den >= 50.0) & (r["status"] == 0) & (asym["sd_fpkm"] > 0)
        ratio = (r["upper"] - r["lower"])[pick] / (2.0 * np.sqrt(best["cut"]) * asym["sd_fpkm"][pick])
        out.update(runs=runs, status=best["n_status"], items_launched=best["items_launched"], wall_ms=1e3 * best["wall_s"],
                   device_ms=best["baseline_ms"] + best["drop_ms"] + best["search_ms"], search_ms=best["search_ms"],
                   evals_per_item_mean=best["evals_sum"] / max(1, searches), evals_max=best["evals_max"], passes_max=best["passes_max"],
                   presence_wall_ms=1e3 * min(pres), wall_over_presence=best["wall_s"] / min(pres),
                   width_over_wald={"n": int(pick.sum()), "median": float(np.median(ratio)) if pick.any() else None,
                                    "p05": float(np.quantile(ratio, 0.05)) if pick.any() else None,
                                    "p95": float(np.quantile(ratio, 0.95)) if pick.any() else None})
        if a.genes:
            out["genes"] = genes_part(dev, a, solve, family_sizes(n_tx), best)
        th2, _ = dev.solve(**solve)
        out["solve_unchanged"] = bool(th2.tobytes() == th.tobytes())
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
