"""Cost of the two-sample test (emsar_hip_compare) on bench.py's time_to_mle segment problem against one solve; prints one JSON object.

    python tools/compare_bench.py [--genes | --usage | --groups [--genes]] [--rounds 3] [--max-iter 20000] [--max-evals 40] [--seed 5] [--out FILE]

Sample A is the problem as it stands (same seeds, 100 k transcripts in families); sample B is a Poisson redraw of A's row weights (a
technical replicate: the null holds for every transcript).  Both are uploaded into contexts of their own and solved once (the first
solve finds and packs the sets); then every transcript is compared, --rounds times.  Reported: wall and device ms of the best call (HIP
events around the searches), transcripts per status, evaluations per search (mean, max), the wall time of one solve of A in the same
process and the ratio, the share of TESTED transcripts with p < 0.05 (about 0.05 or less under the null), and whether a solve after
the calls returns the bits it returned before.
--genes: emsar_hip_compare_genes instead, the generator's families as genes (boot_bench.family_sizes): the same figures per gene, and
the most parts a gene had.
--usage: emsar_hip_compare_usage over every transcript of a family of two or more (the families as genes): after one warm-up call the
median wall and device ms of 5 calls, next to the median of 5 calls of emsar_hip_compare on the same transcripts and one solve, all
from this run; outer points per search and inner evaluations per outer point.
--groups: emsar_hip_compare_groups over all transcripts in one call, K = 4 samples in two groups (0, 0, 1, 1): sample 0 is the problem as
it stands, samples 1 to 3 are Poisson redraws of its row weights (seeds --seed, +1, +2): after one warm-up call the median wall and the
device ms of 5 calls, the searches, outer points per search, inner evaluations per outer point and the UNCONVERGED count, next to the
median of 5 calls of emsar_hip_compare on samples 0 and 2 and one solve, all from this run.
--groups --genes: emsar_hip_compare_groups_genes over all family genes in one call on the same four samples and groups: the same
figures per gene search and the most parts a gene had, next to the medians of emsar_hip_compare_groups over all transcripts, of
emsar_hip_compare_genes on samples 0 and 2 and of one solve, all from this run.  A record, never a test threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--max-evals", type=int, default=40)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--genes", action="store_true")
    ap.add_argument("--usage", action="store_true")
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from boot_bench import family_sizes, segment_problem
    from emsar_amd import EmsarHip
    n_tx, rp, ci, R, E = segment_problem()
    RB = np.random.default_rng(a.seed).poisson(R).astype(np.int32)
    solve = dict(max_iter=a.max_iter, tol=1e-10)
    out = {"n_tx": int(n_tx), "rows": int(len(rp) - 1), "max_iter": a.max_iter, "max_evals": a.max_evals, "seed": a.seed}
    if a.groups:
        out.update(groups_record(n_tx, rp, ci, R, E, a.seed, solve, family_sizes(n_tx) if a.genes else None))
        return finish(out, a.out)
    with EmsarHip(0) as A, EmsarHip(0) as B:
        for dev, w in ((A, R), (B, RB)):
            dev.upload_structure(n_tx, rp, ci)
            dev.upload_sample(w, E, None)
        if a.genes:
            sizes = family_sizes(n_tx)
            A.set_gene_map(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes), len(sizes))
            out.update(call="compare_genes", n_genes=int(len(sizes)))
        th, _ = A.solve(**solve)                             # finds and packs the sets, warms up
        B.solve(**solve)
        if a.usage:
            out.update(usage_record(A, B, n_tx, family_sizes(n_tx), solve))
            th2, _ = A.solve(**solve)
            out["solve_unchanged"] = bool(th2.tobytes() == th.tobytes())
            return finish(out, a.out)
        solves = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            A.solve(**solve)
            solves.append(time.perf_counter() - t0)
        runs = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            r = (A.compare_genes if a.genes else A.compare)(B, max_evals=a.max_evals, **solve)
            d = r["stats"].as_dict()
            d["wall_s"] = time.perf_counter() - t0
            runs.append(d)
        best = min(runs, key=lambda d: d["wall_s"])
        tested = r["status"] == 0
        out.update(runs=runs, status=best["n_status"], items_launched=best["items_launched"], wall_ms=1e3 * best["wall_s"],
                   device_ms=best["device_ms"], evals_per_item_mean=best["evals_sum"] / max(1, best["items_launched"]),
                   evals_max=best["evals_max"], passes_max=best["passes_max"], min_raw_lambda=best["min_raw_lambda"],
                   solve_wall_ms=1e3 * min(solves), wall_over_solve=best["wall_s"] / min(solves),
                   share_p_below_0_05=float(np.mean(r["pvalue"][tested] < 0.05)) if tested.any() else None)
        if a.genes:
            out["parts_max"] = best["parts_max"]
        th2, _ = A.solve(**solve)
        out["solve_unchanged"] = bool(th2.tobytes() == th.tobytes())
    finish(out, a.out)


def timed(f, calls):
    """the median wall time of `calls` calls after a warm-up call, and that call's result"""
    f()
    runs = []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = f()
        runs.append((time.perf_counter() - t0, r))
    runs.sort(key=lambda x: x[0])
    return runs[len(runs) // 2]


def groups_record(n_tx, rp, ci, R, E, seed, solve, sizes=None, calls=5):
    """--groups: the figures of emsar_hip_compare_groups at K = 4 in two groups, of emsar_hip_compare on samples 0 and 2 and of one solve;
    sizes (the families as genes): those of emsar_hip_compare_groups_genes, next to compare_groups, compare_genes and one solve"""
    from emsar_amd import EmsarHip
    groups = (0, 0, 1, 1)
    weights = [R] + [np.random.default_rng(seed + k).poisson(R).astype(np.int32) for k in range(3)]
    with EmsarHip(0) as d0, EmsarHip(0) as d1, EmsarHip(0) as d2, EmsarHip(0) as d3:
        devs = (d0, d1, d2, d3)
        for dev, w in zip(devs, weights):
            dev.upload_structure(n_tx, rp, ci)
            dev.upload_sample(w, E, None)
        th = [dev.solve(**solve)[0] for dev in devs]          # finds and packs the sets, warms up
        if sizes is not None:
            return groups_genes_record(devs, groups, sizes, th, solve, calls)
        wall_g, r = timed(lambda: d0.compare_groups(devs[1:], groups, **solve), calls)
        wall_c, c = timed(lambda: d0.compare(d2, **solve), calls)
        wall_s, _ = timed(lambda: d0.solve(**solve), calls)
        d, dc = r["stats"].as_dict(), c["stats"].as_dict()
        tested = r["status"] == 0
        unchanged = all(dev.solve(**solve)[0].tobytes() == t.tobytes() for dev, t in zip(devs, th))
    return dict(call="compare_groups", n_samples=4, groups=list(groups), calls=calls, status=d["n_status"], unconverged=d["n_status"]["UNCONVERGED"],
                searches=d["items_launched"], wall_ms=1e3 * wall_g, device_ms=d["device_ms"],
                outer_per_search_mean=d["outer_sum"] / max(1, d["items_launched"]), outer_max=d["outer_max"],
                inner_evals_per_outer_point=d["evals_sum"] / max(1, d["outer_sum"]), evals_max=d["evals_max"], passes_sum=d["passes_sum"],
                passes_max=d["passes_max"], min_raw_lambda=d["min_raw_lambda"], compare_wall_ms=1e3 * wall_c, compare_device_ms=dc["device_ms"],
                compare_passes_sum=dc["passes_sum"], solve_wall_ms=1e3 * wall_s, wall_over_compare=wall_g / wall_c, wall_over_solve=wall_g / wall_s,
                share_p_between_below_0_05=float(np.mean(r["p_between"][tested] < 0.05)) if tested.any() else None,
                share_p_within_below_0_05=float(np.mean(r["p_within"][tested] < 0.05)) if tested.any() else None, solve_unchanged=bool(unchanged))


def groups_genes_record(devs, groups, sizes, th, solve, calls):
    """--groups --genes, on the loaded and solved contexts of groups_record"""
    d0 = devs[0]
    d0.set_gene_map(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes), len(sizes))
    wall_g, r = timed(lambda: d0.compare_groups_genes(devs[1:], groups, **solve), calls)
    wall_t, t = timed(lambda: d0.compare_groups(devs[1:], groups, **solve), calls)
    wall_c, c = timed(lambda: d0.compare_genes(devs[2], **solve), calls)
    wall_s, _ = timed(lambda: d0.solve(**solve), calls)
    d, dt, dc = r["stats"].as_dict(), t["stats"].as_dict(), c["stats"].as_dict()
    tested = r["status"] == 0
    unchanged = all(dev.solve(**solve)[0].tobytes() == x.tobytes() for dev, x in zip(devs, th))
    return dict(call="compare_groups_genes", n_samples=len(devs), groups=list(groups), n_genes=int(len(sizes)), calls=calls, status=d["n_status"],
                unconverged=d["n_status"]["UNCONVERGED"], searches=d["items_launched"], wall_ms=1e3 * wall_g, device_ms=d["device_ms"],
                outer_per_search_mean=d["outer_sum"] / max(1, d["items_launched"]), outer_max=d["outer_max"],
                inner_evals_per_outer_point=d["evals_sum"] / max(1, d["outer_sum"]), evals_max=d["evals_max"], passes_sum=d["passes_sum"],
                passes_max=d["passes_max"], parts_max=d["parts_max"], min_raw_lambda=d["min_raw_lambda"],
                compare_groups_wall_ms=1e3 * wall_t, compare_groups_device_ms=dt["device_ms"], compare_groups_searches=dt["items_launched"],
                compare_genes_wall_ms=1e3 * wall_c, compare_genes_device_ms=dc["device_ms"], compare_genes_searches=dc["items_launched"],
                solve_wall_ms=1e3 * wall_s, wall_over_compare_groups=wall_g / wall_t, wall_over_compare_genes=wall_g / wall_c,
                wall_over_solve=wall_g / wall_s,
                share_p_between_below_0_05=float(np.mean(r["p_between"][tested] < 0.05)) if tested.any() else None,
                share_p_within_below_0_05=float(np.mean(r["p_within"][tested] < 0.05)) if tested.any() else None, solve_unchanged=bool(unchanged))


def usage_record(A, B, n_tx, sizes, solve, calls=5):
    """--usage: the figures of emsar_hip_compare_usage, of emsar_hip_compare on the same transcripts and of one solve"""
    gene_of = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    A.set_gene_map(gene_of, len(sizes))
    q = np.flatnonzero(np.asarray(sizes)[gene_of] >= 2).astype(np.int32)

    wall_u, r = timed(lambda: A.compare_usage(B, q, **solve), calls)
    wall_c, c = timed(lambda: A.compare(B, q, **solve), calls)
    wall_s, _ = timed(lambda: A.solve(**solve), calls)
    d, dc = r["stats"].as_dict(), c["stats"].as_dict()
    tested = r["status"] == 0
    return dict(call="compare_usage", n_genes=int(len(sizes)), n_query=int(len(q)), calls=calls, status=d["n_status"], items_launched=d["items_launched"],
                wall_ms=1e3 * wall_u, device_ms=d["device_ms"], outer_per_item_mean=d["outer_sum"] / max(1, d["items_launched"]), outer_max=d["outer_max"],
                inner_evals_per_outer_point=d["evals_sum"] / max(1, d["outer_sum"]), evals_max=d["evals_max"], passes_sum=d["passes_sum"],
                passes_max=d["passes_max"], parts_max=d["parts_max"], min_raw_lambda=d["min_raw_lambda"],
                compare_wall_ms=1e3 * wall_c, compare_device_ms=dc["device_ms"], compare_passes_sum=dc["passes_sum"], solve_wall_ms=1e3 * wall_s,
                wall_over_compare=wall_u / wall_c, wall_over_solve=wall_u / wall_s,
                share_p_below_0_05=float(np.mean(r["pvalue"][tested] < 0.05)) if tested.any() else None)


def finish(out, path):
    txt = json.dumps(out, indent=1)
    print(txt)
    if path:
        with open(path, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
