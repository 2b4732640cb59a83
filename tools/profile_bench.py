"""Cost of the profile-likelihood intervals (emsar_hip_profile) on bench.py's time_to_mle segment problem; prints one JSON object.

    python tools/profile_bench.py [--rounds 3] [--level 0.95] [--max-iter 20000] [--max-evals 40] [--out FILE]

The problem (same seeds, 100 k transcripts in families) is uploaded and solved (the first solve finds and packs the sets); then every
transcript's interval is computed, --rounds times, and the presence test is run on the same input in the same process.  Reported: wall
and device ms per call (baseline_ms + drop_ms + search_ms: HIP events), transcripts per status, set solves per search item (mean, max),
the ratio of the wall time to emsar_hip_presence's, and -- for the transcripts the asymptotic standard errors call ESTIMATED with at
least 50 expected reads -- the median and the 5 % and 95 % points of (upper - lower) / (2 sqrt(q) sd_fpkm): 1 where the likelihood is
quadratic over the interval."""
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
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--max-evals", type=int, default=40)
    ap.add_argument("--out")
    a = ap.parse_args()
    from boot_bench import segment_problem
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
        th2, _ = dev.solve(**solve)
        out["solve_unchanged"] = bool(th2.tobytes() == th.tobytes())
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
