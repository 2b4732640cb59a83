"""Cost and calibration of the asymptotic standard errors (emsar_hip_asymptotic) on bench.py's time_to_mle segment problem; prints one
JSON object.

    python tools/asym_bench.py [--rounds 3] [--boot 400] [--out FILE]

The problem (same seeds, 100 k transcripts in families) is uploaded and solved; then the standard errors of the solve's theta are
computed --rounds times.  Reported: the wall and stage times of one call (plan_ms on the host; rows_ms, sets_ms, genes_ms: HIP events)
next to one solve and next to bootstrap at B = 100; the components per kernel class, the largest component and the TOO_LARGE share
of the transcripts; and, over the ESTIMATED transcripts with theta * den >= 50 reads, the median and the 5 - 95 % range of
asymptotic sd / bootstrap sd (B = --boot).  These are records, not thresholds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SOLVE = dict(max_iter=200000, tol=1e-10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--boot", type=int, default=400)
    ap.add_argument("--out")
    a = ap.parse_args()
    from boot_bench import segment_problem
    from emsar_amd import EmsarHip
    n_tx, rp, ci, R, E = segment_problem()
    out = {"n_tx": int(n_tx), "rows": int(len(rp) - 1)}
    with EmsarHip(0) as dev:
        dev.upload_structure(n_tx, rp, ci)
        dev.upload_sample(R, E, None)
        dev.solve(**SOLVE)                                 # finds and packs the sets, warms up
        solves = []
        for _ in range(3):
            t0 = time.perf_counter()
            th, st = dev.solve(**SOLVE)
            solves.append(time.perf_counter() - t0)
        out.update(solve_s_best=min(solves), converged=int(st.converged))
        runs = []
        for _ in range(a.rounds + 1):                      # the first call uploads the caller-order CSR
            t0 = time.perf_counter()
            r = dev.asymptotic(th)
            d = r["stats"].as_dict()
            d["wall_s"] = time.perf_counter() - t0
            runs.append(d)
        best = min(runs[1:], key=lambda d: d["wall_s"])
        status = r["status"]
        out.update(first_call_s=runs[0]["wall_s"], wall_s=best["wall_s"], plan_ms=best["plan_ms"], rows_ms=best["rows_ms"], sets_ms=best["sets_ms"],
                   genes_ms=best["genes_ms"], status=best["n_status"], components=best["components"], components_class=best["components_class"],
                   max_n=best["max_n"], too_large_share=float((status == 3).mean()), min_pivot_ratio=best["min_pivot_ratio"],
                   theta_unestimated_share=best["theta_unestimated_share"], wall_over_solve=best["wall_s"] / min(solves))
        t0 = time.perf_counter()
        dev.bootstrap(100, 1, **SOLVE)
        out["bootstrap100_s"] = time.perf_counter() - t0
        out["bootstrap100_over_asymptotic"] = out["bootstrap100_s"] / best["wall_s"]
        if a.boot > 0:
            _, bsd, _, _, _ = dev.bootstrap(a.boot, 2, **SOLVE)
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(np.asarray(rp).astype(np.int64)))
            den = np.bincount(ci, weights=np.asarray(E, dtype=np.float64)[rows], minlength=n_tx)
            pick = (status == 0) & (th * den >= 50.0) & (bsd > 0)
            ratio = r["sd_fpkm"][pick] / bsd[pick]
            q = np.quantile(ratio, [0.05, 0.5, 0.95]) if pick.any() else [float("nan")] * 3
            out.update(boot_n=a.boot, compared=int(pick.sum()), sd_ratio_q05=float(q[0]), sd_ratio_median=float(q[1]), sd_ratio_q95=float(q[2]))
        th2, _ = dev.solve(**SOLVE)
        out["solve_unchanged"] = bool(th2.tobytes() == th.tobytes())
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
