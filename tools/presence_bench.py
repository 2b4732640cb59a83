"""Cost of the presence test (emsar_hip_presence) on bench.py's time_to_mle segment problem; prints one JSON object.

    python tools/presence_bench.py [--rounds 3] [--solve-only] [--out FILE]

The problem (same seeds, 100 k transcripts in families) is uploaded and solved twice (the first solve finds and packs the sets); then
every transcript is tested, --rounds times.  Reported: transcripts per status, set solves launched (baselines + drops), the passes of
the drop solves, the device time of the two phases (baseline_ms, drop_ms: HIP events), the wall time of a call, and the ratio of that
wall time to one solve's.  --solve-only times the solve alone (three timed solves after the packing one): the figure compared across
builds when the set solver's code is touched."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SOLVE = dict(max_iter=200000, tol=1e-10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solve-only", action="store_true")
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
        out.update(solve_s=solves, solve_s_best=min(solves), solve_kernel_ms=st.kernel_ms, sets_resident=st.sets_resident,
                   sets_streamed=st.sets_streamed, converged=int(st.converged))
        if not a.solve_only:
            runs = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                r = dev.presence(**SOLVE)
                d = r["stats"].as_dict()
                d["wall_s"] = time.perf_counter() - t0
                runs.append(d)
            best = min(runs, key=lambda d: d["wall_s"])
            out.update(runs=runs, status=best["n_status"], items_launched=best["items_launched"], drop_passes_max=best["drop_passes_max"],
                       drop_passes_sum=best["drop_passes_sum"], min_raw_lambda=min(d["min_raw_lambda"] for d in runs),
                       baseline_ms=best["baseline_ms"], drop_ms=best["drop_ms"], wall_s=best["wall_s"],
                       wall_over_solve=best["wall_s"] / min(solves))
            th2, _ = dev.solve(**SOLVE)
            out["solve_unchanged"] = bool(th2.tobytes() == th.tobytes())
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
