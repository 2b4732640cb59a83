"""Cost of the model fit (emsar_hip_model_fit) on two workloads; prints one JSON object.

    python tools/fit_bench.py [--rounds 5] [--cfg3-scale 0.1] [--skip-cfg3] [--out FILE]

  segment   bench.py's time_to_mle problem (same seeds, 100 k transcripts), solved, then fitted at its MLE with the families as genes
  cfg3      BASELINE config 3 at --cfg3-scale, collapsed to weighted segments on the device, fitted at its MLE
Per workload: the first call (index build and upload included, total_ms), then --rounds calls: device time per stage (HIP events) --
rows, transcripts (k_fit_tx + k_fit_tx_finish), gene sums, totals -- next to the stage's algorithmic bytes
    rows         CSR (8 B per row + 4 B per entry) + theta gathers (8 B per entry) + R and E (12 B per row) + records (32 B per row)
    transcripts  4 B index slot + one 32 B record gather + 8 B theta per entry (index padding included), 36 B per transcript written
    totals       32 B per row, one workgroup
and, as a yardstick, one plain EM pass of the same context (run_passes) in the layout the solve used and in the CSR layout.
Kernel-level times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def em_pass_ms(dev, n=20):
    dev.reset_theta()
    dev.run_passes(3)
    return dev.run_passes(n) / n


def run(dev, n_tx, rp, ci, R, E, den, solve_kw, genes, rounds):
    from emsar_amd import hip
    n_rows, nnz = len(rp) - 1, len(ci)
    out = {"n_tx": int(n_tx), "rows": int(n_rows), "nnz": int(nnz)}
    dev.upload_structure(n_tx, rp, ci, layout=hip.LAYOUT_CSR)
    dev.upload_sample(R, E, den)
    out["em_pass_csr_ms"] = em_pass_ms(dev)
    dev.upload_structure(n_tx, rp, ci)
    dev.upload_sample(R, E, den)
    out["em_pass_ms"] = em_pass_ms(dev)
    out["layout"] = dev.info()["layout"]
    if genes is not None:
        dev.set_gene_map(genes, int(genes.max()) + 1)
    th, st = dev.solve(**solve_kw)
    out.update(solve_ms=st.solve_ms, converged=int(st.converged))
    first = dev.model_fit(th, E, genes=genes is not None)["stats"]
    out["first_call"] = first.as_dict()
    slots = first.index_slots
    out["bytes"] = {"rows": 8 * (n_rows + 1) + 4 * nnz + 8 * nnz + 12 * n_rows + 32 * n_rows,
                    "transcripts": 4 * slots + 40 * nnz + 36 * n_tx, "totals": 32 * n_rows, "index_bytes": first.index_bytes}
    runs = [dev.model_fit(th, E, genes=genes is not None)["stats"].as_dict() for _ in range(rounds)]
    out["runs"] = runs
    best = {k: min(r[k] for r in runs) for k in ("kernel_ms", "rows_ms", "tx_ms", "genes_ms", "totals_ms", "total_ms")}
    out["best"] = best
    out["gb_per_s"] = {"rows": out["bytes"]["rows"] / best["rows_ms"] / 1e6, "transcripts": out["bytes"]["transcripts"] / best["tx_ms"] / 1e6,
                       "totals": out["bytes"]["totals"] / best["totals_ms"] / 1e6}
    out["kernel_over_em_pass"] = best["kernel_ms"] / out["em_pass_ms"]
    out["kernel_over_em_pass_csr"] = best["kernel_ms"] / out["em_pass_csr_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfg3-scale", type=float, default=0.1)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from boot_bench import family_sizes, segment_problem
    from emsar_amd import EmsarHip, synth
    out = {}
    with EmsarHip(0) as dev:
        n_tx, rp, ci, R, E = segment_problem()
        sizes = family_sizes(n_tx)
        fam = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
        out["segment"] = run(dev, n_tx, rp, ci, R, E, None, dict(max_iter=200000, tol=1e-10), fam, a.rounds)
        if not a.skip_cfg3:
            import bench
            cfg = dict(synth.CONFIGS["cfg3"])
            cfg["n_reads"] = max(1000, int(cfg["n_reads"] * a.cfg3_scale))
            s = bench.family_matrix_threaded(**cfg)
            crp, cci, cw, _, _ = dev.collapse_rows(s["n_tx"], s["row_ptr"], s["col_idx"], want_map=False)
            dev.set_deterministic(True)
            _, fam = synth.make_families(s["n_tx"], cfg["seed"])
            kw = dict(max_iter=200000, tol=1e-10, zero_cut=2.5e-7, abs_step=1e-13)
            out["cfg3"] = {"scale": a.cfg3_scale, "reads": int(s["n_reads"]),
                           **run(dev, s["n_tx"], crp, cci, cw, None, s["den"], kw, np.asarray(fam, dtype=np.int32), a.rounds)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
