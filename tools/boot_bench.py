"""Cost of the Poisson bootstrap (emsar_hip_bootstrap) on two workloads; prints one JSON object.

    python tools/boot_bench.py [--reps 100] [--cfg3-scale 0.1] [--cfg3-reps 10] [--genes | --subsample | --quantiles | --isoforms] [--out FILE]

  segment   bench.py's time_to_mle problem (same seeds): one solve, then B replicates in one call -- device time per stage (HIP events),
            wall time, ms per replicate against one solve, the batch size and the slowest set's passes
  cfg3      BASELINE config 3 at --cfg3-scale, collapsed to weighted segments on the device, B = --cfg3-reps: one giant component, so
            every replicate is a streaming solve of its own (deterministic mode, as emsar-hip runs it)
  --genes  instead: emsar_hip_bootstrap against emsar_hip_bootstrap_genes on both workloads, the generator's families as genes, and on
            the segment problem also a worst-case map with 90 % of the transcripts in one gene -- reduce_ms and total_ms of each, the
            calls alternated (two rounds) so that the solves' own spread shows
  --subsample  instead: emsar_hip_subsample (fractions 0.1, 0.25, 0.5, 0.75, 1.0, B replicates each) next to one solve and next to
            emsar_hip_bootstrap with the same B on the same context, the calls alternated (two rounds); per fraction also a call of its
            own, which gives the time per replicate at that fraction
  --quantiles  instead: emsar_hip_bootstrap_genes against emsar_hip_bootstrap_quantiles (q = 0.025, 0.5, 0.975, gene outputs included) on both
            workloads, the generator's families as genes, same context and B, the calls alternated (two rounds) -- total_ms of both,
            quantile_ms (device time of the quantile stage) and held_bytes
  --isoforms   instead: emsar_hip_bootstrap_quantiles against emsar_hip_bootstrap_isoforms (the same q and gene outputs, plus usage_mean,
            usage_sd, dominant_count and usage_q) on both workloads, the generator's families as genes, same context and B, the calls
            alternated (two rounds) -- reduce_ms, quantile_ms and total_ms of both
Kernel-level times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def family_sizes(n_tx):
    """the family sizes segment_problem() drew (same seed), which family_matrix laid out as consecutive tid blocks"""
    rng = np.random.default_rng(11)
    sizes = np.minimum(rng.zipf(1.6, size=40000), 60)
    sizes = sizes[np.cumsum(sizes) <= 100000]
    assert int(sizes.sum()) == n_tx
    return sizes


def segment_problem():
    from emsar_amd import synth
    rng = np.random.default_rng(11)                       # bench.py time_to_mle, draw for draw
    sizes = np.minimum(rng.zipf(1.6, size=40000), 60)
    sizes = sizes[np.cumsum(sizes) <= 100000]
    n_tx, rp, ci, _ = synth.family_matrix([int(x) for x in sizes], rows_per_tid=3, seed=11, dup=0.0)
    E = rng.uniform(0.5, 2.0, size=len(rp) - 1)
    theta_true = np.where(rng.random(n_tx) < 0.3, 0.0, rng.lognormal(0.0, 2.0, size=n_tx))
    R = rng.poisson(E * np.add.reduceat(theta_true[ci], rp[:-1].astype(np.int64))).astype(np.int32)
    return n_tx, rp, ci, R, E


def worst_case_map(n_tx, fam_of, seed=1):
    """90 % of the transcripts, drawn at random, in gene 0; the rest keep their family (numbered after it)"""
    big = np.random.default_rng(seed).random(n_tx) < 0.9
    g = (fam_of + 1).astype(np.int32)
    g[big] = 0
    used, g = np.unique(g, return_inverse=True)
    return g.astype(np.int32), len(used)


def run_genes(dev, B, solve_kw, maps, seed=1, rounds=2):
    """bootstrap vs bootstrap_genes with each map of `maps` ({name: (gene_of_tx, n_genes)}), alternated"""
    dev.solve(**solve_kw)
    dev.bootstrap(min(B, 2), seed, **solve_kw)
    for gm, ng in maps.values():                          # first calls: kernels loaded, draw map built
        dev.set_gene_map(gm, ng)
        dev.bootstrap_genes(min(B, 2), seed, **solve_kw)
    out = {"replicates": B, "none": []}
    for name, (gm, ng) in maps.items():
        out[name] = {"n_genes": int(ng), "largest_gene": int(np.bincount(gm).max()), "runs": []}
    for _ in range(rounds):
        st = dev.bootstrap(B, seed, **solve_kw)[4]
        out["none"].append({"reduce_ms": st.reduce_ms, "total_ms": st.total_ms, "batch": st.batch})
        for name, (gm, ng) in maps.items():
            dev.set_gene_map(gm, ng)
            st = dev.bootstrap_genes(B, seed, **solve_kw)["stats"]
            out[name]["runs"].append({"reduce_ms": st.reduce_ms, "total_ms": st.total_ms, "batch": st.batch})
    return out


QUANTILES = [0.025, 0.5, 0.975]


def run_quantiles(dev, B, solve_kw, gene_of_tx, n_genes, seed=1, rounds=2):
    """bootstrap_genes vs bootstrap_quantiles over QUANTILES, the same B, alternated"""
    dev.set_gene_map(gene_of_tx, n_genes)
    dev.solve(**solve_kw)
    dev.bootstrap_genes(min(B, 2), seed, **solve_kw)      # first calls: draw map, kernels loaded
    dev.bootstrap_quantiles(min(B, 2), QUANTILES, seed, want_genes=True, **solve_kw)
    out = {"replicates": B, "n_genes": int(n_genes), "q": QUANTILES, "bootstrap_genes": [], "bootstrap_quantiles": []}
    for _ in range(rounds):
        st = dev.bootstrap_genes(B, seed, **solve_kw)["stats"]
        out["bootstrap_genes"].append({"total_ms": st.total_ms, "reduce_ms": st.reduce_ms, "batch": st.batch})
        r = dev.bootstrap_quantiles(B, QUANTILES, seed, want_genes=True, **solve_kw)
        st, qs = r["stats"], r["qstats"]
        out["bootstrap_quantiles"].append({"total_ms": st.total_ms, "reduce_ms": st.reduce_ms, "batch": st.batch, "quantile_ms": qs.quantile_ms,
                                           "held_bytes": qs.held_bytes})
    return out


def run_isoforms(dev, B, solve_kw, gene_of_tx, n_genes, seed=1, rounds=2):
    """bootstrap_quantiles vs bootstrap_isoforms over QUANTILES, gene outputs in both, the same B, alternated"""
    dev.set_gene_map(gene_of_tx, n_genes)
    dev.solve(**solve_kw)
    dev.bootstrap_quantiles(min(B, 2), QUANTILES, seed, want_genes=True, **solve_kw)      # first calls: draw map, kernels loaded
    dev.bootstrap_isoforms(min(B, 2), seed, q=QUANTILES, want_genes=True, **solve_kw)
    out = {"replicates": B, "n_genes": int(n_genes), "q": QUANTILES, "bootstrap_quantiles": [], "bootstrap_isoforms": []}
    for _ in range(rounds):
        for name, call in (("bootstrap_quantiles", lambda: dev.bootstrap_quantiles(B, QUANTILES, seed, want_genes=True, **solve_kw)),
                           ("bootstrap_isoforms", lambda: dev.bootstrap_isoforms(B, seed, q=QUANTILES, want_genes=True, **solve_kw))):
            r = call()
            st, qs = r["stats"], r["qstats"]
            out[name].append({"total_ms": st.total_ms, "reduce_ms": st.reduce_ms, "quantile_ms": qs.quantile_ms, "batch": st.batch,
                              "held_bytes": qs.held_bytes})
    return out


SUB_FRACTIONS = [0.1, 0.25, 0.5, 0.75, 1.0]


def run_subsample(dev, B, solve_kw, seed=1, rounds=2):
    """subsample over SUB_FRACTIONS vs one solve vs bootstrap, B replicates each, alternated; then every fraction alone"""
    dev.solve(**solve_kw)
    dev.bootstrap(min(B, 2), seed, **solve_kw)            # first calls: draw map, kernels loaded
    dev.subsample([0.5], min(B, 2), seed, **solve_kw)
    out = {"replicates": B, "fractions": SUB_FRACTIONS, "solve": [], "bootstrap": [], "subsample": [], "per_fraction": []}
    for _ in range(rounds):
        t0 = time.perf_counter()
        _, st = dev.solve(**solve_kw)
        out["solve"].append({"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st.kernel_ms})
        t0 = time.perf_counter()
        bs = dev.bootstrap(B, seed, **solve_kw)[4]
        out["bootstrap"].append({"wall_ms": (time.perf_counter() - t0) * 1e3, "ms_per_replicate": bs.total_ms / B, **bs.as_dict()})
        t0 = time.perf_counter()
        r = dev.subsample(SUB_FRACTIONS, B, seed, **solve_kw)
        ss = r["stats"]
        out["subsample"].append({"wall_ms": (time.perf_counter() - t0) * 1e3, "ms_per_replicate": ss.total_ms / (B * len(SUB_FRACTIONS)),
                                 "depth_mean": [float(x) for x in r["depth_mean"]], **ss.as_dict()})
    for f in SUB_FRACTIONS:
        runs = []
        for _ in range(rounds):
            ss = dev.subsample([f], B, seed, **solve_kw)["stats"]
            runs.append({"ms_per_replicate": ss.total_ms / B, **ss.as_dict()})
        out["per_fraction"].append({"fraction": f, "runs": runs})
    return out


def run(dev, B, solve_kw, seed=1):
    dev.solve(**solve_kw)                                 # sets found and packed, warm
    t0 = time.perf_counter()
    th, st = dev.solve(**solve_kw)
    solve_s = time.perf_counter() - t0
    dev.bootstrap(min(B, 2), seed, **solve_kw)            # first call: draw map, kernels loaded
    t0 = time.perf_counter()
    mean, sd, tsd, _, bs = dev.bootstrap(B, seed, **solve_kw)
    boot_s = time.perf_counter() - t0
    return {"solve_ms": solve_s * 1e3, "solve_kernel_ms": st.kernel_ms, "solve_set_passes_max": st.set_passes_max,
            "sets_resident": st.sets_resident, "sets_streamed": st.sets_streamed, "replicates": B, "boot_wall_ms": boot_s * 1e3,
            "boot_ms_per_replicate": boot_s * 1e3 / B, "replicate_over_solve": boot_s / B / solve_s, **bs.as_dict(),
            "sd_fpkm_median_rel": float(np.median((sd / np.maximum(mean, 1e-300))[mean > 1e-3]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cfg3-scale", type=float, default=0.1)
    ap.add_argument("--cfg3-reps", type=int, default=10)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--genes", action="store_true")
    ap.add_argument("--subsample", action="store_true")
    ap.add_argument("--quantiles", action="store_true")
    ap.add_argument("--isoforms", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from emsar_amd import EmsarHip, synth
    out = {}
    with EmsarHip(0) as dev:
        n_tx, rp, ci, R, E = segment_problem()
        dev.upload_structure(n_tx, rp, ci)
        dev.upload_sample(R, E, None)
        seg_kw = dict(max_iter=200000, tol=1e-10)
        if a.subsample:
            out["segment"] = {"n_tx": int(n_tx), "segments": int(len(R)), **run_subsample(dev, a.reps, seg_kw)}
        elif a.quantiles or a.isoforms:
            sizes = family_sizes(n_tx)
            fam = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
            out["segment"] = {"n_tx": int(n_tx), "segments": int(len(R)),
                              **(run_isoforms if a.isoforms else run_quantiles)(dev, a.reps, seg_kw, fam, int(fam.max()) + 1)}
        elif a.genes:
            sizes = family_sizes(n_tx)
            fam = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
            maps = {"families": (fam, int(fam.max()) + 1), "worst_90pct": worst_case_map(n_tx, fam)}
            out["segment"] = {"n_tx": int(n_tx), "segments": int(len(R)), **run_genes(dev, a.reps, seg_kw, maps)}
        else:
            out["segment"] = {"n_tx": int(n_tx), "segments": int(len(R)), **run(dev, a.reps, seg_kw)}
        if not a.skip_cfg3:
            import bench
            cfg = dict(synth.CONFIGS["cfg3"])
            cfg["n_reads"] = max(1000, int(cfg["n_reads"] * a.cfg3_scale))
            s = bench.family_matrix_threaded(**cfg)
            crp, cci, cw, _, _ = dev.collapse_rows(s["n_tx"], s["row_ptr"], s["col_idx"], want_map=False)
            dev.set_deterministic(True)
            dev.upload_structure(s["n_tx"], crp, cci)
            dev.upload_sample(cw, None, s["den"])
            kw = dict(max_iter=200000, tol=1e-10, zero_cut=2.5e-7, abs_step=1e-13)
            info = {"scale": a.cfg3_scale, "reads": int(s["n_reads"]), "n_tx": int(s["n_tx"]), "segments": int(len(cw))}
            if a.subsample:
                out["cfg3"] = {**info, **run_subsample(dev, a.cfg3_reps, kw)}
            elif a.quantiles or a.isoforms:
                _, fam = synth.make_families(s["n_tx"], cfg["seed"])
                out["cfg3"] = {**info, **(run_isoforms if a.isoforms else run_quantiles)(dev, a.cfg3_reps, kw, fam, int(fam.max()) + 1)}
            elif a.genes:
                _, fam = synth.make_families(s["n_tx"], cfg["seed"])
                out["cfg3"] = {**info, **run_genes(dev, a.cfg3_reps, kw, {"families": (fam, int(fam.max()) + 1)})}
            else:
                out["cfg3"] = {**info, **run(dev, a.cfg3_reps, kw)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
