#!/usr/bin/env python3
"""Cost of the clade-table sample (k_clades, timing class 19) on the benchmark's workloads, what the tables hold afterwards,
and the unsampled iteration against the parent commit.

  python tools/clades_cost.py [--parent DIR [--bench-only]]     the whole job, one child process per step
  python tools/clades_cost.py --config 4 [--loci 100000] [--steps 30] [--warmup 200] [--blocks 3] [--slots 0]

Without --config the tool is a driver: BASELINE configs[3] (100 k loci, 16 leaves; --config 4) and configs[4] (200 k loci, 20
leaves; --config 5 --loci 200000) with all loci, then -- with --parent DIR, a built checkout of the parent commit -- bench.py
of this commit and of the parent alternately, three times each.  Every step runs in a child process of its own under
`timeout -k 10`, one after the other, and the first one that fails ends the job (nothing more is started on the device after
a failure).

A measurement runs, on ONE chain, interleaved blocks of `steps` iterations: unsampled, with a clades sample after every
iteration, unsampled, with an ancestry sample, unsampled, with a gene-trees sample of 100 loci, ... and prints one JSON line:
the median wall ms per iteration of each kind of block (every iteration ends with its one host synchronisation, so wall time
is the device's time per iteration), each kernel's time per sample from HIP events, and the statistics of the tables after
all clades blocks (they accumulate over the blocks): distinct clades a locus (nkeys) as median, 99th percentile and maximum,
the same for dropped, and the fraction of loci with dropped > 0."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CL_CLASS, AN_CLASS, GT_CLASS = 19, 16, 17
JOBS = [(4, 100000), (5, 200000)]      # bench.py's numbering


def drive(a):
    me = os.path.abspath(__file__)
    for config, loci in ([] if a.bench_only else JOBS):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--config", str(config), "--loci", str(loci),
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--blocks", str(a.blocks), "--slots", str(a.slots)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"clades_cost: config {config} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    if not a.parent:
        return 0
    # the unsampled iteration: bench.py of this commit and of the parent, alternately
    runs = {"this": [], "parent": []}
    for k in range(3):
        for who, root in (("parent", os.path.abspath(a.parent)), ("this", REPO)):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps),
                   "--warmup", str(a.bench_warmup)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                print(f"clades_cost: bench.py of {who} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                return r.returncode
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            runs[who].append(json.loads(line))
            print(json.dumps({"bench": who, "run": k, "result": runs[who][-1]}), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"bench_ab": True}
    for who, rs in runs.items():
        for key in sorted(k for k, v in rs[0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)):
            vals = [r[key] for r in rs if key in r]
            if len(vals) == len(rs) and len(set(vals)) > 1:
                out[f"{who}.{key}"] = {"median": med(vals), "min": min(vals), "max": max(vals)}
    print(json.dumps(out), flush=True)
    return 0


def measure(a):
    import numpy as np
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, a.config, a.loci, 6.5, 20261002 + a.config, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack, lib=G.load_library(a.lib) if a.lib else None)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    gt_sel = list(range(0, a.loci, a.loci // 100))[:100]
    s.enable_clades(a.slots, max_bytes=4 << 30)      # (configs[4] with all loci and the default slots: 1.23 GB, above the default limit)
    Q, P, W, limit, _ = s._clades_shape()

    def block(kind):
        nonlocal it
        if kind == "ancestry":
            s.enable_ancestry(a.steps)
        if kind == "gene_trees":
            s.enable_gene_trees(a.steps, gt_sel)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.iteration(it)
            if kind == "clades":
                s.sample_clades()
            elif kind == "ancestry":
                s.sample_ancestry(it)
            elif kind == "gene_trees":
                s.sample_gene_trees(it)
            it += 1
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if kind == "ancestry":
            s.enable_ancestry(0)              # outside the timed block
        if kind == "gene_trees":
            s.enable_gene_trees(0)
        return ms

    hs0 = s.host_stats()
    for c in (CL_CLASS, AN_CLASS, GT_CLASS, 7):
        s.class_stats(c, reset=True)
    ms = {"off": [block("off")], "clades": [], "ancestry": [], "gene_trees": []}
    for _ in range(a.blocks):
        for kind in ("clades", "ancestry", "gene_trees"):
            ms[kind].append(block(kind))
            ms["off"].append(block("off"))
    hs1 = s.host_stats()
    iters = a.steps * (6 * a.blocks + 1)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"config": a.config, "loci": a.loci, "leaves": pack.n, "slots": P, "limit": limit, "words": W, "steps": a.steps, "blocks": a.blocks,
           "table_bytes_per_locus": P * (W + 2) * 8 + 8, "table_bytes": Q * (P * (W + 2) * 8 + 8),
           "ms_per_iter_off_median": round(med(ms["off"]), 4), "ms_per_iter_off_blocks": [round(x, 4) for x in ms["off"]],
           "syncs_per_iter": (hs1["syncs"] - hs0["syncs"]) / iters, "k_mix_finish_launches": s.class_stats(7)["launches"]}
    for kind, cls in (("clades", CL_CLASS), ("ancestry", AN_CLASS), ("gene_trees", GT_CLASS)):
        t = s.class_stats(cls)
        out[f"ms_per_iter_{kind}_blocks"] = [round(x, 4) for x in ms[kind]]
        out[f"{kind}_added_ms_per_sampled_iter"] = round(med(ms[kind]) - med(ms["off"]), 4)
        out[f"{kind}_samples"] = t["launches"]
        out[f"{kind}_kernel_ms_per_sample"] = round(t["ms"] / max(t["launches"], 1), 5)
    out["gene_trees_selected"] = len(gt_sel)
    c = s.clades()
    nk, dr = np.sort(c["nkeys"].astype(np.int64)), np.sort(c["dropped"].astype(np.int64))
    pct = lambda v, p: int(v[min(len(v) - 1, int(p * len(v)))])
    out.update(table_samples=c["samples"], clades_per_sample=pack.n - 1,
               distinct_median=pct(nk, 0.5), distinct_p99=pct(nk, 0.99), distinct_max=int(nk[-1]),
               dropped_median=pct(dr, 0.5), dropped_p99=pct(dr, 0.99), dropped_max=int(dr[-1]),
               fraction_of_loci_with_dropped=round(float(np.count_nonzero(dr)) / max(len(dr), 1), 5),
               fraction_of_loci_full=round(float(np.count_nonzero(nk >= limit)) / max(len(nk), 1), 5))
    s.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=0)      # 0: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--slots", type=int, default=0)       # 0: the default, the smallest power of two >= 8 (leaves - 1)
    ap.add_argument("--step-timeout", type=int, default=420)      # seconds a step may take (driver)
    ap.add_argument("--parent", default=None)             # a built checkout of the parent commit (driver: the bench.py comparison)
    ap.add_argument("--bench-only", action="store_true")  # driver: the bench.py comparison alone
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single configuration only)
    a = ap.parse_args()
    sys.exit(drive(a) if a.config == 0 else measure(a))


if __name__ == "__main__":
    main()
