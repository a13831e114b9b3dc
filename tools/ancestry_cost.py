#!/usr/bin/env python3
"""Cost of the migration-ancestry sample (k_ancestry, timing class 16) on the benchmark's workloads: BASELINE configs[3]
(100 k loci, 16 leaves; --config 4) and configs[4] (200 k loci, 20 leaves; --config 5 --loci 200000), the synthetic data
sets bench.py builds (same generator, seeds and cache), one sample after every iteration.

  python tools/ancestry_cost.py                       both configurations, one child process each
  python tools/ancestry_cost.py --config 4 [--loci 100000] [--steps 50] [--warmup 200] [--blocks 3]

Without --config the tool is a driver: every configuration runs in a child process of its own under `timeout -k 10`, one
after the other, and the first one that fails ends the job (nothing more is started on the device after a failure).

A measurement runs interleaved blocks of `steps` iterations without and with sampling on ONE chain and prints one JSON
line: the median wall ms per iteration of each kind of block (every iteration ends with its one host synchronisation, so
wall time is the device's time per iteration), the kernel's time per sample from HIP events, and how many (locus, leaf)
cells a sample found on a migration's path."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

AN_CLASS = 16
JOBS = [(4, 100000), (5, 200000)]         # bench.py's numbering: BASELINE configs[3] and configs[4]


def drive(a):
    for config, loci in JOBS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--config", str(config), "--loci", str(loci),
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--blocks", str(a.blocks)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"ancestry_cost: config {config} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


def measure(a):
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, a.config, a.loci, 6.5, 20261002 + a.config, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    cells = []

    def block(on):
        nonlocal it
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.iteration(it)
            if on:
                s.sample_ancestry(it)
            it += 1
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if on:
            _, rows = s.ancestry_rows()       # outside the timed block: empties the device buffer for the next one
            cells.extend(rows[:, :pack.n].sum(axis=1).tolist())
        return ms

    s.enable_ancestry(a.steps)
    for c in (AN_CLASS, 7):
        s.class_stats(c, reset=True)
    off, on = [block(False)], []
    for _ in range(a.blocks):
        on.append(block(True))
        off.append(block(False))
    t_an, mf = s.class_stats(AN_CLASS), s.class_stats(7)
    s.close()
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"loci": a.loci, "config": a.config, "leaves": pack.n, "pops": pack.K, "bands": pack.B, "steps": a.steps,
           "accumulator_bytes": pack.L * pack.n * (2 * pack.B + 1) * 8, "row_ints": pack.n * (pack.B + 1),
           "ms_per_iter_off_median": round(med(off), 4), "ms_per_iter_ancestry_median": round(med(on), 4),
           "ms_per_iter_off_blocks": [round(x, 4) for x in off], "ms_per_iter_ancestry_blocks": [round(x, 4) for x in on],
           "ancestry_added_ms_per_sampled_iter": round(med(on) - med(off), 4),
           "ancestry_samples": t_an["launches"], "ancestry_kernel_ms_per_sample": round(t_an["ms"] / max(t_an["launches"], 1), 5),
           "cells_on_a_migration_path_per_sample": round(sum(cells) / max(len(cells), 1), 1),
           "k_mix_finish_launches": mf["launches"]}
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=0)      # 0: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=420)      # seconds a configuration may take (driver)
    a = ap.parse_args()
    sys.exit(drive(a) if a.config == 0 else measure(a))


if __name__ == "__main__":
    main()
