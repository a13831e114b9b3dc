#!/usr/bin/env python3
"""Cost of the coalescent / sample-pair statistics (k_coal_stats + k_rows_fold, timing class 14) on the benchmark's
workloads: BASELINE configs[3] (100 k loci, 16 leaves; --config 4) and configs[4] (200 k loci, 20 leaves; --config 5
--loci 200000), the synthetic data sets bench.py builds (same generator, seeds and cache), one sample after every iteration.

  python tools/coal_stats_cost.py [--config 4] [--loci 100000] [--steps 50] [--warmup 200] [--blocks 3]

Runs interleaved blocks of `steps` iterations without and with sampling on one chain (off, on, off, on, ..., off) and
prints one JSON line: the median wall ms per iteration of the unsampled and of the sampled blocks (every iteration ends
with its one host synchronisation, so wall time is the device's time per iteration) and the two kernels' time per sample
from HIP events.  A sample also runs the commit of an accepted mixing proposal as a kernel of its own (otherwise it rides
in the next sweep kernel): launches of k_mix_finish are reported too.  Under
`rocprofv3 --kernel-trace --stats -- python tools/coal_stats_cost.py ...` the kernels' own statistics come from the
profiler."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gphocs_amd as G  # noqa: E402
import bench  # noqa: E402

CS_CLASS = 14     # gph_engine_class_stats / last_kernel_ms class of k_coal_stats + k_rows_fold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--config", type=int, default=4)      # bench.py's numbering: 4 = BASELINE configs[3]
    ap.add_argument("--blocks", type=int, default=3)      # sampled blocks, each between two unsampled ones
    a = ap.parse_args()
    G.build()
    pack = bench.build_workload(G, a.config, a.loci, 6.5, 20261002 + a.config, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1

    def block(sample):
        nonlocal it
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.iteration(it)
            if sample:
                s.sample_coal_stats(it)
            it += 1
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if sample:
            s.coal_stats(raw=True)     # outside the timed block: empties the device buffer for the next one
        return ms

    s.enable_coal_stats(a.steps)
    s.class_stats(CS_CLASS, reset=True)
    s.class_stats(7, reset=True)
    off, on = [block(False)], []
    for _ in range(a.blocks):
        on.append(block(True))
        off.append(block(False))
    cs = s.class_stats(CS_CLASS)      # (event times are collected at the host synchronisations of the iterations after)
    mf = s.class_stats(7)             # k_mix_finish: over all blocks
    rd = len(s.coal_stats_columns())
    s.close()
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"loci": a.loci, "config": a.config, "leaves": pack.n, "pops": pack.K, "row_doubles": rd, "steps": a.steps,
                      "ms_per_iter_off_median": round(med(off), 4), "ms_per_iter_on_median": round(med(on), 4),
                      "ms_per_iter_off_blocks": [round(x, 4) for x in off], "ms_per_iter_on_blocks": [round(x, 4) for x in on],
                      "added_ms_per_sampled_iter": round(med(on) - med(off), 4),
                      "coal_stats_samples": cs["launches"],
                      "coal_stats_kernels_ms_per_sample": round(cs["ms"] / max(cs["launches"], 1), 5),
                      "k_mix_finish_launches": mf["launches"],
                      "k_mix_finish_ms_per_launch": round(mf["ms"] / max(mf["launches"], 1), 5)}))


if __name__ == "__main__":
    main()
