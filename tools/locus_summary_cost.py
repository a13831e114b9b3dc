#!/usr/bin/env python3
"""Cost of the per-locus posterior summaries (k_locus_summary) on the benchmark's workload: BASELINE configs[3], the
synthetic data set bench.py builds (same generator, seeds and cache), one sample after every iteration.

  python tools/locus_summary_cost.py [--loci 100000] [--steps 50] [--warmup 200]

Runs blocks of `steps` iterations without sampling, with sampling, and without again on one chain and prints one JSON
line: wall ms per iteration of each block (every iteration ends with its one host synchronisation, so wall time is the
device's time per iteration) and k_locus_summary's time per launch from HIP events.  A sample also runs the commit of an accepted mixing proposal as a
kernel of its own (otherwise it rides in the next sweep kernel): launches of k_mix_finish are reported too.  Under
`rocprofv3 --kernel-trace --stats -- python tools/locus_summary_cost.py ...` the kernel's own statistics come from the
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

LS_CLASS = 13     # gph_engine_class_stats / last_kernel_ms class of k_locus_summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--config", type=int, default=4)      # bench.py's numbering: 4 = BASELINE configs[3]
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
                s.sample_locus_summary()
            it += 1
        # (the last sample is still queued here: 1 / steps of one k_locus_summary outside the block; a fetch would put a
        # device-to-host copy of every accumulator inside it)
        return (time.perf_counter() - t0) * 1e3 / a.steps

    off0 = block(False)
    s.enable_locus_summary()
    s.class_stats(LS_CLASS, reset=True)
    s.class_stats(7, reset=True)
    on = block(True)
    off1 = block(False)
    cs = s.class_stats(LS_CLASS)      # (event times are collected at the host synchronisations of the iterations after)
    mf = s.class_stats(7)             # k_mix_finish: over the three blocks
    ncol = len([k for k in s.locus_summary(raw=True) if k != "samples"])
    s.close()
    off = 0.5 * (off0 + off1)
    print(json.dumps({"loci": a.loci, "config": a.config, "columns": ncol, "steps": a.steps,
                      "ms_per_iter_off": round(off, 4), "ms_per_iter_on": round(on, 4),
                      "ms_per_iter_off_blocks": [round(off0, 4), round(off1, 4)],
                      "added_ms_per_sampled_iter": round(on - off, 4),
                      "k_locus_summary_launches": cs["launches"],
                      "k_locus_summary_ms_per_launch": round(cs["ms"] / max(cs["launches"], 1), 5),
                      "k_mix_finish_launches": mf["launches"],
                      "k_mix_finish_ms_per_launch": round(mf["ms"] / max(mf["launches"], 1), 5),
                      "accumulator_bytes_per_sample": 2 * 8 * ncol * a.loci}))


if __name__ == "__main__":
    main()
