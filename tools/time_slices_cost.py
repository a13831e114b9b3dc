#!/usr/bin/env python3
"""Cost of the time-sliced statistics (k_time_slices + k_rows_fold, timing class 15) on the benchmark's workloads:
BASELINE configs[3] (100 k loci, 16 leaves; --config 4) and configs[4] (200 k loci, 20 leaves; --config 5 --loci 200000),
the synthetic data sets bench.py builds (same generator, seeds and cache), one sample after every iteration.

  python tools/time_slices_cost.py [--config 4] [--loci 100000] [--slices 4] [--steps 50] [--warmup 200] [--blocks 3]

Runs interleaved blocks of `steps` iterations without sampling, with time-slices sampling and with coal-stats sampling
(the yardstick, k_coal_stats + k_rows_fold, class 14) on one chain and prints one JSON line: the median wall ms per
iteration of each kind of block (every iteration ends with its one host synchronisation, so wall time is the device's time
per iteration), the kernels' time per sample from HIP events, and the bytes the kernel stages per sample -- the page
ranges of gph_timeslices.h (GphTsImg) times the loci -- with the rate that makes of the kernel time.  `floor_bytes` is the
smaller figure the issue names as the floor: chain heads plus the event records in use (counted from a state dump of the
first 256 loci, scaled to all loci)."""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gphocs_amd as G  # noqa: E402
import bench  # noqa: E402

TS_CLASS, CS_CLASS = 15, 14


def used_events(s, K, nloci):
    """event records in use per locus, from a state dump (C lines), averaged over the first loci"""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "state")
        s.dump_state(p, False)
        loci = ev = 0
        for ln in open(p):
            if ln.startswith("LOCUS"):
                loci += 1
                if loci > nloci:
                    break
            elif ln.startswith("C "):
                ev += len(ln.split()) - 2
    return ev / max(min(loci, nloci), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--config", type=int, default=4)      # bench.py's numbering: 4 = BASELINE configs[3]
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--floor-from-dump", action="store_true")     # a state dump of every locus is slow at 100 k loci
    ap.add_argument("--copy-GBps", type=float, default=4200.0)    # the page-copy rate DESIGN.md cites for the evaluate kernels
    a = ap.parse_args()
    G.build()
    pack = bench.build_workload(G, a.config, a.loci, 6.5, 20261002 + a.config, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1

    def block(kind):
        nonlocal it
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.iteration(it)
            if kind == "ts":
                s.sample_time_slices(it)
            elif kind == "cs":
                s.sample_coal_stats(it)
            it += 1
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if kind == "ts":
            s.time_slices()            # outside the timed block: empties the device buffer for the next one
        elif kind == "cs":
            s.coal_stats(raw=True)
        return ms

    s.enable_time_slices(a.slices, a.steps)
    s.enable_coal_stats(a.steps)
    for c in (TS_CLASS, CS_CLASS, 7):
        s.class_stats(c, reset=True)
    off, ts, cs = [block("off")], [], []
    for _ in range(a.blocks):
        ts.append(block("ts"))
        off.append(block("off"))
        cs.append(block("cs"))
        off.append(block("off"))
    t_ts, t_cs, mf = s.class_stats(TS_CLASS), s.class_stats(CS_CLASS), s.class_stats(7)
    rd = len(s.time_slices_columns())
    per_locus = s.time_slices_staged_bytes()
    ev = used_events(s, pack.K, 256) if a.floor_from_dump else None
    s.close()
    med = lambda v: sorted(v)[len(v) // 2]
    ms_ts = t_ts["ms"] / max(t_ts["launches"], 1)
    staged = per_locus * pack.L        # what the library says it copies per locus (gph_engine_time_slices_shape)
    out = {"loci": a.loci, "config": a.config, "leaves": pack.n, "pops": pack.K, "bands": pack.B, "slices": a.slices, "row_doubles": rd,
           "steps": a.steps, "ms_per_iter_off_median": round(med(off), 4), "ms_per_iter_time_slices_median": round(med(ts), 4),
           "ms_per_iter_coal_stats_median": round(med(cs), 4),
           "ms_per_iter_off_blocks": [round(x, 4) for x in off], "ms_per_iter_time_slices_blocks": [round(x, 4) for x in ts],
           "ms_per_iter_coal_stats_blocks": [round(x, 4) for x in cs],
           "time_slices_added_ms_per_sampled_iter": round(med(ts) - med(off), 4),
           "coal_stats_added_ms_per_sampled_iter": round(med(cs) - med(off), 4),
           "time_slices_samples": t_ts["launches"], "time_slices_kernels_ms_per_sample": round(ms_ts, 5),
           "coal_stats_kernels_ms_per_sample": round(t_cs["ms"] / max(t_cs["launches"], 1), 5),
           "staged_bytes_per_sample": staged, "staged_GBps": round(staged / (ms_ts * 1e-3) / 1e9, 2) if ms_ts > 0 else None,
           "k_mix_finish_launches": mf["launches"]}
    if ev is not None:
        floor = (ev * 16 + pack.K * 2) * pack.L
        floor_ms = floor / (a.copy_GBps * 1e9) * 1e3
        out.update(used_events_per_locus=round(ev, 2), floor_bytes=int(floor),
                   floor_GBps=round(floor / (ms_ts * 1e-3) / 1e9, 2) if ms_ts > 0 else None,
                   floor_ms_at_copy_rate=round(floor_ms, 5), fraction_of_floor=round(floor_ms / ms_ts, 5) if ms_ts > 0 else None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
