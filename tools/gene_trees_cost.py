#!/usr/bin/env python3
"""Cost of the sampled-genealogies sample (k_gene_trees, timing class 17) on the benchmark's workloads: BASELINE configs[3]
(100 k loci, 16 leaves; --config 4) with selections of 100 loci, 10 000 loci and all of them, and configs[4] (200 k loci,
20 leaves; --config 5 --loci 200000) with all loci -- the synthetic data sets bench.py builds (same generator, seeds and
cache), one sample after every iteration.

  python tools/gene_trees_cost.py                       the four configurations, one child process each
  python tools/gene_trees_cost.py --config 4 [--loci 100000] [--select 10000] [--steps 30] [--warmup 200] [--blocks 3]

Without --config the tool is a driver: every configuration runs in a child process of its own under `timeout -k 10`, one
after the other, and the first one that fails ends the job (nothing more is started on the device after a failure).

A measurement runs interleaved blocks of `steps` iterations without and with sampling on ONE chain and prints one JSON
line: the median wall ms per iteration of each kind of block (every iteration ends with its one host synchronisation, so
wall time is the device's time per iteration), the kernel's time per sample from HIP events, and the bytes of a sample.
The row buffer of a timed block holds the block's `steps` samples (max_bytes raised to what that takes) and is dropped, not
fetched, after the block.  With all loci selected the tool then times one flush as the program does it: a buffer of the
default size (min(64, 256 MB / row) rows) filled, fetched and appended to a file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GT_CLASS = 17
JOBS = [(4, 100000, 100), (4, 100000, 10000), (4, 100000, 0), (5, 200000, 0)]      # bench.py's numbering; select 0: all loci


def drive(a):
    for config, loci, select in JOBS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--config", str(config), "--loci", str(loci),
               "--select", str(select), "--steps", str(a.steps), "--warmup", str(a.warmup), "--blocks", str(a.blocks)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"gene_trees_cost: config {config}, {select or 'all'} loci ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


def measure(a):
    import numpy as np
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, a.config, a.loci, 6.5, 20261002 + a.config, os.path.join(REPO, "bench_cache"))
    sel = None if a.select == 0 else list(range(0, a.loci, a.loci // a.select))[:a.select]      # evenly spread over the data set
    s = G.Sampler(pack, lib=G.load_library(a.lib) if a.lib else None)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    s.enable_gene_trees(1, sel)
    nsel, N, rb, _, _ = s._gene_trees_shape()
    row_bytes = nsel * rb
    s.enable_gene_trees(0)

    def block(on):
        nonlocal it
        if on:
            s.enable_gene_trees(a.steps, sel, max_bytes=a.steps * row_bytes)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.iteration(it)
            if on:
                s.sample_gene_trees(it)
            it += 1
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if on:
            s.enable_gene_trees(0)            # outside the timed block: the rows are dropped, not fetched
        return ms

    hs0 = s.host_stats()
    for c in (GT_CLASS, 7):
        s.class_stats(c, reset=True)
    off, on = [block(False)], []
    for _ in range(a.blocks):
        on.append(block(True))
        off.append(block(False))
    hs1 = s.host_stats()
    t_gt, mf = s.class_stats(GT_CLASS), s.class_stats(7)
    iters = a.steps * (2 * a.blocks + 1)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"loci": a.loci, "config": a.config, "leaves": pack.n, "selected": nsel, "record_bytes": rb, "bytes_per_sample": row_bytes,
           "steps": a.steps, "ms_per_iter_off_median": round(med(off), 4), "ms_per_iter_gene_trees_median": round(med(on), 4),
           "ms_per_iter_off_blocks": [round(x, 4) for x in off], "ms_per_iter_gene_trees_blocks": [round(x, 4) for x in on],
           "gene_trees_added_ms_per_sampled_iter": round(med(on) - med(off), 4),
           "gene_trees_samples": t_gt["launches"], "gene_trees_kernel_ms_per_sample": round(t_gt["ms"] / max(t_gt["launches"], 1), 5),
           "gene_trees_kernel_GB_per_s_read_plus_written": round(2 * row_bytes / max(t_gt["ms"] / max(t_gt["launches"], 1), 1e-9) / 1e6, 1),
           "syncs_per_iter": (hs1["syncs"] - hs0["syncs"]) / iters, "k_mix_finish_launches": mf["launches"]}
    if a.select == 0:
        # one flush as the program does it: the default buffer filled, fetched, appended to a file
        cap = max(1, min(64, (256 << 20) // row_bytes))
        s.enable_gene_trees(cap, sel)
        for _ in range(cap):
            s.iteration(it)
            s.sample_gene_trees(it)
            it += 1
        buf = np.zeros(cap * row_bytes, dtype=np.uint8)
        its = np.zeros(cap, dtype=np.int32)
        got = C.c_int32()
        with tempfile.TemporaryDirectory() as td, open(os.path.join(td, "flush.part"), "wb") as f:
            t0 = time.perf_counter()
            rc = s.lib.gph_engine_gene_trees_fetch(s.engine, its.ctypes.data_as(C.POINTER(C.c_int32)), buf.ctypes.data, cap, C.byref(got))
            t1 = time.perf_counter()
            buf.tofile(f)
            f.flush()
            t2 = time.perf_counter()
        assert rc == 0 and got.value == cap
        out.update(flush_rows=cap, flush_bytes=cap * row_bytes, flush_fetch_ms=round((t1 - t0) * 1e3, 2), flush_write_ms=round((t2 - t1) * 1e3, 2),
                   flush_ms=round((t2 - t0) * 1e3, 2))
    s.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=0)      # 0: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--select", type=int, default=0)      # 0: all loci
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=420)      # seconds a configuration may take (driver)
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single configuration only)
    a = ap.parse_args()
    sys.exit(drive(a) if a.config == 0 else measure(a))


if __name__ == "__main__":
    main()
