#!/usr/bin/env python3
"""Cost of one sample of the per-locus effective sample sizes (k_ess, timing class 21) on BASELINE configs[3], and the plain
iteration against the parent commit.

  python tools/ess_cost.py [--parent DIR [--bench-only]] [--out profiles/ess_cost_mi355x.json]     the whole job
  python tools/ess_cost.py --measure [--loci 100000] [--samples 30] [--warmup 20] [--launches 9]

Without --measure the tool is a driver: one measurement on configs[3] (100 k loci, 16 leaves; bench.py's --config 4), then --
with --parent DIR, a built checkout of the parent commit -- `bench.py --gpus 1 --steps 40 --warmup 5` of the parent and of this
commit alternately, three times each.  Every step runs in a child process of its own under `timeout -k 10`, one after the
other, and the first one that fails ends the job (nothing more is started on the device after a failure).  With --out the
JSON lines of the job are also written there, as one list.

A measurement runs a plain Sampler for `warmup` iterations, then `samples` iterations with an ESS sample after each, then
`launches` further iterations with a sample each, whose k_ess launch is timed by HIP events, and prints one JSON line: the
kernel's time per launch (median and all), the wall time of the call (no host synchronisation), the bytes a launch moves by the
layout -- per locus the node records (16 N), four scalars, the focal set read by the n - 1 lanes of the locus (counted once:
the repeats hit the cache), and per series the shift, s1, sq[0] and on average two further levels read and written --, the time
that traffic takes at 4 TB/s, and the ratio of the kernel's time to it; the smallest and the median per-locus ESS go along as
a plausibility check."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ESS_CLASS = 21
HBM_BYTES_PER_S = 4.0e12      # what the evaluate kernels reach (DESIGN)


def drive(a):
    me = os.path.abspath(__file__)
    lines = []

    def finish(rc):
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)
                f.write("\n")
        return rc
    if not a.bench_only:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--measure", "--loci", str(a.loci), "--samples", str(a.samples),
               "--warmup", str(a.warmup), "--launches", str(a.launches)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
            print(f"ess_cost: the measurement ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return finish(r.returncode)
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        print(json.dumps(lines[-1]), flush=True)
    if not a.parent:
        return finish(0)
    runs = {"parent": [], "this": []}
    for k in range(3):
        for who, root in (("parent", os.path.abspath(a.parent)), ("this", REPO)):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps),
                   "--warmup", str(a.bench_warmup)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                print(f"ess_cost: bench.py of {who} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                return finish(r.returncode)
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            runs[who].append(res)
            lines.append({"bench": who, "run": k, "value": res.get("value"), "unit": res.get("unit"), "ms_per_step": res.get("ms_per_step")})
            print(json.dumps(lines[-1]), flush=True)
    out = {"bench_ab": True}
    for who, rs in runs.items():
        v = sorted(r["ms_per_step"] for r in rs)
        out[f"{who}.ms_per_step"] = {"median": v[1], "min": v[0], "max": v[2]}
    out["parent_spread_ms"] = out["parent.ms_per_step"]["max"] - out["parent.ms_per_step"]["min"]
    out["median_difference_ms"] = out["this.ms_per_step"]["median"] - out["parent.ms_per_step"]["median"]
    lines.append(out)
    print(json.dumps(out), flush=True)
    return finish(0)


def measure(a):
    import numpy as np
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, 4, a.loci, 6.5, 20261002 + 4, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack, lib=G.load_library(a.lib) if a.lib else None)
    s.initialize()
    s.ess_enable(max_bytes=4 << 30)
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    for _ in range(a.samples):
        s.iteration(it)
        s.ess_sample()
        it += 1
    s.class_stats(ESS_CLASS, reset=True)
    kernel, wall, syncs = [], [], 0
    for _ in range(a.launches):
        s.iteration(it)
        it += 1
        before = s.host_stats()["syncs"]
        t0 = time.perf_counter()
        s.ess_sample()
        wall.append((time.perf_counter() - t0) * 1e3)
        syncs += s.host_stats()["syncs"] - before
        s.iteration(it)                       # (its host synchronisation collects the event times)
        it += 1
        kernel.append(s.last_kernel_ms(ESS_CLASS))
    st = s.class_stats(ESS_CLASS)
    e = s.ess()
    Q, M, J, W, S = s._ess_shape()
    n = pack.n
    N = 2 * n - 1
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    read = 16 * N + 3 * 8 + 2 * 4 + (n - 1) * W * 8 + M * 5 * 8 + 8 + 4
    written = M * 4 * 8 + 8 + 4
    traffic = Q * (read + written)
    floor_ms = traffic / HBM_BYTES_PER_S * 1e3
    res = {"config": 4, "loci": a.loci, "leaves": n, "series": M, "levels": J, "words": W, "samples": S, "launches_timed": a.launches,
           "launches": st["launches"], "syncs_in_the_sample_calls": syncs,
           "kernel_ms_median": round(med(kernel), 5), "kernel_ms": [round(x, 5) for x in kernel],
           "call_wall_ms_median": round(med(wall), 5), "call_wall_ms": [round(x, 5) for x in wall],
           "bytes_read_per_locus": read, "bytes_written_per_locus": written, "device_bytes_per_locus": M * (2 + 2 * J) * 8 + (n - 1) * W * 8 + 12,
           "traffic_bytes": traffic, "traffic_ms_at_4TBps": round(floor_ms, 5), "kernel_over_traffic": round(med(kernel) / floor_ms, 3),
           "min_ess_min": float(np.min(e["min_ess"])), "min_ess_median": float(np.median(e["min_ess"])),
           "topo_changes_mean": float(np.mean(e["changes"])), "loci_whose_topology_never_changed": int(np.count_nonzero(e["changes"] == 0))}
    s.close()
    print(json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")     # one measurement; without: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=300)      # seconds a step may take (driver)
    ap.add_argument("--parent", default=None)             # a built checkout of the parent commit (driver: the bench.py comparison)
    ap.add_argument("--bench-only", action="store_true")  # driver: the bench.py comparison alone
    ap.add_argument("--bench-steps", type=int, default=40)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=None)                # driver: the JSON lines of the job as one list
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single measurement only)
    a = ap.parse_args()
    sys.exit(measure(a) if a.measure else drive(a))


if __name__ == "__main__":
    main()
