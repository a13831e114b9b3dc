#!/usr/bin/env python3
"""Cost of one comparison of replicate chains' clade tables (k_clades_compare, timing class 20) on BASELINE configs[3], and
the plain iteration against the parent commit.

  python tools/replicates_cost.py [--parent DIR [--bench-only]]     the whole job, one child process per step
  python tools/replicates_cost.py --chains 4 [--loci 100000] [--samples 30] [--warmup 20] [--compares 9] [--slots 0]

Without --chains the tool is a driver: R = 2 and R = 4 chains on configs[3] (100 k loci, 16 leaves; bench.py's --config 4) at
the default slots, then -- with --parent DIR, a built checkout of the parent commit -- `bench.py --gpus 1 --steps 40 --warmup 5`
of the parent and of this commit alternately, three times each.  Every step runs in a child process of its own under
`timeout -k 10`, one after the other, and the first one that fails ends the job (nothing more is started on the device after
a failure).

A measurement runs R plain Samplers (seeds seed + r) for `warmup` iterations, then `samples` iterations with a clades sample
of every chain after each, then `compares` calls of gph_engine_clades_compare, and prints one JSON line: the kernel's time per
call from HIP events (median and all), the wall time of the call (launch, copy of the rows, the one host synchronisation), the
table traffic R x nsel x P x (W + 2) x 8 bytes read once, the time that traffic takes at 4 TB/s, and the ratio of the kernel's
time to it; the mean and maximum ASDSF over the loci go along as a plausibility check."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CMP_CLASS = 20
HBM_BYTES_PER_S = 4.0e12      # what the evaluate kernels reach (DESIGN)


def drive(a):
    me = os.path.abspath(__file__)
    for chains in ([] if a.bench_only else (2, 4)):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--chains", str(chains), "--loci", str(a.loci), "--samples", str(a.samples),
               "--warmup", str(a.warmup), "--compares", str(a.compares), "--slots", str(a.slots)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"replicates_cost: {chains} chains ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    if not a.parent:
        return 0
    runs = {"parent": [], "this": []}
    for k in range(3):
        for who, root in (("parent", os.path.abspath(a.parent)), ("this", REPO)):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps),
                   "--warmup", str(a.bench_warmup)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                print(f"replicates_cost: bench.py of {who} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                return r.returncode
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            runs[who].append(res)
            print(json.dumps({"bench": who, "run": k, "value": res.get("value"), "unit": res.get("unit"), "ms_per_step": res.get("ms_per_step")}), flush=True)
    out = {"bench_ab": True}
    for who, rs in runs.items():
        v = sorted(r["ms_per_step"] for r in rs)
        out[f"{who}.ms_per_step"] = {"median": v[1], "min": v[0], "max": v[2]}
    out["parent_spread_ms"] = out["parent.ms_per_step"]["max"] - out["parent.ms_per_step"]["min"]
    out["median_difference_ms"] = out["this.ms_per_step"]["median"] - out["parent.ms_per_step"]["median"]
    print(json.dumps(out), flush=True)
    return 0


def measure(a):
    import copy
    import numpy as np
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, 4, a.loci, 6.5, 20261002 + 4, os.path.join(REPO, "bench_cache"))
    chains = []
    for r in range(a.chains):
        q = copy.copy(pack)
        q.seed = pack.seed + r
        s = G.Sampler(q, lib=G.load_library(a.lib) if a.lib else None)
        s.initialize()
        s.enable_clades(a.slots, max_bytes=4 << 30)
        chains.append(s)
    it = 0
    for _ in range(a.warmup):
        for s in chains:
            s.iteration(it)
        it += 1
    for _ in range(a.samples):
        for s in chains:
            s.iteration(it)
            s.sample_clades()
        it += 1
    Q, P, W, limit, S = chains[0]._clades_shape()
    lead = chains[0]
    G.clades_compare(chains, a.min_freq)          # the first call allocates the rows and loads the code object
    lead.class_stats(CMP_CLASS, reset=True)
    hs0 = lead.host_stats()
    kernel, wall = [], []
    for _ in range(a.compares):
        t0 = time.perf_counter()
        out = G.clades_compare(chains, a.min_freq)
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(lead.last_kernel_ms(CMP_CLASS))
    hs1 = lead.host_stats()
    st = lead.class_stats(CMP_CLASS)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    traffic = a.chains * Q * P * (W + 2) * 8
    floor_ms = traffic / HBM_BYTES_PER_S * 1e3
    res = {"config": 4, "loci": a.loci, "leaves": pack.n, "chains": a.chains, "slots": P, "limit": limit, "words": W, "samples": S, "min_freq": a.min_freq,
           "compares": a.compares, "launches": st["launches"], "syncs_per_compare": (hs1["syncs"] - hs0["syncs"]) / a.compares,
           "kernel_ms_median": round(med(kernel), 5), "kernel_ms": [round(x, 5) for x in kernel],
           "call_wall_ms_median": round(med(wall), 5), "call_wall_ms": [round(x, 5) for x in wall],
           "table_traffic_bytes": traffic, "traffic_ms_at_4TBps": round(floor_ms, 5), "kernel_over_traffic": round(med(kernel) / floor_ms, 3),
           "asdsf_mean": float(np.mean(out["asdsf"])), "asdsf_max": float(np.max(out["asdsf"])),
           "compared_mean": float(np.mean(out["compared"])), "distinct_mean": float(np.mean(out["distinct"])),
           "fraction_of_loci_with_dropped": round(float(np.count_nonzero(out["dropped"])) / max(Q, 1), 5)}
    for s in chains:
        s.close()
    print(json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=0)      # 0: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--compares", type=int, default=9)
    ap.add_argument("--slots", type=int, default=0)       # 0: the default, the smallest power of two >= 8 (leaves - 1)
    ap.add_argument("--min-freq", type=float, default=0.1)
    ap.add_argument("--step-timeout", type=int, default=300)      # seconds a step may take (driver)
    ap.add_argument("--parent", default=None)             # a built checkout of the parent commit (driver: the bench.py comparison)
    ap.add_argument("--bench-only", action="store_true")  # driver: the bench.py comparison alone
    ap.add_argument("--bench-steps", type=int, default=40)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single measurement only)
    a = ap.parse_args()
    sys.exit(drive(a) if a.chains == 0 else measure(a))


if __name__ == "__main__":
    main()
