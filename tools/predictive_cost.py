#!/usr/bin/env python3
"""Cost of one posterior predictive sample (k_predictive, timing class 22) on BASELINE configs[3], next to k_coal_stats' in the
same job, and the plain iteration against the parent commit.

  python tools/predictive_cost.py [--parent DIR [--bench-only]] [--out profiles/predictive_cost_mi355x.json]     the whole job
  python tools/predictive_cost.py --measure [--loci 100000] [--warmup 20] [--blocks 4] [--block 10] [--launches 9]

Without --measure the tool is a driver: one measurement on configs[3] (100 k loci, 16 leaves; bench.py's --config 4), then --
with --parent DIR, a built checkout of the parent commit -- `bench.py --gpus 1 --steps 40 --warmup 5` of the parent and of this
commit alternately, three times each.  Every step runs in a child process of its own under `timeout -k 10`, one after the
other, and the first one that fails ends the job (nothing more is started on the device after a failure).  With --out the
JSON lines of the job are also written there, as one list.

A measurement runs a plain Sampler for `warmup` iterations, then `blocks` pairs of blocks of `block` iterations, alternately
without and with a predictive sample after every iteration (wall time per iteration of either kind; every iteration ends with
its own host synchronisation, so the sample's kernel is inside the next one), then the same pairs with a coal-stats sample
instead, then `launches` iterations with a sample of each whose kernels are timed by HIP events.  It prints one JSON line: the
kernels' times per launch (median and all), the added wall time per sampled iteration of both samplers, the sites and nodes a
launch hashes and the 64-bit mixes per second that makes."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PD_CLASS, CS_CLASS = 22, 14


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
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--measure", "--loci", str(a.loci), "--warmup", str(a.warmup),
               "--blocks", str(a.blocks), "--block", str(a.block), "--launches", str(a.launches)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
            print(f"predictive_cost: the measurement ended with status {r.returncode}; nothing more is started", file=sys.stderr)
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
                print(f"predictive_cost: bench.py of {who} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
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
    capacity = a.blocks * a.block + a.launches + 1
    s.predictive_enable(20261020, capacity, max_bytes=4 << 30)
    s.enable_coal_stats(capacity)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731

    def blocks(sample):
        """ms per iteration of the blocks without and with `sample` behind every iteration, interleaved"""
        nonlocal it
        per = {False: [], True: []}
        for _ in range(a.blocks):
            for on in (False, True):
                t0 = time.perf_counter()
                for _ in range(a.block):
                    s.iteration(it)
                    if on:
                        sample(it)
                    it += 1
                s.iteration(it)               # (its host synchronisation ends the block's last sample too; counted in both kinds)
                it += 1
                per[on].append((time.perf_counter() - t0) * 1e3 / (a.block + 1))
        return per
    pd = blocks(s.predictive_sample)
    cs = blocks(s.sample_coal_stats)
    s.class_stats(PD_CLASS, reset=True)
    k_pd, k_cs, syncs = [], [], 0
    for _ in range(a.launches):
        s.iteration(it)
        before = s.host_stats()["syncs"]
        s.predictive_sample(it)
        s.sample_coal_stats(it)
        syncs += s.host_stats()["syncs"] - before
        it += 1
        s.iteration(it)                       # (its host synchronisation collects the event times)
        it += 1
        k_pd.append(s.last_kernel_ms(PD_CLASS))
        k_cs.append(s.last_kernel_ms(CS_CLASS))
    e = s.predictive()
    sites = int(e["sites"].sum())
    N = 2 * pack.n - 1
    mixes = sites * N
    seg = e["acc"][:, 0, :]
    res = {"config": 4, "loci": a.loci, "leaves": pack.n, "current_populations": pack.Kc, "statistics": len(e["stats"]), "samples": e["samples"],
           "sites": sites, "sites_per_locus_mean": round(sites / max(1, len(e["sites"])), 2), "nodes": N, "mixes_per_launch_first_pass": mixes,
           "launches_timed": a.launches, "syncs_in_the_sample_calls": syncs,
           "k_predictive_ms_median": round(med(k_pd), 5), "k_predictive_ms": [round(x, 5) for x in k_pd],
           "mixes_per_s": round(mixes / (med(k_pd) * 1e-3), 1) if med(k_pd) > 0 else None,      # (no event times in a host build)
           "k_coal_stats_ms_median": round(med(k_cs), 5), "k_coal_stats_ms": [round(x, 5) for x in k_cs],
           "iteration_ms_without": [round(x, 4) for x in pd[False]], "iteration_ms_with_predictive": [round(x, 4) for x in pd[True]],
           "added_ms_per_predictive_iteration": round(med(pd[True]) - med(pd[False]), 4),
           "iteration_ms_without_2": [round(x, 4) for x in cs[False]], "iteration_ms_with_coal_stats": [round(x, 4) for x in cs[True]],
           "added_ms_per_coal_stats_iteration": round(med(cs[True]) - med(cs[False]), 4),
           "seg_observed_mean": float(np.mean(seg[:, 0])), "seg_replicate_mean": float(np.mean(seg[:, 3]) / max(1, e["samples"])),
           "seg_p_below_0.025_or_above_0.975": int(np.count_nonzero(np.abs((seg[:, 1] + seg[:, 2] / 2) / max(1, e["samples"]) - 0.5) > 0.475))}
    s.close()
    print(json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")     # one measurement; without: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)      # pairs of blocks without / with a sample every iteration
    ap.add_argument("--block", type=int, default=10)      # iterations a block
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
