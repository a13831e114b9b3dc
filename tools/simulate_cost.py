#!/usr/bin/env python3
"""Cost of one sample of replicate genealogies (k_simulate and the site loop behind it, timing class 25) on BASELINE configs[3],
next to k_coal_stats' and k_predictive's in the same job, and the plain iteration against the parent commit.

  python tools/simulate_cost.py [--parent DIR [--bench-only]] [--out profiles/simulate_cost_mi355x.json]     the whole job
  python tools/simulate_cost.py --measure [--loci 100000] [--warmup 20] [--blocks 4] [--block 10] [--launches 9]

Without --measure the tool is a driver: one measurement on configs[3] (100 k loci, 16 leaves; bench.py's --config 4), then --
with --parent DIR, a built checkout of the parent commit -- `bench.py --gpus 1 --steps 40 --warmup 5` of the parent and of this
commit alternately, three times each.  Every step runs in a child process of its own under `timeout -k 10`, one after the
other, and the first one that fails ends the job (nothing more is started on the device after a failure).  With --out the
JSON lines of the job are also written there, as one list.

A measurement runs a plain Sampler for `warmup` iterations; then, with the sampler enabled WITHOUT sites, `launches` iterations
with a simulate sample whose one kernel (k_simulate alone) is timed by HIP events; then, enabled WITH sites, `blocks` pairs of
blocks of `block` iterations alternately without and with a sample after every iteration (wall time per iteration of either
kind), and `launches` iterations with a simulate, a coal-stats and a predictive sample each, timed by HIP events (class 25 is then
k_simulate + the site loop).  It prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SI_CLASS, PD_CLASS, CS_CLASS = 25, 22, 14


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
            print(f"simulate_cost: the measurement ended with status {r.returncode}; nothing more is started", file=sys.stderr)
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
                print(f"simulate_cost: bench.py of {who} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
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
    capacity = a.blocks * a.block + 2 * a.launches + 1
    s.predictive_enable(20261020, capacity, max_bytes=4 << 30)
    s.enable_coal_stats(capacity)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    # k_simulate alone: the sampler without sites
    s.simulate_enable(20261021, capacity, with_sites=False, max_bytes=4 << 30)
    k_alone = []
    for _ in range(a.launches):
        s.iteration(it)
        s.simulate_sample(it)
        it += 1
        s.iteration(it)                       # (its host synchronisation collects the event times)
        it += 1
        k_alone.append(s.last_kernel_ms(SI_CLASS))
    alone = s.simulate()
    # the whole sample: with sites
    s.simulate_enable(20261021, capacity, with_sites=True, max_bytes=4 << 30)
    per = {False: [], True: []}
    for _ in range(a.blocks):
        for on in (False, True):
            t0 = time.perf_counter()
            for _ in range(a.block):
                s.iteration(it)
                if on:
                    s.simulate_sample(it)
                it += 1
            s.iteration(it)                   # (its host synchronisation ends the block's last sample too; counted in both kinds)
            it += 1
            per[on].append((time.perf_counter() - t0) * 1e3 / (a.block + 1))
    k_si, k_pd, k_cs, syncs = [], [], [], 0
    for _ in range(a.launches):
        s.iteration(it)
        before = s.host_stats()["syncs"]
        s.simulate_sample(it)
        s.predictive_sample(it)
        s.sample_coal_stats(it)
        syncs += s.host_stats()["syncs"] - before
        it += 1
        s.iteration(it)
        it += 1
        k_si.append(s.last_kernel_ms(SI_CLASS))
        k_pd.append(s.last_kernel_ms(PD_CLASS))
        k_cs.append(s.last_kernel_ms(CS_CLASS))
    e = s.simulate()
    recs = s.simulate_records()
    S, Q = e["samples"], len(e["loci"])
    live = float(S) * Q - float(e["failed"].sum())
    names = e["stats"]
    midp = {nm: float((e["acc"][:, c, 0].sum() + e["acc"][:, c, 1].sum() / 2) / live) for c, nm in enumerate(names)} if live > 0 else {}
    res = {"config": 4, "loci": a.loci, "leaves": pack.n, "populations": pack.K, "bands": pack.B, "statistics": len(names), "samples": S,
           "launches_timed": a.launches, "syncs_in_the_sample_calls": syncs,
           "k_simulate_alone_ms_median": round(med(k_alone), 5), "k_simulate_alone_ms": [round(x, 5) for x in k_alone],
           "sample_with_sites_ms_median": round(med(k_si), 5), "sample_with_sites_ms": [round(x, 5) for x in k_si],
           "k_predictive_ms_median": round(med(k_pd), 5), "k_predictive_ms": [round(x, 5) for x in k_pd],
           "k_coal_stats_ms_median": round(med(k_cs), 5), "k_coal_stats_ms": [round(x, 5) for x in k_cs],
           "iteration_ms_without": [round(x, 4) for x in per[False]], "iteration_ms_with_simulate": [round(x, 4) for x in per[True]],
           "added_ms_per_simulate_iteration": round(med(per[True]) - med(per[False]), 4),
           "failed_replicates": float(e["failed"].sum()), "failed_replicates_without_sites": float(alone["failed"].sum()),
           "replicate_migrations_last_sample_mean": float(np.mean(recs["num_migs"])) if Q else 0.0,
           "posterior_mid_p": {k: round(v, 4) for k, v in midp.items()}}
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
