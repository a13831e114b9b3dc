#!/usr/bin/env python3
"""Cost of one sfs sample (k_sfs_tree + its fold, timing class 27) and of the one-off data pass (k_sfs_data, class 28) on BASELINE
configs[3], next to one k_pair_times, one k_triplets and one k_coal_stats launch of the same run, each as a fraction of a plain
iteration; and the genome-wide observed / expected ratio per slot on that configuration's synthetic data (drawn under the model).

  python tools/sfs_cost.py [--out profiles/sfs_cost_mi355x.json]                      the whole job
  python tools/sfs_cost.py --measure [--loci 100000] [--warmup 200] [--plain 40] [--launches 9] [--settle 2000]

Without --measure the tool is a driver: the measurement runs in a child process of its own under `timeout -k 10`, and a child
that fails ends the job (nothing more is started on the device after a failure).  With --out the JSON line is also written
there, in a list.

A measurement runs a plain Sampler on configs[3] (100 k loci, 16 leaves, 5 current populations; bench.py's --config 4) with all
loci selected and the default slots, for `warmup` iterations (200, the pre-roll bench.py uses), times `plain` iterations by the
wall clock (every iteration ends with its own host synchronisation), then `launches` iterations with one sample of each of the
four samplers whose kernels are timed by HIP events.  The ratios are the data's totals over the mean of the `launches` rows; they
are taken a second time after `settle` further iterations (2 000), because the pre-roll may end before the genealogies have
settled.  It prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SF_CLASS, SD_CLASS, PT_CLASS, TR_CLASS, CS_CLASS = 27, 28, 26, 23, 14


def drive(a):
    me = os.path.abspath(__file__)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--measure", "--loci", str(a.loci), "--warmup", str(a.warmup),
           "--plain", str(a.plain), "--launches", str(a.launches), "--settle", str(a.settle)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
        print(f"sfs_cost: the measurement ended with status {r.returncode}; nothing more is started", file=sys.stderr)
        return r.returncode
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump([line], f, indent=1)
            f.write("\n")
    return 0


def measure(a):
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, 4, a.loci, 6.5, 20261002 + 4, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack, lib=G.load_library(a.lib) if a.lib else None)
    capacity = a.launches + 1
    t0 = time.perf_counter()
    s.sfs_enable(capacity)
    enable_ms = (time.perf_counter() - t0) * 1e3
    s.pair_times_enable(capacity, [1e-6 * (1e4 ** (k / 32.0)) for k in range(33)])
    s.triplets_enable(capacity)
    s.enable_coal_stats(capacity)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    data_ms = s.last_kernel_ms(SD_CLASS)        # (the first host synchronisation collected the event times of the data pass)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    t0 = time.perf_counter()
    for _ in range(a.plain):
        s.iteration(it)
        it += 1
    iteration_ms = (time.perf_counter() - t0) * 1e3 / a.plain
    classes = (SF_CLASS, PT_CLASS, TR_CLASS, CS_CLASS)
    k, syncs = {c: [] for c in classes}, 0
    for _ in range(a.launches):
        s.iteration(it)
        before = s.host_stats()["syncs"]
        s.sfs_sample(it)
        s.pair_times_sample(it)
        s.triplets_sample(it)
        s.sample_coal_stats(it)
        syncs += s.host_stats()["syncs"] - before
        it += 1
        s.iteration(it)                       # (its host synchronisation collects the event times)
        it += 1
        for c in classes:
            k[c].append(s.last_kernel_ms(c))
    e, o = s.sfs(), s.sfs_observed()
    _, rows = s.sfs_rows()
    NS, NG, group = s._sfs_shape()[:3]
    mean = rows.mean(axis=0)
    ratios = {nm: (round(float(o["obs_total"][j]) / float(mean[j]), 5) if mean[j] > 0 else None) for j, nm in enumerate(e["columns"])}
    spectrum = [j for j in range(NS) if int(e["slots"][j, 1]) == 0]
    together = lambda m: round(float(sum(int(o["obs_total"][j]) for j in spectrum)) / float(sum(m[j] for j in spectrum)), 5)     # noqa: E731
    # the same ratios once the chain has run `settle` iterations more: the pre-roll may end before the genealogies have settled
    for _ in range(a.settle):
        s.iteration(it)
        it += 1
    for _ in range(a.launches):
        s.iteration(it)
        s.sfs_sample(it)
        it += 1
    _, late = s.sfs_rows()
    late_mean = late.mean(axis=0)
    late_ratios = {nm: (round(float(o["obs_total"][j]) / float(late_mean[j]), 5) if late_mean[j] > 0 else None) for j, nm in enumerate(e["columns"])}
    N = 2 * pack.n - 1
    res = {"config": 4, "loci": a.loci, "leaves": pack.n, "current_populations": pack.Kc, "samples_per_population": [int(x) for x in pack.samplesPerPop[:pack.Kc]],
           "slots": NS, "groups": NG, "loci_a_workgroup": group, "samples": e["samples"], "launches_timed": a.launches,
           "syncs_in_the_sample_calls": syncs, "bytes_read_per_launch": (16 * N + 4 * NG) * a.loci, "bytes_read_and_written_per_launch": 8 * NS * a.loci,
           "iteration_ms": round(iteration_ms, 4),
           "k_sfs_tree_and_fold_ms_median": round(med(k[SF_CLASS]), 5), "k_sfs_tree_and_fold_ms": [round(x, 5) for x in k[SF_CLASS]],
           "k_sfs_data_ms_once": round(data_ms, 5), "sfs_enable_wall_ms": round(enable_ms, 3),
           "k_pair_times_ms_median": round(med(k[PT_CLASS]), 5), "k_pair_times_ms": [round(x, 5) for x in k[PT_CLASS]],
           "k_triplets_ms_median": round(med(k[TR_CLASS]), 5), "k_triplets_ms": [round(x, 5) for x in k[TR_CLASS]],
           "k_coal_stats_ms_median": round(med(k[CS_CLASS]), 5), "k_coal_stats_ms": [round(x, 5) for x in k[CS_CLASS]],
           "k_sfs_tree_fraction_of_iteration": round(med(k[SF_CLASS]) / iteration_ms, 5), "k_pair_times_fraction_of_iteration": round(med(k[PT_CLASS]) / iteration_ms, 5),
           "k_triplets_fraction_of_iteration": round(med(k[TR_CLASS]) / iteration_ms, 5), "k_coal_stats_fraction_of_iteration": round(med(k[CS_CLASS]) / iteration_ms, 5),
           "sites_total": o["sites_total"], "observed_total": {nm: int(o["obs_total"][j]) for j, nm in enumerate(e["columns"])},
           "expected_mean": {nm: round(float(mean[j]), 3) for j, nm in enumerate(e["columns"])},
           "observed_over_expected": ratios,
           "observed_over_expected_spectrum_slots_together": together(mean),
           "settle_iterations": a.settle, "iterations_before_the_late_samples": it - a.launches,
           "observed_over_expected_late": late_ratios, "observed_over_expected_late_spectrum_slots_together": together(late_mean)}
    s.close()
    print(json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")     # one measurement; without: the driver
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=200)    # bench.py's pre-roll
    ap.add_argument("--plain", type=int, default=40)      # plain iterations timed by the wall clock
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--settle", type=int, default=2000)   # further iterations before the ratios are taken a second time
    ap.add_argument("--step-timeout", type=int, default=300)      # seconds the measurement may take (driver)
    ap.add_argument("--out", default=None)                # driver: the JSON line of the job, in a list
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single measurement only)
    a = ap.parse_args()
    sys.exit(measure(a) if a.measure else drive(a))


if __name__ == "__main__":
    main()
