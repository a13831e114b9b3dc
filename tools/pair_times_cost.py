#!/usr/bin/env python3
"""Cost of one pair-times sample (k_pair_times, timing class 26) on BASELINE configs[3], next to one k_triplets and one
k_coal_stats launch of the same run, each as a fraction of a plain iteration.

  python tools/pair_times_cost.py [--out profiles/pair_times_cost_mi355x.json]                      the whole job
  python tools/pair_times_cost.py --measure [--loci 100000] [--warmup 200] [--plain 40] [--launches 9]

Without --measure the tool is a driver: the measurement runs in a child process of its own under `timeout -k 10`, and a child
that fails ends the job (nothing more is started on the device after a failure).  With --out the JSON line is also written
there, in a list.

A measurement runs a plain Sampler on configs[3] (100 k loci, 16 leaves, 5 current populations: the default 15 pairs, the default
grid 1e-6,1e-2,34: 540 numbers a row; bench.py's --config 4) for `warmup` iterations (200, the pre-roll bench.py uses), times
`plain` iterations by the wall clock (every iteration ends with its own host synchronisation), then `launches` iterations with
one sample of each of the three samplers whose kernels are timed by HIP events.  The per-phase split of k_pair_times comes from
launches of the same kernel with ONE pair (1 slot instead of 15: stage and phase 1 are unchanged, phase 2 has a fifteenth of its
tasks): phase 2 of the full launch is about (t_all - t_one) * NP / (NP - 1), the rest is stage + phase 1.  It prints one JSON
line."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PT_CLASS, TR_CLASS, CS_CLASS = 26, 23, 14
GRID = (1e-6, 1e-2, 34)


def grid(lo, hi, B):
    E = B - 1
    return [lo if k == 0 else hi if k == E - 1 else lo * math.pow(hi / lo, float(k) / float(E - 1)) for k in range(E)]


def drive(a):
    me = os.path.abspath(__file__)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--measure", "--loci", str(a.loci), "--warmup", str(a.warmup),
           "--plain", str(a.plain), "--launches", str(a.launches)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
        print(f"pair_times_cost: the measurement ended with status {r.returncode}; nothing more is started", file=sys.stderr)
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
    edges = grid(*GRID)
    s.pair_times_enable(capacity, edges)
    s.triplets_enable(capacity)
    s.enable_coal_stats(capacity)
    s.initialize()
    it = 0
    for _ in range(a.warmup):
        s.iteration(it)
        it += 1
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    t0 = time.perf_counter()
    for _ in range(a.plain):
        s.iteration(it)
        it += 1
    iteration_ms = (time.perf_counter() - t0) * 1e3 / a.plain

    def timed(classes, sample):
        """per class the HIP-event times of `launches` launches, one behind each iteration"""
        nonlocal it
        out, syncs = {c: [] for c in classes}, 0
        for _ in range(a.launches):
            s.iteration(it)
            before = s.host_stats()["syncs"]
            sample(it)
            syncs += s.host_stats()["syncs"] - before
            it += 1
            s.iteration(it)                       # (its host synchronisation collects the event times)
            it += 1
            for c in classes:
                out[c].append(s.last_kernel_ms(c))
        return out, syncs

    def all_three(i):
        s.pair_times_sample(i)
        s.triplets_sample(i)
        s.sample_coal_stats(i)
    k, syncs = timed((PT_CLASS, TR_CLASS, CS_CLASS), all_three)
    e = s.pair_times()
    _, rows = s.pair_times_rows()
    NP, B, group = s._pair_times_shape()[:3]
    members = [int(x) for x in pack.samplesPerPop[:pack.Kc]]
    m = [members[P] * (members[P] - 1) // 2 if P == Q else members[P] * members[Q] for P, Q in e["pairs"].tolist()]
    ok = all(int(row[sl * B:(sl + 1) * B].sum()) == len(e["loci"]) * m[sl] for row in rows for sl in range(NP))
    used = sorted({int(b) for row in rows for sl in range(NP) for b in range(B) if row[sl * B + b]})
    s.pair_times_enable(capacity, edges, pairs=[(0, 1)])
    one, _ = timed((PT_CLASS,), s.pair_times_sample)
    t_all, t_one = med(k[PT_CLASS]), med(one[PT_CLASS])
    phase2 = (t_all - t_one) * NP / max(1, NP - 1)
    N = 2 * pack.n - 1
    res = {"config": 4, "loci": a.loci, "leaves": pack.n, "current_populations": pack.Kc, "pairs": NP, "bins": B, "row_numbers": NP * (B + 2),
           "loci_a_workgroup": group, "samples": e["samples"], "bins_used": used,
           "histograms_sum_to_the_leaf_pairs_at_every_sample": bool(ok), "launches_timed": a.launches, "syncs_in_the_sample_calls": syncs,
           "bytes_read_per_launch": 16 * N * a.loci, "bytes_read_and_written_per_launch": 32 * NP * a.loci,
           "iteration_ms": round(iteration_ms, 4),
           "k_pair_times_ms_median": round(t_all, 5), "k_pair_times_ms": [round(x, 5) for x in k[PT_CLASS]],
           "k_triplets_ms_median": round(med(k[TR_CLASS]), 5), "k_triplets_ms": [round(x, 5) for x in k[TR_CLASS]],
           "k_coal_stats_ms_median": round(med(k[CS_CLASS]), 5), "k_coal_stats_ms": [round(x, 5) for x in k[CS_CLASS]],
           "k_pair_times_fraction_of_iteration": round(t_all / iteration_ms, 5), "k_triplets_fraction_of_iteration": round(med(k[TR_CLASS]) / iteration_ms, 5),
           "k_coal_stats_fraction_of_iteration": round(med(k[CS_CLASS]) / iteration_ms, 5),
           "k_pair_times_one_pair_ms_median": round(t_one, 5), "k_pair_times_one_pair_ms": [round(x, 5) for x in one[PT_CLASS]],
           "k_pair_times_phase2_ms_estimate": round(phase2, 5), "k_pair_times_stage_and_phase1_ms_estimate": round(t_all - phase2, 5)}
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
    ap.add_argument("--step-timeout", type=int, default=300)      # seconds the measurement may take (driver)
    ap.add_argument("--out", default=None)                # driver: the JSON line of the job, in a list
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single measurement only)
    a = ap.parse_args()
    sys.exit(measure(a) if a.measure else drive(a))


if __name__ == "__main__":
    main()
