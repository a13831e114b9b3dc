#!/usr/bin/env python3
"""Cost of one expected-substitutions sample (k_mutations with its fold, timing class 24) on BASELINE configs[3] with all loci
selected, next to one k_coal_stats launch of the same run as the yardstick, each as a fraction of a plain iteration.

  python tools/mutations_cost.py [--out profiles/mutations_cost_mi355x.json]                    the whole job
  python tools/mutations_cost.py --measure [--loci 100000] [--warmup 200] [--plain 40] [--launches 9]

Without --measure the tool is a driver: the measurement runs in a child process of its own under `timeout -k 10`, and a child
that fails ends the job (nothing more is started on the device after a failure).  With --out the JSON line is also written
there, in a list.

A measurement runs a plain Sampler on configs[3] (100 k loci, 16 leaves; bench.py's --config 4) for `warmup` iterations (200, the
pre-roll bench.py uses), times `plain` iterations by the wall clock (every iteration ends with its own host synchronisation), then
`launches` iterations with one sample of both samplers, whose kernels are timed by HIP events; the medians are reported.  The
bytes one launch reads are counted from the pack: the current half of every conditional array, the sequence blocks and the node
records.  It prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MU_CLASS, CS_CLASS = 24, 14


def drive(a):
    me = os.path.abspath(__file__)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--measure", "--loci", str(a.loci), "--warmup", str(a.warmup),
           "--plain", str(a.plain), "--launches", str(a.launches)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
        print(f"mutations_cost: the measurement ended with status {r.returncode}; nothing more is started", file=sys.stderr)
        return r.returncode
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump([line], f, indent=1)
            f.write("\n")
    return 0


def measure(a):
    import numpy as np
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, 4, a.loci, 6.5, 20261002 + 4, os.path.join(REPO, "bench_cache"))
    s = G.Sampler(pack, lib=G.load_library(a.lib) if a.lib else None)
    capacity = a.launches + 1
    s.mutations_enable(capacity)
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
    out, syncs = {MU_CLASS: [], CS_CLASS: []}, 0
    for _ in range(a.launches):
        s.iteration(it)
        before = s.host_stats()["syncs"]
        s.mutations_sample(it)
        s.sample_coal_stats(it)
        syncs += s.host_stats()["syncs"] - before
        it += 1
        s.iteration(it)                       # (its host synchronisation collects the event times)
        it += 1
        for c in out:
            out[c].append(s.last_kernel_ms(c))
    e = s.mutations()
    rows = s.mutations_rows()[1]
    n, K, N = pack.n, pack.K, 2 * pack.n - 1
    P = np.diff(pack.pattern_offsets).astype(np.int64)
    cond_bytes = int(32 * (n - 1) * P.sum())
    seq_bytes = int(((n + 1) // 2 * P + 6 * P).sum())
    t_mu, t_cs = med(out[MU_CLASS]), med(out[CS_CLASS])
    tot_mut, tot_exp = float(rows[-1][:K].sum()), float(rows[-1][K:2 * K].sum())
    res = {"config": 4, "loci": a.loci, "leaves": n, "populations": K, "columns": 2 * (K + n), "chunk": e["chunk"], "samples": e["samples"],
           "launches_timed": a.launches, "syncs_in_the_sample_calls": syncs,
           "patterns_mean": round(float(P.mean()), 2), "patterns_max": int(P.max()),
           "bytes_read_per_launch": cond_bytes + seq_bytes + 16 * N * a.loci, "conditional_bytes_read_per_launch": cond_bytes,
           "iteration_ms": round(iteration_ms, 4),
           "k_mutations_ms_median": round(t_mu, 5), "k_mutations_ms": [round(x, 5) for x in out[MU_CLASS]],
           "k_coal_stats_ms_median": round(t_cs, 5), "k_coal_stats_ms": [round(x, 5) for x in out[CS_CLASS]],
           "k_mutations_fraction_of_iteration": round(t_mu / iteration_ms, 5), "k_coal_stats_fraction_of_iteration": round(t_cs / iteration_ms, 5),
           "k_mutations_gb_per_s": round((cond_bytes + seq_bytes + 16 * N * a.loci) / (t_mu * 1e6), 1) if t_mu > 0 else 0.0,
           "last_row_sum_mut": tot_mut, "last_row_sum_exp": tot_exp, "last_row_rel": tot_mut / tot_exp if tot_exp else 0.0}
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
