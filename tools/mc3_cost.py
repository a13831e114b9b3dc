#!/usr/bin/env python3
"""What Metropolis-coupled chains cost on one GPU: rounds of C chains against the plain chain, and what a swap point adds.

  python tools/mc3_cost.py [--parent DIR [--bench-only]]      the whole job, one child process per step
  python tools/mc3_cost.py --config 2 --loci 10000 [--steps 20] [--warmup 200] [--blocks 3]

Without --config the tool is a driver: BASELINE configs[1] (10 000 loci, 8 leaves; --config 2) and configs[3] (100 000 loci, 16
leaves; --config 4), then -- with --parent DIR, a built checkout of the parent commit -- bench.py of this commit and of the
parent alternately, three times each.  Every step runs in a child process of its own under `timeout -k 10`, one after the
other, and the first one that fails ends the job (nothing more is started on the device after a failure).

A measurement holds a plain Sampler and two MC3 groups (C = 2 and 4, beta_c = 1 / (1 + h c) with --heat h, a swap attempted before every
round) on the same data set in one process, pre-rolls all of them, and then times blocks of `steps` rounds alternately:
plain, C = 2, C = 4, plain, ...  A round is one call that ends in every chain's host synchronisation (Sampler.iteration,
MC3.iteration), timed with a host clock, so wall time is the device's time per round.  One JSON line:
  ms per round (median over all rounds of a kind), chain-iterations/s in aggregate and as a fraction of C times the plain
  chain's, and the host time a swap point adds: the median round that began with an ACCEPTED swap minus the median round
  that began with a rejected one (both pay the two uniforms and the decision; the accepted one pays the exchange: at most one
  finish kernel per engine, the event records and waits, and the push of the chain state in front of the next sweep)."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

JOBS = [(2, 10000), (4, 100000)]      # bench.py's numbering


def drive(a):
    me = os.path.abspath(__file__)
    for config, loci in ([] if a.bench_only else JOBS):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--config", str(config), "--loci", str(loci),
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--blocks", str(a.blocks)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"mc3_cost: config {config} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    if not a.parent:
        return 0
    # the plain path: bench.py of this commit and of the parent, alternately
    runs = {"this": [], "parent": []}
    for k in range(3):
        for who, root in (("parent", os.path.abspath(a.parent)), ("this", REPO)):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps),
                   "--warmup", str(a.bench_warmup)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                print(f"mc3_cost: bench.py of {who} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
                return r.returncode
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            runs[who].append(json.loads(line))
            print(json.dumps({"bench": who, "run": k, "result": runs[who][-1]}), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"bench_ab": True}
    for who, rs in runs.items():
        for key in sorted(k for k, v in rs[0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)):
            vals = [r[key] for r in rs if key in r]
            if len(vals) == len(rs) and len(set(vals)) > 1:
                out[f"{who}.{key}"] = {"median": med(vals), "min": min(vals), "max": max(vals), "values": vals}
    print(json.dumps(out), flush=True)
    return 0


def measure(a):
    import gphocs_amd as G
    import bench
    G.build()
    pack = bench.build_workload(G, a.config, a.loci, 6.5, 20261002 + a.config, os.path.join(REPO, "bench_cache"))
    lib = G.load_library(a.lib) if a.lib else None
    plain = G.Sampler(pack, lib=lib)
    plain.initialize()
    groups = {}
    for C in (2, 4):
        groups[C] = G.MC3(pack, [1.0 / (1.0 + a.heat * c) for c in range(C)], swap_every=1, lib=lib)
        groups[C].initialize()
    it = 0
    for _ in range(a.warmup):
        plain.iteration(it)
        for g in groups.values():
            g.iteration(it)
        it += 1
    rounds = {"plain": [], 2: [], 4: []}
    swapped = {2: [], 4: []}            # per timed round of a group: did it begin with an accepted swap?
    for _ in range(a.blocks):
        for kind in ("plain", 2, 4):
            run = plain.iteration if kind == "plain" else groups[kind].iteration
            n0 = sum(groups[kind].swap_counts()[1]) if kind != "plain" else 0
            for k in range(a.steps):
                t0 = time.perf_counter()
                run(it + k)
                rounds[kind].append((time.perf_counter() - t0) * 1e3)
                if kind != "plain":
                    n1 = sum(groups[kind].swap_counts()[1])
                    swapped[kind].append(n1 > n0)
                    n0 = n1
        it += a.steps
    med = lambda v: sorted(v)[len(v) // 2] if v else None
    r4 = lambda x: None if x is None else round(x, 4)
    ms_plain = med(rounds["plain"])
    out = {"config": a.config, "loci": a.loci, "leaves": pack.n, "steps": a.steps, "blocks": a.blocks, "heat": a.heat,
           "hbm_bytes_per_chain": plain.hbm_bytes(), "ms_per_round_plain": r4(ms_plain), "iterations_per_s_plain": r4(1e3 / ms_plain)}
    for C in (2, 4):
        ms = med(rounds[C])
        acc = [t for t, s in zip(rounds[C], swapped[C]) if s]
        rej = [t for t, s in zip(rounds[C], swapped[C]) if not s]
        att, got = groups[C].swap_counts()
        out[f"C{C}"] = {"ms_per_round": r4(ms), "chain_iterations_per_s": r4(C * 1e3 / ms), "fraction_of_C_plain_chains": r4(ms_plain / ms),
                        "round_over_plain_round": r4(ms / ms_plain), "rounds_behind_accepted_swap": len(acc), "rounds_behind_rejected_swap": len(rej),
                        "ms_round_accepted_swap": r4(med(acc)), "ms_round_rejected_swap": r4(med(rej)),
                        "swap_added_ms": r4(med(acc) - med(rej)) if acc and rej else None,
                        "swaps_attempted": sum(att), "swaps_accepted": sum(got)}
    for g in groups.values():
        g.close()
    plain.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=0)      # 0: the driver
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    # the ladder of the timed groups: close enough for swaps of both outcomes at these sizes (lnr = (beta_j - beta_j+1) x a
    # difference of two data log-likelihoods that is in the hundreds here); every beta != 1 runs the heated sweep kernel
    ap.add_argument("--heat", type=float, default=0.003)
    ap.add_argument("--step-timeout", type=int, default=420)      # seconds a step may take (driver)
    ap.add_argument("--parent", default=None)             # a built checkout of the parent commit (driver: the bench.py comparison)
    ap.add_argument("--bench-only", action="store_true")  # driver: the bench.py comparison alone
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--lib", default=None)                # alternative build of the library (a single configuration only)
    a = ap.parse_args()
    sys.exit(drive(a) if a.config == 0 else measure(a))


if __name__ == "__main__":
    main()
