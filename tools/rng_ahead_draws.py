#!/usr/bin/env python3
"""Draws a locus consumes per sweep on the benchmark workload, and how often the draws generated ahead of the sweep
(k_rng_ahead: min(M, roundup64(previous count + margin))) would not have been enough, for a few M and margins.
Host-emulation build, no GPU:  tools/rng_ahead_draws.py [loci=2000] [preroll=50] [iters=50] > profiles/r07_rng_ahead_draws.txt"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))
import gphocs_amd as G  # noqa: E402
import bench  # noqa: E402
import run_hostemu as R  # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
pre = int(sys.argv[2]) if len(sys.argv) > 2 else 50
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 50
os.environ["GPH_RNG_AHEAD_DRAWS"] = "4096"      # the counts do not depend on it; large enough to see every count as it is
lib = G.load_library(R.build_hostemu())
pack = bench.build_workload(G, 4, L, 6.5, 20261006, os.path.join(REPO, "bench_cache"), begin=0, L_total=100000)
s = G.Sampler(pack, lib=lib)
s.initialize()
fn = lib.gph_engine_rng_ahead_
fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
rows = []
for it in range(pre + iters):
    s.iteration(it)
    kp = np.zeros(L, dtype=np.int32)
    assert fn(s.engine, None, kp.ctypes.data, 0) == 0
    rows.append(kp)
s.close()
c = np.array(rows)            # [iteration][locus]
cur, prev = c[pre:], c[pre - 1:-1]
flat = cur.ravel()
print(f"bench workload (config 4, mut-scale 6.5, seed 20261006), first {L} loci of 100 000, host-emulation build")
print(f"draws per locus and sweep, {iters} iterations after a {pre}-iteration pre-roll ({flat.size} locus-sweeps):")
print(f"  mean {flat.mean():.1f}  median {np.median(flat):.0f}  99th {np.percentile(flat, 99):.0f}  99.9th {np.percentile(flat, 99.9):.0f}  max {flat.max()}")
print(f"  sweep-to-sweep change of a locus: mean |d| {np.abs(cur - prev).mean():.1f}, 99.9th of (count - previous) {np.percentile(cur - prev, 99.9):.0f}, max {(cur - prev).max()}")
print("locus-sweeps that run past n_ahead = min(M, roundup64(previous + margin)), and draws written per locus and sweep:")
for M in (256, 320, 384, 448, 512, 640, 768):
    for margin in (0, 64, 128):
        n = np.minimum(M, (prev + margin + 63) // 64 * 64)
        print(f"  M {M:4d} margin {margin:3d}: {np.mean(cur > n) * 1000:8.3f} per 1000   written {n.mean():6.1f} (fixed M: {M})   read {((np.minimum(cur, n) + 63) // 64 * 64).mean():6.1f}")
