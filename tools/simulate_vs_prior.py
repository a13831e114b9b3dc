#!/usr/bin/env python3
"""The end-to-end check of `--simulate` against the sampler itself: a chain at beta 0 samples genealogies from p(G | Theta), the
simulator draws replicates from the same density, so G_s and G_rep are exchangeable given Theta_s and the genome-wide mid-p of
every genealogy statistic must centre on 0.5.  How far from 0.5 chance carries it depends on the chain's autocorrelation and is
not known in advance; a statistic visibly off 0.5 points to the simulator or to the sampler.

  python tools/simulate_vs_prior.py [--cases m3 a7] [--burnin 500] [--samples 2000] [--skip 4] [--host-emulation] [--out FILE]

Per case (a golden pack under tests/golden: m3 has two bands, a7 ancient samples) one Sampler runs `burnin` iterations at beta 0,
then `samples` samples `skip + 1` iterations apart, each followed by one simulate sample of every locus (the genealogy level
alone).  It prints one JSON line per case: per statistic the mid-p pooled over loci and samples, (sum gt + sum eq / 2) /
(replicates that did not fail), the sampled and the replicate mean, and the failed replicates.  --host-emulation: the host build
of the engine sources (no GPU)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run_case(G, lib, name, a):
    pk = G.Pack.load(os.path.join(REPO, "tests", "golden", name + ".gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        s.set_beta(0.0)
        s.simulate_enable(a.seed, 64, with_sites=False)
        s.initialize()
        it = 0
        for _ in range(a.burnin):
            s.iteration(it)
            it += 1
        s.simulate(reset=True)
        for k in range(a.samples):
            for _ in range(a.skip + 1):
                s.iteration(it)
                it += 1
            s.simulate_sample(it)
            if (k + 1) % 64 == 0:
                s.simulate_rows()
        e = s.simulate()
    finally:
        s.close()
    acc = e["acc"]
    live = float(e["samples"]) * len(e["loci"]) - float(e["failed"].sum())
    out = {"case": name, "beta": 0.0, "loci": len(e["loci"]), "leaves": pk.n, "bands": pk.B, "burnin": a.burnin, "samples": e["samples"], "skip": a.skip,
           "failed": float(e["failed"].sum()), "statistics": {}}
    for c, nm in enumerate(e["stats"]):
        out["statistics"][nm] = {"mid_p": round(float((acc[:, c, 0].sum() + acc[:, c, 1].sum() / 2) / live), 4),
                                 "sampled_mean": float(acc[:, c, 2].sum() / live), "replicate_mean": float(acc[:, c, 3].sum() / live)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["m3", "a7"])
    ap.add_argument("--burnin", type=int, default=500)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--host-emulation", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gphocs_amd as G
    lib = None
    if a.host_emulation:
        sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))
        import run_hostemu
        lib = G.load_library(run_hostemu.build_hostemu())
    else:
        G.build()
    lines = []
    for name in a.cases:
        lines.append(run_case(G, lib, name, a))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
