"""The consumer of the sweep's draws ahead (GphRngA, g-phocs_amd/csrc/gph_locus.h): draws from the buffer k_rng_ahead filled,
and the in-kernel chunks where a locus runs past them.

64 loci x 8 leaves (synthetic config 1: four populations, one migration band), 3 iterations, against the oracle run live on the
same pack -- records as tests/parity_util.py compares them, the per-locus state byte for byte -- and every setting against the
default one byte for byte, records included:
  default M (512); M = 64 (every locus runs past its draws in mid-sweep); the same with every locus's count of the sweep before
  set so that its draws end within 63 of what it consumes; the pass off; a first sweep with no draws ahead.
A full sweep of such a locus consumes 77 to 123 draws and the draws ahead come in multiples of 64, so no full sweep can end on
its last draw ahead.  The counts that end exactly on draw CN_RAN and on CN_RAN + 1 are met with SPR-only sweeps (the stepwise
entry point, flags 4) at M = 64: they consume 51 to 90 draws, and the data seed is one that puts loci on 64 and on 65.
Host build here, the device under -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from parity_util import compare_records, compare_states
from rng_ahead_util import ahead, assert_stepped, counts, dump, parse_rng, set_env, sweep

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

LOCI, ITERS, DATA_SEED, SPR_SWEEPS = 64, 3, 4173, 4
SETTINGS = {
    "default": {},
    "m64": {"GPH_RNG_AHEAD_DRAWS": "64"},
    "off": {"GPH_RNG_AHEAD": "0"},
    "first0": {"GPH_RNG_AHEAD_FIRST": "0"},
}


def make_pack(G):
    from gphocs_amd_pkg import synth
    pk = synth.make_synthetic_pack(G.Pack, 1, LOCI, mut_scale=6.5, data_seed=DATA_SEED, mcmc_seed=4242, samples_per_log=8)
    assert pk.n == 8 and pk.L == LOCI
    return pk


def run(G, lib, pk, env, tmp, monkeypatch, forced=None):
    """records, state dump with conditionals, counts [ITERS][LOCI] (None with the pass off), (on, M)"""
    set_env(monkeypatch, env)
    s = G.Sampler(pk, lib=lib)
    tr, st = os.path.join(tmp, "trace"), os.path.join(tmp, "state")
    s.set_record_file(tr)
    s.initialize()
    info = ahead(lib, s)
    ks = []
    for it in range(ITERS):
        if forced is not None:
            ahead(lib, s, np.ascontiguousarray(forced[it], dtype=np.int32), set_=True)
        s.iteration(it)
        if info[0]:
            ks.append(counts(s))
    s.dump_state(st, True)
    s.set_record_file(None)
    assert s.debug_oob()[0] == 0
    s.close()
    return dict(trace=tr, state=st, records=open(tr, "rb").read(), dump=open(st, "rb").read(),
                counts=np.array(ks) if ks else None, info=info[:2])


def spr_sweeps(G, lib, pk, env, tmp, monkeypatch):
    """SPR-only sweeps through the stepwise entry point: the state dump after each, the counts [SPR_SWEEPS][LOCI] (pass on)"""
    set_env(monkeypatch, env)
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    on = ahead(lib, s)[0]
    dumps, ks, S = [], [], [parse_rng(dump(s, os.path.join(tmp, "s")))]
    for _ in range(SPR_SWEEPS):
        sweep(s, 4)
        dumps.append(dump(s, os.path.join(tmp, "s"), True))
        S.append(parse_rng(dumps[-1]))
        if on:
            ks.append(counts(s))
    assert s.debug_oob()[0] == 0
    s.close()
    return dumps, np.array(ks) if ks else None, S


def check(G, lib, tmp_path, monkeypatch):
    pk = make_pack(G)
    tmp = {k: str(tmp_path / k) for k in list(SETTINGS) + ["edges", "edges512", "oracle", "spr"]}
    for d in tmp.values():
        os.makedirs(d)
    r = {k: run(G, lib, pk, env, tmp[k], monkeypatch) for k, env in SETTINGS.items()}
    assert r["default"]["info"] == (1, 512) and r["m64"]["info"] == (1, 64) and r["off"]["info"] == (0, 0) and r["first0"]["info"] == (1, 512)
    k = r["default"]["counts"]
    assert k.shape == (ITERS, LOCI) and k.min() > 64, "every locus was meant to run past 64 draws"
    assert (r["m64"]["counts"] == k).all() and (r["first0"]["counts"] == k).all()
    forced = (k // 64) * 64 - 64             # n_ahead = roundup64(forced + 64) = the multiple of 64 at or below the count
    r["edges"] = run(G, lib, pk, {"GPH_RNG_AHEAD_DRAWS": "1024"}, tmp["edges"], monkeypatch, forced=forced)
    r["edges512"] = run(G, lib, pk, {}, tmp["edges512"], monkeypatch, forced=np.minimum(forced, 512 - 64))
    assert (r["edges"]["counts"] == k).all() and (r["edges512"]["counts"] == k).all()
    for name in r:
        assert r[name]["records"] == r["default"]["records"], name
        assert r[name]["dump"] == r["default"]["dump"], name
    # counts that end exactly on the last draw ahead (64 = CN_RAN) and one behind it: SPR-only sweeps at M = 64
    d64, k64, S64 = spr_sweeps(G, lib, pk, SETTINGS["m64"], tmp["spr"], monkeypatch)
    doff, _, _ = spr_sweeps(G, lib, pk, SETTINGS["off"], tmp["spr"], monkeypatch)
    on_last, one_past = int((k64 == 64).sum()), int((k64 == 65).sum())
    # a condition on the data set, not a measurement
    assert on_last >= 1 and one_past >= 1, f"{on_last} / {one_past} locus-sweeps consume 64 / 65 draws: choose another data seed"
    assert d64 == doff
    for i in range(SPR_SWEEPS):
        assert_stepped(S64[i], S64[i + 1], k64[i], f"SPR sweep {i}")
    # the oracle, live, on the same pack
    path = os.path.join(tmp["oracle"], "pack.gpk")
    G.write_pack(pk, path)
    subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "oracle"], check=True, capture_output=True)
    ot, os_ = os.path.join(tmp["oracle"], "trace"), os.path.join(tmp["oracle"], "state")
    subprocess.run([os.path.join(REPO, "oracle", "gphocs_oracle"), "run", path, str(ITERS), ot, os_, str(ITERS - 1), "1"], check=True)
    compare_records(r["default"]["trace"], ot)
    compare_states(r["default"]["state"], os_)


def test_host_build(tmp_path, monkeypatch):
    import run_hostemu as R
    import gphocs_amd as G
    check(G, G.load_library(R.build_hostemu()), tmp_path, monkeypatch)


@pytest.mark.gpu
def test_device(tmp_path, monkeypatch):
    import torch       # first, as the other device tests do: its HIP runtime has to be the one the process starts with
    assert torch.cuda.is_available(), "this test needs the MI355X"
    import gphocs_amd as G
    G.build()
    pk = make_pack(G)
    check(G, G.load_library(dims=(pk.n, pk.K, pk.B)), tmp_path, monkeypatch)
