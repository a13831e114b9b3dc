"""The sweep's uniforms generated ahead of it (k_rng_ahead + GphRngA) on the MI355X: the per-locus state and the accept
counters are the same with the pass off (GPH_RNG_AHEAD=0: every draw from the in-kernel chunks), on, and on with room for
only 64 draws per locus (nearly every locus runs past them and goes on with the in-kernel chunks).

The model is the benchmark's (synthetic config 4).  Loci: 5 (less than one wavefront of the lane-per-locus pass), 193 (a
partial last wavefront; mutation scale 26 puts two loci beyond 64 phased patterns, i.e. into the second launch group, which
runs on the side stream and must find its draws too) and 4 160 (65 workgroups of the pass).

On the device the "off" run is new code too (the same generator class, every chunk from its out-of-line function): these
tests compare the paths of the new generator with each other.  That the stream is the parent's is what the parity suite
(goldens of the real reference, the live oracle) and the benchmark's output comparison show."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rng_ahead_util import ENV, info_and_counts as _info

pytestmark = pytest.mark.gpu

SETTINGS = {"off": {"GPH_RNG_AHEAD": "0"}, "on": {}, "m64": {"GPH_RNG_AHEAD_DRAWS": "64"},
            "placeA": {"GPH_RNG_AHEAD_PLACE": "A"}, "noalloc": {"GPH_RNG_AHEAD_FAIL_ALLOC": "1"}}
ITERS = 30


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


def _pack(G, loci, mut):
    from gphocs_amd_pkg import synth
    return synth.make_synthetic_pack(G.Pack, 4, loci, mut_scale=mut, data_seed=4100 + loci, mcmc_seed=4242, samples_per_log=8)


def _run(G, pk, setting, monkeypatch, tmp_path, body):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    s = G.Sampler(pk)
    s.initialize()
    body(s)
    st = str(tmp_path / (setting + ".state"))
    s.dump_state(st, True)
    info, kp = _info(s)
    side = np.zeros(4, dtype=np.int32)
    assert s.lib.gph_engine_rng_ahead_(s.engine, side.ctypes.data, None, -1) == 0
    res = dict(side=(int(side[0]), int(side[1])), state=open(st, "rb").read(), accept=s.accept_counts(), info=info, kprev=kp, launches=s.host_stats())
    assert s.debug_oob()[0] == 0
    s.close()
    return res


def _three_settings_agree(G, pk, monkeypatch, tmp_path, body):
    """every setting against the pass off: on (the pass for the next sweep behind this one's kernel where the engine decides on
    the device, else in front of the sweep), 64 draws, always in front of the sweep, and a failed allocation of the buffers"""
    r = {k: _run(G, pk, k, monkeypatch, tmp_path, body) for k in SETTINGS}
    assert r["off"]["info"][0] == 0 and r["on"]["info"][:3] == (1, 512, 16) and r["m64"]["info"][:3] == (1, 64, 16)
    assert r["placeA"]["info"][:3] == (1, 512, 16) and r["placeA"]["side"] == (0, 0)
    assert r["noalloc"]["info"][0] == 0      # the buffers were not to be had: the run went on without the pass
    for k in ("on", "m64", "placeA", "noalloc"):
        assert r[k]["accept"] == r["off"]["accept"], k
        assert r[k]["state"] == r["off"]["state"], k
    assert (r["on"]["kprev"] == r["m64"]["kprev"]).all()
    return r


@pytest.mark.parametrize("loci,mut", [(5, 6.5), (193, 26.0), (4160, 6.5)])
def test_iterations_same_state_and_counters(G, monkeypatch, tmp_path, loci, mut):
    pk = _pack(G, loci, mut)
    P = np.diff(pk.pattern_offsets)
    if loci == 193:
        assert (P > 64).any() and (P <= 64).sum() > 64, "this data set was meant to have loci in two launch groups"   # max_phased_patterns > 64
    else:
        assert P.max() <= 64

    def body(s):
        for it in range(ITERS):
            s.iteration(it)
    r = _three_settings_agree(G, pk, monkeypatch, tmp_path, body)
    assert r["on"]["side"] == (1, 1)         # chained iterations, decisions on the device: the last sweep left a pass for the next
    kp = r["on"]["kprev"]
    assert kp.min() > 0 and (kp > 64).mean() > 0.9      # the last sweep's counts: M = 64 did send the loci past their draws


def test_stepwise_sweep_entry_point_single_proposal_kinds(G, monkeypatch, tmp_path):
    """gph_engine_genealogy_sweep with flags 1 only (node ages) and 4 only (SPR): both callers of the sweep launch get the pass"""
    pk = _pack(G, 193, 26.0)

    def body(s):
        out = G.GphSweepResult()
        for flags in (1, 4, 1, 4, 4, 1):
            assert s.lib.gph_engine_genealogy_sweep(s.engine, flags, pk.ftCoalTime, pk.ftMigTime, C.byref(out)) == 0
    r = _three_settings_agree(G, pk, monkeypatch, tmp_path, body)
    assert r["on"]["side"][1] == 0           # a stepwise sweep leaves no pass behind it: the next one runs its own in front


def test_variable_locus_rates(G, monkeypatch, tmp_path):
    """golden v8 (`locus-mut-rate VAR`): UpdateLocusRate draws from the per-locus generators between two sweeps, so a pass made
    behind the sweep would be stale: with variable rates the engine decides on the host and every pass runs in front of its sweep"""
    pk = G.Pack.load(os.path.join(GOLDEN, "v8.gpk"))

    def body(s):
        for it in range(ITERS):
            s.iteration(it)
    r = _three_settings_agree(G, pk, monkeypatch, tmp_path, body)
    assert r["on"]["side"] == (0, 0)
