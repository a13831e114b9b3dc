"""The sweep's draws ahead (k_rng_ahead + GphRngA) on the MI355X against a generator written a second time
(tests/rng_ahead_util.py): the bodies of tests/test_rng_ahead_stream.py on the device forms -- the transposed tile store and
its per-lane gates, rng_chunk64, the 512-byte refill load, lane 0 writing the count -- and what exists only here: the pass
that runs behind a chained sweep on a stream of its own (placement B) and its hand-over to and from everything that voids it.
Everything is exact: 32-bit integers and IEEE doubles compared as bit patterns."""
import os

import numpy as np
import pytest

import rng_ahead_util as U
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.fixture(scope="module")
def pk193(G):
    pk = U.synthetic_pack(G, 4, 193, 26.0)
    P = np.diff(pk.pattern_offsets)
    assert (P > 64).any() and (P <= 64).sum() > 64, "this data set was meant to have loci in two launch groups"
    return pk


def _lib(G, pk):
    return G.load_library(dims=(pk.n, pk.K, pk.B))


@pytest.mark.parametrize("case", list(U.PASS_CASES))
def test_pass_against_the_independent_generator(G, case, monkeypatch, tmp_path):
    """counts from -64 to 2^20 side by side in every wavefront of k_rng_ahead (nmax by shuffle, the d0 < n gate, the n_of[r]
    mask of the tile store, the checkpoint at d1): what each lane had to write is the independent generator's, what it had
    not is untouched, and the sweep that consumed the draws left every generator k steps on"""
    loci, mut, env, vals = U.PASS_CASES[case]
    M, Cd, ns = U.expected_n(case)
    pk = U.synthetic_pack(G, 4, loci, mut)
    got = U.check_pass(G, _lib(G, pk), pk, env, vals, monkeypatch, tmp_path)
    assert got[:2] == (M, Cd)
    if loci >= len(vals):
        assert got[2] == ns


@pytest.fixture(scope="module")
def plain(G, pk193, tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        return U.first_sweep(G, _lib(G, pk193), pk193, mp, tmp_path_factory.mktemp("plain"))
    finally:
        mp.undo()


@pytest.mark.parametrize("edge", ["a", "b", "c", "a@checked"])
def test_counts_forced_onto_the_chunk_edges(G, pk193, plain, edge, monkeypatch, tmp_path):
    """the first sweep after initialize() is deterministic; its counts k0 (199 .. 313 on this data set) put 13 / 12 / 10 loci on
    the residues 0 / 1 / 63 of 64.  Fresh engines with the previous counts forced through the hook:
    (a) n = (k0 // 64) * 64: every locus runs from its draws ahead into its first in-kernel chunk; k0 % 64 == 0 ends exactly
        on the last draw ahead (rng_store: the last checkpoint, no replay), == 1 takes exactly one draw from rng_chunk64,
        == 63 ends one short of a chunk;
    (b) n = ((k0 - 1) // 64) * 64: k0 % 64 == 0 ends on the last draw of an in-kernel chunk (rng_store replays 64 steps);
    (c) n = 0 although M > 0: nothing comes from the buffer.
    a@checked: (a) through the checked build, the indices of rng_refill, rng_store and the pass under its index checks"""
    k0 = plain["k"]
    assert U.check_edge_residues(k0) == [13, 12, 10]
    assert plain["oob"] == (0, 0)
    lib = _lib(G, pk193)
    if edge.endswith("@checked"):
        chk = os.path.join(REPO, "g-phocs_amd", G.CHECKED_LIB)
        assert os.path.exists(chk)
        lib = G.load_library(chk)
        assert lib.gph_build_id().decode().startswith("chk-")
    got = U.first_sweep(G, lib, pk193, monkeypatch, tmp_path, U.edge_counts(k0)[edge[0]])
    U.check_forced(plain, got, edge)
    assert got["oob"] == (0, int(edge.endswith("@checked")))


def test_a_sweep_that_draws_nothing(G, monkeypatch, tmp_path):
    """k = 0: flags 2 (migration nodes only) on the synthetic model without migration bands -- synth.CONFIGS[2]; CONFIGS[1] has
    a band -- hands out no draw: every count 0, every generator where it was, and the next pass generates 64 draws from there"""
    pk = U.synthetic_pack(G, 2, 65, 6.5)
    U.check_no_draws(G, _lib(G, pk), pk, monkeypatch, tmp_path)


def test_hand_overs_between_the_placements(G, pk193, monkeypatch, tmp_path):
    """One script of calls (rng_ahead_util.handover_script) with the pass off, with the default placement (behind the sweep
    where the engine decides on the device) and with GPH_RNG_AHEAD_PLACE=A; after every call the state dump, the accept
    counters and (B possible, a pass stands).  Chained iterations alternate with everything that voids the pass -- a unit
    call, a stepwise sweep, the hook's write, gph_mcmc_update_gb (gph_engine_part_), a second initialize() -- and with what must
    not void it: one sample of each of the five samplers, gph_engine_check_all, a state dump.  Every byte equals the run
    without the pass and every sweep leaves each generator k steps on.  The second initialize() and the two iterations behind
    it equal a fresh engine's at the same points; gph_mcmc_initialize goes on with the chain above the loci (the control
    stream that samples the start values, the accept counters), with or without the pass, so the fresh engine is given the
    chain state the second initialize() left and initialises its genealogies once, as parity_util's re-initialisation test
    does, and the accept counters are compared as increments."""
    lib = _lib(G, pk193)
    off = U.handover_script(G, lib, pk193, {"GPH_RNG_AHEAD": "0"}, monkeypatch, tmp_path)
    assert all(r["k"] is None for r in off[0])
    U.check_handover(*off, expect_side=0)
    on = U.handover_script(G, lib, pk193, {}, monkeypatch, tmp_path)
    U.check_handover(*on, ref=off[0], expect_side=1)
    place_a = U.handover_script(G, lib, pk193, {"GPH_RNG_AHEAD_PLACE": "A"}, monkeypatch, tmp_path)
    U.check_handover(*place_a, ref=off[0], expect_side=0)
    for a, b in zip(on[0], place_a[0]):
        assert (a["k"] == b["k"]).all(), a["name"]
