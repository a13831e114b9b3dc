"""The sweep's draws ahead (k_rng_ahead + GphRngA) against a generator written a second time (tests/rng_ahead_util.py), on
the host-emulation build: every byte of the pass's buffers for counts that differ from locus to locus, and where the sweep
leaves each locus's generator.  Everything is exact: 32-bit integers and IEEE doubles compared as bit patterns.
tests/test_rng_ahead_stream_gpu.py runs the same bodies on the device."""
import os
import sys

import numpy as np
import pytest

import rng_ahead_util as U
from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))


@pytest.fixture(scope="module")
def G():
    import gphocs_amd as G
    return G


@pytest.fixture(scope="module")
def lib(G):
    import run_hostemu as R
    return G.load_library(R.build_hostemu())


@pytest.mark.parametrize("seed", [12345, 777])
def test_independent_generator_reproduces_the_reference_stream(seed):
    """the restatement itself, before it is used on the engine: the 300 uniforms of tests/golden/rng_<seed>.txt (the table
    tests/test_oracle_vs_reference.py::test_rng_stream pins the oracle's rndu with) and the state they end in (line `X`)"""
    lines = open(os.path.join(GOLDEN, f"rng_{seed}.txt")).read().split("\n")
    want = np.array([float.fromhex(ln.split()[1]) for ln in lines[:300]])
    assert all(ln.startswith("U ") for ln in lines[:300]) and not lines[300].startswith("U ")
    end = [int(v) for v in [ln for ln in lines if ln.startswith("X ")][0].split()[1:4]]
    S0 = np.array([[11, 23, 170 * (seed % 178) + 137]], dtype=np.uint32)
    states, draws = U.stream(S0, 300)
    assert (draws[:, 0] == want.view(np.uint64)).all()
    assert states[300, 0].tolist() == end
    # a step keeps no more than 32 bits, whatever the state
    big = U.step(np.array([[0xFFFFFFFF, 0xFFFFFFFE, 0x80000000]], dtype=np.uint64))
    assert big.tolist() == [[(171 * 0xFFFFFFFF - 30269 * (0xFFFFFFFF // 177)) % 2**32, (172 * 0xFFFFFFFE - 30307 * (0xFFFFFFFE // 176)) % 2**32,
                             (170 * 0x80000000 - 30323 * (0x80000000 // 178)) % 2**32]]


def test_helpers():
    assert U.n_ahead([-64, -1, 0, 1, 63, 64, 65, 448, 449, 1 << 20], 512).tolist() == [0, 64, 64, 128, 128, 128, 192, 512, 512, 512]
    assert U.n_ahead([448, 449, 960, 1023], 1024).tolist() == [512, 576, 1024, 1024]
    d = b"ITER 3\nLOCUS 7 root 22 dataLnL -0x1p+8 genLnL 0x1p+7 rng 4246994186 3582554523 1\nN 0\nLOCUS 8 root 1 dataLnL 0x0p+0 genLnL 0x0p+0 rng 1 2 3\n"
    assert U.parse_rng(d).tolist() == [[4246994186, 3582554523, 1], [1, 2, 3]]
    for case in U.PASS_CASES:
        M, _, ns = U.expected_n(case)
        assert {0, 64, M} <= ns and (M != 512 or ns == set(range(0, 513, 64))), case


def test_fetch_on_the_host_build(G, lib, monkeypatch, tmp_path):
    """gph_engine_rng_ahead_fetch_: refused with the pass off; in input order, although the slots are sorted by pattern count;
    reading changes nothing"""
    pk = U.synthetic_pack(G, 4, 193, 26.0)
    U.set_env(monkeypatch, {"GPH_RNG_AHEAD": "0"})
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    assert U._fetch_fn(lib)(s.engine, None, None, None) == U.GPH_ESTATE
    s.close()
    U.set_env(monkeypatch, {})
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    S0 = U.parse_rng(U.dump(s, tmp_path / "s"))
    P = np.diff(pk.pattern_offsets)
    assert (np.argsort(-P, kind="stable") != np.arange(len(P))).any(), "this data set was meant to have its loci reordered into slots"
    U.sweep(s)
    draws, ckpt, tail = U.fetch(s)
    assert draws.shape == (193, 512) and ckpt.shape == (193, 33, 4) and tail.shape == (193, 4)
    assert (ckpt[:, 0, :3] == S0).all() and (tail[:, 3] == 320).all()       # the first sweep: 320 draws from the state initialize() left
    again = U.fetch(s)
    assert all((a == b).all() for a, b in zip((draws, ckpt, tail), again))
    s.close()


@pytest.mark.parametrize("case", list(U.PASS_CASES))
def test_pass_against_the_independent_generator(G, lib, case, monkeypatch, tmp_path):
    loci, mut, env, vals = U.PASS_CASES[case]
    M, Cd, ns = U.expected_n(case)
    got = U.check_pass(G, lib, U.synthetic_pack(G, 4, loci, mut), env, vals, monkeypatch, tmp_path)
    assert got[:2] == (M, Cd)
    if loci >= len(vals):
        assert got[2] == ns


@pytest.fixture(scope="module")
def plain(G, lib, tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        pk = U.synthetic_pack(G, 4, 193, 26.0)
        return pk, U.first_sweep(G, lib, pk, mp, tmp_path_factory.mktemp("plain"))
    finally:
        mp.undo()


@pytest.mark.parametrize("edge", ["a", "b", "c"])
def test_counts_forced_onto_the_chunk_edges(G, lib, plain, edge, monkeypatch, tmp_path):
    """the host form of tests/test_rng_ahead_stream_gpu.py's edge test (there: what each edge is).  The first sweep's counts put
    13 / 12 / 10 loci on the residues 0 / 1 / 63 of 64"""
    pk, ref = plain
    assert U.check_edge_residues(ref["k"]) == [13, 12, 10]
    U.check_forced(ref, U.first_sweep(G, lib, pk, monkeypatch, tmp_path, U.edge_counts(ref["k"])[edge]), edge)


def test_a_sweep_that_draws_nothing(G, lib, monkeypatch, tmp_path):
    """k = 0 (rng_ahead_util.check_no_draws): the synthetic model without migration bands is synth.CONFIGS[2]"""
    U.check_no_draws(G, lib, U.synthetic_pack(G, 2, 65, 6.5), monkeypatch, tmp_path)


def test_hand_over_script_on_the_host_build(G, lib, monkeypatch, tmp_path):
    """the calls of the device's hand-over test where no pass ever runs behind a sweep (the host build decides on the host):
    the script is legal, the pass changes no byte of it, and every sweep leaves the generators where its counts say"""
    pk = U.synthetic_pack(G, 4, 193, 26.0)
    off = U.handover_script(G, lib, pk, {"GPH_RNG_AHEAD": "0"}, monkeypatch, tmp_path)
    U.check_handover(*off)
    on = U.handover_script(G, lib, pk, {}, monkeypatch, tmp_path)
    assert all(r["k"] is not None for r in on[0])
    U.check_handover(*on, ref=off[0], expect_side=0)
