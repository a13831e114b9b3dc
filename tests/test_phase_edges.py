"""Phase integration at the edges of its groups, and the boundary that says which phase words are legal (CPU: the host builds of
tests/hostemu).

The packs of phase_edges_util.py -- a golden's model over made-up loci whose groups of phases are 32 and 64 rows long, end in the
wave's last lane, end at the last row of a shorter locus, straddle row 64 of a wide one, have counts that are no power of two --
run against the oracle run live on the same pack (counters exact, sums over loci <= 1e-10 relative, the final state with the
conditionals field by field: parity_util's own bar) and against model_lnl(), the likelihood of the final gene trees in 60-digit
decimal arithmetic (<= 1e-10 relative per locus, a cap: the deviations measured are printed and stand in the docstrings).

gph_engine_load_loci refuses what is no phase layout, before anything is allocated, and names the locus (test_refused_*)."""
import copy
import os
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import compare_records, compare_states
import phase_edges_util as U

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

BUILDS = {"default": dict(), "mid": dict(mid=True), "big": dict(big=True), "wave64": dict(wave64=True)}
# id: (host build, model, layout that becomes locus 0, a count of 70000, iterations)
CASES = {
    "default-m3": ("default", "m3", 0, False, 30),
    "default-v8-ref64": ("default", "v8", U.I_64, False, 30),       # locus-mut-rate VAR: locus 0 is the scan's reference locus, the only
    "default-v8-ref63": ("default", "v8", U.I_P63, False, 30),      # route into lr_ref_eval: [64], and P = 63 with a group of 32
    "default-x8": ("default", "x8", 0, True, 24),                    # 32 leaves; the 32-bit count form without GPH_CNT16
    "mid-y9": ("mid", "y9", 0, False, 30),                           # the list-driven form, 40 leaves
    "big-n7": ("big", "n7", 0, False, 20),                           # the list-driven form, 72 leaves
    "wave64-m3": ("wave64", "m3", 0, False, 6),                     # the device forms on the 64-lane fiber wave
}
_libs, _runs = {}, {}


def library(build):
    if build not in _libs:
        import run_hostemu
        import gphocs_amd as G
        _libs[build] = G.load_library(run_hostemu.build_hostemu(**BUILDS[build]))
    return _libs[build]


def chain(case, oracle_cli, tmp_path_factory):
    """engine and oracle, once per case"""
    if case not in _runs:
        import gphocs_amd as G
        from gphocs_amd_pkg import synth
        build, base, first, big_count, iters = CASES[case]
        d = tmp_path_factory.mktemp(case)
        pack = U.narrow_pack(base, big_count=big_count, first=first)
        path = str(d / "pack.gpk")
        synth.write_pack(pack, path)
        f = {k: str(d / k) for k in ("e.trace", "e.state", "o.trace", "o.state")}
        t0 = time.time()
        r = U.run(G, library(build), G.Pack.load(path), iters, f["e.trace"], f["e.state"])
        t1 = time.time()
        U.run_oracle(oracle_cli, path, iters, f["o.trace"], f["o.state"])
        print(f"{case}: engine {t1 - t0:.2f} s, oracle {time.time() - t1:.2f} s")
        _runs[case] = dict(pack=pack, iters=iters, r=r, files=f)
    return _runs[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_pack_holds_the_edges_and_the_chain_moves(case, oracle_cli, tmp_path_factory):
    c = chain(case, oracle_cli, tmp_path_factory)
    pack = c["pack"]
    U.covered(pack, c["iters"], c["r"], U.kinds_for(pack))
    build, base, first, big_count, _ = CASES[case]
    assert pack.layouts[0] == U.NARROW[first]
    assert (int(pack.counts.max()) == 70000) == big_count
    assert c["r"]["oob"][0] == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_live_oracle(case, oracle_cli, tmp_path_factory):
    f = chain(case, oracle_cli, tmp_path_factory)["files"]
    worst = compare_records(f["e.trace"], f["o.trace"])
    compare_states(f["e.state"], f["o.state"])
    print(f"{case}: worst accumulator deviation {worst:.3e}")


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_decimal_model(case, oracle_cli, tmp_path_factory):
    """largest |engine - model| / |model| over the loci after the last iteration, as measured on the host builds:
    default-m3 1.5e-15, default-v8-ref64 1.6e-15, default-v8-ref63 1.4e-14, default-x8 3.0e-15, mid-y9 1.1e-14, big-n7 3.3e-14,
    wave64-m3 (6 iterations) 1.8e-14"""
    c = chain(case, oracle_cli, tmp_path_factory)
    worst = U.model_deviation(c["pack"], c["r"])
    print(f"{case}: largest deviation from the decimal model {worst:.3e}")
    assert worst <= U.MODEL_TOL


def test_groups_of_2_to_the_14_and_15(oracle_cli, tmp_path):
    """phase words 16384 (the largest plain count) and 0x8000 | 15 (the smallest encoded one) on the wide path, three iterations;
    the decimal model on the final trees: 5.6e-14 measured"""
    import gphocs_amd as G
    from gphocs_amd_pkg import synth
    pack = U.huge_pack()
    assert sorted(set(pack.numPhases.tolist()))[-2:] == [16384, 0x8000 | 15]
    path = str(tmp_path / "k15.gpk")
    synth.write_pack(pack, path)
    f = {k: str(tmp_path / k) for k in ("e.trace", "e.state", "o.trace", "o.state")}
    r = U.run(G, library("default"), G.Pack.load(path), 3, f["e.trace"], f["e.state"], with_cond=False)
    U.run_oracle(oracle_cli, path, 3, f["o.trace"], f["o.state"], with_cond=False)
    compare_records(f["e.trace"], f["o.trace"])
    compare_states(f["e.state"], f["o.state"])
    worst = U.model_deviation(pack, r)
    print(f"2^14 / 2^15: largest deviation from the decimal model {worst:.3e}")
    assert worst <= U.MODEL_TOL


# ---------------------------------------------------------------- the load boundary
MALFORMED = sorted(U.malformed(U.m3()))


@pytest.mark.parametrize("what", MALFORMED)
def test_refused_with_the_locus_named(what, capfd):
    p = U.m3()
    locus, pattern, code, change = U.malformed(p)[what]
    q = copy.deepcopy(p)
    change(q)
    U.check_refusal(library("default"), q, capfd, locus, code, pattern)


def test_refused_by_size_before_a_row_is_read(capfd):
    """8 (n - 1) P >= 2^31: the offsets of the second locus claim 2^25 rows at 12 leaves, the arrays hold m3's few hundred --
    the sizes are judged from the offsets alone, so neither the rows nor the memory are needed.  (The other size rule, a sequence
    block of 2^31 bytes, binds first only for n = 1: 8 (n - 1) P grows faster for every n >= 2.)"""
    p = U.m3()
    assert 8 * (p.n - 1) * ((1 << 25) - 1) >= 1 << 31
    U.check_refusal(library("default"), U.oversized(p), capfd, 1, -101)
    # the largest locus that passes the rule is judged by its rows again
    q = U.oversized(p, ((1 << 31) - 1) // (8 * (p.n - 1)))
    q.numPhases[int(q.pattern_offsets[1])] = 0
    U.check_refusal(library("default"), q, capfd, 1, -103, 0)


def test_a_valid_engine_runs_after_refusals(capfd):
    """the refusals leave nothing behind: in the same process, after all of them, m3 still gives its golden's records"""
    import tempfile
    import gphocs_amd as G
    p = U.m3()
    lib = library("default")
    for what in MALFORMED:
        locus, pattern, code, change = U.malformed(p)[what]
        q = copy.deepcopy(p)
        change(q)
        U.check_refusal(lib, q, capfd, locus, code, pattern)
    with tempfile.TemporaryDirectory() as td:
        tr = os.path.join(td, "t")
        s = G.Sampler(p, lib=lib)
        assert s.last_error() == (-1, 0) and lib.gph_engine_last_error_text(s.engine) == b""
        s.set_record_file(tr)
        s.initialize()
        for it in range(120):
            s.iteration(it)
        s.set_record_file(None)
        s.close()
        compare_records(tr, os.path.join(GOLDEN, "m3.rtrace"))
