"""The cross-locus reduction kernel k_reduce_stage on the MI355X, directly (-m gpu): the bodies of reduce_util.py through the
product libraries -- the 128-column rows of variant `s` and the 384-column rows of the many-band variant `b`, whose statistics
are folded in windows of 128 columns.  On top of what test_reduce.py checks on the host build, the sums are held bit for bit to
the numpy restatement of the documented shape (reduce_util.shape_model), one launch and six back to back, and the bound of the
comparison with math.fsum is the shape's longest addition path instead of L.

Then the engine's own rows at wide columns and many loci: goldens of the big models replicated past 2 048 loci (chunk 9: a second
step of every sub-sequence, empty blocks at the tail), three iterations against the oracle run live.  Replicas of a locus are
identical, so that part cannot see a permutation -- the probe can; it shows that the engine's statistics stride and column count
reach the kernel as the probe assumes."""
import os
import subprocess
import time

import pytest

from parity_util import compare_records, compare_states
import reduce_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.fixture(scope="module")
def lib128(G):
    lib = G.load_library(dims=U.DIMS_128)
    assert U.constants(lib).cols == 128
    return lib


@pytest.fixture(scope="module")
def lib384(G):
    lib = G.load_library(dims=U.DIMS_384)
    assert U.constants(lib).cols == 384
    return lib


def test_constants(lib128, lib384):
    for i in (U.constants(lib128), U.constants(lib384)):
        assert i.stride == 3 * i.cols + 8 and i.row == 2 * i.stride and i.ticket == 0
        assert i.subs > 0 and i.blocks % i.subs == 0 and i.unroll > 0
        # the second unroll trip of section 0 (16 columns: the largest Q) needs a chunk above unroll * Q: 131 073 loci have it;
        # 2 049 give a second step at the smallest Q and leave blocks empty at the tail
        assert U.chunk_of(i, max(U.LOCI_LARGE)) > i.unroll * U.subsequences(i, i.out_slots)
        assert U.chunk_of(i, 2049) > U.subsequences(i, 128) and 2049 <= (i.blocks - 1) * U.chunk_of(i, 2049)


def test_refusals(lib128, lib384):
    U.check_refusals(lib128)
    U.check_refusals(lib384)


@pytest.mark.parametrize("ncols", U.WIDTHS_0)
def test_section_0(lib128, ncols):
    print(f"section 0, {ncols} columns: worst |row - fsum| / bound {U.check_width(lib128, 0, ncols, 1000 + ncols, model=True):.3f}")


@pytest.mark.parametrize("ncols", U.WIDTHS_128)
def test_section_1(lib128, ncols):
    print(f"section 1, {ncols} columns: worst |row - fsum| / bound {U.check_width(lib128, 1, ncols, 2000 + ncols, model=True):.3f}")


@pytest.mark.parametrize("ncols", U.WIDTHS_384)
def test_section_1_windows(lib384, ncols):
    print(f"section 1, {ncols} columns: worst |row - fsum| / bound {U.check_width(lib384, 1, ncols, 3000 + ncols, model=True):.3f}")


@pytest.mark.parametrize("ncols", (16, 26))
def test_section_1_narrow_on_the_wide_rows(lib384, ncols):
    """the cw 16 and 32 paths with the partials of a 384-column row (the row's width is the partials' stride)"""
    U.check_width(lib384, 1, ncols, 3500 + ncols, model=True, loci=(257, 2049))


# the large counts, two tests a case: the references (36 million numbers through math.fsum at the largest) take a second or two each
@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_128)
def test_many_loci_sums(lib128, sec, ncols, L):
    r = U.check_floats(lib128, sec, ncols, L, 4001 + L, model=True)
    print(f"section {sec}, {ncols} columns, {L} loci: worst |row - fsum| / bound {r:.3f}")


@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_128)
def test_many_loci_integers_and_extremes(lib128, sec, ncols, L):
    U.check_integers(lib128, sec, ncols, L, 4000 + L)
    U.check_extremes(lib128, sec, ncols, L, 4002 + L)


@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_384)
def test_many_loci_sums_windows(lib384, sec, ncols, L):
    r = U.check_floats(lib384, sec, ncols, L, 5001 + L, model=True)
    print(f"section {sec}, {ncols} columns, {L} loci: worst |row - fsum| / bound {r:.3f}")


@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_384)
def test_many_loci_integers_and_extremes_windows(lib384, sec, ncols, L):
    U.check_integers(lib384, sec, ncols, L, 5000 + L)
    U.check_extremes(lib384, sec, ncols, L, 5002 + L)


@pytest.mark.parametrize("sec,ncols", U.LARGE_128)
def test_back_to_back_at_many_loci(lib128, sec, ncols):
    U.check_back_to_back(lib128, sec, ncols, 32769, 7000 + ncols, model=True)


def test_back_to_back_at_many_loci_windows(lib384):
    U.check_back_to_back(lib384, 1, 278, 32769, 7278, model=True)


@pytest.mark.parametrize("ncols", (16, 26, 64, 110))
def test_both_sections_in_one_launch(lib128, ncols):
    for L in (1, 257, 2049, 32769):
        U.check_fused(lib128, ncols, L, 6000 + L)


def test_both_sections_in_one_launch_windows(lib384):
    for L in (257, 2049, 32769):
        U.check_fused(lib384, 278, L, 6100 + L)


# ---------------------------------------------------------------- the engine's own rows at wide columns and many loci
# golden: (library variant, statistics columns 2K + 2B: b2 and x8 take the cw 64 path -- b2 with the partials of a 384-column
# row -- and y9 the two-columns-a-lane path).  The oracle's three iterations on one CPU core, measured: b2 0.08 s at 300 loci and
# 0.47 s at 2 100, x8 0.21 s and 1.63 s, y9 0.35 s and 2.69 s
ENGINE_CASES = {"b2": ("b", 62), "x8": ("x", 94), "y9": ("h", 110)}
ENGINE_LOCI = (300, 2100)
ENGINE_ITERS = 3


@pytest.mark.parametrize("L", ENGINE_LOCI)
@pytest.mark.parametrize("case", sorted(ENGINE_CASES))
def test_engine_rows_against_live_oracle(G, case, L, oracle_cli, tmp_path):
    from conftest import GOLDEN
    from gphocs_amd_pkg import synth
    base = G.Pack.load(os.path.join(GOLDEN, case + ".gpk"))
    pk = G.replicate_pack(G.Pack, base, L)
    assert pk.L == L and (G.variant_for(pk.n, pk.K, pk.B), 2 * pk.K + 2 * pk.B) == ENGINE_CASES[case]
    pth = str(tmp_path / "p.gpk")
    synth.write_pack(pk, pth)
    mine, theirs = str(tmp_path / "hip.rec"), str(tmp_path / "oracle.rec")
    t0 = time.time()
    s = G.Sampler(G.Pack.load(pth), lib=G.load_library(dims=(pk.n, pk.K, pk.B)))
    s.set_record_file(mine)
    s.initialize()
    for it in range(ENGINE_ITERS):
        s.iteration(it)
    s.dump_state(mine + ".state", False)
    s.set_record_file(None)
    s.close()
    t1 = time.time()
    subprocess.run([oracle_cli, "run", pth, str(ENGINE_ITERS), theirs, theirs + ".state", str(ENGINE_ITERS - 1), "0"], check=True, timeout=300)
    t2 = time.time()
    worst = compare_records(mine, theirs)
    compare_states(mine + ".state", theirs + ".state")
    assert sum(1 for l in open(mine + ".state") if l.startswith("LOCUS ")) == L
    print(f"{case} x {L} loci, {2 * pk.K + 2 * pk.B} statistics columns: engine {t1 - t0:.2f} s, oracle {t2 - t1:.2f} s, "
          f"worst accumulator rel diff {worst:.3e}")
