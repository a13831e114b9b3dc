"""Pairwise coalescence-time distributions (gph_engine_pair_times_*) on the CPU: the host-emulation build of the engine sources
runs k_pair_times' workgroup body, the device text itself, over the same pages.

The device's A, Y, X, M and per-sample rows are held to the definitions of include/gphocs_hip.h by a model that does not use the
kernel's counting formula (tests/pair_times_util.py): one chain samples its gene trees, its population ages and its pair-times
accumulators after every iteration, and plain Python enumerates every leaf pair of every slot over the decoded records, finds the
lca by climbing father pointers and groups by it.  Every double is compared as float.hex, every integer exactly, after 1, 2 and
the last sample; the enumeration itself is held to both invariants (sum of a histogram = m_PQ, y <= m_PQ).

Cases: m3 (3 x 4 leaves, 6 slots), j1 (5 x 2 leaves, 15 slots), a7 (an ancient sample, 4 / 2 / 4), stress (haploid and diploid
samples, unequal sizes), x8 (16 x 2 leaves, 136 slots, 4 896 numbers a row: added to directly), n7 (72 leaves, loci 0 and 1) and
w139 (20 x 2 leaves under 39 populations, 210 slots: the row no longer fits LDS) on the host build with the reference's own caps;
two hand-made packs of two leaves; 70 synthetic loci for the edges of the groups of loci."""
import os
import sys

import pytest

from conftest import REPO
from sampler_util import hostemu_library
from test_ancestry import GOLDEN_ITERS
from pair_times_util import (EDGES, ROW_LDS_WORDS, all_pairs, bin_of, check_case, check_chain_untouched, check_edges_that_are_ages, check_group_edges,
                             check_lifecycle, check_no_band_no_young_coalescence, check_one_population, check_pair_lists, check_refusals,
                             check_two_populations, check_young_coalescence_needs_a_migration, grid, locus_sample, small_model, split_of)

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


@pytest.fixture(scope="module")
def two_pack(hostemu, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("min"), hostemu[1], "two")


@pytest.fixture(scope="module")
def one_pack(hostemu, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("min"), hostemu[1], "one")


# ---------------------------------------------------------------- the model, pinned by itself
def test_model_counts_a_known_tree():
    """((0, 1), (2, (3, 4))) with populations {0, 2}, {1, 3}, {4}; edges 2 and 4; splits 3 for (0, 1), inf for (0, 0), 1 for (1, 2)"""
    age = [0.0] * 5 + [1.0, 2.0, 4.0, 8.0]
    father = [5, 5, 7, 6, 6, 8, 7, 8, -1]                   # 5 = (0, 1), 6 = (3, 4), 7 = (2, 6), 8 = root (5, 7)
    got = locus_sample(father, age, 5, [[0, 2], [1, 3], [4]], [(0, 1), (0, 0), (1, 2)], [2.0, 4.0], [3.0, float("inf"), 1.0])
    # (0, 1): 0-1 at 5 (age 1), 0-3 at 8, 2-1 at 8, 2-3 at 7 (age 4: the edge itself, upper bin)
    assert got[0] == ([1, 0, 3], 1.0 + 4.0 + 16.0, 1, 1, 1.0)
    # (0, 0): 0-2 at the root
    assert got[1] == ([0, 0, 1], 8.0, 1, 1, 8.0)
    # (1, 2): 1-4 at the root, 3-4 at 6 (age 2: the edge itself); none below the split 1
    assert got[2] == ([0, 1, 1], 2.0 + 8.0, 0, 0, 2.0)


def test_model_split_and_bins():
    pf, pa = [3, 3, 4, 4, -1], [0.0, 0.0, 0.0, 0.5, 0.75]
    assert split_of(pa, pf, 0, 1) == 0.5 and split_of(pa, pf, 0, 2) == 0.75 and split_of(pa, pf, 2, 2) == 0.75 and split_of(pa, pf, 1, 1) == 0.5
    assert split_of([0.0], [-1], 0, 0) == float("inf")
    assert [bin_of([1.0, 2.0], a) for a in (0.0, 0.999, 1.0, 1.5, 2.0, 9.0)] == [0, 0, 1, 1, 2, 2]
    e = grid(1e-6, 1e-2, 34)
    assert len(e) == 33 and e[0] == 1e-6 and e[-1] == 1e-2 and all(a < b for a, b in zip(e, e[1:])) and e == EDGES


# ---------------------------------------------------------------- 1: goldens, bit for bit
@pytest.mark.parametrize("name", ["m3", "j1", "a7", "stress", "x8"])
def test_accumulators_and_rows_equal_the_enumeration(hostemu, name):
    r = check_case(hostemu[1], name)
    pk = r["pack"]
    words = len(all_pairs(pk)) * (len(EDGES) + 3)
    if name == "m3":
        assert pk.samplesPerPop.tolist() == [4, 4, 4] and len(all_pairs(pk)) == 6 and words <= ROW_LDS_WORDS
    if name == "j1":
        assert pk.samplesPerPop.tolist() == [2] * 5 and len(all_pairs(pk)) == 15 and words <= ROW_LDS_WORDS
    if name == "a7":
        assert pk.samplesPerPop.tolist() == [4, 2, 4] and (r["trees"]["age"][:, :, :pk.n] > 0).any(), "no leaf above age 0"
    if name == "stress":
        assert len(set(pk.samplesPerPop.tolist())) > 1
    if name == "x8":
        assert pk.samplesPerPop.tolist() == [2] * 16 and len(all_pairs(pk)) == 136 and words > ROW_LDS_WORDS


def test_x8_with_a_row_that_fits_lds(hostemu):
    """136 slots x (10 + 2) = 1 632 numbers: x8's many slots through the LDS row as well"""
    r = check_case(hostemu[1], "x8", iters=3, edges=grid(1e-5, 1e-2, 10))
    assert len(all_pairs(r["pack"])) * 12 <= ROW_LDS_WORDS


def test_distributions_of_72_leaves(hostemu_big):
    r = check_case(hostemu_big, "n7", loci=[0, 1])
    assert r["pack"].n == 72 and max(r["pack"].samplesPerPop.tolist()) == 12


def test_a_row_too_long_for_lds_is_added_to_directly(hostemu_big):
    """39 populations, 20 of them current: 210 slots x 36 numbers, beyond the 2 048 a workgroup's row in LDS holds"""
    r = check_case(hostemu_big, "w139", iters=3)
    assert r["pack"].K == 39 and len(all_pairs(r["pack"])) * (len(EDGES) + 3) == 7560 > ROW_LDS_WORDS


def test_two_populations_of_one_leaf(hostemu, two_pack):
    check_two_populations(hostemu[1], two_pack)


def test_one_population_with_two_leaves(hostemu, one_pack):
    check_one_population(hostemu[1], one_pack)


def test_edges_that_are_ages(hostemu):
    check_edges_that_are_ages(hostemu[1])


# ---------------------------------------------------------------- 2: group edges, pairs, invariants, refusals, limits
def test_groups_of_loci_at_their_edges(hostemu):
    check_group_edges(hostemu[1])


def test_explicit_pairs_in_another_order(hostemu):
    check_pair_lists(hostemu[1])


@pytest.mark.parametrize("name", ["g2", "v9"])
def test_without_a_band_nothing_coalesces_below_a_split(hostemu, name):
    check_no_band_no_young_coalescence(hostemu[1], name)


def test_a_coalescence_below_the_split_needs_a_migration(hostemu):
    check_young_coalescence_needs_a_migration(hostemu[1])


def test_refusals_name_the_cause_and_touch_nothing(hostemu, capfd, two_pack):
    check_refusals(hostemu[1], capfd, two_pack)


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


# ---------------------------------------------------------------- 3: the chain is untouched
@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)


# ---------------------------------------------------------------- 4: the program and the launcher
def test_program_writes_the_two_pair_times_files(hostemu, tmp_path):
    from pair_times_util import check_program
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def test_ranks_join_to_the_one_rank_files(hostemu, tmp_path):
    from pair_times_util import check_ranks
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_pair_times_files(hostemu, tmp_path):
    from pair_times_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
