"""Triplet topology weights (gph_engine_triplets_*) on the CPU: the host-emulation build of the engine sources runs k_triplets'
workgroup body, the device text itself, over the same pages.

The device's W, A and per-sample rows are held to the definitions of include/gphocs_hip.h by a model that does not use the
kernel's counting formula (tests/triplets_util.py): one chain samples its gene trees and its triplet accumulators after every
iteration, and plain Python enumerates every leaf triple of every population triple over the decoded records, finds the sister
pair by climbing father pointers and groups by its lca.  Every double is compared as float.hex, every integer exactly, after 1,
2 and the last sample; the enumeration itself is held to both invariants (per triple the three counts sum to n_P n_Q n_R).

Cases: m3 (3 x 4 leaves, T = 1: three live slots), j1 (5 x 2 leaves, T = 10), a7 (an ancient sample, 4 / 2 / 4), stress (haploid
and diploid samples, unequal sizes), x8 (16 x 2 leaves, 1 680 slots: more slots than lanes), n7 (72 leaves, counts up to 12^3,
loci 0 and 1) and w139 (20 x 2 leaves, 3 420 slots: the row no longer fits LDS) on the host build with the reference's own caps;
a hand-made pack of one haploid leaf in each of three populations; 70 synthetic loci for the edges of the groups of loci."""
import os
import sys

import pytest

from conftest import REPO
from sampler_util import hostemu_library
from test_ancestry import GOLDEN_ITERS
from triplets_util import (all_triples, check_case, check_chain_untouched, check_group_edges, check_lifecycle, check_minimum, check_refusals,
                           check_triple_lists, locus_sample, min_model, ROW_LDS_SLOTS)

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
def min_pack(hostemu, tmp_path_factory):
    return min_model(tmp_path_factory.mktemp("min"), hostemu[1])


# ---------------------------------------------------------------- the model, pinned by itself
def test_model_counts_a_known_tree():
    """((0, 1), (2, (3, 4))) with populations {0, 2}, {1, 3}, {4}: the four leaf triples by hand"""
    age = [0.0] * 5 + [1.0, 2.0, 4.0, 8.0]
    father = [5, 5, 7, 6, 6, 8, 7, 8, -1]                   # 5 = (0, 1), 6 = (3, 4), 7 = (2, 6), 8 = root (5, 7)
    got = locus_sample(father, age, 5, [[0, 2], [1, 3], [4]], [(0, 1, 2)])
    # (0,1,4): 0,1 sisters at 5;  (0,3,4): 3,4 sisters at 6;  (2,1,4): 2,4 sisters at 7;  (2,3,4): 3,4 sisters at 6
    assert got == [(1, 1.0), (1, 4.0), (2, 4.0)]


# ---------------------------------------------------------------- 1: goldens, bit for bit
@pytest.mark.parametrize("name", ["m3", "j1", "a7", "stress", "x8"])
def test_weights_ages_and_rows_equal_the_enumeration(hostemu, name):
    r = check_case(hostemu[1], name)
    pk = r["pack"]
    if name == "m3":
        assert pk.samplesPerPop.tolist() == [4, 4, 4] and len(all_triples(pk)) == 1
    if name == "j1":
        assert pk.samplesPerPop.tolist() == [2] * 5 and len(all_triples(pk)) == 10
    if name == "a7":
        assert pk.samplesPerPop.tolist() == [4, 2, 4] and (r["trees"]["age"][:, :, :pk.n] > 0).any(), "no leaf above age 0"
    if name == "stress":
        assert len(set(pk.samplesPerPop.tolist())) > 1
    if name == "x8":
        assert pk.samplesPerPop.tolist() == [2] * 16 and 3 * len(all_triples(pk)) == 1680


def test_weights_of_72_leaves(hostemu_big):
    r = check_case(hostemu_big, "n7", loci=[0, 1])
    assert r["pack"].n == 72 and max(r["pack"].samplesPerPop.tolist()) == 12


def test_a_row_too_long_for_lds_is_added_to_directly(hostemu_big):
    """20 current populations, 3 420 slots: beyond the 2 048 a workgroup's row in LDS holds (x8, 1 680, is below)"""
    r = check_case(hostemu_big, "w139", iters=3)
    assert 3 * len(all_triples(r["pack"])) == 3420 > ROW_LDS_SLOTS >= 1680


def test_one_leaf_in_each_of_three_populations(hostemu, min_pack):
    check_minimum(hostemu[1], min_pack)


# ---------------------------------------------------------------- 2: group edges, selections, refusals, limits
def test_groups_of_loci_at_their_edges(hostemu):
    check_group_edges(hostemu[1])


def test_explicit_triples_in_another_order(hostemu):
    check_triple_lists(hostemu[1])


def test_refusals_name_the_cause_and_touch_nothing(hostemu, capfd, tmp_path):
    from predictive_util import edge_model
    check_refusals(hostemu[1], capfd, edge_model(tmp_path, hostemu[1]))


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


# ---------------------------------------------------------------- 3: the chain is untouched
@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    on, off = check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


# ---------------------------------------------------------------- 4: the program and the launcher
def test_program_writes_the_two_triplets_files(hostemu, tmp_path):
    from triplets_util import check_program
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def test_ranks_join_to_the_one_rank_files(hostemu, tmp_path):
    from triplets_util import check_ranks
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_triplets_files(hostemu, tmp_path):
    from triplets_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
