"""Site-frequency spectra, data against sampled genealogies (gph_engine_sfs_*) on the CPU: the host-emulation build of the engine
sources runs the workgroup bodies of k_sfs_tree and k_sfs_data, the device text itself, over the same pages and sequence blocks.

The device's E, per-sample rows and data side are held to the definitions of include/gphocs_hip.h by a model that does not use the
kernels' formulas (tests/sfs_util.py): one chain samples its gene trees and its sfs accumulators after every iteration, and plain
Python collects each node's leaf set by climbing father pointers, classifies with sets and sums in the stated order; the data side
comes from the pack's columns with Python sets of bases.  Every double is compared as float.hex, every integer exactly, after 1, 2
and the last sample.

Cases: m3 (3 x 4 leaves), j1 (5 x 2), a7 (an ancient sample: leaf ages), stress (haploid and diploid samples, unequal sizes), x8
(16 x 2 leaves, 496 slots); a hand-made pack with populations of 1, 2, 3 and 4 leaves; two populations of one leaf; 70 synthetic
loci for the edges of the groups of loci."""
import os
import sys

import pytest

from conftest import REPO
from sampler_util import hostemu_library
from test_ancestry import GOLDEN_ITERS
from sfs_util import (check_case, check_chain_untouched, check_group_edges, check_lifecycle, check_model_invariants, check_one_leaf_populations,
                      check_pair_lists, check_pair_times_link, check_phase_rows, check_predictive_link, check_refusals, check_refused_sites,
                      check_small_shapes, locus_data, locus_tree, slot_names, small_model, two_base_loci)

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def small_base(hostemu, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("small"), hostemu[1], "small")


@pytest.fixture(scope="module")
def ones_base(hostemu, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("ones"), hostemu[1], "ones")


# ---------------------------------------------------------------- the model, pinned by itself
def test_model_classifies_a_known_tree_and_known_columns(hostemu):
    """((0, 1), (2, (3, 4))) with populations {0, 2}, {1, 3, 4}: 5 = (0, 1) at 1, 6 = (3, 4) at 2, 7 = (2, 6) at 4, 8 = root at 8; leaf
    3 is an ancient sample of age 0.5.  Slots: sfs_0:1, sfs_1:1, then privP, privQ, shared, fixed of (0, 1).
    Everything below the first assert exercises the Python model alone; that first assert -- the entry points the model describes
    are exported -- is what ties this pin to the feature and makes it fail without it"""
    import gphocs_amd as G
    assert "gph_engine_sfs_enable" in G.EXPORTS and hasattr(hostemu[1], "gph_engine_sfs_enable")   # (what the model describes exists)
    import numpy as np
    members = [frozenset({0, 2}), frozenset({1, 3, 4})]
    slots = [(0, "sfs", 0, 0, 1), (1, "sfs", 1, 1, 1), (2, "privP", 0, 1, 0), (2, "privQ", 0, 1, 0), (2, "shared", 0, 1, 0), (2, "fixed", 0, 1, 0)]
    groups = [("pop", 0), ("pop", 1), ("pair", 0, 1)]
    assert slot_names(slots) == ["sfs_0:1", "sfs_1:1", "privP_0|1", "privQ_0|1", "shared_0|1", "fixed_0|1"]
    age = [0.0, 0.0, 0.0, 0.5, 0.0, 1.0, 2.0, 4.0, 8.0]
    father = [5, 5, 7, 6, 6, 8, 7, 8, -1]
    got = locus_tree(father, age, 5, members, slots, 0.5)
    # branches (length): 0 (1), 1 (1), 2 (4), 3 (1.5), 4 (2), 5 (7), 6 (2), 7 (4)
    # population 0 = {0, 2}: one leaf of the two under 0, 2, 5 (0, 1) and 7 (2, 3, 4): 1 + 4 + 7 + 4
    assert got[0] == (16.0, 8.0)
    # population 1 = {1, 3, 4}: one or two of the three under 1, 3, 4, 5 (1), 6 and 7 (3, 4: folds to 1): 1 + 1.5 + 2 + 7 + 2 + 4
    assert got[1] == (17.5, 8.75)
    # privP: inside 0, none or all of 1: leaves 0 and 2.  privQ: leaves 1, 3, 4 and node 6.  shared: 5 (0 | 1), 7 (2 | 3, 4)
    assert got[2] == (5.0, 2.5) and got[3] == (6.5, 3.25) and got[4] == (11.0, 5.5)
    # fixed: no node holds all of one population and none of the other
    assert got[5] == (0.0, 0.0)
    cols = np.array([[0, 1, 0, 1, 1],     # fixed: 0 shows T, 1 shows C
                     [0, 0, 1, 0, 0],     # private to 0, one carrier
                     [0, 4, 0, 1, 1],     # an N in population 1: it and the pair are unusable, population 0 is monomorphic
                     [0, 1, 1, 2, 1]])    # two bases in each, three across the pair: both spectra, no class
    obs, use, sites = locus_data(cols, [3, 5, 7, 11], members, slots, groups)
    assert sites == 26 and use == [26, 19, 8] and obs == [5 + 11, 11, 5, 0, 0, 3]


# ---------------------------------------------------------------- 1: goldens, bit for bit
@pytest.mark.parametrize("name", ["m3", "j1", "a7", "stress", "x8"])
def test_accumulators_rows_and_observed_equal_the_model(hostemu, name):
    r = check_case(hostemu[1], name)
    pk = r["pack"]
    if name == "m3":
        assert pk.samplesPerPop.tolist()[:pk.Kc] == [4, 4, 4] and len(r["slots"]) == 6 + 12
        assert check_model_invariants(r) >= {"privP", "privQ", "shared", None, 1, 2}
    if name == "j1":
        assert pk.samplesPerPop.tolist()[:pk.Kc] == [2] * 5 and len(r["slots"]) == 5 + 40
    if name == "a7":
        assert pk.samplesPerPop.tolist()[:pk.Kc] == [4, 2, 4] and (r["trees"]["age"][:, :, :pk.n] > 0).any(), "no leaf above age 0"
    if name == "stress":
        assert len(set(pk.samplesPerPop.tolist()[:pk.Kc])) > 1
    if name == "x8":
        assert pk.samplesPerPop.tolist()[:pk.Kc] == [2] * 16 and len(r["slots"]) == 16 + 4 * 120


@pytest.mark.parametrize("name", ["sample", "stress", "bigp"])
def test_counts_do_not_depend_on_the_phase_row_read(hostemu, name):
    check_phase_rows(hostemu[1], name)


# ---------------------------------------------------------------- 2: smallest shapes
def test_populations_of_one_to_four_leaves_and_the_odd_columns(hostemu, small_base):
    check_small_shapes(hostemu[1], small_base)


def test_two_populations_of_one_leaf(hostemu, ones_base):
    check_one_leaf_populations(hostemu[1], ones_base)


def test_groups_of_loci_at_their_edges(hostemu):
    check_group_edges(hostemu[1])


# ---------------------------------------------------------------- 3: invariants across the outputs
def test_spectrum_weighs_to_the_pairwise_differences_of_predictive(hostemu, small_base):
    from mutations_util import phased_pack
    assert check_predictive_link(hostemu[1], phased_pack(small_base, two_base_loci())) >= 9


def test_spectrum_weighs_to_the_pair_times_of_a_population(hostemu):
    check_pair_times_link(hostemu[1])


# ---------------------------------------------------------------- 4: pairs, refusals, limits
def test_explicit_pairs_in_another_order_and_none(hostemu):
    check_pair_lists(hostemu[1])


def test_refusals_name_the_cause_and_touch_nothing(hostemu, capfd, ones_base):
    check_refusals(hostemu[1], capfd, ones_base)


def test_a_locus_of_2_to_the_32_sites_is_refused_by_name(hostemu, capfd, ones_base):
    check_refused_sites(hostemu[1], ones_base, capfd)


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


# ---------------------------------------------------------------- 5: the chain is untouched
@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)


# ---------------------------------------------------------------- 7: the program and the launcher
def test_program_writes_the_two_sfs_files(hostemu, tmp_path):
    from sfs_util import check_program
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def test_ranks_join_to_the_one_rank_files(hostemu, tmp_path):
    from sfs_util import check_ranks
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_sfs_files(hostemu, tmp_path):
    from sfs_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
