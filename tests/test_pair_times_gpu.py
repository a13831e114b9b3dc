"""Pairwise coalescence-time distributions on the MI355X (-m gpu): k_pair_times in the product libraries, with the tightest
capacity variant per case, held to what tests/test_pair_times.py holds the host build to -- A, Y, X, M EQUAL, as float.hex, to the
enumeration of leaf pairs over the same chain's gene-tree records and population ages, every per-sample row as integers, after 1,
2 and the last sample; the hand-made minimums; edges that are ages; the edges of the groups of loci; explicit pairs; the
invariants; refusals; reset and limits; the chain's trajectory unchanged by sampling -- plus the engine's host synchronisations
and the checked build's index checks."""
import os

import pytest

from test_ancestry import GOLDEN_ITERS
from pair_times_util import (check_case, check_chain_untouched, check_edges_that_are_ages, check_group_edges, check_lifecycle,
                             check_no_band_no_young_coalescence, check_one_population, check_pair_lists, check_refusals, check_two_populations,
                             check_young_coalescence_needs_a_migration, grid, small_model)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.fixture(scope="module")
def two_pack(G, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("min"), G.load_library(dims=(2, 3, 0)), "two")


@pytest.fixture(scope="module")
def one_pack(G, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("min"), G.load_library(dims=(2, 1, 0)), "one")


@pytest.mark.parametrize("name", ["m3", "j1", "a7", "stress", "x8"])
def test_device_accumulators_and_rows_equal_the_enumeration(G, name):
    check_case(None, name, key="gpu")


def test_x8_with_a_row_that_fits_lds(G):
    check_case(None, "x8", iters=3, edges=grid(1e-5, 1e-2, 10), key="gpu")


def test_device_distributions_of_72_leaves(G):
    check_case(None, "n7", loci=[0, 1], key="gpu")


def test_a_row_too_long_for_lds_is_added_to_directly(G):
    check_case(None, "w139", iters=3, key="gpu")


def test_two_populations_of_one_leaf(G, two_pack):
    check_two_populations(None, two_pack)


def test_one_population_with_two_leaves(G, one_pack):
    check_one_population(None, one_pack)


def test_edges_that_are_ages(G):
    check_edges_that_are_ages(None)


def test_groups_of_loci_at_their_edges(G):
    check_group_edges(None)


def test_explicit_pairs_in_another_order(G):
    check_pair_lists(None)


@pytest.mark.parametrize("name", ["g2", "v9"])
def test_without_a_band_nothing_coalesces_below_a_split(G, name):
    check_no_band_no_young_coalescence(None, name)


def test_a_coalescence_below_the_split_needs_a_migration(G):
    check_young_coalescence_needs_a_migration(None)


def test_refusals_name_the_cause_and_touch_nothing(G, capfd, two_pack):
    check_refusals(None, capfd, two_pack)


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)


def test_checked_build_reports_no_index_violation(G, two_pack):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    assert check_case(lib, "m3")["oob"] == (0, 1)
    assert check_two_populations(lib, two_pack)["oob"] == (0, 1)


def test_program_writes_the_two_pair_times_files(G, tmp_path):
    from pair_times_util import check_program
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_join_to_the_one_rank_files(G, tmp_path):
    from pair_times_util import check_ranks
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_pair_times_files(G, tmp_path):
    from pair_times_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(None, tmp_path)
