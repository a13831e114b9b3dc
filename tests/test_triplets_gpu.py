"""Triplet topology weights on the MI355X (-m gpu): k_triplets in the product libraries, with the tightest capacity variant per
case, held to what tests/test_triplets.py holds the host build to -- W and A EQUAL, as float.hex, to the enumeration of leaf
triples over the same chain's gene-tree records, every per-sample row as integers, after 1, 2 and the last sample; the hand-made
minimum; the edges of the groups of loci; explicit triples; refusals; reset and limits; the chain's trajectory unchanged by
sampling -- plus the engine's host synchronisations and the checked build's index checks."""
import os

import pytest

from test_ancestry import GOLDEN_ITERS
from triplets_util import (check_case, check_chain_untouched, check_group_edges, check_lifecycle, check_minimum, check_refusals, check_triple_lists,
                           min_model)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.fixture(scope="module")
def min_pack(G, tmp_path_factory):
    return min_model(tmp_path_factory.mktemp("min"), G.load_library(dims=(3, 5, 0)))


@pytest.mark.parametrize("name", ["m3", "j1", "a7", "stress", "x8"])
def test_device_weights_ages_and_rows_equal_the_enumeration(G, name):
    check_case(None, name, key="gpu")


def test_device_weights_of_72_leaves(G):
    check_case(None, "n7", loci=[0, 1], key="gpu")


def test_a_row_too_long_for_lds_is_added_to_directly(G):
    check_case(None, "w139", iters=3, key="gpu")


def test_one_leaf_in_each_of_three_populations(G, min_pack):
    check_minimum(None, min_pack)


def test_groups_of_loci_at_their_edges(G):
    check_group_edges(None)


def test_explicit_triples_in_another_order(G):
    check_triple_lists(None)


def test_refusals_name_the_cause_and_touch_nothing(G, capfd, tmp_path):
    from predictive_util import edge_model
    check_refusals(None, capfd, edge_model(tmp_path, G.load_library(dims=(4, 3, 0))))


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    on, off = check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


def test_checked_build_reports_no_index_violation(G, min_pack):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    assert check_case(lib, "m3")["oob"] == (0, 1)
    assert check_minimum(lib, min_pack)["oob"] == (0, 1)


def test_program_writes_the_two_triplets_files(G, tmp_path):
    from triplets_util import check_program
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_join_to_the_one_rank_files(G, tmp_path):
    from triplets_util import check_ranks
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_triplets_files(G, tmp_path):
    from triplets_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(None, tmp_path)
