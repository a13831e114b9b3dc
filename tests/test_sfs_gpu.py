"""Site-frequency spectra on the MI355X (-m gpu): k_sfs_tree and k_sfs_data in the product libraries, with the tightest capacity
variant per case, held to what tests/test_sfs.py holds the host build to -- E EQUAL, as float.hex, to the set model over the same
chain's gene-tree records and locus rates, every per-sample row as float.hex, the data side as integers, after 1, 2 and the last
sample; the hand-made smallest shapes; the edges of the groups of loci; explicit pairs; the invariants; refusals; reset and limits;
the chain's trajectory unchanged by sampling -- plus the engine's host synchronisations and the checked build's index checks."""
import os

import pytest

from test_ancestry import GOLDEN_ITERS
from sfs_util import (check_case, check_chain_untouched, check_group_edges, check_lifecycle, check_model_invariants, check_one_leaf_populations,
                      check_pair_lists, check_pair_times_link, check_phase_rows, check_predictive_link, check_refusals, check_refused_sites,
                      check_small_shapes, small_model, two_base_loci)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.fixture(scope="module")
def small_base(G, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("small"), G.load_library(dims=(10, 7, 0)), "small")


@pytest.fixture(scope="module")
def ones_base(G, tmp_path_factory):
    return small_model(tmp_path_factory.mktemp("ones"), G.load_library(dims=(2, 3, 0)), "ones")


@pytest.mark.parametrize("name", ["m3", "j1", "a7", "stress", "x8"])
def test_device_accumulators_rows_and_observed_equal_the_model(G, name):
    r = check_case(None, name, key="gpu")
    if name == "m3":
        assert check_model_invariants(r) >= {"privP", "privQ", "shared", None, 1, 2}


@pytest.mark.parametrize("name", ["sample", "stress", "bigp"])
def test_counts_do_not_depend_on_the_phase_row_read(G, name):
    check_phase_rows(None, name)


def test_populations_of_one_to_four_leaves_and_the_odd_columns(G, small_base):
    check_small_shapes(None, small_base)


def test_two_populations_of_one_leaf(G, ones_base):
    check_one_leaf_populations(None, ones_base)


def test_groups_of_loci_at_their_edges(G):
    check_group_edges(None)


def test_spectrum_weighs_to_the_pairwise_differences_of_predictive(G, small_base):
    from mutations_util import phased_pack
    assert check_predictive_link(None, phased_pack(small_base, two_base_loci())) >= 9


def test_spectrum_weighs_to_the_pair_times_of_a_population(G):
    check_pair_times_link(None)


def test_explicit_pairs_in_another_order_and_none(G):
    check_pair_lists(None)


def test_refusals_name_the_cause_and_touch_nothing(G, capfd, ones_base):
    check_refusals(None, capfd, ones_base)


def test_a_locus_of_2_to_the_32_sites_is_refused_by_name(G, capfd, ones_base):
    check_refused_sites(None, ones_base, capfd)


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)


def test_checked_build_reports_no_index_violation(G, ones_base, small_base):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    assert check_case(lib, "m3")["oob"] == (0, 1)
    assert check_one_leaf_populations(lib, ones_base)["oob"] == (0, 1)
    assert check_small_shapes(lib, small_base)["oob"] == (0, 1)


def test_program_writes_the_two_sfs_files(G, tmp_path):
    from sfs_util import check_program
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_join_to_the_one_rank_files(G, tmp_path):
    from sfs_util import check_ranks
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_sfs_files(G, tmp_path):
    from sfs_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(None, tmp_path)
