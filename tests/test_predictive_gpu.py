"""Posterior predictive checks on the MI355X (-m gpu): k_predictive in the product libraries, with the tightest capacity
variant per case, held to what tests/test_predictive.py holds the host build to -- every accumulator word EQUAL, as float.hex,
to the numpy / math.exp model over the same chain's gene-tree records, every per-sample row and observed value as integers,
after 1, 2 and 9 samples; the edges of the site loop on hand-made packs; the selections; reset and limits; the seed; the
chain's trajectory unchanged by sampling -- plus the engine's host synchronisations and the checked build's index checks."""
import os

import pytest

from predictive_util import (check_case, check_chain_untouched, check_edges, check_lifecycle, check_refused_locus, check_seed, check_selections,
                             edge_model, model_loci, check_against_model, check_rows, run_chain)
from test_ancestry import GOLDEN_ITERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.fixture(scope="module")
def edge_base(G, tmp_path_factory):
    return edge_model(tmp_path_factory.mktemp("edge"), G.load_library(dims=(4, 3, 0)))


@pytest.mark.parametrize("name", ["m3", "v8", "a7", "j3", "sample", "stress", "bigp"])
def test_device_accumulators_rows_and_observed_equal_the_model(G, name):
    check_case(None, name, key="gpu")


def test_device_accumulators_of_72_leaves(G):
    check_case(None, "n7", loci=[0, 1], key="gpu")


@pytest.mark.parametrize("big_count", [False, True])
def test_site_loop_edges(G, edge_base, big_count):
    check_edges(None, edge_base, big_count)


def test_a_locus_whose_sums_could_pass_32_bits_is_refused_by_name(G, edge_base, capfd):
    check_refused_locus(None, edge_base, capfd)


def test_selections(G):
    check_selections(None)


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


def test_seed_decides_the_replicates(G):
    check_seed(None)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    on, off = check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


def test_checked_build_reports_no_index_violation(G, edge_base):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    r = run_chain(lib, "m3", 9)
    pk = r["pack"]
    model, rows, obs_row = model_loci(pk, r["trees"], r["rates"], r["seed"], 9, list(range(pk.L)))
    check_against_model(r["pd"][9], model, 9, "checked m3")
    check_rows(r, rows, obs_row, 9, "checked m3")
    assert r["oob"] == (0, 1)
    assert check_edges(lib, edge_base, True)["oob"] == (0, 1)


def test_program_writes_the_two_predictive_files(G, tmp_path):
    from predictive_util import check_program
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_join_to_the_one_rank_files(G, tmp_path):
    from predictive_util import check_ranks
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_predictive_files(G, tmp_path):
    from predictive_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(None, tmp_path)
