"""Replicate genealogies on the MI355X (-m gpu): k_simulate and the site loop behind it in the product libraries, with the
tightest capacity variant per case, held to what tests/test_simulate.py holds the host build to -- every replicate record field by
field with ages as bit patterns, every accumulator word EQUAL as float.hex to the plain-Python restatement over the same chain's
records and models, every row as integers, after 1, 2 and 9 samples; the migration cap and the boundaries on hand-made 4-leaf
models; the selections; reset and limits; the seed; with_sites = 0; the chain's trajectory, its host synchronisations and
`resident` unchanged by sampling -- plus the checked build's index checks."""
import os

import pytest

from simulate_util import (MAX_MIGS, check_case, check_chain_untouched, check_edge_model, check_lifecycle, check_refused_locus, check_seed,
                           check_selections, check_sites_off, edge_model_bands)
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
    return edge_model_bands(tmp_path_factory.mktemp("edge"), G.load_library(dims=(4, 3, 2)))


@pytest.mark.parametrize("name", ["m3", "v8", "a7", "j3", "stress"])
def test_device_records_accumulators_and_rows_equal_the_restatement(G, tmp_path, name):
    r = check_case(None, name, tmp_path, key="gpu")
    if name == "a7":
        assert (r["trees"]["age"][:, :, :r["pack"].n] > 0).any(), "no leaf above age 0"


def test_device_replicates_of_72_leaves(G, tmp_path):
    check_case(None, "n7", tmp_path, loci=[0, 1], key="gpu")


def test_attempts_beyond_the_cap_are_redrawn(G, edge_base, tmp_path):
    r, _ = check_edge_model(None, edge_base, tmp_path, "cap")
    assert r["retried"] > 0 and (r["recs"][24]["num_migs"] <= MAX_MIGS).all()


def test_a_replicate_whose_every_attempt_fails_is_counted_and_left_out(G, edge_base, tmp_path):
    r, _ = check_edge_model(None, edge_base, tmp_path, "all-fail", iters=3)
    e = r["si"][3]
    assert e["failed"].tolist() == [3.0, 3.0, 3.0] and not e["acc"].any() and not e["site_acc"][:, :, 1:].any()
    assert (r["recs"][3]["root"] == -1).all()


@pytest.mark.parametrize("which", ["inner-band", "late-samples", "shared-ages"])
def test_boundaries(G, edge_base, tmp_path, which):
    check_edge_model(None, edge_base, tmp_path, which)


def test_seed_decides_the_replicates(G, tmp_path):
    check_seed(None, tmp_path)


def test_selections(G, tmp_path):
    check_selections(None, tmp_path)


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


def test_a_locus_whose_site_sums_could_pass_32_bits_is_refused_by_name(G, edge_base, capfd):
    check_refused_locus(None, edge_base, capfd)


def test_without_sites_the_genealogy_level_is_identical(G, tmp_path):
    check_sites_off(None, tmp_path)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    on, off = check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10, predictive=(name == "m3"))
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


def test_checked_build_reports_no_index_violation(G, tmp_path):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    r = check_case(lib, "m3", tmp_path, key="gpu checked")
    assert r["oob"] == (0, 1)


def test_program_writes_the_two_simulate_files(G, tmp_path):
    from simulate_util import check_program
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_join_to_the_one_rank_files(G, tmp_path):
    from simulate_util import check_ranks
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_simulate_files(G, tmp_path):
    from simulate_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(None, tmp_path)
