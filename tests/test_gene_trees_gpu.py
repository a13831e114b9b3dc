"""Sampled genealogies per locus on the MI355X (-m gpu): k_gene_trees in the product libraries, with the tightest capacity
variant per golden (m3: m, j1 / a7: s or l, x8: x, b2: b with its many bands, n7: n with the reference's own caps), held to
what tests/test_gene_trees.py holds the host build to -- every field of every record EQUAL to the state dump's, the
selections byte for byte, the chain's trajectory unchanged by sampling, capacity, the program's file, the ranks, failed
runs -- plus the engine's host synchronisations and the checked build's index checks."""
import os

import pytest

from test_gene_trees import (CASES, GOLDEN_ITERS, _SEEN, check_against_dumps, check_capacity, check_case_set, check_chain_untouched,
                             check_failed_runs_leave_nothing, check_no_bands, check_program, check_ranks, check_selections)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.mark.parametrize("name", list(CASES))
def test_device_records_equal_the_state_dumps_and_leave_the_chain_unchanged(G, tmp_path, name):
    check_against_dumps(None, name, CASES[name], tmp_path, key="gpu")
    on, off = check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)
    # no host synchronisation and no exchange is added to an iteration by a sample (the capacity holds all samples)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]
    assert on["launches"] == GOLDEN_ITERS[name]


def test_the_case_set_reaches_every_path(G, tmp_path):
    for name in CASES:
        if ("gpu", name) not in _SEEN:
            check_against_dumps(None, name, CASES[name], tmp_path, key="gpu")
    check_case_set("gpu", list(CASES))


def test_a_model_without_bands_has_no_migration(G, tmp_path):
    check_no_bands(None, tmp_path, key="gpu")


def test_selections(G, tmp_path):
    check_selections(None, tmp_path)


def test_checked_build_reports_no_index_violation(G, tmp_path):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    r = check_against_dumps(lib, "m3", CASES["m3"], tmp_path, key="chk")
    assert r["oob"] == (0, 1)
    check_selections(lib, tmp_path, iters=3)


def test_capacity_limit_and_lifecycle(G):
    check_capacity(None, G)


def test_program_writes_the_trees_file(G, tmp_path):
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_concatenate_to_the_one_rank_file(G, tmp_path):
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_trees_file(G, tmp_path):
    check_failed_runs_leave_nothing(None, tmp_path)
