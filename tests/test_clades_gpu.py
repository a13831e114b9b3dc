"""Per-locus clade tables on the MI355X (-m gpu): k_clades in the product libraries, with the tightest capacity variant per
golden (m3: m, j1 / a7: s or l, x8: x, b2: b, n7: n with two key words), held to what tests/test_clades.py holds the host
build to -- every table EQUAL, as a set of (key, cnt, float.hex(age)) entries, to the plain-Python model over the same chain's
gene-tree records, at the default, tight, middle and wide slot settings; the group edges and selections; the chain's
trajectory unchanged by sampling; reset and limits -- plus the engine's host synchronisations and the checked build's index
checks."""
import os

import pytest

from test_ancestry import CASES, GOLDEN_ITERS
from test_clades import (check_case, check_chain_untouched, check_consensus_of_a_chain, check_failed_runs_leave_nothing, check_group_edges,
                         check_lifecycle, check_program, check_ranks, check_tables, run_chain)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.mark.parametrize("name", list(CASES))
def test_device_tables_equal_the_model_over_the_gene_tree_records(G, name):
    check_case(None, name, CASES[name], key="gpu")


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    on, off = check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]
    # (the launches of class 19 = the samples: check_chain_untouched; a sample may also bring forward the commit of a mixing
    # proposal that the next sweep kernel would have run, as for every sampler)


def test_group_edges_and_selections(G):
    check_group_edges(None)


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


def test_checked_build_reports_no_index_violation(G):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    for slots in (0, 8, 512):
        r = run_chain(lib, "m3", CASES["m3"], slots)
        check_tables(r["clades"], r["trees"], r["pack"].n, f"checked m3 slots {slots}")
        assert r["oob"] == (0, 1)
    for sel in ([15], list(range(0, 16, 3))):
        assert run_chain(lib, "m3", 4, 16, loci=sel, trees=False)["oob"] == (0, 1)


def test_consensus_of_sampled_tables(G):
    check_consensus_of_a_chain(None)


def test_program_writes_the_clades_and_consensus_files(G, tmp_path):
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_concatenate_to_the_one_rank_files(G, tmp_path):
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_clades_files(G, tmp_path):
    check_failed_runs_leave_nothing(None, tmp_path)
