"""Effective sample sizes on the MI355X (-m gpu): k_ess in the product libraries, with the tightest capacity variant per case
(m3 / v8: s or m, a70: s, x8: x, n7: n with two key words, t136: n with three), held to what tests/test_ess.py holds the host
build to -- every accumulator word EQUAL, as float.hex, to the plain-Python model over the same chain's gene-tree records, the
focal sets and topoChanges exactly, after 1, 2, 37 and 64 samples; the selections; gph_ess against its restatement; the
read-out; the chain's trajectory unchanged by sampling; the program's files; reset and limits -- plus the engine's host
synchronisations and the checked build's index checks."""
import os

import pytest

from ess_util import (CHECKPOINTS, ar1, check_against_model, check_case, check_chain_untouched, check_failed_runs_leave_nothing, check_levels,
                      check_lifecycle, check_program, check_ranks, check_selections, ess_series, run_chain, same_bits)
from test_ancestry import GOLDEN_ITERS
from test_ess import AR1_SEED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.mark.parametrize("name,iters", [("m3", 64), ("x8", 64), ("v8", 64), ("a70", 64), ("n7", 64), ("t136", 37)])
def test_device_accumulators_equal_the_model_over_the_gene_tree_records(G, name, iters):
    r, _ = check_case(None, name, iters, checkpoints=[c for c in CHECKPOINTS if c <= iters], key="gpu")
    e = r["ess"][iters]
    assert len(e["series"]) == (6 if name == "v8" else 5)
    assert e["words"] == {"n7": 2, "t136": 3}.get(name, 1)


def test_selections(G):
    check_selections(None)


def test_gph_ess_equals_its_restatement_in_a_product_library(G):
    lib = G.load_library()
    for x, lag in ((ar1(4099, 0.9, AR1_SEED), 0), (ar1(4099, 0.9, AR1_SEED), 5), ([2.5] * 100, 0), ([(-1.0) ** t for t in range(200)], 0),
                   ([1.0, 3.0], 0), ([1.0, 3.0, 2.0], 0)):
        same_bits(G.ess(x, lag, lib=lib), ess_series(x, lag), f"S {len(x)} max_lag {lag}")
    got = G.ess(ar1(65536, 0.9, AR1_SEED), lib=lib)
    assert 19 / 1.6 <= got["tauBatch"] <= 19 * 1.6 and 19 / 1.6 <= got["tauAcf"] <= 19 * 1.6


def test_read_out_and_the_level_rule(G):
    check_levels(None)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    on, off = check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]
    # (the launches of class 21 = the samples: check_chain_untouched)


def test_reset_limits_and_lifecycle(G):
    check_lifecycle(None, G)


def test_checked_build_reports_no_index_violation(G):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    everything = run_chain(lib, "m3", 9)
    check_against_model(everything["ess"][9], everything["trees"], everything["rates"], everything["pack"].n, 9, "checked m3")
    assert everything["oob"] == (0, 1)
    for sel in ([15], list(range(0, 16, 3))):
        r = run_chain(lib, "m3", 4, loci=sel, trees=False)
        assert r["oob"] == (0, 1) and r["ess"][4]["loci"].tolist() == sel


def test_program_writes_the_two_ess_files(G, tmp_path):
    check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_concatenate_to_the_one_rank_files(G, tmp_path):
    check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_ess_files(G, tmp_path):
    check_failed_runs_leave_nothing(None, tmp_path)
