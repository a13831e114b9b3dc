"""Expected substitutions per population branch and per sample on the MI355X (-m gpu): k_mutations in the product libraries, with
the tightest capacity variant per case, held to what tests/test_mutations.py holds the host build to -- the float model's inside
pass EQUAL to every record's dataLnL, then accumulators and per-sample rows EQUAL to the model as float.hex after 1, 2 and 9
samples; the tile edges; selections with a partial chunk; refusals; reset and limits; the chain's trajectory unchanged by
sampling -- plus the engine's host synchronisations and the checked build's index checks."""
import os
import shutil

import pytest

from conftest import GOLDEN
from test_ancestry import GOLDEN_ITERS
import mutations_util as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.mark.parametrize("name", ["m3", "j1", "a7", "v8", "stress", "bigp", "x8"])
def test_device_accumulators_and_rows_equal_the_model(G, name):
    r = M.check_case(None, name, key="gpu", loci=M.STRESS_LOCI if name == "stress" else None)
    if name in ("j1", "x8"):
        assert r["maxseg"] > M.SEGS, "no branch with more segments than a list holds: the second walk never ran"


def test_a_column_of_64_phases(G, tmp_path):
    for ext in (".ctl", ".seq"):
        shutil.copy(os.path.join(GOLDEN, "p7" + ext), tmp_path)
    pk = G.Pack.from_control(os.path.join(tmp_path, "p7.ctl"), seq_path=os.path.join(tmp_path, "p7.seq"))
    assert max(M.phases_of(w) for w in pk.numPhases) == 64
    M.check_case(None, "p7", pack=pk, key="gpu")


def test_72_leaves(G):
    M.check_case(None, "n7", loci=[0, 1], key="gpu")


def test_a_block_that_stays_in_hbm(G):
    M.check_case(None, "q6", loci=[0], iters=3, key="gpu")


def test_136_leaves_without_segment_lists(G):
    M.check_case(None, "t136", iters=2, checkpoints=(1,), key="gpu")


def test_zero_length_branches(G, tmp_path):
    from predictive_util import edge_model
    M.check_zero_length_branches(None, edge_model(tmp_path, G.load_library(dims=(4, 3, 0))))


def test_columns_at_the_tile_edges(G, tmp_path):
    from predictive_util import edge_model
    M.check_tile_edges(None, edge_model(tmp_path, G.load_library(dims=(4, 3, 0))))


def test_selections_and_partial_chunks(G):
    M.check_selections(None)


def test_refusals_name_the_cause_and_touch_nothing(G, capfd):
    M.check_refusals(None, capfd)


def test_reset_limits_and_lifecycle(G):
    M.check_lifecycle(None, G)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged_and_adds_no_synchronisation(G, tmp_path, name):
    on, off = M.check_chain_untouched(None, name, GOLDEN_ITERS[name], tmp_path, tol=1e-10)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


def test_checked_build_reports_no_index_violation(G, tmp_path):
    from predictive_util import edge_model
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    assert M.check_case(lib, "m3", key="gpu chk")["oob"] == (0, 1)
    assert M.check_tile_edges(lib, edge_model(tmp_path, lib))["oob"] == (0, 1)


def test_program_writes_the_two_mutations_files(G, tmp_path):
    M.check_program(None, None, tmp_path)


def test_ranks_sharing_the_device_join_to_the_rank_order_sum(G, tmp_path):
    M.check_ranks(None, G.load_library(dims=(12, 5, 2)), tmp_path)


def test_failed_run_leaves_no_mutations_files(G, tmp_path):
    M.check_failed_runs_leave_nothing(None, tmp_path)
