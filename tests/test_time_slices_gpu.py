"""Time-sliced coalescence / migration statistics on the MI355X (-m gpu): k_time_slices and k_rows_fold in the
product libraries, on every capacity class the goldens reach, held to what tests/test_time_slices.py holds the host build
to -- every sample against the restatement over a state dump (counts equal, fp64 sums within the summation bound), the
slices adding up to the pages' own statistics, two runs bitwise equal, the chain's trajectory unchanged by sampling, the
program's file -- plus the engine's host synchronisations, launches and the checked build's index checks.

x8 runs on variant x, n7 (72 leaves, variant n: the reference's own caps) with the walkers of one locus per group."""
import os

import pytest

from conftest import GOLDEN
from test_time_slices import (ITERS, SUM_CASES, check_against_restatement, check_chain_untouched, check_failed_runs_leave_nothing,
                              check_program, check_ranks, run_chain)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.mark.parametrize("name,S", [("g1", 4), ("m3", 1), ("m3", 4), ("m3", 7), ("a7", 4), ("j1", 7), ("v8", 4), ("x8", 7), ("n7", 4)])
def test_device_rows_match_the_restatement_and_leave_the_chain_unchanged(G, tmp_path, name, S):
    iters = ITERS[name]
    r = check_against_restatement(None, name, iters, S, tmp_path, need_mig=name in ("m3", "j1"))
    on, off = check_chain_untouched(None, name, iters, S, r["raw"], tmp_path)
    # no host synchronisation and no exchange is added to an iteration by a sample
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]
    # DESIGN: two kernels per sample, plus the k_mix_finish launches (timing class 7) a sample makes of accepted mixing
    # commits that otherwise ride in the next sweep kernel: one launch per launch group of loci, two groups at most
    extra = (s1["launches"] - s0["launches"]) - (n1["launches"] - n0["launches"])
    mf = on["mix_finishes"] - off["mix_finishes"]
    assert 0 <= mf <= iters and 2 * iters + mf <= extra <= 2 * iters + 2 * mf


@pytest.mark.parametrize("name,S", SUM_CASES + [("n7", 4)])
def test_slices_add_up_to_the_pages_own_statistics(G, tmp_path, name, S):
    check_against_restatement(None, name, ITERS[name], S, tmp_path, log_period=1, need_mig=name in ("m3", "j1"))


def test_several_chunks_fold_in_chunk_order(G, tmp_path):
    r = check_against_restatement(None, "m3", 20, 4, tmp_path, chunk=5, need_mig=True)
    again = run_chain(None, "m3", 20, 4, tmp_path, tag="again", chunk=5)["raw"]
    assert r["raw"].tobytes() == again.tobytes()


def test_checked_build_reports_no_index_violation(G, tmp_path):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    r = check_against_restatement(lib, "m3", 30, 4, tmp_path, need_mig=True)
    assert r["oob"] == (0, 1)
    r = check_against_restatement(lib, "x8", 5, 7, tmp_path)
    assert r["oob"] == (0, 1)


def test_full_buffer_and_bad_slice_counts(G):
    pk = G.Pack.load(os.path.join(GOLDEN, "g1.gpk"))
    s = G.Sampler(pk)
    try:
        s.initialize()
        for bad in (0, 33):
            with pytest.raises(ValueError):
                s.enable_time_slices(bad, 2)
        s.enable_time_slices(32, 2)
        for it in range(2):
            s.iteration(it)
            s.sample_time_slices(it)
        with pytest.raises(BufferError):
            s.sample_time_slices(2)
        assert s.time_slices()[:, 0].tolist() == [0.0, 1.0]
        s.sample_time_slices(2)
        assert s.time_slices()[:, 0].tolist() == [2.0]
    finally:
        s.close()


def test_program_writes_the_slices_file(G, tmp_path):
    check_program(None, None, tmp_path, "j1", 7)


def test_ranks_sharing_the_device_add_up_to_the_one_rank_rows(G, tmp_path):
    check_ranks(None, G.load_library(dims=(12, 5, 2)), "m3", 4, tmp_path)


def test_failed_run_leaves_no_slices_file(G, tmp_path):
    check_failed_runs_leave_nothing(None, tmp_path)
