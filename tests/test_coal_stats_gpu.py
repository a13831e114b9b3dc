"""Coalescent / sample-pair statistics on the MI355X (-m gpu): k_coal_stats and k_rows_fold in the product libraries, on
every capacity class the goldens reach, held to what tests/test_coal_stats.py holds the host build to -- every sample
against the restatement over a state dump (integers equal, fp64 sums within the summation bound), two runs bitwise equal,
the chain's trajectory unchanged by sampling, the program's files, the launcher's ranks -- plus the engine's host
synchronisations and the checked build's index checks.

Tiled pairs: x8 (496 pairs, 8 tiles of 64 lanes) and n7 (72 leaves: 2556 pairs, 10 tiles of 256 lanes); the other goldens
fit one tile."""
import os

import pytest

from conftest import GOLDEN
from sampler_util import _copy_case, _data_lines, _run, read_outputs
from test_coal_stats import (GOLDEN_ITERS, check_against_restatement, check_chain_untouched, check_failed_runs_leave_nothing,
                             check_ranks, expected_files, run_chain)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


# g1 / m3 / a7: the tightest variants they load (s / m), j1: bands with ancestral ends, v8: locus-mut-rate VAR (host-mode
# decisions), x8: variant x, n7: variant n (the reference's own caps)
CASES = {"g1": 30, "m3": 120, "a7": 60, "j1": 80, "v8": 60, "x8": 24, "n7": 12}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_rows_match_the_restatement_and_leave_the_chain_unchanged(G, tmp_path, name):
    iters = CASES[name]
    r = check_against_restatement(None, name, iters, tmp_path)
    on, off = check_chain_untouched(None, name, iters, GOLDEN_ITERS.get(name, iters), r["raw"], tmp_path, tol=1e-10)
    # no host synchronisation and no exchange is added to an iteration by a sample
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]
    # two kernels per sample, plus at most one k_mix_finish (an accepted mixing commit, which otherwise rides in the next
    # sweep kernel)
    samples = GOLDEN_ITERS.get(name, iters)
    extra = (s1["launches"] - s0["launches"]) - (n1["launches"] - n0["launches"])
    assert 2 * samples <= extra <= 3 * samples


def test_several_chunks_fold_in_chunk_order(G, tmp_path):
    r = check_against_restatement(None, "m3", 20, tmp_path, chunk=5)
    again = run_chain(None, "m3", 20, tmp_path, tag="again", chunk=5)["raw"]
    assert r["raw"].tobytes() == again.tobytes()


def test_checked_build_reports_no_index_violation(G, tmp_path):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    r = check_against_restatement(lib, "m3", 60, tmp_path)
    assert r["oob"] == (0, 1)
    r = check_against_restatement(lib, "x8", 6, tmp_path)
    assert r["oob"] == (0, 1)


def test_full_buffer_refuses_the_sample(G):
    pk = G.Pack.load(os.path.join(GOLDEN, "g1.gpk"))
    s = G.Sampler(pk)
    try:
        s.enable_coal_stats(2)
        s.initialize()
        for it in range(2):
            s.iteration(it)
            s.sample_coal_stats(it)
        with pytest.raises(BufferError):
            s.sample_coal_stats(2)
        assert s.coal_stats(raw=True)[:, 0].tolist() == [0.0, 1.0]
        s.sample_coal_stats(2)
        assert s.coal_stats(raw=True)[:, 0].tolist() == [2.0]
    finally:
        s.close()


def test_program_writes_the_statistics_files(G, tmp_path):
    a, b, c = tmp_path / "with", tmp_path / "without", tmp_path / "small"
    for d in (a, b, c):
        _copy_case("j1", d)
    _run(None, a, ["-s", "out", "j1.ctl"])
    _run(None, b, ["j1.ctl"])
    trace = a / "j1.trace"
    assert open(trace).read() == open(b / "j1.trace").read()
    from parity_util import compare_trace_files
    compare_trace_files(os.path.join(GOLDEN, "j1.trace"), str(trace))
    got = read_outputs(a, "out")
    want, its, p, _ = expected_files(str(a), "j1.ctl")
    assert [int(ln.split("\t")[0]) for ln in _data_lines(trace)] == its
    assert got == want
    _run(None, c, ["-s", "out", "--coal-stats-rows", "7", "j1.ctl"])
    assert read_outputs(c, "out") == got


def test_ranks_sharing_the_device_add_up_to_the_one_rank_rows(G, tmp_path):
    check_ranks(None, G.load_library(dims=(12, 5, 2)), "m3", tmp_path)


def test_failed_run_leaves_no_statistics_file(G, tmp_path):
    check_failed_runs_leave_nothing(None, tmp_path)
