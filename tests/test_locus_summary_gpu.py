"""Per-locus posterior summaries on the MI355X (-m gpu): k_locus_summary in the product libraries, on every capacity class
the goldens reach, checked as tests/test_locus_summary.py checks the host build -- raw accumulators rebuilt bit for bit
from state dumps, the chain's trajectory unchanged by sampling, the program's table, the launcher's ranks -- plus the
engine's host synchronisations and the checked build's index checks."""
import os

import pytest

from conftest import GOLDEN
from sampler_util import _copy_case, _data_lines, _locus_names, _pop_names, _run
from test_locus_summary import GOLDEN_ITERS, check_against_dumps, check_trajectory_unchanged, expected_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


# g1 / m3: the tightest variants they load (s / m), x8: x, j1: bands with ancestral ends, b2: b (many bands), n7: n (the
# reference's own caps), v8: locus-mut-rate VAR (host-mode decisions)
CASES = {"g1": 30, "m3": 120, "x8": 24, "j1": 80, "b2": 24, "n7": 12, "v8": 60}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_summaries_match_state_dumps_and_leave_the_chain_unchanged(G, tmp_path, name):
    iters = CASES[name]
    r = check_against_dumps(None, name, iters, tmp_path)
    on, off = check_trajectory_unchanged(None, name, iters, GOLDEN_ITERS.get(name, iters), r["raw"], tmp_path, tol=1e-10)
    # no host synchronisation and no exchange is added to an iteration by a sample
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


def test_checked_build_reports_no_index_violation(G, tmp_path):
    lib = G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB))
    r = check_against_dumps(lib, "m3", 60, tmp_path)
    assert r["oob"] == (0, 1)


def test_program_writes_the_summary_table(G, tmp_path):
    a, b = tmp_path / "with", tmp_path / "without"
    _copy_case("j1", a)
    _copy_case("j1", b)
    _run(None, a, ["-l", "sum.tsv", "j1.ctl"])
    _run(None, b, ["j1.ctl"])
    trace = a / "j1.trace"
    assert open(trace).read() == open(b / "j1.trace").read()
    from parity_util import compare_trace_files
    compare_trace_files(os.path.join(GOLDEN, "j1.trace"), str(trace))
    got = open(a / "sum.tsv").read()
    want, S, p = expected_table(str(a), "j1.ctl", _pop_names(a / "j1.ctl"))
    assert S == len(_data_lines(trace))
    assert [r.split("\t")[1] for r in got.splitlines()[1:]] == _locus_names(a / "j1.seq")
    assert got == want


def test_launcher_ranks_sharing_the_device_write_the_same_table(G, tmp_path):
    one, two = tmp_path / "g1", tmp_path / "g2"
    _copy_case("m3", one)
    _copy_case("m3", two)
    _run(None, one, ["-l", "sum.tsv", "m3.ctl"])
    _run(None, two, ["-g", "2", "-l", "sum.tsv", "m3.ctl"])
    assert open(two / "sum.tsv").read() == open(one / "sum.tsv").read()
    assert not [f for f in os.listdir(two) if ".part" in f]
