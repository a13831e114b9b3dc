"""Metropolis-coupled chains on the MI355X: the bodies of tests/test_mc3.py (mc3_util.py) through the product libraries.

Here the chains of a group run on host threads of their own and their launches sit on their own streams at the same time; an
exchange hands device pointers from one engine to the other and orders the two streams through events.  The emulation it is
compared with runs plain Samplers one after the other, so every equality below is also a statement about that ordering.
A: the exchange alone on the five packs, twice in a row, behind accepted and rejected mixing proposals, the refusals.  B, C:
the group against the emulation, bit for bit.  D: the program.  E: the cold chain against the quadrature, with the margin
derived in tests/test_mc3.py (the host build runs the same code at the same sizes)."""
import pytest

import mc3_util as M

pytestmark = pytest.mark.gpu


def library(dims):
    import gphocs_amd as G
    return G.load_library(dims=dims)


def m3_library():
    p = M.load("m3")
    return library((p.n, p.K, p.B))


@pytest.mark.parametrize("name", M.EXCHANGE_PACKS)
def test_a_exchange(tmp_path, name):
    M.check_exchange(None, name, tmp_path)


def test_a_exchanged_twice(tmp_path):
    M.check_exchange_twice(None, "m3", tmp_path)


def test_a_exchange_behind_accepted_and_rejected_mixing(tmp_path):
    M.check_exchange_repeated(None, tmp_path)


def test_a_refusals(tmp_path):
    M.check_refusals(None, tmp_path)


@pytest.mark.parametrize("name", list(M.GROUP_RUNS))
def test_b_group_against_emulation(tmp_path, name):
    log = M.check_group(None, name, M.GROUP_RUNS[name], tmp_path)
    if name == "m3":
        assert all(any(e["accepted"] for e in log if e["lower"] == c) for c in (0, 1))


def test_b_swap_every_four(tmp_path):
    M.check_group(None, "m3", M.GROUP_RUNS["m3"], tmp_path, swap_every=4)


def test_c_outputs_follow_the_cold_state(tmp_path):
    M.check_group(None, "m3", M.GROUP_RUNS["m3"], tmp_path, trees=True)


def test_d_swaps_off_changes_no_output(tmp_path):
    M.check_program_outputs_unchanged(None, tmp_path)


def test_d_trace_and_report_against_emulation(tmp_path):
    M.check_program_against_emulation(None, m3_library(), tmp_path)


@pytest.mark.parametrize("args,names", M.USAGE_ERRORS)
def test_d_usage_errors(tmp_path, args, names):
    M.check_usage_error(None, tmp_path, args, names)


@pytest.mark.parametrize("options,names", M.LIBRARY_REFUSALS)
def test_d_library_refuses_the_same(tmp_path, capfd, options, names):
    M.check_library_refusal(m3_library(), tmp_path, capfd, options, names)


def test_d_failed_run_leaves_no_report(tmp_path):
    M.check_failed_run_leaves_no_report(None, tmp_path)


def test_e_cold_chain_samples_the_posterior(tmp_path):
    from test_mc3 import SD_PLAIN
    M.check_cold_chain_samples_posterior(library((2, 3, 0)), tmp_path, SD_PLAIN)
