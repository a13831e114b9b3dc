"""Replicate chains and their convergence diagnostics on the MI355X: the bodies of tests/test_replicates.py
(replicates_util.py) through the product libraries, the tightest capacity variant per golden (m3: m, x8: x, n7: n with two key
words).

Here the chains sit on streams of their own and k_clades_compare reads R engines' tables from the stream of the first: every
equality with the model over tables fetched AFTERWARDS is also a statement about the events that order those streams.  On top
of the host build's tests: a compare costs exactly one host synchronisation and one launch of timing class 20 on the leading
engine (asserted inside the ordering test), and the checked library reports no index outside its array."""
import os

import pytest

import replicates_util as U

pytestmark = pytest.mark.gpu


def m3_library():
    import gphocs_amd as G
    p = U.load("m3")
    return G.load_library(dims=(p.n, p.K, p.B))


@pytest.mark.parametrize("slots,drops", [(2048, False), (128, True), (8, True), (2, True)])
def test_a_m3_against_the_model(slots, drops):
    U.check_against_model(None, "m3", 120, slots, drops=drops)


def test_a_x8_against_the_model():
    U.check_against_model(None, "x8", 24, 1024, drops=False)


def test_a_n7_two_key_words():
    U.check_against_model(None, "n7", 12, 2048, Rs=(2,), drops=False)


def test_a_sixteen_chains():
    U.check_against_model(None, "m3", 6, 64, Rs=(16,))


def test_a_min_freq():
    U.check_min_freq(None)


def test_a_twins_and_permuted_chains():
    U.check_hand_set_edges(None)


def test_b_group_edges_and_selections():
    U.check_group_edges(None)


def test_c_ordering_and_non_interference(tmp_path):
    U.check_ordering(None, tmp_path)


def test_c_checked_build_reports_no_index_violation():
    import gphocs_amd as G
    U.check_checked_build(G.load_library(os.path.join(os.path.dirname(G.LIB_PATH), G.CHECKED_LIB)))


def test_d_refusals():
    U.check_refusals(None)


def test_e_psrf():
    U.check_psrf(m3_library())


def test_f_program_outputs(tmp_path):
    U.check_program(None, m3_library(), tmp_path)


def test_f_without_clades_no_asdsf_table(tmp_path):
    U.check_program_without_clades(None, tmp_path)


@pytest.mark.parametrize("args,names", U.USAGE_ERRORS)
def test_f_usage_errors(tmp_path, args, names):
    U.check_usage_error(None, tmp_path, args, names)


@pytest.mark.parametrize("options,names", U.LIBRARY_REFUSALS)
def test_f_library_refuses_the_same(tmp_path, capfd, options, names):
    U.check_library_refusal(m3_library(), tmp_path, capfd, options, names)


def test_f_failed_run_leaves_no_tables(tmp_path):
    U.check_failed_run_leaves_no_tables(None, tmp_path)
