"""Replicate chains and their convergence diagnostics on the CPU: the host build of the engine sources (tests/hostemu), which
runs k_clades_compare's own text lane by lane.

replicates_util.py holds the test bodies (the MI355X runs the same ones, test_replicates_gpu.py), the model they compare with
-- gph_engine_clades_compare restated in plain Python over each chain's fetched tables -- and the tolerances with their
derivation.

A  the kernel against the model.  m3 (12 leaves, 16 loci, 120 iterations), R = 2 and 4, at 2048 slots (limit 1536 >= 120 x 11:
   no table can drop), 128 (the default: seeds +0 .. +3 visit 449 .. 537 distinct clades a locus, every table is full), 8 (the
   tight setting of test_clades.py) and 2 (one clade kept, a table smaller than the wavefront); x8 (32 leaves, 10 loci, 24
   iterations) at 1024 (limit 768 >= 744); n7 (72 leaves, two key words, 12 iterations) at 2048 on the big build; R = 16 on m3;
   min_freq 0, 0.1 and 1; a chain against its twin of the same seed (asdsf == maxSd == 0.0, shared == distinct) and the order of
   the chains permuted; the trivial clade is counted nowhere.
B  group edges: selections of 1, 3, 4, 5 loci and one with gaps, every row bit-equal to the all-loci compare's; a selection
   beyond the rank's block launches nothing.
C  the compare right behind the samples of all chains, and again after more; the tables still equal the model over each
   chain's gene-tree records; chain 0's records and final dump with and without the compares.
D  every refusal leaves the engines usable.
E  gph_psrf against the Python loop, bit for bit, and its edges.
F  the program."""
import pytest

import replicates_util as U


@pytest.fixture(scope="module")
def hostemu():
    from sampler_util import hostemu_library
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("slots,drops", [(2048, False), (128, True), (8, True), (2, True)])
def test_a_m3_against_the_model(hostemu, slots, drops):
    U.check_against_model(hostemu[1], "m3", 120, slots, drops=drops)


def test_a_x8_against_the_model(hostemu):
    U.check_against_model(hostemu[1], "x8", 24, 1024, drops=False)


def test_a_n7_two_key_words(hostemu_big):
    U.check_against_model(hostemu_big, "n7", 12, 2048, Rs=(2,), drops=False)


def test_a_sixteen_chains(hostemu):
    U.check_against_model(hostemu[1], "m3", 6, 64, Rs=(16,))


def test_a_min_freq(hostemu):
    U.check_min_freq(hostemu[1])


def test_a_twins_and_permuted_chains(hostemu):
    U.check_hand_set_edges(hostemu[1])


# ---------------------------------------------------------------- B
def test_b_group_edges_and_selections(hostemu):
    U.check_group_edges(hostemu[1])


# ---------------------------------------------------------------- C
def test_c_ordering_and_non_interference(hostemu, tmp_path):
    U.check_ordering(hostemu[1], tmp_path)


# ---------------------------------------------------------------- D
def test_d_refusals(hostemu):
    U.check_refusals(hostemu[1])


# ---------------------------------------------------------------- E
def test_e_psrf(hostemu):
    U.check_psrf(hostemu[1])


# ---------------------------------------------------------------- F
def test_f_program_outputs(hostemu, tmp_path):
    U.check_program(hostemu[0], hostemu[1], tmp_path)


def test_f_without_clades_no_asdsf_table(hostemu, tmp_path):
    U.check_program_without_clades(hostemu[0], tmp_path)


@pytest.mark.parametrize("args,names", U.USAGE_ERRORS)
def test_f_usage_errors(hostemu, tmp_path, args, names):
    U.check_usage_error(hostemu[0], tmp_path, args, names)


@pytest.mark.parametrize("options,names", U.LIBRARY_REFUSALS)
def test_f_library_refuses_the_same(hostemu, tmp_path, capfd, options, names):
    U.check_library_refusal(hostemu[1], tmp_path, capfd, options, names)


def test_f_failed_run_leaves_no_tables(hostemu, tmp_path):
    U.check_failed_run_leaves_no_tables(hostemu[0], tmp_path)
