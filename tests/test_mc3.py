"""Metropolis-coupled chains on the CPU: the host build of the engine sources (tests/hostemu).

mc3_util.py holds the test bodies (the MI355X runs the same ones, test_mc3_gpu.py) and the emulation they compare with: an
MC3 run rebuilt from plain Samplers whose betas are exchanged with set_beta.  Everything but E is bit for bit.

A  the exchange alone, on m3 (bands, SPR), v8 (locus-mut-rate VAR), a7 (a sample age), bigp (P > 64: two launch groups), x8
   (32 leaves): the dumps are crossed, what belongs to the engine stays, checkAll passes, and five more iterations give the
   dumps of the emulation; exchanged twice, a pair equals one that never was; on m3, exchanges in front of iterations 7 .. 20,
   some behind an accepted mixing proposal (its commit is still owed to the pages), some behind a rejected one; the refusals.
B  the group against the emulation: C = 3, beta = (1, 0.7, 0.4), a swap attempted before every iteration, on m3 (120
   iterations), v8 (60), a7 (100); every chain's dump, chain 0's TRACE lines, the summed accept counters, the swap log field
   by field.  m3 again with a swap every 4 iterations.
C  chain 0's sampled genealogies are those of whoever holds beta = 1 in the emulation, after every call.
D  the program: --mc3 with the swaps off leaves every output file as it is without it; with them the trace is the emulation's
   cold holder's and the report its log; usage errors; no report after a failed run.
E  the cold chain still samples the posterior: the toy model of power_posterior_util.py, `--mc3 4 --mc3-heat 2`, burn-in 500,
   2000 samples.  h = 2 was chosen on the host build: the pairs' accepted fractions are 0.211, 0.737, 0.870 there (the range
   [0.1, 0.9] is asserted), and it is the heat at which a wrong sign of lnr shows (below).  The mean of the data log-likelihood
   over the trace (the last column: the trace prints dataLogLikelihood under "Full-ld-ln") is compared with
   E_1[l] = d ln Z(beta) / d beta at beta = 1, by a central difference (eps = 1e-3) of the quadrature:
     quadrature  -1830.5752900 at steps (1e-4, 2e-4), refinement error 1.2e-4 against (2e-4, 4e-4) (the test recomputes both)
   The margin is 4 standard deviations of that mean over 8 seeds of the PLAIN chain at the same length on the host build
   (seeds 101 .. 108 of the control file) plus the refinement error -- coupling must not make the chain worse:
     -1831.225258 -1830.743501 -1831.077727 -1829.708179 -1830.952982 -1831.441195 -1830.576936 -1830.440297
     mean -1830.7708, standard deviation 0.5425;  margin 4 x 0.5425 + 1.2e-4 = 2.1701
   This run: mean -1830.790954 (0.2157 from the quadrature).  With the sign of lnr flipped in gph_mc3.h the same run gives
   -1832.787046 (2.2118 off: outside the margin) and accepted fractions 0.881, 0.879, 0.922 (outside the range)."""
import pytest

import mc3_util as M

SD_PLAIN = 0.5425          # over the 8 seeds of the docstring


@pytest.fixture(scope="module")
def hostemu():
    from sampler_util import hostemu_library
    return hostemu_library()


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("name", M.EXCHANGE_PACKS)
def test_a_exchange(hostemu, tmp_path, name):
    M.check_exchange(hostemu[1], name, tmp_path)


def test_a_exchanged_twice(hostemu, tmp_path):
    M.check_exchange_twice(hostemu[1], "m3", tmp_path)


def test_a_exchange_behind_accepted_and_rejected_mixing(hostemu, tmp_path):
    M.check_exchange_repeated(hostemu[1], tmp_path)


def test_a_refusals(hostemu, tmp_path):
    M.check_refusals(hostemu[1], tmp_path)


# ---------------------------------------------------------------- B, C
@pytest.mark.parametrize("name", list(M.GROUP_RUNS))
def test_b_group_against_emulation(hostemu, tmp_path, name):
    log = M.check_group(hostemu[1], name, M.GROUP_RUNS[name], tmp_path)
    if name == "m3":
        assert all(any(e["accepted"] for e in log if e["lower"] == c) for c in (0, 1))


def test_b_swap_every_four(hostemu, tmp_path):
    M.check_group(hostemu[1], "m3", M.GROUP_RUNS["m3"], tmp_path, swap_every=4)


def test_c_outputs_follow_the_cold_state(hostemu, tmp_path):
    M.check_group(hostemu[1], "m3", M.GROUP_RUNS["m3"], tmp_path, trees=True)


# ---------------------------------------------------------------- D
def test_d_swaps_off_changes_no_output(hostemu, tmp_path):
    M.check_program_outputs_unchanged(hostemu[0], tmp_path)


def test_d_trace_and_report_against_emulation(hostemu, tmp_path):
    M.check_program_against_emulation(hostemu[0], hostemu[1], tmp_path)


@pytest.mark.parametrize("args,names", M.USAGE_ERRORS)
def test_d_usage_errors(hostemu, tmp_path, args, names):
    M.check_usage_error(hostemu[0], tmp_path, args, names)


@pytest.mark.parametrize("options,names", M.LIBRARY_REFUSALS)
def test_d_library_refuses_the_same(hostemu, tmp_path, capfd, options, names):
    M.check_library_refusal(hostemu[1], tmp_path, capfd, options, names)


def test_d_failed_run_leaves_no_report(hostemu, tmp_path):
    M.check_failed_run_leaves_no_report(hostemu[0], tmp_path)


# ---------------------------------------------------------------- E
def test_e_cold_chain_samples_the_posterior(hostemu, tmp_path):
    M.check_cold_chain_samples_posterior(hostemu[1], tmp_path, SD_PLAIN)
