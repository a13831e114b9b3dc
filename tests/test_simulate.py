"""Replicate genealogies simulated from the sampled parameters (gph_engine_simulate_*) on the CPU: the host-emulation build of the
engine sources runs k_simulate, the device text itself, lane by lane, and k_predictive's site loop on the replicate records.

The restatement of the definition (tests/simulate_util.py, plain Python floats and math.log) is first held to closed forms of the
structured coalescent on hand-made models; then the library is held to the restatement bit for bit: every replicate record field
by field with ages as bit patterns, every accumulator word as float.hex, every row as integers, after 1, 2 and 9 samples of one
chain on m3 (bands), v8 (VAR rates), a7 (ancient samples), j3 (four current populations), sample / stress (phase groups, for the
site level) and n7 (72 leaves, loci 0 and 1, the host build with the reference's caps); on hand-made models for the migration cap
and the boundaries; the seed, selections, reset / limits / lifecycle, with_sites = 0, and the chain left untouched."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from sampler_util import hostemu_library
from simulate_util import (MAX_MIGS, attempt, attempt_key, check_case, check_chain_untouched, check_edge_model, check_lifecycle, check_refused_locus,
                           check_seed, check_selections, check_sites_off, closed_form_model_1, closed_form_model_2, edge_model_bands, edge_models, simulate)
from test_ancestry import GOLDEN_ITERS

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))
REPLICATES, CTL_SEED = 16384, 31         # the seed of the hand-made control file (predictive_util.EDGE_CTL); fixed, not searched


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


@pytest.fixture(scope="module")
def edge_base(hostemu, tmp_path_factory):
    return edge_model_bands(tmp_path_factory.mktemp("edge"), hostemu[1])


def _z(count, p, N=REPLICATES):
    return (count / N - p) / math.sqrt(p * (1 - p) / N)


# ---------------------------------------------------------------- 1: the restatement against closed forms
def test_restatement_two_populations_without_a_band():
    """mean coal_A = 1 - exp(-2 tau / theta_A), the same for B (binomial variance), and mean TMRCA = tau + sum_k P(k lineages
    reach the root) theta_R (1 - 1 / k) (sample standard error): within 5 standard errors at 16 384 replicates"""
    m, tau, (thA, thB, thR) = closed_form_model_1()
    reps = [simulate(m, CTL_SEED, 0, t) for t in range(REPLICATES)]
    assert all(r is not None and r["attempts"] == 0 and not r["migs"] for r in reps)
    pA, pB = 1 - math.exp(-2 * tau / thA), 1 - math.exp(-2 * tau / thB)
    assert 0.4 < pA < 0.6 and 0.4 < pB < 0.6
    for p, exact in ((0, pA), (1, pB)):
        assert all(r["ncoal"][p] in (0, 1) for r in reps)
        z = _z(sum(r["ncoal"][p] for r in reps), exact)
        print(f"coal_{p}: z {z:+.2f}")
        assert abs(z) <= 5.0
    pk = {2: pA * pB, 3: pA * (1 - pB) + (1 - pA) * pB, 4: (1 - pA) * (1 - pB)}
    exact = tau + sum(pr * thR * (1 - 1 / k) for k, pr in pk.items())
    tm = np.array([r["y"][0] for r in reps])
    assert (tm > tau).all() and all(sum(r["ncoal"]) == 3 for r in reps)
    z = (tm.mean() - exact) / (tm.std(ddof=1) / math.sqrt(REPLICATES))
    print(f"tmrca: mean {tm.mean():.6g} exact {exact:.6g} z {z:+.2f}")
    assert abs(z) <= 5.0


def test_restatement_one_band():
    """one leaf each and a band whose target is A, live on [0, tau): P(a migration) = 1 - exp(-m tau); mean coal_B = the integral
    of m exp(-m s) (1 - exp(-2 (tau - s) / theta_B)) over [0, tau), in closed form"""
    m, tau, thB, mr = closed_form_model_2()
    reps = [simulate(m, CTL_SEED, 0, t) for t in range(REPLICATES)]
    assert all(r is not None and r["attempts"] == 0 and len(r["migs"]) <= 1 for r in reps)
    pm = 1 - math.exp(-mr * tau)
    a = 2 / thB
    pc = pm - mr * math.exp(-a * tau) * (math.exp((a - mr) * tau) - 1) / (a - mr)
    assert 0.4 < pm < 0.6 and 0 < pc < pm
    zm, zc = _z(sum(len(r["migs"]) for r in reps), pm), _z(sum(r["ncoal"][1] for r in reps), pc)
    print(f"migration: z {zm:+.2f}; coal_B: exact {pc:.4f} z {zc:+.2f}")
    assert abs(zm) <= 5.0 and abs(zc) <= 5.0
    assert all(r["ncoal"][0] == 0 and r["ncoal"][1] + r["ncoal"][2] == 1 for r in reps)
    assert all(r["ncoal"][1] == 0 or r["migs"] for r in reps)                  # no coalescence in B without the migration
    assert all(mg[1:4] == (0, 1, 0) and 0 < mg[4] < tau for r in reps for mg in r["migs"])


# ---------------------------------------------------------------- 2: goldens, bit for bit
@pytest.mark.parametrize("name", ["m3", "v8", "a7", "j3", "sample", "stress"])
def test_records_accumulators_and_rows_equal_the_restatement(hostemu, tmp_path, name):
    r = check_case(hostemu[1], name, tmp_path)
    if name == "a7":
        assert (r["trees"]["age"][:, :, :r["pack"].n] > 0).any(), "no leaf above age 0"
        assert any(rep and max(rep["age"][:r["pack"].n]) > 0 for rep in r["last"])
    if name == "m3":
        assert any(rep and rep["migs"] for rep in r["last"]), "no replicate of the last sample has a migration"


def test_replicates_of_72_leaves(hostemu_big, tmp_path):
    check_case(hostemu_big, "n7", tmp_path, loci=[0, 1])


# ---------------------------------------------------------------- 3: the migration cap
def test_attempts_beyond_the_cap_are_redrawn(hostemu, edge_base, tmp_path):
    m = edge_models()["cap"]
    abandoned = sum(attempt(m, attempt_key(99, g, t, 0))[0] == 1 for g in range(3) for t in range(24))
    assert 0 < abandoned < 3 * 24, "the model does not exercise the retry"
    r, _ = check_edge_model(hostemu[1], edge_base, tmp_path, "cap")
    assert r["retried"] > 0 and all(rep is None or len(rep["migs"]) <= MAX_MIGS for rep in r["last"])
    assert (r["recs"][24]["num_migs"] <= MAX_MIGS).all()


def test_a_replicate_whose_every_attempt_fails_is_counted_and_left_out(hostemu, edge_base, tmp_path):
    r, m = check_edge_model(hostemu[1], edge_base, tmp_path, "all-fail", iters=3)
    assert all(attempt(m, attempt_key(99, 0, 0, a))[0] == 1 for a in range(16))
    e = r["si"][3]
    assert e["failed"].tolist() == [3.0, 3.0, 3.0] and not e["acc"].any() and not e["site_acc"][:, :, 1:].any()
    K, B = 3, 2
    assert [[int(v) for v in row] for row in r["rows"][1]] == [[0] * (2 * (K + B) + 3) + [3] + [0] * 4] * 3
    assert (r["recs"][3]["root"] == -1).all() and r["oob"][0] == 0


# ---------------------------------------------------------------- 4: the boundaries
@pytest.mark.parametrize("which", ["inner-band", "late-samples", "shared-ages"])
def test_boundaries(hostemu, edge_base, tmp_path, which):
    r, m = check_edge_model(hostemu[1], edge_base, tmp_path, which)
    reps = [simulate(m, 99, g, t) for g in range(3) for t in range(24)]
    migs = [mg for rep in reps if rep for mg in rep["migs"]]
    assert migs, "no migration: the bands are not exercised"
    for br, b, sp, tp, ag in migs:
        assert m["bandStart"][b] <= ag < m["bandEnd"][b]
    if which == "inner-band":
        assert all(b == 0 and 0.004 <= ag < 0.012 for _, b, _, _, ag in migs)
    if which != "inner-band":
        assert all(rep["age"][2] == rep["age"][3] == m["sampleAge"][1] > 0 for rep in reps if rep)
        for rep in reps:                         # before B's samples enter, only a lineage that came into B through band 0 can leave it
            inB = 0
            for _, b, _, _, ag in rep["migs"] if rep else []:
                if ag < m["sampleAge"][1]:
                    inB += 1 if b == 0 else -1
                    assert inB >= 0


# ---------------------------------------------------------------- 5 - 8: seed, selections, lifecycle, sites off
def test_seed_decides_the_replicates(hostemu, tmp_path):
    check_seed(hostemu[1], tmp_path)


def test_selections(hostemu, tmp_path):
    check_selections(hostemu[1], tmp_path)


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


def test_a_locus_whose_site_sums_could_pass_32_bits_is_refused_by_name(hostemu, edge_base, capfd):
    check_refused_locus(hostemu[1], edge_base, capfd)


def test_without_sites_the_genealogy_level_is_identical(hostemu, tmp_path):
    check_sites_off(hostemu[1], tmp_path)


# ---------------------------------------------------------------- 9: the chain is untouched
@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    on, off = check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path, predictive=(name == "m3"))
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]


# ---------------------------------------------------------------- 10: the program and the launcher
def test_program_writes_the_two_simulate_files(hostemu, tmp_path):
    from simulate_util import check_program
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def test_ranks_join_to_the_one_rank_files(hostemu, tmp_path):
    from simulate_util import check_ranks
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_simulate_files(hostemu, tmp_path):
    from simulate_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
