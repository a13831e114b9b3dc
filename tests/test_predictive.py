"""Posterior predictive checks (gph_engine_predictive_*) on the CPU: the host-emulation build of the engine sources runs
k_predictive's workgroup body, the device text itself, over the same pages and sequence blocks.

The device's accumulators, rows and observed values are held to the definitions of include/gphocs_hip.h by an independent
restatement (tests/predictive_util.py): one chain samples its gene trees and its predictive accumulators after every iteration,
and plain Python / numpy rebuilds every word from the decoded records, the rates and the pack alone.  Every double is compared
as float.hex, every integer exactly.  The restatement itself is pinned first: its pair differences against JC69's expectation,
and its statistics' invariance under the phases of a group.

Cases: m3 (baseline), v8 (locus-mut-rate VAR), a7 (ancient samples: leaf ages > 0), j3 (4 current populations), sample (groups of
2 phases), stress (13 leaves, groups of up to 32 phases), bigp (more than 64 rows a locus); n7 (72 leaves, loci 0 and 1) on the
host build with the reference's own caps; hand-made packs for the edges of the site loop."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from predictive_util import (check_case, check_chain_untouched, check_edges, check_lifecycle, check_refused_locus, check_seed, check_selections,
                             edge_model, leaf_pops, model_pair_differences, phase_groups, statistics)
from sampler_util import hostemu_library, load_pack
from test_ancestry import GOLDEN_ITERS

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))


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
    return edge_model(tmp_path_factory.mktemp("edge"), hostemu[1])


# ---------------------------------------------------------------- the model, pinned by itself
def test_model_pair_differences_follow_jc69():
    """400 000 sites of a fixed 3-leaf tree: each pair's difference frequency within 5 binomial standard errors of
    3/4 (1 - exp(-4 rate d / 3)), d = 2 age(lca) - age_i - age_j"""
    sites = 400000
    for diff, p in model_pair_differences(sites):
        z = (diff / sites - p) / math.sqrt(p * (1 - p) / sites)
        print(f"differences {diff} expected {p * sites:.1f} z {z:+.2f}")
        assert abs(z) <= 5.0


@pytest.mark.parametrize("name", ["sample", "stress", "bigp"])
def test_model_statistics_do_not_depend_on_the_phase(name):
    """every row of every group of more than one phase gives the first row's statistics and N positions"""
    pk = load_pack(name)
    pops, groups = leaf_pops(pk), phase_groups(pk)
    assert groups, f"{name} has no group of more than one phase"
    for g, r, k in groups:
        rows = pk.leafcodes[r:r + k].astype(np.int64)
        want = statistics(rows[:1].T, rows[:1].T == 4, pops, pk.Kc)
        for j in range(1, k):
            assert ((rows[j] == 4) == (rows[0] == 4)).all(), f"{name} locus {g} row {r + j}: N positions"
            assert statistics(rows[j:j + 1].T, rows[j:j + 1].T == 4, pops, pk.Kc) == want, f"{name} locus {g} row {r + j}"
    print(f"{name}: {len(groups)} groups, up to {max(k for _, _, k in groups)} phases")


# ---------------------------------------------------------------- 1: goldens, bit for bit
@pytest.mark.parametrize("name", ["m3", "v8", "a7", "j3", "sample", "stress", "bigp"])
def test_accumulators_rows_and_observed_equal_the_model(hostemu, name):
    r, _ = check_case(hostemu[1], name)
    if name == "a7":
        assert (r["trees"]["age"][:, :, :r["pack"].n] > 0).any(), "no leaf above age 0"
    if name == "bigp":
        assert int(np.diff(r["pack"].pattern_offsets).max()) > 64


def test_accumulators_of_72_leaves(hostemu_big):
    check_case(hostemu_big, "n7", loci=[0, 1])


# ---------------------------------------------------------------- 2: the site loop's edges
@pytest.mark.parametrize("big_count", [False, True])
def test_site_loop_edges(hostemu, edge_base, big_count):
    check_edges(hostemu[1], edge_base, big_count)


def test_a_locus_whose_sums_could_pass_32_bits_is_refused_by_name(hostemu, edge_base, capfd):
    check_refused_locus(hostemu[1], edge_base, capfd)


# ---------------------------------------------------------------- 3: selections, reset, limits
def test_selections(hostemu):
    check_selections(hostemu[1])


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


# ---------------------------------------------------------------- 4: the seed
def test_seed_decides_the_replicates(hostemu):
    check_seed(hostemu[1])


# ---------------------------------------------------------------- 5: the chain is untouched
@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    on, off = check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]


# ---------------------------------------------------------------- 6: the program and the launcher
def test_program_writes_the_two_predictive_files(hostemu, tmp_path):
    from predictive_util import check_program
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def test_ranks_join_to_the_one_rank_files(hostemu, tmp_path):
    from predictive_util import check_ranks
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_predictive_files(hostemu, tmp_path):
    from predictive_util import check_failed_runs_leave_nothing
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
