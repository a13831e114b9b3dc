"""Effective sample sizes (gph_ess, gph_ess_read, gph_engine_ess_*) on the CPU: the host-emulation build of the engine sources
runs k_ess' workgroup body over the same pages.

The device's accumulators are held to the definitions of include/gphocs_hip.h by an independent restatement (tests/ess_util.py):
one chain samples its gene trees (k_gene_trees; tests/test_gene_trees.py holds those records to the state dumps) and its ESS
accumulators after every iteration, and plain Python rebuilds every word from the decoded records alone -- the five (six)
series, gph_ess_add on each, clade sets by father climbs for the focal set, the topo series and topoChanges.  Every double is
compared as float.hex, every integer exactly, after 1, 2, 37 and 64 samples.

Cases: m3 (the default build), x8 (32 leaves: G = 8 records a workgroup), v8 (locus-mut-rate VAR: the rate series), a70
(synthetic, 70 loci of 8 leaves: G = 32, a partial last group); n7 (72 leaves, two key words, G = 3) and t136 (synthetic, 136
leaves: G = 1, three key words) on the host build with the reference's own caps.  The largest shape the kernel is built for,
200 leaves with four key words, has no fixture: its LDS need is the formula of csrc/gph_ess.h."""
import math
import os
import sys

import pytest

from conftest import REPO
from ess_util import (CHECKPOINTS, ar1, check_case, check_chain_untouched, check_failed_runs_leave_nothing, check_levels, check_lifecycle, check_program,
                      check_ranks, check_selections, ess_series, same_bits)
from sampler_util import hostemu_library
from test_ancestry import GOLDEN_ITERS

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

AR1_SEED = 20161020     # fixed after the Python model alone was seen inside the bound (test_ar1_tau_is_near_its_true_value)


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


# ---------------------------------------------------------------- item 1: the device's accumulators against the model
@pytest.mark.parametrize("name", ["m3", "x8", "v8", "a70"])
def test_accumulators_equal_the_model_over_the_gene_tree_records(hostemu, name):
    r, _ = check_case(hostemu[1], name)
    e = r["ess"][64]
    assert len(e["series"]) == (6 if name == "v8" else 5)
    if name == "a70":
        assert r["pack"].L == 70 and 70 % (256 // r["pack"].n) != 0


@pytest.mark.parametrize("name,iters", [("n7", 37), ("t136", 4)])
def test_accumulators_of_many_leaves(hostemu_big, name, iters):
    """n7: two key words; t136: one record a workgroup, three key words (fewer samples: the host emulation of 136 leaves is slow)"""
    r, model = check_case(hostemu_big, name, iters, checkpoints=[c for c in CHECKPOINTS if c <= iters])
    words = r["ess"][iters]["words"]
    assert words == (3 if name == "t136" else 2)
    assert any(k >> (64 * (words - 1)) and k & ((1 << 64) - 1) for m in model for k in m["focal"]), "no focal key with bits in the first and the last word"


def test_selections(hostemu):
    check_selections(hostemu[1])


# ---------------------------------------------------------------- item 2: gph_ess against its restatement
def _both(lib, x, max_lag=0):
    import gphocs_amd as G
    got, want = G.ess(x, max_lag, lib=lib), ess_series(x, max_lag)
    same_bits(got, want, f"S {len(x)} max_lag {max_lag}")
    return got


def test_gph_ess_equals_its_restatement(hostemu):
    import gphocs_amd as G
    lib = hostemu[1]
    x = ar1(4099, 0.9, AR1_SEED)
    r = _both(lib, x)
    assert r["level"] == 6 and r["truncated"] == 0 and 1.0 < r["tauAcf"] and r["essAcf"] < 4099
    r = _both(lib, x, 5)                         # a small max_lag ends the sum
    assert r["truncated"] == 1
    r = _both(lib, [2.5] * 100)                  # a constant series: ess 0, never "perfectly mixed"
    assert (r["essBatch"], r["essAcf"], r["tauBatch"], r["tauAcf"], r["sd"]) == (0.0, 0.0, 0.0, 0.0, 0.0) and r["mean"] == 2.5
    r = _both(lib, [(-1.0) ** t for t in range(200)])      # alternating: negative correlation, capped at S
    assert r["essBatch"] == 200.0 and r["essAcf"] == 200.0
    _both(lib, [1.0, 3.0])
    _both(lib, [1.0, 3.0, 2.0])
    _both(lib, [0.1 * t * t for t in range(17)])
    for bad in ([], [1.0]):
        with pytest.raises(ValueError):
            G.ess(bad, lib=lib)
    assert lib.gph_ess(None, 10, 0, None) == -1


def test_ar1_tau_is_near_its_true_value(hostemu):
    """AR(1) with phi = 0.9 has tau = (1 + phi) / (1 - phi) = 19.  At S = 65536 the batch level is 8 (256 batches of 256), whose
    estimate has a relative standard deviation of about sqrt(2 / 255) = 0.089 plus a bias of about -tau / batch = -7 %: the
    bound [19 / 1.6, 19 * 1.6] is five standard deviations wide.  The model alone is checked first"""
    x = ar1(65536, 0.9, AR1_SEED)
    want = ess_series(x)
    assert want["level"] == 8
    for k in ("tauBatch", "tauAcf"):
        print(k, want[k])
        assert 19 / 1.6 <= want[k] <= 19 * 1.6, f"the model's {k} = {want[k]}"
    got = _both(hostemu[1], x)
    assert 19 / 1.6 <= got["tauBatch"] <= 19 * 1.6 and 19 / 1.6 <= got["tauAcf"] <= 19 * 1.6
    assert math.isclose(got["essAcf"], 65536 / got["tauAcf"])


# ---------------------------------------------------------------- item 3: the read-out
def test_read_out_and_the_level_rule(hostemu):
    check_levels(hostemu[1])


# ---------------------------------------------------------------- item 4: the chain is untouched
@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    on, off = check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]


# ---------------------------------------------------------------- item 6: lifecycle
def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


# ---------------------------------------------------------------- item 5: the program and the launcher
def test_program_writes_the_two_ess_files(hostemu, tmp_path):
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def test_ranks_concatenate_to_the_one_rank_files(hostemu, tmp_path):
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_ess_files(hostemu, tmp_path):
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
