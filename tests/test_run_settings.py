"""Run settings beyond the one point every other fixture sits on ("What's missing" 4): tools/random_models.py
wide_model(k) takes the SHAPE of random_model(k) and draws the step sizes (every finetune-* over four decades around the value all
other control files use, finetune-tau over three), the missing-data rate (0 .. 30 % N), the locus length (120 .. 2000 bp), mixing
on / off, the locus rates (CONST / VAR / FIXED <rate file>) and haploid samples (`sN h`: one leaf, odd leaf counts).

Fixtures (tests/golden/wide/wKK.{gpk.gz,rtrace.gz,json}) come from the REAL reference: its pack and its per-proposal records
(gzip of the files tests/golden/rnd holds plain; unpacked once per run of this module); all of them are models the reference
runs to the end (its own aborts are tests/golden/rnd's).

 * not gpu: the fixture set reaches every setting (test_fixture_set_reaches_every_setting); the oracle reproduces every fixture's
   records byte for byte; the host build of the engine sources reproduces them (counters exact, sums over loci within 1e-10) and
   the live oracle's final per-locus state byte for byte; with all four statistics samplers taking a sample after every
   iteration the records and the final state are the bytes of the run without them; where oracle/_ref is present, 20 FRESH wide
   models go through the real reference and the oracle.
 * gpu: the same through the C ABI on the MI355X, with the tightest capacity variant per pack; three packs (30 % N, VAR,
   haploid) through the checked build, which must report no index out of range."""
import glob
import gzip
import json
import os
import sys

import pytest

from conftest import GOLDEN, REPO
from parity_util import ZERO_RESIDUE
from test_model_shapes import _check_engine, _check_oracle, _fresh_models

WIDE = os.path.join(GOLDEN, "wide")
MODELS = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(WIDE, "w*.json")))
META = {m: json.load(open(os.path.join(WIDE, m + ".json"))) for m in MODELS}

# each step size's range: `decades` wide, centred (in the logarithm) on the value of every fixture outside this family
FINETUNES = dict(coal_time=(0.01, 4), mig_time=(0.3, 4), theta=(0.04, 4), mig_rate=(0.02, 4), tau=(8e-7, 3), mixing=(0.003, 4))
VAR_FINETUNES = (0.03, 0.3, 3.0)

# a total over loci that is exactly 0.0 in the engine and a rounding residue in the reference (w45, once): parity_util.ZERO_RESIDUE.
# Every non-zero total is held to 1e-10, per-locus state stays byte for byte.
RESIDUE = ZERO_RESIDUE


def _leaves(meta):
    return 2 * sum(meta["model"]["pops"]) - len(meta["model"].get("haploid", ()))


def _pick(pred):
    got = [m for m in MODELS if pred(META[m])]
    assert got, "no such fixture"
    return got[0]


def _records(name):
    """-> [(iteration, kind, accept count)] of a fixture's IT lines"""
    out = []
    for l in gzip.open(os.path.join(WIDE, name + ".rtrace.gz"), "rt"):
        t = l.split()
        if t and t[0] == "IT":
            out.append((int(t[1]), t[2], int(t[3])))
    return out


def test_fixture_set_reaches_every_setting():
    import math
    assert 12 <= len(MODELS) <= 24
    assert not any(META[m]["reference_aborts"] for m in MODELS), "the wide set holds only models the reference runs to the end"
    run = {m: META[m]["run"] for m in MODELS}
    assert all(4 <= run[m]["loci"] <= 8 and 40 <= run[m]["iters"] <= 60 for m in MODELS)
    assert all(os.path.getsize(p) < 100000 for p in glob.glob(os.path.join(WIDE, "*")))
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(WIDE, "*"))) < 2000000
    assert sum(1 for m in MODELS if run[m]["nmask"] >= 0.1) >= 3
    assert sum(1 for m in MODELS if run[m]["nmask"] >= 0.3) >= 1
    assert sum(1 for m in MODELS if run[m]["no_mixing"]) >= 3
    assert sum(1 for m in MODELS if run[m]["rates"] == "VAR") >= 3
    assert sum(1 for m in MODELS if run[m]["rates"] == "FIXED") >= 3
    hap = [m for m in MODELS if META[m]["model"].get("haploid")]
    assert len(hap) >= 3 and any(_leaves(META[m]) % 2 for m in hap), "haploid samples, an odd leaf count among them"
    assert any(run[m]["seqlen"] == 2000 for m in MODELS) and any(run[m]["seqlen"] == 120 for m in MODELS)
    for key, (centre, decades) in FINETUNES.items():
        u = [math.log10(run[m]["finetune"][key] / centre) for m in MODELS]
        assert all(abs(x) <= decades / 2 + 1e-9 for x in u), key
        assert any(x < -decades / 2 + 1 for x in u), f"finetune-{key}: no fixture in the lowest decade of its range"
        assert any(x >= decades / 2 - 1 for x in u), f"finetune-{key}: no fixture in the highest decade of its range"
    var = [run[m]["var_rates"][1] for m in MODELS if run[m]["rates"] == "VAR"]
    assert min(var) == VAR_FINETUNES[0] and max(var) == VAR_FINETUNES[-1], "finetune-locus-rate: its lowest and its highest value"
    # every proposal kind accepted at least once and NOT accepted at least once, in the reference's own records.  A record
    # carries the accept count of one call; the number of proposals the call made is: INT one per internal node and locus,
    # SPR one per node and locus (see below), LRATE one per locus but the reference locus, THETA one per population, MIGR one
    # per band, TAUx / SAGEx / MIX one.  MIGN makes one per migration node: the fixture's .json carries how many the reference
    # held before its last iteration (reference_mig_nodes_before_last_iteration)
    acc, rej = set(), set()
    for m in MODELS:
        L, n, mo = run[m]["loci"], _leaves(META[m]), META[m]["model"]
        K, B = 2 * len(mo["pops"]) - 1, len(mo["bands"])
        bound = dict(INT=L * (n - 1), SPR=L * (2 * n - 1), LRATE=L - 1, THETA=K, MIGR=B, TAU=1, SAGE=1, MIX=1)
        # UpdateGB_MigSPR skips the node that is the root WHEN IT IS VISITED, and an accepted move can change the root: a sweep
        # proposes for up to all 2n - 1 nodes (w08 accepts 41 of "40"), and for at least n of them, since only the n - 1 internal
        # nodes can be a root.  Fewer than n acceptances per locus is therefore a refusal for certain
        least = dict(bound, SPR=L * n)
        last = run[m]["iters"] - 1
        for it, kind, a in _records(m):
            kind = kind.rstrip("0123456789")
            if kind in ("INIT", "CHECK"):
                continue
            # the bound is the number of proposals of the call (GPhoCS.c: UpdateGB_InternalNode loops over the n - 1 internal
            # nodes of every locus, UpdateGB_MigSPR over the 2n - 1 nodes, UpdateLocusRate over every locus but the
            # reference one, UpdateTheta over the populations, UpdateMigRates over the bands; n counts one leaf per haploid and
            # two per diploid sample, ancient ones included): no call may accept more than it proposed
            if kind != "MIGN":
                assert a <= bound[kind], (m, it, kind, a, bound[kind])
            elif it == last:
                assert a <= META[m]["reference_mig_nodes_before_last_iteration"], (m, it, kind, a)
            if a > 0:
                acc.add(kind)
            if kind == "MIGN":
                if it == last and a < META[m]["reference_mig_nodes_before_last_iteration"]:
                    rej.add(kind)
            elif a < least[kind]:
                rej.add(kind)
    kinds = {"INT", "MIGN", "SPR", "LRATE", "THETA", "MIGR", "TAU", "SAGE", "MIX"}
    assert acc == kinds, f"never accepted: {sorted(kinds - acc)}"
    assert rej == kinds, f"never refused: {sorted(kinds - rej)}"


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """the directory of the unpacked fixtures: wKK.gpk, wKK.rtrace"""
    d = tmp_path_factory.mktemp("wide")
    for m in MODELS:
        for ext in (".gpk", ".rtrace"):
            (d / (m + ext)).write_bytes(gzip.open(os.path.join(WIDE, m + ext + ".gz")).read())
    return str(d)


@pytest.mark.parametrize("name", MODELS)
def test_oracle_reproduces_the_reference_records(oracle_cli, wide, name, tmp_path):
    _check_oracle(oracle_cli, name, tmp_path, wide, META)


def _hostemu():
    sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))
    import run_hostemu as R
    import gphocs_amd as G
    # 20 leaves / 13 populations / 8 bands at most: the small host build (32 / 32 / 16)
    return G, G.load_library(R.build_hostemu())


@pytest.mark.parametrize("name", MODELS)
def test_host_build_on_wide_models(oracle_cli, wide, name, tmp_path):
    G, lib = _hostemu()
    _check_engine(G, lib, oracle_cli, name, tmp_path, wide, META, residue=RESIDUE)


def _tightest(G, wide, name):
    pk = G.Pack.load(os.path.join(wide, name + ".gpk"))
    return G.load_library(dims=(pk.n, pk.K, pk.B))


@pytest.fixture(scope="module")
def GPU():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_hip_on_wide_models(GPU, oracle_cli, wide, name, tmp_path):
    _check_engine(GPU, _tightest(GPU, wide, name), oracle_cli, name, tmp_path, wide, META, residue=RESIDUE)


def _checked_cases():
    if not MODELS:
        return []
    # three different packs
    return [_pick(lambda q: q["run"]["nmask"] >= 0.3 and q["run"]["rates"] != "VAR" and not q["model"].get("haploid")),
            _pick(lambda q: q["run"]["rates"] == "VAR" and not q["model"].get("haploid")),
            _pick(lambda q: q["model"].get("haploid") and _leaves(q) % 2 == 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _checked_cases())
def test_checked_build_finds_no_index_out_of_range(GPU, oracle_cli, wide, name, tmp_path):
    """30 % N, VAR rates, haploid samples with an odd leaf count: through the library compiled with -DGPH_BOUNDS"""
    G = GPU
    lib = G.load_library(os.path.join(REPO, "g-phocs_amd", G.CHECKED_LIB))
    assert lib.gph_build_id().decode().startswith("chk-")
    seen = []
    _check_engine(G, lib, oracle_cli, name, tmp_path, wide, META, residue=RESIDUE,
                  after=lambda s, k: seen.append(s.debug_oob()) if k == META[name]["run"]["iters"] - 1 else None)
    assert seen == [(0, 1)], f"index out of range at {seen} (source line + 100000 x file: 1 gph_locus.h, 2 gph_kernels.h)"


def _sampler_cases():
    if not MODELS:
        return []
    return [_pick(lambda q: q["run"]["no_mixing"]), _pick(lambda q: q["run"]["rates"] == "VAR" and not q["run"]["no_mixing"])]


def _with_all_samplers(G, lib, oracle_cli, wide, name, tmp_path):
    """all four statistics samplers on, a sample after every iteration: the chain's records and its final per-locus state are
    the BYTES of the run without them (and both runs are held to the reference's records and the oracle's state)"""
    it = META[name]["run"]["iters"]
    taken = []

    def before(s):
        s.enable_locus_summary(True)
        s.enable_coal_stats(it)
        s.enable_time_slices(4, it)
        s.enable_ancestry(it)

    def after(s, k):
        s.sample_locus_summary()
        s.sample_coal_stats(k)
        s.sample_time_slices(k)
        s.sample_ancestry(k)
        taken.append(k)
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    tr1, st1 = _check_engine(G, lib, oracle_cli, name, tmp_path / "on", wide, META, before, after, residue=RESIDUE)
    tr0, st0 = _check_engine(G, lib, oracle_cli, name, tmp_path / "off", wide, META, residue=RESIDUE)
    assert taken == list(range(it))
    assert open(tr1, "rb").read() == open(tr0, "rb").read(), "sampling changed the records"
    assert open(st1, "rb").read() == open(st0, "rb").read(), "sampling changed the final state"


@pytest.mark.parametrize("name", _sampler_cases())
def test_statistics_samplers_leave_the_chain_unchanged(oracle_cli, wide, name, tmp_path):
    G, lib = _hostemu()
    _with_all_samplers(G, lib, oracle_cli, wide, name, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _sampler_cases())
def test_statistics_samplers_leave_the_chain_unchanged_on_the_gpu(GPU, oracle_cli, wide, name, tmp_path):
    _with_all_samplers(GPU, _tightest(GPU, wide, name), oracle_cli, wide, name, tmp_path)


def test_fresh_wide_models_reference_vs_oracle(oracle_cli, ref_cli, tmp_path):
    """20 wide models that are NOT committed fixtures (ids 300-319), through the real reference and the oracle"""
    if ref_cli is None:
        pytest.skip("oracle/_ref/gphocs_ref not built: the committed fixtures cover this")
    assert not any(300 <= int(m[1:]) < 320 for m in MODELS)
    _fresh_models(oracle_cli, tmp_path, range(300, 320), wide=True)
