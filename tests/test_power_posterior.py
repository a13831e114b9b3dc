"""Power-posterior (heated) chains on the CPU: Sampler.set_beta on the host build of the engine sources (tests/hostemu).

beta scales the data term of the five acceptance ratios that have one -- sweep_internal, sweep_spr, the locus-rate scan, the
tau / sample-age finish, the mixing finish -- and nothing else.  The identities of power_posterior_util.py check that bit for
bit, against chains at beta = 1 on packs whose pattern counts are multiplied by 2 or by 0:

  A  beta = 1/2 on doubled counts  is the chain of  beta = 1 on the pack   (recorded data log-likelihoods exactly doubled)
  B  beta = 2 on the pack          is the chain of  beta = 1 on doubled counts
  C  beta = 0 on the pack          is the chain of  beta = 1 on counts 0   (a pack with no information: the prior)
  D  set_beta(1.0), before initialize or in mid-run, leaves every byte of the state dump as it is without the call

m3 (migration bands, SPR traffic), v8 (locus-mut-rate VAR) and a7 (an estimated sample age) cover the five places between
them; all three have mixing on.  Each shows, at beta = 1, accepted and rejected proposals of every kind it is there for
(covered()).  m3 also runs on the host builds with the capacities of the big-tree and many-band library variants and on the
64-lane fiber wave.  E: two ranks (gloo) at beta = 1/2 equal one rank."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest

from conftest import REPO
from parity_util import compare_records
import power_posterior_util as U

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

BUILDS = {"default": dict(), "mid": dict(mid=True), "big": dict(big=True), "wave64": dict(wave64=True)}
CASES = [("default", n) for n in U.FIXTURES] + [(b, "m3") for b in ("mid", "big", "wave64")]
WAVE64_ITERS = 6      # the fiber wave runs a quarter of a second per iteration: the fewest at which m3 still covers its kinds
_libs, _runs = {}, {}


def iterations(build, name):
    return WAVE64_ITERS if build == "wave64" else U.FIXTURES[name][0]


def library(build):
    if build not in _libs:
        import run_hostemu
        import gphocs_amd as G
        _libs[build] = G.load_library(run_hostemu.build_hostemu(**BUILDS[build]))
    return _libs[build]


def chains(build, name):
    """the four chains A and B compare, run once per (build, fixture): pack and doubled pack at beta = 1 (set_beta never
    called), doubled at 1/2, pack at 2; and the state dump of the first for D"""
    key = (build, name)
    if key not in _runs:
        lib, iters = library(build), iterations(build, name)
        p = U.load(name)
        d = U.scaled_counts(p, 2)
        with tempfile.TemporaryDirectory() as td:
            one = U.run(lib, p, iters, dump=os.path.join(td, "one.state"))
            dump = open(os.path.join(td, "one.state"), "rb").read()
        _runs[key] = dict(pack=p, one=one, dump=dump, dbl=U.run(lib, d, iters), dbl_half=U.run(lib, d, iters, beta=0.5),
                          two=U.run(lib, p, iters, beta=2.0))
    return _runs[key]


@pytest.mark.parametrize("build,name", CASES)
def test_fixture_covers_its_proposals(build, name):
    r = chains(build, name)
    U.covered(r["pack"], iterations(build, name), r["one"], U.FIXTURES[name][1])
    # and the data matter to the chain: twice the counts give another one
    assert r["one"]["accept"] != r["dbl"]["accept"]


@pytest.mark.parametrize("build,name", CASES)
def test_a_half_on_doubled_counts(build, name):
    r = chains(build, name)
    assert r["dbl_half"]["beta"] == 0.5
    U.same_chain(r["one"], r["dbl_half"])
    U.data_scaled(r["one"], r["dbl_half"], 2.0)


@pytest.mark.parametrize("build,name", CASES)
def test_b_two_on_the_pack(build, name):
    r = chains(build, name)
    U.same_chain(r["dbl"], r["two"])
    U.data_scaled(r["two"], r["dbl"], 2.0)


@pytest.mark.parametrize("build,name", CASES)
def test_c_zero_is_the_prior(build, name):
    lib, iters = library(build), iterations(build, name)
    p = chains(build, name)["pack"]
    blank = U.run(lib, U.scaled_counts(p, 0), iters)
    zero = U.run(lib, p, iters, beta=0.0)
    assert blank["dataLogLikelihood"] == 0.0 and not blank["treeDataLnL"].any()
    U.same_chain(blank, zero)
    assert zero["dataLogLikelihood"] != 0.0           # what the chain records stays the plain likelihood
    assert zero["accept"] != chains(build, name)["one"]["accept"]


@pytest.mark.parametrize("build,name", CASES)
def test_d_beta_one_changes_nothing(build, name, tmp_path):
    lib, iters = library(build), iterations(build, name)
    p, plain, want = (chains(build, name)[k] for k in ("pack", "one", "dump"))
    before = U.run(lib, p, iters, beta=1.0, dump=str(tmp_path / "before.state"))
    midrun = U.run(lib, p, iters, beta=1.0, beta_from=iters // 2, dump=str(tmp_path / "midrun.state"))
    assert len(want) > 1000
    assert (tmp_path / "before.state").read_bytes() == want and (tmp_path / "midrun.state").read_bytes() == want
    for r in (before, midrun):
        U.same_chain(plain, r)
        U.data_scaled(plain, r, 1.0)


def test_beta_takes_effect_from_the_next_call():
    """set in mid-run, beta leaves the iterations before it alone and changes those after it"""
    lib, (iters, _) = library("default"), U.FIXTURES["m3"]
    p = chains("default", "m3")["pack"]
    late = U.run(lib, p, iters, beta=0.25, beta_from=iters)        # never reached
    U.same_chain(chains("default", "m3")["one"], late)
    mid = U.run(lib, p, iters, beta=0.25, beta_from=iters // 2)
    assert mid["accept"] != late["accept"] and mid["beta"] == 0.25


def test_beta_range():
    import gphocs_amd as G
    s = G.Sampler(U.load("m3"), lib=library("default"))
    try:
        assert s.beta == 1.0
        for bad in (-0.5, 64.5, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(RuntimeError):
                s.set_beta(bad)
            assert s.beta == 1.0
        for good in (0.0, 64.0, 0.3):
            s.set_beta(good)
            assert s.beta == good
        b = ctypes.c_double()
        assert s.lib.gph_engine_get_beta(s.engine, ctypes.byref(b)) == 0 and b.value == 0.3
        assert s.lib.gph_engine_set_beta(s.engine, 65.0) != 0 and s.lib.gph_mcmc_set_beta(None, 1.0) != 0
    finally:
        s.close()


# ---------------------------------------------------------------- E: rank invariance
WORKER = r'''
import os, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, os.path.join(%(repo)r, "tests")); sys.path.insert(0, os.path.join(%(repo)r, "tests", "hostemu"))
import numpy as np, torch, torch.distributed as dist
import gphocs_amd as G, run_hostemu as R
import power_posterior_util as U
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
def allreduce(sums, mins):
    if sums.size:
        t = torch.from_numpy(sums); dist.all_reduce(t, op=dist.ReduceOp.SUM)
    if mins.size:
        t = torch.from_numpy(mins); dist.all_reduce(t, op=dist.ReduceOp.MIN)
s = G.Sampler(U.load(%(name)r), lib=G.load_library(R.build_hostemu()), rank=rank, world=world, allreduce=allreduce)
s.set_beta(0.5)                      # every rank the same value
s.set_record_file(%(out)r + ".%%d" %% rank)
s.initialize()
for it in range(%(iters)d):
    s.iteration(it)
s.set_record_file(None)
s.close()
dist.destroy_process_group()
'''


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def test_e_two_ranks_equal_one_rank(tmp_path):
    """v8: the locus-rate scan is chained through the ranks, and every rank's scan multiplies by its own copy of beta"""
    import gphocs_amd as G
    name, (iters, _) = "v8", U.FIXTURES["v8"]
    lib = library("default")

    def record(path, beta):
        s = G.Sampler(U.load(name), lib=lib)
        if beta is not None:
            s.set_beta(beta)
        s.set_record_file(path)
        s.initialize()
        for it in range(iters):
            s.iteration(it)
        s.set_record_file(None)
        s.close()
        return open(path).read()
    one = str(tmp_path / "one")
    assert record(one, 0.5) != record(str(tmp_path / "plain"), None)      # it is a heated chain that is compared
    out = str(tmp_path / "rec")
    script = tmp_path / "worker.py"
    script.write_text(WORKER % dict(repo=REPO, name=name, out=out, iters=iters))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    assert open(out + ".0").read() == open(out + ".1").read()
    compare_records(out + ".0", one)            # accept counters exact, sums over loci to 1e-10: the reduction order differs
