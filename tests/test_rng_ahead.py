"""The sweep's uniforms generated ahead of it (k_rng_ahead + GphRngA), on the host-emulation build.

The pass must change nothing: the random stream, the records and every byte of the per-locus state are those of the serial
generator whichever path serves a draw -- the buffer, the in-kernel chunks behind it, or only those.  Every setting below is
compared with the run that has the pass switched off (GPH_RNG_AHEAD=0: the serial generator of every other kernel), after
every iteration, so the generator state a sweep leaves in the page is checked each time and not only at the end."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from rng_ahead_util import ENV, ahead

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

CASES = {"m3": 40, "a7": 40, "j1": 50, "stress": 6}
SETTINGS = {
    "off": {"GPH_RNG_AHEAD": "0"},
    "on": {},
    "m64": {"GPH_RNG_AHEAD_DRAWS": "64"},            # nearly every locus runs past its draws
    "first0": {"GPH_RNG_AHEAD_FIRST": "0"},          # a first sweep with no draws ahead at all: everything from the in-kernel chunks
    "ckpt64": {"GPH_RNG_AHEAD_CKPT": "64"},          # the other checkpoint distance
    "m64ckpt64": {"GPH_RNG_AHEAD_DRAWS": "64", "GPH_RNG_AHEAD_CKPT": "64"},
}


@pytest.fixture(scope="module")
def lib():
    import run_hostemu as R
    import gphocs_amd as G
    return G.load_library(R.build_hostemu())


def run(lib, name, iters, env, tmp, monkeypatch, before=None):
    """records, the state dump after every iteration, the draw counts of every sweep [iters][L], the pass's settings"""
    import gphocs_amd as G
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = G.Sampler(G.Pack.load(os.path.join(GOLDEN, name + ".gpk")), lib=lib)
    tr, st = os.path.join(tmp, "t"), os.path.join(tmp, "s")
    s.set_record_file(tr)
    s.initialize()
    info = ahead(lib, s)
    states, counts = [], []
    for it in range(iters):
        if before:
            before(s, it)
        s.iteration(it)
        s.dump_state(st, it == iters - 1)       # the last one with the conditional arrays
        states.append(open(st, "rb").read())
        if info[0]:
            kp = np.zeros(s.end - s.begin, dtype=np.int32)
            ahead(lib, s, kp)
            counts.append(kp)
    s.set_record_file(None)
    assert s.debug_oob()[0] == 0
    s.close()
    return open(tr, "rb").read(), states, np.array(counts), info


@pytest.fixture(scope="module")
def reference(lib, tmp_path_factory):
    """the run with the pass off, once per golden"""
    cache = {}

    def get(name):
        if name not in cache:
            mp = pytest.MonkeyPatch()
            try:
                cache[name] = run(lib, name, CASES[name], SETTINGS["off"], str(tmp_path_factory.mktemp("ref_" + name)), mp)
            finally:
                mp.undo()
            assert cache[name][3][0] == 0
        return cache[name]
    return get


def same(got, ref):
    assert got[0] == ref[0], "records differ"
    for it, (a, b) in enumerate(zip(got[1], ref[1])):
        assert a == b, f"state after iteration {it} differs"
    assert len(got[1]) == len(ref[1])


@pytest.mark.parametrize("setting", [k for k in SETTINGS if k != "off"])
@pytest.mark.parametrize("name", list(CASES))
def test_same_bytes_whichever_path_serves_the_draws(lib, reference, name, setting, tmp_path, monkeypatch):
    got = run(lib, name, CASES[name], SETTINGS[setting], str(tmp_path), monkeypatch)
    on, M, Cd, _ = got[3]
    assert on == 1 and M == int(SETTINGS[setting].get("GPH_RNG_AHEAD_DRAWS", 512)) and Cd == int(SETTINGS[setting].get("GPH_RNG_AHEAD_CKPT", 16))
    same(got, reference(name))
    counts = got[2]
    assert counts.shape == (CASES[name], len(counts[0])) and counts.max() > 0
    if setting in ("m64", "m64ckpt64"):
        assert (counts > 64).mean() > 0.5, "M = 64 was meant to make most loci run past their draws"
    if setting == "on":
        # draws kept for a sweep: min(M, roundup64(previous count + 64)), the first sweep 320; most sweeps must be served from them
        n_ahead = np.minimum(M, (np.vstack([np.full((1, counts.shape[1]), 256), counts[:-1]]) + 64 + 63) // 64 * 64)
        assert (counts <= n_ahead).mean() > 0.5


def test_first_sweep_without_draws_ahead(lib, tmp_path, monkeypatch):
    """GPH_RNG_AHEAD_FIRST=0: the first pass generates nothing (and still leaves the state where the in-kernel chunks start)"""
    got = run(lib, "m3", 2, SETTINGS["first0"], str(tmp_path), monkeypatch)
    assert got[3][0] == 1 and got[2][0].min() > 0


def test_counts_that_end_on_a_checkpoint_and_on_the_last_draw_ahead(lib, reference, tmp_path, monkeypatch):
    """a locus that consumes an exact multiple of C draws (the checkpoint is the state: no replay), and one that consumes
    exactly the draws generated for it (the last checkpoint, nothing from the in-kernel chunks): the first is found among the
    recorded counts of the plain run, the second is made by setting the locus's count of the sweep before through the test
    hook, so that min(M, roundup64(count + 64)) is what the locus is going to consume"""
    name, iters = "j1", CASES["j1"]
    ref = reference(name)
    plain = run(lib, name, iters, SETTINGS["on"], str(tmp_path), monkeypatch)
    counts, (_, M, Cd, _) = plain[2], plain[3]
    same(plain, ref)
    n_ahead = np.minimum(M, (np.vstack([np.full((1, counts.shape[1]), 256), counts[:-1]]) + 64 + 63) // 64 * 64)
    on_ckpt = (counts > 0) & (counts % Cd == 0) & (counts <= n_ahead)
    assert on_ckpt.any(), "no locus-sweep of this run ends on a checkpoint: choose another golden"
    cand = np.argwhere((counts > 0) & (counts % 64 == 0) & (counts <= M))
    assert len(cand) > 0, "no locus-sweep of this run consumes a multiple of 64 draws: choose another golden"
    it0, locus = (int(v) for v in cand[0])
    hit = []

    def before(s, it):
        if it == it0:
            kp = np.zeros(s.end - s.begin, dtype=np.int32)
            ahead(lib, s, kp)
            kp[locus] = counts[it0, locus] - 64
            ahead(lib, s, kp, set_=True)
            hit.append(it)
    forced = run(lib, name, iters, SETTINGS["on"], str(tmp_path), monkeypatch, before=before)
    assert hit == [it0] and forced[2][it0, locus] == counts[it0, locus]
    same(forced, ref)
    assert (forced[2] == counts).all()


def test_off_is_the_serial_generator(lib, reference):
    """GPH_RNG_AHEAD=0 on the host build: no buffers, the generator of every other kernel"""
    assert reference("m3")[3] == (0, 0, 1, 0)


def test_capacity_statement(lib, tmp_path, monkeypatch):
    """bytes per locus of the pass's buffers: M doubles, M / C + 1 checkpoints and the tail of 16 bytes, a count"""
    got = run(lib, "m3", 1, SETTINGS["on"], str(tmp_path), monkeypatch)
    assert got[3] == (1, 512, 16, 512 * 8 + 16 * (512 // 16 + 1) + 16 + 4)


def test_allocation_failure_switches_the_pass_off(lib, reference, tmp_path, monkeypatch, capfd):
    """GPH_RNG_AHEAD_FAIL_ALLOC=1: the buffers are not to be had -- one line on stderr, the engine runs on without the pass"""
    got = run(lib, "m3", CASES["m3"], {"GPH_RNG_AHEAD_FAIL_ALLOC": "1"}, str(tmp_path), monkeypatch)
    assert got[3] == (0, 0, 1, 0)
    same(got, reference("m3"))
    assert capfd.readouterr().err.count("draws ahead of the sweep") == 1


def _build_sanitizer_program():
    """tests/hostemu/rng_ahead_san: its own main() and the host build of the engine sources under AddressSanitizer and
    UndefinedBehaviorSanitizer, with the index checks of the checked build; rebuilt when a source changes (by content)"""
    import hashlib
    import subprocess
    csrc = os.path.join(REPO, "g-phocs_amd", "csrc")
    main = os.path.join(REPO, "tests", "hostemu", "rng_ahead_san.cpp")
    srcs = [os.path.join(csrc, f) for f in ("gph_engine.hip", "gph_mcmc.cpp", "gph_input.cpp", "gph_program.cpp", "gph_readtrace.cpp", "gph_comm.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [main, os.path.join(REPO, "include", "gphocs_hip.h")]
    h = hashlib.sha256()
    for d in sorted(deps):
        h.update(os.path.basename(d).encode() + b"\0" + open(d, "rb").read())
    want, exe = h.hexdigest()[:16], os.path.join(REPO, "tests", "hostemu", "rng_ahead_san")
    try:
        if os.path.exists(exe) and open(exe + ".buildid").read().strip() == want:
            return exe
    except OSError:
        pass
    tmp = f"{exe}.tmp.{os.getpid()}"
    cmd = ["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DGPH_BOUNDS",
           "-O1", "-g", "-std=c++17", "-DGPH_HOSTEMU", "-DGPH_LOGSTEPS", "-DGPH_CAP_LEAVES=32", "-DGPH_CAP_K=32", "-DGPH_CAP_B=16",
           "-ffp-contract=off", "-pthread", main, "-x", "c++"] + srcs + ["-lrt", "-ldl", "-o", tmp]
    try:
        subprocess.run(cmd, check=True)
        os.replace(tmp, exe)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    with open(exe + ".buildid", "w") as f:
        f.write(want + "\n")
    return exe


def test_sanitizer_program(tmp_path):
    """the stand-alone program of tests/hostemu/rng_ahead_san.cpp (golden m3, 20 iterations, the pass off against 64 draws
    ahead) under AddressSanitizer / UndefinedBehaviorSanitizer: a process of its own, nothing of it is loaded into python"""
    import subprocess
    exe = _build_sanitizer_program()
    env = {k: v for k, v in os.environ.items() if k not in ENV and k != "LD_PRELOAD"}
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rng_ahead_san OK" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
