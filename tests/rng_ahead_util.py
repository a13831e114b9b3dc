"""What the tests of the sweep's draws ahead (k_rng_ahead + GphRngA) share: the generator written a second time, from its
description alone, in numpy -- nothing in here computes a draw or a state with the library under test -- the readers of
what the engine exposes (state dumps, the test hook gph_engine_rng_ahead_ and the fetch next to it), and the test bodies that
run against both builds: host emulation (tests/test_rng_ahead_stream.py) and the device (tests/test_rng_ahead_stream_gpu.py).

The generator: three 32-bit recurrences (x, y, z); a step is
    x = (171 x - 30269 (x // 177)) mod 2^32,  y = (172 y - 30307 (y // 176)) mod 2^32,  z = (170 z - 30323 (z // 178)) mod 2^32
and the draw after a step is r - floor(r) with r = x / 30269.0 + y / 30307.0 + z / 30323.0 in float64, summed in this order.
Everything is compared exactly: states as integers, draws as their 64-bit patterns."""
import ctypes as C

import numpy as np

ENV = ("GPH_RNG_AHEAD", "GPH_RNG_AHEAD_DRAWS", "GPH_RNG_AHEAD_CKPT", "GPH_RNG_AHEAD_FIRST", "GPH_RNG_AHEAD_FAIL_ALLOC", "GPH_RNG_AHEAD_PLACE")
GPH_ESTATE = -4        # include/gphocs_hip.h
_M32 = np.uint64(0xFFFFFFFF)

# counts written through the hook, side by side in one wavefront: -64 gives n = 0 (what GPH_RNG_AHEAD_FIRST=0 produces), the
# last three n = M at the default M = 512
VALS = (-64, -1, 0, 1, 63, 64, 65, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 449, 512, 4096, 1 << 20)
VALS_1024 = VALS + (960, 1023, 1024)


# (loci, mutation scale, settings, counts): 193 loci = three full wavefronts of the lane-per-locus pass plus one lane, and two
# launch groups of the sweep; then the sizes around one wavefront; then the other checkpoint distance and two other M
PASS_CASES = {
    "L193": (193, 26.0, {}, VALS),
    "L1": (1, 6.5, {}, VALS),
    "L63": (63, 6.5, {}, VALS),
    "L64": (64, 6.5, {}, VALS),
    "L65": (65, 6.5, {}, VALS),
    "L193-ckpt64": (193, 26.0, {"GPH_RNG_AHEAD_CKPT": "64"}, VALS),
    "L193-m64": (193, 26.0, {"GPH_RNG_AHEAD_DRAWS": "64"}, VALS),
    "L193-m1024": (193, 26.0, {"GPH_RNG_AHEAD_DRAWS": "1024"}, VALS_1024),
}


def expected_n(case):
    """every n the counts of a case must produce (a condition on VALS: the mixed counts do meet in one wavefront)"""
    _, _, env, vals = PASS_CASES[case]
    M = int(env.get("GPH_RNG_AHEAD_DRAWS", 512))
    return M, int(env.get("GPH_RNG_AHEAD_CKPT", 16)), set(int(v) for v in n_ahead(np.array(vals), M))


# ---------------------------------------------------------------- the independent generator
def step(s):
    """one step of every locus's generator; s: [L][3] uint64 holding 32-bit values"""
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    out = np.empty_like(s)
    out[:, 0] = (np.uint64(171) * x - np.uint64(30269) * (x // np.uint64(177))) & _M32
    out[:, 1] = (np.uint64(172) * y - np.uint64(30307) * (y // np.uint64(176))) & _M32
    out[:, 2] = (np.uint64(170) * z - np.uint64(30323) * (z // np.uint64(178))) & _M32
    return out


def draw_bits(s):
    """the draw that follows the step which left s, as uint64 bit patterns"""
    r = s[:, 0].astype(np.float64) / 30269.0 + s[:, 1].astype(np.float64) / 30307.0
    r = r + s[:, 2].astype(np.float64) / 30323.0
    return (r - np.floor(r)).view(np.uint64)


def stream(S0, steps):
    """states [steps + 1][L][3] (uint32, states[0] = S0) and draws [steps][L] (uint64 bit patterns) of every locus"""
    s = np.ascontiguousarray(S0, dtype=np.uint64).reshape(-1, 3)
    states = np.empty((steps + 1, len(s), 3), dtype=np.uint32)
    draws = np.empty((steps, len(s)), dtype=np.uint64)
    states[0] = s
    for d in range(steps):
        s = step(s)
        states[d + 1] = s
        draws[d] = draw_bits(s)
    return states, draws


def n_ahead(kprev, M):
    """draws the pass keeps for a locus that consumed kprev in its previous sweep: clip(roundup64(kprev + 64), 0, M)"""
    k = np.asarray(kprev, dtype=np.int64)
    return np.clip((k + 64 + 63) // 64 * 64, 0, M)


# ---------------------------------------------------------------- what the engine exposes
def parse_rng(dump):
    """[L][3] uint32: the generator state of every locus in a state dump (`LOCUS <id> ... rng <x> <y> <z>`), by locus id"""
    rows = {}
    for ln in dump.split(b"\n"):
        if ln.startswith(b"LOCUS "):
            t = ln.split()
            i = t.index(b"rng")
            assert int(t[1]) not in rows
            rows[int(t[1])] = [int(v) for v in t[i + 1:i + 4]]
    assert rows and sorted(rows) == list(range(min(rows), min(rows) + len(rows))), "the dump's loci are not one contiguous block"
    return np.array([rows[k] for k in sorted(rows)], dtype=np.uint32)


def dump(s, path, with_cond=False):
    s.dump_state(str(path), with_cond)
    with open(str(path), "rb") as f:
        return f.read()


def _hook(lib):
    fn = lib.gph_engine_rng_ahead_
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    return fn


def ahead(lib, s, kprev=None, set_=False):
    """(on, M, C, bytes per locus) and, if asked for, the per-locus draw counts (read, or written from `kprev`)"""
    fn = _hook(lib)
    info = np.zeros(4, dtype=np.int32)
    assert fn(s.engine, info.ctypes.data, None, 0) == 0
    if kprev is not None:
        assert kprev.dtype == np.int32 and len(kprev) == s.end - s.begin
        assert fn(s.engine, None, kprev.ctypes.data, int(set_)) == 0
    return tuple(int(v) for v in info)


def info_and_counts(s):
    """(on, M, C, bytes per locus) and the counts of the last sweep (None with the pass off)"""
    fn = _hook(s.lib)
    info = np.zeros(4, dtype=np.int32)
    assert fn(s.engine, info.ctypes.data, None, 0) == 0
    kp = None
    if info[0]:
        kp = np.zeros(s.end - s.begin, dtype=np.int32)
        assert fn(s.engine, None, kp.ctypes.data, 0) == 0
    return tuple(int(v) for v in info), kp


def counts(s):
    kp = np.zeros(s.end - s.begin, dtype=np.int32)
    ahead(s.lib, s, kp)
    return kp


def set_counts(s, kprev):
    ahead(s.lib, s, np.ascontiguousarray(kprev, dtype=np.int32), set_=True)


def side(s):
    """(the pass for the next sweep can run behind this one's kernel, such a pass stands): the hook with set = -1"""
    pair = np.zeros(4, dtype=np.int32)
    assert _hook(s.lib)(s.engine, pair.ctypes.data, None, -1) == 0
    return int(pair[0]), int(pair[1])


def _fetch_fn(lib):
    fn = lib.gph_engine_rng_ahead_fetch_
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def fetch(s):
    """the pass's buffers in input order: draws [L][M] as uint64 bit patterns, checkpoints [L][M / C + 1][4], tail [L][4]"""
    _, M, Cd, _ = ahead(s.lib, s)
    L = s.end - s.begin
    draws = np.zeros((L, M), dtype=np.float64)
    ckpt = np.zeros((L, M // Cd + 1, 4), dtype=np.uint32)
    tail = np.zeros((L, 4), dtype=np.uint32)
    assert _fetch_fn(s.lib)(s.engine, draws.ctypes.data, ckpt.ctypes.data, tail.ctypes.data) == 0
    return draws.view(np.uint64), ckpt, tail


def set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def synthetic_pack(G, config, loci, mut):
    """config 4: the call tests/test_rng_ahead_gpu.py makes for its data sets"""
    from gphocs_amd_pkg import synth
    return synth.make_synthetic_pack(G.Pack, config, loci, mut_scale=mut, data_seed=4100 + loci, mcmc_seed=4242, samples_per_log=8)


def sweep(s, flags=7):
    """one stepwise gph_engine_genealogy_sweep: its pass runs in front of it"""
    import gphocs_amd as G
    out = G.GphSweepResult()
    assert s.lib.gph_engine_genealogy_sweep(s.engine, flags, s.pack.ftCoalTime, s.pack.ftMigTime, C.byref(out)) == 0
    return out


def assert_stepped(S0, S1, k, what=""):
    """S1 = S0 stepped k times, per locus: the sweep leaves the generator where the serial code leaves it"""
    k = np.asarray(k, dtype=np.int64)
    assert k.min() >= 0
    states, _ = stream(S0, int(k.max()))
    want = states[k, np.arange(len(k))]
    bad = np.flatnonzero((want != S1).any(axis=1))
    assert len(bad) == 0, f"{what}: the generator of loci {bad[:8].tolist()} is not where {k[bad[:8]].tolist()} draws leave it"


# ---------------------------------------------------------------- k_rng_ahead against the independent generator
def check_pass(G, lib, pk, env, vals, monkeypatch, tmp_path, rounds=3):
    """counts that differ from lane to lane written through the hook, one stepwise sweep, then every byte of the pass's buffers:
    what the pass had to write equals the independent generator's stream, what it had no business writing is what stood there
    before.  Returns the (M, C) the engine ran with and every n met"""
    set_env(monkeypatch, env)
    s = G.Sampler(pk, lib=lib)
    L = s.end - s.begin
    s.initialize()
    on, M, Cd, _ = ahead(lib, s)
    assert on == 1
    sweep(s)                                    # every slot holds a pass
    snap = fetch(s)
    st = tmp_path / "state"
    seen = set()
    for r in range(rounds):
        kw = np.array([vals[(7 * j + r) % len(vals)] for j in range(L)], dtype=np.int32)
        set_counts(s, kw)
        assert (counts(s) == kw).all()
        S0 = parse_rng(dump(s, st))
        assert len(S0) == L
        sweep(s)
        draws, ckpt, tail = fetch(s)
        k = counts(s)
        S1 = parse_rng(dump(s, st))
        n = n_ahead(kw, M)
        seen |= set(int(v) for v in n)
        states, want = stream(S0, max(M, int(k.max())))
        for j in range(L):
            nj = int(n[j])
            assert (draws[j, :nj] == want[:nj, j]).all(), f"round {r} locus {j} (n = {nj}): draws {np.flatnonzero(draws[j, :nj] != want[:nj, j])[:8].tolist()} differ"
            assert (draws[j, nj:] == snap[0][j, nj:]).all(), f"round {r} locus {j} (n = {nj}): draws beyond n were written"
            nc = nj // Cd + 1                    # checkpoints at 0, C, ..., n
            assert (ckpt[j, :nc, :3] == states[0:nj + 1:Cd, j]).all() and (ckpt[j, :nc, 3] == 0).all(), f"round {r} locus {j} (n = {nj}): checkpoints"
            assert (ckpt[j, nc:] == snap[1][j, nc:]).all(), f"round {r} locus {j} (n = {nj}): checkpoints beyond n were written"
            assert (tail[j, :3] == states[nj, j]).all() and int(tail[j, 3]) == nj, f"round {r} locus {j} (n = {nj}): tail {tail[j].tolist()}"
        assert (k > 0).all()
        assert_stepped(S0, S1, k, f"round {r}")
        snap = (draws, ckpt, tail)
    assert s.debug_oob()[0] == 0
    s.close()
    return M, Cd, seen


# ---------------------------------------------------------------- counts forced onto the chunk edges
def first_sweep(G, lib, pk, monkeypatch, tmp_path, kprev=None):
    """a fresh engine, (kprev(k0 of the caller) written through the hook,) iteration 0: S0, the counts, the dump with
    conditionals, S1"""
    set_env(monkeypatch, {})
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    if kprev is not None:
        set_counts(s, kprev)
    S0 = parse_rng(dump(s, tmp_path / "s0"))
    s.iteration(0)
    k = counts(s)
    full = dump(s, tmp_path / "s1", True)
    oob = s.debug_oob()
    s.close()
    return dict(S0=S0, k=k, dump=full, S1=parse_rng(full), oob=oob)


def edge_counts(k0):
    """(a) every locus runs from its draws ahead into its first in-kernel chunk (k0 % 64 == 0: ends exactly on the last draw
    ahead, == 1: exactly one draw from the in-kernel chunk); (b) k0 % 64 == 0 ends on the last draw of an in-kernel chunk;
    (c) nothing comes from the buffer although M > 0"""
    k0 = np.asarray(k0, dtype=np.int64)
    return {"a": (k0 // 64) * 64 - 64, "b": ((k0 - 1) // 64) * 64 - 64, "c": np.full(len(k0), -64)}


def check_edge_residues(k0):
    """a condition on the input, not a measurement: the data set must put loci on the edges"""
    res = [int((k0 % 64 == m).sum()) for m in (0, 1, 63)]
    assert min(res) >= 5, f"the first sweep's counts put {res} loci on the residues 0 / 1 / 63 of 64: choose another data set"
    assert k0.min() > 64
    return res


def check_forced(plain, got, what):
    assert (got["S0"] == plain["S0"]).all(), what
    assert (got["k"] == plain["k"]).all(), f"{what}: counts differ at loci {np.flatnonzero(got['k'] != plain['k'])[:8].tolist()}"
    assert got["dump"] == plain["dump"], f"{what}: the state after the sweep differs"
    assert_stepped(got["S0"], got["S1"], plain["k"], what)
    assert got["oob"][0] == 0, what


def check_no_draws(G, lib, pk, monkeypatch, tmp_path):
    """k = 0: a sweep that proposes nothing (flags 2: migration nodes only, a model without bands) hands out no draw, leaves
    every generator where it was, and the pass of the sweep behind it generates 64 draws from there"""
    assert pk.B == 0
    set_env(monkeypatch, {})
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    S0 = parse_rng(dump(s, tmp_path / "s0"))
    sweep(s, 2)
    assert (counts(s) == 0).all()
    assert (parse_rng(dump(s, tmp_path / "s1")) == S0).all()
    sweep(s, 2)
    draws, ckpt, tail = fetch(s)
    states, want = stream(S0, 64)
    assert (tail[:, 3] == 64).all() and (tail[:, :3] == states[64]).all()
    assert (draws[:, :64] == want.T).all() and (ckpt[:, 0, :3] == S0).all()
    assert (counts(s) == 0).all() and (parse_rng(dump(s, tmp_path / "s1")) == S0).all()
    assert s.debug_oob()[0] == 0
    s.close()


# ---------------------------------------------------------------- hand-overs between the placements
class Chain(C.Structure):      # gph_chain_state (include/gphocs_hip.h)
    _fields_ = [("theta", C.c_double * 40), ("popAge", C.c_double * 40), ("sampleAge", C.c_double * 40),
                ("migRate", C.c_double * 100), ("bandStart", C.c_double * 100), ("bandEnd", C.c_double * 100),
                ("rng", C.c_uint32 * 3), ("logLikelihood", C.c_double), ("dataLogLikelihood", C.c_double),
                ("rateVar", C.c_double), ("coal_stats", C.c_double * 40), ("num_coals", C.c_double * 40),
                ("mig_stats", C.c_double * 100), ("num_migs", C.c_double * 100), ("rubberband_mig_conflicts", C.c_int64)]


def handover_script(G, lib, pk, env, monkeypatch, tmp_path):
    """the calls of tests/test_rng_ahead_stream_gpu.py::test_hand_overs_between_the_placements, a record after every call:
    (name, dump, accept counters, (B possible, a pass stands), counts or None, the call holds a sweep)"""
    set_env(monkeypatch, env)
    s = G.Sampler(pk, lib=lib)
    on = None
    rec = []
    st = tmp_path / "state"

    def note(name, has_sweep=False):
        rec.append(dict(name=name, dump=dump(s, st), accept=s.accept_counts(), side=side(s), k=counts(s) if on else None, sweep=has_sweep))

    def it(i):
        s.iteration(i)
        note(f"iteration {i}", True)

    s.initialize()
    on = ahead(lib, s)[0]
    note("initialize")
    it(0), it(1)
    s.unit(6, pk.n)               # traceLineage of the first internal node (where it is a locus's root: nothing), undone
    note("unit")
    it(2)
    sweep(s)
    note("stepwise sweep", True)
    it(3)
    s.enable_locus_summary()
    s.sample_locus_summary()
    note("locus summary")
    s.enable_coal_stats(4)
    s.sample_coal_stats(3)
    note("coal stats")
    s.enable_time_slices(4, 4)
    s.sample_time_slices(3)
    note("time slices")
    s.enable_ancestry(4)
    s.sample_ancestry(3)
    note("ancestry")
    s.enable_gene_trees(4)
    s.sample_gene_trees(3)
    note("gene trees")
    ok, sd, sg = C.c_int32(), C.c_double(), C.c_double()
    assert lib.gph_engine_check_all(s.engine, C.byref(ok), C.byref(sd), C.byref(sg)) == 0 and ok.value == 1
    note("check_all")
    note("state dump")            # (the dump of the record before this one, then its own)
    it(4)
    if on:
        set_counts(s, counts(s))
    else:
        kp = np.zeros(s.end - s.begin, dtype=np.int32)
        assert _hook(lib)(s.engine, None, kp.ctypes.data, 1) == GPH_ESTATE
    note("hook write")
    it(5)
    acc, mig = (C.c_int64 * 3)(), C.c_int64()
    assert lib.gph_mcmc_update_gb(s.mcmc, C.c_int32(6), C.c_double(pk.ftCoalTime), C.c_double(pk.ftMigTime), acc, C.byref(mig)) == 0
    note("update_gb", True)
    it(6)
    s.initialize()
    note("initialize again")
    ch = Chain()
    assert lib.gph_mcmc_get_chain(s.mcmc, C.byref(ch)) == 0
    it(0), it(1)
    oob, err = s.debug_oob(), s.last_error()
    s.close()
    # a fresh engine at the same points.  gph_mcmc_initialize goes on with the chain above the loci -- the control stream that
    # samples the start values, the accept counters -- so a second call is not a first one: the fresh engine takes the chain
    # state the second initialize() left (as parity_util.reinit_after_accepted_mixing does) and initialises its genealogies once
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    assert lib.gph_mcmc_set_chain(s.mcmc, C.byref(ch)) == 0
    assert lib.gph_mcmc_initialize_genealogies(s.mcmc) == 0
    fresh = [dict(dump=dump(s, st), accept=s.accept_counts())]
    for i in range(2):
        s.iteration(i)
        fresh.append(dict(dump=dump(s, st), accept=s.accept_counts()))
    assert s.debug_oob()[0] == 0
    s.close()
    return rec, oob, err, fresh


# what stands after each call where the pass can run behind the sweep (placement B): a chained iteration leaves a pass for the
# next one; whatever steps a generator or rewrites a page outside the chain voids it; what only reads the pages does not
HANDOVER_SIDE = {"initialize": 0, "unit": 0, "stepwise sweep": 0, "hook write": 0, "update_gb": 0, "initialize again": 0,
                 "locus summary": 1, "coal stats": 1, "time slices": 1, "ancestry": 1, "gene trees": 1, "check_all": 1, "state dump": 1}


def check_handover(rec, oob, err, fresh, ref=None, expect_side=None):
    names = [r["name"] for r in rec]
    assert names.count("iteration 0") == 2 and len(names) == 22
    if ref is not None:
        assert names == [r["name"] for r in ref]
        for a, b in zip(rec, ref):
            assert a["accept"] == b["accept"], a["name"]
            assert a["dump"] == b["dump"], a["name"]
    # the second initialize() and the two iterations behind it: a fresh engine's at the same points
    assert len(fresh) == 3 and rec[-3]["name"] == "initialize again"
    for a, b in zip(rec[-3:], fresh):
        assert a["dump"] == b["dump"], a["name"]
        assert [x - y for x, y in zip(a["accept"], rec[-3]["accept"])] == [x - y for x, y in zip(b["accept"], fresh[0]["accept"])], a["name"]
    for prev, r in zip(rec, rec[1:]):
        if r["sweep"]:
            if r["k"] is not None:
                assert_stepped(parse_rng(prev["dump"]), parse_rng(r["dump"]), r["k"], r["name"])
        elif r["name"] != "initialize again":
            assert (parse_rng(prev["dump"]) == parse_rng(r["dump"])).all(), r["name"]
    if expect_side is not None:
        for r in rec:
            want = 1 if r["name"].startswith("iteration") else HANDOVER_SIDE[r["name"]]
            assert r["side"] == (expect_side, want if expect_side else 0), (r["name"], r["side"])
    assert oob[0] == 0 and err == (-1, 0), (oob, err)
