"""Coalescence and migration statistics per time slice (gph_engine_time_slices_*, `G-PhoCS-hip -s PREFIX --time-slices S`)
on the CPU: the host-emulation build of the engine sources runs the bodies of k_time_slices and k_rows_fold over
the same pages.

The yardstick is `restate` below: the statistic as csrc/gph_timeslices.h and include/gphocs_hip.h define it, in plain
Python over the state dump taken at the sample (MODEL, C, M and S lines), walker by walker, locus after locus in locus
order.  It shares no code with the engine.

Counts (C, N) must be equal.  The fp64 sums (D, M) add the same non-negative terms -- every term is formed by the same
IEEE operations in both implementations -- in another order (lanes take every G-th locus of a chunk, chunks are folded),
so they are held to the summation bound test_coal_stats.py derives and nothing looser: relative difference
<= (2T + 4) * 2^-53, T = the terms the restatement added into the cell.

The cross-check against the pages' own statistics (the S lines: coal_stats, ncoal, mig_stats, nmig, byte-exact with the
reference) runs with a log period of one iteration: the pages' fp64 statistics are updated incrementally by every accepted
proposal and re-derived from the chain only by checkAll, once per log period, so only right after checkAll are they the
plain chain-order sums the bound speaks of.  The counts are compared at every sample of every run.

Which golden runs which path: every golden below fits one tile of walkers; with S = 7 the slice width is inexact.  The
deferred synchronizeEvents pass (vsync) is pending at every sample of the runs with the goldens' own log period and never
with a log period of one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import compare_trace_files
from sampler_util import EXE, _copy_case, _data_lines, _pop_names, _run, hostemu_library, load_pack, read_outputs, run_ranks, within_bound  # noqa: F401

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

COAL, IN_MIG, OUT_MIG, BAND_START, BAND_END = 0, 1, 2, 3, 4
ITERS = {"m3": 30, "a7": 24, "j1": 30, "v8": 24, "g1": 24, "x8": 5, "n7": 3}


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


# ---------------------------------------------------------------- the restatement, from a state dump
def parse_dump(path, K, B):
    """(model, {global locus: dict(chain[K] of (type, node, nlin, time), band of migration node, coal, ncoal, mig, nmig)})"""
    model, loci, cur = None, {}, None
    for ln in open(path):
        t = ln.split()
        if not t:
            continue
        if t[0] == "MODEL":
            v = [float.fromhex(x) for x in t[1:]]
            assert len(v) == 3 * K + 3 * B
            model = dict(popAge=[v[3 * p + 1] for p in range(K)], bandStart=[v[3 * K + 3 * b + 1] for b in range(B)],
                         bandEnd=[v[3 * K + 3 * b + 2] for b in range(B)])
        elif t[0] == "LOCUS":
            cur = dict(chain=[None] * K, band={})
            loci[int(t[1])] = cur
        elif t[0] == "C" and cur is not None:
            ev = []
            for x in t[2:]:
                f = x.split(":")
                ev.append((int(f[1]), int(f[2]), int(f[3]), float.fromhex(f[4])))
            cur["chain"][int(t[1])] = ev
        elif t[0] == "S" and cur is not None:
            v = t[1:]
            assert len(v) == 2 * K + 2 * B
            cur["coal"] = [float.fromhex(v[2 * k]) for k in range(K)]
            cur["ncoal"] = [int(v[2 * k + 1]) for k in range(K)]
            cur["mig"] = [float.fromhex(v[2 * K + 2 * b]) for b in range(B)]
            cur["nmig"] = [int(v[2 * K + 2 * b + 1]) for b in range(B)]
        elif t[0] == "M" and cur is not None:
            for x in t[2:]:
                f = x.split(":")
                cur["band"][int(f[0])] = int(f[2])
    return model, loci


def restate(model, loci, pk, S):
    """the statistic of one sample: C, D [K][S]; N, M [B][S]; TD, TM terms added per cell; splits = intervals cut by a boundary"""
    K, B, root = pk.K, pk.B, pk.rootPop
    father, tgt = [int(x) for x in pk.popFather], [int(x) for x in pk.bandTgt]
    popAge, bandStart, bandEnd = model["popAge"], model["bandStart"], model["bandEnd"]
    C = [[0] * S for _ in range(K)]
    D = [[0.0] * S for _ in range(K)]
    TD = [[0] * S for _ in range(K)]
    N = [[0] * S for _ in range(B)]
    M = [[0.0] * S for _ in range(B)]
    TM = [[0] * S for _ in range(B)]
    splits = 0
    for g in sorted(loci):
        d = loci[g]
        for p in range(K):
            a = popAge[p]
            if p == root:
                Sp, w, end = 1, 0.0, 0.0
            else:
                Sp = S
                w = (popAge[father[p]] - a) / S
                end = a + w
            s = 0
            for typ, node, nlin, time in d["chain"][p]:
                t = time
                a = a + t
                while Sp > 1 and s < Sp - 1 and a > end:
                    t = t - (a - end)
                    D[p][s] += (nlin * (nlin - 1)) * t
                    TD[p][s] += 1
                    splits += 1
                    s += 1
                    t = a - end
                    end = end + w
                D[p][s] += (nlin * (nlin - 1)) * t
                TD[p][s] += 1
                if typ == COAL:
                    C[p][s] += 1
        for b in range(B):
            q = tgt[b]
            a = popAge[q]
            live = False
            s, w, end = 0, 0.0, 0.0
            for typ, node, nlin, time in d["chain"][q]:
                t = time
                a = a + t
                if live:
                    while s < S - 1 and a > end:
                        t = t - (a - end)
                        M[b][s] += nlin * t
                        TM[b][s] += 1
                        splits += 1
                        s += 1
                        t = a - end
                        end = end + w
                    M[b][s] += nlin * t
                    TM[b][s] += 1
                    if typ == IN_MIG and d["band"][node] == b:
                        N[b][s] += 1
                    if typ == BAND_END and node == b:
                        break
                elif typ == BAND_START and node == b:
                    live = True
                    s = 0
                    w = (bandEnd[b] - bandStart[b]) / S
                    end = bandStart[b] + w
    return dict(C=C, D=D, TD=TD, N=N, M=M, TM=TM, splits=splits)


def page_totals(loci, K, B):
    """the pages' own statistics summed in locus order, with the number of events behind each sum"""
    coal, mig, ncoal, nmig = [0.0] * K, [0.0] * B, [0] * K, [0] * B
    for g in sorted(loci):
        d = loci[g]
        for p in range(K):
            coal[p] += d["coal"][p]
            ncoal[p] += d["ncoal"][p]
        for b in range(B):
            mig[b] += d["mig"][b]
            nmig[b] += d["nmig"][b]
    return coal, ncoal, mig, nmig


def split_row(row, S, K, B):
    cells = np.asarray(row[1:]).reshape(K + B, S, 2)
    return cells[:K, :, 0], cells[:K, :, 1], cells[K:, :, 0], cells[K:, :, 1]


def run_chain(lib, name, iters, S, tmp, sample=True, dumps=False, record=None, capacity=None, tag="", chunk=0, log_period=None):
    """one chain over golden `name` (lib None: the tightest capacity variant), a sample after every iteration"""
    import gphocs_amd as G
    pk = load_pack(name)
    if log_period:
        pk.samplesPerLog = log_period
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            s.enable_time_slices(S, capacity or iters, chunk=chunk)
        s.initialize()
        hs0 = s.host_stats()
        paths = []
        for it in range(iters):
            s.iteration(it)
            if sample:
                s.sample_time_slices(it)
            if dumps:
                p = str(tmp / f"{name}.{S}.{it}{tag}.dump")
                s.dump_state(p, False)
                paths.append(p)
        hs1 = s.host_stats()
        s.set_record_file(None)
        raw = s.time_slices(raw=True) if sample else None
        cols = s.time_slices_columns() if sample else None
        final = str(tmp / f"{name}.final.{S}{'s' if sample else 'n'}{'d' if dumps else ''}{tag}")
        s.dump_state(final, True)
        return dict(raw=raw, cols=cols, final=final, dumps=paths, pack=pk, stats=(hs0, hs1), oob=s.debug_oob(),
                    mix_finishes=s.class_stats(7)["launches"])
    finally:
        s.close()


def check_against_restatement(lib, name, iters, S, tmp_path, chunk=0, log_period=None, need_mig=False):
    """items 1, 2 and 3 of the issue: every sample against the restatement over the dump taken at that sample; the slice
    sums against the pages' own statistics (counts always, fp64 sums when log_period == 1); the inputs are not vacuous"""
    r = run_chain(lib, name, iters, S, tmp_path, dumps=True, chunk=chunk, log_period=log_period, tag=f".c{chunk}.l{log_period}")
    pk, raw = r["pack"], r["raw"]
    K, B = pk.K, pk.B
    assert raw.shape == (iters, 1 + 2 * S * (K + B))
    cols = r["cols"]
    assert len(cols) == raw.shape[1] and cols[:3] == ["iter", "numCoal.0.1", "deltaT.0.1"] and cols[2 * S - 1:2 * S + 1] == [f"numCoal.0.{S}", f"deltaT.0.{S}"]
    if B:
        assert cols[-2:] == [f"numMig.{B - 1}.{S}", f"migT.{B - 1}.{S}"]
    worst = dict(D=0.0, M=0.0, sumD=0.0, sumM=0.0)
    coal_slices = [set() for _ in range(K)]
    mig_slices = [set() for _ in range(B)]
    splits = 0
    for it in range(iters):
        model, loci = parse_dump(r["dumps"][it], K, B)
        want = restate(model, loci, pk, S)
        splits += want["splits"]
        C, D, N, M = split_row(raw[it], S, K, B)
        assert raw[it][0] == it
        assert C.tolist() == want["C"], f"{name} S={S} sample {it}: C"
        assert N.tolist() == want["N"], f"{name} S={S} sample {it}: N"
        for got, ref, T, key, n in ((D, want["D"], want["TD"], "D", K), (M, want["M"], want["TM"], "M", B)):
            for q in range(n):
                for s in range(S):
                    ok, rel = within_bound(float(got[q, s]), ref[q][s], T[q][s])
                    worst[key] = max(worst[key], rel)
                    assert ok, f"{name} S={S} sample {it}: {key}[{q}][{s}] {got[q, s]!r} vs {ref[q][s]!r}, {T[q][s]} terms"
        assert not C[pk.rootPop, 1:].any() and not D[pk.rootPop, 1:].any()        # the root has one slice
        # the slices of a branch / a band add up to the pages' own statistics
        coal, ncoal, mig, nmig = page_totals(loci, K, B)
        assert C.sum(axis=1).tolist() == ncoal and N.sum(axis=1).tolist() == nmig
        if log_period == 1:
            for q in range(K):
                ok, rel = within_bound(float(sum(float(x) for x in D[q])), coal[q], sum(want["TD"][q]))
                worst["sumD"] = max(worst["sumD"], rel)
                assert ok, f"{name} S={S} sample {it}: sum of D[{q}] {sum(D[q])!r} vs coal_stats {coal[q]!r}"
            for q in range(B):
                ok, rel = within_bound(float(sum(float(x) for x in M[q])), mig[q], sum(want["TM"][q]))
                worst["sumM"] = max(worst["sumM"], rel)
                assert ok, f"{name} S={S} sample {it}: sum of M[{q}] {sum(M[q])!r} vs mig_stats {mig[q]!r}"
        for q in range(K):
            coal_slices[q] |= {s for s in range(S) if want["C"][q][s]}
        for q in range(B):
            mig_slices[q] |= {s for s in range(S) if want["N"][q][s]}
    print(f"{name} S={S}: worst relative differences {worst}, {splits} split intervals")
    if S > 1:
        # item 3: the restatement alone shows that the slices are exercised
        assert sum(len(x) >= 2 for x in coal_slices) >= 2, coal_slices
        assert splits >= 1
        if need_mig:
            assert any(len(x) >= 2 for x in mig_slices), mig_slices
    return r


def check_chain_untouched(lib, name, iters, S, raw_d, tmp_path):
    """items 4 and 5: sampling without dumps -- records and final state byte-identical to a run without sampling; the rows
    bitwise those of the run with dumps (a second run of the same chain)"""
    rec_on, rec_off = str(tmp_path / f"on{S}.rtrace"), str(tmp_path / f"off{S}.rtrace")
    on = run_chain(lib, name, iters, S, tmp_path, record=rec_on)
    off = run_chain(lib, name, iters, S, tmp_path, sample=False, record=rec_off)
    assert open(rec_on).read() == open(rec_off).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert on["raw"].tobytes() == raw_d.tobytes(), f"{name}: two runs of the same chain differ"
    return on, off


@pytest.mark.parametrize("S", [1, 4, 7])
@pytest.mark.parametrize("name", ["m3", "a7", "j1", "v8", "g1", "x8"])
def test_rows_match_the_restatement_and_leave_the_chain_unchanged(hostemu, tmp_path, name, S):
    _, lib = hostemu
    r = check_against_restatement(lib, name, ITERS[name], S, tmp_path, need_mig=name in ("m3", "j1"))
    on, off = check_chain_untouched(lib, name, ITERS[name], S, r["raw"], tmp_path)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert r["oob"][0] == 0


SUM_CASES = [("m3", 1), ("m3", 4), ("j1", 7), ("j1", 1), ("a7", 4), ("v8", 7), ("g1", 1), ("g1", 4), ("x8", 4)]


@pytest.mark.parametrize("name,S", SUM_CASES)
def test_slices_add_up_to_the_pages_own_statistics(hostemu, tmp_path, name, S):
    """log period 1: checkAll re-derives the pages' statistics from the chain at the end of every iteration; with S = 1 the
    sums are the whole row.  Every golden of the test above, the same iteration counts"""
    _, lib = hostemu
    check_against_restatement(lib, name, ITERS[name], S, tmp_path, log_period=1, need_mig=name in ("m3", "j1"))


def test_walkers_in_more_than_one_tile(tmp_path):
    """w139: 39 populations and 100 bands, 32 slices -- 139 walkers, and 192 lanes of accumulators alone (12 * 32 bytes a lane)
    are more LDS than a workgroup may have, whatever the image of a locus takes: the walkers are tiled over blockIdx.y, and
    every tile stages the group's images itself"""
    import run_hostemu
    import gphocs_amd as G
    big = G.load_library(run_hostemu.build_hostemu(big=True))
    S = 32
    r = check_against_restatement(big, "w139", 3, S, tmp_path)
    pk = r["pack"]
    assert (pk.K + pk.B + 63) // 64 * 64 * 12 * S > 61440          # GPH_TS_LDS_MAX
    assert r["oob"][0] == 0


def test_several_chunks_fold_in_chunk_order(hostemu, tmp_path):
    """chunks of 5 slots: four partial rows per sample; counts as with one chunk, sums within the bound, reproducible"""
    _, lib = hostemu
    one = run_chain(lib, "m3", 20, 4, tmp_path, tag="one")["raw"]
    r = check_against_restatement(lib, "m3", 20, 4, tmp_path, chunk=5, need_mig=True)
    again = run_chain(lib, "m3", 20, 4, tmp_path, tag="again", chunk=5)["raw"]
    assert r["raw"].tobytes() == again.tobytes()
    assert r["raw"][:, 1::2].tolist() == one[:, 1::2].tolist()        # the count columns


def test_capacity_and_arguments(hostemu, tmp_path):
    import gphocs_amd as G
    _, lib = hostemu
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.time_slices()                       # not enabled
        s.initialize()
        with pytest.raises(RuntimeError):
            s.sample_time_slices(0)
        for bad in (0, -3, 33, 1000):
            assert s.lib.gph_engine_time_slices_enable(s.engine, bad, 4) == -1        # GPH_EARG
            with pytest.raises(ValueError):
                s.enable_time_slices(bad, 4)
        assert s.lib.gph_engine_time_slices_enable(s.engine, 4, -1) == -1
        s.enable_time_slices(32, 1)               # the largest supported count
        s.sample_time_slices(0)
        assert s.time_slices().shape == (1, 1 + 2 * 32 * (pk.K + pk.B))
        s.enable_time_slices(4, 3)
        for it in range(3):
            s.iteration(it)
            s.sample_time_slices(it)
        s.iteration(3)
        with pytest.raises(BufferError):
            s.sample_time_slices(3)
        assert s.lib.gph_engine_time_slices_sample(s.engine, 3) == G.COAL_STATS_FULL == -5
        rows = s.time_slices()
        assert rows[:, 0].tolist() == [0.0, 1.0, 2.0]
        assert s.time_slices().shape[0] == 0              # the fetch emptied the buffer
        s.sample_time_slices(3)                            # ... and there is room again
        t = s.time_slices(raw=False)
        assert len(t) == 1 and t[0]["iter"] == 3 and t[0]["numCoal"].shape == (pk.K, 4) and t[0]["migT"].shape == (pk.B, 4)
        assert t[0]["numCoal"].sum() == pk.L * (pk.n - 1)          # every genealogy has n - 1 coalescences, each in one slice
        s.enable_time_slices(4, 0)
        with pytest.raises(RuntimeError):
            s.sample_time_slices(4)
    finally:
        s.close()


def test_reference_caps_are_sized_within_the_lds(hostemu):
    """39 populations, 100 bands, 200 leaves, S = 8 on the largest capacity variant: the host build with those capacities
    sizes the workgroup the way the device build does; it must fit"""
    import run_hostemu
    import gphocs_amd as G
    big = G.load_library(run_hostemu.build_hostemu(big=True))
    pk = G.Pack.load(os.path.join(GOLDEN, "n7.gpk"))
    s = G.Sampler(pk, lib=big)
    try:
        s.initialize()
        s.enable_time_slices(8, 1)
        s.sample_time_slices(0)
        assert s.time_slices().shape == (1, 1 + 2 * 8 * (pk.K + pk.B))
        s.enable_time_slices(32, 1)
        s.sample_time_slices(0)
    finally:
        s.close()


# ---------------------------------------------------------------- the program and the launcher
def band_names(ctl_path, pk):
    pops = _pop_names(ctl_path)
    return [f"{pops[int(pk.bandSrc[b])]}->{pops[int(pk.bandTgt[b])]}" for b in range(pk.B)]


def format_file(rows, S, pops, bands):
    """PREFIX.slices.tsv of raw rows: the header of GPhoCS.c:933 and the formats of GPhoCS.c:1005"""
    hdr = ["iter"]
    for nm in pops:
        for k in range(1, S + 1):
            hdr += [f"numCoal_{nm}:{k}", f"deltaT_{nm}:{k}"]
    for nm in bands:
        for k in range(1, S + 1):
            hdr += [f"numMig_{nm}:{k}", f"migT_{nm}:{k}"]
    lines = ["\t".join(hdr)]
    for r in rows:
        lines.append("%7d" % int(r[0]) + "".join("\t%9d\t%8f" % (int(r[c]), r[c + 1]) for c in range(1, len(r), 2)))
    return "\n".join(lines) + "\n"


def expected_rows(ctl_dir, ctl, S, lib=None, sampler_lib=None, terms_dir=None):
    """the raw rows of an equivalent Sampler run: burn-in first, a sample wherever a trace line is written.  terms_dir: a
    state dump is taken there at every sample and p.terms[sample] = the restatement's terms per cell, in row order"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    s = G.Sampler(p, lib=sampler_lib)
    its, terms = [], []
    try:
        s.enable_time_slices(S, p.numSamplesMcmc)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.sample_time_slices(it)
                its.append(it)
                if terms_dir is not None:
                    d = os.path.join(str(terms_dir), f"one.{it}.dump")
                    s.dump_state(d, False)
                    want = restate(*parse_dump(d, p.K, p.B), p, S)
                    terms.append([t for q in want["TD"] + want["TM"] for t in q])
                    os.remove(d)
        raw = s.time_slices()
    finally:
        s.close()
    assert raw[:, 0].tolist() == its
    p.terms = terms
    return raw, its, p


def check_program(lib_path, lib, tmp_path, name, S):
    a, b, c, d = tmp_path / "with", tmp_path / "without", tmp_path / "small", tmp_path / "plain"
    for x in (a, b, c, d):
        _copy_case(name, x)
    _run(lib_path, a, ["-s", "out", "--time-slices", str(S), name + ".ctl"])
    _run(lib_path, b, ["-s", "out", name + ".ctl"])
    _run(lib_path, d, [name + ".ctl"])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read() == open(d / (name + ".trace")).read()
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), str(trace))
    got, base = read_outputs(a, "out"), read_outputs(b, "out")
    assert sorted(got) == sorted(list(base) + ["slices.tsv"])       # no part left behind
    assert all(got[f] == base[f] for f in base)                     # the -s files are byte-identical with and without the flag
    raw, its, p = expected_rows(str(a), name + ".ctl", S, lib, lib)
    assert [int(ln.split("\t")[0]) for ln in _data_lines(trace)] == its
    want = format_file(raw, S, _pop_names(a / (name + ".ctl")), band_names(a / (name + ".ctl"), p))
    assert got["slices.tsv"].splitlines()[0] == want.splitlines()[0]
    assert got["slices.tsv"] == want
    # a device buffer of 4 rows, flushed again and again; composed with the locus table
    _run(lib_path, c, ["-s", "out", "--coal-stats-rows", "4", "--time-slices", str(S), "-l", "sum.tsv", name + ".ctl"])
    assert len(its) > 3 * 4
    assert read_outputs(c, "out") == got
    return raw, its, p


@pytest.mark.parametrize("name,S", [("g1", 4), ("j1", 7)])
def test_program_writes_the_slices_file(hostemu, tmp_path, name, S):
    path, lib = hostemu
    check_program(path, lib, tmp_path, name, S)


def test_time_slices_without_a_prefix_is_a_usage_error(hostemu, tmp_path):
    path, lib = hostemu
    _copy_case("g1", tmp_path)
    env = dict(os.environ, GPHOCS_HIP_LIB=path)
    r = subprocess.run([EXE, "--time-slices", "4", "g1.ctl"], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and "usage" in r.stderr and not os.path.exists(tmp_path / "g1.trace")
    import gphocs_amd as G
    assert G.run_control_file(lib, "g1.ctl", time_slices=4) == -1


def check_ranks(lib_path, lib, name, S, tmp_path, rank_counts=(2, 3)):
    """two and three ranks at full precision.  The ranks' parts, added in rank order by gph_time_slices_combined, are bit for
    bit the rank-order sum this test forms itself from the part files; against the one-rank rows the counts are equal and
    every fp64 sum is within (2T + 4) * 2^-53 -- one rank and several are two orderings of the same terms -- with T the
    terms of that cell, counted by the restatement over the one-rank run's dump at that sample.  Then the file
    gph_time_slices_write makes of the parts: the documented formats applied to those rows, no part left; and the
    launcher's -g run gives the same file."""
    import gphocs_amd as G
    one_dir = tmp_path / "one"
    _copy_case(name, one_dir)
    one, its, p = expected_rows(str(one_dir), name + ".ctl", S, lib, lib, terms_dir=one_dir)
    pops, bands = _pop_names(one_dir / (name + ".ctl")), band_names(one_dir / (name + ".ctl"), p)
    rd = 1 + 2 * S * (p.K + p.B)
    terms = np.asarray(p.terms)
    assert terms.shape == (len(its), S * (p.K + p.B))
    for ranks in rank_counts:
        d = tmp_path / f"w{ranks}"
        run_ranks(lib_path, name, ranks, d, coal_stats="out", coal_stats_rows=5, time_slices=S)
        parts = [read_part(d / f"out.slices.part{r}") for r in range(ranks)]
        assert all(q[0] == (S, p.K, p.B, rd) and q[2] == len(its) for q in parts)
        mine = parts[0][1].copy()
        for q in parts[1:]:
            mine[:, 1:] = mine[:, 1:] + q[1][:, 1:]
        comb = G.time_slices_combined(lib, d / "out", ranks)
        assert comb.tobytes() == mine.tobytes(), f"{ranks} ranks: not the rank-order sum of the parts"
        assert comb[:, 0].tolist() == its
        assert comb[:, 1::2].tolist() == one[:, 1::2].tolist(), f"{ranks} ranks: counts"
        got, want = comb[:, 2::2], one[:, 2::2]
        for i in range(got.shape[0]):
            for j in range(got.shape[1]):
                ok, rel = within_bound(float(got[i, j]), float(want[i, j]), int(terms[i, j]))
                assert ok, f"{ranks} ranks: sample {i} cell {j}: {got[i, j]!r} vs {want[i, j]!r}, {terms[i, j]} terms (rel {rel:.3g})"
        assert lib.gph_time_slices_write(str(d / "out").encode(), ranks) == 0
        assert lib.gph_coal_stats_discard(str(d / "out").encode(), ranks) == 0        # (the coal-stats parts of the same run)
        files = read_outputs(d, "out")
        assert list(files) == ["slices.tsv"] and files["slices.tsv"] == format_file(comb, S, pops, bands)
        # the launcher: the same ranks, the same parts, the same file
        e = tmp_path / f"g{ranks}"
        _copy_case(name, e)
        _run(lib_path, e, ["-g", str(ranks), "-s", "out", "--coal-stats-rows", "5", "--time-slices", str(S), name + ".ctl"])
        out = read_outputs(e, "out")
        assert not [f for f in out if "part" in f] and out["slices.tsv"] == files["slices.tsv"]


def read_part(path):
    """((S, K, B, row_doubles), records [samples][row_doubles], trailer count) of a rank's PREFIX.slices.part<r>"""
    import struct
    b = open(path, "rb").read()
    assert b[:8] == b"GPHTS1\n\0"
    hdr = struct.unpack_from("<4i", b, 8)
    nbytes, = struct.unpack_from("<i", b, 24)
    count, = struct.unpack_from("<q", b, len(b) - 8)
    return hdr, np.frombuffer(b[28 + nbytes:-8], dtype=np.float64).reshape(-1, hdr[3]), count


def test_ranks_add_up_to_the_one_rank_rows(hostemu, tmp_path):
    path, lib = hostemu
    check_ranks(path, lib, "m3", 4, tmp_path)


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run that fails AFTER rows were flushed to the parts (a directory sits where PREFIX.slices.tsv, or PREFIX.coal.tsv,
    must be written): status non-zero, no part, no slices file and no coal-stats file left -- one rank and two"""
    for ranks in (1, 2):
        for block in ("out.slices.tsv", "out.coal.tsv"):
            d = tmp_path / f"f{ranks}{block}"
            _copy_case("g1", d)
            os.mkdir(d / block)
            args = (["-g", str(ranks)] if ranks > 1 else []) + ["-s", "out", "--coal-stats-rows", "1", "--time-slices", "4", "g1.ctl"]
            env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
            r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
            assert r.returncode != 0
            assert len(open(d / "g1.trace").read().splitlines()) == 31        # the chain itself ran to its end
            assert [f for f in os.listdir(d) if f.startswith("out.")] == [block] and not os.listdir(d / block)


def test_failed_run_leaves_no_slices_file(hostemu, tmp_path):
    path, _ = hostemu
    check_failed_runs_leave_nothing(path, tmp_path)
