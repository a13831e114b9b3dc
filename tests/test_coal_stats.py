"""Genome-wide coalescent statistics and sample-pair statistics per sample (gph_engine_coal_stats_*, `G-PhoCS-hip -s PREFIX`)
on the CPU: the host-emulation build of the engine sources runs the per-locus body of k_coal_stats and the fold of
k_rows_fold over the same pages.

The yardstick is `restate` below: an independent restatement, in plain Python over state dumps taken at every sample (the
LOCUS / N / S lines), of the reference's computeNodeStats / computeFlatStats (patch.c:2172-2320) -- recursive LCAs over
the son links, sequential sums over the loci in locus order.  It shares no code with the engine.

Integers (cnt, first, numCoal, numMig) must be equal.  The fp64 sums (agesum, coalStat, migStat) add non-negative terms
in another order than the restatement (slots in chunks instead of loci in order), so they are held to the summation
bound and nothing looser: two orderings of T non-negative terms differ by at most 2(T-1)u relative, u = 2^-53, plus 2u per
term for the two products of a flat-statistic term -- relative difference <= (2T + 4) * 2^-53, T = the terms actually
summed (cnt for agesum, L * (n - 1) for the flat statistics).  The two log-likelihood columns are compared at
parity_util.REL_TOL with the chain's own values at the sample -- dataState.dataLogLikelihood and dataState.logLikelihood *
numLoci, full precision, as gph_mcmc_get_state hands them to the trace writer (the record file's TRACE line holds the same
two numbers rounded to six decimals).

Which golden runs which path: m3, a7, j1, v8, g1 fit one tile of pairs (66 pairs or fewer in a workgroup of 64 or 128
lanes); x8 (32 leaves, 31 populations: 496 pairs, 64 lanes a workgroup) runs the tiled path with 8 tiles, and n7 (72
leaves: 2556 pairs in 10 tiles of 256) runs it on the device (tests/test_coal_stats_gpu.py).  With chunks of 5 slots
(gph_engine_coal_stats_set_chunk) the 16 loci of m3 make four chunks, so the fold adds several partial rows.
A workgroup with fewer lanes than genealogy nodes (64 lanes, which takes 25 populations or more, with 33 leaves or more:
N = 2n - 1 > 64) stages the node records beyond the first 64 by a strided loop straight from the page, and a lane ranks
several internal nodes: y9 (40 leaves, 39 populations: N = 79 in 64 lanes, 780 pairs in 13 tiles) on the host build with
the 64-leaf capacities.  x8 has N = 63 in 64 lanes, n7 N = 143 in 256."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import REL_TOL, compare_records, compare_trace_files
from sampler_util import (EXE, U, _copy_case, _data_lines, _pop_names, _run, hostemu_library, printed_names, read_outputs, run_ranks,  # noqa: F401
                          within_bound)

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

GOLDEN_ITERS = {"m3": 120, "a7": 100, "v8": 60, "j1": 150, "g1": 30, "x8": 24, "n7": 12}
FIXED = ["iter", "coalStat", "numCoal", "migStat", "numMig", "genLnL", "dataLnL"]


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


# ---------------------------------------------------------------- the restatement, from state dumps
def parse_dump(path, K, B):
    """{global locus: dict(father, left, right, age, pop per node; ncoal[K], nmig[B])} of a gph_engine_dump_loci dump"""
    loci, cur = {}, None
    for ln in open(path):
        t = ln.split()
        if not t:
            continue
        if t[0] == "LOCUS":
            cur = dict(root=int(t[3]), father={}, left={}, right={}, age={}, pop={})
            loci[int(t[1])] = cur
        elif t[0] == "N" and cur is not None:
            v = int(t[1])
            cur["father"][v], cur["left"][v], cur["right"][v] = int(t[2]), int(t[3]), int(t[4])
            cur["age"][v], cur["pop"][v] = float.fromhex(t[5]), int(t[6])
        elif t[0] == "S" and cur is not None:
            v = t[1:]
            assert len(v) == 2 * K + 2 * B
            cur["ncoal"] = [int(v[2 * k + 1]) for k in range(K)]
            cur["nmig"] = [int(v[2 * K + 2 * b + 1]) for b in range(B)]
    return loci


def pair_index(n):
    return {(i, j): p for p, (i, j) in enumerate((i, j) for i in range(n) for j in range(i + 1, n))}


def restate(loci, n, K, B):
    """patch.c:2172-2320 as the issue words it, one sample: dict(cnt, first [pairs][K] ints; agesum [pairs][K]; coalStat,
    migStat; numCoal, numMig), sums sequential over the loci in locus order"""
    pidx = pair_index(n)
    NP = len(pidx)
    cnt = [[0] * K for _ in range(NP)]
    first = [[0] * K for _ in range(NP)]
    agesum = [[0.0] * K for _ in range(NP)]
    coalStat = migStat = 0.0
    numCoal = numMig = 0
    for g in sorted(loci):
        d = loci[g]
        lca = {}

        def leaves(v):
            if v < n:
                return [v]
            a, b = leaves(d["left"][v]), leaves(d["right"][v])
            for x in a:
                for y in b:
                    lca[(min(x, y), max(x, y))] = v
            return a + b
        assert sorted(leaves(d["root"])) == list(range(n))
        firstNode, firstAge = [-1] * K, [0.0] * K
        for v in range(n, 2 * n - 1):
            p = d["pop"][v]
            if firstNode[p] < 0 or d["age"][v] < firstAge[p]:
                firstNode[p], firstAge[p] = v, d["age"][v]
        for ij, p in pidx.items():
            v = lca[ij]
            P = d["pop"][v]
            cnt[p][P] += 1
            agesum[p][P] += d["age"][v]
            if firstNode[P] == v:
                first[p][P] += 1
        a = sorted(d["age"][v] for v in range(n, 2 * n - 1))
        for i, k in enumerate(range(n, 1, -1)):
            dT = a[0] if i == 0 else a[i] - a[i - 1]
            migStat += dT * k
            coalStat += dT * k * (k - 1)
        numCoal += sum(d["ncoal"])
        numMig += sum(d["nmig"])
    return dict(cnt=cnt, first=first, agesum=agesum, coalStat=coalStat, migStat=migStat, numCoal=numCoal, numMig=numMig)


def split_row(row, n, K):
    npk = n * (n - 1) // 2 * K
    blocks = [np.asarray(row[7 + b * npk:7 + (b + 1) * npk]).reshape(-1, K) for b in range(3)]
    return row[:7], blocks[0], blocks[1], blocks[2]


def run_chain(lib, name, iters, tmp, sample=True, dumps=False, record=None, capacity=None, tag="", chunk=0):
    """one chain over golden `name` (lib None: the tightest capacity variant), a sample after every iteration: the raw rows,
    the final state dump, the per-iteration dumps, the pack, host_stats() after initialize and at the end, debug_oob()"""
    import gphocs_amd as G
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            s.enable_coal_stats(capacity or iters, chunk=chunk)
        s.initialize()
        hs0 = s.host_stats()
        paths, lnl = [], []
        for it in range(iters):
            s.iteration(it)
            if sample:
                s.sample_coal_stats(it)
            if dumps:
                p = str(tmp / f"{name}.{it}.dump")
                s.dump_state(p, False)
                paths.append(p)
                st = s.state()
                lnl.append((st["dataLogLikelihood"], st["logLikelihood"]))
        hs1 = s.host_stats()
        s.set_record_file(None)
        raw = s.coal_stats(raw=True) if sample else None
        cols = s.coal_stats_columns() if sample else None
        final = str(tmp / f"{name}.final.{'s' if sample else 'n'}{'d' if dumps else ''}{tag}")
        s.dump_state(final, True)
        return dict(raw=raw, cols=cols, final=final, dumps=paths, lnl=lnl, pack=pk, stats=(hs0, hs1), oob=s.debug_oob())
    finally:
        s.close()


def check_against_restatement(lib, name, iters, tmp_path, chunk=0):
    """items 1 and 2: every sample against the restatement over the state dump taken at that sample"""
    rec = str(tmp_path / f"{name}.dumps.rtrace")
    r = run_chain(lib, name, iters, tmp_path, dumps=True, record=rec, chunk=chunk)
    pk, raw = r["pack"], r["raw"]
    n, K, B, L = pk.n, pk.K, pk.B, pk.L
    pidx = pair_index(n)
    assert raw.shape == (iters, 7 + 3 * len(pidx) * K)
    assert r["cols"][:7] == FIXED and len(r["cols"]) == raw.shape[1]
    assert r["cols"][7] == "cnt.0.1.0" and r["cols"][-1] == f"agesum.{n - 2}.{n - 1}.{K - 1}"
    lnl = r["lnl"]
    worst = dict(agesum=0.0, flat=0.0, lnl=0.0)
    for it in range(iters):
        want = restate(parse_dump(r["dumps"][it], K, B), n, K, B)
        fixed, cnt, first, agesum = split_row(raw[it], n, K)
        assert fixed[0] == it
        assert cnt.tolist() == want["cnt"], f"{name} sample {it}: cnt"
        assert first.tolist() == want["first"], f"{name} sample {it}: first"
        assert fixed[2] == want["numCoal"] and fixed[4] == want["numMig"], f"{name} sample {it}: event counts"
        assert np.all(cnt.sum(axis=1) == L) and np.all(first <= cnt)
        for p in range(len(pidx)):
            for k in range(K):
                ok, rel = within_bound(float(agesum[p, k]), want["agesum"][p][k], want["cnt"][p][k])
                worst["agesum"] = max(worst["agesum"], rel)
                assert ok, f"{name} sample {it}: agesum[{p}][{k}] {agesum[p, k]!r} vs {want['agesum'][p][k]!r}, {want['cnt'][p][k]} terms"
        for col, key in ((1, "coalStat"), (3, "migStat")):
            ok, rel = within_bound(float(fixed[col]), want[key], L * (n - 1))
            worst["flat"] = max(worst["flat"], rel)
            assert ok, f"{name} sample {it}: {key} {fixed[col]!r} vs {want[key]!r}"
        data, logl = lnl[it]
        for got, ref in ((fixed[6], data), (fixed[5] + fixed[6], logl * L)):
            rel = abs(got - ref) / abs(ref)
            worst["lnl"] = max(worst["lnl"], rel)
            assert rel <= REL_TOL, f"{name} sample {it}: log-likelihood {got!r} vs the chain's {ref!r}"
    print(f"{name}: worst relative differences {worst}")
    return r


def check_chain_untouched(lib, name, iters, full, raw_d, tmp_path, tol=1e-12):
    """items 3 and 4: over the golden's whole run, sampling without dumps -- records and final state byte-identical to a run
    without sampling and still the golden's records; the rows of the first `iters` samples bitwise those of the run with
    dumps (a second run of the same chain).  Returns the two runs."""
    rec_on, rec_off = str(tmp_path / "on.rtrace"), str(tmp_path / "off.rtrace")
    on = run_chain(lib, name, full, tmp_path, record=rec_on)
    off = run_chain(lib, name, full, tmp_path, sample=False, record=rec_off)
    assert open(rec_on).read() == open(rec_off).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(rec_on, os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["raw"][:iters].tobytes() == raw_d.tobytes(), f"{name}: two runs of the same chain differ"
    return on, off


@pytest.mark.parametrize("name,iters", [("m3", 120), ("a7", 60), ("v8", 60), ("j1", 80), ("g1", 30)])
def test_rows_match_the_restatement_and_leave_the_chain_unchanged(hostemu, tmp_path, name, iters):
    _, lib = hostemu
    r = check_against_restatement(lib, name, iters, tmp_path)
    on, off = check_chain_untouched(lib, name, iters, GOLDEN_ITERS[name], r["raw"], tmp_path)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert r["oob"][0] == 0


def test_tiled_pairs_on_a_wide_model(hostemu, tmp_path):
    """x8: 496 pairs over 31 populations -- 8 tiles of 64 pairs"""
    _, lib = hostemu
    r = check_against_restatement(lib, "x8", 8, tmp_path)
    check_chain_untouched(lib, "x8", 8, GOLDEN_ITERS["x8"], r["raw"], tmp_path)


def test_more_node_records_than_lanes(tmp_path):
    """y9: 79 node records in a workgroup of 64 lanes -- the second trip of the staging loop and of the ranking loop; chunks
    of 3 slots: 3 + 3 + 2 loci, the last chunk the short one"""
    import run_hostemu
    import gphocs_amd as G
    mid = G.load_library(run_hostemu.build_hostemu(mid=True))
    r = check_against_restatement(mid, "y9", 4, tmp_path, chunk=3)
    pk = r["pack"]
    assert 2 * pk.n - 1 > 64 and pk.K >= 25          # what makes the workgroup 64 lanes wide and the records more than that
    assert r["oob"][0] == 0


def test_several_chunks_fold_in_chunk_order(hostemu, tmp_path):
    """chunks of 5 slots: four partial rows per sample; integers as with one chunk, sums within the bound, reproducible"""
    _, lib = hostemu
    one = run_chain(lib, "m3", 20, tmp_path, tag="one")["raw"]
    r = check_against_restatement(lib, "m3", 20, tmp_path, chunk=5)
    again = run_chain(lib, "m3", 20, tmp_path, tag="again", chunk=5)["raw"]
    assert r["raw"].tobytes() == again.tobytes()
    pk = r["pack"]
    npk = pk.n * (pk.n - 1) // 2 * pk.K
    ints = [0, 2, 4] + list(range(7, 7 + 2 * npk))
    assert r["raw"][:, ints].tolist() == one[:, ints].tolist()


def test_lifecycle_and_capacity(hostemu, tmp_path):
    """enable / disable / re-enable, fetch empties the buffer, a full buffer refuses the sample and keeps its rows"""
    import gphocs_amd as G
    _, lib = hostemu
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.coal_stats()                        # not enabled
        s.initialize()
        with pytest.raises(RuntimeError):
            s.sample_coal_stats(0)
        s.enable_coal_stats(3)
        for it in range(3):
            s.iteration(it)
            s.sample_coal_stats(it)
        s.iteration(3)
        with pytest.raises(BufferError):
            s.sample_coal_stats(3)
        assert s.lib.gph_engine_coal_stats_sample(s.engine, 3) == G.COAL_STATS_FULL == -5
        rows = s.coal_stats(raw=True)
        assert rows[:, 0].tolist() == [0.0, 1.0, 2.0]
        assert s.coal_stats(raw=True).shape[0] == 0        # the fetch emptied the buffer
        s.sample_coal_stats(3)                             # ... and there is room again
        t = s.coal_stats()
        assert len(t) == 1 and t[0]["iter"] == 3
        d = t[0]
        assert d["probCoal"].shape == (pk.n, pk.n, pk.K)
        assert np.array_equal(d["probCoal"], d["probCoal"].transpose(1, 0, 2)) and not d["probCoal"][np.arange(pk.n), np.arange(pk.n)].any()
        assert np.allclose(d["probCoal"].sum(axis=2) + np.eye(pk.n), 1.0, atol=1e-15, rtol=0)
        assert np.all(d["probFirstCoal"] <= d["probCoal"]) and np.all(d["meanCoal"][d["probCoal"] == 0] == 0)
        s.enable_coal_stats(0)
        with pytest.raises(RuntimeError):
            s.sample_coal_stats(4)
        s.enable_coal_stats(2)
        s.sample_coal_stats(4)
        assert s.coal_stats(raw=True)[:, 0].tolist() == [4.0]
    finally:
        s.close()


# ---------------------------------------------------------------- the program and the launcher
def gamma_lpdf(shape, rate, x):
    """log density of a gamma(shape, rate) distribution at x"""
    return shape * math.log(rate) - math.lgamma(shape) + (shape - 1.0) * math.log(x) - rate * x


def expected_files(ctl_dir, ctl, lib=None, sampler_lib=None):
    """{file suffix: text} the program must write: the documented divisions applied to the raw rows of an equivalent Sampler
    run (burn-in first, a sample wherever a trace line is written), printed with printCoalStats's formats"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    s = G.Sampler(p, lib=sampler_lib)
    priors, its = [], []
    try:
        s.enable_coal_stats(p.numSamplesMcmc)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.sample_coal_stats(it)
                st = s.state()
                lp = 0.0
                for k in range(p.K):
                    lp += gamma_lpdf(p.thetaAlpha[k], p.thetaBeta[k], st["theta"][k])
                for k in range(p.Kc, p.K):
                    lp += gamma_lpdf(p.ageAlpha[k], p.ageBeta[k], st["popAge"][k])
                for b in range(p.B):
                    lp += gamma_lpdf(p.mrAlpha[b], p.mrBeta[b], st["migRate"][b])
                priors.append(lp)
                its.append(it)
        raw = s.coal_stats(raw=True)
    finally:
        s.close()
    assert raw[:, 0].tolist() == its
    rows = np.hstack([raw, np.asarray(priors).reshape(-1, 1)])
    files = format_files(rows, p.n, p.K, p.L, _pop_names(os.path.join(ctl_dir, ctl)), printed_names(p.sampleNames))
    return files, its, p, rows


def format_files(rows, n, K, L, pops, names):
    """{file suffix: text} of records (raw row + logPrior): the documented divisions, printCoalStats's formats"""
    pidx = pair_index(n)
    files = {}
    lines = ["iter\tcoalStat\tnumCoal\tmigStat\tnumMig\tlogPrior\tlogGenLikelihood\tlogDataLikelihood"]
    for r in rows:
        lines.append("%7d\t%8f\t%9d\t%8f\t%9d\t%8f\t%8f\t%8f" % (int(r[0]), r[1], int(r[2]), r[3], int(r[4]), r[-1], r[5] + r[6], r[6]))
    files["coal.tsv"] = "\n".join(lines) + "\n"
    for k, pop in enumerate(pops):
        for st in ("probCoal", "probFirstCoal", "meanCoal"):
            lines = ["iter" + "".join(f"\t{a}|{b}|{pop}|{st}" for a in names for b in names)]
            for r in rows:
                _, cnt, first, agesum = split_row(r[:-1], n, K)
                vals = []
                for i in range(n):
                    for j in range(n):
                        if i == j:
                            vals.append(0.0)
                            continue
                        q = pidx[(min(i, j), max(i, j))]
                        c = cnt[q, k]
                        vals.append(c / L if st == "probCoal" else first[q, k] / L if st == "probFirstCoal" else (agesum[q, k] / c if c > 0 else 0.0))
                lines.append("%7d" % int(r[0]) + "".join("\t%8f" % v for v in vals))
            files[f"{pop}.{st}.tsv"] = "\n".join(lines) + "\n"
    return files




@pytest.mark.parametrize("name", ["g1", "j1"])
def test_program_writes_the_statistics_files(hostemu, tmp_path, name):
    path, lib = hostemu
    a, b, c = tmp_path / "with", tmp_path / "without", tmp_path / "small"
    for d in (a, b, c):
        _copy_case(name, d)
    _run(path, a, ["-s", "out", name + ".ctl"])
    _run(path, b, [name + ".ctl"])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), str(trace))
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    want, its, p, _ = expected_files(str(a), name + ".ctl", lib, lib)
    assert [int(ln.split("\t")[0]) for ln in _data_lines(trace)] == its
    assert sorted(got) == sorted(want)            # 1 + 3 K files, no part left behind
    assert len(got) == 1 + 3 * p.K
    for f in want:
        assert got[f].splitlines()[0] == want[f].splitlines()[0], f
        assert got[f] == want[f], f
    # a device buffer of 4 rows, flushed again and again: every row once, the same files
    _run(path, c, ["-s", "out", "--coal-stats-rows", "4", name + ".ctl"])
    assert len(its) > 3 * 4
    assert read_outputs(c, "out") == got


def test_burn_in_sample_skip_and_composition_with_the_locus_table(hostemu, tmp_path):
    path, lib = hostemu
    txt = open(os.path.join(GOLDEN, "m3.ctl")).read().replace("mcmc-iterations\t  120", "mcmc-iterations\t  40\n\tburn-in 7\n\tmcmc-sample-skip 2")
    assert "burn-in 7" in txt
    a, b = tmp_path / "s", tmp_path / "l"
    _copy_case("m3", a, txt)
    _copy_case("m3", b, txt)
    _run(path, a, ["-s", "out", "-l", "sum.tsv", "m3.ctl"])
    _run(path, b, ["-l", "sum.tsv", "m3.ctl"])
    assert open(a / "sum.tsv").read() == open(b / "sum.tsv").read()
    data = _data_lines(a / "m3.trace")
    want, its, _, _ = expected_files(str(a), "m3.ctl", lib, lib)
    assert its == list(range(0, 40, 3)) == [int(ln.split("\t")[0]) for ln in data]
    assert read_outputs(a, "out") == want


def read_part(path):
    """(n, K, row_doubles, L, records [samples][row_doubles + 1], trailer count) of a rank's PREFIX.coal.part<r>"""
    import struct
    b = open(path, "rb").read()
    assert b[:8] == b"GPHCS1\n\0"
    n, K, rd = struct.unpack_from("<3i", b, 8)
    L, = struct.unpack_from("<q", b, 20)
    nbytes, = struct.unpack_from("<i", b, 28)
    body = b[32 + nbytes:-8]
    count, = struct.unpack_from("<q", b, len(b) - 8)
    return n, K, rd, L, np.frombuffer(body, dtype=np.float64).reshape(-1, rd + 1), count


def check_ranks(lib_path, lib, name, tmp_path, rank_counts=(2, 3)):
    """item 7 at full precision.  The ranks' parts, added in rank order by gph_coal_stats_combined, against the one-rank
    rows: integers equal, fp64 sums within (2T + 4) * 2^-53 -- one rank and several ranks are two orderings of the same
    terms -- and bit for bit the rank-order sum this test forms itself from the part files.  The log-likelihoods and logPrior
    at parity_util.REL_TOL: the sampled migration rates follow from cross-rank sums, so the parameters logPrior is a function
    of agree between rank counts to that tolerance, not to the bit.  Then the files gph_coal_stats_write makes of them: the documented formats applied to those rows,
    written once, no part left; and the launcher's -g run gives the same files."""
    import gphocs_amd as G
    one_dir = tmp_path / "one"
    _copy_case(name, one_dir)
    _, its, p, one = expected_files(str(one_dir), name + ".ctl", lib, lib)
    n, K, L = p.n, p.K, p.L
    npk = n * (n - 1) // 2 * K
    pops, names = _pop_names(one_dir / (name + ".ctl")), printed_names(p.sampleNames)
    for ranks in rank_counts:
        d = tmp_path / f"w{ranks}"
        run_ranks(lib_path, name, ranks, d, coal_stats="out", coal_stats_rows=5)
        parts = [read_part(d / f"out.coal.part{r}") for r in range(ranks)]
        assert all(q[:4] == (n, K, 7 + 3 * npk, L) and q[5] == len(its) for q in parts)
        mine = parts[0][4].copy()
        for q in parts[1:]:
            mine[:, 1:-1] = mine[:, 1:-1] + q[4][:, 1:-1]
        comb = G.coal_stats_combined(lib, d / "out", ranks)
        assert comb.tobytes() == mine.tobytes(), f"{ranks} ranks: not the rank-order sum of the parts"
        ints = [0, 2, 4] + list(range(7, 7 + 2 * npk))
        assert comb[:, ints].tolist() == one[:, ints].tolist(), f"{ranks} ranks: integer columns"
        cnt = one[:, 7:7 + npk]
        for col, T in [(1, L * (n - 1)), (3, L * (n - 1))]:
            for g, w in zip(comb[:, col], one[:, col]):
                assert within_bound(float(g), float(w), T)[0], f"{ranks} ranks: column {col}: {g!r} vs {w!r}"
        G_, W_ = comb[:, 7 + 2 * npk:7 + 3 * npk], one[:, 7 + 2 * npk:7 + 3 * npk]
        for i, j in zip(*np.nonzero(G_ != W_)):
            assert within_bound(float(G_[i, j]), float(W_[i, j]), int(cnt[i, j]))[0], f"{ranks} ranks: agesum[{i}][{j}]"
        for col in (5, 6, comb.shape[1] - 1):
            assert np.all(np.abs(comb[:, col] - one[:, col]) <= REL_TOL * np.abs(one[:, col]))
        assert lib.gph_coal_stats_write(str(d / "out").encode(), ranks) == 0
        got = read_outputs(d, "out")
        assert got == format_files(comb, n, K, L, pops, names)           # no part among them: written once
        # the launcher: the same ranks, the same parts, the same files
        e = tmp_path / f"g{ranks}"
        _copy_case(name, e)
        _run(lib_path, e, ["-g", str(ranks), "-s", "out", "--coal-stats-rows", "5", name + ".ctl"])
        assert read_outputs(e, "out") == got
    # a part cut short (its record count gone) is refused, and nothing is left
    d = tmp_path / "cut"
    run_ranks(lib_path, name, 2, d, coal_stats="out", coal_stats_rows=5)
    b = open(d / "out.coal.part1", "rb").read()
    open(d / "out.coal.part1", "wb").write(b[:-8])
    assert lib.gph_coal_stats_write(str(d / "out").encode(), 2) != 0
    assert not read_outputs(d, "out")


@pytest.mark.parametrize("name", ["m3", "v8"])
def test_ranks_add_up_to_the_one_rank_rows(hostemu, tmp_path, name):
    path, lib = hostemu
    check_ranks(path, lib, name, tmp_path)


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run that fails AFTER rows were flushed to the parts (the device buffer holds one row; a directory sits where
    PREFIX.coal.tsv must be written): status non-zero, no part and no statistics file left -- one rank (the program's own
    path) and two (the launcher's); and the job that fails before it starts (more ranks than loci)"""
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("g1", d)
        os.mkdir(d / "out.coal.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["-s", "out", "--coal-stats-rows", "1", "g1.ctl"]
        env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "g1.trace").read().splitlines()) == 31        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.coal.tsv"] and not os.listdir(d / "out.coal.tsv")
    d = tmp_path / "z"
    _copy_case("z0", d)
    nloci = int(open(os.path.join(GOLDEN, "z0.seq")).read().split()[0])
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    r = subprocess.run([EXE, "-g", str(min(nloci * 2 + 1, 40)), "-s", "out", "z0.ctl"], cwd=d, capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode != 0
    assert not [f for f in os.listdir(d) if f.startswith("out.")]


def test_failed_run_leaves_no_statistics_file(hostemu, tmp_path):
    path, _ = hostemu
    check_failed_runs_leave_nothing(path, tmp_path)
