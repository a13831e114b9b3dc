"""Per-locus, per-sample migration ancestry (gph_engine_ancestry_*, `G-PhoCS-hip --ancestry PREFIX`) on the CPU: the
host-emulation build of the engine sources runs k_ancestry's workgroup body over the same pages.

The definitions are restated here in plain Python over state dumps (their N and M lines): the path of leaf i is i,
father(i), ..., root; a live migration node is on the path iff its branch is a node of the path; hit[b][i] = some live
migration of band b on the path of i, first[b][i] = the smallest age among those, any[i] = some hit[b][i].  Per locus
cnt += hit, age = age + first (where hit), any += any over the samples, in sample order: every raw column must be EQUAL to
the rebuilt one (the additions are plain fp64 additions owned by one lane), and every per-sample row must equal the
column sums of hit / any over the loci exactly.

m3, j1, a7 and x8 run on the default host build, b2 (20 bands: GPH_BIG_BANDS) and n7 (72 leaves: GPH_BIG_TREE) on the
host build with the reference's own caps."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import compare_records, compare_trace_files
from sampler_util import (EXE, _copy_case, _data_lines, _fmt, _locus_names, _pop_names, _run, hostemu_library, load_pack, printed_names,  # noqa: F401
                          read_outputs, run_ranks)

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

GOLDEN_ITERS = {"m3": 120, "j1": 150, "a7": 100, "x8": 24, "b2": 24, "n7": 12}
CASES = {"m3": 120, "j1": 80, "a7": 100, "x8": 24, "b2": 24, "n7": 12}      # samples with a state dump each
BIG = ("b2", "n7")
FULL = -5               # GPH_EFULL


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


# ---------------------------------------------------------------- the restatement, from state dumps
def parse_dump(path, K, B):
    """{global locus: dict(father{node}, migs [(branch, band, age)], nmig[B])} of a gph_engine_dump_loci dump"""
    loci, cur = {}, None
    for ln in open(path):
        t = ln.split()
        if not t:
            continue
        if t[0] == "LOCUS":
            cur = dict(father={}, migs=[], nmig=None)
            loci[int(t[1])] = cur
        elif t[0] == "N" and cur is not None:
            cur["father"][int(t[1])] = int(t[2])
        elif t[0] == "S" and cur is not None:
            v = t[1:]
            assert len(v) == 2 * K + 2 * B
            cur["nmig"] = [int(v[2 * K + 2 * b + 1]) for b in range(B)]
        elif t[0] == "M" and cur is not None:
            assert len(t) == 2 + int(t[1])
            for w in t[2:]:
                f = w.split(":")                     # mg:branch:band:spop:tpop:sev:tev:age
                cur["migs"].append((int(f[1]), int(f[2]), float.fromhex(f[7])))
    return loci


def restate(locus, n, B):
    """hit[b][i], first[b][i] (None where no hit), any[i] of one locus, and what the path of each leaf met"""
    father, migs = locus["father"], locus["migs"]
    hit = [[0] * n for _ in range(B)]
    first = [[None] * n for _ in range(B)]
    met = []
    for i in range(n):
        path, v = set(), i
        while v >= 0 and v not in path:
            path.add(v)
            v = father[v]
        on = [(band, age) for branch, band, age in migs if branch in path]
        met.append(on)
        for band, age in on:
            hit[band][i] = 1
            first[band][i] = age if first[band][i] is None else min(first[band][i], age)
    anyv = [1 if any(hit[b][i] for b in range(B)) else 0 for i in range(n)]
    return hit, first, anyv, met


def rebuild(dumps, n, B, L):
    """the accumulators and the per-sample rows rebuilt from the dumps in sample order, the invariants that tie hit to the
    pages' own migration counts, and the observations the vacuity conditions need"""
    cnt = [[[0.0] * n for _ in range(B)] for _ in range(L)]
    age = [[[0.0] * n for _ in range(B)] for _ in range(L)]
    anyc = [[0.0] * n for _ in range(L)]
    rows = []
    seen = dict(two_on_a_path=False, two_bands=False, shared_internal=False)
    for loci in dumps:
        assert sorted(loci) == list(range(L))
        row = [0] * (n * (B + 1))
        for g in range(L):
            hit, first, anyv, met = restate(loci[g], n, B)
            for b in range(B):
                # a band with live migrations reaches at least one leaf, a band without reaches none
                assert (loci[g]["nmig"][b] > 0) == (sum(hit[b]) > 0), f"locus {g} band {b}: nmig {loci[g]['nmig'][b]} vs hits {hit[b]}"
                for i in range(n):
                    if hit[b][i]:
                        cnt[g][b][i] += 1.0
                        age[g][b][i] = age[g][b][i] + first[b][i]
                        row[(1 + b) * n + i] += 1
            for i in range(n):
                anyc[g][i] += anyv[i]
                row[i] += anyv[i]
                seen["two_on_a_path"] |= len(met[i]) >= 2
                seen["two_bands"] |= len({band for band, _ in met[i]}) >= 2
            for branch, _, _ in loci[g]["migs"]:
                seen["shared_internal"] |= branch >= n and sum(1 for i in range(n) if branch in _path(loci[g], i)) >= 2
        rows.append(row)
    return cnt, age, anyc, rows, seen


def _path(locus, i):
    out, v = set(), i
    while v >= 0 and v not in out:
        out.add(v)
        v = locus["father"][v]
    return out


def run_chain(lib, name, iters, tmp, sample=True, dumps=False, record=None, capacity=None, tag=""):
    """one chain over golden `name` (lib None: the tightest capacity variant), a sample after every iteration: the raw
    accumulators, the per-sample rows with their iterations, the final state dump, the per-iteration dumps, the pack,
    host_stats() after initialize and at the end, debug_oob()"""
    import gphocs_amd as G
    pk = load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            s.enable_ancestry(capacity or iters)
        s.initialize()
        hs0 = s.host_stats()
        paths = []
        for it in range(iters):
            s.iteration(it)
            if sample:
                s.sample_ancestry(it)
            if dumps:
                p = str(tmp / f"{name}.{it}.dump")
                s.dump_state(p, False)
                paths.append(p)
        hs1 = s.host_stats()
        s.set_record_file(None)
        raw = s.ancestry_loci(raw=True) if sample else None
        its, rows = s.ancestry_rows() if sample else (None, None)
        final = str(tmp / f"{name}.final.{'s' if sample else 'n'}{'d' if dumps else ''}{tag}")
        s.dump_state(final, True)
        return dict(raw=raw, its=its, rows=rows, final=final, dumps=paths, pack=pk, stats=(hs0, hs1), oob=s.debug_oob())
    finally:
        s.close()


def expected_names(n, B):
    return [f"cnt.{b}.{i}" for b in range(B) for i in range(n)] + [f"age.{b}.{i}" for b in range(B) for i in range(n)] + \
           [f"any.{i}" for i in range(n)]


_SEEN = {}              # (which libraries, golden) -> what its dumps showed: the conditions over the whole case set


def check_against_dumps(lib, name, iters, tmp_path, key="cpu"):
    """items 1 and 2: sampled at every iteration with a state dump there -- raw columns and rows rebuilt from the dumps"""
    r = run_chain(lib, name, iters, tmp_path, dumps=True)
    pk, raw = r["pack"], r["raw"]
    n, K, B, L = pk.n, pk.K, pk.B, pk.L
    assert list(raw) == expected_names(n, B) + ["samples"]
    assert np.all(raw["samples"] == iters)
    assert r["its"].tolist() == list(range(iters)) and r["rows"].shape == (iters, n * (B + 1))
    cnt, age, anyc, rows, seen = rebuild([parse_dump(p, K, B) for p in r["dumps"]], n, B, L)
    partial = False
    for b in range(B):
        for i in range(n):
            assert raw[f"cnt.{b}.{i}"].tolist() == [cnt[g][b][i] for g in range(L)], f"{name}: cnt.{b}.{i} differs from the state dumps"
            assert raw[f"age.{b}.{i}"].tolist() == [age[g][b][i] for g in range(L)], f"{name}: age.{b}.{i} differs from the state dumps"
            partial = partial or any(0 < cnt[g][b][i] < iters for g in range(L))
    for i in range(n):
        got = raw[f"any.{i}"]
        assert got.tolist() == [anyc[g][i] for g in range(L)], f"{name}: any.{i} differs from the state dumps"
        assert np.all(got <= iters)
        for b in range(B):
            assert np.all(got >= raw[f"cnt.{b}.{i}"])
    assert r["rows"].tolist() == rows, f"{name}: a per-sample row is not the column sum of hit / any"
    assert partial, f"{name}: no cell with 0 < cnt < S -- the case shows nothing"
    _SEEN[(key, name)] = seen
    print(f"{name}: {seen}")
    return r


def check_chain_untouched(lib, name, iters, full, raw_d, tmp_path, tol=1e-12):
    """item 3: over the golden's whole run, records and final state dump with sampling on byte-identical to a run with sampling
    off and still the reference's records; the accumulators after `iters` samples are those of the run with dumps when the
    run is as long.  Returns the two runs."""
    rec_on, rec_off = str(tmp_path / "on.rtrace"), str(tmp_path / "off.rtrace")
    on = run_chain(lib, name, full, tmp_path, record=rec_on)
    off = run_chain(lib, name, full, tmp_path, sample=False, record=rec_off)
    assert open(rec_on).read() == open(rec_off).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(rec_on, os.path.join(GOLDEN, name + ".rtrace")) <= tol
    if full == iters:
        for col in raw_d:
            assert on["raw"][col].tolist() == raw_d[col].tolist(), f"{name}: two runs of the same chain differ in {col}"
    return on, off


def check_case_set(key, names):
    """the conditions against a vacuous pass that hold over the case set"""
    got = {c: any(_SEEN[(key, nm)][c] for nm in names) for c in ("two_on_a_path", "two_bands", "shared_internal")}
    assert got["two_on_a_path"], "no (sample, locus, leaf) with two live migrations on its path"
    assert got["two_bands"], "no leaf with hits in two different bands"
    assert got["shared_internal"], "no migration on an internal node's branch shared by several leaves"


@pytest.mark.parametrize("name", list(CASES))
def test_accumulators_and_rows_match_the_state_dumps_and_leave_the_chain_unchanged(hostemu, hostemu_big, tmp_path, name):
    lib = hostemu_big if name in BIG else hostemu[1]
    r = check_against_dumps(lib, name, CASES[name], tmp_path)
    check_chain_untouched(lib, name, CASES[name], GOLDEN_ITERS[name], r["raw"], tmp_path)
    assert r["oob"][0] == 0


def test_the_case_set_reaches_every_path(hostemu, hostemu_big, tmp_path):
    for name in CASES:
        if ("cpu", name) not in _SEEN:        # (run alone: the dumps of the cases not checked yet in this process)
            check_against_dumps(hostemu_big if name in BIG else hostemu[1], name, CASES[name], tmp_path)
    check_case_set("cpu", list(CASES))


def test_a_group_without_migrations_next_to_one_with(hostemu, tmp_path):
    """a70: 70 loci of 8 leaves are three workgroups of 32 slots (the last one cut by L), and live migrations are rare: a sample
    with fewer loci that hold one than there are workgroups has a workgroup that returns at the vote next to one that stays"""
    name, iters = "a70", 40
    r = check_against_dumps(hostemu[1], name, iters, tmp_path, key="edge")
    pk = r["pack"]
    per_group = 256 // pk.n
    groups = (pk.L + per_group - 1) // per_group
    assert groups >= 2 and pk.L % per_group
    with_migs = [sum(1 for d in parse_dump(p, pk.K, pk.B).values() if d["migs"]) for p in r["dumps"]]
    assert any(0 < k < groups for k in with_migs), with_migs
    assert r["oob"][0] == 0


# ---------------------------------------------------------------- capacity and lifecycle
def check_capacity(lib, G):
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.ancestry_loci()                          # not enabled
        need = pk.L * pk.n * (2 * pk.B + 1) * 8
        assert s.lib.gph_engine_ancestry_enable(s.engine, 2, need - 1) == FULL
        with pytest.raises(MemoryError):
            s.enable_ancestry(2, max_bytes=need - 1)
        s.initialize()                                 # the engine is still usable
        with pytest.raises(RuntimeError):
            s.sample_ancestry(0)
        s.enable_ancestry(2, max_bytes=need)
        for it in range(2):
            s.iteration(it)
            s.sample_ancestry(it)
        assert s.lib.gph_engine_ancestry_sample(s.engine, 2) == FULL
        with pytest.raises(BufferError):
            s.sample_ancestry(2)
        two = s.ancestry_loci(raw=True)
        assert np.all(two["samples"] == 2)             # the refused sample accumulated nothing
        its, rows = s.ancestry_rows()
        assert its.tolist() == [0, 1] and rows.shape == (2, pk.n * (pk.B + 1))
        s.sample_ancestry(2)                           # a free row again
        three = s.ancestry_loci(raw=True, reset=True)
        assert np.all(three["samples"] == 3)
        assert all(np.all(three[c] >= two[c]) for c in three if c.startswith(("cnt", "any")))
        zero = s.ancestry_loci(raw=True)
        assert np.all(zero["samples"] == 0) and all(not np.any(zero[c]) for c in zero)
        its, rows = s.ancestry_rows()                  # the reset of the accumulators keeps the rows taken
        assert its.tolist() == [2]
        s.iteration(3)
        s.sample_ancestry(3)
        one = s.ancestry_loci(raw=True)
        its, rows = s.ancestry_rows()
        assert its.tolist() == [3] and np.all(one["samples"] == 1)
        n, B = pk.n, pk.B
        assert rows[0].tolist() == [int(one[f"any.{i}"].sum()) for i in range(n)] + \
                                   [int(one[f"cnt.{b}.{i}"].sum()) for b in range(B) for i in range(n)]
        t = s.ancestry_loci()
        assert t["pAny"].shape == (pk.L, n) and t["p"].shape == (pk.L, B, n) and t["samples"] == 1
        assert t["age"][0, 0, 0] == (one["age.0.0"][0] / one["cnt.0.0"][0] if one["cnt.0.0"][0] > 0 else 0.0)
        s.enable_ancestry(0)
        with pytest.raises(RuntimeError):
            s.sample_ancestry(4)
    finally:
        s.close()


def test_capacity_limit_and_reset(hostemu):
    import gphocs_amd as G
    check_capacity(hostemu[1], G)


def test_a_model_without_bands_has_only_the_any_columns(hostemu, tmp_path):
    import gphocs_amd as G
    pk = G.Pack.load(os.path.join(GOLDEN, "g2.gpk"))
    assert pk.B == 0
    s = G.Sampler(pk, lib=hostemu[1])
    try:
        s.enable_ancestry(3)
        s.initialize()
        for it in range(3):
            s.iteration(it)
            s.sample_ancestry(it)
        raw = s.ancestry_loci(raw=True)
        assert list(raw) == [f"any.{i}" for i in range(pk.n)] + ["samples"]
        assert all(not np.any(raw[c]) for c in raw if c != "samples")
        its, rows = s.ancestry_rows()
        assert rows.shape == (3, pk.n) and not np.any(rows)
    finally:
        s.close()


# ---------------------------------------------------------------- the program and the launcher
def expected_files(ctl_dir, ctl, lib=None, sampler_lib=None):
    """{file suffix: text} the program must write: the formulas of README.md applied to the raw accumulators and rows of an
    equivalent Sampler run (burn-in first, a sample wherever a trace line is written)"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.enable_ancestry(p.numSamplesMcmc)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.sample_ancestry(it)
        raw = s.ancestry_loci(raw=True)
        its, rows = s.ancestry_rows()
    finally:
        s.close()
    S = int(raw["samples"][0])
    n, B = p.n, p.B
    pops = _pop_names(os.path.join(ctl_dir, ctl))
    names = printed_names(p.sampleNames)
    bands = [f"{pops[p.bandSrc[b]]}->{pops[p.bandTgt[b]]}" for b in range(B)]
    lines = ["\t".join(["locus", "name", "leaf", "sample", "samples", "pAny"] + [c for bd in bands for c in ("p_" + bd, "age_" + bd)])]
    for g in range(p.L):
        for i in range(n):
            a = raw[f"any.{i}"][g]
            if not a > 0:
                continue
            row = [str(g), p.locusNames[g], str(i), names[i], str(S), _fmt(a / S)]
            for b in range(B):
                c, t = raw[f"cnt.{b}.{i}"][g], raw[f"age.{b}.{i}"][g]
                row += [_fmt(c / S), _fmt(t / c if c > 0 else 0.0)]
            lines.append("\t".join(row))
    files = {"loci.tsv": "\n".join(lines) + "\n"}
    head = ["iter"] + [f"any_{names[i]}#{i}" for i in range(n)] + [f"{bd}|{names[i]}#{i}" for bd in bands for i in range(n)]
    lines = ["\t".join(head)] + ["%7d" % it + "".join("\t%9d" % v for v in r) for it, r in zip(its.tolist(), rows.tolist())]
    files["samples.tsv"] = "\n".join(lines) + "\n"
    return files, its.tolist(), p


def check_program(lib_path, lib, tmp_path, name="j1"):
    """item 6: the two files are the documented formulas applied to the raw accumulators; the trace is untouched and the
    golden's; two ranks write the same files and leave no part; the other options' files do not change"""
    a, b, c, d, e = (tmp_path / x for x in ("with", "without", "two", "all", "rest"))
    for x in (a, b, c, d, e):
        _copy_case(name, x)
    ctl = name + ".ctl"
    _run(lib_path, a, ["--ancestry", "out", ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), str(trace))
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    want, its, p = expected_files(str(a), ctl, lib, lib)
    assert [int(ln.split("\t")[0]) for ln in _data_lines(trace)] == its
    assert sorted(got) == ["loci.tsv", "samples.tsv"]             # no part left behind
    for f in want:
        assert got[f].splitlines()[0] == want[f].splitlines()[0], f
        assert got[f] == want[f], f
    rows = got["loci.tsv"].splitlines()[1:]
    assert 0 < len(rows) < p.L * p.n                                # all-zero rows are omitted, others are there
    seq_names = _locus_names(a / (name + ".seq"))
    keys = [(int(r.split("\t")[0]), int(r.split("\t")[2])) for r in rows]
    assert keys == sorted(keys) and all(r.split("\t")[1] == seq_names[k[0]] for r, k in zip(rows, keys))     # sequence-file order, then leaf order
    _run(lib_path, c, ["-g", "2", "--ancestry", "out", ctl])
    assert read_outputs(c, "out") == got
    assert not [f for f in os.listdir(c) if ".part" in f]
    _run(lib_path, d, ["--ancestry", "out", "-l", "sum.tsv", "-s", "cs", "--time-slices", "4", ctl])
    _run(lib_path, e, ["-l", "sum.tsv", "-s", "cs", "--time-slices", "4", ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    rest = read_outputs(e, "cs")
    assert len(rest) == 2 + 3 * p.K and read_outputs(d, "cs") == rest
    assert open(d / (name + ".trace")).read() == open(trace).read()


def test_program_writes_the_ancestry_files(hostemu, tmp_path):
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, the per-locus file is written, a directory sits where
    PREFIX.samples.tsv must be written: status non-zero, no part and no file of ours left, for one rank and for two; and the
    job that fails before it starts (more ranks than loci)"""
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.samples.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--ancestry", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.samples.tsv"] and not os.listdir(d / "out.samples.tsv")
    d = tmp_path / "z"
    _copy_case("z0", d)
    nloci = int(open(os.path.join(GOLDEN, "z0.seq")).read().split()[0])
    r = subprocess.run([EXE, "-g", str(min(nloci * 2 + 1, 40)), "--ancestry", "out", "z0.ctl"], cwd=d, capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode != 0
    assert not [f for f in os.listdir(d) if f.startswith("out.")]


def test_failed_run_leaves_no_ancestry_file(hostemu, tmp_path):
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)


def read_part(path):
    """(n, B, records [samples][1 + n (B + 1)] int32, per-locus text) of a rank's PREFIX.ancestry.part<r>"""
    b = open(path, "rb").read()
    assert b[:8] == b"GPHAN1\n\0"
    n, B, ri, nbytes = struct.unpack_from("<4i", b, 8)
    assert ri == n * (B + 1)
    count, tbytes = struct.unpack_from("<2q", b, len(b) - 16)
    body = 24 + nbytes
    assert len(b) == body + count * (ri + 1) * 4 + tbytes + 16
    rec = np.frombuffer(b[body:body + count * (ri + 1) * 4], dtype=np.int32).reshape(count, ri + 1)
    return n, B, rec, b[body + count * (ri + 1) * 4:len(b) - 16].decode()


def check_ranks(lib_path, lib, name, tmp_path, rank_counts=(1, 2, 3)):
    """item 4: the ranks' parts -- per-locus rows concatenated in rank order, per-sample rows added -- are the one-rank
    files, whether this test combines them itself or gph_ancestry_write does; a part cut short is refused and nothing is left"""
    one_dir = tmp_path / "one"
    _copy_case(name, one_dir)
    want, its, p = expected_files(str(one_dir), name + ".ctl", lib, lib)
    head = want["loci.tsv"].splitlines(True)[0]
    for ranks in rank_counts:
        d = tmp_path / f"w{ranks}"
        run_ranks(lib_path, name, ranks, d, ancestry="out", ancestry_rows=7)
        if ranks == 1:                 # one rank writes its files itself (a communicator of one included)
            assert read_outputs(d, "out") == want
            continue
        parts = [read_part(d / f"out.ancestry.part{r}") for r in range(ranks)]
        assert all(q[:2] == (p.n, p.B) and q[2][:, 0].tolist() == its for q in parts)
        assert head + "".join(q[3] for q in parts) == want["loci.tsv"], f"{ranks} ranks: the concatenated per-locus tables"
        added = sum(q[2][:, 1:].astype(np.int64) for q in parts)
        mine = "".join("%7d" % it + "".join("\t%9d" % v for v in r) + "\n" for it, r in zip(its, added.tolist()))
        assert want["samples.tsv"].splitlines(True)[0] + mine == want["samples.tsv"], f"{ranks} ranks: the added per-sample rows"
        assert lib.gph_ancestry_write(str(d / "out").encode(), ranks) == 0
        assert read_outputs(d, "out") == want                          # no part among them: written once
    d = tmp_path / "cut"
    run_ranks(lib_path, name, 2, d, ancestry="out", ancestry_rows=7)
    b = open(d / "out.ancestry.part1", "rb").read()
    open(d / "out.ancestry.part1", "wb").write(b[:-8])
    assert lib.gph_ancestry_write(str(d / "out").encode(), 2) != 0
    assert not read_outputs(d, "out")


def test_ranks_concatenate_and_add_up_to_the_one_rank_files(hostemu, tmp_path):
    path, lib = hostemu
    check_ranks(path, lib, "m3", tmp_path)
