"""Per-locus posterior summaries (gph_engine_locus_summary_*, `G-PhoCS-hip -l FILE`) on the CPU: the host-emulation build of
the engine sources runs k_locus_summary's per-locus body over the same pages.

The accumulators are rebuilt bit for bit from state dumps taken at every sample (the LOCUS / N / S / R lines, in the
engine's own operation order), sampling must leave the chain's trajectory byte for byte unchanged, and the program's
table must be the documented formulas applied to the engine's raw accumulators."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import compare_records, compare_trace_files
from sampler_util import EXE, _copy_case, _data_lines, _fmt, _locus_names, _pop_names, _run, hostemu_library  # noqa: F401

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

GOLDEN_ITERS = {"m3": 120, "a7": 100, "v8": 60, "j1": 150, "g1": 30}


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


# ---------------------------------------------------------------- the reference computation, from state dumps
def parse_dump(path, K, B):
    """{global locus: (dataLnL, genLnL, tmrca, rate or None, ncoal[K], nmig[B])} of a gph_engine_dump_loci dump"""
    loci, cur = {}, None
    for ln in open(path):
        t = ln.split()
        if not t:
            continue
        if t[0] == "LOCUS":
            cur = dict(g=int(t[1]), root=int(t[3]), data=float.fromhex(t[5]), gen=float.fromhex(t[7]), rate=None, age={})
            loci[cur["g"]] = cur
        elif t[0] == "R" and cur is not None:
            cur["rate"] = float.fromhex(t[1])
        elif t[0] == "N" and cur is not None:
            cur["age"][int(t[1])] = float.fromhex(t[5])
        elif t[0] == "S" and cur is not None:
            v = t[1:]
            assert len(v) == 2 * K + 2 * B
            cur["ncoal"] = [int(v[2 * k + 1]) for k in range(K)]
            cur["nmig"] = [int(v[2 * K + 2 * b + 1]) for b in range(B)]
    return {g: (d["data"], d["gen"], d["age"][d["root"]], d["rate"], d["ncoal"], d["nmig"]) for g, d in loci.items()}


def raw_from_dumps(dumps, K, B, var):
    """the accumulators, rebuilt in the kernel's operation order: shift = the first sample's value, then s1 += d, s2 += d * d
    with d = x - shift; counts summed as doubles; pmig = samples with a migration"""
    L = len(dumps[0])
    cols = {}

    def put(name, g, v):
        cols.setdefault(name, [0.0] * L)[g] = v

    for g in range(L):
        acc = {}
        for i, dmp in enumerate(dumps):
            data, gen, tmrca, rate, ncoal, nmig = dmp[g]
            moments = [("dataLnL", data), ("genLnL", gen), ("tmrca", tmrca)] + ([("rate", rate)] if var else [])
            for q, x in moments:
                if i == 0:
                    acc[q] = [x, 0.0, 0.0]
                else:
                    d = x - acc[q][0]
                    acc[q][1] = acc[q][1] + d
                    acc[q][2] = acc[q][2] + d * d
            for b in range(B):
                m = float(nmig[b])
                hit = 1.0 if m > 0.0 else 0.0
                acc[f"nmig.{b}"] = m if i == 0 else acc[f"nmig.{b}"] + m
                acc[f"pmig.{b}"] = hit if i == 0 else acc[f"pmig.{b}"] + hit
            for k in range(K):
                c = float(ncoal[k])
                acc[f"ncoal.{k}"] = c if i == 0 else acc[f"ncoal.{k}"] + c
        for q in ["dataLnL", "genLnL", "tmrca"] + (["rate"] if var else []):
            for j, m in enumerate(("shift", "s1", "s2")):
                put(f"{q}.{m}", g, acc[q][j])
        for key in [k for k in acc if "." in k]:
            put(key, g, acc[key])
    return cols


def expected_names(K, B, var):
    names = [f"{q}.{m}" for q in ("dataLnL", "genLnL", "tmrca") for m in ("shift", "s1", "s2")]
    names += [f"nmig.{b}" for b in range(B)] + [f"pmig.{b}" for b in range(B)] + [f"ncoal.{k}" for k in range(K)]
    return names + (["rate.shift", "rate.s1", "rate.s2"] if var else [])


def run_sampler(lib, name, iters, tmp, dumps=False, sample=True, record=None, fetch_at=None):
    """one chain over golden `name` (lib None: the tightest capacity variant): raw summaries after iteration fetch_at - 1
    (or None), the final state dump, the per-iteration dumps, the pack, host_stats() after initialize and at the end, and
    debug_oob() at the end"""
    import gphocs_amd as G
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            s.enable_locus_summary()       # before initialize: the rate columns of `locus-mut-rate VAR` appear there
        s.initialize()
        hs0 = s.host_stats()
        raw, paths = None, []
        for it in range(iters):
            s.iteration(it)
            if sample:
                s.sample_locus_summary()
            if dumps:
                p = str(tmp / f"{name}.{it}.dump")
                s.dump_state(p, False)
                paths.append(p)
            if fetch_at is not None and it + 1 == fetch_at:
                raw = s.locus_summary(raw=True)
        s.set_record_file(None)
        hs1 = s.host_stats()
        final = str(tmp / f"{name}.final.{'s' if sample else 'n'}{'d' if dumps else ''}")
        s.dump_state(final, True)
        return dict(raw=raw, final=final, dumps=paths, pack=pk, stats=(hs0, hs1), oob=s.debug_oob())
    finally:
        s.close()


def check_against_dumps(lib, name, iters, tmp_path):
    """1. sampled at every iteration, with a state dump there: the raw columns rebuilt from the dumps, bit for bit"""
    r = run_sampler(lib, name, iters, tmp_path, dumps=True, fetch_at=iters)
    raw_d, paths, pk = r["raw"], r["dumps"], r["pack"]
    var = int(getattr(pk, "mutRateMode", 0)) == 1
    assert list(raw_d) == expected_names(pk.K, pk.B, var) + ["samples"]
    assert np.all(raw_d["samples"] == iters)
    want = raw_from_dumps([parse_dump(p, pk.K, pk.B) for p in paths], pk.K, pk.B, var)
    for col, v in want.items():
        got = raw_d[col].tolist()
        assert got == v, f"{name}: raw column {col} differs from the state dumps"
    return r


def check_trajectory_unchanged(lib, name, iters, full, raw_d, tmp_path, tol=1e-12):
    """2. sampling without dumps over the golden's whole run (`full` iterations): records byte-identical to a run without
    sampling and still the reference's, the final state identical, and the summaries after `iters` iterations those of the
    run with dumps.  Returns the two runs."""
    rec_on, rec_off = str(tmp_path / "on.rtrace"), str(tmp_path / "off.rtrace")
    on = run_sampler(lib, name, full, tmp_path, record=rec_on, fetch_at=iters)
    off = run_sampler(lib, name, full, tmp_path, sample=False, record=rec_off)
    assert open(rec_on).read() == open(rec_off).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(rec_on, os.path.join(GOLDEN, name + ".rtrace")) <= tol
    for col in raw_d:
        assert on["raw"][col].tolist() == raw_d[col].tolist(), f"{name}: the dumps changed raw column {col}"
    return on, off


@pytest.mark.parametrize("name,iters", [("m3", 120), ("a7", 60), ("v8", 60), ("j1", 80)])
def test_summaries_match_state_dumps_and_leave_the_chain_unchanged(hostemu, tmp_path, name, iters):
    _, lib = hostemu
    r = check_against_dumps(lib, name, iters, tmp_path)
    check_trajectory_unchanged(lib, name, iters, GOLDEN_ITERS[name], r["raw"], tmp_path)
    assert r["oob"][0] == 0


def test_summary_lifecycle(hostemu, tmp_path):
    """enable / re-enable / reset / disable, and the derived table of the Python API"""
    import gphocs_amd as G
    _, lib = hostemu
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.locus_summary()                     # not enabled
        s.initialize()
        with pytest.raises(RuntimeError):
            s.sample_locus_summary()
        s.enable_locus_summary()
        for it in range(5):
            s.iteration(it)
            s.sample_locus_summary()
        raw = s.locus_summary(raw=True, reset=True)
        assert np.all(raw["samples"] == 5)
        assert s.locus_summary(raw=True)["samples"][0] == 0
        s.iteration(5)
        s.sample_locus_summary()
        one = s.locus_summary(raw=True)
        assert one["dataLnL.s1"].tolist() == [0.0] * pk.L and one["tmrca.s2"].tolist() == [0.0] * pk.L
        assert one["pmig.0"].tolist() == [1.0 if m > 0 else 0.0 for m in one["nmig.0"]]
        s.iteration(6)
        s.sample_locus_summary()
        t = s.locus_summary()
        r = s.locus_summary(raw=True)
        assert list(t)[:7] == ["samples", "dataLnL", "dataLnL_sd", "genLnL", "genLnL_sd", "tmrca", "tmrca_sd"]
        assert "mig_A->B" in t and "pmig_C->B" in t and "coal_root" in t
        assert t["dataLnL"].tolist() == [a + b / 2 for a, b in zip(r["dataLnL.shift"], r["dataLnL.s1"])]
        s.enable_locus_summary(False)
        with pytest.raises(RuntimeError):
            s.sample_locus_summary()
    finally:
        s.close()


# ---------------------------------------------------------------- the program and the launcher
def expected_table(ctl_dir, ctl, names_pop, lib=None, sampler_lib=None):
    """the table the program must write: the formulas of README.md applied to the raw accumulators of an equivalent Sampler
    run (the program's iteration loop: burn-in first, a sample wherever a trace line is written).  lib reads the control
    file, sampler_lib runs the chain (None: the tightest capacity variant, as the program picks it)"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.enable_locus_summary()
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.sample_locus_summary()
        raw = s.locus_summary(raw=True)
    finally:
        s.close()
    S = int(raw["samples"][0])
    K, B = p.K, p.B
    var = int(p.mutRateMode) == 1
    head = ["locus", "name", "samples", "dataLnL", "dataLnL_sd", "genLnL", "genLnL_sd", "tmrca", "tmrca_sd"]
    for b in range(B):
        band = f"{names_pop[p.bandSrc[b]]}->{names_pop[p.bandTgt[b]]}"
        head += ["mig_" + band, "pmig_" + band]
    head += ["coal_" + names_pop[k] for k in range(K)] + (["rate", "rate_sd"] if var else [])
    lines = ["\t".join(head)]

    def mom(q, g):
        sh, s1, s2 = raw[q + ".shift"][g], raw[q + ".s1"][g], raw[q + ".s2"][g]
        var_ = (s2 - s1 * s1 / S) / (S - 1) if S > 1 else 0.0
        return [_fmt(sh + s1 / S), _fmt(max(var_, 0) ** 0.5)]
    for g in range(p.L):
        row = [str(g), p.locusNames[g], str(S)] + mom("dataLnL", g) + mom("genLnL", g) + mom("tmrca", g)
        for b in range(B):
            row += [_fmt(raw[f"nmig.{b}"][g] / S), _fmt(raw[f"pmig.{b}"][g] / S)]
        row += [_fmt(raw[f"ncoal.{k}"][g] / S) for k in range(K)]
        if var:
            row += mom("rate", g)
        lines.append("\t".join(row))
    return "\n".join(lines) + "\n", S, p


@pytest.mark.parametrize("name", ["g1", "j1"])
def test_program_writes_the_summary_table(hostemu, tmp_path, name):
    path, lib = hostemu
    a, b = tmp_path / "with", tmp_path / "without"
    _copy_case(name, a)
    _copy_case(name, b)
    _run(path, a, ["-l", "sum.tsv", name + ".ctl"])
    _run(path, b, [name + ".ctl"])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), str(trace))
    assert not os.path.exists(b / "sum.tsv")
    got = open(a / "sum.tsv").read()
    pops = _pop_names(a / (name + ".ctl"))
    want, S, p = expected_table(str(a), name + ".ctl", pops, lib, lib)
    assert S == len(_data_lines(trace))
    rows = got.splitlines()
    assert len(rows) == 1 + p.L
    assert [r.split("\t")[1] for r in rows[1:]] == _locus_names(a / (name + ".seq"))
    assert rows[0] == want.splitlines()[0]
    assert got == want


def test_burn_in_and_sample_skip(hostemu, tmp_path):
    path, lib = hostemu
    txt = open(os.path.join(GOLDEN, "m3.ctl")).read().replace("mcmc-iterations\t  120", "mcmc-iterations\t  40\n\tburn-in 7\n\tmcmc-sample-skip 2")
    assert "burn-in 7" in txt
    _copy_case("m3", tmp_path, txt)
    _run(path, tmp_path, ["-l", "sum.tsv", "m3.ctl"])
    data = _data_lines(tmp_path / "m3.trace")
    assert data[0].split("\t")[0] == "0" and len(data) == 14       # iterations 0, 3, ..., 39
    got = open(tmp_path / "sum.tsv").read()
    want, S, _ = expected_table(str(tmp_path), "m3.ctl", _pop_names(tmp_path / "m3.ctl"), lib, lib)
    assert S == len(data)
    assert all(r.split("\t")[2] == str(S) for r in got.splitlines()[1:])
    assert got == want


@pytest.mark.parametrize("name", ["m3", "v8"])
def test_launcher_ranks_write_the_same_table(hostemu, tmp_path, name):
    path, _ = hostemu
    one = tmp_path / "g1"
    _copy_case(name, one)
    _run(path, one, ["-l", "sum.tsv", name + ".ctl"])
    want = open(one / "sum.tsv").read()
    for ranks in (2, 3):
        d = tmp_path / f"g{ranks}"
        _copy_case(name, d)
        _run(path, d, ["-g", str(ranks), "-l", "sum.tsv", name + ".ctl"])
        assert open(d / "sum.tsv").read() == want, f"-g {ranks}"
        assert not [f for f in os.listdir(d) if ".part" in f]


def test_failed_run_leaves_no_table(hostemu, tmp_path):
    """more ranks than loci: the job fails as a whole, and neither the table nor a part of it is left behind"""
    path, _ = hostemu
    _copy_case("z0", tmp_path)
    nloci = int(open(os.path.join(GOLDEN, "z0.seq")).read().split()[0])
    r = subprocess.run([EXE, "-g", str(min(nloci * 2 + 1, 40)), "-l", "sum.tsv", "z0.ctl"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, GPHOCS_HIP_LIB=path))
    assert r.returncode != 0
    assert not [f for f in os.listdir(tmp_path) if f.startswith("sum.tsv")]
