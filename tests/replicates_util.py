"""What the tests of the replicate chains share (test_replicates.py on the host build, test_replicates_gpu.py on the MI355X).

The model.  gph_engine_clades_compare is restated here in plain Python over Sampler.clades() of each chain: one dict
{key: cnt} per chain and locus, U = the union of the keys without the all-leaves key, and for every k in U the formulas of
include/gphocs_hip.h in their operand order -- f_r = c_r / S_r, m = (((f_0 + f_1) + ...) + f_R-1) / R,
v = (sum_r (f_r - m) (f_r - m)) / (R - 1), sd = math.sqrt(v), compared iff max_r f_r >= min_freq.  It never touches the kernel.

Tolerances.  The integer columns and `loci` are exact.  Every term is IEEE arithmetic in a fixed order, so only the order of
the sum over a locus's clades is free: with non-negative terms <= 0.71 two orders differ by at most (terms + a few roundings a
term) 2^-53, hence |asdsf - model| <= (compared + 64) 2.3e-16 with the row's own `compared`, |maxSd - model| <= 64 x 2.3e-16
(it is a maximum of equal terms: in fact equal), nothing looser anywhere.  gph_psrf is compared bit for bit (float.hex)."""
import copy
import ctypes as C
import math
import os

import numpy as np

EARG, ESTATE = -1, -4
CLS = 20                 # timing class of k_clades_compare
EPS = 2.3e-16
INT_COLS = ("compared", "distinct", "shared", "dropped")


def load(name):
    from sampler_util import load_pack
    return load_pack(name)


def seeded(pack, seed):
    q = copy.copy(pack)
    q.seed = seed
    return q


class Chains:
    """R plain Samplers of one pack, chain r seeded with seed + shift[r] (default r), clade tables on"""

    def __init__(self, lib, pack, R, slots, loci=None, shifts=None, trees=0, record=None):
        import gphocs_amd as G
        self.pack, self.s = pack, []
        for r in range(R):
            s = G.Sampler(seeded(pack, pack.seed + (shifts[r] if shifts else r)), lib=lib)
            self.s.append(s)
            if record and r == 0:
                s.set_record_file(record)
            if trees:
                s.enable_gene_trees(trees, loci)
            s.enable_clades(slots, loci)
            s.initialize()
        self.it = 0

    def run(self, iters, sample=True):
        for _ in range(iters):
            for s in self.s:
                s.iteration(self.it)
                if sample:
                    s.sample_clades()
            self.it += 1

    def close(self):
        for s in self.s:
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---------------------------------------------------------------- the model
def tables(s):
    """Sampler.clades() as (loci, samples, [per locus {key: cnt}], dropped[Q])"""
    c = s.clades()
    Q, W = len(c["loci"]), c["words"]
    out = []
    for q in range(Q):
        tab = {}
        for p in np.nonzero(c["cnt"][q])[0].tolist():
            tab[sum(int(c["keys"][q, p, w]) << (64 * w) for w in range(W))] = int(c["cnt"][q, p])
        assert len(tab) == int(np.count_nonzero(c["cnt"][q]))
        out.append(tab)
    return c["loci"].tolist(), int(c["samples"]), out, [int(d) for d in c["dropped"]]


def model_rows(samplers, n, min_freq):
    """the rows of the compare over these chains, from their fetched tables alone"""
    T = [tables(s) for s in samplers]
    R = len(T)
    loci = T[0][0]
    assert all(t[0] == loci for t in T)
    root = (1 << n) - 1
    rows = []
    for q in range(len(loci)):
        U = set()
        for t in T:
            U |= set(t[2][q])
        had_root = root in U
        U.discard(root)
        sds, shared = [], 0
        for k in sorted(U):
            c = [t[2][q].get(k, 0) for t in T]
            f = [float(c[r]) / float(T[r][1]) for r in range(R)]
            fs = 0.0
            for x in f:
                fs = fs + x
            m = fs / R
            ss = 0.0
            for x in f:
                ss = ss + (x - m) * (x - m)
            sd = math.sqrt(ss / (R - 1))
            shared += all(x > 0 for x in c)
            if max(f) >= min_freq:
                sds.append(sd)
        tot = 0.0
        for x in sds:
            tot = tot + x
        rows.append(dict(asdsf=tot / len(sds) if sds else 0.0, max_sd=max(sds) if sds else 0.0, compared=len(sds), distinct=len(U), shared=shared,
                         dropped=sum(t[3][q] for t in T), had_root=had_root))
    return loci, rows


def assert_rows(got, loci, rows, what):
    assert got["loci"].tolist() == loci, what
    for q, m in enumerate(rows):
        for k in INT_COLS:
            assert int(got[k][q]) == m[k], f"{what}: locus {loci[q]}: {k} {int(got[k][q])} != {m[k]}"
        da, dm = abs(float(got["asdsf"][q]) - m["asdsf"]), abs(float(got["max_sd"][q]) - m["max_sd"])
        assert da <= (m["compared"] + 64) * EPS, f"{what}: locus {loci[q]}: asdsf off by {da!r}"
        assert dm <= 64 * EPS, f"{what}: locus {loci[q]}: maxSd off by {dm!r}"
        assert 0.0 <= m["max_sd"] <= 0.7072 and m["asdsf"] <= m["max_sd"]


def compare(samplers, min_freq=0.1):
    import gphocs_amd as G
    return G.clades_compare(samplers, min_freq)


# ---------------------------------------------------------------- A: the kernel against the model
def check_against_model(lib, name, iters, slots, Rs=(2, 4), drops=None, min_freqs=(0.1,)):
    """max(Rs) chains sampled after every iteration; the compare of the first R of them for every R, at every min_freq.
    drops: True = every row must show dropped > 0, False = none may, None = whatever happens.  Returns {(R, F): got}"""
    pack = load(name)
    out = {}
    with Chains(lib, pack, max(Rs), slots) as ch:
        ch.run(iters)
        for R in Rs:
            for F in min_freqs:
                got = compare(ch.s[:R], F)
                loci, rows = model_rows(ch.s[:R], pack.n, F)
                assert loci == list(range(pack.L)) and len(rows) == pack.L
                assert_rows(got, loci, rows, f"{name} slots {slots} R {R} F {F}")
                assert all(r["had_root"] or r["dropped"] > 0 for r in rows)       # the trivial clade was there to be skipped
                if drops is True:
                    assert all(r["dropped"] > 0 for r in rows), f"{name} slots {slots}: a table did not fill"
                if drops is False:
                    assert all(r["dropped"] == 0 for r in rows), f"{name} slots {slots}: a table dropped clades"
                if slots >= 64:
                    assert all(r["distinct"] > r["shared"] for r in rows) and (R > 4 or any(r["shared"] > 0 for r in rows))
                out[(R, F)] = got
                print(f"{name} slots {slots} R {R} F {F}: compared {sorted(r['compared'] for r in rows)} distinct {sorted(r['distinct'] for r in rows)} "
                      f"asdsf {min(r['asdsf'] for r in rows):.4g} .. {max(r['asdsf'] for r in rows):.4g}")
        assert all(s.debug_oob()[0] == 0 for s in ch.s)
    return out


def check_min_freq(lib):
    """m3 at 2048 slots: min_freq 0, 0.1 and 1; the threshold changes `compared` and nothing else"""
    out = check_against_model(lib, "m3", 120, 2048, Rs=(2,), drops=False, min_freqs=(0.0, 0.1, 1.0))
    a, b, c = out[(2, 0.0)], out[(2, 0.1)], out[(2, 1.0)]
    assert np.all(a["compared"] == a["distinct"]) and np.all(a["compared"] > b["compared"]) and np.all(b["compared"] > 0)
    assert np.all(b["compared"] >= c["compared"])
    for k in ("distinct", "shared", "dropped"):
        assert a[k].tolist() == b[k].tolist() == c[k].tolist()


def check_hand_set_edges(lib):
    """a chain against a second chain of the same seed; the order of the chains permuted"""
    pack = load("m3")
    with Chains(lib, pack, 4, 2048, shifts=(0, 0, 1, 2)) as ch:
        ch.run(30)
        a, twin, b, c = ch.s
        got = compare([a, twin], 0.1)
        assert np.all(got["asdsf"] == 0.0) and np.all(got["max_sd"] == 0.0) and not np.any(np.signbit(got["asdsf"]))
        assert got["shared"].tolist() == got["distinct"].tolist() and np.all(got["compared"] > 0)
        loci, rows = model_rows([a, twin], pack.n, 0.1)
        assert_rows(got, loci, rows, "twins")
        first = compare([a, b, c], 0.1)
        loci, rows = model_rows([a, b, c], pack.n, 0.1)
        assert_rows(first, loci, rows, "a b c")
        for order in ([c, a, b], [b, c, a], [c, b, a]):
            other = compare(order, 0.1)
            for k in INT_COLS:
                assert other[k].tolist() == first[k].tolist(), k
            assert_rows(other, *model_rows(order, pack.n, 0.1), "permuted")
            assert np.all(np.abs(other["asdsf"] - first["asdsf"]) <= 2 * (first["compared"] + 64) * EPS)


# ---------------------------------------------------------------- B: group edges
def check_group_edges(lib, name="x8", iters=5, slots=64):
    """selections of 1, 3, 4, 5 loci and one with gaps: every row is the same locus's row of the all-loci compare, the fp columns
    bit for bit (same tables, same kernel); a selection beyond the rank's block launches nothing"""
    pack = load(name)
    L = pack.L
    assert L >= 9
    with Chains(lib, pack, 2, slots) as ch:
        ch.run(iters)
        full = compare(ch.s, 0.1)
        assert_rows(full, *model_rows(ch.s, pack.n, 0.1), "all loci")
    for sel in ([L - 1], [1, 2, 3], [L - 4, L - 3, L - 2, L - 1], [0, 1, 2, 3, 4], list(range(0, L, 3))):
        with Chains(lib, pack, 2, slots, loci=sel) as ch:
            ch.run(iters)
            got = compare(ch.s, 0.1)
            assert got["loci"].tolist() == sel
            for q, g in enumerate(sel):
                for k in INT_COLS:
                    assert int(got[k][q]) == int(full[k][g]), (sel, g, k)
                for k in ("asdsf", "max_sd"):
                    assert float(got[k][q]).hex() == float(full[k][g]).hex(), (sel, g, k)
    with Chains(lib, pack, 2, slots, loci=[L + 5]) as ch:
        ch.run(2)
        n0 = [s.host_stats()["launches"] for s in ch.s]
        got = compare(ch.s, 0.1)
        assert got["loci"].tolist() == [] and got["asdsf"].shape == (0,)
        assert [s.host_stats()["launches"] for s in ch.s] == n0 and ch.s[0].class_stats(CLS)["launches"] == 0


# ---------------------------------------------------------------- C: ordering and non-interference
def check_ordering(lib, tmp, name="m3", R=3, first=10, more=5, slots=0):
    """the compare right behind sample_clades() of all chains, no fetch between; again after more samples; nothing was written"""
    from rng_ahead_util import dump
    from test_clades import check_tables
    pack = load(name)
    iters = first + more

    def chain0(with_compare):
        tag = "with" if with_compare else "without"
        rec = os.path.join(str(tmp), f"{tag}.rec")
        with Chains(lib, pack, R if with_compare else 1, slots, trees=iters, record=rec) as ch:
            compares = 0
            s0 = ch.s[0].host_stats()["syncs"]
            for it in range(iters):
                for s in ch.s:
                    s.iteration(it)
                    s.sample_gene_trees(it)
                    s.sample_clades()
                if with_compare and it + 1 in (first, iters):
                    before = ch.s[0].host_stats()["syncs"]
                    got = compare(ch.s, 0.1)
                    assert ch.s[0].host_stats()["syncs"] == before + 1       # one host synchronisation a compare
                    compares += 1
                    loci, rows = model_rows(ch.s, pack.n, 0.1)                # (the tables fetched afterwards)
                    assert_rows(got, loci, rows, f"behind sample {it + 1}")
                    assert all(int(s.clades()["samples"]) == it + 1 for s in ch.s)
            assert s0 >= 0 and ch.s[0].class_stats(CLS)["launches"] == compares
            assert all(s.class_stats(CLS)["launches"] == 0 for s in ch.s[1:])
            for r, s in enumerate(ch.s):
                check_tables(s.clades(), s.gene_trees(), pack.n, f"chain {r} after the compares")
            ch.s[0].set_record_file(None)
            return open(rec).read(), dump(ch.s[0], os.path.join(str(tmp), f"{tag}.dump"), True)

    rec_a, dump_a = chain0(True)
    rec_b, dump_b = chain0(False)
    assert rec_a == rec_b and len(rec_a) > 1000 and dump_a == dump_b


def check_checked_build(lib):
    """the checked library: every index of k_clades_compare stays inside its array"""
    pack = load("m3")
    for slots in (0, 8, 512):
        with Chains(lib, pack, 3, slots) as ch:
            ch.run(12)
            got = compare(ch.s, 0.1)
            assert_rows(got, *model_rows(ch.s, pack.n, 0.1), f"checked slots {slots}")
            assert ch.s[0].debug_oob() == (0, 1)


# ---------------------------------------------------------------- D: refusals
def check_refusals(lib):
    """every GPH_EARG / GPH_ESTATE case leaves the engines usable: the same valid compare before and after"""
    import gphocs_amd as G
    pack, other = load("m3"), load("a7")
    with Chains(lib, pack, 3, 64) as ch, Chains(lib, pack, 1, 128) as wide, Chains(lib, pack, 1, 64, loci=[0, 2]) as fewer, \
            Chains(lib, other, 1, 64) as alien:
        for c in (ch, wide, fewer, alien):
            c.run(3)
        a, b, c3 = ch.s
        lib_ = a.lib
        off = G.Sampler(seeded(pack, pack.seed + 9), lib=lib_)
        off.initialize()
        empty = G.Sampler(seeded(pack, pack.seed + 9), lib=lib_)
        empty.enable_clades(64)
        empty.initialize()
        try:
            want = compare(ch.s, 0.1)
            Q = pack.L
            rows = np.full((Q, 6), -7.0)
            cnt = C.c_int64(-1)

            def call(engines, R=None, F=0.1, out=rows, max_loci=Q, count=cnt):
                hs = (C.c_void_p * max(len(engines), 1))(*engines)
                return lib_.gph_engine_clades_compare(hs, len(engines) if R is None else R, F, None if out is None else out.ctypes.data_as(C.POINTER(C.c_double)),
                                                      max_loci, None if count is None else C.byref(count))
            e = [s.engine for s in ch.s]
            assert call(e[:1]) == EARG and call(e, R=1) == EARG and call(e, R=17) == EARG and call(e, R=0) == EARG
            assert call([e[0], None]) == EARG and call([e[0], e[1], e[0]]) == EARG and call([e[0], e[0]]) == EARG
            for F in (-0.1, 1.5, math.nan, math.inf, -math.inf):
                assert call(e, F=F) == EARG
            assert call(e, max_loci=Q - 1) == EARG and call(e, max_loci=-1) == EARG and call(e, out=None) == EARG and call(e, count=None) == EARG
            assert lib_.gph_engine_clades_compare(None, 2, 0.1, rows.ctypes.data_as(C.POINTER(C.c_double)), Q, C.byref(cnt)) == EARG
            assert call([e[0], wide.s[0].engine]) == EARG                    # other slots
            assert call([e[0], fewer.s[0].engine]) == EARG                   # another selection
            if alien.s[0].lib is lib_:
                assert call([e[0], alien.s[0].engine]) == EARG               # another data set: leaves, selection
            else:
                assert call([e[0], alien.s[0].engine]) == EARG               # another library variant's engine
            assert call([e[0], off.engine]) == ESTATE and call([off.engine, e[0]]) == ESTATE      # tables not enabled
            assert call([e[0], empty.engine]) == ESTATE                      # no sample yet
            assert np.all(rows == -7.0) and cnt.value == -1                  # nothing was handed out
            with __import__("pytest").raises(ValueError):
                compare([a], 0.1)
            with __import__("pytest").raises(ValueError):
                compare(ch.s, 2.0)
            with __import__("pytest").raises(RuntimeError):
                compare([a, off], 0.1)
            again = compare(ch.s, 0.1)
            for k in want:
                assert want[k].tolist() == again[k].tolist(), k
            assert_rows(again, *model_rows(ch.s, pack.n, 0.1), "behind the refusals")
        finally:
            off.close()
            empty.close()


# ---------------------------------------------------------------- E: gph_psrf
def py_psrf(x):
    """the loop of include/gphocs_hip.h, operand for operand"""
    R, S = len(x), len(x[0])
    mean, sv, sm = [], 0.0, 0.0
    for r in range(R):
        s = 0.0
        for v in x[r]:
            s = s + v
        m = s / float(S)
        ss = 0.0
        for v in x[r]:
            d = v - m
            ss = ss + d * d
        mean.append(m)
        sv = sv + ss / float(S - 1)
        sm = sm + m
    Wv, M = sv / float(R), sm / float(R)
    sb = 0.0
    for m in mean:
        d = m - M
        sb = sb + d * d
    Bn = sb / float(R - 1)
    V = (float(S - 1) / float(S)) * Wv + Bn
    psrf = (1.0 if Bn == 0.0 else math.inf) if Wv == 0.0 else math.sqrt(V / Wv)
    return dict(mean=M, sd_within=math.sqrt(Wv), sd_between=math.sqrt(Bn), psrf=psrf)


def check_psrf(lib):
    import gphocs_amd as G
    import pytest
    rng = np.random.default_rng(20240611)
    for R in (2, 3, 16):
        for S in (2, 3, 120):
            for scale, shift in ((1.0, 0.0), (1e-3, 5000.0), (40.0, -300.0)):
                x = rng.standard_normal((R, S)) * scale + shift + rng.standard_normal((R, 1)) * scale * 0.3
                got, want = G.psrf(x, lib=lib), py_psrf(x.tolist())
                for k in want:
                    assert float(got[k]).hex() == float(want[k]).hex(), (R, S, k, got[k], want[k])
                assert got["psrf"] > 0 and got["sd_within"] > 0
    const = G.psrf(np.full((3, 7), 2.5), lib=lib)
    assert (const["mean"], const["sd_within"], const["sd_between"], const["psrf"]) == (2.5, 0.0, 0.0, 1.0)
    row = rng.standard_normal(9)
    same = G.psrf(np.stack([row, row]), lib=lib)
    assert same["sd_between"] == 0.0 and same["sd_within"] > 0 and 0.9 < same["psrf"] < 1.0
    assert float(same["psrf"]).hex() == float(py_psrf([row.tolist(), row.tolist()])["psrf"]).hex()
    apart = G.psrf(np.array([[1.0] * 5, [2.0] * 5]), lib=lib)
    assert apart["sd_within"] == 0.0 and apart["sd_between"] > 0 and apart["psrf"] == math.inf
    o = (C.c_double * 4)()
    x = np.zeros((2, 2))
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.gph_psrf(xp, 1, 2, o) == EARG and lib.gph_psrf(xp, 2, 1, o) == EARG and lib.gph_psrf(xp, 0, 0, o) == EARG
    assert lib.gph_psrf(None, 2, 2, o) == EARG and lib.gph_psrf(xp, 2, 2, None) == EARG and lib.gph_psrf(xp, 2, 2, o) == 0
    for bad in (np.zeros((1, 5)), np.zeros((3, 1)), np.zeros(4)):
        with pytest.raises(ValueError):
            G.psrf(bad, lib=lib)


# ---------------------------------------------------------------- F: the program
CASE = "m3"
OUTS = ["--clades", "cl", "--clades-slots", "2048", "-l", "sum.tsv", "-s", "cs", "--gene-trees", "gt"]
REP = ["--replicates", "3", "--replicates-out", "rep"]
ASDSF_HEADER = "locus name samples asdsf maxSd compared distinct shared dropped".split()


def program(lib_path, cwd, args, ok=True):
    from mc3_util import program as run
    return run(lib_path, cwd, args, ok)


def inputs(d):
    return sorted(f for f in os.listdir(str(d)) if f in (CASE + ".ctl", CASE + ".seq"))


def ctl_with_seed(shift):
    import re
    from conftest import GOLDEN
    txt = open(os.path.join(GOLDEN, CASE + ".ctl")).read()
    m = re.search(r"(random-seed\s+)(\d+)", txt)
    return txt[:m.start()] + m.group(1) + str(int(m.group(2)) + shift) + txt[m.end():]


def parse_asdsf(path):
    lines = open(str(path)).read().splitlines()
    assert lines[0].split("\t") == ASDSF_HEADER
    t = lines[-1].split()
    assert t[0] == "#" and t[1::2] == ["chains", "minfreq", "loci", "meanAsdsf", "maxAsdsf"]
    return [ln.split("\t") for ln in lines[1:-1]], dict(chains=int(t[2]), minfreq=float(t[4]), loci=int(t[6]), mean=t[8], max=t[10])


def check_program(lib_path, lib, tmp):
    """F: the run with --replicates 3 against the run without, the other chains' traces against plain runs of their seeds, the two
    tables against the model over three plain Samplers"""
    from mc3_util import pack_of
    from parity_util import compare_trace_files
    from sampler_util import _copy_case, _locus_names
    import gphocs_amd as G
    _copy_case(CASE, tmp / "plain")
    _copy_case(CASE, tmp / "rep")
    program(lib_path, tmp / "plain", OUTS + [CASE + ".ctl"])
    r = program(lib_path, tmp / "rep", REP + ["--replicates-every", "40"] + OUTS + [CASE + ".ctl"])
    skip = (CASE + ".ctl", CASE + ".seq")
    files = sorted(f for f in os.listdir(str(tmp / "plain")) if f not in skip)
    assert CASE + ".trace" in files and "sum.tsv" in files and any(f.startswith("cs.") for f in files)
    assert any(f.startswith("gt.") for f in files) and any(f.startswith("cl.") for f in files)
    for f in files:
        want = (tmp / "plain" / f).read_bytes()
        assert len(want) > 100 and (tmp / "rep" / f).read_bytes() == want, f
    assert sorted(f for f in os.listdir(str(tmp / "rep")) if f not in skip and f not in files) == \
        ["rep.asdsf.tsv", "rep.chain1.trace", "rep.chain2.trace", "rep.psrf.tsv"]
    # the other chains' traces: plain runs whose control file has random-seed + r
    for c in (1, 2):
        _copy_case(CASE, tmp / f"seed{c}", ctl_text=ctl_with_seed(c))
        program(lib_path, tmp / f"seed{c}", [CASE + ".ctl"])
        compare_trace_files(str(tmp / f"seed{c}" / (CASE + ".trace")), str(tmp / "rep" / f"rep.chain{c}.trace"))
    # three plain Samplers: what the chains are
    pack = pack_of(lib, tmp / "rep", CASE + ".ctl")
    header = open(str(tmp / "rep" / (CASE + ".trace"))).readline().rstrip("\n").split("\t")[1:]
    npar = pack.numParameters
    assert len(header) == npar + 2 and header[-2:] == ["Data-ld-ln", "Full-ld-ln"]
    pf = np.asarray(pack.printFactors, dtype=np.float64)
    iters = len(open(str(tmp / "rep" / (CASE + ".trace"))).read().splitlines()) - 1
    assert iters == 120
    x = [[] for _ in range(3)]
    with Chains(lib, pack, 3, 2048) as ch:
        for it in range(iters):
            for c, s in enumerate(ch.s):
                s.iteration(it)
                s.sample_clades()
                v = np.zeros(npar + 4)
                assert s.lib.gph_mcmc_param_vals(s.mcmc, v.ctypes.data, npar) == 0
                st = s.state()
                x[c].append([float(v[i] * pf[i]) for i in range(npar)] + [st["logLikelihood"], st["dataLogLikelihood"]])
        loci, rows = model_rows(ch.s, pack.n, 0.1)
    want = ["param\tmean\tsdWithin\tsdBetween\tpsrf"]
    worst = 0.0
    for i, name in enumerate(header):
        p = py_psrf([[x[c][s][i] for s in range(iters)] for c in range(3)])
        want.append("%s\t%.10g\t%.10g\t%.10g\t%.10g" % (name, p["mean"], p["sd_within"], p["sd_between"], p["psrf"]))
        worst = max(worst, p["psrf"])
    want.append("# chains 3 samples %d maxPsrf %.10g" % (iters, worst))
    assert open(str(tmp / "rep" / "rep.psrf.tsv")).read() == "\n".join(want) + "\n"
    got, tail = parse_asdsf(tmp / "rep" / "rep.asdsf.tsv")
    names = _locus_names(str(tmp / "rep" / (CASE + ".seq")))
    assert len(got) == len(rows) == pack.L and (tail["chains"], tail["minfreq"], tail["loci"]) == (3, 0.1, pack.L)
    printed = []
    for q, (g, m) in enumerate(zip(got, rows)):
        assert g[:3] == [str(loci[q]), names[loci[q]], str(iters)]
        assert [int(v) for v in g[5:]] == [m[k] for k in INT_COLS]
        assert abs(float(g[3]) - m["asdsf"]) <= (m["compared"] + 64) * EPS + 5e-10 * m["asdsf"]
        assert abs(float(g[4]) - m["max_sd"]) <= 64 * EPS + 5e-10 * m["max_sd"]
        assert m["dropped"] == 0 and m["compared"] > 0
        printed.append(float(g[3]))
    mean = 0.0
    for v in [m["asdsf"] for m in rows]:
        mean = mean + v
    mean = mean / len(rows)
    assert abs(float(tail["mean"]) - mean) <= 64 * EPS + 1e-9 * mean and abs(float(tail["max"]) - max(printed)) <= 1e-9 * max(printed)
    says = [ln for ln in r.stdout.replace("Replicates:", "\nReplicates:").splitlines() if ln.startswith("Replicates: sample ")]
    assert [ln.split()[2] for ln in says] == ["40:", "80:", "120:"] and len(says) == 3
    t = says[-1].split()
    assert t[3:5] == ["ASDSF", "mean"] and (t[5], t[6], t[7], t[8:]) == (tail["mean"], "max", tail["max"], ["over", str(pack.L), "loci"])


def check_program_without_clades(lib_path, tmp):
    from sampler_util import _copy_case
    _copy_case(CASE, tmp)
    r = program(lib_path, tmp, REP + [CASE + ".ctl"])
    assert sorted(f for f in os.listdir(str(tmp)) if f.startswith("rep.")) == ["rep.chain1.trace", "rep.chain2.trace", "rep.psrf.tsv"]
    assert "Replicates:" not in r.stdout
    assert len(open(str(tmp / "rep.psrf.tsv")).read().splitlines()) == 1 + 11 + 1


USAGE_ERRORS = [
    (["--replicates", "1", "--replicates-out", "rep"], "--replicates"), (["--replicates", "17", "--replicates-out", "rep"], "--replicates"),
    (["--replicates", "3"], "--replicates-out"), (["--replicates-out", "rep"], "--replicates"),
    (["--replicates-min-freq", "0.2"], "--replicates-min-freq"), (["--replicates-every", "2", "--clades", "cl"], "--replicates-every"),
    (REP + ["--replicates-min-freq", "1.5"], "--replicates-min-freq"), (REP + ["--replicates-min-freq", "-0.1"], "--replicates-min-freq"),
    (REP + ["--clades", "cl", "--replicates-every", "0"], "--replicates-every"), (REP + ["--replicates-every", "5"], "--replicates-every"),
    (REP + ["-g", "2"], "--replicates"), (REP + ["--mc3", "2"], "--replicates"), (REP + ["--beta", "0.5"], "--replicates"),
    (REP + ["--marginal-likelihood", "ml"], "--replicates")]
LIBRARY_REFUSALS = [
    (dict(replicates=1, replicates_out="rep"), "--replicates"), (dict(replicates=17, replicates_out="rep"), "--replicates"),
    (dict(replicates=-3, replicates_out="rep"), "--replicates"), (dict(replicates=3), "--replicates-out"),
    (dict(replicates_out="rep"), "--replicates"), (dict(replicates_min_freq=0.2), "--replicates-min-freq"),
    (dict(replicates_every=2, clades="cl"), "--replicates-every"), (dict(replicates=3, replicates_out="rep", replicates_min_freq=1.5), "--replicates-min-freq"),
    (dict(replicates=3, replicates_out="rep", replicates_min_freq=math.nan), "--replicates-min-freq"),
    (dict(replicates=3, replicates_out="rep", clades="cl", replicates_every=-1), "--replicates-every"),
    (dict(replicates=3, replicates_out="rep", replicates_every=5), "--replicates-every"),
    (dict(replicates=3, replicates_out="rep", comm=True), "--replicates"), (dict(replicates=3, replicates_out="rep", mc3=2), "--replicates"),
    (dict(replicates=3, replicates_out="rep", beta=0.5), "--replicates"), (dict(replicates=3, replicates_out="rep", marginal="ml"), "--replicates")]


def check_usage_error(lib_path, tmp, args, names):
    from sampler_util import _copy_case
    _copy_case(CASE, tmp)
    r = program(lib_path, tmp, args + [CASE + ".ctl"], ok=False)
    assert names in r.stderr and "Starting MCMC" not in r.stdout and "Reading control settings" not in r.stdout
    assert sorted(os.listdir(str(tmp))) == [CASE + ".ctl", CASE + ".seq"]


def check_library_refusal(lib, tmp, capfd, options, names):
    import gphocs_amd as G
    from sampler_util import _copy_case
    _copy_case(CASE, tmp)
    options = dict(options)
    comm = None
    if options.get("comm"):
        comm = lib.gph_comm_create_shm(("/gphocs-rep-%d" % os.getpid()).encode(), 0, 1)
        assert comm
        options["comm"] = comm
    cwd = os.getcwd()
    os.chdir(str(tmp))
    try:
        assert G.run_control_file(lib, CASE + ".ctl", **options) == EARG
    finally:
        os.chdir(cwd)
        if comm:
            lib.gph_comm_destroy(comm)
    assert names in capfd.readouterr().err and sorted(os.listdir(str(tmp))) == [CASE + ".ctl", CASE + ".seq"]


def check_failed_run_leaves_no_tables(lib_path, tmp):
    """a run that fails late -- a directory where rep.psrf.tsv must go -- exits non-zero and leaves no rep.*.tsv file"""
    from sampler_util import _copy_case
    _copy_case(CASE, tmp)
    os.mkdir(str(tmp / "rep.psrf.tsv"))
    (tmp / "rep.asdsf.tsv").write_text("stale\n")
    program(lib_path, tmp, REP + ["--clades", "cl", CASE + ".ctl"], ok=False)
    left = [f for f in os.listdir(str(tmp)) if f.startswith("rep.") and f.endswith(".tsv") and os.path.isfile(str(tmp / f))]
    assert left == [] and os.path.isdir(str(tmp / "rep.psrf.tsv"))
    assert not any(f.startswith("cl.") for f in os.listdir(str(tmp)))
