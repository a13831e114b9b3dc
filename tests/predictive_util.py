"""What tests/test_predictive.py (host-emulation build) and tests/test_predictive_gpu.py (-m gpu, the product libraries) share:
an independent restatement of include/gphocs_hip.h's posterior predictive definitions -- the generator in numpy uint64, the
thresholds with math.exp (glibc's exp; numpy's is not bound to its bits), the replicate, the statistics, the accumulators --
run over the chain's own gene-tree records, rates and the pack, and the check_* functions both files call.  Nothing here calls
the library to compute what it checks, and nothing has a tolerance: accumulator words are compared as float.hex, rows and
observed values as integers."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import compare_records
from sampler_util import load_pack

CLS = 22                # timing class of k_predictive
GT_O_DATALNL = 3        # gph_engine_gene_trees_shape: the offset of dataLnL in a record; FS_MUTRATE lies 4 doubles behind it
FULL, EARG, ESTATE = -5, -1, -4
CHECKPOINTS = (1, 2, 9)
M64 = (1 << 64) - 1
U = np.uint64


# ---------------------------------------------------------------- the definitions restated
def mix_int(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def mix_np(z):
    """mix64 over a numpy uint64 array (products wrap modulo 2^64)"""
    z = z ^ (z >> U(30))
    z = z * U(0xBF58476D1CE4E5B9)
    z = z ^ (z >> U(27))
    z = z * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def sample_key(seed, g, t):
    kl = mix_int(seed ^ mix_int(g + 0x9E3779B97F4A7C15))
    return mix_int(kl + t)


def thresholds(age, father, rate):
    """thr_v per node; None: the root (always fires)"""
    out = []
    for v, f in enumerate(father):
        if f < 0:
            out.append(None)
            continue
        ln = rate * (age[f] - age[v])
        q = 0.0 if ln < 1e-100 else 1 - math.exp(-4 * ln / 3.0)
        out.append(int(q * 9007199254740992.0))
    return out


def replicate(K, age, father, rate, n, sites):
    """bases [n][sites] of the replicate of one locus at one sample"""
    N = len(father)
    thr = thresholds(age, father, rate)
    s = np.arange(sites, dtype=np.uint64) << U(16)
    h = [mix_np(U(K) ^ (s | U(v))) for v in range(N)]
    fires = [np.ones(sites, bool) if thr[v] is None else (h[v] >> U(11)) < U(thr[v]) for v in range(N)]
    out = np.zeros((n, sites), dtype=np.int64)
    for i in range(n):
        done = np.zeros(sites, bool)
        v = i
        while True:
            take = fires[v] & ~done
            out[i][take] = (h[v][take] & U(3)).astype(np.int64)
            done |= take
            if father[v] < 0:
                break
            v = father[v]
        assert done.all()
    return out


def statistics(bases, missing, pops, Kc, weight=None):
    """the C sums over the sites (columns of `bases`, each counted `weight` times): python ints"""
    sites = bases.shape[1]
    w = np.ones(sites, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    cnt = np.zeros((Kc, 4, sites), dtype=np.int64)
    for i, p in enumerate(pops):
        for b in range(4):
            cnt[p, b] += (bases[i] == b) & ~missing[i]
    shown = (cnt.sum(axis=0) > 0).sum(axis=0)
    out = [int(((shown >= 2) * w).sum())]
    m = cnt.sum(axis=1)
    for p in range(Kc):
        for q in range(p, Kc):
            if p == q:
                d = (m[p] * m[p] - (cnt[p] * cnt[p]).sum(axis=0)) // 2
            else:
                d = m[p] * m[q] - (cnt[p] * cnt[q]).sum(axis=0)
            out.append(int((d * w).sum()))
    return out


def columns(pack, g):
    """(codes [U][n], counts [U]) of locus g: the first row of every group of phases"""
    r0, r1 = int(pack.pattern_offsets[g]), int(pack.pattern_offsets[g + 1])
    first = [r for r in range(r0, r1) if int(pack.numPhases[r]) != 0]
    return pack.leafcodes[first].astype(np.int64).reshape(len(first), pack.n), pack.counts[first].astype(np.int64)


def leaf_pops(pack):
    return [p for p in range(pack.Kc) for _ in range(int(pack.samplesPerPop[p]))]


def stat_names(Kc):
    return ["seg"] + [f"diff_{p}|{q}" for p in range(Kc) for q in range(p, Kc)]


def observed(pack, g):
    codes, counts = columns(pack, g)
    return statistics(codes.T, codes.T == 4, leaf_pops(pack), pack.Kc, counts), int(counts.sum())


def model_loci(pack, t, rates, seed, S, loci, t0=0):
    """per locus of `loci` (global indices = the records' loci) over the samples t0 .. t0 + S - 1 of the gene-tree records t
    (sample k of them has generator index k - t0): dict(acc [C][5], sites), and the per-sample rows [S][C] with the observed
    row [C]"""
    n, Kc, pops = pack.n, pack.Kc, leaf_pops(pack)
    C = 1 + Kc * (Kc + 1) // 2
    out, rows, obs_row = [], [[0] * C for _ in range(S)], [0] * C
    rec_loci = t["loci"].tolist()
    for g in loci:
        q = rec_loci.index(g)
        codes, counts = columns(pack, g)
        obs, sites = observed(pack, g)
        col = np.repeat(np.arange(len(counts)), counts)
        missing = (codes[col].T == 4) if sites else np.zeros((n, 0), bool)
        acc = [[float(obs[c]), 0.0, 0.0, 0.0, 0.0] for c in range(C)]
        for c in range(C):
            obs_row[c] += obs[c]
        for k in range(S):
            rec = t0 + k
            father = [int(f) for f in t["father"][rec, q]]
            age = [float(a) for a in t["age"][rec, q]]
            assert father[int(t["root"][rec, q])] < 0 and sum(f < 0 for f in father) == 1
            T = statistics(replicate(sample_key(seed, g, k), age, father, float(rates[rec, q]), n, sites), missing, pops, Kc)
            for c in range(C):
                x = float(T[c])
                a = acc[c]
                if x > a[0]:
                    a[1] = a[1] + 1.0
                if x == a[0]:
                    a[2] = a[2] + 1.0
                a[3] = a[3] + x
                a[4] = a[4] + x * x
                rows[k][c] += T[c]
        out.append(dict(acc=acc, sites=sites))
    return out, rows, obs_row


# ---------------------------------------------------------------- one chain, sampled
def run_chain(lib, name, iters, seed=4242, loci=None, tree_loci=None, checkpoints=(), sample=True, trees=True, record=None, final=None, pack=None,
              reset_at=None):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees and a predictive
    sample after every iteration; Sampler.predictive() is fetched (no reset) after each of `checkpoints` samples and at the
    end, the rows at the end"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci if tree_loci is None else tree_loci)
            s.predictive_enable(seed, iters, loci)
        s.initialize()
        hs0 = s.host_stats()
        at = {}
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                if reset_at == it:
                    s.predictive(reset=True)
                s.predictive_sample(it)
                if it + 1 in checkpoints:
                    at[it + 1] = s.predictive()
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        rows = None
        if sample:
            at[iters] = s.predictive()
            rows = s.predictive_rows()
        t = rates = None
        if sample and trees:
            off = s._gene_trees_shape()[3][GT_O_DATALNL]
            t = s.gene_trees(raw=True)
            rec = t["records"]
            rates = np.ascontiguousarray(rec[:, :, off + 32:off + 40]).view(np.float64)[:, :, 0] if rec.size else np.zeros(rec.shape[:2])
        if final:
            s.dump_state(final, True)
        return dict(pd=at, rows=rows, trees=t, rates=rates, pack=pk, stats=(hs0, hs1), launches=launches, oob=s.debug_oob(), seed=seed)
    finally:
        s.close()


def check_against_model(e, model, S, what):
    """every accumulator word as float.hex, obs and sites as integers"""
    Q, C = len(e["loci"]), len(e["stats"])
    assert e["samples"] == S and e["acc"].shape == (Q, C, 5) and len(model) == Q
    for q in range(Q):
        m, g = model[q], int(e["loci"][q])
        assert int(e["sites"][q]) == m["sites"], f"{what} S {S}: locus {g}: sites"
        for c in range(C):
            got, want = [float(v).hex() for v in e["acc"][q, c]], [float(v).hex() for v in m["acc"][c]]
            assert got == want, f"{what} S {S}: locus {g} statistic {e['stats'][c]}: {e['acc'][q, c].tolist()} != {m['acc'][c]}"
            assert int(e["acc"][q, c, 0]) == int(m["acc"][c][0])


def check_rows(r, rows, obs_row, iters, what):
    its, got, obs = r["rows"]
    assert its.tolist() == list(range(iters)), what
    assert [int(v) for v in obs] == obs_row, f"{what}: the observed row"
    assert [[int(v) for v in row] for row in got] == rows, f"{what}: the per-sample rows"


def check_case(lib, name, iters=9, checkpoints=CHECKPOINTS, loci=None, key="cpu", pack=None):
    """goldens, bit for bit: every fetch at the checkpoints against the model over the chain's own records"""
    r = run_chain(lib, name, iters, loci=loci, checkpoints=[c for c in checkpoints if c < iters], pack=pack)
    pk, t = r["pack"], r["trees"]
    sel = list(range(pk.L)) if loci is None else list(loci)
    assert r["launches"] == iters and r["oob"][0] == 0
    assert t["loci"].tolist() == sel
    moved = 0
    for S, e in sorted(r["pd"].items()):
        assert e["loci"].tolist() == sel and e["stats"] == stat_names(pk.Kc)
        model, rows, obs_row = model_loci(pk, t, r["rates"], r["seed"], S, sel)
        check_against_model(e, model, S, name)
    check_rows(r, rows, obs_row, iters, name)
    moved = sum(any(a[3] > 0.0 for a in m["acc"]) for m in model)
    print(f"{name} [{key}] n {pk.n} Kc {pk.Kc} loci {len(model)} samples {iters}: loci with a segregating replicate {moved}, "
          f"observed row {obs_row[:4]}, last row {rows[-1][:4]}")
    assert moved > 0, "no replicate of any locus ever showed a difference: the case checks nothing"
    return r, model


# ---------------------------------------------------------------- hand-made packs: the site loop's edges
EDGE_CTL = """GENERAL-INFO-START
	seq-file            e.seq
	trace-file          e.trace
	locus-mut-rate          CONST
	num-loci            1
	random-seed         31
	mcmc-iterations	  3
	iterations-per-log  1
	logs-per-line       10
	find-finetunes		FALSE
	finetune-coal-time	0.01
	finetune-mig-time	0.3
	finetune-theta		0.04
	finetune-mig-rate	0.02
	finetune-tau		0.0000008
	finetune-mixing		0.003
	tau-theta-print		10000.0
	tau-theta-alpha		1.0
	tau-theta-beta		100.0
	mig-rate-print		0.001
	mig-rate-alpha		0.002
	mig-rate-beta		0.00001
GENERAL-INFO-END
CURRENT-POPS-START
	POP-START
		name		A
		samples		a d
	POP-END
	POP-START
		name		B
		samples		b d
	POP-END
CURRENT-POPS-END
ANCESTRAL-POPS-START
	POP-START
		name			root
		children		A		B
		tau-initial	0.02
		tau-beta		50.0
		finetune-tau			0.0000008
	POP-END
ANCESTRAL-POPS-END
"""
EDGE_SEQ = "1\n\nl0 2 8\na\tACGTACGT\nb\tACGAACGT\n"


def edge_model(tmp_path, lib):
    """a pack of 4 leaves in 2 populations (two diploids) with large thetas and a deep root, so that replicates differ; its loci
    are replaced by edge_pack"""
    import gphocs_amd as G
    d = tmp_path / "edge-model"
    os.makedirs(d, exist_ok=True)
    (d / "e.ctl").write_text(EDGE_CTL)
    (d / "e.seq").write_text(EDGE_SEQ)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        p = G.Pack.from_control("e.ctl", lib=lib)
    finally:
        os.chdir(cwd)
    assert p.n == 4 and p.Kc == 2 and p.samplesPerPop.tolist() == [2, 2]
    return p


def edge_pack(base, loci):
    """`base` with its loci replaced: loci = a list of loci, each a list of (codes string, count) columns (one phase each)"""
    import copy
    import gphocs_amd as G
    p = copy.deepcopy(base)
    offs, leaf, ph, cnt = [0], [], [], []
    for cols in loci:
        for codes, count in cols:
            assert len(codes) == p.n
            leaf.append([G.Pack.CODES[ch] for ch in codes])
            ph.append(1)
            cnt.append(count)
        offs.append(offs[-1] + len(cols))
    p.L = p.numLoci = len(loci)
    p.pattern_offsets = np.array(offs, np.int64)
    p.leafcodes = np.array(leaf, np.uint8).reshape(-1, p.n)
    p.numPhases = G.encode_phases(ph)
    p.counts = np.array(cnt, np.int32)
    p.mutRates = np.ones(p.L)
    p.locusNames = [f"e{g}" for g in range(p.L)]
    return p


def _ones(k, start=0):
    """k distinct columns of count 1 (all sixteen two-population patterns in turn, some with an N)"""
    pats = ["AACC", "ACGT", "AAAA", "ANCC", "TTTA", "GCGC", "NAAT", "CCCG", "ATAT", "GGNC", "TACG", "CCAA", "AGGN", "TTTT", "CAGT", "GNNA"]
    return [(pats[(start + i) % len(pats)], 1) for i in range(k)]


def edge_loci(big_count=False):
    """the site-loop edges: 0 rows; 1, 63, 64, 65 and 257 sites; one column of count 130 followed by columns of count 1; a column of
    all N; a leaf that is N everywhere; a population that is entirely N in one column; big_count: one count of 70 000 (the
    block then keeps 32-bit counts)"""
    loci = [
        [],                                                        # 0 rows, 0 sites
        [("ACCA", 1)],                                             # 1 site
        [("AACC", 60)] + _ones(3),                                 # 63
        _ones(64),                                                 # 64: one row a site
        [("ACGT", 33), ("AACA", 32)],                              # 65
        [("AAAC", 200), ("ACAC", 50)] + _ones(7, 3),               # 257
        [("AACC", 130)] + _ones(20, 5),                            # a column spans several lane trips, then rows of one site
        [("NNNN", 40), ("AACG", 30)],                              # a column of all N
        [("NACC", 25), ("NAAA", 10), ("NCGT", 9)],                 # a leaf that is N everywhere
        [("NNAC", 31), ("ACNN", 29), ("AACT", 12)],                # a population entirely N in a column (m_p = 0)
        [("AAAA", 0), ("ACGT", 5), ("CCAA", 0)],                   # columns of count 0 own no site
        # more rows than a tile of the column table holds (4096 at 4 leaves): the second tile's sites go on where the first ended
        [(c, 1 + (i % 3 == 0)) for i, (c, _) in enumerate(_ones(4200, 7))],
    ]
    if big_count:
        loci.append([("AACC", 70000), ("ACCA", 3)])
    return loci


def check_edges(lib, base, big_count, iters=3, seed=99):
    pk = edge_pack(base, edge_loci(big_count))
    sites = [sum(c for _, c in cols) for cols in edge_loci(big_count)]
    assert sites[:7] == [0, 1, 63, 64, 65, 257, 150] and (not big_count or sites[-1] == 70003)
    r = run_chain(lib, "edges", iters, seed=seed, checkpoints=(1, 2), pack=pk)
    assert r["oob"][0] == 0 and r["launches"] == iters
    for S, e in sorted(r["pd"].items()):
        model, rows, obs_row = model_loci(pk, r["trees"], r["rates"], seed, S, list(range(pk.L)))
        check_against_model(e, model, S, f"edges (big {big_count})")
        assert e["sites"].tolist() == sites
        assert not e["acc"][0, :, (0, 1, 3, 4)].any() and e["acc"][0, :, 2].tolist() == [float(S)] * len(e["stats"])     # 0 sites: T = 0 = obs
    check_rows(r, rows, obs_row, iters, "edges")
    assert any(a[3] > 0.0 for m in model for a in m["acc"])
    return r


def check_refused_locus(lib, base, capfd):
    """sites x max n_p n_q = 2^32 exactly (2^30 sites, 2 x 2 leaves): refused by name, nothing enabled; the other locus alone is
    taken.  (The accepting side of the bound would simulate 2^30 - 1 sites: the rule's arithmetic is 64-bit integer, its other
    side is every other test)"""
    import gphocs_amd as G
    count = (1 << 32) // 4
    pk = edge_pack(base, [[("AACC", 5)], [("AACC", count // 2), ("ACCA", count - count // 2)]])
    s = G.Sampler(pk, lib=lib)
    try:
        capfd.readouterr()
        rc = s.lib.gph_engine_predictive_enable(s.engine, 1, 4, None, 0, 0)
        err = capfd.readouterr().err
        assert rc == EARG and "locus 1" in err and "2^32" in err, err
        assert s._predictive_shape() == (0, 0, 0, 0)
        with pytest.raises(ValueError):
            s.predictive_enable(1, 4)
        s.predictive_enable(1, 4, [0])                     # the other locus alone is fine
        assert s._predictive_shape()[0] == 1
        assert s.predictive()["acc"][0, :, 0].astype(np.int64).tolist() == observed(pk, 0)[0]
    finally:
        s.close()


# ---------------------------------------------------------------- selections, lifecycle, seed, the chain untouched
def check_selections(lib, name="m3", iters=4):
    """a stride (`0-5:2`) and the last locus alone: each row equals the same locus's row of the all-loci model (the key holds the
    GLOBAL locus index); the usage errors; a rank without a selected locus"""
    import gphocs_amd as G
    everything = run_chain(lib, name, iters)
    pk, t = everything["pack"], everything["trees"]
    L = pk.L
    for sel in ([0, 2, 4], [L - 1]):
        r = run_chain(lib, name, iters, loci=sel, trees=False)
        e = r["pd"][iters]
        assert e["loci"].tolist() == sel and r["launches"] == iters
        model, rows, obs_row = model_loci(pk, t, everything["rates"], r["seed"], iters, sel)
        check_against_model(e, model, iters, f"{name} selection {sel}")
        check_rows(r, rows, obs_row, iters, f"{name} selection {sel}")
    s = G.Sampler(pk, lib=lib)
    try:
        for bad in ([3, 2], [2, 2], [-1], [0, -1]):
            with pytest.raises(ValueError):
                s.predictive_enable(1, 4, bad)
            assert s.lib.gph_engine_predictive_enable(s.engine, 1, 4, (ctypes.c_int64 * len(bad))(*bad), len(bad), 0) == EARG
        assert s.lib.gph_engine_predictive_enable(s.engine, 1, -1, None, 0, 0) == EARG
        s.predictive_enable(1, 4, [L + 5])     # beyond the rank's block: ignored -- the rank takes its (zero) rows and launches nothing
        s.initialize()
        n0 = s.host_stats()["launches"]
        s.predictive_sample(0)
        s.predictive_sample(1)
        assert s.host_stats()["launches"] == n0 and s.class_stats(CLS)["launches"] == 0
        e = s.predictive()
        C = len(stat_names(pk.Kc))
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["acc"].shape == (0, C, 5)
        its, rows, obs = s.predictive_rows()
        assert its.tolist() == [0, 1] and not rows.any() and not obs.any()
    finally:
        s.close()


def check_lifecycle(lib, G, name="m3", iters=3):
    """reset (accumulators zeroed, obs formed again, t back at 0), enable twice, a full row buffer, GPH_EFULL with nothing
    allocated, GPH_ESTATE"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    L, C, cap = pk.L, len(stat_names(pk.Kc)), 2 * iters
    need = L * (C * 40 + 8) + C * 8 + ((pk.n + 15) & ~15) + cap * C * 8
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.predictive()                                 # not enabled
        assert s.lib.gph_engine_predictive_fetch_loci(s.engine, None, None, 0) == ESTATE
        assert s.lib.gph_engine_predictive_sample(s.engine, 0) == ESTATE
        assert s._predictive_shape() == (0, 0, 0, 0)
        s.predictive_enable(7, cap)
        assert s._predictive_shape() == (L, C, 0, 0)
        assert s.lib.gph_engine_predictive_sample(s.engine, 0) == ESTATE          # before initialize
        assert s.lib.gph_engine_predictive_enable(s.engine, 7, cap, None, 0, need - 1) == FULL
        assert s._predictive_shape() == (0, 0, 0, 0)       # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.predictive_enable(7, cap, max_bytes=need - 1)
        s.initialize()                                     # the engine is still usable
        with pytest.raises(RuntimeError):
            s.predictive_sample(0)
        s.predictive_enable(7, cap, [1, 2])                # enable twice: another selection, then the real one
        assert s._predictive_shape() == (2, C, 0, 0)
        s.predictive_enable(7, cap, max_bytes=need)
        want_obs = [observed(pk, g)[0] for g in range(L)]
        before = s.predictive()
        assert before["samples"] == 0 and before["acc"][:, :, 0].astype(np.int64).tolist() == want_obs and not before["acc"][:, :, 1:].any()
        for it in range(iters):
            s.iteration(it)
            s.predictive_sample(it)
        first = s.predictive(reset=True)
        assert first["samples"] == iters and first["acc"][:, :, 3].any()
        zero = s.predictive()
        assert zero["samples"] == 0 and zero["acc"].tobytes() == before["acc"].tobytes()
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.predictive_sample(it)
        assert s._predictive_shape() == (L, C, iters, cap)
        with pytest.raises(BufferError):
            s.predictive_sample(99)                        # the row buffer is full
        second = s.predictive()
        its, rows, obs = s.predictive_rows()
        assert its.tolist() == list(range(2 * iters)) and s._predictive_shape()[3] == 0
        assert [int(v) for v in obs] == [sum(o[c] for o in want_obs) for c in range(C)]
        s2 = G.Sampler(pk, lib=lib)                        # the same chain, sampled over the second half only: t restarts at 0
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.predictive_enable(7, cap)
                s2.iteration(it)
                if it >= iters:
                    s2.predictive_sample(it)
            fresh = s2.predictive()
            rows2 = s2.predictive_rows()[1]
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        assert second["acc"].tobytes() == fresh["acc"].tobytes() != first["acc"].tobytes()
        assert rows[iters:].tobytes() == rows2.tobytes()
        s.initialize()                                     # a new chain starts from zeroed accumulators and no rows
        again = s.predictive()
        assert again["samples"] == 0 and again["acc"].tobytes() == before["acc"].tobytes() and s._predictive_shape()[3] == 0
    finally:
        s.close()


def check_seed(lib, name="m3", iters=3):
    """two seeds give different s1; the same seed gives equal bits (and equal rows)"""
    a = run_chain(lib, name, iters, seed=1, trees=False)
    b = run_chain(lib, name, iters, seed=2, trees=False)
    c = run_chain(lib, name, iters, seed=1, trees=False)
    ea, eb, ec = a["pd"][iters], b["pd"][iters], c["pd"][iters]
    assert ea["acc"].tobytes() == ec["acc"].tobytes() and a["rows"][1].tobytes() == c["rows"][1].tobytes()
    assert ea["acc"][:, :, 3].tolist() != eb["acc"][:, :, 3].tolist()
    assert ea["acc"][:, :, 0].tolist() == eb["acc"][:, :, 0].tolist()          # the data do not depend on the seed
    big = run_chain(lib, name, 1, seed=(1 << 64) - 3, trees=True)           # a seed that uses all 64 bits
    model, _, _ = model_loci(big["pack"], big["trees"], big["rates"], (1 << 64) - 3, 1, list(range(big["pack"].L)))
    check_against_model(big["pd"][1], model, 1, f"{name} 64-bit seed")


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """records and final state dump with sampling on identical to a run with sampling off, and still the reference's records;
    launches of class 22 = the samples.  Returns the two runs"""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        r = run_chain(lib, name, full, sample=on, trees=False, record=rec, final=final, pack=G.Pack.load(os.path.join(GOLDEN, name + ".gpk")))
        out.append(dict(rec=rec, final=final, stats=r["stats"], launches=r["launches"], samples=r["pd"][full]["samples"] if on else 0))
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    return on, off


# ---------------------------------------------------------------- the model pinned by itself
def model_pair_differences(sites=400000, seed=777, locus=5, rate=1.3):
    """fixed 3-leaf tree ((0, 1), 2): leaf ages 0, 0, 0.002, internal ages 0.01 (node 3) and 0.03 (node 4, the root).  Per pair
    (differences, expected frequency)"""
    age, father = [0.0, 0.0, 0.002, 0.01, 0.03], [3, 3, 4, 4, -1]
    b = replicate(sample_key(seed, locus, 0), age, father, rate, 3, sites)
    out = []
    for i, j, lca in ((0, 1, 3), (0, 2, 4), (1, 2, 4)):
        d = 2 * age[lca] - age[i] - age[j]
        out.append((int((b[i] != b[j]).sum()), 0.75 * (1 - math.exp(-4 * rate * d / 3))))
    return out


def phase_groups(pack):
    """(locus, first row, rows) of every group of more than one phase"""
    out = []
    for g in range(pack.L):
        r, r1 = int(pack.pattern_offsets[g]), int(pack.pattern_offsets[g + 1])
        while r < r1:
            w = int(pack.numPhases[r])
            k = w if w < 0x8000 else 1 << (w & 31)
            assert k >= 1
            if k > 1:
                out.append((g, r, k))
            r += k
    return out


# ---------------------------------------------------------------- the program and the launcher
def _g(x):
    return "%.10g" % x


def expected_files(ctl_dir, ctl, spec_loci, seed=None, lib=None, sampler_lib=None):
    """the text of PREFIX.predictive.tsv and PREFIX.predictive-genome.tsv the program must write, formatted from the MODEL: an
    equivalent Sampler run (burn-in first) samples its gene trees wherever a trace line is written, and model_loci does the rest"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    sel = list(range(p.L)) if spec_loci is None else list(spec_loci)
    seed = p.seed if seed is None else seed
    its = [it for it in range(p.numSamplesMcmc) if it % (p.sampleSkip + 1) == 0]
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.enable_gene_trees(len(its), sel)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it in its:
                s.sample_gene_trees(it)
        off = s._gene_trees_shape()[3][GT_O_DATALNL]
        t = s.gene_trees(raw=True)
        rates = np.ascontiguousarray(t["records"][:, :, off + 32:off + 40]).view(np.float64)[:, :, 0]
    finally:
        s.close()
    S = len(its)
    model, rows, obs_row = model_loci(p, t, rates, seed & M64, S, sel)
    names = ["seg"] + [f"diff_{p.popName[a]}|{p.popName[b]}" for a in range(p.Kc) for b in range(a, p.Kc)]
    C = len(names)
    head = ["locus", "name", "samples", "sites"] + [f"{k}_{nm}" for nm in names for k in ("obs", "mean", "sd", "p")] + ["minP", "stat"]
    out, lowest = ["\t".join(head)], None
    for q, g in enumerate(sel):
        cells, minp, at = [], None, None
        for c in range(C):
            obs, gt, eq, s1, s2 = model[q]["acc"][c]
            mean = s1 / float(S) if S else 0.0
            var = (s2 - s1 * s1 / float(S)) / float(S - 1) if S > 1 else 0.0
            pv = (gt + eq / 2) / float(S) if S else 0.0
            two = 2 * min(pv, 1 - pv)
            if minp is None or two < minp:
                minp, at = two, c
            cells += [_g(obs), _g(mean), _g(math.sqrt(var) if var > 0.0 else 0.0), _g(pv)]
        if lowest is None or minp < lowest[0]:
            lowest = (minp, g)
        out.append("\t".join([str(g), p.locusNames[g], str(S), str(model[q]["sites"])] + cells + [_g(minp), names[at]]))
    lowest = lowest or (0.0, -1)
    out.append("# loci %d samples %d seed %d minMinP %s (locus %d)" % (len(sel), S, seed & M64, _g(lowest[0]), lowest[1]))
    gen = ["\t".join(["iter"] + names)] + ["%7d" % it + "".join("\t%d" % v for v in rows[k]) for k, it in enumerate(its)]
    pline = "p" + "".join("\t" + _g((sum(r[c] > obs_row[c] for r in rows) + sum(r[c] == obs_row[c] for r in rows) / 2) / float(S)) for c in range(C))
    gen += ["# observed" + "".join("\t%d" % v for v in obs_row),
            "# mean" + "".join("\t" + _g(float(sum(r[c] for r in rows)) / float(S)) for c in range(C)),
            "# " + pline, "# loci %d samples %d seed %d" % (len(sel), S, seed & M64)]
    return "\n".join(out) + "\n", "\n".join(gen) + "\n", "Predictive: " + pline


def check_program(lib_path, lib, tmp_path):
    """both files are the model's, character for character, and the log repeats the p line; --predictive-seed and
    --predictive-rows (a buffer that fills several times); the other options' files do not move; with --mc3 (no swaps) and
    --replicates the files are chain 0's = the plain run's; the usage errors"""
    import subprocess
    import gphocs_amd as G
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import PROGRAM_CASE, PROGRAM_LOCI, PROGRAM_SPEC, program_ctl
    name = PROGRAM_CASE
    ctl = name + ".ctl"
    a, b, c, d, e, m, r = (tmp_path / x for x in ("with", "without", "seed", "all", "rest", "mc3", "rep"))
    for x in (a, b, c, d, e, m, r):
        _copy_case(name, x, program_ctl(name))
    on = ["--predictive", "out", "--predictive-loci", PROGRAM_SPEC]
    run = _run(lib_path, a, on + [ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["predictive-genome.tsv", "predictive.tsv"]           # no part left behind
    want_loci, want_genome, want_log = expected_files(str(a), ctl, PROGRAM_LOCI, None, lib, lib)
    assert got["predictive.tsv"] == want_loci
    assert got["predictive-genome.tsv"] == want_genome
    assert want_log in run.stdout.splitlines()
    # another seed, a row buffer of 3 rows that fills four times, all loci
    _run(lib_path, c, ["--predictive", "out", "--predictive-seed", "18446744073709551614", "--predictive-rows", "3", ctl])
    other = read_outputs(c, "out")
    want_loci2, want_genome2, _ = expected_files(str(c), ctl, None, (1 << 64) - 2, lib, lib)
    assert other["predictive.tsv"] == want_loci2 and other["predictive-genome.tsv"] == want_genome2
    assert want_genome2.splitlines()[1:15] != want_genome.splitlines()[1:15]
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "--clades", "cl", "--clades-loci", "1-5", "--gene-trees", "gt", "--gene-trees-loci", "1-5", "--ess", "es"]
    _run(lib_path, d, on + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix, count in (("cl", 2), ("gt", 1), ("es", 2)):
        others = read_outputs(e, prefix)
        assert len(others) == count and read_outputs(d, prefix) == others
    assert open(d / (name + ".trace")).read() == open(e / (name + ".trace")).read() == open(trace).read()
    # chain 0 of a group of chains is the plain run's chain
    _run(lib_path, m, ["--mc3", "2", "--mc3-swap-every", "-1"] + on + [ctl])
    assert read_outputs(m, "out") == got
    _run(lib_path, r, ["--replicates", "2", "--replicates-out", "rep"] + on + [ctl])
    assert read_outputs(r, "out") == got
    # usage errors: they name the option, before anything is read, nothing written
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    L = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).L
    pre = ["--predictive", "out"]
    for args, words in ((["--predictive-loci", "0-3"], ["--predictive "]), (["--predictive-seed", "5"], ["--predictive "]), (["--predictive-rows", "4"], ["--predictive "]),
                        (pre + ["--predictive-loci", "0-4,3"], ["locus 3 ", "--predictive-loci"]), (pre + ["--predictive-loci", "5,5"], ["locus 5 ", "--predictive-loci"]),
                        (pre + ["--predictive-loci", f"3,{L}"], [f"locus {L} ", "--predictive-loci"]), (pre + ["--predictive-loci", "2-x"], ["2-x", "--predictive-loci"]),
                        (pre + ["--predictive-seed", "-4"], ["--predictive-seed"]), (pre + ["--predictive-seed", "7x"], ["--predictive-seed"]),
                        (pre + ["--predictive-rows", "0"], ["usage"])):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and all(w in res.stderr for w in words), (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    cwd = os.getcwd()
    os.chdir(u)
    try:
        p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        anylib = lib or G.load_library(dims=(p.n, p.K, p.B))
        for kw in (dict(predictive_loci="0-3"), dict(predictive_seed=5), dict(predictive_rows=4), dict(predictive="out", predictive_rows=-1)):
            assert G.run_control_file(anylib, ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, joined by gph_predictive_write, are the one-rank files -- per-locus rows concatenated, per-sample
    rows added (the key holds the global locus index) -- for all loci and for a selection that lies wholly in rank 1's block; the
    launcher does the same; a part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, predictive="out", predictive_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["predictive-genome.tsv", "predictive.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        assert [int(ln.split("\t")[0]) for ln in want["predictive.tsv"].splitlines()[1:-1]] == loci
        run_ranks(lib_path, name, 2, two, predictive="out", predictive_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.predictive.part0", "out.predictive.part1"]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.predictive.part{r}", cut)
            text = open(cut / "out.predictive.part1").read().splitlines(True)
            open(cut / "out.predictive.part1", "w").write("".join(text[:-1]))
            assert lib.gph_predictive_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_predictive_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                          # no part among them
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--predictive", "out", "--predictive-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.predictive-genome.tsv must be
    written: status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.predictive-genome.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--predictive", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.predictive-genome.tsv"] and not os.listdir(d / "out.predictive-genome.tsv")
