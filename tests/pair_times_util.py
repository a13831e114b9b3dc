"""What tests/test_pair_times.py (host-emulation build) and tests/test_pair_times_gpu.py (-m gpu, the product libraries) share: a
model of include/gphocs_hip.h's pairwise coalescence-time distributions that does NOT use the kernel's counting formula -- it
enumerates every leaf pair of a slot, finds the lca by climbing father pointers, and groups the leaf pairs by lca, which gives w_v
directly; the stated summation order is then applied in plain Python floats; `split` comes from Sampler.state()["popAge"] read at
each sample and from the pack's population fathers -- run over the chain's own gene-tree records, and the check_* functions both
files call.  Nothing here calls the library to compute what it checks, and nothing has a tolerance: A, Y, X, M are compared as
float.hex, rows as integers."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import compare_records
from sampler_util import load_pack
from triplets_util import lca_table, leaf_pops

CLS = 26                # timing class of k_pair_times
FULL, EARG, ESTATE = -5, -1, -4
CHECKPOINTS = (1, 2)
ROW_LDS_WORDS = 2048    # GPH_TR_ROW_LDS / 4: the numbers of a row that a workgroup sums in LDS first (csrc/gph_pairtimes.h)
DEFAULT_GRID = (1e-6, 1e-2, 34)


# ---------------------------------------------------------------- the definitions restated, by enumeration
def grid(lo, hi, B):
    """the program's --pair-times-grid LO,HI,B: E = B - 1 edges, geometric, the two ends exact"""
    E = B - 1
    return [lo if k == 0 else hi if k == E - 1 else lo * math.pow(hi / lo, float(k) / float(E - 1)) for k in range(E)]


EDGES = grid(*DEFAULT_GRID)


def leaf_pairs(pack, P, Q):
    a, b = int(pack.samplesPerPop[P]), int(pack.samplesPerPop[Q])
    return a * (a - 1) // 2 if P == Q else a * b


def all_pairs(pack):
    return [(P, Q) for P in range(pack.Kc) for Q in range(P, pack.Kc) if leaf_pairs(pack, P, Q) >= 1]


def column_names(pairs, B):
    return ([f"{P}|{Q}:{k}" for P, Q in pairs for k in range(B)] + [f"below_{P}|{Q}" for P, Q in pairs] + [f"loci_{P}|{Q}" for P, Q in pairs])


def ancestors(pop_father, p):
    out, a = [], int(pop_father[p])
    while a >= 0:
        out.append(a)
        a = int(pop_father[a])
        assert len(out) <= len(pop_father)
    return out


def split_of(pop_age, pop_father, P, Q):
    if P == Q:
        f = int(pop_father[P])
        return math.inf if f < 0 else float(pop_age[f])
    both = set(ancestors(pop_father, P)) & set(ancestors(pop_father, Q))
    return min(float(pop_age[a]) for a in both)


def bin_of(edges, a):
    return sum(1 for e in edges if e <= a)


def locus_sample(father, age, n, members, pairs, edges, splits):
    """one locus at one sample: per slot (hist [B], a, y, x, tmin).  members[p]: the leaves of population p"""
    lca = lca_table(father, n)
    B = len(edges) + 1
    out = []
    for (P, Q), split in zip(pairs, splits):
        w = {}
        if P == Q:
            lp = [(a, b) for i, a in enumerate(members[P]) for b in members[P][i + 1:]]
        else:
            lp = [(a, b) for a in members[P] for b in members[Q]]
        for a, b in lp:
            v = lca[a][b]
            w[v] = w.get(v, 0) + 1
        hist, s, y, tmin = [0] * B, 0.0, 0, math.inf
        for v in sorted(w):                                # node-index order; nodes with w_v = 0 do not occur
            assert v >= n
            hist[bin_of(edges, age[v])] += w[v]
            term = age[v] * float(w[v])
            s = s + term
            if age[v] < split:
                y += w[v]
            tmin = min(tmin, age[v])
        assert sum(hist) == len(lp) and y <= len(lp)
        out.append((hist, s, y, 1 if y > 0 else 0, tmin))
    return out


def model_loci(pack, t, pop_ages, S, loci, pairs, edges, t0=0):
    """per locus of `loci` over the samples t0 .. t0 + S - 1 of the gene-tree records t: A, Y, X, M [slots] (python floats), the
    per-sample x [S][locus][slot], and the per-sample rows [S][NP (B + 2)] (python ints)"""
    n, pops = pack.n, leaf_pops(pack)
    members = [[i for i in range(n) if pops[i] == p] for p in range(pack.Kc)]
    NP, B = len(pairs), len(edges) + 1
    accs, xs, rows = [], [[None] * len(loci) for _ in range(S)], [[0] * (NP * (B + 2)) for _ in range(S)]
    rec_loci = t["loci"].tolist()
    for qi, g in enumerate(loci):
        q = rec_loci.index(g)
        A, Y, X, M = [0.0] * NP, [0.0] * NP, [0.0] * NP, [0.0] * NP
        for k in range(S):
            rec = t0 + k
            father = [int(f) for f in t["father"][rec, q]]
            age = [float(a) for a in t["age"][rec, q]]
            assert father[int(t["root"][rec, q])] < 0 and sum(f < 0 for f in father) == 1
            splits = [split_of(pop_ages[rec], pack.popFather, P, Q) for P, Q in pairs]
            xs[k][qi] = []
            for sl, (hist, a, y, x, tmin) in enumerate(locus_sample(father, age, n, members, pairs, edges, splits)):
                A[sl] = A[sl] + a
                Y[sl] = Y[sl] + float(y)
                X[sl] = X[sl] + float(x)
                M[sl] = M[sl] + tmin
                xs[k][qi].append(x)
                for b in range(B):
                    rows[k][sl * B + b] += hist[b]
                rows[k][NP * B + sl] += y
                rows[k][NP * B + NP + sl] += x
        accs.append((A, Y, X, M))
    return accs, xs, rows


# ---------------------------------------------------------------- one chain, sampled
def run_chain(lib, name, iters, loci=None, pairs=None, edges=None, checkpoints=(), sample=True, trees=True, record=None, final=None, pack=None):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees and a pair-times sample
    after every iteration; Sampler.pair_times() is fetched (no reset) after each of `checkpoints` samples and at the end, the rows
    at the end; with `trees`, popAge of the chain state is read at every sample"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.pair_times_enable(iters, EDGES if edges is None else edges, loci, pairs)
        group = s._pair_times_shape()[2]
        s.initialize()
        hs0 = s.host_stats()
        at, pop_ages = {}, []
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                    pop_ages.append([float(a) for a in s.state()["popAge"]])
                s.pair_times_sample(it)
                if it + 1 in checkpoints:
                    at[it + 1] = s.pair_times()
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        rows = t = cols = None
        if sample:
            at[iters] = s.pair_times()
            cols = s.pair_times_columns()
            rows = s.pair_times_rows()
            if trees:
                t = s.gene_trees()
        if final:
            s.dump_state(final, True)
        return dict(pt=at, rows=rows, trees=t, pop_ages=pop_ages, pack=pk, stats=(hs0, hs1), launches=launches, oob=s.debug_oob(), group=group, columns=cols)
    finally:
        s.close()


def check_against_model(e, accs, S, what):
    """A, Y, X, M as float.hex"""
    Q, NP = len(e["loci"]), len(e["pairs"])
    assert e["samples"] == S and e["A"].shape == e["Y"].shape == e["X"].shape == e["M"].shape == (Q, NP) and len(accs) == Q
    for q in range(Q):
        g = int(e["loci"][q])
        for nm, want in zip("AYXM", accs[q]):
            got = [float(v).hex() for v in e[nm][q]]
            assert got == [float(v).hex() for v in want], f"{what} S {S}: locus {g} {nm}: {e[nm][q].tolist()} != {want}"


def check_rows(r, rows, iters, nsel, pack, what):
    """the rows as integers; the invariants on the device's own words"""
    its, got = r["rows"]
    e = r["pt"][iters]
    NP, B = len(e["pairs"]), len(e["edges"]) + 1
    assert its.tolist() == list(range(iters)), what
    assert got.shape == (iters, NP * (B + 2))
    assert [[int(v) for v in row] for row in got] == rows, f"{what}: the per-sample rows"
    for row in got:
        for sl, (P, Q) in enumerate(e["pairs"].tolist()):
            m = leaf_pairs(pack, P, Q)
            assert int(row[sl * B:(sl + 1) * B].sum()) == nsel * m
            assert int(row[NP * B + sl]) <= nsel * m and int(row[NP * B + NP + sl]) <= nsel


def check_case(lib, name, iters=9, checkpoints=CHECKPOINTS, loci=None, key=None, pack=None, pairs=None, edges=None):
    """bit for bit after 1, 2 and the last sample: every fetch against the enumeration over the chain's own records"""
    key = key or ("gpu" if lib is None else "given library")
    r = run_chain(lib, name, iters, loci=loci, pairs=pairs, edges=edges, checkpoints=[c for c in checkpoints if c < iters], pack=pack)
    pk, t = r["pack"], r["trees"]
    ed = EDGES if edges is None else list(edges)
    sel = list(range(pk.L)) if loci is None else list(loci)
    pr = all_pairs(pk) if pairs is None else [tuple(sorted(x)) for x in pairs]
    assert r["launches"] == iters and r["oob"][0] == 0
    assert t["loci"].tolist() == sel
    assert r["columns"] == column_names(pr, len(ed) + 1)
    for S, e in sorted(r["pt"].items()):
        assert e["loci"].tolist() == sel and e["pairs"].tolist() == [list(x) for x in pr]
        assert e["edges"].tobytes() == np.array(ed, dtype=np.float64).tobytes()
        accs, xs, rows = model_loci(pk, t, r["pop_ages"], S, sel, pr, ed)
        check_against_model(e, accs, S, name)
    check_rows(r, rows, iters, len(sel), pk, name)
    B = len(ed) + 1
    used = sorted({b for row in rows for sl in range(len(pr)) for b in range(B) if row[sl * B + b]})
    below = sum(row[len(pr) * B + sl] for row in rows for sl in range(len(pr)))
    print(f"{name} [{key}] n {pk.n} Kc {pk.Kc} pairs {len(pr)} bins {B} loci {len(sel)} samples {iters} G {r['group']}: bins used {used}, pairs below "
          f"their split {below}, row numbers {len(pr) * (B + 2)}")
    assert len(used) > 1 or B == 2, "every coalescence fell into one bin: the case checks nothing"
    r["xs"] = xs
    return r


# ---------------------------------------------------------------- the hand-made minimums
def _ctl(current, ancestral):
    return """GENERAL-INFO-START
	seq-file            t.seq
	trace-file          t.trace
	locus-mut-rate          CONST
	num-loci            2
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
""" + current + "CURRENT-POPS-END\nANCESTRAL-POPS-START\n" + ancestral + "ANCESTRAL-POPS-END\n"


TWO_CTL = _ctl("\tPOP-START\n\t\tname\t\tA\n\t\tsamples\t\ta h\n\tPOP-END\n\tPOP-START\n\t\tname\t\tB\n\t\tsamples\t\tb h\n\tPOP-END\n",
               "\tPOP-START\n\t\tname\t\t\troot\n\t\tchildren\t\tA\t\tB\n\t\ttau-initial\t0.005\n\t\ttau-beta\t\t200.0\n\t\tfinetune-tau\t\t\t0.0000008\n\tPOP-END\n")
TWO_SEQ = "2\n\nl0 2 8\na\tACGTACGT\nb\tACGAACGT\n\nl1 2 8\na\tACGTACGT\nb\tTCGTACGT\n"
ONE_CTL = _ctl("\tPOP-START\n\t\tname\t\tA\n\t\tsamples\t\ta h b h\n\tPOP-END\n", "")


def small_model(tmp_path, lib, which):
    """`two`: two populations of one haploid leaf each under one root, no band; `one`: one population with two haploid leaves"""
    import gphocs_amd as G
    d = tmp_path / f"min-{which}"
    os.makedirs(d, exist_ok=True)
    (d / "t.ctl").write_text(TWO_CTL if which == "two" else ONE_CTL)
    (d / "t.seq").write_text(TWO_SEQ)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        p = G.Pack.from_control("t.ctl", lib=lib)
    finally:
        os.chdir(cwd)
    assert p.n == 2 and p.L == 2 and p.B == 0
    assert (p.Kc, p.K, p.samplesPerPop.tolist()[:p.Kc]) == ((2, 3, [1, 1]) if which == "two" else (1, 1, [2]))
    return p


def check_two_populations(lib, pack, iters=8):
    """one slot (0, 1), one internal node: every row has exactly one count a locus, at bin(age[root]); y = 0 at every sample"""
    r = run_chain(lib, "two", iters, pack=pack, checkpoints=(1, 2))
    t = r["trees"]
    assert r["launches"] == iters and r["oob"][0] == 0
    B = len(EDGES) + 1
    its, rows = r["rows"]
    assert rows.shape == (iters, B + 2)
    for k in range(iters):
        want = [0] * (B + 2)
        for q in range(pack.L):
            assert int(t["root"][k, q]) == 2
            want[bin_of(EDGES, float(t["age"][k, q, 2]))] += 1
            assert float(t["age"][k, q, 2]) >= r["pop_ages"][k][2]           # no band: the coalescence lies above the split
        assert rows[k].tolist() == want
    for S, e in sorted(r["pt"].items()):
        assert e["pairs"].tolist() == [[0, 1]]
        accs, _, _ = model_loci(pack, t, r["pop_ages"], S, [0, 1], [(0, 1)], EDGES)
        check_against_model(e, accs, S, "two populations")
        assert not e["Y"].any() and not e["X"].any()
        for q in range(pack.L):
            A = 0.0
            for k in range(S):
                A = A + float(t["age"][k, q, 2])
            assert float(e["A"][q, 0]).hex() == A.hex() == float(e["M"][q, 0]).hex()
    return r


def check_one_population(lib, pack, iters=6):
    """the slot is (0, 0), split is +inf: y = 1 at every sample"""
    r = run_chain(lib, "one", iters, pack=pack, checkpoints=(1, 2))
    assert r["launches"] == iters and r["oob"][0] == 0
    B = len(EDGES) + 1
    its, rows = r["rows"]
    assert (rows[:, B] == pack.L).all() and (rows[:, B + 1] == pack.L).all() and (rows[:, :B].sum(axis=1) == pack.L).all()
    for S, e in sorted(r["pt"].items()):
        assert e["pairs"].tolist() == [[0, 0]]
        accs, _, _ = model_loci(pack, r["trees"], r["pop_ages"], S, [0, 1], [(0, 0)], EDGES)
        check_against_model(e, accs, S, "one population")
        assert e["Y"].tolist() == [[float(S)]] * pack.L and e["X"].tolist() == [[float(S)]] * pack.L
    return r


# ---------------------------------------------------------------- edges, group edges, pairs, invariants
def check_edges_that_are_ages(lib, name="m3", iters=3):
    """node ages of the chain's own records as edges, as bit patterns: an age equal to an edge lies in the upper bin; a grid of one
    edge and a grid of 127"""
    first = run_chain(lib, name, iters)
    pk, t = first["pack"], first["trees"]
    ages = np.unique(t["age"][:, :, pk.n:].reshape(-1))
    ages = ages[ages > 0.0]
    assert len(ages) >= 40
    for edges in (ages[::(len(ages) + 126) // 127], ages[len(ages) // 2:len(ages) // 2 + 1], ages[3:40:4]):
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        assert 1 <= len(edges) <= 127
        r = check_case(lib, name, iters=iters, edges=edges.tolist())
        hit = np.isin(r["trees"]["age"][:, :, pk.n:], edges).sum()
        assert r["trees"]["age"].tobytes() == t["age"].tobytes() and hit >= len(edges), "no age of the chain equals an edge"
    e127 = grid(1e-7, 1.0, 128)
    assert len(e127) == 127
    check_case(lib, name, iters=iters, edges=e127)


def check_group_edges(lib, name="a70", iters=2):
    """G - 1, G, G + 1 and 2 G + 1 selected loci for the kernel's own G, and the last locus of the rank alone"""
    everything = run_chain(lib, name, iters)
    pk, t, G_ = everything["pack"], everything["trees"], everything["group"]
    pr, L = all_pairs(pk), pk.L
    assert 1 < G_ and 2 * G_ + 1 <= L and pk.n >= 8
    accs, _, rows = model_loci(pk, t, everything["pop_ages"], iters, list(range(L)), pr, EDGES)
    check_against_model(everything["pt"][iters], accs, iters, name)
    check_rows(everything, rows, iters, L, pk, name)
    for sel in (list(range(1, G_)), list(range(L - G_, L)), list(range(0, G_ + 1)), list(range(2, 2 * G_ + 3)), [L - 1]):
        r = run_chain(lib, name, iters, loci=sel, trees=False)
        e = r["pt"][iters]
        assert e["loci"].tolist() == sel and r["launches"] == iters and r["group"] == G_
        accs, _, rows = model_loci(pk, t, everything["pop_ages"], iters, sel, pr, EDGES)
        check_against_model(e, accs, iters, f"{name} selection of {len(sel)}")
        check_rows(r, rows, iters, len(sel), pk, f"{name} selection of {len(sel)}")
    assert [len(x) for x in (list(range(1, G_)), list(range(L - G_, L)), list(range(0, G_ + 1)), list(range(2, 2 * G_ + 3)))] == [G_ - 1, G_, G_ + 1, 2 * G_ + 1]


def check_pair_lists(lib, name="j1", iters=3):
    """pairs given as (Q, P) and in another order than the default: the default run's slots permuted; a P = Q pair alone"""
    everything = run_chain(lib, name, iters, trees=False)
    full = everything["pt"][iters]
    pr = [tuple(x) for x in full["pairs"].tolist()]
    NPf, B = len(pr), len(EDGES) + 1
    for given in ([(4, 0), (3, 3), (2, 1), (0, 0), (3, 1)], [(2, 2)]):
        r = run_chain(lib, name, iters, pairs=given, trees=False)
        e = r["pt"][iters]
        NP = len(given)
        assert e["pairs"].tolist() == [sorted(x) for x in given] and r["columns"] == column_names([tuple(sorted(x)) for x in given], B)
        for j, x in enumerate(given):
            k = pr.index(tuple(sorted(x)))
            for nm in "AYXM":
                assert e[nm][:, j].tobytes() == full[nm][:, k].tobytes()
            got, want = r["rows"][1], everything["rows"][1]
            assert got[:, j * B:(j + 1) * B].tolist() == want[:, k * B:(k + 1) * B].tolist()
            assert got[:, NP * B + j].tolist() == want[:, NPf * B + k].tolist() and got[:, NP * B + NP + j].tolist() == want[:, NPf * B + NPf + k].tolist()
    assert full["A"].any() and full["M"].any()


def check_no_band_no_young_coalescence(lib, name, iters=6):
    """a model without a migration band: every below_ and loci_ column of a P < Q slot is 0 at every sample (the device's words)"""
    r = run_chain(lib, name, iters, trees=False)
    pk, e = r["pack"], r["pt"][iters]
    assert pk.B == 0 and pk.Kc >= 2
    NP, B = len(e["pairs"]), len(EDGES) + 1
    rows = r["rows"][1]
    cross = [sl for sl, (P, Q) in enumerate(e["pairs"].tolist()) if P < Q]
    assert cross and rows[:, :NP * B].any()
    for sl in cross:
        assert not rows[:, NP * B + sl].any() and not rows[:, NP * B + NP + sl].any()
        assert not e["Y"][:, sl].any() and not e["X"][:, sl].any()


def check_young_coalescence_needs_a_migration(lib, name="m3", iters=40):
    """a locus with x = 1 in a P < Q slot at a sample has num_migs > 0 in that sample's gene-tree record; x per sample is the step
    of the device's own X accumulator"""
    r = run_chain(lib, name, iters, checkpoints=range(1, iters))
    t = r["trees"]
    pairs = r["pt"][iters]["pairs"].tolist()
    cross = [sl for sl, (P, Q) in enumerate(pairs) if P < Q]
    prev, seen = None, 0
    for S in range(1, iters + 1):
        X = r["pt"][S]["X"]
        step = X if prev is None else X - prev
        prev = X
        assert ((step == 0.0) | (step == 1.0)).all()
        for q in range(X.shape[0]):
            if any(step[q, sl] == 1.0 for sl in cross):
                seen += 1
                assert int(t["num_migs"][S - 1, q]) > 0, f"sample {S - 1} locus {q}: a coalescence below the split without a migration"
    print(f"{name}: (sample, locus) with a cross-population coalescence below the split {seen}")
    assert seen > 0, "no locus ever coalesced below a split: the case checks nothing"


# ---------------------------------------------------------------- refusals, lifecycle
def check_refusals(lib, capfd, one_pop_one_leaf, name="j1"):
    """GPH_EARG with a message that names the cause, the sampler left as it was"""
    import gphocs_amd as G
    pk = load_pack(name)
    L, Kc = pk.L, pk.Kc
    s = G.Sampler(pk, lib=lib)
    good = [1e-4, 1e-3]

    def refused(loci, pairs, edges, *words):
        la = None if loci is None else (ctypes.c_int64 * max(len(loci), 1))(*loci)
        pa = None if pairs is None else (ctypes.c_int32 * (2 * len(pairs)))(*[x for p in pairs for x in p])
        ea = (ctypes.c_double * max(len(edges), 1))(*edges)
        before = (s._pair_times_shape(), s.pair_times_columns())
        capfd.readouterr()
        rc = s.lib.gph_engine_pair_times_enable(s.engine, 4, la, 0 if loci is None else len(loci), pa, 0 if pairs is None else len(pairs), ea, len(edges), 0)
        err = capfd.readouterr().err
        assert rc == EARG and "pair times" in err and all(w in err for w in words), (loci, pairs, edges, err)
        assert (s._pair_times_shape(), s.pair_times_columns()) == before
        with pytest.raises(ValueError):
            s.pair_times_enable(4, edges, loci, pairs)

    try:
        for on in (False, True):
            if on:
                s.pair_times_enable(4, good, [1, 2], [(0, 1)])
                assert s._pair_times_shape()[:2] + s._pair_times_shape()[3:] == (1, 3, 2, 0, 0)
            refused(None, [(0, Kc)], good, "pair 0", f"population {Kc}")
            refused(None, [(0, 1), (-1, 2)], good, "pair 1", "population -1")
            refused(None, [(0, 1), (1, 0)], good, "pair 1", "twice")
            refused(None, [(2, 2), (2, 2)], good, "pair 1", "twice")
            refused([0, L], None, good, f"locus {L}", "out of range")
            refused([-1], None, good, "locus -1", "out of range")
            refused([2, 2], None, good, "locus 2", "twice")
            refused([3, 2], None, good, "locus 2", "increasing")
            refused(None, None, [], "0 edges")
            refused(None, None, [1e-6 * (k + 1) for k in range(128)], "128 edges")
            refused(None, None, [1e-4, math.inf], "edge 1", "finite")
            refused(None, None, [math.nan], "edge 0", "finite")
            refused(None, None, [0.0, 1e-3], "edge 0", "positive")
            refused(None, None, [-1e-3], "edge 0", "positive")
            refused(None, None, [1e-4, 1e-3, 1e-3], "edge 2", "above")
            refused(None, None, [1e-3, 1e-4], "edge 1", "above")
        assert s.lib.gph_engine_pair_times_enable(s.engine, -1, None, 0, None, 0, (ctypes.c_double * 1)(1e-3), 1, 0) == EARG
    finally:
        s.close()
    s = G.Sampler(one_pop_one_leaf, lib=lib)               # two populations of one leaf each: (0, 0) has no leaf pair
    try:
        capfd.readouterr()
        ea = (ctypes.c_double * 2)(*good)
        assert s.lib.gph_engine_pair_times_enable(s.engine, 4, None, 0, (ctypes.c_int32 * 2)(0, 0), 1, ea, 2, 0) == EARG
        assert "population 0 has fewer than two samples" in capfd.readouterr().err
        assert s._pair_times_shape() == (0, 0, 0, 0, 0, 0)
        with pytest.raises(ValueError):
            s.pair_times_enable(4, good, pairs=[(1, 1)])
        s.pair_times_enable(4, good)                       # the default skips the pairs without a leaf pair
        assert s.pair_times()["pairs"].tolist() == [[0, 1]]
    finally:
        s.close()


def check_lifecycle(lib, G, name="m3", iters=3):
    """reset, enable twice, a full row buffer, GPH_EFULL one byte short with the feature off, GPH_ESTATE, disable, a rank without a
    selected locus"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    L, NP, cap, E = pk.L, len(all_pairs(pk)), 2 * iters, len(EDGES)
    B = E + 1
    o_edge = (L * NP * 32 + NP * 4 + 15) & ~15             # behind the accumulators: the pair table, the edges, the leaf bytes
    o_pop = (o_edge + E * 8 + 15) & ~15
    need = o_pop + ((pk.n + pk.Kc + 15) & ~15) + cap * NP * (B + 2) * 8
    s = G.Sampler(pk, lib=lib)
    off = (0, 0, 0, 0, 0, 0)
    try:
        with pytest.raises(RuntimeError):
            s.pair_times()                                 # not enabled
        with pytest.raises(RuntimeError):
            s.pair_times_rows()
        assert s.lib.gph_engine_pair_times_fetch_loci(s.engine, None, 0, 0) == ESTATE
        assert s.lib.gph_engine_pair_times_sample(s.engine, 0) == ESTATE
        assert s._pair_times_shape() == off
        s.pair_times_enable(cap, EDGES)
        G_ = s._pair_times_shape()[2]
        assert s._pair_times_shape() == (NP, B, G_, L, 0, 0) and 1 <= G_ <= 32
        assert s.lib.gph_engine_pair_times_sample(s.engine, 0) == ESTATE            # before initialize
        ea = (ctypes.c_double * E)(*EDGES)
        assert s.lib.gph_engine_pair_times_enable(s.engine, cap, None, 0, None, 0, ea, E, need - 1) == FULL
        assert s._pair_times_shape() == off                # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.pair_times_enable(cap, EDGES, max_bytes=need - 1)
        s.initialize()                                     # the engine is still usable
        with pytest.raises(RuntimeError):
            s.pair_times_sample(0)
        s.pair_times_enable(cap, EDGES[:5], [1, 2])        # enable twice: another selection and grid, then the real one
        assert s._pair_times_shape() == (NP, 6, G_, 2, 0, 0)
        s.pair_times_enable(cap, EDGES, max_bytes=need)
        before = s.pair_times()
        assert before["samples"] == 0 and not any(before[k].any() for k in "AYXM")
        for it in range(iters):
            s.iteration(it)
            s.pair_times_sample(it)
        first = s.pair_times(reset=True)
        assert first["samples"] == iters and first["A"].any() and first["M"].any()
        zero = s.pair_times()
        assert zero["samples"] == 0 and not any(zero[k].any() for k in "AYXM")
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.pair_times_sample(it)
        assert s._pair_times_shape() == (NP, B, G_, L, iters, cap)
        with pytest.raises(BufferError):
            s.pair_times_sample(99)                        # the row buffer is full
        assert s.lib.gph_engine_pair_times_sample(s.engine, 99) == FULL
        second = s.pair_times()
        its, rows = s.pair_times_rows()
        assert its.tolist() == list(range(2 * iters)) and s._pair_times_shape()[5] == 0
        s2 = G.Sampler(pk, lib=lib)                        # the same chain, sampled over the second half only
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.pair_times_enable(cap, EDGES)
                s2.iteration(it)
                if it >= iters:
                    s2.pair_times_sample(it)
            fresh = s2.pair_times()
            rows2 = s2.pair_times_rows()[1]
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        assert all(second[k].tobytes() == fresh[k].tobytes() for k in "AYXM")
        assert rows[iters:].tobytes() == rows2.tobytes()
        s.initialize()                                     # a new chain starts from zeroed accumulators and no rows
        again = s.pair_times()
        assert again["samples"] == 0 and not again["A"].any() and s._pair_times_shape()[5] == 0
        s.pair_times_enable(4, EDGES, [])                  # no selected locus: zero rows, nothing launched
        n0 = s.host_stats()["launches"]
        c0 = s.class_stats(CLS)["launches"]
        s.pair_times_sample(0)
        s.pair_times_sample(1)
        assert s.host_stats()["launches"] == n0 and s.class_stats(CLS)["launches"] == c0
        e = s.pair_times()
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["A"].shape == (0, NP)
        its, rows = s.pair_times_rows()
        assert its.tolist() == [0, 1] and not rows.any()
        s.pair_times_enable(0, EDGES)                      # disable
        assert s._pair_times_shape() == off
        assert s.lib.gph_engine_pair_times_sample(s.engine, 0) == ESTATE
    finally:
        s.close()


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """records and final state dump with sampling on identical to a run with sampling off, and still the reference's records;
    launches of class 26 = the samples.  Returns the two runs"""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        r = run_chain(lib, name, full, sample=on, trees=False, record=rec, final=final, pack=G.Pack.load(os.path.join(GOLDEN, name + ".gpk")))
        out.append(dict(rec=rec, final=final, stats=r["stats"], launches=r["launches"], samples=r["pt"][full]["samples"] if on else 0))
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]
    return on, off


# ---------------------------------------------------------------- the program and the launcher
def _g(x):
    return "%.10g" % x


def _mean_sd(v):
    s = 0.0
    for x in v:
        s = s + x
    mean = s / float(len(v)) if v else 0.0
    ss = 0.0
    for x in v:
        ss = ss + (x - mean) * (x - mean)
    return mean, math.sqrt(ss / float(len(v) - 1)) if len(v) > 1 else 0.0


def expected_files(ctl_dir, ctl, lib=None, sampler_lib=None, loci=None, pairs=None, edges=None):
    """the text of PREFIX.pair-times.tsv and of PREFIX.pair-times-genome.tsv the program must write and its line on stdout,
    formatted from the output of an equivalent Sampler run (burn-in first, a sample wherever a trace line is written)"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    ed = EDGES if edges is None else edges
    its = [it for it in range(p.numSamplesMcmc) if it % (p.sampleSkip + 1) == 0]
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.pair_times_enable(len(its), ed, loci, pairs)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it in its:
                s.pair_times_sample(it)
        e = s.pair_times()
        got_its, rows = s.pair_times_rows()
    finally:
        s.close()
    S, Q = len(its), len(e["loci"])
    pr = e["pairs"].tolist()
    NP, B = len(pr), len(ed) + 1
    assert e["samples"] == S and got_its.tolist() == its
    label = [f"{p.popName[P]}|{p.popName[Qp]}" for P, Qp in pr]
    m = [leaf_pairs(p, P, Qp) for P, Qp in pr]
    out = ["\t".join(["locus", "name", "samples", "P", "Q", "pairs", "meanAge", "minAge", "pBelow", "fBelow"])]
    for q, g in enumerate(e["loci"].tolist()):
        for k, (P, Qp) in enumerate(pr):
            allc = float(S) * float(m[k])
            out.append("\t".join([str(g), p.locusNames[g], str(S), p.popName[P], p.popName[Qp], str(m[k]), _g(float(e["A"][q, k]) / allc),
                                  _g(float(e["M"][q, k]) / float(S)), _g(float(e["X"][q, k]) / float(S)), _g(float(e["Y"][q, k]) / allc)]))
    out.append(f"# loci {Q} samples {S} pairs {NP} bins {B}")
    gen = ["\t".join(["iter"] + [f"{label[k]}:{b}" for k in range(NP) for b in range(B)] + ["below_" + x for x in label] + ["loci_" + x for x in label])]
    gen += ["%7d" % it + "".join("\t%d" % int(v) for v in rows[k]) for k, it in enumerate(its)]
    gen.append("# edges" + "".join(" %.17g" % x for x in ed))
    best = None
    for k in range(NP):
        allc = float(Q) * float(m[k])
        cdf, sds = [], []
        for b in range(B):
            mean, sd = _mean_sd([float(int(rows[s_, k * B:k * B + b + 1].sum())) / allc for s_ in range(S)])
            cdf.append(_g(mean))
            sds.append(_g(sd))
        gen.append(" ".join(["# cdf", label[k]] + cdf))
        gen.append(" ".join(["# sd", label[k]] + sds))
        bm, bs = _mean_sd([float(int(rows[s_, NP * B + k])) / allc for s_ in range(S)])
        lm, _ = _mean_sd([float(int(rows[s_, NP * B + NP + k])) / float(Q) for s_ in range(S)])
        text = f"{label[k]} mean {_g(bm)} sd {_g(bs)} loci {_g(lm)}"
        gen.append("# below " + text)
        if pr[k][0] != pr[k][1] and (best is None or bm > best[0]):
            best = (bm, text)
    return "\n".join(out) + "\n", "\n".join(gen) + "\n", "PairTimes: " + (best[1] if best else "none")


def check_program(lib_path, lib, tmp_path):
    """both files of a short m3 run against values recomputed from Sampler output; --pair-times-pops, -grid, -loci and -rows; every
    other output of a run with -l -s --ancestry --triplets is the same bytes with and without; chain 0 of --mc3 / --replicates; the
    usage errors"""
    import subprocess
    import gphocs_amd as G
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import program_ctl
    name = "m3"
    ctl = name + ".ctl"
    a, b, c, d, e, m, r = (tmp_path / x for x in ("with", "without", "pops", "all", "rest", "mc3", "rep"))
    for x in (a, b, c, d, e, m, r):
        _copy_case(name, x, program_ctl(name))
    on = ["--pair-times", "out"]
    run = _run(lib_path, a, on + [ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["pair-times-genome.tsv", "pair-times.tsv"]           # no part left behind
    want_loci, want_gen, log = expected_files(str(a), ctl, lib, lib)
    assert got["pair-times.tsv"] == want_loci
    assert got["pair-times-genome.tsv"] == want_gen
    assert log in run.stdout.splitlines()
    edges_line = [ln for ln in got["pair-times-genome.tsv"].splitlines() if ln.startswith("# edges")]
    assert edges_line == ["# edges" + "".join(" %.17g" % x for x in grid(*DEFAULT_GRID))]
    # names in another order, a grid of its own, a selection, a row buffer of 3 rows that fills several times
    pn = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).popName
    _run(lib_path, c, on + ["--pair-times-pops", f"{pn[2]},{pn[0]};{pn[1]},{pn[1]}", "--pair-times-grid", "1e-5,0.05,7", "--pair-times-loci", "1-9:4",
                            "--pair-times-rows", "3", ctl])
    other = read_outputs(c, "out")
    want_loci2, want_gen2, _ = expected_files(str(c), ctl, lib, lib, [1, 5, 9], [(2, 0), (1, 1)], grid(1e-5, 0.05, 7))
    assert other["pair-times.tsv"] == want_loci2 and other["pair-times-genome.tsv"] == want_gen2
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "-s", "cs", "--ancestry", "an", "--triplets", "tw"]
    _run(lib_path, d, on + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix in ("cs", "an", "tw"):
        others = read_outputs(e, prefix)
        assert others and read_outputs(d, prefix) == others
    assert open(d / (name + ".trace")).read() == open(e / (name + ".trace")).read() == open(trace).read()
    # chain 0 of a group of chains is the plain run's chain
    _run(lib_path, m, ["--mc3", "2", "--mc3-swap-every", "-1"] + on + [ctl])
    assert read_outputs(m, "out") == got
    _run(lib_path, r, ["--replicates", "2", "--replicates-out", "rep"] + on + [ctl])
    assert read_outputs(r, "out") == got
    # usage errors: they name the option, nothing written (the trace file is opened after the sequence file is read)
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    L = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).L
    for args, words in ((["--pair-times-loci", "0-3"], ["--pair-times "]), (["--pair-times-pops", f"{pn[0]},{pn[1]}"], ["--pair-times "]),
                        (["--pair-times-rows", "4"], ["--pair-times "]), (["--pair-times-grid", "1e-6,1e-2,34"], ["--pair-times "]),
                        (on + ["--pair-times-pops", f"{pn[0]},nobody"], ["nobody", "--pair-times-pops"]),
                        (on + ["--pair-times-pops", f"{pn[0]}"], ["--pair-times-pops"]),
                        (on + ["--pair-times-pops", f"{pn[0]},{pn[1]},{pn[2]}"], ["--pair-times-pops"]),
                        (on + ["--pair-times-pops", f"{pn[0]},{pn[1]};{pn[1]},{pn[0]}"], ["twice", "--pair-times-pops"]),
                        (on + ["--pair-times-pops", f"{pn[0]},{pn[3]}"], [pn[3], "--pair-times-pops"]),               # an ancestral population
                        (on + ["--pair-times-grid", "0,1e-2,34"], ["LO", "--pair-times-grid"]),
                        (on + ["--pair-times-grid", "-1e-6,1e-2,34"], ["LO", "--pair-times-grid"]),
                        (on + ["--pair-times-grid", "1e-2,1e-2,34"], ["HI", "--pair-times-grid"]),
                        (on + ["--pair-times-grid", "1e-2,1e-3,34"], ["HI", "--pair-times-grid"]),
                        (on + ["--pair-times-grid", "1e-6,1e-2,2"], ["B = 2", "--pair-times-grid"]),
                        (on + ["--pair-times-grid", "1e-6,1e-2,129"], ["B = 129", "--pair-times-grid"]),
                        (on + ["--pair-times-grid", "1e-6,1e-2"], ["--pair-times-grid"]),
                        (on + ["--pair-times-loci", "5,5"], ["locus 5 ", "--pair-times-loci"]), (on + ["--pair-times-loci", f"3,{L}"], [f"locus {L} ", "--pair-times-loci"]),
                        (on + ["--pair-times-rows", "0"], ["usage"])):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and all(w in res.stderr for w in words), (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    two = tmp_path / "two-leaves"                          # a pair without a leaf pair
    os.makedirs(two)
    (two / "t.ctl").write_text(TWO_CTL)
    (two / "t.seq").write_text(TWO_SEQ)
    res = subprocess.run([EXE] + on + ["--pair-times-pops", "A,A", "t.ctl"], cwd=two, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode != 0 and "--pair-times-pops" in res.stderr and "fewer than two samples" in res.stderr, res.stderr[-500:]
    assert sorted(os.listdir(two)) == ["t.ctl", "t.seq"]
    cwd = os.getcwd()
    os.chdir(u)
    try:
        p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        anylib = lib or G.load_library(dims=(p.n, p.K, p.B))
        for kw in (dict(pair_times_loci="0-3"), dict(pair_times_pops="A,B"), dict(pair_times_rows=4), dict(pair_times_grid="1e-6,1e-2,34"),
                   dict(pair_times="out", pair_times_rows=-1), dict(pair_times="out", pair_times_grid="1,1,5")):
            assert G.run_control_file(anylib, ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, joined by gph_pair_times_write, are the one-rank files byte for byte -- per-locus rows
    concatenated, per-sample rows added -- for all loci and for a selection that lies wholly in rank 1's block; the launcher does
    the same; a part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, pair_times="out", pair_times_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["pair-times-genome.tsv", "pair-times.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        NP = len(all_pairs(pk))
        assert [int(ln.split("\t")[0]) for ln in want["pair-times.tsv"].splitlines()[1:-1]] == [g for g in loci for _ in range(NP)]
        run_ranks(lib_path, name, 2, two, pair_times="out", pair_times_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.pair-times.part0", "out.pair-times.part1"]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.pair-times.part{r}", cut)
            text = open(cut / "out.pair-times.part1").read().splitlines(True)
            open(cut / "out.pair-times.part1", "w").write("".join(text[:-1]))
            assert lib.gph_pair_times_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_pair_times_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                          # no part among them
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--pair-times", "out", "--pair-times-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.pair-times-genome.tsv must be
    written: status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.pair-times-genome.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--pair-times", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.pair-times-genome.tsv"] and not os.listdir(d / "out.pair-times-genome.tsv")
