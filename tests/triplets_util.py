"""What tests/test_triplets.py (host-emulation build) and tests/test_triplets_gpu.py (-m gpu, the product libraries) share: a
model of include/gphocs_hip.h's triplet topology weights that does NOT use the kernel's counting formula -- it enumerates every
leaf triple (a, b, c) of a population triple, finds the sister pair by climbing father pointers, and groups the leaf triples by
the sister pair's lca v, which gives w_v directly; the stated summation order is then applied in plain Python floats -- run over
the chain's own gene-tree records, and the check_* functions both files call.  Nothing here calls the library to compute what it
checks, and nothing has a tolerance: W and A are compared as float.hex, rows as integers."""
import ctypes
import math
import os
from itertools import combinations

import pytest

from conftest import GOLDEN
from parity_util import compare_records
from sampler_util import load_pack

CLS = 23                # timing class of k_triplets
FULL, EARG, ESTATE = -5, -1, -4
CHECKPOINTS = (1, 2)
G_CAP = 32              # GPH_TR_MAXG: loci a workgroup takes at most (csrc/gph_triplets.h)
ROW_LDS_SLOTS = 2048    # GPH_TR_ROW_LDS / 4: the slots of a row that a workgroup sums in LDS first


# ---------------------------------------------------------------- the definitions restated, by enumeration
def leaf_pops(pack):
    return [p for p in range(pack.Kc) for _ in range(int(pack.samplesPerPop[p]))]


def all_triples(pack):
    return [t for t in combinations(range(pack.Kc), 3) if all(int(pack.samplesPerPop[p]) >= 1 for p in t)]


def slot_names(triples):
    return [nm for P, Q, R in triples for nm in (f"{P},{Q}|{R}", f"{P},{R}|{Q}", f"{Q},{R}|{P}")]


def lca_table(father, n):
    """lca[a][b] of every pair of leaves, by climbing father pointers from both"""
    paths = []
    for i in range(n):
        path, v = [], i
        while v >= 0:
            path.append(v)
            v = father[v]
            assert len(path) <= len(father)
        paths.append(path)
    out = [[-1] * n for _ in range(n)]
    for a in range(n):
        on_a = set(paths[a])
        for b in range(n):
            out[a][b] = next(v for v in paths[b] if v in on_a)
    return out


def locus_sample(father, age, n, members, triples):
    """one locus at one sample: per slot (cnt, age).  members[p]: the leaves of population p"""
    lca = lca_table(father, n)
    out = []
    for P, Q, R in triples:
        w = [dict(), dict(), dict()]                       # per topology: lca of the sister pair -> leaf triples
        for a in members[P]:
            for b in members[Q]:
                ab = lca[a][b]
                for c in members[R]:
                    ac, bc = lca[a][c], lca[b][c]
                    if ac == bc and ab != ac:
                        t, v = 0, ab                       # a and b are sisters relative to c
                    elif ab == bc and ac != ab:
                        t, v = 1, ac
                    else:
                        assert ab == ac and bc != ab, "a binary tree gives a leaf triple exactly one topology"
                        t, v = 2, bc
                    w[t][v] = w[t].get(v, 0) + 1
        for t in range(3):
            cnt, s = 0, 0.0
            for v in sorted(w[t]):                         # node-index order; nodes with w_v = 0 do not occur
                assert v >= n
                cnt += w[t][v]
                term = age[v] * float(w[t][v])
                s = s + term
            out.append((cnt, s))
    return out


def model_loci(pack, t, S, loci, triples, t0=0):
    """per locus of `loci` over the samples t0 .. t0 + S - 1 of the gene-tree records t: W [slots], A [slots] (python floats);
    and the per-sample rows [S][slots] (python ints).  Both invariants are asserted on the enumeration itself"""
    n, pops = pack.n, leaf_pops(pack)
    members = [[i for i in range(n) if pops[i] == p] for p in range(pack.Kc)]
    slots = 3 * len(triples)
    Ws, As, rows = [], [], [[0] * slots for _ in range(S)]
    rec_loci = t["loci"].tolist()
    for g in loci:
        q = rec_loci.index(g)
        W, A = [0.0] * slots, [0.0] * slots
        for k in range(S):
            rec = t0 + k
            father = [int(f) for f in t["father"][rec, q]]
            age = [float(a) for a in t["age"][rec, q]]
            assert father[int(t["root"][rec, q])] < 0 and sum(f < 0 for f in father) == 1
            for sl, (cnt, a) in enumerate(locus_sample(father, age, n, members, triples)):
                W[sl] = W[sl] + float(cnt)
                A[sl] = A[sl] + a
                rows[k][sl] += cnt
        for j, (P, Q, R) in enumerate(triples):
            assert sum(W[3 * j:3 * j + 3]) == S * len(members[P]) * len(members[Q]) * len(members[R])
        Ws.append(W)
        As.append(A)
    for k in range(S):
        for j, (P, Q, R) in enumerate(triples):
            assert sum(rows[k][3 * j:3 * j + 3]) == len(loci) * len(members[P]) * len(members[Q]) * len(members[R])
    return Ws, As, rows


# ---------------------------------------------------------------- one chain, sampled
def run_chain(lib, name, iters, loci=None, triples=None, checkpoints=(), sample=True, trees=True, record=None, final=None, pack=None):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees and a triplets sample
    after every iteration; Sampler.triplets() is fetched (no reset) after each of `checkpoints` samples and at the end, the rows at
    the end"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.triplets_enable(iters, loci, triples)
        s.initialize()
        hs0 = s.host_stats()
        at = {}
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                s.triplets_sample(it)
                if it + 1 in checkpoints:
                    at[it + 1] = s.triplets()
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        rows = t = None
        if sample:
            at[iters] = s.triplets()
            rows = s.triplets_rows()
            if trees:
                t = s.gene_trees()
        if final:
            s.dump_state(final, True)
        return dict(tr=at, rows=rows, trees=t, pack=pk, stats=(hs0, hs1), launches=launches, oob=s.debug_oob())
    finally:
        s.close()


def check_against_model(e, Ws, As, S, pack, what):
    """W and A as float.hex; the invariant on the device's own words"""
    Q, T = len(e["loci"]), len(e["triples"])
    assert e["samples"] == S and e["W"].shape == e["A"].shape == (Q, T, 3) and len(Ws) == Q
    for q in range(Q):
        g = int(e["loci"][q])
        for arr, want, nm in ((e["W"], Ws, "W"), (e["A"], As, "A")):
            got = [float(v).hex() for v in arr[q].reshape(-1)]
            assert got == [float(v).hex() for v in want[q]], f"{what} S {S}: locus {g} {nm}: {arr[q].reshape(-1).tolist()} != {want[q]}"
        for j, (P, Qp, R) in enumerate(e["triples"].tolist()):
            assert float(e["W"][q, j].sum()) == float(S * int(pack.samplesPerPop[P]) * int(pack.samplesPerPop[Qp]) * int(pack.samplesPerPop[R]))


def check_rows(r, rows, iters, nsel, pack, what):
    its, got = r["rows"]
    assert its.tolist() == list(range(iters)), what
    assert [[int(v) for v in row] for row in got] == rows, f"{what}: the per-sample rows"
    e = r["tr"][iters]
    for row in got:
        for j, (P, Q, R) in enumerate(e["triples"].tolist()):
            assert int(row[3 * j:3 * j + 3].sum()) == nsel * int(pack.samplesPerPop[P]) * int(pack.samplesPerPop[Q]) * int(pack.samplesPerPop[R])


def check_case(lib, name, iters=9, checkpoints=CHECKPOINTS, loci=None, key="cpu", pack=None, triples=None):
    """bit for bit after 1, 2 and the last sample: every fetch against the enumeration over the chain's own records"""
    r = run_chain(lib, name, iters, loci=loci, triples=triples, checkpoints=[c for c in checkpoints if c < iters], pack=pack)
    pk, t = r["pack"], r["trees"]
    sel = list(range(pk.L)) if loci is None else list(loci)
    tri = all_triples(pk) if triples is None else [tuple(sorted(x)) for x in triples]
    assert r["launches"] == iters and r["oob"][0] == 0
    assert t["loci"].tolist() == sel
    for S, e in sorted(r["tr"].items()):
        assert e["loci"].tolist() == sel and e["triples"].tolist() == [list(x) for x in tri] and e["slots"] == slot_names(tri)
        Ws, As, rows = model_loci(pk, t, S, sel, tri)
        check_against_model(e, Ws, As, S, pk, name)
    check_rows(r, rows, iters, len(sel), pk, name)
    minority = sum(1 for W in Ws for j in range(len(tri)) if sorted(W[3 * j:3 * j + 3])[1] > 0.0)
    print(f"{name} [{key}] n {pk.n} Kc {pk.Kc} triples {len(tri)} loci {len(sel)} samples {iters}: (locus, triple) pairs with two "
          f"topologies or more {minority}, last row {rows[-1][:6]}")
    assert minority > 0, "every triple of every locus showed one topology only: the case checks nothing"
    return r


# ---------------------------------------------------------------- the hand-made minimum: one haploid leaf in each of three populations
MIN_CTL = """GENERAL-INFO-START
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
	POP-START
		name		A
		samples		a h
	POP-END
	POP-START
		name		B
		samples		b h
	POP-END
	POP-START
		name		C
		samples		c h
	POP-END
CURRENT-POPS-END
ANCESTRAL-POPS-START
	POP-START
		name			AB
		children		A		B
		tau-initial	0.005
		tau-beta		200.0
		finetune-tau			0.0000008
	POP-END
	POP-START
		name			root
		children		AB		C
		tau-initial	0.006
		tau-beta		150.0
		finetune-tau			0.0000008
	POP-END
ANCESTRAL-POPS-END
"""
MIN_SEQ = "2\n\nl0 3 8\na\tACGTACGT\nb\tACGAACGT\nc\tACTAACGA\n\nl1 3 8\na\tACGTACGT\nb\tTCGTACGT\nc\tACGTACGA\n"


def min_model(tmp_path, lib):
    """a pack of 3 haploid leaves in 3 populations (n = 3, T = 1), two loci; thetas large against the taus, so that the
    topologies vary"""
    import gphocs_amd as G
    d = tmp_path / "min-model"
    os.makedirs(d, exist_ok=True)
    (d / "t.ctl").write_text(MIN_CTL)
    (d / "t.seq").write_text(MIN_SEQ)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        p = G.Pack.from_control("t.ctl", lib=lib)
    finally:
        os.chdir(cwd)
    assert p.n == 3 and p.Kc == 3 and p.samplesPerPop.tolist() == [1, 1, 1] and p.L == 2
    return p


def check_minimum(lib, pack, iters=12):
    """exactly one slot has cnt = 1 at every sample, and A is the sum of the ages of the one non-root internal node"""
    r = run_chain(lib, "minimum", iters, pack=pack, checkpoints=(1, 2))
    t = r["trees"]
    assert r["launches"] == iters and r["oob"][0] == 0
    its, rows = r["rows"]
    assert rows.shape == (iters, 3) and (rows.sum(axis=1) == pack.L).all()
    for S, e in sorted(r["tr"].items()):
        Ws, As, _ = model_loci(pack, t, S, [0, 1], [(0, 1, 2)])
        check_against_model(e, Ws, As, S, pack, "minimum")
        for q in range(pack.L):
            W, A = [0.0] * 3, [0.0] * 3
            for k in range(S):
                father, root = t["father"][k, q].tolist(), int(t["root"][k, q])
                inner = 7 - root                                            # nodes 3 and 4 are the internal ones
                kids = sorted(i for i in range(3) if father[i] == inner)
                assert root in (3, 4) and len(kids) == 2
                sl = {(0, 1): 0, (0, 2): 1, (1, 2): 2}[tuple(kids)]
                W[sl] = W[sl] + 1.0
                A[sl] = A[sl] + float(t["age"][k, q, inner])
            assert e["W"][q, 0].tolist() == W and [float(v).hex() for v in e["A"][q, 0]] == [v.hex() for v in A]
    return r


# ---------------------------------------------------------------- group edges, selections, refusals, lifecycle
def check_group_edges(lib, name="a70", iters=2):
    """70 loci in groups of 32: all of them (32 + 32 + 6), 33 of them (32 + 1), one locus, the last locus of the rank alone"""
    everything = run_chain(lib, name, iters)
    pk, t = everything["pack"], everything["trees"]
    tri = all_triples(pk)
    L = pk.L
    assert L > 2 * G_CAP and L % G_CAP and pk.n >= 8
    Ws, As, rows = model_loci(pk, t, iters, list(range(L)), tri)
    check_against_model(everything["tr"][iters], Ws, As, iters, pk, name)
    check_rows(everything, rows, iters, L, pk, name)
    for sel in (list(range(0, 2 * G_CAP + 2, 2)), [5], [L - 1]):
        r = run_chain(lib, name, iters, loci=sel, trees=False)
        e = r["tr"][iters]
        assert e["loci"].tolist() == sel and r["launches"] == iters
        Ws, As, rows = model_loci(pk, t, iters, sel, tri)
        check_against_model(e, Ws, As, iters, pk, f"{name} selection of {len(sel)}")
        check_rows(r, rows, iters, len(sel), pk, f"{name} selection of {len(sel)}")


def check_triple_lists(lib, name="j1", iters=3):
    """an explicit triple list in non-default order, members unsorted: the matching rows of the default run"""
    everything = run_chain(lib, name, iters, trees=False)
    full = everything["tr"][iters]
    tri = [tuple(x) for x in full["triples"].tolist()]
    given = [(4, 0, 2), (1, 0, 3), (2, 1, 0)]
    r = run_chain(lib, name, iters, triples=given, trees=False)
    e = r["tr"][iters]
    assert e["triples"].tolist() == [sorted(x) for x in given] and e["slots"] == slot_names([tuple(sorted(x)) for x in given])
    for j, x in enumerate(given):
        k = tri.index(tuple(sorted(x)))
        assert e["W"][:, j].tobytes() == full["W"][:, k].tobytes() and e["A"][:, j].tobytes() == full["A"][:, k].tobytes()
        assert r["rows"][1][:, 3 * j:3 * j + 3].tolist() == everything["rows"][1][:, 3 * k:3 * k + 3].tolist()
    assert full["W"].any() and full["A"].any()


def check_refusals(lib, capfd, two_pops, name="j1"):
    """GPH_EARG with a message that names the cause, the sampler left as it was; two current populations"""
    import gphocs_amd as G
    pk = load_pack(name)
    L, Kc = pk.L, pk.Kc
    s = G.Sampler(pk, lib=lib)

    def refused(loci, triples, *words):
        la = None if loci is None else (ctypes.c_int64 * len(loci))(*loci)
        ta = None if triples is None else (ctypes.c_int32 * (3 * len(triples)))(*[x for t in triples for x in t])
        before = s._triplets_shape()
        capfd.readouterr()
        rc = s.lib.gph_engine_triplets_enable(s.engine, 4, la, 0 if loci is None else len(loci), ta, 0 if triples is None else len(triples), 0)
        err = capfd.readouterr().err
        assert rc == EARG and all(w in err for w in words), (loci, triples, err)
        assert s._triplets_shape() == before
        with pytest.raises(ValueError):
            s.triplets_enable(4, loci, triples)

    try:
        for on in (False, True):
            if on:
                s.triplets_enable(4, [1, 2], [(0, 1, 2)])
                assert s._triplets_shape() == (1, 3, 2, 0, 0)
            refused(None, [(0, 1, 1)], "triple 0", "repeats")
            refused(None, [(0, 1, 2), (3, 3, 4)], "triple 1", "repeats")
            refused(None, [(0, 1, Kc)], "triple 0", f"population {Kc}")
            refused(None, [(0, -1, 2)], "triple 0", "population -1")
            refused(None, [(0, 1, 2), (2, 1, 0)], "triple 1", "twice")
            refused([0, L], None, f"locus {L}", "out of range")
            refused([-1], None, "locus -1", "out of range")
            refused([2, 2], None, "locus 2", "twice")
            refused([3, 2], None, "locus 2", "increasing")
        assert s.lib.gph_engine_triplets_enable(s.engine, -1, None, 0, None, 0, 0) == EARG
    finally:
        s.close()
    s = G.Sampler(two_pops, lib=lib)
    try:
        capfd.readouterr()
        assert s.lib.gph_engine_triplets_enable(s.engine, 4, None, 0, None, 0, 0) == EARG
        assert "2 current population" in capfd.readouterr().err
        assert s._triplets_shape() == (0, 0, 0, 0, 0)
        with pytest.raises(ValueError):
            s.triplets_enable(4)
    finally:
        s.close()


def check_lifecycle(lib, G, name="m3", iters=3):
    """reset (W, A and the sample count zeroed), enable twice, a full row buffer, GPH_EFULL one byte short with the feature off,
    GPH_ESTATE, a rank without a selected locus"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    L, T, cap = pk.L, len(all_triples(pk)), 2 * iters
    need = L * T * 48 + ((T * 4 + 15) & ~15) + ((pk.n + pk.Kc + 15) & ~15) + cap * 3 * T * 8
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.triplets()                                   # not enabled
        assert s.lib.gph_engine_triplets_fetch_loci(s.engine, None, 0, 0) == ESTATE
        assert s.lib.gph_engine_triplets_sample(s.engine, 0) == ESTATE
        assert s._triplets_shape() == (0, 0, 0, 0, 0)
        s.triplets_enable(cap)
        assert s._triplets_shape() == (T, 3 * T, L, 0, 0)
        assert s.lib.gph_engine_triplets_sample(s.engine, 0) == ESTATE            # before initialize
        assert s.lib.gph_engine_triplets_enable(s.engine, cap, None, 0, None, 0, need - 1) == FULL
        assert s._triplets_shape() == (0, 0, 0, 0, 0)      # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.triplets_enable(cap, max_bytes=need - 1)
        s.initialize()                                     # the engine is still usable
        with pytest.raises(RuntimeError):
            s.triplets_sample(0)
        s.triplets_enable(cap, [1, 2])                     # enable twice: another selection, then the real one
        assert s._triplets_shape() == (T, 3 * T, 2, 0, 0)
        s.triplets_enable(cap, max_bytes=need)
        before = s.triplets()
        assert before["samples"] == 0 and not before["W"].any() and not before["A"].any()
        for it in range(iters):
            s.iteration(it)
            s.triplets_sample(it)
        first = s.triplets(reset=True)
        assert first["samples"] == iters and first["W"].any() and first["A"].any()
        zero = s.triplets()
        assert zero["samples"] == 0 and not zero["W"].any() and not zero["A"].any()
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.triplets_sample(it)
        assert s._triplets_shape() == (T, 3 * T, L, iters, cap)
        with pytest.raises(BufferError):
            s.triplets_sample(99)                          # the row buffer is full
        second = s.triplets()
        its, rows = s.triplets_rows()
        assert its.tolist() == list(range(2 * iters)) and s._triplets_shape()[4] == 0
        s2 = G.Sampler(pk, lib=lib)                        # the same chain, sampled over the second half only
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.triplets_enable(cap)
                s2.iteration(it)
                if it >= iters:
                    s2.triplets_sample(it)
            fresh = s2.triplets()
            rows2 = s2.triplets_rows()[1]
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        assert second["W"].tobytes() == fresh["W"].tobytes() and second["A"].tobytes() == fresh["A"].tobytes()
        assert rows[iters:].tobytes() == rows2.tobytes()
        s.initialize()                                     # a new chain starts from zeroed accumulators and no rows
        again = s.triplets()
        assert again["samples"] == 0 and not again["W"].any() and s._triplets_shape()[4] == 0
        s.triplets_enable(4, [])                           # no selected locus: zero rows, nothing launched
        n0 = s.host_stats()["launches"]
        c0 = s.class_stats(CLS)["launches"]
        s.triplets_sample(0)
        s.triplets_sample(1)
        assert s.host_stats()["launches"] == n0 and s.class_stats(CLS)["launches"] == c0
        e = s.triplets()
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["W"].shape == (0, T, 3)
        its, rows = s.triplets_rows()
        assert its.tolist() == [0, 1] and not rows.any()
    finally:
        s.close()


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """records and final state dump with sampling on identical to a run with sampling off, and still the reference's records;
    launches of class 23 = the samples.  Returns the two runs"""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        r = run_chain(lib, name, full, sample=on, trees=False, record=rec, final=final, pack=G.Pack.load(os.path.join(GOLDEN, name + ".gpk")))
        out.append(dict(rec=rec, final=final, stats=r["stats"], launches=r["launches"], samples=r["tr"][full]["samples"] if on else 0))
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    return on, off


# ---------------------------------------------------------------- the program and the launcher
def _g(x):
    return "%.10g" % x


def _label(m, t):
    return f"{m[0 if t < 2 else 1]},{m[1 if t == 0 else 2]}|{m[2 if t == 0 else 1 if t == 1 else 0]}"


def expected_files(ctl_dir, ctl, lib=None, sampler_lib=None, loci=None, triples=None):
    """the text of PREFIX.triplets.tsv and the head (header and integer rows) of PREFIX.triplets-genome.tsv the program must
    write, formatted from the output of an equivalent Sampler run (burn-in first, a sample wherever a trace line is written)"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    its = [it for it in range(p.numSamplesMcmc) if it % (p.sampleSkip + 1) == 0]
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.triplets_enable(len(its), loci, triples)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it in its:
                s.triplets_sample(it)
        e = s.triplets()
        got_its, rows = s.triplets_rows()
    finally:
        s.close()
    S = len(its)
    assert e["samples"] == S and got_its.tolist() == its
    out = ["\t".join(["locus", "name", "samples", "P", "Q", "R", "w_PQ|R", "w_PR|Q", "w_QR|P", "age_PQ|R", "age_PR|Q", "age_QR|P", "top"])]
    labels = []
    for j, tri in enumerate(e["triples"].tolist()):
        labels += [_label([p.popName[x] for x in tri], t) for t in range(3)]
    for q, g in enumerate(e["loci"].tolist()):
        for j, tri in enumerate(e["triples"].tolist()):
            m = [p.popName[x] for x in tri]
            allc = float(S) * (float(p.samplesPerPop[tri[0]]) * float(p.samplesPerPop[tri[1]]) * float(p.samplesPerPop[tri[2]]))
            W, A = [float(v) for v in e["W"][q, j]], [float(v) for v in e["A"][q, j]]
            top = max(range(3), key=lambda t: (W[t], -t))
            out.append("\t".join([str(g), p.locusNames[g], str(S)] + m + [_g(w / allc) for w in W] + [_g(a / w if w > 0.0 else 0.0) for a, w in zip(A, W)] +
                                 [_label(m, top)]))
    gen = ["\t".join(["iter"] + labels)] + ["%7d" % it + "".join("\t%d" % int(v) for v in rows[k]) for k, it in enumerate(its)]
    return "\n".join(out) + "\n", gen, [[p.popName[x] for x in tri] for tri in e["triples"].tolist()], len(e["loci"])


def asym_lines(gen_text, names, Q):
    """the "# asym" lines, the last line and the log line, recomputed from the file's own integer rows"""
    lines = gen_text.splitlines()
    rows = [[int(x) for x in ln.split("\t")[1:]] for ln in lines[1:] if not ln.startswith("#")]
    S, T = len(rows), len(names)
    out, best = [], None
    for j, m in enumerate(names):
        tot = [sum(r[3 * j + t] for r in rows) for t in range(3)]
        major = max(range(3), key=lambda t: (tot[t], -t))
        ma, mb = [t for t in range(3) if t != major]
        D = []
        for r in rows:
            a, b = float(r[3 * j + ma]), float(r[3 * j + mb])
            D.append((a - b) / (a + b) if a + b > 0.0 else 0.0)
        mean = 0.0
        for d in D:
            mean = mean + d
        mean = mean / float(S)
        ss = 0.0
        for d in D:
            ss = ss + (d - mean) * (d - mean)
        sd = math.sqrt(ss / float(S - 1)) if S > 1 else 0.0
        allc = float(tot[0]) + float(tot[1]) + float(tot[2])
        text = (f"{m[0]},{m[1]},{m[2]} major {_label(m, major)} minorA {_label(m, ma)} minorB {_label(m, mb)} wMajor {_g(float(tot[major]) / allc)} "
                f"D {_g(mean)} sd {_g(sd)} pPos {_g(sum(d > 0.0 for d in D) / float(S))}")
        out.append("# asym " + text)
        if best is None or abs(mean) > best[0]:
            best = (abs(mean), text)
    return out + [f"# loci {Q} samples {S} triples {T}"], "Triplets: " + best[1]


def check_program(lib_path, lib, tmp_path):
    """both files of a short m3 run against values recomputed from Sampler output (formats, top) and the "# asym" lines
    recomputed from the file's own rows; --triplets-pops, --triplets-loci and --triplets-rows; every other output of a run with
    -l -s --ancestry --clades is the same bytes with and without; chain 0 of --mc3 / --replicates; the usage errors"""
    import subprocess
    import gphocs_amd as G
    from predictive_util import EDGE_CTL, EDGE_SEQ
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import program_ctl
    name = "m3"
    ctl = name + ".ctl"
    a, b, c, d, e, m, r = (tmp_path / x for x in ("with", "without", "pops", "all", "rest", "mc3", "rep"))
    for x in (a, b, c, d, e, m, r):
        _copy_case(name, x, program_ctl(name))
    on = ["--triplets", "out"]
    run = _run(lib_path, a, on + [ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["triplets-genome.tsv", "triplets.tsv"]               # no part left behind
    want_loci, want_gen, names, Q = expected_files(str(a), ctl, lib, lib)
    assert got["triplets.tsv"] == want_loci
    tail, log = asym_lines(got["triplets-genome.tsv"], names, Q)
    assert got["triplets-genome.tsv"].splitlines() == want_gen + tail
    assert log in run.stdout.splitlines()
    # names in another order, a selection, a row buffer of 3 rows that fills several times
    pn = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).popName
    _run(lib_path, c, ["--triplets", "out", "--triplets-pops", f"{pn[2]},{pn[0]},{pn[1]}", "--triplets-loci", "1-9:4", "--triplets-rows", "3", ctl])
    other = read_outputs(c, "out")
    want_loci2, want_gen2, names2, Q2 = expected_files(str(c), ctl, lib, lib, [1, 5, 9], [(2, 0, 1)])
    assert other["triplets.tsv"] == want_loci2 and Q2 == 3
    assert other["triplets-genome.tsv"].splitlines() == want_gen2 + asym_lines(other["triplets-genome.tsv"], names2, Q2)[0]
    assert [ln for ln in got["triplets.tsv"].splitlines() if ln.split("\t")[0] in ("1", "5", "9")] == want_loci2.splitlines()[1:]
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "-s", "cs", "--ancestry", "an", "--clades", "cl"]
    _run(lib_path, d, on + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix in ("cs", "an", "cl"):
        others = read_outputs(e, prefix)
        assert others and read_outputs(d, prefix) == others
    assert open(d / (name + ".trace")).read() == open(e / (name + ".trace")).read() == open(trace).read()
    # chain 0 of a group of chains is the plain run's chain
    _run(lib_path, m, ["--mc3", "2", "--mc3-swap-every", "-1"] + on + [ctl])
    assert read_outputs(m, "out") == got
    _run(lib_path, r, ["--replicates", "2", "--replicates-out", "rep"] + on + [ctl])
    assert read_outputs(r, "out") == got
    # usage errors: they name the option, nothing written
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    L = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).L
    pre = ["--triplets", "out"]
    for args, words in ((["--triplets-loci", "0-3"], ["--triplets "]), (["--triplets-pops", ",".join(pn[:3])], ["--triplets "]), (["--triplets-rows", "4"], ["--triplets "]),
                        (pre + ["--triplets-pops", f"{pn[0]},{pn[1]},nobody"], ["nobody", "--triplets-pops"]),
                        (pre + ["--triplets-pops", f"{pn[0]},{pn[1]}"], ["--triplets-pops"]),
                        (pre + ["--triplets-pops", f"{pn[0]},{pn[1]},{pn[0]}"], ["--triplets-pops"]),
                        (pre + ["--triplets-pops", f"{pn[0]},{pn[1]},{pn[2]};{pn[2]},{pn[1]},{pn[0]}"], ["twice", "--triplets-pops"]),
                        (pre + ["--triplets-pops", f"{pn[0]},{pn[1]},{pn[3]}"], [pn[3], "--triplets-pops"]),       # an ancestral population
                        (pre + ["--triplets-loci", "5,5"], ["locus 5 ", "--triplets-loci"]), (pre + ["--triplets-loci", f"3,{L}"], [f"locus {L} ", "--triplets-loci"]),
                        (pre + ["--triplets-rows", "0"], ["usage"])):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and all(w in res.stderr for w in words), (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    two = tmp_path / "two-pops"                            # a model with two current populations
    os.makedirs(two)
    (two / "e.ctl").write_text(EDGE_CTL)
    (two / "e.seq").write_text(EDGE_SEQ)
    res = subprocess.run([EXE] + pre + ["e.ctl"], cwd=two, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode != 0 and "--triplets" in res.stderr and "2 current population" in res.stderr, res.stderr[-500:]
    assert sorted(os.listdir(two)) == ["e.ctl", "e.seq"]
    cwd = os.getcwd()
    os.chdir(u)
    try:
        p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        anylib = lib or G.load_library(dims=(p.n, p.K, p.B))
        for kw in (dict(triplets_loci="0-3"), dict(triplets_pops="A,B,C"), dict(triplets_rows=4), dict(triplets="out", triplets_rows=-1)):
            assert G.run_control_file(anylib, ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, joined by gph_triplets_write, are the one-rank files -- per-locus rows concatenated,
    per-sample rows added -- for all loci and for a selection that lies wholly in rank 1's block; the launcher does the same; a
    part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, triplets="out", triplets_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["triplets-genome.tsv", "triplets.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        T = len(all_triples(pk))
        assert [int(ln.split("\t")[0]) for ln in want["triplets.tsv"].splitlines()[1:]] == [g for g in loci for _ in range(T)]
        run_ranks(lib_path, name, 2, two, triplets="out", triplets_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.triplets.part0", "out.triplets.part1"]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.triplets.part{r}", cut)
            text = open(cut / "out.triplets.part1").read().splitlines(True)
            open(cut / "out.triplets.part1", "w").write("".join(text[:-1]))
            assert lib.gph_triplets_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_triplets_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                          # no part among them
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--triplets", "out", "--triplets-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.triplets-genome.tsv must be
    written: status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.triplets-genome.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--triplets", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.triplets-genome.tsv"] and not os.listdir(d / "out.triplets-genome.tsv")
