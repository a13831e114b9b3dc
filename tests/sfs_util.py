"""What tests/test_sfs.py (host-emulation build) and tests/test_sfs_gpu.py (-m gpu, the product libraries) share: a model of
include/gphocs_hip.h's site-frequency spectra that does NOT use the kernels' formulas -- the genealogy side collects each node's
leaf SET by climbing father pointers from every leaf, classifies with set operations and sums in the stated order in plain Python
floats; the data side takes predictive_util.columns and Python sets of bases per population -- run over the chain's own gene-tree
records and locus rates (obtained as mutations_util obtains them), and the check_* functions both files call.  Nothing here calls
the library to compute what it checks: every double is compared as float.hex, every integer exactly; the one tolerance (the link to
--pair-times) is derived where it is used."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
from mutations_util import phased_pack
from parity_util import compare_records
from predictive_util import columns, leaf_pops, phase_groups
from sampler_util import load_pack

CLS, CLS_DATA = 27, 28  # timing classes of k_sfs_tree (with its fold) and k_sfs_data
FULL, EARG, ESTATE = -5, -1, -4
GT_O_DATALNL = 3        # gph_engine_gene_trees_shape: the offset of dataLnL in a record; FS_MUTRATE lies 4 doubles behind it
CHECKPOINTS = (1, 2)
CLASSES = ("privP", "privQ", "shared", "fixed")
G_CAP = 32              # GPH_TR_MAXG: loci a workgroup takes at most


# ---------------------------------------------------------------- the definitions restated, with sets
def pop_members(pack):
    pops = leaf_pops(pack)
    return [frozenset(i for i in range(pack.n) if pops[i] == p) for p in range(pack.Kc)]


def all_pairs(pack):
    m = pop_members(pack)
    return [(P, Q) for P in range(pack.Kc) for Q in range(P + 1, pack.Kc) if m[P] and m[Q]]


def slot_table(pack, pairs=None):
    """(slots, groups): a slot is (group, kind, P, Q, k), kind "sfs" or one of CLASSES; a group ("pop", p) or ("pair", P, Q)"""
    m = pop_members(pack)
    pr = all_pairs(pack) if pairs is None else [tuple(sorted(x)) for x in pairs]
    slots, groups = [], []
    for p in range(pack.Kc):
        if len(m[p]) >= 2:
            groups.append(("pop", p))
            slots += [(len(groups) - 1, "sfs", p, p, k) for k in range(1, len(m[p]) // 2 + 1)]
    for P, Q in pr:
        groups.append(("pair", P, Q))
        slots += [(len(groups) - 1, c, P, Q, 0) for c in CLASSES]
    return slots, groups


def slot_names(slots, pop=str):
    return [f"sfs_{pop(P)}:{k}" if kind == "sfs" else f"{kind}_{pop(P)}|{pop(Q)}" for _, kind, P, Q, k in slots]


def group_names(groups, pop=str):
    return [pop(g[1]) if g[0] == "pop" else f"{pop(g[1])}|{pop(g[2])}" for g in groups]


def leaf_sets(father, n):
    """the leaves under every node, by climbing from every leaf"""
    under = [set() for _ in father]
    for i in range(n):
        v, steps = i, 0
        while v >= 0:
            under[v].add(i)
            v = father[v]
            steps += 1
            assert steps <= len(father)
    return under


def node_classes(U, mP, mQ):
    """the classes of a pair that a node with the leaves U under it belongs to"""
    A, B = U & mP, U & mQ
    a_in, b_in = bool(A) and A != mP, bool(B) and B != mQ
    out = []
    if a_in and (not B or B == mQ):
        out.append("privP")
    if b_in and (not A or A == mP):
        out.append("privQ")
    if a_in and b_in:
        out.append("shared")
    if (A == mP and not B) or (not A and B == mQ):
        out.append("fixed")
    return out


def in_slot(slot, U, members):
    _, kind, P, Q, k = slot
    if kind == "sfs":
        A = U & members[P]
        return bool(A) and A != members[P] and min(len(A), len(members[P] - A)) == k
    return kind in node_classes(U, members[P], members[Q])


def locus_tree(father, age, n, members, slots, rate):
    """one locus at one sample: per slot (x, e)"""
    under = leaf_sets(father, n)
    out = []
    for slot in slots:
        x = 0.0
        for v in range(len(father)):                    # node-index order; the root has no branch
            if father[v] >= 0 and in_slot(slot, under[v], members):
                x = x + (age[father[v]] - age[v])
        out.append((x, rate * x))
    return out


def locus_data(codes, counts, members, slots, groups):
    """the data side of one locus from its columns (codes [U][n], counts [U]): obs [NS], use [NG], sites"""
    at = {(kind, P, Q, k): s for s, (_, kind, P, Q, k) in enumerate(slots)}
    obs, use, sites = [0] * len(slots), [0] * len(groups), 0
    for col, c in zip(codes.tolist(), [int(x) for x in counts]):
        sites += c
        for g, grp in enumerate(groups):
            if grp[0] == "pop":
                p = grp[1]
                shown = [col[i] for i in sorted(members[p])]
                if any(b >= 4 for b in shown) or len(set(shown)) > 2:
                    continue
                use[g] += c
                if len(set(shown)) == 2:
                    obs[at[("sfs", p, p, min(shown.count(b) for b in set(shown)))]] += c
            else:
                _, P, Q = grp
                bp, bq = [col[i] for i in sorted(members[P])], [col[i] for i in sorted(members[Q])]
                if any(b >= 4 for b in bp + bq) or len(set(bp) | set(bq)) > 2:
                    continue
                use[g] += c
                pp, pq = len(set(bp)) == 2, len(set(bq)) == 2
                kind = "shared" if pp and pq else "privP" if pp else "privQ" if pq else "fixed" if set(bp) != set(bq) else None
                if kind:
                    obs[at[(kind, P, Q, 0)]] += c
    return obs, use, sites


def model_data(pack, loci, slots, groups):
    m = pop_members(pack)
    return [locus_data(*columns(pack, g), m, slots, groups) for g in loci]


def model_samples(pack, t, rates, loci, slots):
    """per sample and locus of `loci`: [(x, e) per slot] over the chain's own records and locus rates"""
    m, n = pop_members(pack), pack.n
    rec_loci = t["loci"].tolist()
    out = []
    for k in range(len(t["iters"])):
        per = []
        for g in loci:
            q = rec_loci.index(g)
            father = [int(f) for f in t["father"][k, q]]
            assert father[int(t["root"][k, q])] < 0 and sum(f < 0 for f in father) == 1
            per.append(locus_tree(father, [float(a) for a in t["age"][k, q]], n, m, slots, float(rates[k, q])))
        out.append(per)
    return out


def model_acc(samples, S, NS):
    """E after S samples: one plain add a sample"""
    E = [[0.0] * NS for _ in samples[0]]
    for k in range(S):
        for q, v in enumerate(samples[k]):
            for s in range(NS):
                E[q][s] = E[q][s] + v[s][1]
    return E


def model_row(per, data, slots, G):
    """a sample's row: (double)use e of the loci of a workgroup in selection order from 0.0, the workgroups in order from 0.0"""
    NS = len(slots)
    row = [0.0] * NS
    for q0 in range(0, len(per), G):
        part = [0.0] * NS
        for q in range(q0, min(q0 + G, len(per))):
            for s in range(NS):
                part[s] = part[s] + float(data[q][1][slots[s][0]]) * per[q][s][1]
        for s in range(NS):
            row[s] = row[s] + part[s]
    return row


def hexes(xs):
    return [float(x).hex() for x in xs]


# ---------------------------------------------------------------- one chain, sampled
def run_chain(lib, name, iters, loci=None, pairs=None, checkpoints=(), sample=True, trees=True, record=None, final=None, pack=None):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees and an sfs sample after
    every iteration; Sampler.sfs() is fetched (no reset) after each of `checkpoints` samples and at the end, the rows and the data
    side at the end"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.sfs_enable(iters, loci, pairs)
        group = s._sfs_shape()[2]
        data_launches = s.class_stats(CLS_DATA)["launches"]
        s.initialize()
        hs0 = s.host_stats()
        at = {}
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                s.sfs_sample(it)
                if it + 1 in checkpoints:
                    at[it + 1] = s.sfs()
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        rows = t = rates = obs = None
        if sample:
            at[iters] = s.sfs()
            rows = s.sfs_rows()
            obs = s.sfs_observed()
            if trees:
                off = s._gene_trees_shape()[3][GT_O_DATALNL]
                t = s.gene_trees(raw=True)
                rec = t["records"]
                rates = np.ascontiguousarray(rec[:, :, off + 32:off + 40]).view(np.float64)[:, :, 0] if rec.size else np.zeros(rec.shape[:2])
        if final:
            s.dump_state(final, True)
        return dict(sf=at, rows=rows, obs=obs, trees=t, rates=rates, pack=pk, stats=(hs0, hs1), launches=launches, data_launches=data_launches,
                    oob=s.debug_oob(), group=group)
    finally:
        s.close()


def check_tables(e, slots, groups):
    """the device's slot and group tables are the model's"""
    kinds = ("sfs",) + CLASSES
    assert e["columns"] == slot_names(slots) and e["groups"] == group_names(groups)
    assert e["slots"].tolist() == [[g, kinds.index(kind), P, Q, k] for g, kind, P, Q, k in slots]


def check_observed(o, data, sel, what):
    """obs, use, sites per locus and their totals, as integers; the invariants on the device's own words"""
    Q = len(sel)
    assert o["loci"].tolist() == sel and o["obs"].shape[0] == o["use"].shape[0] == Q
    for q in range(Q):
        obs, use, sites = data[q]
        assert o["obs"][q].tolist() == obs and o["use"][q].tolist() == use and int(o["sites"][q]) == sites, f"{what}: the data side of locus {sel[q]}"
    assert o["obs_total"].tolist() == [sum(d[0][s] for d in data) for s in range(o["obs"].shape[1])]
    assert o["use_total"].tolist() == [sum(d[1][g] for d in data) for g in range(o["use"].shape[1])]
    assert o["sites_total"] == sum(d[2] for d in data)


def check_data_invariants(o, slots, groups):
    """sum_k obs[sfs_p:k] <= use_p <= sites, and the four classes of a pair <= use_PQ <= sites, on the device's words"""
    for q in range(len(o["loci"])):
        for g in range(len(groups)):
            inside = sum(int(o["obs"][q, s]) for s, sl in enumerate(slots) if sl[0] == g)
            assert inside <= int(o["use"][q, g]) <= int(o["sites"][q])


def check_case(lib, name, iters=9, checkpoints=CHECKPOINTS, loci=None, key=None, pack=None, pairs=None, min_live=None):
    """bit for bit after 1, 2 and the last sample: every fetch and every row against the set model over the chain's own records"""
    key = key or ("gpu" if lib is None else "given library")
    r = run_chain(lib, name, iters, loci=loci, pairs=pairs, checkpoints=[c for c in checkpoints if c < iters], pack=pack)
    pk, t = r["pack"], r["trees"]
    sel = list(range(pk.L)) if loci is None else list(loci)
    slots, groups = slot_table(pk, pairs)
    NS = len(slots)
    assert r["launches"] == iters and r["data_launches"] == 1 and r["oob"][0] == 0 and 1 <= r["group"] <= G_CAP
    assert t["loci"].tolist() == sel
    data = model_data(pk, sel, slots, groups)
    check_observed(r["obs"], data, sel, name)
    check_data_invariants(r["obs"], slots, groups)
    samples = model_samples(pk, t, r["rates"], sel, slots)
    for S, e in sorted(r["sf"].items()):
        check_tables(e, slots, groups)
        assert e["loci"].tolist() == sel and e["samples"] == S and e["group"] == r["group"] and e["E"].shape == (len(sel), NS)
        want = model_acc(samples, S, NS)
        for q in range(len(sel)):
            assert hexes(e["E"][q]) == hexes(want[q]), f"{name} S {S}: locus {sel[q]}: {e['E'][q].tolist()} != {want[q]}"
    its, rows = r["rows"]
    assert its.tolist() == list(range(iters)) and rows.shape == (iters, NS)
    for k in range(iters):
        assert hexes(rows[k]) == hexes(model_row(samples[k], data, slots, r["group"])), f"{name}: row {k}"
    live = sum(1 for s in range(NS) if any(v[s][0] > 0.0 for per in samples for v in per))
    print(f"{name} [{key}] n {pk.n} Kc {pk.Kc} slots {NS} groups {len(groups)} loci {len(sel)} samples {iters} G {r['group']}: slots with a branch {live}, "
          f"observed {int(r['obs']['obs_total'].sum())} of {r['obs']['sites_total']} sites")
    assert live >= (NS // 2 + 1 if min_live is None else min_live), "most slots never had a branch: the case checks nothing"
    r["samples"], r["data"], r["slots"], r["groups"] = samples, data, slots, groups
    return r


# ---------------------------------------------------------------- invariants of the model and of the device
def check_model_invariants(r):
    """per pair and node at most one class holds, and the four classes plus "none" add up to the tree's length (exactly, in
    rationals over the floats the model added); per population the bins and "none" add up to it too"""
    pk, t = r["pack"], r["trees"]
    m, n = pop_members(pk), pk.n
    seen = set()
    for k in range(len(t["iters"])):
        for q in range(len(t["loci"])):
            father = [int(f) for f in t["father"][k, q]]
            age = [float(a) for a in t["age"][k, q]]
            under = leaf_sets(father, n)
            length = sum(Fraction(age[father[v]] - age[v]) for v in range(len(father)) if father[v] >= 0)
            for grp in r["groups"]:
                parts = {}
                for v in range(len(father)):
                    if father[v] < 0:
                        continue
                    if grp[0] == "pair":
                        cls = node_classes(under[v], m[grp[1]], m[grp[2]])
                    else:
                        cls = [s[4] for s in r["slots"] if s[1] == "sfs" and s[2] == grp[1] and in_slot(s, under[v], m)]
                    assert len(cls) <= 1, f"sample {k} locus {q} node {v}: {cls}"
                    key = cls[0] if cls else None
                    parts[key] = parts.get(key, Fraction(0)) + Fraction(age[father[v]] - age[v])
                    seen.add(key)
                assert sum(parts.values()) == length
    return seen


def check_predictive_link(lib, pack, seed=5):
    """without N and without a third base: sum_k k (n_p - k) obs[sfs_p:k] = --predictive's observed diff_p|p exactly, and
    n_P n_Q obs[fixed] is part of diff_P|Q -- both from the device"""
    import gphocs_amd as G
    assert not (pack.leafcodes >= 4).any()
    s = G.Sampler(pack, lib=lib)
    try:
        s.sfs_enable(2)
        s.predictive_enable(seed, 2)
        o, e, pd = s.sfs_observed(), s.sfs(), s.predictive()
    finally:
        s.close()
    m = pop_members(pack)
    slots = e["slots"].tolist()
    assert (o["use"] == o["sites"][:, None]).all(), "a column with a third base"
    checked = 0
    for q in range(pack.L):
        for p in range(pack.Kc):
            mine = [(s, sl[4]) for s, sl in enumerate(slots) if sl[1] == 0 and sl[2] == p]
            if mine:
                n_p = len(m[p])
                assert sum(k * (n_p - k) * int(o["obs"][q, s]) for s, k in mine) == int(pd["acc"][q, pd["stats"].index(f"diff_{p}|{p}"), 0])
                checked += 1
        for s, sl in enumerate(slots):
            if sl[1] == 4:
                assert len(m[sl[2]]) * len(m[sl[3]]) * int(o["obs"][q, s]) <= int(pd["acc"][q, pd["stats"].index(f"diff_{sl[2]}|{sl[3]}"), 0])
                checked += 1
    assert checked and o["obs"].any()
    return checked


def check_pair_times_link(lib, name="m3"):
    """no ancient sample: sum_k k (n_p - k) x[sfs_p:k] = 2 a of --pair-times' slot (p, p) of the same sample -- both count, for
    every pair of leaves of p, the path between them.  After ONE sample E = rate x and A = a.  Both sides are sums of at most N
    non-negative fp64 terms (the products by the small integers k (n_p - k) and the rate are one rounding each, inside the same
    bound): relative tolerance 4 N 2^-52"""
    import gphocs_amd as G
    pk = load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        s.sfs_enable(1, pairs=[])
        s.pair_times_enable(1, [1e-4], pairs=[(p, p) for p in range(pk.Kc) if int(pk.samplesPerPop[p]) >= 2])
        s.enable_gene_trees(1)
        s.initialize()
        s.iteration(0)
        s.sfs_sample(0)
        s.pair_times_sample(0)
        s.sample_gene_trees(0)
        e, pt, t = s.sfs(), s.pair_times(), s.gene_trees(raw=True)
        off = s._gene_trees_shape()[3][GT_O_DATALNL]
    finally:
        s.close()
    assert not t["age"][:, :, :pk.n].any(), "an ancient sample"
    rates = np.ascontiguousarray(t["records"][:, :, off + 32:off + 40]).view(np.float64)[:, :, 0]
    tol = 4 * (2 * pk.n - 1) * 2.0 ** -52
    slots, worst = e["slots"].tolist(), 0.0
    for q in range(pk.L):
        for j, (p, _) in enumerate(pt["pairs"].tolist()):
            n_p = int(pk.samplesPerPop[p])
            lhs = sum(k * (n_p - k) * float(e["E"][q, s]) for s, (_, kind, P, _, k) in enumerate(slots) if kind == 0 and P == p)
            rhs = 2.0 * float(pt["A"][q, j]) * float(rates[0, q])
            assert rhs > 0.0
            worst = max(worst, abs(lhs - rhs) / rhs)
            assert abs(lhs - rhs) <= tol * rhs, f"locus {q} population {p}: {lhs!r} != {rhs!r}"
    print(f"{name}: sum k (n - k) x = 2 a within {worst:.3g} (bound {tol:.3g})")


# ---------------------------------------------------------------- the hand-made packs
def _ctl(current, ancestral):
    return """GENERAL-INFO-START
	seq-file            t.seq
	trace-file          t.trace
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
""" + current + "CURRENT-POPS-END\nANCESTRAL-POPS-START\n" + ancestral + "ANCESTRAL-POPS-END\n"


def _pop(name, samples):
    return f"\tPOP-START\n\t\tname\t\t{name}\n\t\tsamples\t\t{' '.join(s + ' h' for s in samples)}\n\tPOP-END\n"


def _anc(name, a, b, tau):
    return f"\tPOP-START\n\t\tname\t\t\t{name}\n\t\tchildren\t\t{a}\t\t{b}\n\t\ttau-initial\t{tau}\n\t\ttau-beta\t\t200.0\n\t\tfinetune-tau\t\t\t0.0000008\n\tPOP-END\n"


SMALL_SAMPLES = (["a0"], ["b0", "b1"], ["c0", "c1", "c2"], ["d0", "d1", "d2", "d3"])
SMALL_CTL = _ctl("".join(_pop(nm, s) for nm, s in zip("ABCD", SMALL_SAMPLES)),
                 _anc("AB", "A", "B", 0.002) + _anc("CD", "C", "D", 0.003) + _anc("root", "AB", "CD", 0.005))
ONES_CTL = _ctl(_pop("A", ["a0"]) + _pop("B", ["b0"]), _anc("root", "A", "B", 0.005))


def small_model(tmp_path, lib, which="small"):
    """`small`: populations of 1, 2, 3 and 4 haploid leaves, ((A, B), (C, D)); `ones`: two populations of one leaf each"""
    import gphocs_amd as G
    samples = SMALL_SAMPLES if which == "small" else (["a0"], ["b0"])
    d = tmp_path / f"sfs-{which}"
    os.makedirs(d, exist_ok=True)
    (d / "t.ctl").write_text(SMALL_CTL if which == "small" else ONES_CTL)
    (d / "t.seq").write_text("1\n\nl0 %d 8\n" % sum(len(s) for s in samples) + "".join(f"{nm}\tACGTACGT\n" for s in samples for nm in s))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        p = G.Pack.from_control("t.ctl", lib=lib)
    finally:
        os.chdir(cwd)
    assert p.samplesPerPop.tolist()[:p.Kc] == [len(s) for s in samples] and p.B == 0
    return p


def _random_codes(rng, n, missing=0.05):
    return "".join("N" if rng.random() < missing else "TCAG"[int(rng.integers(4)) if rng.random() < 0.3 else 0] for _ in range(n))


# columns of the small pack, leaves A | B B | C C C | D D D D, with what each is there for
SMALL_COLUMNS = [
    (["NNNNNNNNNN"], 3),        # all N: sites only
    (["ANCAAAAACC"], 2),        # an N in B only: B and its pairs unusable, C, D and C|D counted
    (["AAAACGAAAA"], 4),        # three bases in C: C and its pairs unusable
    (["AACAGGAAAA"], 6),        # three bases across B u C, two in each: B and C usable, B|C not
    (["AAAAACAACC"], 5),        # C: one carrier (bin 1); D: two of four, the self-folded bin 2, once
    (["CAAACCACCC"], 1),        # C: two carriers fold to bin 1; D: three fold to bin 1; A against B fixed
    (["ACCCCCCCCC"], 7),        # A fixed against everybody
    (["GGGGGGGGGG"], 11),       # monomorphic
    (["AACACCAAAA"], 2),        # B and C polymorphic: shared in B|C, privP / privQ against the others
]


def small_loci(n=10, lanes=256, seed=3):
    """a handful of loci for the small pack: the hand-written columns; a multi-phase group whose later rows own no site; a locus
    with more rows than a workgroup has lanes; loci of random columns; a locus of count-0 columns"""
    rng = np.random.default_rng(seed)
    rand = lambda k, miss=0.05: [([_random_codes(rng, n, miss)], int(rng.integers(1, 9))) for _ in range(k)]     # noqa: E731
    phased = [(["AACAACAACC", "ACAACAACAC", "ACAACACCAA"], 5), (["AAAAAAAAAA"], 2), (["CACACAACGT", "CCAACAAGCT"], 3)]
    return [SMALL_COLUMNS, phased + rand(4), rand(lanes + 44), rand(20, 0.0), rand(7, 0.3), [(["ACACACACAC"], 0), (["AACCAACCAA"], 4)]]


def two_base_loci(n=10, seed=9):
    """loci without N and without a third base in any column"""
    rng = np.random.default_rng(seed)
    col = lambda: "".join("AC"[int(rng.random() < 0.3)] for _ in range(n))      # noqa: E731
    return [[([col()], int(rng.integers(1, 6))) for _ in range(k)] for k in (30, 9, 1)]


def check_small_shapes(lib, base, iters=3):
    pk = phased_pack(base, small_loci())
    assert pk.n == 10 and int(np.diff(pk.pattern_offsets)[2]) == 300 > 256
    r = check_case(lib, "small shapes", iters=iters, checkpoints=(1, 2), pack=pk)
    slots, groups, o = r["slots"], r["groups"], r["obs"]
    names = slot_names(slots)
    assert names[:4] == ["sfs_1:1", "sfs_2:1", "sfs_3:1", "sfs_3:2"] and len(slots) == 4 + 4 * 6 and len(groups) == 3 + 6
    want = {"sfs_1:1": 6 + 2, "sfs_2:1": 5 + 1 + 6 + 2, "sfs_3:1": 1, "sfs_3:2": 2 + 5, "fixed_0|1": 1 + 7, "privP_0|1": 0, "privQ_0|1": 6 + 2, "shared_0|1": 0,
            "shared_1|2": 2, "privQ_2|3": 2, "privP_2|3": 6 + 2, "shared_2|3": 5 + 1, "fixed_0|3": 7, "fixed_0|2": 7}
    for nm, v in want.items():
        assert int(o["obs"][0, names.index(nm)]) == v, nm
    gn = group_names(groups)
    assert int(o["sites"][0]) == 41
    assert [int(o["use"][0, gn.index(g)]) for g in ("1", "2", "3", "0|1", "1|2", "2|3")] == [36, 34, 38, 36, 26, 34]
    # against the one-leaf population only `fixed` (and privQ, the other side's own polymorphism) ever counts
    for P, Q in ((0, 1), (0, 2), (0, 3)):
        assert not o["obs"][:, names.index(f"privP_{P}|{Q}")].any() and not o["obs"][:, names.index(f"shared_{P}|{Q}")].any()
        for S, e in r["sf"].items():
            assert not e["E"][:, names.index(f"privP_{P}|{Q}")].any() and not e["E"][:, names.index(f"shared_{P}|{Q}")].any()
            assert (e["E"][:, names.index(f"fixed_{P}|{Q}")] > 0.0).all()
    # the later rows of a group of phases own no site: locus 1's sites are those of its columns
    assert int(o["sites"][1]) == 5 + 2 + 3 + sum(c for _, c in small_loci()[1][3:]) and int(o["sites"][5]) == 4
    assert check_model_invariants(r) >= {"privP", "privQ", "shared", "fixed", None, 1, 2}
    return r


def check_one_leaf_populations(lib, pack, iters=3):
    """two populations of one leaf: no bins, one pair; both branches are `fixed`: x = 2 age[root] at every sample"""
    pk = phased_pack(pack, [[(["AC"], 3), (["AA"], 4), (["NA"], 1)], [(["GT"], 2)]])
    r = check_case(lib, "two leaves", iters=iters, checkpoints=(1,), pack=pk, min_live=1)
    assert slot_names(r["slots"]) == ["privP_0|1", "privQ_0|1", "shared_0|1", "fixed_0|1"]
    assert r["obs"]["obs"].tolist() == [[0, 0, 0, 3], [0, 0, 0, 2]] and r["obs"]["use"].tolist() == [[7], [2]] and r["obs"]["sites"].tolist() == [8, 2]
    for per in r["samples"]:
        for q, v in enumerate(per):
            assert [x for x, _ in v[:3]] == [0.0, 0.0, 0.0] and v[3][0] > 0.0
    return r


def check_phase_rows(lib, name):
    """both haplotypes of a diploid lie in one population: the counts of every multi-phase group do not depend on the phase row
    read -- the model over the group's LAST row equals the device's words (which read its first)"""
    import copy
    import gphocs_amd as G
    pk = load_pack(name)
    found = phase_groups(pk)
    assert found, f"{name} has no group of more than one phase"
    slots, groups = slot_table(pk)
    m = pop_members(pk)
    for g, r, k in found:
        rows = pk.leafcodes[r:r + k].astype(np.int64)
        want = locus_data(rows[:1], [1], m, slots, groups)
        for j in range(1, k):
            assert locus_data(rows[j:j + 1], [1], m, slots, groups) == want, f"{name} locus {g} row {r + j}"
    last = copy.deepcopy(pk)
    for g, r, k in found:
        last.leafcodes[r] = pk.leafcodes[r + k - 1]
    s = G.Sampler(pk, lib=lib)
    try:
        s.sfs_enable(1)
        o = s.sfs_observed()
    finally:
        s.close()
    check_observed(o, model_data(last, list(range(pk.L)), slots, groups), list(range(pk.L)), f"{name}, last phase rows")
    print(f"{name}: {len(found)} groups, up to {max(k for _, _, k in found)} phases")


# ---------------------------------------------------------------- group edges, pairs, refusals, lifecycle
def check_group_edges(lib, name="a70", iters=2):
    """G - 1, G, G + 1 and 2 G + 1 selected loci for the kernel's own G (the last across an edge of the fold's chunks), and the
    last locus of the rank alone"""
    everything = check_case(lib, name, iters=iters, checkpoints=(1,))
    pk, G_, samples, data, slots = everything["pack"], everything["group"], everything["samples"], everything["data"], everything["slots"]
    L, NS = pk.L, len(slots)
    assert 1 < G_ and 2 * G_ + 1 <= L and L % G_
    sels = (list(range(1, G_)), list(range(L - G_, L)), list(range(0, G_ + 1)), list(range(2, 2 * G_ + 3)), [L - 1])
    assert [len(x) for x in sels] == [G_ - 1, G_, G_ + 1, 2 * G_ + 1, 1]
    for sel in sels:
        r = run_chain(lib, name, iters, loci=sel, trees=False)
        e = r["sf"][iters]
        assert e["loci"].tolist() == sel and r["launches"] == iters and r["group"] == G_
        sub, dsub = [[per[g] for g in sel] for per in samples], [data[g] for g in sel]
        want = model_acc(sub, iters, NS)
        for q in range(len(sel)):
            assert hexes(e["E"][q]) == hexes(want[q])
        check_observed(r["obs"], dsub, sel, f"{name} selection of {len(sel)}")
        for k in range(iters):
            assert hexes(r["rows"][1][k]) == hexes(model_row(sub[k], dsub, slots, G_)), f"{name} selection of {len(sel)}: row {k}"


def check_pair_lists(lib, name="j1", iters=3):
    """pairs given as (Q, P) and in another order than the default: the default run's slots permuted; `none`: the bins alone"""
    everything = run_chain(lib, name, iters, trees=False)
    full, fobs = everything["sf"][iters], everything["obs"]
    pk = everything["pack"]
    for given in ([(4, 0), (2, 1), (3, 1)], []):
        r = run_chain(lib, name, iters, pairs=given, trees=False)
        e, o = r["sf"][iters], r["obs"]
        slots, groups = slot_table(pk, given)
        check_tables(e, slots, groups)
        assert len(groups) == sum(int(x) >= 2 for x in pk.samplesPerPop[:pk.Kc]) + len(given)
        for j, nm in enumerate(e["columns"]):
            k = full["columns"].index(nm)
            assert e["E"][:, j].tobytes() == full["E"][:, k].tobytes() and o["obs"][:, j].tolist() == fobs["obs"][:, k].tolist()
            gj, gk = int(e["slots"][j, 0]), int(full["slots"][k, 0])
            assert o["use"][:, gj].tolist() == fobs["use"][:, gk].tolist()
            assert r["rows"][1][:, j].tobytes() == everything["rows"][1][:, k].tobytes()
    assert full["E"].any() and fobs["obs"].any()


def check_refusals(lib, capfd, ones_pack, name="j1"):
    """GPH_EARG with a message that names the cause, the sampler left as it was"""
    import gphocs_amd as G
    pk = load_pack(name)
    L, Kc = pk.L, pk.Kc
    s = G.Sampler(pk, lib=lib)

    def refused(loci, pairs, *words):
        la = None if loci is None else (ctypes.c_int64 * max(len(loci), 1))(*loci)
        pa = None if pairs is None else (ctypes.c_int32 * max(2 * len(pairs), 1))(*[x for p in pairs for x in p])
        before = (s._sfs_shape(), s.sfs_columns())
        capfd.readouterr()
        rc = s.lib.gph_engine_sfs_enable(s.engine, 4, la, 0 if loci is None else len(loci), pa, 0 if pairs is None else len(pairs), 0)
        err = capfd.readouterr().err
        assert rc == EARG and "sfs" in err and all(w in err for w in words), (loci, pairs, err)
        assert (s._sfs_shape(), s.sfs_columns()) == before
        with pytest.raises(ValueError):
            s.sfs_enable(4, loci, pairs)

    try:
        for on in (False, True):
            if on:
                s.sfs_enable(4, [1, 2], [(0, 1)])
                assert s._sfs_shape()[:2] + s._sfs_shape()[3:] == (Kc + 4, Kc + 1, 2, 0, 0)
            refused(None, [(0, Kc)], "pair 0", f"population {Kc}")
            refused(None, [(0, 1), (-1, 2)], "pair 1", "population -1")
            refused(None, [(0, 1), (1, 0)], "pair 1", "twice")
            refused(None, [(2, 2)], "pair 0", "population 2 twice")
            refused([0, L], None, f"locus {L}", "out of range")
            refused([-1], None, "locus -1", "out of range")
            refused([2, 2], None, "locus 2", "twice")
            refused([3, 2], None, "locus 2", "increasing")
        assert s.lib.gph_engine_sfs_enable(s.engine, -1, None, 0, None, 0, 0) == EARG
    finally:
        s.close()
    s = G.Sampler(ones_pack, lib=lib)                      # two populations of one leaf each: without the pair there is no slot
    try:
        capfd.readouterr()
        assert s.lib.gph_engine_sfs_enable(s.engine, 4, None, 0, (ctypes.c_int32 * 2)(0, 0), 0, 0) == EARG
        assert "no population has two samples and no pair is taken" in capfd.readouterr().err
        assert s._sfs_shape() == (0, 0, 0, 0, 0, 0)
        with pytest.raises(ValueError):
            s.sfs_enable(4, pairs=[])
        s.sfs_enable(4)
        assert s.sfs_columns() == ["privP_0|1", "privQ_0|1", "shared_0|1", "fixed_0|1"]
    finally:
        s.close()


def check_refused_sites(lib, base, capfd):
    """a selected locus whose sites reach 2^32 is refused by name, nothing enabled; the other locus alone is taken"""
    import gphocs_amd as G
    half = 1 << 31
    pk = phased_pack(base, [[(["AC"], 5)], [(["AC"], half - 1), (["CA"], half - 1), (["AA"], 2)]])
    s = G.Sampler(pk, lib=lib)
    try:
        capfd.readouterr()
        assert s.lib.gph_engine_sfs_enable(s.engine, 2, None, 0, None, 0, 0) == EARG
        err = capfd.readouterr().err
        assert "locus 1" in err and str(1 << 32) in err and "2^32" in err
        assert s._sfs_shape() == (0, 0, 0, 0, 0, 0)
        s.sfs_enable(2, [0])
        assert s.sfs_observed()["sites"].tolist() == [5]
    finally:
        s.close()


def check_lifecycle(lib, G, name="m3", iters=3):
    """reset, enable twice, a full row buffer, GPH_EFULL one byte short with the feature off, GPH_ESTATE, disable, a rank without a
    selected locus"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    slots, groups = slot_table(pk)
    L, NS, NG, cap = pk.L, len(slots), len(groups), 2 * iters
    s = G.Sampler(pk, lib=lib)
    off = (0, 0, 0, 0, 0, 0)
    try:
        with pytest.raises(RuntimeError):
            s.sfs()                                        # not enabled
        with pytest.raises(RuntimeError):
            s.sfs_rows()
        with pytest.raises(RuntimeError):
            s.sfs_observed()
        assert s.lib.gph_engine_sfs_fetch_loci(s.engine, None, 0, 0) == ESTATE
        assert s.lib.gph_engine_sfs_sample(s.engine, 0) == ESTATE
        assert s._sfs_shape() == off
        s.sfs_enable(cap)
        G_ = s._sfs_shape()[2]
        assert s._sfs_shape() == (NS, NG, G_, L, 0, 0) and 1 <= G_ <= G_CAP
        tables = (((L * NS * 12 + L * NG * 4 + L * 4 + 7) & ~7) + (NS + NG + 1) * 8 + 2 * (NS + NG) * 4 + 15) & ~15
        need = tables + ((pk.n + pk.Kc + 15) & ~15) + ((L + G_ - 1) // G_ + cap) * (1 + NS) * 8
        assert s.lib.gph_engine_sfs_sample(s.engine, 0) == ESTATE                   # before initialize
        assert s.lib.gph_engine_sfs_enable(s.engine, cap, None, 0, None, 0, need - 1) == FULL
        assert s._sfs_shape() == off                       # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.sfs_enable(cap, max_bytes=need - 1)
        s.initialize()                                     # the engine is still usable
        with pytest.raises(RuntimeError):
            s.sfs_sample(0)
        s.sfs_enable(cap, [1, 2], [])                      # enable twice: another selection and no pair, then the real one
        assert s._sfs_shape()[:2] + s._sfs_shape()[3:] == (NS - 4 * len(all_pairs(pk)), NG - len(all_pairs(pk)), 2, 0, 0)
        s.sfs_enable(cap, max_bytes=need)
        before, data = s.sfs(), s.sfs_observed()
        assert before["samples"] == 0 and not before["E"].any() and data["obs"].any() and data["sites"].all()
        for it in range(iters):
            s.iteration(it)
            s.sfs_sample(it)
        first = s.sfs(reset=True)
        assert first["samples"] == iters and first["E"].any()
        zero = s.sfs()
        assert zero["samples"] == 0 and not zero["E"].any()
        assert s.sfs_observed()["obs"].tobytes() == data["obs"].tobytes()          # the data side stays
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.sfs_sample(it)
        assert s._sfs_shape() == (NS, NG, G_, L, iters, cap)
        with pytest.raises(BufferError):
            s.sfs_sample(99)                               # the row buffer is full
        assert s.lib.gph_engine_sfs_sample(s.engine, 99) == FULL
        second = s.sfs()
        its, rows = s.sfs_rows()
        assert its.tolist() == list(range(2 * iters)) and s._sfs_shape()[5] == 0
        s2 = G.Sampler(pk, lib=lib)                        # the same chain, sampled over the second half only
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.sfs_enable(cap)
                s2.iteration(it)
                if it >= iters:
                    s2.sfs_sample(it)
            fresh = s2.sfs()
            rows2 = s2.sfs_rows()[1]
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters and second["E"].tobytes() == fresh["E"].tobytes()
        assert rows[iters:].tobytes() == rows2.tobytes()
        s.initialize()                                     # a new chain starts from zeroed accumulators and no rows, the data side stays
        again = s.sfs()
        assert again["samples"] == 0 and not again["E"].any() and s._sfs_shape()[5] == 0
        assert s.sfs_observed()["use"].tobytes() == data["use"].tobytes()
        s.sfs_enable(4, [])                                # no selected locus: the fold alone, rows of zeros
        c0 = s.class_stats(CLS_DATA)["launches"]
        s.sfs_sample(0)
        s.sfs_sample(1)
        e, o = s.sfs(), s.sfs_observed()
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["E"].shape == (0, NS) and s.class_stats(CLS_DATA)["launches"] == c0
        assert not o["obs_total"].any() and o["sites_total"] == 0
        its, rows = s.sfs_rows()
        assert its.tolist() == [0, 1] and rows.shape == (2, NS) and not rows.any()
        s.sfs_enable(0)                                    # disable
        assert s._sfs_shape() == off
        assert s.lib.gph_engine_sfs_sample(s.engine, 0) == ESTATE
    finally:
        s.close()


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """records and final state dump with sampling on identical to a run with sampling off, and still the reference's records;
    launches of class 27 = the samples; no host synchronisation added by the sample calls.  Returns the two runs"""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        r = run_chain(lib, name, full, sample=on, trees=False, record=rec, final=final, pack=G.Pack.load(os.path.join(GOLDEN, name + ".gpk")))
        out.append(dict(rec=rec, final=final, stats=r["stats"], launches=r["launches"], samples=r["sf"][full]["samples"] if on else 0))
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


def genome_text(names, its, rows, observed, Q):
    """PREFIX.sfs-genome.tsv and the line on stdout from the rows as added and the observed totals"""
    S, NS = len(its), len(names)
    out = ["\t".join(["iter"] + names)]
    out += ["%7d" % it + "".join("\t" + _g(float(v)) for v in rows[k]) for k, it in enumerate(its)]
    lines, best = [["# observed"], ["# mean"], ["# sd"], ["# ratio"], ["# z"]], (-1.0, "none")
    for s in range(NS):
        tot = 0.0
        for k in range(S):
            tot = tot + float(rows[k][s])
        mean = tot / float(S) if S else 0.0
        ss = 0.0
        for k in range(S):
            ss = ss + (float(rows[k][s]) - mean) * (float(rows[k][s]) - mean)
        sd = math.sqrt(ss / float(S - 1)) if S > 1 else 0.0
        ob = float(int(observed[s]))
        ratio = ob / mean if mean != 0.0 else 0.0
        den = math.sqrt(mean + sd * sd)
        z = (ob - mean) / den if den != 0.0 else 0.0
        for ln, v in zip(lines, (str(int(observed[s])), _g(mean), _g(sd), _g(ratio), _g(z))):
            ln.append(v)
        if abs(z) > best[0]:
            best = (abs(z), f"{names[s]} observed {int(observed[s])} mean {_g(mean)} ratio {_g(ratio)} z {_g(z)}")
    out += ["\t".join(ln) for ln in lines] + [f"# loci {Q} samples {S}"]
    return "\n".join(out) + "\n", "SFS: " + best[1]


def expected_files(ctl_dir, ctl, lib=None, sampler_lib=None, loci=None, pairs=None):
    """the text of PREFIX.sfs.tsv and of PREFIX.sfs-genome.tsv the program must write and its line on stdout, formatted from the
    ABI's numbers of an equivalent Sampler run (burn-in first, a sample wherever a trace line is written)"""
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
        s.sfs_enable(len(its), loci, pairs)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it in its:
                s.sfs_sample(it)
        e, o = s.sfs(), s.sfs_observed()
        got_its, rows = s.sfs_rows()
    finally:
        s.close()
    S, Q = len(its), len(e["loci"])
    assert e["samples"] == S and got_its.tolist() == its
    slots, groups = slot_table(p, pairs)
    names, gn = slot_names(slots, lambda q: p.popName[q]), group_names(groups, lambda q: p.popName[q])
    out = ["\t".join(["locus", "name", "samples", "sites"] + ["use_" + g for g in gn] + [f"{w}_{nm}" for nm in names for w in ("obs", "exp")] + ["rel"])]
    for q, g in enumerate(e["loci"].tolist()):
        cells, sobs, sexp = [], 0.0, 0.0
        for k, sl in enumerate(slots):
            ex = (float(int(o["use"][q, sl[0]])) * float(e["E"][q, k])) / float(S)
            if sl[1] == "sfs":
                sobs = sobs + float(int(o["obs"][q, k]))
                sexp = sexp + ex
            cells += [str(int(o["obs"][q, k])), _g(ex)]
        out.append("\t".join([str(g), p.locusNames[g], str(S), str(int(o["sites"][q]))] + [str(int(u)) for u in o["use"][q]] + cells + [_g(sobs / sexp if sexp > 0.0 else 0.0)]))
    out.append(f"# loci {Q} samples {S} slots {len(slots)}")
    gen, log = genome_text(names, its, rows, o["obs_total"], Q)
    return "\n".join(out) + "\n", gen, log


def check_program(lib_path, lib, tmp_path):
    """both files of a short m3 run equal to files built from the ABI's numbers; --sfs-pairs, -loci and -rows; every other output
    of a run with -l -s --triplets --pair-times is the same bytes with and without; chain 0 of --mc3 / --replicates; the usage errors"""
    import subprocess
    import gphocs_amd as G
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import program_ctl
    name = "m3"
    ctl = name + ".ctl"
    a, b, c, d, e, m, r, z = (tmp_path / x for x in ("with", "without", "pairs", "all", "rest", "mc3", "rep", "none"))
    for x in (a, b, c, d, e, m, r, z):
        _copy_case(name, x, program_ctl(name))
    on = ["--sfs", "out"]
    run = _run(lib_path, a, on + [ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["sfs-genome.tsv", "sfs.tsv"]                          # no part left behind
    want_loci, want_gen, log = expected_files(str(a), ctl, lib, lib)
    assert got["sfs.tsv"] == want_loci
    assert got["sfs-genome.tsv"] == want_gen
    assert log in run.stdout.splitlines()
    # names in another order, a selection, a row buffer of 3 rows that fills several times; and no pair at all
    pn = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).popName
    _run(lib_path, c, on + ["--sfs-pairs", f"{pn[2]},{pn[0]};{pn[1]},{pn[2]}", "--sfs-loci", "1-9:4", "--sfs-rows", "3", ctl])
    want_loci2, want_gen2, _ = expected_files(str(c), ctl, lib, lib, [1, 5, 9], [(2, 0), (1, 2)])
    other = read_outputs(c, "out")
    assert other["sfs.tsv"] == want_loci2 and other["sfs-genome.tsv"] == want_gen2
    _run(lib_path, z, on + ["--sfs-pairs", "none", ctl])
    want_loci3, want_gen3, _ = expected_files(str(z), ctl, lib, lib, None, [])
    bins = read_outputs(z, "out")
    assert bins["sfs.tsv"] == want_loci3 and bins["sfs-genome.tsv"] == want_gen3 and "priv" not in want_gen3
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "-s", "cs", "--triplets", "tw", "--pair-times", "pt"]
    _run(lib_path, d, on + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix in ("cs", "tw", "pt"):
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
    for args, words in ((["--sfs-loci", "0-3"], ["--sfs "]), (["--sfs-pairs", f"{pn[0]},{pn[1]}"], ["--sfs "]), (["--sfs-rows", "4"], ["--sfs "]),
                        (on + ["--sfs-pairs", f"{pn[0]},nobody"], ["nobody", "--sfs-pairs"]),
                        (on + ["--sfs-pairs", f"{pn[0]}"], ["--sfs-pairs"]),
                        (on + ["--sfs-pairs", f"{pn[0]},{pn[0]}"], ["--sfs-pairs"]),
                        (on + ["--sfs-pairs", f"{pn[0]},{pn[1]},{pn[2]}"], ["--sfs-pairs"]),
                        (on + ["--sfs-pairs", f"{pn[0]},{pn[1]};{pn[1]},{pn[0]}"], ["twice", "--sfs-pairs"]),
                        (on + ["--sfs-pairs", f"{pn[0]},{pn[3]}"], [pn[3], "--sfs-pairs"]),                           # an ancestral population
                        (on + ["--sfs-loci", "5,5"], ["locus 5 ", "--sfs-loci"]), (on + ["--sfs-loci", f"3,{L}"], [f"locus {L} ", "--sfs-loci"]),
                        (on + ["--sfs-rows", "0"], ["usage"])):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and all(w in res.stderr for w in words), (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    ones = tmp_path / "one-leaf-populations"               # no population has two samples and no pair is taken
    os.makedirs(ones)
    (ones / "t.ctl").write_text(ONES_CTL)
    (ones / "t.seq").write_text("1\n\nl0 2 8\na0\tACGTACGT\nb0\tACGAACGT\n")
    res = subprocess.run([EXE] + on + ["--sfs-pairs", "none", "t.ctl"], cwd=ones, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode != 0 and "--sfs-pairs" in res.stderr and "no population" in res.stderr, res.stderr[-500:]
    assert sorted(os.listdir(ones)) == ["t.ctl", "t.seq"]
    cwd = os.getcwd()
    os.chdir(u)
    try:
        p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        anylib = lib or G.load_library(dims=(p.n, p.K, p.B))
        for kw in (dict(sfs_loci="0-3"), dict(sfs_pairs="A,B"), dict(sfs_rows=4), dict(sfs="out", sfs_rows=-1)):
            assert G.run_control_file(anylib, ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def part_lines(path):
    """(L lines, O totals, [(iteration, [floats])]) of a rank's part: the R lines carry the doubles' 64-bit patterns"""
    import struct
    L, O, R = [], None, []
    for ln in open(path).read().splitlines():
        if ln.startswith("L\t"):
            L.append(ln[2:])
        if ln.startswith("O\t"):
            O = [int(x) for x in ln.split("\t")[1:]]
        if ln.startswith("R\t"):
            f = ln.split("\t")
            R.append((int(f[1]), [struct.unpack("<d", struct.pack("<Q", int(x)))[0] for x in f[2:]]))
    return L, O, R


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, joined by gph_sfs_write: the per-locus file is the one-rank file (rows concatenated), the
    observed totals add to the one-rank totals, every per-sample row is the fp64 sum of the two parts' rows in rank order and the
    summary lines follow from those -- for all loci; for a selection that lies wholly in rank 1's block both files are the one-rank
    files byte for byte, from the launcher too; a part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, sfs="out", sfs_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["sfs-genome.tsv", "sfs.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        assert [int(ln.split("\t")[0]) for ln in want["sfs.tsv"].splitlines()[1:-1]] == loci
        run_ranks(lib_path, name, 2, two, sfs="out", sfs_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.sfs.part0", "out.sfs.part1"]
        (L0, O0, R0), (L1, O1, R1) = part_lines(two / "out.sfs.part0"), part_lines(two / "out.sfs.part1")
        assert [it for it, _ in R0] == [it for it, _ in R1] and len(R0) > 0
        added = [[(0.0 + x) + y for x, y in zip(v0, v1)] for (_, v0), (_, v1) in zip(R0, R1)]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.sfs.part{r}", cut)
            text = open(cut / "out.sfs.part1").read().splitlines(True)
            open(cut / "out.sfs.part1", "w").write("".join(text[:-1]))
            assert lib.gph_sfs_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_sfs_write(str(two / "out").encode(), 2) == 0
        joined = read_outputs(two, "out")
        assert sorted(joined) == ["sfs-genome.tsv", "sfs.tsv"]                  # no part among them
        assert joined["sfs.tsv"] == want["sfs.tsv"] and joined["sfs.tsv"].splitlines()[1:-1] == L0 + L1
        names = want["sfs-genome.tsv"].splitlines()[0].split("\t")[1:]
        observed = [x + y for x, y in zip(O0, O1)]
        assert ["# observed"] + [str(x) for x in observed] == [ln for ln in want["sfs-genome.tsv"].splitlines() if ln.startswith("# observed")][0].split("\t")
        assert joined["sfs-genome.tsv"] == genome_text(names, [it for it, _ in R0], added, observed, len(loci))[0]
        if spec is not None:
            # every selected locus lies in rank 1's block: rank 0 adds zeros, the sums are the one-rank sums of one workgroup
            assert joined == want
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--sfs", "out", "--sfs-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.sfs-genome.tsv must be written:
    status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.sfs-genome.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--sfs", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.sfs-genome.tsv"] and not os.listdir(d / "out.sfs-genome.tsv")
