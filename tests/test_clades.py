"""Per-locus clade tables (gph_engine_clades_*, gph_clades_consensus) on the CPU: the host-emulation build of the engine
sources runs k_clades' workgroup body over the same pages.

The tables are held to the contract of include/gphocs_hip.h by an independent restatement: one chain samples its gene trees
(k_gene_trees, tests/test_gene_trees.py holds those records to the state dumps) and its clades after every iteration, and
plain Python rebuilds the tables from the decoded records alone -- father climbs, integer masks, a dict under the insertion
rule.  Per locus the device's table must equal the model's AS A SET of (key, cnt, float.hex(age)) entries, with nkeys and
dropped; there is no tolerance anywhere in this file except the existing one of the chain against the golden's records.

Cases and iteration counts are CASES of tests/test_ancestry.py: m3, j1, a7, x8 on the default host build, b2 and n7 (72
leaves, two key words) on the host build with the reference's own caps.

Slot settings per case (SLOTS): the default; the tight one (the largest power of two with 3P/4 < n - 1: every locus drops
clades from its first sample on); a middle one at which, by the model alone, some locus fills up after its first sample and
some dropped clade comes again later and stays out.  The middle setting must also show a locus with dropped = 0.  The
goldens' posteriors are flat -- a locus visits 105 .. 764 distinct clades in these runs and, m3 apart, every locus of a
case about equally many (j1 274 .. 308, a7 313 .. 352, x8 411 .. 462, b2 105 .. 179, n7 753 .. 764) -- so only m3 has a power of
two whose limit separates its loci (512: limit 384 between 210 and 493 .. 537).  For the other cases the never-full table is
reached by a fourth, wide setting (the model must show dropped = 0 at every locus there; n7's default is that setting): each
of the three conditions is asserted for every case, over its middle and wide settings together, and the test fails when a
setting stops reaching them."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import compare_records
from sampler_util import EXE, _copy_case, _fmt, _locus_names, _run, hostemu_library, load_pack, printed_names, read_outputs, run_ranks
from test_ancestry import BIG, CASES, GOLDEN_ITERS
from test_gene_trees import PROGRAM_CASE, PROGRAM_LOCI, PROGRAM_SPEC, program_ctl

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

FULL, EARG, ESTATE = -5, -1, -4
CLS = 19                # timing class of k_clades
# name: (tight, middle, wide or None); 0 = the default is run besides
SLOTS = {"m3": (8, 512, None), "j1": (8, 64, 512), "a7": (8, 64, 512), "x8": (32, 64, 1024), "b2": (8, 32, 256), "n7": (64, 128, None)}
EDGE_CASE = "x8"        # 32 leaves: G = 8 records a workgroup, 10 loci


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


def default_slots(n):
    p = 2
    while p < 8 * (n - 1):
        p *= 2
    return p


def tight_slots(n):
    p = 2
    while 3 * (2 * p) // 4 < n - 1:
        p *= 2
    return p


# ---------------------------------------------------------------- the model: plain Python over decoded gene-tree records
def model_tables(t, n, limit):
    """per selected locus dict(tab {key: [cnt, age]}, dropped, first = nkeys after the first sample, again = a clade that was
    dropped came again later (and was dropped again: the rule never lets it in))"""
    S, Q = t["father"].shape[:2]
    N = 2 * n - 1
    out = []
    for q in range(Q):
        tab, dropped, first, seen_dropped, again = {}, 0, None, set(), False
        for s in range(S):
            father, age = t["father"][s, q].tolist(), t["age"][s, q].tolist()
            mask = [0] * N
            for i in range(n):
                v = i
                for _ in range(N):
                    f = father[v]
                    if not n <= f < N:
                        break
                    mask[f] |= 1 << i
                    v = f
            for v in range(n, N):
                k = mask[v]
                if k in tab:
                    tab[k][0] += 1
                    tab[k][1] = tab[k][1] + age[v]
                elif len(tab) < limit:
                    tab[k] = [1, age[v]]
                else:
                    dropped += 1
                    again = again or k in seen_dropped
                    seen_dropped.add(k)
            if s == 0:
                first = len(tab)
        out.append(dict(tab=tab, dropped=dropped, first=first, again=again))
    return out


def device_tables(c):
    """Sampler.clades() as a list of sets of (key, cnt, float.hex(age)), one per locus"""
    Q, P, W = c["keys"].shape if c["keys"].size else (len(c["loci"]), c["slots"], c["words"])
    out = []
    for q in range(Q):
        ent = set()
        for p in np.nonzero(c["cnt"][q])[0].tolist():
            key = sum(int(c["keys"][q, p, w]) << (64 * w) for w in range(W))
            ent.add((key, int(c["cnt"][q, p]), float(c["age"][q, p]).hex()))
        assert len(ent) == int(np.count_nonzero(c["cnt"][q])), "two slots of a table hold the same key"
        out.append(ent)
    return out


def run_chain(lib, name, iters, slots=0, loci=None, sample=True, record=None, trees=True, tag=""):
    """one chain over golden `name` (lib None: the tightest capacity variant) with a sample of the gene trees and of the
    clades after every iteration: the tables, the decoded gene trees, the final state dump, host_stats() after initialize
    and at the end, the launches of timing class 19, debug_oob()"""
    import gphocs_amd as G
    pk = load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.enable_clades(slots, loci)
        s.initialize()
        hs0 = s.host_stats()
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                s.sample_clades()
        hs1 = s.host_stats()
        s.set_record_file(None)
        c = s.clades() if sample else None
        t = s.gene_trees() if sample and trees else None
        return dict(clades=c, trees=t, pack=pk, stats=(hs0, hs1), launches=s.class_stats(CLS)["launches"], oob=s.debug_oob(), sampler_tag=tag)
    finally:
        s.close()


def check_tables(c, t, n, what):
    """item 1: the device's tables against the model of the same chain's gene-tree records; returns the model"""
    S, P, W, limit = c["samples"], c["slots"], c["words"], c["limit"]
    Q = len(c["loci"])
    assert W == (n + 63) // 64 and limit == 3 * P // 4 and P >= 2 and P & (P - 1) == 0
    assert c["keys"].shape == (Q, P, W) and c["cnt"].shape == (Q, P) and c["age"].shape == (Q, P)
    assert t["father"].shape[:2] == (S, Q) and t["loci"].tolist() == c["loci"].tolist()
    model = model_tables(t, n, limit)
    got = device_tables(c)
    root = (1 << n) - 1
    for q in range(Q):
        m = model[q]
        want = {(k, v[0], float(v[1]).hex()) for k, v in m["tab"].items()}
        assert got[q] == want, f"{what}: locus {int(c['loci'][q])}: {len(got[q] ^ want)} entries differ"
        assert int(c["nkeys"][q]) == len(m["tab"]) and int(c["dropped"][q]) == m["dropped"], f"{what}: locus {int(c['loci'][q])}"
        assert sum(e[1] for e in got[q]) + int(c["dropped"][q]) == S * (n - 1)
        cnt_root = [e[1] for e in got[q] if e[0] == root]
        if cnt_root or m["dropped"] == 0:               # (a table that was full before the root came never holds it)
            assert cnt_root == [S], f"{what}: locus {int(c['loci'][q])}: the root's clade"
    return model


def check_case(lib, name, iters, key="cpu"):
    """item 1 for one case: the default, the tight, the middle and (where the middle cannot show it) the wide setting"""
    tight, middle, wide = SLOTS[name]
    seen = dict(no_drop=False, fills_later=False, again=False)
    launches = []
    for slots in (0, tight, middle) + ((wide,) if wide else ()):
        r = run_chain(lib, name, iters, slots)
        c, n = r["clades"], r["pack"].n
        assert c["samples"] == iters and c["loci"].tolist() == list(range(r["pack"].L))
        assert c["slots"] == (slots or default_slots(n))
        model = check_tables(c, r["trees"], n, f"{name} slots {slots}")
        launches.append(r["launches"])
        print(f"{name} [{key}] slots {c['slots']} limit {c['limit']}: nkeys {sorted(len(m['tab']) for m in model)} dropped {sorted(m['dropped'] for m in model)}")
        if slots == tight:
            assert tight == tight_slots(n) and 3 * tight // 4 < n - 1 <= 3 * (2 * tight) // 4
            assert all(m["first"] == c["limit"] and m["dropped"] >= iters * (n - 1 - c["limit"]) > 0 for m in model)
        if slots == middle:
            seen["fills_later"] = any(m["first"] < c["limit"] == len(m["tab"]) for m in model)
            seen["again"] = any(m["again"] for m in model)
            seen["no_drop"] = seen["no_drop"] or any(m["dropped"] == 0 for m in model)
        if slots == wide or (wide is None and slots == 0 and name != "m3"):
            assert all(m["dropped"] == 0 for m in model), f"{name}: the wide setting drops clades"
            seen["no_drop"] = True
        if name == "n7":
            assert c["words"] == 2 and any(k & ((1 << 64) - 1) and k >> 64 for m in model for k in m["tab"]), "no kept key with bits in both words"
        assert r["oob"][0] == 0
    assert all(seen.values()), f"{name}: the slot settings no longer reach {[k for k, v in seen.items() if not v]}"
    assert launches == [iters] * len(launches)


@pytest.mark.parametrize("name", list(CASES))
def test_tables_equal_the_model_over_the_gene_tree_records(hostemu, hostemu_big, name):
    check_case(hostemu_big if name in BIG else hostemu[1], name, CASES[name])


def test_one_record_a_workgroup(hostemu_big):
    """t136: 136 leaves -- G = 1, every lane of a workgroup on the one locus, keys of three words"""
    iters = 4
    r = run_chain(hostemu_big, "t136", iters)
    c, n = r["clades"], r["pack"].n
    assert 256 // n == 1 and c["words"] == 3 and c["samples"] == iters and r["launches"] == iters
    model = check_tables(c, r["trees"], n, "t136")
    assert all(m["dropped"] == 0 for m in model) and any(k >> 128 and k & ((1 << 64) - 1) for m in model for k in m["tab"])
    assert r["oob"][0] == 0


# ---------------------------------------------------------------- group edges
def check_group_edges(lib, name=EDGE_CASE, iters=5, slots=64):
    """item 2: selections of 1, G - 1, G and G + 1 loci and one with gaps -- each table equals, as a set, the same locus's
    table of the all-loci run; the usage errors of the gene-trees selection"""
    import gphocs_amd as G
    everything = run_chain(lib, name, iters, slots)
    pk = everything["pack"]
    n, L = pk.n, pk.L
    per_group = max(1, 256 // n)
    assert 2 <= per_group and per_group + 1 <= L, "the case has too few loci for a group and one more"
    P = np.diff(np.asarray(pk.pattern_offsets)).tolist()
    assert any(P[g] < P[g + 1] for g in range(L - 1)), "the loci are already in slot order: nothing is shown about the indirection"
    check_tables(everything["clades"], everything["trees"], n, f"{name} all")
    full = device_tables(everything["clades"])
    for sel in ([L - 1], list(range(1, per_group)), list(range(L - per_group, L)), list(range(per_group + 1)), list(range(0, L, 3))):
        r = run_chain(lib, name, iters, slots, loci=sel, trees=False)
        c = r["clades"]
        assert c["loci"].tolist() == sel and c["samples"] == iters and r["launches"] == iters
        got = device_tables(c)
        for q, g in enumerate(sel):
            assert got[q] == full[g], f"selection {sel}: locus {g}"
            assert (int(c["nkeys"][q]), int(c["dropped"][q])) == (int(everything["clades"]["nkeys"][g]), int(everything["clades"]["dropped"][g]))
    s = G.Sampler(pk, lib=lib)
    try:
        for bad in ([3, 2], [2, 2], [-1], [0, -1], [-2, 5]):
            with pytest.raises(ValueError):
                s.enable_clades(0, bad)
            assert s.lib.gph_engine_clades_enable(s.engine, 0, (ctypes.c_int64 * len(bad))(*bad), len(bad), 0) == EARG
        # beyond the rank's block: not this rank's, ignored -- a rank without a selected locus counts its samples, launches nothing
        s.enable_clades(0, [L + 5])
        s.initialize()
        n0 = s.host_stats()["launches"]
        s.sample_clades()
        s.sample_clades()
        assert s.host_stats()["launches"] == n0 and s.class_stats(CLS)["launches"] == 0
        c = s.clades()
        assert c["samples"] == 2 and c["loci"].tolist() == [] and c["keys"].shape == (0, default_slots(n), 1)
    finally:
        s.close()


def test_group_edges_and_selections(hostemu):
    check_group_edges(hostemu[1])


# ---------------------------------------------------------------- the chain is untouched
def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """item 3: over the golden's whole run, records and final state dump with sampling on identical to a run with sampling
    off, and still the reference's records.  Returns the two runs."""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        s = G.Sampler(pk, lib=lib)
        try:
            s.set_record_file(rec)
            if on:
                s.enable_clades()
            s.initialize()
            hs0 = s.host_stats()
            for it in range(full):
                s.iteration(it)
                if on:
                    s.sample_clades()
            hs1 = s.host_stats()
            s.set_record_file(None)
            samples = s.clades()["samples"] if on else 0
            s.dump_state(final, True)
            out.append(dict(rec=rec, final=final, stats=(hs0, hs1), launches=s.class_stats(CLS)["launches"], samples=samples))
        finally:
            s.close()
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    return on, off


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)


# ---------------------------------------------------------------- lifecycle
def check_lifecycle(lib, G, name="m3", iters=6):
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    n, L = pk.n, pk.L
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.clades()                                 # not enabled
        assert s.lib.gph_engine_clades_fetch(s.engine, None, None, None, 0) == ESTATE
        assert s._clades_shape() == (0, 0, 0, 0, 0)
        for bad in (1, 3, 12, 96, -2, -64):
            assert s.lib.gph_engine_clades_enable(s.engine, bad, None, 0, 0) == EARG
            with pytest.raises(ValueError):
                s.enable_clades(bad)
        s.enable_clades(16)
        assert s._clades_shape() == (L, 16, 1, 12, 0)
        need = L * (16 * 3 * 8 + 8)
        assert s.lib.gph_engine_clades_enable(s.engine, 16, None, 0, need - 1) == FULL
        with pytest.raises(MemoryError):
            s.enable_clades(16, max_bytes=need - 1)
        s.initialize()                                 # the engine is still usable
        assert s.lib.gph_engine_clades_sample(s.engine) == ESTATE
        with pytest.raises(RuntimeError):
            s.sample_clades()                          # the refused enable left the feature off
        s.enable_clades(2)                             # the smallest table: one clade a locus
        assert s._clades_shape() == (L, 2, 1, 1, 0)
        s.enable_clades(16, max_bytes=need)
        for it in range(iters):
            s.iteration(it)
            s.sample_clades()
        first = s.clades(reset=True)
        assert first["samples"] == iters and np.all(first["nkeys"] == 12) and np.all(first["cnt"].sum(axis=1) + first["dropped"] == iters * (n - 1))
        zero = s.clades()
        assert zero["samples"] == 0 and not zero["cnt"].any() and not zero["keys"].any() and not zero["age"].view(np.uint64).any()
        assert not zero["nkeys"].any() and not zero["dropped"].any()
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.sample_clades()
        second = s.clades()
        s2 = G.Sampler(pk, lib=lib)                    # the same chain, sampled over the second half only
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.enable_clades(16)
                s2.iteration(it)
                if it >= iters:
                    s2.sample_clades()
            fresh = s2.clades()
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        assert device_tables(second) == device_tables(fresh) and device_tables(second) != device_tables(first)
        assert second["nkeys"].tolist() == fresh["nkeys"].tolist() and second["dropped"].tolist() == fresh["dropped"].tolist()
        s.initialize()                                 # a new chain starts from empty tables
        assert s.clades()["samples"] == 0 and not s.clades()["cnt"].any()
    finally:
        s.close()
    s = G.Sampler(pk, lib=lib)
    try:
        assert s.lib.gph_engine_clades_sample(s.engine) == ESTATE      # before enable, before initialize
        s.initialize()
        with pytest.raises(RuntimeError):
            s.sample_clades()
    finally:
        s.close()


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_lifecycle(hostemu[1], G)


# ---------------------------------------------------------------- the consensus as text
def parse_consensus(text):
    """the tree text back into (set of (frozenset of leaf labels, support text, age text) of the annotated nodes, the leaf
    labels in the order they appear, the children's smallest-leaf order holds)"""
    pos, clades, order = 0, [], []

    def node():
        nonlocal pos
        if text[pos] != "(":
            end = pos
            while text[end] not in ",();[":
                end += 1
            label, pos = text[pos:end], end
            order.append(label)
            return frozenset([label]), label
        pos += 1
        kids = []
        while True:
            kids.append(node())
            pos += 1
            if text[pos - 1] == ")":
                break
            assert text[pos - 1] == ","
        assert len(kids) >= 2
        mine = frozenset().union(*[k[0] for k in kids])
        assert sum(len(k[0]) for k in kids) == len(mine)
        if text.startswith("[&support=", pos):
            end = text.index("]", pos)
            sup, age = text[pos + 10:end].split(",age=")
            clades.append((mine, sup, age))
            pos = end + 1
        return mine, kids[0][1]
    node()
    assert text[pos:] == ";"
    return clades, order


def py_consensus(tab, S, n, labels):
    """the grammar of include/gphocs_hip.h restated over {key: (cnt, age)}: (text, resolved)"""
    major = {k: v for k, v in tab.items() if 2 * v[0] > S}
    root = (1 << n) - 1

    def sub(k):
        inside = sorted((c for c in major if c != k and c & k == c), key=lambda c: -bin(c).count("1"))
        top = []
        for c in inside:
            if not any(c & o == c for o in top):
                top.append(c)
        covered = 0
        for c in top:
            covered |= c
        kids = [((c & -c).bit_length() - 1, sub(c)) for c in top] + [(i, labels[i]) for i in range(n) if k >> i & 1 and not covered >> i & 1]
        text = "(" + ",".join(x for _, x in sorted(kids)) + ")"
        if k in major:
            text += "[&support=%.10g,age=%.10g]" % (major[k][0] / S, major[k][1] / major[k][0])
        return text
    return (labels[0] if n == 1 else sub(root)) + ";", len(major)


def _entries(tab, n):
    """{key: (cnt, age)} as the keys / cnt / age arrays of one locus, in a table of 64 slots"""
    W = (n + 63) // 64
    keys, cnt, age = np.zeros((64, W), dtype=np.uint64), np.zeros(64, dtype=np.uint64), np.zeros(64)
    for p, (k, (c, a)) in enumerate(tab.items()):
        for w in range(W):
            keys[5 + p, w] = (k >> (64 * w)) & ((1 << 64) - 1)
        cnt[5 + p], age[5 + p] = c, a
    return keys, cnt, age


def test_consensus_of_hand_built_tables(hostemu):
    import gphocs_amd as G
    lib = hostemu[1]
    lab = [f"s{i}.{i}" for i in range(5)]
    # five leaves, 10 samples: {0,1} 9 times, {0,1,2} 6 times, {3,4} exactly half (not in), {2,3} 2 times, the root always
    tab = {0b00011: (9, 4.5), 0b00111: (6, 12.0), 0b11000: (5, 5.0), 0b01100: (2, 1.0), 0b11111: (10, 1.0 / 3.0)}
    text, res = G.clades_consensus(lib, *_entries(tab, 5), 10, lab)
    assert text == "(((s0.0,s1.1)[&support=0.9,age=0.5],s2.2)[&support=0.6,age=2],s3.3,s4.4)[&support=1,age=0.03333333333];" and res == 3
    assert (text, res) == py_consensus(tab, 10, 5, lab)
    # children by their smallest leaf: the clade {1,4} comes after leaf 0 and before leaves 2, 3
    tab = {0b10010: (3, 3.0), 0b11111: (3, 6.0)}
    assert G.clades_consensus(lib, *_entries(tab, 5), 3, lab) == ("(s0.0,(s1.1,s4.4)[&support=1,age=1],s2.2,s3.3)[&support=1,age=2];", 2)
    # a full table that dropped the root's clade: the top level has no annotation and is not counted
    tab = {0b00011: (3, 3.0)}
    assert G.clades_consensus(lib, *_entries(tab, 5), 3, lab) == ("((s0.0,s1.1)[&support=1,age=1],s2.2,s3.3,s4.4);", 1)
    # an empty table, and a single leaf
    assert G.clades_consensus(lib, *_entries({}, 5), 3, lab) == ("(s0.0,s1.1,s2.2,s3.3,s4.4);", 0)
    assert G.clades_consensus(lib, *_entries({}, 1), 3, lab[:1]) == ("s0.0;", 0)
    # two key words: 70 leaves, a clade across the word boundary
    lab70 = [f"x.{i}" for i in range(70)]
    tab = {(1 << 63) | (1 << 64): (2, 2.0), (1 << 70) - 1: (2, 8.0)}
    text, res = G.clades_consensus(lib, *_entries(tab, 70), 2, lab70)
    assert (text, res) == py_consensus(tab, 2, 70, lab70) and "(x.63,x.64)[&support=1,age=1]" in text and res == 2
    # never a wrong tree: clades that overlap without nesting, a clade of one leaf, a bit beyond the leaves, a refused label
    for bad in ({0b00011: (3, 1.0), 0b00110: (3, 1.0), 0b11111: (3, 1.0)}, {0b00100: (3, 1.0)}, {0b100011: (3, 1.0)}):
        with pytest.raises(ValueError):
            G.clades_consensus(lib, *_entries(bad, 5), 3, lab)
    for labels in (["s0.0", "s 1.1", "s2.2", "s3.3", "s4.4"], ["s0.0", "x;y.1", "s2.2", "s3.3", "s4.4"], ["a(b", "s1.1", "s2.2", "s3.3", "s4.4"]):
        with pytest.raises(ValueError):
            G.clades_consensus(lib, *_entries({0b11111: (3, 1.0)}, 5), 3, labels)


def check_consensus_of_a_chain(lib, name="g1", iters=30, loci=(0, 3, 6, 9, 17)):
    """the consensus of sampled tables: the text is the restated grammar, parses back, and its clade set is exactly the kept
    clades with 2 cnt > S"""
    import gphocs_amd as G
    r = run_chain(lib, name, iters, 0, loci=list(loci), trees=False)
    c, n = r["clades"], r["pack"].n
    lib = lib or G.load_library(dims=(n, r["pack"].K, r["pack"].B))       # (the builder is host code: any build of the library)
    labels = [f"L{i}.{i}" for i in range(n)]
    tabs = device_tables(c)
    some = 0
    for q in range(len(loci)):
        text, res = G.clades_consensus(lib, c["keys"][q], c["cnt"][q], c["age"][q], iters, labels)
        tab = {k: (cnt, float.fromhex(a)) for k, cnt, a in tabs[q]}
        assert (text, res) == py_consensus(tab, iters, n, labels)
        clades, order = parse_consensus(text)
        want = {(frozenset(labels[i] for i in range(n) if k >> i & 1), "%.10g" % (v[0] / iters), "%.10g" % (v[1] / v[0]))
                for k, v in tab.items() if 2 * v[0] > iters}
        assert set(clades) == want and len(clades) == len(want) == res and sorted(order) == sorted(labels)
        assert any(len(m) == n for m, _, _ in clades)                 # the root's clade: cnt = S
        some += res > 1
    print(f"{name}: loci whose consensus resolves more than the root: {some} of {len(loci)}")


def test_consensus_of_sampled_tables(hostemu):
    check_consensus_of_a_chain(hostemu[1])


# ---------------------------------------------------------------- the program and the launcher
def expected_files(ctl_dir, ctl, spec_loci, lib=None, sampler_lib=None, F=0.5, slots=0):
    """the text of PREFIX.clades.tsv and PREFIX.consensus.tsv the program must write: an equivalent Sampler run (burn-in
    first, a sample wherever a trace line is written), both files restated in Python over Sampler.clades().  Returns the two
    texts, the tables as {key: (cnt, age)} per locus, the pack and the labels"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.enable_clades(slots, spec_loci)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.sample_clades()
        c = s.clades()
    finally:
        s.close()
    n, S = p.n, c["samples"]
    names = printed_names(p.sampleNames)
    labels = [f"{names[i]}.{i}" for i in range(n)]
    tabs = [{k: (cnt, float.fromhex(a)) for k, cnt, a in ent} for ent in device_tables(c)]
    rows = ["\t".join(["locus", "name", "samples", "dropped", "size", "support", "meanAge", "members"])]
    trees = ["\t".join(["locus", "name", "samples", "distinct", "dropped", "resolved", "tree"])]
    for q, g in enumerate(c["loci"].tolist()):
        dropped = str(int(c["dropped"][q]))
        for k, (cnt, age) in sorted(tabs[q].items(), key=lambda kv: (-kv[1][0], bin(kv[0]).count("1"), kv[0])):
            if cnt / S >= F:
                rows.append("\t".join([str(g), p.locusNames[g], str(S), dropped, str(bin(k).count("1")), _fmt(cnt / S), _fmt(age / cnt),
                                       ",".join(labels[i] for i in range(n) if k >> i & 1)]))
        text, resolved = py_consensus(tabs[q], S, n, labels)
        trees.append("\t".join([str(g), p.locusNames[g], str(S), str(int(c["nkeys"][q])), dropped, str(resolved), text]))
    return "\n".join(rows) + "\n", "\n".join(trees) + "\n", tabs, p, labels


def check_program(lib_path, lib, tmp_path, name=PROGRAM_CASE):
    """item 6: both files are the restatement over an equivalent Sampler run, character for character; the consensus parses
    back to exactly the kept clades with 2 cnt > S; --clades-min-support 0 lists every kept clade; the other options' files do
    not change; the usage errors"""
    a, b, z, d, e = (tmp_path / x for x in ("with", "without", "zero", "all", "rest"))
    for x in (a, b, z, d, e):
        _copy_case(name, x, program_ctl(name))
    ctl = name + ".ctl"
    _run(lib_path, a, ["--clades", "out", "--clades-loci", PROGRAM_SPEC, ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    want_rows, want_trees, tabs, p, labels = expected_files(str(a), ctl, PROGRAM_LOCI, lib, lib)
    assert sorted(got) == ["clades.tsv", "consensus.tsv"]                # no part left behind
    assert got["clades.tsv"] == want_rows and got["consensus.tsv"] == want_trees
    S = len(open(trace).read().splitlines()) - 1
    assert S == 14
    seq_names = _locus_names(a / (name + ".seq"))
    lines = [ln.split("\t") for ln in got["consensus.tsv"].splitlines()[1:]]
    assert [int(r[0]) for r in lines] == PROGRAM_LOCI and all(r[1] == seq_names[int(r[0])] and int(r[2]) == S for r in lines)
    for q, r in enumerate(lines):
        clades, order = parse_consensus(r[6])
        want = {frozenset(labels[i] for i in range(p.n) if k >> i & 1) for k, v in tabs[q].items() if 2 * v[0] > S}
        assert {m for m, _, _ in clades} == want and len(clades) == len(want) == int(r[5]) and sorted(order) == sorted(labels)
        assert int(r[3]) == len(tabs[q])
    rows = [ln.split("\t") for ln in got["clades.tsv"].splitlines()[1:]]
    assert all(float(r[5]) >= 0.5 for r in rows) and {int(r[0]) for r in rows} == set(PROGRAM_LOCI)
    # every kept clade, and a table of another size
    _run(lib_path, z, ["--clades", "out", "--clades-loci", PROGRAM_SPEC, "--clades-min-support", "0", "--clades-slots", "32", ctl])
    zero = read_outputs(z, "out")
    want_rows, want_trees, ztabs, _, _ = expected_files(str(z), ctl, PROGRAM_LOCI, lib, lib, F=0.0, slots=32)
    assert zero["clades.tsv"] == want_rows and zero["consensus.tsv"] == want_trees
    assert len(zero["clades.tsv"].splitlines()) - 1 == sum(len(t) for t in ztabs) == 24 * len(PROGRAM_LOCI)
    assert any(int(ln.split("\t")[4]) > 0 for ln in zero["consensus.tsv"].splitlines()[1:])        # tables that dropped clades
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "-s", "cs", "--time-slices", "4", "--ancestry", "an", "--gene-trees", "gt", "--gene-trees-loci", "1-5"]
    _run(lib_path, d, ["--clades", "out", "--clades-loci", PROGRAM_SPEC] + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix, count in (("cs", 2 + 3 * p.K), ("an", 2), ("gt", 1)):
        other = read_outputs(e, prefix)
        assert len(other) == count and read_outputs(d, prefix) == other
    assert open(d / (name + ".trace")).read() == open(e / (name + ".trace")).read() == open(trace).read()
    # usage errors: before any iteration, nothing written
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    on = ["--clades", "out"]
    for args, word in ((["--clades-loci", "0-3"], "--clades"), (["--clades-slots", "64"], "--clades"), (["--clades-min-support", "0.3"], "--clades"),
                       (["--clades-min-support", "0"], "--clades"),
                       (on + ["--clades-slots", "96"], "power of two"), (on + ["--clades-slots", "1"], "power of two"), (on + ["--clades-slots", "0"], "power of two"),
                       (on + ["--clades-min-support", "1.5"], "[0, 1]"), (on + ["--clades-min-support", "-0.1"], "[0, 1]"), (on + ["--clades-min-support", "half"], "[0, 1]"),
                       (on + ["--clades-loci", "0-4,3"], "locus 3 "), (on + ["--clades-loci", "5,5"], "locus 5 "), (on + ["--clades-loci", f"3,{p.L}"], f"locus {p.L} "),
                       (on + ["--clades-loci", "0-30:4"], f"locus {(p.L + 3) // 4 * 4} "), (on + ["--clades-loci", "2-x"], "2-x")):
        r = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    # the same refusals from the options struct (a caller of gph_run that is not the launcher)
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(u)
    try:
        for kw in (dict(clades_loci="0-3"), dict(clades_slots=64), dict(clades_min_support=0.3), dict(clades="out", clades_slots=96),
                   dict(clades="out", clades_min_support=1.5)):
            assert G.run_control_file(lib or G.load_library(dims=(p.n, p.K, p.B)), ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])
    # a name that cannot stand in a tree: refused with --clades before the first iteration
    v = tmp_path / "name"
    _copy_case(name, v, program_ctl(name, lambda x: re.sub(r"(\bsamples\s+)s0\b", r"\1A=1", x, count=1)))
    seq, count = re.subn(r"(?m)^s0(\s)", r"A=1\1", open(v / (name + ".seq")).read())
    assert count == p.L
    open(v / (name + ".seq"), "w").write(seq)
    r = subprocess.run([EXE, "--clades", "out", ctl], cwd=v, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and "cannot stand in a tree" in r.stderr and "A=1" in r.stderr
    assert sorted(os.listdir(v)) == sorted([ctl, name + ".seq"])


def test_program_writes_the_clades_and_consensus_files(hostemu, tmp_path):
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, concatenated by gph_clades_write, are the one-rank files -- for all loci, and for a
    selection that lies wholly in rank 1's block; the launcher does the same; a part cut short or missing is refused and
    nothing is left"""
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, clades="out", clades_loci=spec, clades_slots=64)
        assert pk.L == 16
        want = read_outputs(one, "out")
        assert sorted(want) == ["clades.tsv", "consensus.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        assert [int(ln.split("\t")[0]) for ln in want["consensus.tsv"].splitlines()[1:]] == loci
        assert all(ln.split("\t")[2] == str(GOLDEN_ITERS[name]) for ln in want["consensus.tsv"].splitlines()[1:])
        run_ranks(lib_path, name, 2, two, clades="out", clades_loci=spec, clades_slots=64)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.clades.part0", "out.clades.part1"]
        if spec is not None:                                         # rank 0 holds no selected locus: a part without rows
            assert open(two / "out.clades.part0").read() == "GPHCL1\nE\t0\n"
        else:
            for kind in ("cut", "gone"):
                d = tmp_path / kind
                os.makedirs(d)
                for r in range(2):
                    shutil.copy(two / f"out.clades.part{r}", d)
                if kind == "cut":
                    text = open(d / "out.clades.part1").read().splitlines(True)
                    open(d / "out.clades.part1", "w").write("".join(text[:-1]))
                else:
                    os.unlink(d / "out.clades.part0")
                assert lib.gph_clades_write(str(d / "out").encode(), 2) != 0
                assert not read_outputs(d, "out")
        assert lib.gph_clades_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                      # no part among them
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--clades", "out", "--clades-loci", spec, "--clades-slots", "64", name + ".ctl"])
            assert read_outputs(three, "out") == want


def test_ranks_concatenate_to_the_one_rank_files(hostemu, tmp_path):
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.consensus.tsv must be written:
    status non-zero, no part and no file of ours left, for one rank and for two"""
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.consensus.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--clades", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.consensus.tsv"] and not os.listdir(d / "out.consensus.tsv")


def test_failed_run_leaves_no_clades_files(hostemu, tmp_path):
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)
