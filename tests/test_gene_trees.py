"""Sampled genealogies per locus (gph_engine_gene_trees_*, `G-PhoCS-hip --gene-trees PREFIX`) on the CPU: the host-emulation
build of the engine sources runs k_gene_trees' workgroup body over the same pages.

A record describes one locus at one sample: the node records, root, the live migrations in `living` order and the two
log-likelihoods -- what the LOCUS, N and M lines of a state dump print at the same point of the chain.  Every field must be
EQUAL to the dump's, ages as float.hex; there is no tolerance anywhere in this file except the existing one of the chain
against the golden's records.  The tree text is restated here in plain Python over the decoded records and parsed back.

m3, j1, a7 and x8 run on the default host build, b2 (20 bands: GPH_BIG_BANDS) and n7 (72 leaves: GPH_BIG_TREE) on the
host build with the reference's own caps; the iteration counts are those of tests/test_ancestry.py."""
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
from sampler_util import EXE, _copy_case, _fmt, _locus_names, _pop_names, _run, hostemu_library, load_pack, printed_names, read_outputs, run_ranks
from test_ancestry import BIG, CASES, GOLDEN_ITERS

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

FULL, EARG, ESTATE = -5, -1, -4
MIGS = 10               # GPH_MAX_MIGS
INT_FIELDS = ("father", "left", "right", "npop", "root", "num_migs", "mig_branch", "mig_band", "mig_spop", "mig_tpop")
HEX_FIELDS = ("age", "dataLnL", "genLnL", "mig_age")
PROGRAM_CASE, PROGRAM_SPEC, PROGRAM_LOCI = "g1", "0-9:3,17", [0, 3, 6, 9, 17]       # g1: 24 loci


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


# ---------------------------------------------------------------- the state dumps
def parse_dump(path):
    """{global locus: dict(root, dataLnL, genLnL, nodes [(father, left, right, age, npop)], migs [(branch, band, spop, tpop,
    age)] in M-line order)} of a state dump; ages and log-likelihoods as floats read from the dump's hex"""
    loci, cur = {}, None
    for ln in open(path):
        t = ln.split()
        if not t:
            continue
        if t[0] == "LOCUS":
            assert t[2] == "root" and t[4] == "dataLnL" and t[6] == "genLnL"
            cur = dict(root=int(t[3]), dataLnL=float.fromhex(t[5]), genLnL=float.fromhex(t[7]), nodes=[], migs=[])
            loci[int(t[1])] = cur
        elif t[0] == "N" and cur is not None:
            assert int(t[1]) == len(cur["nodes"])
            cur["nodes"].append((int(t[2]), int(t[3]), int(t[4]), float.fromhex(t[5]), int(t[6])))
        elif t[0] == "M" and cur is not None:
            assert len(t) == 2 + int(t[1])
            for w in t[2:]:
                f = w.split(":")                     # mg:branch:band:spop:tpop:sev:tev:age
                cur["migs"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), float.fromhex(f[7])))
    return loci


def expected_from_dump(loci, which, N):
    """the arrays Sampler.gene_trees() must return for one sample, from that sample's dump: ints as int arrays, fp64 values
    as lists of float.hex"""
    Q = len(which)
    ints = {k: np.full((Q, N) if k in ("father", "left", "right", "npop") else (Q, MIGS) if k.startswith("mig_") else (Q,), -1, dtype=np.int64)
            for k in INT_FIELDS}
    hexes = dict(age=[], dataLnL=[], genLnL=[], mig_age=[])
    for q, g in enumerate(which):
        d = loci[g]
        assert len(d["nodes"]) == N and len(d["migs"]) <= MIGS
        for v, (fa, le, ri, _, pop) in enumerate(d["nodes"]):
            ints["father"][q, v], ints["left"][q, v], ints["right"][q, v], ints["npop"][q, v] = fa, le, ri, pop
        ints["root"][q], ints["num_migs"][q] = d["root"], len(d["migs"])
        for k, (br, band, sp, tp, _) in enumerate(d["migs"]):
            ints["mig_branch"][q, k], ints["mig_band"][q, k], ints["mig_spop"][q, k], ints["mig_tpop"][q, k] = br, band, sp, tp
        hexes["age"].append([nd[3].hex() for nd in d["nodes"]])
        hexes["dataLnL"].append(d["dataLnL"].hex())
        hexes["genLnL"].append(d["genLnL"].hex())
        hexes["mig_age"].append([m[4].hex() for m in d["migs"]] + [(0.0).hex()] * (MIGS - len(d["migs"])))
    return ints, hexes


def _hexes(a):
    a = np.asarray(a)
    return [x.hex() for x in a.tolist()] if a.ndim == 1 else [[x.hex() for x in r] for r in a.tolist()]


def what_the_dumps_show(dumps, n):
    """the observations the conditions against a vacuous pass need, from the dumps alone"""
    seen = dict(mig_on_internal_branch=False, two_live_migs=False, ancient_leaf=False)
    for loci in dumps:
        for d in loci.values():
            seen["mig_on_internal_branch"] |= any(m[0] >= n for m in d["migs"])
            seen["two_live_migs"] |= len(d["migs"]) >= 2
            seen["ancient_leaf"] |= any(d["nodes"][i][3] > 0.0 for i in range(n))
    return seen


def run_chain(lib, name, iters, tmp, sample=True, dumps=False, record=None, capacity=None, loci=None, tag=""):
    """one chain over golden `name` (lib None: the tightest capacity variant), a sample after every iteration: the decoded
    records (with the raw bytes), the final state dump, the per-iteration dumps, the pack, host_stats() after initialize and
    at the end, the launches of timing class 17, debug_oob()"""
    import gphocs_amd as G
    pk = load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            s.enable_gene_trees(capacity or iters, loci)
        s.initialize()
        hs0 = s.host_stats()
        paths = []
        for it in range(iters):
            s.iteration(it)
            if sample:
                s.sample_gene_trees(it)
            if dumps:
                p = str(tmp / f"{name}.{it}.dump")
                s.dump_state(p, False)
                paths.append(p)
        hs1 = s.host_stats()
        s.set_record_file(None)
        trees = s.gene_trees(raw=True) if sample else None
        final = str(tmp / f"{name}.final.{'s' if sample else 'n'}{'d' if dumps else ''}{tag}")
        s.dump_state(final, True)
        return dict(trees=trees, final=final, dumps=paths, pack=pk, stats=(hs0, hs1), launches=s.class_stats(17)["launches"], oob=s.debug_oob())
    finally:
        s.close()


_SEEN = {}              # (which libraries, golden) -> what its dumps showed: the conditions over the whole case set


def check_against_dumps(lib, name, iters, tmp_path, key="cpu"):
    """item 1: sampled at every iteration with a state dump there -- every field of every record of every locus"""
    r = run_chain(lib, name, iters, tmp_path, dumps=True)
    pk, t = r["pack"], r["trees"]
    n, L, N = pk.n, pk.L, 2 * pk.n - 1
    assert t["iters"].tolist() == list(range(iters)) and t["loci"].tolist() == list(range(L))
    assert t["age"].shape == (iters, L, N) and t["mig_age"].shape == (iters, L, MIGS) and t["root"].shape == (iters, L)
    assert t["records"].shape[2] % 16 == 0 and 16 * N + 288 <= t["records"].shape[2] <= 16 * N + 288 + 5 * 16
    dumps = [parse_dump(p) for p in r["dumps"]]
    for s, loci in enumerate(dumps):
        assert sorted(loci) == list(range(L))
        ints, hexes = expected_from_dump(loci, range(L), N)
        for k in INT_FIELDS:
            assert np.array_equal(t[k][s], ints[k]), f"{name}: sample {s}: {k} differs from the state dump"
        for k in HEX_FIELDS:
            assert _hexes(t[k][s]) == hexes[k], f"{name}: sample {s}: {k} differs from the state dump"
    assert r["launches"] == iters
    _SEEN[(key, name)] = what_the_dumps_show(dumps, n)
    print(f"{name}: {_SEEN[(key, name)]}")
    return r


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """item 3: over the golden's whole run, records and final state dump with sampling on byte-identical to a run with
    sampling off, and still the reference's records.  Returns the two runs."""
    rec_on, rec_off = str(tmp_path / "on.rtrace"), str(tmp_path / "off.rtrace")
    on = run_chain(lib, name, full, tmp_path, record=rec_on)
    off = run_chain(lib, name, full, tmp_path, sample=False, record=rec_off)
    assert open(rec_on).read() == open(rec_off).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(rec_on, os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["trees"]["iters"].tolist() == list(range(full))
    return on, off


def check_case_set(key, names):
    """item 5: the conditions against a vacuous pass that hold over the case set, from the dumps"""
    got = {c: any(_SEEN[(key, nm)][c] for nm in names) for c in ("mig_on_internal_branch", "two_live_migs", "ancient_leaf")}
    assert got["mig_on_internal_branch"], "no record with a migration on an internal node's branch"
    assert got["two_live_migs"], "no record with two live migrations"
    assert got["ancient_leaf"], "no leaf with age > 0"


@pytest.mark.parametrize("name", list(CASES))
def test_records_equal_the_state_dumps_and_leave_the_chain_unchanged(hostemu, hostemu_big, tmp_path, name):
    lib = hostemu_big if name in BIG else hostemu[1]
    r = check_against_dumps(lib, name, CASES[name], tmp_path)
    check_chain_untouched(lib, name, GOLDEN_ITERS[name], tmp_path)
    assert r["oob"][0] == 0


def test_the_case_set_reaches_every_path(hostemu, hostemu_big, tmp_path):
    for name in CASES:
        if ("cpu", name) not in _SEEN:        # (run alone: the dumps of the cases not checked yet in this process)
            check_against_dumps(hostemu_big if name in BIG else hostemu[1], name, CASES[name], tmp_path)
    check_case_set("cpu", list(CASES))


def test_a_record_of_more_than_one_trip(hostemu_big, tmp_path):
    """t136: 136 leaves -- a record of more than 256 units, which takes its workgroup's 256 lanes a second trip"""
    r = check_against_dumps(hostemu_big, "t136", 3, tmp_path, key="edge")
    assert r["trees"]["records"].shape[2] // 16 > 256
    assert r["oob"][0] == 0


def check_no_bands(lib, tmp_path, key="cpu"):
    """g2 has no migration band: num_migs is 0 everywhere and every migration entry is -1 / age 0"""
    r = check_against_dumps(lib, "g2", 3, tmp_path, key=key)
    t = r["trees"]
    assert r["pack"].B == 0 and not np.any(t["num_migs"]) and np.all(t["mig_branch"] == -1) and not np.any(t["mig_age"])


def test_a_model_without_bands_has_no_migration(hostemu, tmp_path):
    check_no_bands(hostemu[1], tmp_path)


# ---------------------------------------------------------------- selections
def check_selections(lib, tmp_path, iters=6):
    """item 2: the records of a selection are the corresponding records of the "all" run of the same chain, byte for byte"""
    import gphocs_amd as G
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    L = pk.L
    P = np.diff(np.asarray(pk.pattern_offsets)).tolist()
    # slots are sorted by decreasing pattern count: where the count rises from one locus to a later one, the later locus
    # sits in an earlier slot -- the slot order of this golden is not its locus order
    assert any(P[g] < P[g + 1] for g in range(L - 1)), "m3's loci are already in slot order: the test shows nothing about the indirection"
    third = list(range(0, L, 3))
    assert any(P[a] < P[b] for a, b in zip(third, third[1:])), "every third locus of m3 is in slot order"
    everything = run_chain(lib, "m3", iters, tmp_path, tag="all")["trees"]
    assert everything["loci"].tolist() == list(range(L))
    bd, units = 256, everything["records"].shape[2] // 16
    per_group = max(1, bd // units)           # records a workgroup
    sizes = set()
    for sel in ([0], [L - 1], [1, L - 1], third, None):
        r = run_chain(lib, "m3", iters, tmp_path, loci=sel, tag="sel")
        t, want = r["trees"], list(range(L)) if sel is None else sel
        assert t["loci"].tolist() == want and t["iters"].tolist() == list(range(iters))
        assert t["records"].tobytes() == everything["records"][:, want, :].tobytes(), f"selection {sel}"
        for k in INT_FIELDS + HEX_FIELDS:
            assert t[k].tobytes() == np.ascontiguousarray(everything[k][:, want]).tobytes(), f"selection {sel}: {k}"
        assert r["launches"] == iters
        sizes.add((len(want) * units) % bd != 0 and len(want) % per_group != 0)
    assert True in sizes                      # a unit count that is no multiple of the workgroup size: a last group in part
    s = G.Sampler(pk, lib=lib)
    try:
        for bad in ([3, 2], [2, 2], [-1], [0, -1], [-2, 5]):
            with pytest.raises(ValueError):
                s.enable_gene_trees(2, bad)
            assert s.lib.gph_engine_gene_trees_enable(s.engine, 2, (ctypes.c_int64 * len(bad))(*bad), len(bad), 0) == EARG
        # beyond the rank's block: not this rank's, ignored -- and a rank without a selected locus counts its samples, launches nothing
        s.enable_gene_trees(3, [L + 5])
        s.initialize()
        n0 = s.host_stats()["launches"]
        s.sample_gene_trees(7)
        s.sample_gene_trees(9)
        assert s.host_stats()["launches"] == n0 and s.class_stats(17)["launches"] == 0
        t = s.gene_trees()
        assert t["iters"].tolist() == [7, 9] and t["loci"].tolist() == [] and t["age"].shape == (2, 0, 2 * pk.n - 1)
    finally:
        s.close()


def test_selections(hostemu, tmp_path):
    check_selections(hostemu[1], tmp_path)


# ---------------------------------------------------------------- capacity and lifecycle
def check_capacity(lib, G):
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    s = G.Sampler(pk, lib=lib)
    C = ctypes
    try:
        with pytest.raises(RuntimeError):
            s.gene_trees()                             # not enabled
        got = C.c_int32()
        assert s.lib.gph_engine_gene_trees_fetch(s.engine, None, None, 0, C.byref(got)) == ESTATE
        s.enable_gene_trees(2)
        nsel, N, rb, _, held = s._gene_trees_shape()
        assert (nsel, N, held) == (pk.L, 2 * pk.n - 1, 0) and rb % 16 == 0
        need = 2 * nsel * rb
        assert s.lib.gph_engine_gene_trees_enable(s.engine, 2, None, 0, need - 1) == FULL
        with pytest.raises(MemoryError):
            s.enable_gene_trees(2, max_bytes=need - 1)
        s.initialize()                                 # the engine is still usable
        with pytest.raises(RuntimeError):
            s.sample_gene_trees(0)                     # the refused enable left the feature off
        s.enable_gene_trees(2, max_bytes=need)
        for it in range(2):
            s.iteration(it)
            s.sample_gene_trees(it)
        assert s.lib.gph_engine_gene_trees_sample(s.engine, 2) == FULL
        with pytest.raises(BufferError):
            s.sample_gene_trees(2)
        assert s._gene_trees_shape()[4] == 2
        two = s.gene_trees(raw=True)
        assert two["iters"].tolist() == [0, 1] and two["records"].shape == (2, nsel, rb)
        assert s._gene_trees_shape()[4] == 0
        s.iteration(2)
        s.sample_gene_trees(2)                         # a free row again
        s2 = G.Sampler(pk, lib=lib)                    # the refused sample changed nothing: the same chain, sampled at 2 only
        try:
            s2.enable_gene_trees(1)
            s2.initialize()
            for it in range(3):
                s2.iteration(it)
            s2.sample_gene_trees(2)
            want = s2.gene_trees(raw=True)
        finally:
            s2.close()
        one = s.gene_trees(raw=True)
        assert one["iters"].tolist() == [2] and one["records"].tobytes() == want["records"].tobytes()
        empty = s.gene_trees()
        assert empty["iters"].tolist() == [] and empty["age"].shape[0] == 0
        s.enable_gene_trees(0)
        with pytest.raises(RuntimeError):
            s.sample_gene_trees(4)
        with pytest.raises(RuntimeError):
            s.gene_trees()
    finally:
        s.close()


def test_capacity_limit_and_lifecycle(hostemu):
    import gphocs_amd as G
    check_capacity(hostemu[1], G)


# ---------------------------------------------------------------- the tree as text: hand-built records
def _newick(lib, n, age, father, left, right, npop, root, migs, pops=("A", "B", "AB"), bands=("A->B", "B->A"), labels=None):
    """migs: [(branch, band, age)] in `living` order"""
    import gphocs_amd as G
    mb = [m[0] for m in migs] + [-1] * (MIGS - len(migs))
    md = [m[1] for m in migs] + [-1] * (MIGS - len(migs))
    ma = [m[2] for m in migs] + [0.0] * (MIGS - len(migs))
    return G.gene_tree_newick(lib, age, father, left, right, npop, root, mb, md, ma, list(pops), list(bands),
                              list(labels or [f"s{i}.{i}" for i in range(n)]))


# three leaves, nodes 3 = (0, 1) at age 2, 4 = (3, 2) at age 5; leaf 2 is ancient (age 1)
T3 = dict(n=3, age=[0.0, 0.0, 1.0, 2.0, 5.0], father=[3, 3, 4, 4, -1], left=[-1, -1, -1, 0, 3], right=[-1, -1, -1, 1, 2],
          npop=[0, 0, 1, 0, 2], root=4)


def test_newick_of_hand_built_records(hostemu):
    lib = hostemu[1]
    # an ancient leaf: its branch is 5 - 1 = 4 long
    assert _newick(lib, migs=[], **T3) == "((s0.0[&pop=A]:2,s1.1[&pop=A]:2)[&pop=A]:3,s2.2[&pop=B]:4)[&pop=AB];"
    # two migrations of different bands on the branch of leaf 0, `living` order against their ages: ordered by age
    assert _newick(lib, migs=[(0, 1, 1.5), (0, 0, 0.5)], **T3) == \
        "((((s0.0[&pop=A]:0.5)[&mig=A->B]:1)[&mig=B->A]:0.5,s1.1[&pop=A]:2)[&pop=A]:3,s2.2[&pop=B]:4)[&pop=AB];"
    # two migrations of equal age: `living` order, a zero-length piece between them
    assert _newick(lib, migs=[(1, 1, 0.75), (1, 0, 0.75)], **T3) == \
        "((s0.0[&pop=A]:2,((s1.1[&pop=A]:0.75)[&mig=B->A]:0)[&mig=A->B]:1.25)[&pop=A]:3,s2.2[&pop=B]:4)[&pop=AB];"
    # one migration on a leaf's branch (the ancient leaf: 2.5 - 1 above it) and one on an internal branch
    assert _newick(lib, migs=[(3, 0, 4.0), (2, 1, 2.5)], **T3) == \
        "(((s0.0[&pop=A]:2,s1.1[&pop=A]:2)[&pop=A]:2)[&mig=A->B]:1,(s2.2[&pop=B]:1.5)[&mig=B->A]:2.5)[&pop=AB];"
    # lengths are %.10g of the fp64 difference
    third = dict(T3, age=[0.0, 0.0, 1.0, 1.0 / 3.0, 5.0])
    assert _newick(lib, migs=[], **third) == \
        "((s0.0[&pop=A]:0.3333333333,s1.1[&pop=A]:0.3333333333)[&pop=A]:4.666666667,s2.2[&pop=B]:4)[&pop=AB];"
    # a single leaf is a tree too
    assert _newick(lib, n=1, age=[0.0], father=[-1], left=[-1], right=[-1], npop=[1], root=0, migs=[]) == "s0.0[&pop=B];"
    for kw in (dict(pops=("a,b", "B", "AB")), dict(labels=["s0.0", "s 1.1", "s2.2"]), dict(pops=("A", "B", "A(B")), dict(labels=["s0.0", "x;y.1", "s2.2"]),
               dict(bands=("A->B", "B:A"))):
        with pytest.raises(ValueError):
            _newick(lib, migs=[], **T3, **kw)
    with pytest.raises(ValueError):                    # a record that is no tree: a father index beyond the nodes
        _newick(lib, migs=[], **dict(T3, left=[-1, -1, -1, 0, 9]))


# ---------------------------------------------------------------- the program and the launcher
def py_newick(t, s, q, n, pops, bands, labels):
    """the grammar of include/gphocs_hip.h restated over record (s, q) of Sampler.gene_trees()"""
    age, father, left, right, npop = (t[k][s, q].tolist() for k in ("age", "father", "left", "right", "npop"))
    root, nm = int(t["root"][s, q]), int(t["num_migs"][s, q])
    mbr, mband, mage = (t[k][s, q].tolist() for k in ("mig_branch", "mig_band", "mig_age"))

    def sub(v):
        text = (labels[v] if v < n else "(" + sub(left[v]) + "," + sub(right[v]) + ")") + f"[&pop={pops[npop[v]]}]"
        if v == root:
            return text
        a = age[v]
        for k in sorted((k for k in range(nm) if mbr[k] == v), key=lambda k: mage[k]):      # (sorted is stable: `living` order at equal ages)
            text = "(" + text + ":" + _fmt(mage[k] - a) + ")" + f"[&mig={bands[mband[k]]}]"
            a = mage[k]
        return text + ":" + _fmt(age[father[v]] - a)
    return sub(root) + ";"


def parse_newick(text):
    """the tree field back into nested dicts: kids, label (leaves), kind / val of the annotation, len"""
    pos = 0

    def node():
        nonlocal pos
        kids, label = [], None
        if text[pos] == "(":
            pos += 1
            while True:
                kids.append(node())
                m = re.match(r":([^,();\[\]]+)", text[pos:])
                kids[-1]["len"] = float(m.group(1))
                pos += m.end()
                pos += 1
                if text[pos - 1] == ")":
                    break
                assert text[pos - 1] == ","
        else:
            m = re.match(r"[^\[\]():,;]+", text[pos:])
            label, pos = m.group(0), pos + m.end()
        m = re.match(r"\[&(pop|mig)=([^\]]+)\]", text[pos:])
        pos += m.end()
        return dict(kids=kids, label=label, kind=m.group(1), val=m.group(2))
    top = node()
    assert text[pos:] == ";"
    return top


def check_parses_back(text, t, s, q, n, pops, bands):
    """the parsed tree is the record's: father array (through the leaf sets of the nodes), populations, migration bands"""
    father, left, right, npop = (t[k][s, q].tolist() for k in ("father", "left", "right", "npop"))
    root, nm = int(t["root"][s, q]), int(t["num_migs"][s, q])
    clade = {}

    def leaves(v):
        clade[v] = frozenset([v]) if v < n else leaves(left[v]) | leaves(right[v])
        return clade[v]
    leaves(root)
    node_of = {c: v for v, c in clade.items()}
    assert len(node_of) == 2 * n - 1
    seen = []

    def walk(nd, parent):
        migs = []
        while nd["kind"] == "mig":                 # outermost = oldest
            assert len(nd["kids"]) == 1
            migs.append(nd["val"])
            nd = nd["kids"][0]
        got = walk_body(nd)
        v = node_of[got]
        seen.append(v)
        assert father[v] == parent_id(parent) and pops[npop[v]] == nd["val"]
        on = sorted((k for k in range(nm) if t["mig_branch"][s, q, k] == v), key=lambda k: t["mig_age"][s, q, k])
        assert migs[::-1] == [bands[t["mig_band"][s, q, k]] for k in on]
        return got

    def walk_body(nd):
        if nd["label"] is not None:
            return frozenset([int(nd["label"].rsplit(".", 1)[1])])
        assert len(nd["kids"]) == 2
        mine = frozenset().union(*[_below(k) for k in nd["kids"]])
        for k in nd["kids"]:
            walk(k, mine)
        return mine

    def _below(nd):
        while nd["kind"] == "mig":
            nd = nd["kids"][0]
        return frozenset([int(nd["label"].rsplit(".", 1)[1])]) if nd["label"] is not None else frozenset().union(*[_below(k) for k in nd["kids"]])

    def parent_id(c):
        return -1 if c is None else node_of[c]
    top = parse_newick(text)
    assert top["kind"] == "pop"
    walk(top, None)
    assert sorted(seen) == list(range(2 * n - 1))


def program_ctl(name=PROGRAM_CASE, edit=None):
    txt = open(os.path.join(GOLDEN, name + ".ctl")).read()
    txt, k = re.subn(r"mcmc-iterations\s+\d+", "mcmc-iterations\t  40\n\tburn-in 7\n\tmcmc-sample-skip 2", txt)
    assert k == 1
    return edit(txt) if edit else txt


def expected_tsv(ctl_dir, ctl, spec_loci, lib=None, sampler_lib=None):
    """the text of PREFIX.trees.tsv the program must write: an equivalent Sampler run (burn-in first, a sample wherever a
    trace line is written), the grammar restated in Python over its decoded records"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.enable_gene_trees(p.numSamplesMcmc, spec_loci)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.sample_gene_trees(it)
        t = s.gene_trees()
    finally:
        s.close()
    n, B = p.n, p.B
    pops = _pop_names(os.path.join(ctl_dir, ctl))
    names = printed_names(p.sampleNames)
    labels = [f"{names[i]}.{i}" for i in range(n)]
    bands = [f"{pops[p.bandSrc[b]]}->{pops[p.bandTgt[b]]}" for b in range(B)]
    lines = ["\t".join(["iter", "locus", "name", "dataLnL", "genLnL", "tmrca", "numMigs", "tree"])]
    for s_, it in enumerate(t["iters"].tolist()):
        for q, g in enumerate(t["loci"].tolist()):
            root = int(t["root"][s_, q])
            lines.append("\t".join([str(it), str(g), p.locusNames[g], _fmt(t["dataLnL"][s_, q]), _fmt(t["genLnL"][s_, q]), _fmt(t["age"][s_, q, root]),
                                    str(int(t["num_migs"][s_, q])), py_newick(t, s_, q, n, pops, bands, labels)]))
    return "\n".join(lines) + "\n", t, p, (pops, bands)


def check_program(lib_path, lib, tmp_path, name=PROGRAM_CASE):
    """item 7: the file is the restated grammar over an equivalent Sampler run, character for character, and parses back;
    the other options' files do not change; the usage errors"""
    a, b, d, e = (tmp_path / x for x in ("with", "without", "all", "rest"))
    for x in (a, b, d, e):
        _copy_case(name, x, program_ctl(name))
    ctl = name + ".ctl"
    _run(lib_path, a, ["--gene-trees", "out", "--gene-trees-loci", PROGRAM_SPEC, "--gene-trees-rows", "5", ctl])      # (14 samples: three flushes)
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    want, t, p, (pops, bands) = expected_tsv(str(a), ctl, PROGRAM_LOCI, lib, lib)
    assert sorted(got) == ["trees.tsv"]                              # no part left behind
    assert got["trees.tsv"].splitlines()[0] == want.splitlines()[0]
    assert got["trees.tsv"] == want
    rows = [ln.split("\t") for ln in got["trees.tsv"].splitlines()[1:]]
    its = [int(ln.split("\t")[0]) for ln in open(trace).read().splitlines()[1:]]
    assert [(int(r[0]), int(r[1])) for r in rows] == [(it, g) for it in its for g in PROGRAM_LOCI] and len(its) == 14
    seq_names = _locus_names(a / (name + ".seq"))
    assert all(r[2] == seq_names[int(r[1])] for r in rows)
    for k, r in enumerate(rows):
        check_parses_back(r[7], t, k // len(PROGRAM_LOCI), k % len(PROGRAM_LOCI), p.n, pops, bands)
    _run(lib_path, d, ["--gene-trees", "out", "--gene-trees-loci", PROGRAM_SPEC, "-l", "sum.tsv", "-s", "cs", "--time-slices", "4", "--ancestry", "an", ctl])
    _run(lib_path, e, ["-l", "sum.tsv", "-s", "cs", "--time-slices", "4", "--ancestry", "an", ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    rest = read_outputs(e, "cs")
    assert len(rest) == 2 + 3 * p.K and read_outputs(d, "cs") == rest
    assert sorted(read_outputs(e, "an")) == ["loci.tsv", "samples.tsv"] and read_outputs(d, "an") == read_outputs(e, "an")
    assert open(d / (name + ".trace")).read() == open(trace).read()
    # usage errors: before any iteration, nothing written
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    for args, word in ((["--gene-trees-loci", "0-3"], "--gene-trees"), (["--gene-trees-rows", "4"], "--gene-trees"),
                       (["--gene-trees", "out", "--gene-trees-loci", "0-4,3"], "locus 3 "), (["--gene-trees", "out", "--gene-trees-loci", "5,5"], "locus 5 "),
                       (["--gene-trees", "out", "--gene-trees-loci", f"3,{p.L}"], f"locus {p.L} "), (["--gene-trees", "out", "--gene-trees-loci", "0-30:4"], f"locus {(p.L + 3) // 4 * 4} "),
                       (["--gene-trees", "out", "--gene-trees-loci", "2-x"], "2-x"), (["--gene-trees", "out", "--gene-trees-rows", "0"], "usage")):
        r = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    # a name that cannot stand in a tree: refused with --gene-trees before the first iteration, nothing changes without
    for k, edit in enumerate((lambda x: re.sub(r"(\bsamples\s+)s0\b", r"\1A=1", x, count=1),)):
        v = tmp_path / f"name{k}"
        _copy_case(name, v, program_ctl(name, edit))
        seq, count = re.subn(r"(?m)^s0(\s)", r"A=1\1", open(v / (name + ".seq")).read())      # (the sequence file names its samples too)
        assert count == p.L
        open(v / (name + ".seq"), "w").write(seq)
        r = subprocess.run([EXE, "--gene-trees", "out", ctl], cwd=v, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0 and "cannot stand in a tree" in r.stderr and "A=1" in r.stderr
        assert sorted(os.listdir(v)) == sorted([ctl, name + ".seq"])
        _run(lib_path, v, [ctl])
        assert len(open(v / (name + ".trace")).read().splitlines()) == 15


def test_program_writes_the_trees_file(hostemu, tmp_path):
    path, lib = hostemu
    check_program(path, lib, tmp_path)


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """item 9: a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.trees.tsv must be
    written: status non-zero, no part and no file of ours left, for one rank and for two; and the job that fails before it
    starts (more ranks than loci)"""
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.trees.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--gene-trees", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.trees.tsv"] and not os.listdir(d / "out.trees.tsv")
    d = tmp_path / "z"
    _copy_case("z0", d)
    nloci = int(open(os.path.join(GOLDEN, "z0.seq")).read().split()[0])
    r = subprocess.run([EXE, "-g", str(min(nloci * 2 + 1, 40)), "--gene-trees", "out", "z0.ctl"], cwd=d, capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode != 0
    assert not [f for f in os.listdir(d) if f.startswith("out.")]


def test_failed_run_leaves_no_trees_file(hostemu, tmp_path):
    check_failed_runs_leave_nothing(hostemu[0], tmp_path)


# ---------------------------------------------------------------- ranks
def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """item 8: two ranks' parts, written into the file by gph_gene_trees_write, are the one-rank file -- for all loci, and
    for a selection that lies wholly in rank 1's block (rank 0 holds no selected locus); the launcher does the same; a part
    cut short or missing is refused and nothing is left"""
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, gene_trees="out", gene_trees_loci=spec, gene_trees_rows=7)
        assert pk.L == 16
        want = read_outputs(one, "out")                              # one rank writes its file itself (a communicator of one included)
        assert sorted(want) == ["trees.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        rows = [ln.split("\t") for ln in want["trees.tsv"].splitlines()[1:]]
        assert [(int(r[0]), int(r[1])) for r in rows] == [(it, g) for it in range(GOLDEN_ITERS[name]) for g in loci]
        run_ranks(lib_path, name, 2, two, gene_trees="out", gene_trees_loci=spec, gene_trees_rows=7)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.trees.part0", "out.trees.part1"]
        if spec is not None:                                         # rank 0's part: a header, 120 iterations, no record
            b0 = open(two / "out.trees.part0", "rb").read()
            assert b0[:8] == b"GPHGT1\n\0" and int.from_bytes(b0[8 + 4 * 12:8 + 4 * 12 + 8], "little") == 0
            assert int.from_bytes(b0[-8:], "little") == GOLDEN_ITERS[name]
        if spec is None:
            # a part that was not closed by its rank, and a part that is missing: refused, and nothing is left
            for kind in ("cut", "gone"):
                d = tmp_path / kind
                os.makedirs(d)
                for r in range(2):
                    shutil.copy(two / f"out.trees.part{r}", d)
                if kind == "cut":
                    b = open(d / "out.trees.part1", "rb").read()
                    open(d / "out.trees.part1", "wb").write(b[:-8])
                else:
                    os.unlink(d / "out.trees.part0")
                assert lib.gph_gene_trees_write(str(d / "out").encode(), 2) != 0
                assert not read_outputs(d, "out")
        assert lib.gph_gene_trees_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                      # no part among them: written once
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--gene-trees", "out", "--gene-trees-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def test_ranks_concatenate_to_the_one_rank_file(hostemu, tmp_path):
    path, lib = hostemu
    check_ranks(path, lib, tmp_path)
