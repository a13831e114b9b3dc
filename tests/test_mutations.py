"""Expected substitutions per population branch and per sample (gph_engine_mutations_*) on the CPU.

A  The formulas apart from their restatement: hand-made packs of 3 .. 5 leaves (a code-4 leaf, a two-phase column, an all-N
   column, a zero-length branch) through the float model of tests/mutations_util.py and through an enumeration of every assignment
   of bases to the internal nodes in decimal at 50 digits, with E_same / E_diff from the uniformisation series -- compared by
   relative difference in M_v under REL_BOUND (64 x the largest value observed, mutations_util.py), with the two per-locus sums.
B  The kernel against the float model, bit for bit: the host-emulation build runs k_mutations' text over the same pages; one chain
   samples its gene trees, its population ages and the accumulators after every iteration, the model's inside pass is held to every
   record's dataLnL as float.hex, then accumulators and rows are compared as float.hex after 1, 2 and 9 samples.  Goldens m3, j1,
   a7, v8, stress, p7, bigp, x8; n7 (loci 0-1) and q6 (locus 0) on the host build with the reference's own caps; a synthetic pack
   whose columns end on, before and behind a tile edge; a pack with a locus whose every branch has u == 0; t136 (136 leaves: no
   segment lists); selections with a partial chunk, one locus, the last locus.
C  Refusals, reset, limits, the chain untouched, host synchronisations unchanged.
D  The program: both files against Sampler output, the "#" lines against the file's own rows, the other outputs unmoved, two ranks
   against the rank-order sum of their parts, a part cut short, usage errors, a late failure."""
import os
import sys
from decimal import Decimal

import pytest

from conftest import GOLDEN, REPO
from sampler_util import hostemu_library
from test_ancestry import GOLDEN_ITERS
import mutations_util as M

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


@pytest.fixture(scope="module")
def hostemu_big():
    import run_hostemu
    import gphocs_amd as G
    return G.load_library(run_hostemu.build_hostemu(big=True))


# ---------------------------------------------------------------- A: the formulas, against the enumeration
CODE = {"T": 0, "C": 1, "A": 2, "G": 3, "N": 4}


def rows_of(columns):
    """columns: ([codes string of every phase], count) -> (codes, phase words, counts)"""
    codes, words, counts = [], [], []
    for phases, count in columns:
        for k, c in enumerate(phases):
            codes.append([CODE[ch] for ch in c])
            words.append(len(phases) if k == 0 else 0)
            counts.append(count if k == 0 else 0)
    return codes, words, counts


def tree(n, pairs, ages):
    """internal node n + k joins pairs[k]; the last one is the root"""
    N = 2 * n - 1
    father, left, right = [-1] * N, [-1] * N, [-1] * N
    for k, (a, b) in enumerate(pairs):
        left[n + k], right[n + k] = a, b
        father[a] = father[b] = n + k
    return father, left, right, [0.0] * n + list(ages), N - 1


# populations: 0, 1 current, 2 = their father; K = 3
POPS = dict(popAge=[0.0, 0.0, 0.004], popFather=[2, 2, -1], bandSrc=[1])
HAND = {
    # three leaves, one of them missing in two columns
    "code4": dict(n=3, tree=tree(3, [(0, 1), (3, 2)], [0.003, 0.009]), npop=[0, 0, 1, 0, 2], migs=[], rate=1.0,
                  cols=[(["TTN"], 5), (["TCN"], 2), (["TCA"], 1), (["NTT"], 3), (["TTT"], 40)]),
    # four leaves, a column of two phases, a migration on the branch above leaf 2 (band 0: source population 1), rate 1.7
    "twophase": dict(n=4, tree=tree(4, [(0, 1), (2, 3), (4, 5)], [0.002, 0.0055, 0.012]), npop=[0, 0, 0, 1, 0, 2, 2], migs=[(2, 0, 0.001)], rate=1.7,
                     cols=[(["TTTT"], 30), (["TCTT", "TTCT"], 2), (["TTCC"], 3), (["ATCC", "TACC"], 1), (["GGGT"], 1)]),
    # five leaves, an all-N column among others
    "allN": dict(n=5, tree=tree(5, [(0, 1), (2, 5), (3, 4), (6, 7)], [0.001, 0.0045, 0.002, 0.02]), npop=[0, 0, 0, 1, 1, 0, 2, 1, 2], migs=[], rate=0.6,
                 cols=[(["NNNNN"], 7), (["TTTCC"], 2), (["TCTTT"], 1), (["TTTTT"], 25)]),
    # the all-N column alone: M_v is the prior's rate t_v count
    "onlyN": dict(n=3, tree=tree(3, [(0, 1), (3, 2)], [0.003, 0.009]), npop=[0, 0, 1, 0, 2], migs=[], rate=1.3, cols=[(["NNN"], 11)]),
    # a zero-length branch: node 3 at the age of leaf 1, which is an ancient sample at 0.002 -- and leaf 1's own branch has u == 0
    "zero": dict(n=3, tree=(lambda f: (f[0], f[1], f[2], [0.0, 0.002, 0.0, 0.002, 0.009], f[4]))(tree(3, [(0, 1), (3, 2)], [0.002, 0.009])),
                 npop=[0, 0, 1, 0, 2], migs=[], rate=1.0, cols=[(["TCA"], 2), (["TTT"], 9), (["CTT"], 1)]),
}


def hand(name):
    h = HAND[name]
    father, left, right, age, root = h["tree"]
    rows = rows_of(h["cols"])
    v = M.locus_sample(h["n"], 3, father, left, right, h["npop"], age, root, h["migs"], h["rate"], rows, POPS["popAge"], POPS["popFather"], POPS["bandSrc"])
    return h, (father, left, right, age, root), rows, v


@pytest.mark.parametrize("name", sorted(HAND))
def test_float_model_equals_the_enumeration(name):
    """M_v of every branch, sum_p mut_p = sum_v M_v and sum_p exp_p = rate sites tree length, all under REL_BOUND"""
    h, (father, left, right, age, root), rows, v = hand(name)
    want, sites = M.enumerate_locus(h["n"], father, left, right, age, root, h["rate"], rows)
    assert v["sites"] == float(sites)
    worst = Decimal(0)
    for c in range(2 * h["n"] - 1):
        if c == root:
            continue
        d = M.rel(v["M"][c], want[c])
        worst = max(worst, d)
        print(f"{name} branch {c}: M {v['M'][c]!r} enumeration {float(want[c])!r} rel {float(d):.3g}")
        assert d <= Decimal(M.REL_BOUND), (name, c, v["M"][c], want[c])
    total, length = sum(want), sum(Decimal(age[father[c]]) - Decimal(age[c]) for c in range(2 * h["n"] - 1) if c != root and v["E"][c] is not None)
    d1 = M.rel(sum(Decimal(x) for x in v["mut"]), sum(Decimal(x) for x in v["M"]))
    d2 = M.rel(sum(Decimal(x) for x in v["exp"]), Decimal(h["rate"]) * sites * length)
    d3 = M.rel(sum(Decimal(x) for x in v["mut"]), total)
    print(f"{name}: worst M_v {float(worst):.3g}, sum mut vs sum M {float(d1):.3g}, sum exp vs rate sites length {float(d2):.3g}, sum mut vs enumeration {float(d3):.3g}")
    assert d1 <= Decimal(M.REL_BOUND) and d2 <= Decimal(M.REL_BOUND) and d3 <= Decimal(M.REL_BOUND)


def test_all_missing_column_gives_the_prior():
    """an all-N column: M_v = rate t_v count for every branch, the leaves' terminal branches included"""
    h, (father, left, right, age, root), rows, v = hand("onlyN")
    for c in range(4):
        want = Decimal(h["rate"]) * (Decimal(age[father[c]]) - Decimal(age[c])) * 11
        assert M.rel(v["M"][c], want) <= Decimal(M.REL_BOUND)
    assert [M.rel(v["mutExt"][i], Decimal(v["expExt"][i])) <= Decimal(M.REL_BOUND) for i in range(3)] == [True] * 3


def test_zero_length_branch_contributes_nothing():
    h, (father, left, right, age, root), rows, v = hand("zero")
    assert v["M"][1] == 0.0 and v["E"][1] is None and v["mutExt"][1] == 0.0 and v["expExt"][1] == 0.0
    assert v["M"][0] > 0.0 and v["M"][3] > 0.0


def test_segments_follow_populations_and_migrations():
    """leaf 2 of `twophase`: population 0 up to the migration at 0.001, the band's source population 1 up to tau 0.004, then 2"""
    h, (father, left, right, age, root), _, _ = hand("twophase")
    seg = M.segments(2, father[2], age, h["npop"], h["migs"], POPS["popAge"], POPS["popFather"], POPS["bandSrc"])
    assert [p for p, _ in seg] == [0, 1, 2] and [dt for _, dt in seg] == [0.001, 0.004 - 0.001, 0.0055 - 0.004]
    seg = M.segments(4, father[4], age, h["npop"], h["migs"], POPS["popAge"], POPS["popFather"], POPS["bandSrc"])
    assert [p for p, _ in seg] == [0, 2]


def test_series_matches_the_closed_forms():
    """the uniformisation series against the closed forms the header states, in decimal"""
    for ln in (Decimal("0.0004"), Decimal("0.03"), Decimal("0.9")):
        a = 4 * ln / 3
        u = 1 - (-a).exp()
        qe = 1 - u
        Es, Ed = M.series_expectations(a, terms=120)
        assert abs(Ed - (a * qe / u + Decimal("0.75") * a)) < Decimal("1e-40") and abs(Es - Decimal("0.75") * a * u / (1 + 3 * qe)) < Decimal("1e-40")


# ---------------------------------------------------------------- B: the kernel against the float model, bit for bit
@pytest.mark.parametrize("name", ["m3", "j1", "a7", "v8", "stress", "bigp", "x8"])
def test_accumulators_and_rows_equal_the_model(hostemu, name):
    r = M.check_case(hostemu[1], name, loci=M.STRESS_LOCI if name == "stress" else None)
    t, pk = r["trees"], r["pack"]
    if name in ("m3", "j1"):
        assert int(t["num_migs"].sum()) > 0, "no live migration in any record"
    if name in ("j1", "x8"):
        assert r["maxseg"] > M.SEGS, "no branch with more segments than a list holds: the second walk never ran"
    if name == "m3":
        assert 1 < r["maxseg"] <= M.SEGS
    if name == "a7":
        assert (t["age"][:, :, :pk.n] > 0).any(), "no leaf above age 0"
    if name == "v8":
        assert len(set(r["rates"].reshape(-1).tolist())) > 1, "one rate only"
    if name == "stress":
        assert pk.n == 13
    if name == "bigp":
        assert max(int(pk.pattern_offsets[g + 1] - pk.pattern_offsets[g]) for g in range(pk.L)) > 64
    if name == "x8":
        assert pk.n == 32


def test_a_column_of_64_phases(hostemu, tmp_path):
    import shutil
    import gphocs_amd as G
    for ext in (".ctl", ".seq"):
        shutil.copy(os.path.join(GOLDEN, "p7" + ext), tmp_path)
    pk = G.Pack.from_control(os.path.join(tmp_path, "p7.ctl"), lib=hostemu[1], seq_path=os.path.join(tmp_path, "p7.seq"))
    assert max(M.phases_of(w) for w in pk.numPhases) == 64
    M.check_case(hostemu[1], "p7", pack=pk)


def test_72_leaves(hostemu_big):
    r = M.check_case(hostemu_big, "n7", loci=[0, 1])
    assert r["pack"].n == 72


def test_a_block_that_stays_in_hbm(hostemu_big):
    r = M.check_case(hostemu_big, "q6", loci=[0], iters=3)
    assert r["pack"].n == 72 and int(r["pack"].pattern_offsets[1]) > 64


def test_136_leaves_without_segment_lists(hostemu_big):
    """from about 120 leaves on the segment lists no longer fit next to a tile: every population lane walks every branch"""
    r = M.check_case(hostemu_big, "t136", iters=2, checkpoints=(1,))
    assert r["pack"].n == 136


def test_zero_length_branches(hostemu, tmp_path):
    from predictive_util import edge_model
    M.check_zero_length_branches(hostemu[1], edge_model(tmp_path, hostemu[1]))


def test_columns_at_the_tile_edges(hostemu, tmp_path):
    from predictive_util import edge_model
    M.check_tile_edges(hostemu[1], edge_model(tmp_path, hostemu[1]))


def test_selections_and_partial_chunks(hostemu):
    M.check_selections(hostemu[1])


# ---------------------------------------------------------------- C: refusals, limits, the chain untouched
def test_refusals_name_the_cause_and_touch_nothing(hostemu, capfd):
    M.check_refusals(hostemu[1], capfd)


def test_reset_limits_and_lifecycle(hostemu):
    import gphocs_amd as G
    M.check_lifecycle(hostemu[1], G)


@pytest.mark.parametrize("name", ["m3", "x8"])
def test_sampling_leaves_the_chain_unchanged(hostemu, tmp_path, name):
    on, off = M.check_chain_untouched(hostemu[1], name, GOLDEN_ITERS[name], tmp_path)
    (s0, s1), (n0, n1) = on["stats"], off["stats"]
    assert s1["syncs"] - s0["syncs"] == n1["syncs"] - n0["syncs"]
    assert s1["collectives"] - s0["collectives"] == n1["collectives"] - n0["collectives"]
    assert s1["resident"] == n1["resident"]


# ---------------------------------------------------------------- D: the program and the launcher
def test_program_writes_the_two_mutations_files(hostemu, tmp_path):
    path, lib = hostemu
    M.check_program(path, lib, tmp_path)


def test_ranks_join_to_the_rank_order_sum(hostemu, tmp_path):
    path, lib = hostemu
    M.check_ranks(path, lib, tmp_path)


def test_failed_run_leaves_no_mutations_files(hostemu, tmp_path):
    M.check_failed_runs_leave_nothing(hostemu[0], tmp_path)
