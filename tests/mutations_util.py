"""What tests/test_mutations.py (host-emulation build) and tests/test_mutations_gpu.py (-m gpu, the product libraries) share.

Two models of include/gphocs_hip.h's expected substitutions, neither of which calls the library to compute what it checks:

  float model   the header's definition restated in plain Python floats, operation by operation (locus_sample).  It works from a
                gene-tree record, the locus rate, the population ages of the chain state, the model and the pack; it recomputes the
                inside conditionals with child_factor's arithmetic and holds them to the record's dataLnL first.  The kernel is
                compared with it as float.hex: accumulators and per-sample rows, nothing has a tolerance.
  enumeration   the posterior mass of "the ends of the branch differ" by enumerating every assignment of bases to the internal
                nodes in `decimal` at 50 digits, and E_same / E_diff from the uniformisation series sum_m Poisson(m) E[changes | m,
                ends] (a dynamic programme over the jump chain, not the closed forms).  The float model is compared with it by
                relative difference in M_v.

REL_BOUND.  Nobody had measured the float model against the enumeration.  Measured on the host over the hand-made packs of
test_mutations.py (3 .. 5 leaves; a code-4 leaf, a two-phase column, an all-N column, a zero-length branch):
  OBSERVED_REL = 1.19e-14, the largest relative difference in M_v of any branch (`allN`, the branch above leaf 1: rate t = 6e-4,
  where u = 1 - exp(-a) -- the likelihood's own edge_prob -- loses log2(1 / a) bits to cancellation); the other packs stay below
  4.2e-15, sum_p mut_p against sum_v M_v and sum_p exp_p against rate sites length below 1.1e-16
and the tests assert 64 x that, a margin for other packs and libm-free reorderings.  Far below 1e-10: nothing to explain."""
import ctypes
import math
import os
from decimal import Decimal, getcontext

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import compare_records
from sampler_util import load_pack

CLS = 24                # timing class of k_mutations (with its fold)
FULL, EARG, ESTATE = -5, -1, -4
CHECKPOINTS = (1, 2)
TILE = 32               # GPH_MU_TILE: the rows of a tile at most (csrc/gph_mutations.h)
SEGS = 4                # GPH_MU_SEGS: the segments a branch's list holds; a branch with more is walked again
CHUNK = 64              # GPH_MU_CHUNK: the selected loci a partial row sums (csrc/gph_mutations.h); _shape reports it
OBSERVED_REL = 1.19e-14
REL_BOUND = 64 * OBSERVED_REL
GT_O_DATALNL = 3
STRESS_LOCI = list(range(0, 40, 3))     # golden stress has 40 loci; every third keeps the model's share of the test to a second or two


# ---------------------------------------------------------------- the pack as the definitions see it
def phases_of(word):
    w = int(word)
    return w if w < 0x8000 else 1 << (w & 31)


def locus_rows(pack, g):
    """(codes [P][n], phase words [P], counts [P]) of locus g, rows in block order"""
    r0, r1 = int(pack.pattern_offsets[g]), int(pack.pattern_offsets[g + 1])
    return (pack.leafcodes[r0:r1].astype(int).tolist(), [int(w) for w in pack.numPhases[r0:r1]], [int(c) for c in pack.counts[r0:r1]])


def columns_of(words):
    """[(first row, rows)] of every column"""
    out = []
    for r, w in enumerate(words):
        if w != 0:
            out.append([r, 1])
        else:
            out[-1][1] += 1
    return [tuple(c) for c in out]


# ---------------------------------------------------------------- the float model: the header restated
def edge(rate, t):
    """(len, a, u, pe, qe) of a branch of duration t"""
    ln = rate * t
    a = 4 * ln / 3.0
    u = 0.0 if ln < 1e-100 else 1 - math.exp(-4 * ln / 3.0)
    pe = u / 4.0
    return ln, a, u, pe, 1 - 4.0 * pe


def leaf_vector(code):
    return [1.0 if code == 4 or code == x else 0.0 for x in range(4)]


def factor(i, pe, qe):
    S = 0.0
    S += i[0]
    S += i[1]
    S += i[2]
    S += i[3]
    if S >= 4:
        return [1.0, 1.0, 1.0, 1.0]
    Sp = S * pe
    return [Sp + i[x] * qe for x in range(4)]


def inside(n, left, right, root, pe, qe, codes):
    """I_v of every node at one row, bottom up: child_factor's arithmetic, v = (1.0 * f_l) * f_r"""
    I = [leaf_vector(codes[i]) for i in range(n)] + [None] * (n - 1)

    def rec(v):
        if I[v] is None:
            fl, fr = factor(rec(left[v]), pe[left[v]], qe[left[v]]), factor(rec(right[v]), pe[right[v]], qe[right[v]])
            I[v] = [(1.0 * fl[x]) * fr[x] for x in range(4)]
        return I[v]
    rec(root)
    return I


def down(O, fs, ic, pe, qe):
    U = [O[x] * fs[x] for x in range(4)]
    SU = ((U[0] + U[1]) + U[2]) + U[3]
    pS = pe * SU
    o = [pS + qe * U[x] for x in range(4)]
    J = [(ic[1] + ic[2]) + ic[3], (ic[0] + ic[2]) + ic[3], (ic[0] + ic[1]) + ic[3], (ic[0] + ic[1]) + ic[2]]
    return pe * (((U[0] * J[0] + U[1] * J[1]) + U[2] * J[2]) + U[3] * J[3]), o


def row_masses(n, left, right, root, pe, qe, I):
    """D_c of every branch at one row (top down), and R"""
    N = 2 * n - 1
    D, O = [0.0] * N, [None] * N
    O[root] = [1.0] * 4
    todo = [root]
    while todo:
        v = todo.pop()
        l, r = left[v], right[v]
        fl, fr = factor(I[l], pe[l], qe[l]), factor(I[r], pe[r], qe[r])
        D[l], O[l] = down(O[v], fr, I[l], pe[l], qe[l])
        D[r], O[r] = down(O[v], fl, I[r], pe[r], qe[r])
        todo += [c for c in (l, r) if c >= n]
    rc = I[root]
    return D, ((rc[0] + rc[1]) + rc[2]) + rc[3]


def segments(v, f, age, npop, migs, popAge, popFather, bandSrc):
    """[(population, dt)] of the branch above v in time order; migs: (branch, band, age) in `living` order"""
    cur, t, out = npop[v], age[v], []
    events = sorted((m[2], k) for k, m in enumerate(migs) if m[0] == v)
    for b, k in events + [(age[f], -1)]:
        while popFather[cur] >= 0 and popAge[popFather[cur]] <= b:
            F = popFather[cur]
            out.append((cur, popAge[F] - t))
            cur, t = F, popAge[F]
        out.append((cur, b - t))
        t = b
        if k >= 0:
            cur = bandSrc[migs[k][1]]
    return out


def locus_sample(n, K, father, left, right, npop, age, root, migs, rate, rows, popAge, popFather, bandSrc):
    """one locus at one sample -> dict(M [N], mut [K], exp [K], mutExt [n], expExt [n], sites, lnl (the likelihood's own root sum),
    lnl_rr (the sum over log(RR / (4 ph)) count), Dv [N], E [N] (E_same, E_diff))"""
    codes, words, counts = rows
    N, P = 2 * n - 1, len(codes)
    pe, qe, ed = [0.0] * N, [1.0] * N, [None] * N
    for v in range(N):
        if v != root:
            ed[v] = edge(rate, age[father[v]] - age[v])
            pe[v], qe[v] = ed[v][3], ed[v][4]
    D, R, Is = [], [], []
    for r in range(P):
        I = inside(n, left, right, root, pe, qe, codes[r])
        d, rr = row_masses(n, left, right, root, pe, qe, I)
        D.append(d)
        R.append(rr)
        Is.append(I[root])
    cols = columns_of(words)
    sites = float(sum(counts[r0] for r0, _ in cols))
    lnl = lnl_rr = 0.0
    for r0, k in cols:
        prob = 0.0
        for r in range(r0, r0 + k):
            for x in range(4):
                prob += Is[r][x]
        ph = phases_of(words[r0])
        assert ph == k
        lnl += math.log(prob / (4 * ph)) * counts[r0]
        RR = 0.0
        for r in range(r0, r0 + k):
            RR = RR + R[r]
        lnl_rr += math.log(RR / (4 * ph)) * counts[r0]
    M, Dvs, Es = [0.0] * N, [0.0] * N, [None] * N
    for v in range(N):
        if v == root or ed[v][2] == 0.0:
            continue
        Dv = 0.0
        for r0, k in cols:
            DD = RR = 0.0
            for r in range(r0, r0 + k):
                DD = DD + D[r][v]
                RR = RR + R[r]
            d = 0.0 if RR == 0.0 else DD / RR
            Dv = Dv + float(counts[r0]) * d
        _, a, u, _, q = ed[v]
        Ediff = (a * q) / u + 0.75 * a
        Esame = ((0.75 * a) * u) / (1 + 3 * q)
        M[v] = Esame * (sites - Dv) + Ediff * Dv
        Dvs[v], Es[v] = Dv, (Esame, Ediff)
    mut, ex = [0.0] * K, [0.0] * K
    maxseg = 0
    for v in range(N):
        if v == root or ed[v][2] == 0.0:
            continue
        tv = age[father[v]] - age[v]
        maxseg = max(maxseg, len(segments(v, father[v], age, npop, migs, popAge, popFather, bandSrc)))
        for p, dt in segments(v, father[v], age, npop, migs, popAge, popFather, bandSrc):
            mut[p] = mut[p] + M[v] * (dt / tv)
            ex[p] = ex[p] + (rate * dt) * sites
    mutExt = [M[i] for i in range(n)]
    expExt = [(rate * (age[father[i]] - age[i])) * sites for i in range(n)]
    return dict(M=M, mut=mut, exp=ex, mutExt=mutExt, expExt=expExt, sites=sites, lnl=lnl, lnl_rr=lnl_rr, Dv=Dvs, E=Es, maxseg=maxseg)


# ---------------------------------------------------------------- the enumeration, in decimal
def series_expectations(a, terms=80):
    """(E_same, E_diff) of a JC69 branch with uniformisation rate a (4 len / 3: every event draws one of the four bases) from
    sum_m Poisson(m; a) E[changes | m, ends]: A_m[z] = P(X_m = z), C_m[z] = E[changes; X_m = z] by recursion over the jump chain"""
    getcontext().prec = 50
    a = Decimal(a)
    A, Cc = [Decimal(1), Decimal(0), Decimal(0), Decimal(0)], [Decimal(0)] * 4
    pois = (-a).exp()
    num, den = [Decimal(0)] * 4, [Decimal(0)] * 4
    for m in range(terms):
        for z in range(4):
            num[z] += pois * Cc[z]
            den[z] += pois * A[z]
        A, Cc = ([sum(A) / 4 for _ in range(4)],
                 [sum(Cc[w] + (A[w] if w != z else 0) for w in range(4)) / 4 for z in range(4)])
        pois = pois * a / (m + 1)
    return num[0] / den[0], num[1] / den[1]


def enumerate_locus(n, father, left, right, age, root, rate, rows):
    """M_v [N] in decimal: the mass of differing ends by enumerating the bases of the internal nodes, E from the series"""
    getcontext().prec = 50
    from itertools import product
    codes, words, counts = rows
    N = 2 * n - 1
    inner = list(range(n, N))
    pd = [None] * N                               # P(a given other base at the top | base at the bottom)
    for v in range(N):
        if v != root:
            ln = Decimal(rate) * (Decimal(age[father[v]]) - Decimal(age[v]))
            pd[v] = (1 - (-4 * ln / 3).exp()) / 4 if ln > 0 else Decimal(0)
    cols = columns_of(words)
    sites = sum(counts[r0] for r0, _ in cols)
    out = [Decimal(0)] * N
    Dv = [Decimal(0)] * N
    for r0, k in cols:
        tot, diff = Decimal(0), [Decimal(0)] * N
        for r in range(r0, r0 + k):
            options = [range(4) if codes[r][i] == 4 else (codes[r][i],) for i in range(n)] + [range(4)] * (n - 1)
            for base in product(*options):
                w = Decimal(1) / 4
                for v in range(N):
                    if v != root:
                        w *= pd[v] if base[v] != base[father[v]] else 1 - 3 * pd[v]
                tot += w
                for v in range(N):
                    if v != root and base[v] != base[father[v]]:
                        diff[v] += w
        for v in range(N):
            if v != root:
                Dv[v] += counts[r0] * diff[v] / tot
    for v in range(N):
        if v == root or pd[v] == 0:
            continue
        ln = Decimal(rate) * (Decimal(age[father[v]]) - Decimal(age[v]))
        Es, Ed = series_expectations(4 * ln / 3)
        out[v] = Es * (sites - Dv[v]) + Ed * Dv[v]
    return out, sites


def rel(got, want):
    want = Decimal(want)
    if want == 0:
        return Decimal(0) if Decimal(got) == 0 else Decimal("Infinity")
    return abs(Decimal(got) - want) / abs(want)


# ---------------------------------------------------------------- one chain, sampled
def run_chain(lib, name, iters, loci=None, checkpoints=(), sample=True, trees=True, record=None, final=None, pack=None):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees, the chain's population
    ages and a mutations sample after every iteration; Sampler.mutations() is fetched (no reset) after each of `checkpoints`
    samples and at the end, the rows at the end"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.mutations_enable(iters, loci)
        s.initialize()
        hs0 = s.host_stats()
        at, pop_ages = {}, []
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                    pop_ages.append([float(x) for x in s.state()["popAge"]])
                s.mutations_sample(it)
                if it + 1 in checkpoints:
                    at[it + 1] = s.mutations()
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        rows = t = rates = None
        if sample:
            at[iters] = s.mutations()
            rows = s.mutations_rows()
            if trees:
                off = s._gene_trees_shape()[3][GT_O_DATALNL]
                t = s.gene_trees(raw=True)
                rec = t["records"]
                rates = np.ascontiguousarray(rec[:, :, off + 32:off + 40]).view(np.float64)[:, :, 0] if rec.size else np.zeros(rec.shape[:2])
        if final:
            s.dump_state(final, True)
        return dict(mu=at, rows=rows, trees=t, rates=rates, pop_ages=pop_ages, pack=pk, stats=(hs0, hs1), launches=launches, oob=s.debug_oob())
    finally:
        s.close()


def column_names(pack):
    K, n = pack.K, pack.n
    return [f"mut.{p}" for p in range(K)] + [f"exp.{p}" for p in range(K)] + [f"mutExt.{i}" for i in range(n)] + [f"expExt.{i}" for i in range(n)]


def model_samples(pack, r, loci):
    """per sample and locus of `loci`: the C values of the float model over the chain's own records; the dataLnL of every record
    is asserted first.  What is held to the record is the likelihood's own root sum, flat over the 4 ph values of a column.  The
    sum over log(RR / (4 ph)) count, with RR = sum R the quantity the kernel divides by, is asserted equal as well where every
    column of the locus has one phase; with more phases the two associate differently (R adds four values a row first), so for
    those loci (p7, stress, the tile-edge and two-phase packs) RR is tied to the chain only through the bit comparison of the
    accumulators and rows that follows"""
    t, n, K = r["trees"], pack.n, pack.K
    rec_loci = t["loci"].tolist()
    popFather, bandSrc = [int(x) for x in pack.popFather], [int(x) for x in pack.bandSrc]
    out = []
    for k in range(len(t["iters"])):
        per = []
        for g in loci:
            q = rec_loci.index(g)
            nm = int(t["num_migs"][k, q])
            migs = [(int(t["mig_branch"][k, q, m]), int(t["mig_band"][k, q, m]), float(t["mig_age"][k, q, m])) for m in range(nm)]
            for m in range(nm):
                assert int(t["mig_spop"][k, q, m]) == bandSrc[migs[m][1]]
            v = locus_sample(n, K, t["father"][k, q].tolist(), t["left"][k, q].tolist(), t["right"][k, q].tolist(), t["npop"][k, q].tolist(),
                             [float(a) for a in t["age"][k, q]], int(t["root"][k, q]), migs, float(r["rates"][k, q]), locus_rows(pack, g),
                             r["pop_ages"][k], popFather, bandSrc)
            assert v["lnl"].hex() == float(t["dataLnL"][k, q]).hex(), f"sample {k} locus {g}: the model's inside pass gives dataLnL {v['lnl']!r}, the record {float(t['dataLnL'][k, q])!r}"
            v["single_phase"] = all(w != 0 for w in locus_rows(pack, g)[1])
            if v["single_phase"]:
                assert v["lnl_rr"].hex() == v["lnl"].hex()
            per.append(v)
        out.append(per)
    return out


def flat(v):
    return v["mut"] + v["exp"] + v["mutExt"] + v["expExt"]


def model_acc(samples, S):
    """the accumulators after S samples: per locus C floats, acc = acc + value in sample order"""
    Q, C = len(samples[0]), len(flat(samples[0][0])) if samples[0] else 0
    acc = [[0.0] * C for _ in range(Q)]
    for k in range(S):
        for q in range(Q):
            for c, x in enumerate(flat(samples[k][q])):
                acc[q][c] = acc[q][c] + x
    return acc


def model_row(per, chunk=CHUNK):
    """a sample's row: the loci of a chunk in selection order from 0.0, the chunks in chunk order from 0.0"""
    if not per:
        return []
    C = len(flat(per[0]))
    parts = []
    for q0 in range(0, len(per), chunk):
        part = [0.0] * C
        for v in per[q0:q0 + chunk]:
            for c, x in enumerate(flat(v)):
                part[c] = part[c] + x
        parts.append(part)
    row = [0.0] * C
    for part in parts:
        for c in range(C):
            row[c] = row[c] + part[c]
    return row


def hexes(xs):
    return [float(x).hex() for x in xs]


def check_against_model(e, acc, S, pack, what):
    Q = len(e["loci"])
    got = np.concatenate([e["mut"], e["exp"], e["mutExt"], e["expExt"]], axis=1) if Q else np.zeros((0, 0))
    assert e["samples"] == S and len(acc) == Q and e["columns"] == column_names(pack) and e["chunk"] == CHUNK
    for q in range(Q):
        assert hexes(got[q]) == hexes(acc[q]), f"{what} S {S}: locus {int(e['loci'][q])}: {got[q].tolist()} != {acc[q]}"


def check_case(lib, name, iters=9, checkpoints=CHECKPOINTS, loci=None, key="cpu", pack=None):
    """bit for bit after 1, 2 and the last sample: every fetch and every row against the float model over the chain's own records"""
    r = run_chain(lib, name, iters, loci=loci, checkpoints=[c for c in checkpoints if c < iters], pack=pack)
    pk, t = r["pack"], r["trees"]
    sel = list(range(pk.L)) if loci is None else list(loci)
    assert r["launches"] == iters and r["oob"][0] == 0
    assert t["loci"].tolist() == sel
    samples = model_samples(pk, r, sel)
    for S, e in sorted(r["mu"].items()):
        assert e["loci"].tolist() == sel
        check_against_model(e, model_acc(samples, S), S, pk, name)
    its, rows = r["rows"]
    assert its.tolist() == list(range(iters)) and rows.shape == (iters, 2 * (pk.K + pk.n))
    for k in range(iters):
        assert hexes(rows[k]) == hexes(model_row(samples[k])), f"{name}: the row of sample {k}"
    last = r["mu"][iters]
    tot_mut, tot_exp = float(last["mut"].sum()), float(last["exp"].sum())
    migs = int(t["num_migs"].sum())
    r["maxseg"] = max(v["maxseg"] for per in samples for v in per)
    print(f"{name} [{key}] n {pk.n} K {pk.K} loci {len(sel)} samples {iters}: live migrations in the records {migs}, most segments a branch {r['maxseg']}, sum mut {tot_mut:.6g}, "
          f"sum exp {tot_exp:.6g}, rel {tot_mut / tot_exp if tot_exp else 0.0:.4g}")
    assert tot_mut > 0.0 and tot_exp > 0.0, "no substitution expected anywhere: the case checks nothing"
    r["samples"] = samples
    return r


# ---------------------------------------------------------------- hand-made packs
def phased_pack(base, loci, rates=None):
    """`base` with its loci replaced: loci = a list of loci, each a list of columns ([codes string of every phase], count)"""
    import copy
    import gphocs_amd as G
    p = copy.deepcopy(base)
    offs, leaf, ph, cnt = [0], [], [], []
    for cols in loci:
        rows = 0
        for phases, count in cols:
            for k, codes in enumerate(phases):
                assert len(codes) == p.n
                leaf.append([G.Pack.CODES[ch] for ch in codes])
                ph.append(len(phases) if k == 0 else 0)
                cnt.append(count if k == 0 else 0)
            rows += len(phases)
        offs.append(offs[-1] + rows)
    p.L = p.numLoci = len(loci)
    p.pattern_offsets = np.array(offs, np.int64)
    p.leafcodes = np.array(leaf, np.uint8).reshape(-1, p.n)
    p.numPhases = G.encode_phases(ph)
    p.counts = np.array(cnt, np.int32)
    p.mutRates = np.ones(p.L) if rates is None else np.array(rates, dtype=np.float64)
    p.locusNames = [f"e{g}" for g in range(p.L)]
    return p


def _codes(rng, n, missing=0.05):
    return "".join("N" if rng.random() < missing else "TCAG"[int(rng.integers(4)) if rng.random() < 0.3 else 0] for _ in range(n))


def tile_edge_loci(n, tile=TILE, seed=5):
    """three loci whose columns end on, one before and one behind a tile edge of `tile` rows, with columns that cross an edge"""
    rng = np.random.default_rng(seed)

    def single():
        return ([_codes(rng, n)], int(rng.integers(1, 9)))

    def group(k):
        return ([_codes(rng, n, 0.0) for _ in range(k)], int(rng.integers(1, 5)))
    a = [single() for _ in range(tile - 3)] + [group(2), group(2)] + [single() for _ in range(5)]                   # rows tile - 3 .. tile - 2, tile - 1 .. tile
    b = [single() for _ in range(tile - 2)] + [group(2)] + [single() for _ in range(6)]                             # rows tile - 2 .. tile - 1
    c = [single() for _ in range(tile - 4)] + [group(8)] + [single() for _ in range(2 * tile - 2 - (tile + 4))] + [group(4)]    # rows tile - 4 .. tile + 3, 2 tile - 2 .. 2 tile + 1
    return [a, b, c]


def check_tile_edges(lib, base, iters=2):
    pk = phased_pack(base, tile_edge_loci(base.n))
    P = np.diff(pk.pattern_offsets).tolist()
    assert P == [TILE + 6, TILE + 6, 2 * TILE + 2]
    return check_case(lib, "tile edges", iters=iters, checkpoints=(1,), pack=pk)


def check_zero_length_branches(lib, base, iters=3):
    """three loci, the middle one with a locus rate of 1e-120: rate t < 1e-100 on every branch of it, so u == 0 everywhere (its
    columns are invariant or missing, as a likelihood without substitutions requires).  The kernel equals the model bit for bit on
    all three; on the middle one mut, exp and mutExt are exactly 0 in the accumulators, and the rows are those of the other two"""
    rng = np.random.default_rng(11)
    plain = lambda: [([_codes(rng, base.n)], int(rng.integers(1, 9))) for _ in range(12)]      # noqa: E731
    still = [(["T" * base.n], 30), (["N" + "C" * (base.n - 1)], 4), (["N" * base.n], 2), (["G" * (base.n - 1) + "N"], 5)]
    pk = phased_pack(base, [plain(), still, plain()], rates=[1.0, 1e-120, 1.0])
    r = check_case(lib, "zero-length branches", iters=iters, checkpoints=(1,), pack=pk)
    assert r["rates"][:, 1].tolist() == [1e-120] * iters and r["rates"][:, 0].tolist() == [1.0] * iters
    for S, e in r["mu"].items():
        assert not e["mut"][1].any() and not e["exp"][1].any() and not e["mutExt"][1].any()
        assert e["mut"][0].any() and e["mut"][2].any() and (e["expExt"][1] > 0.0).all() and (e["expExt"][1] < 1e-100).all()
    for k, per in enumerate(r["samples"]):
        assert all(m == 0.0 for m in per[1]["M"]) and all(x is None for x in per[1]["E"])
        assert hexes(r["rows"][1][k][:2 * pk.K]) == hexes([(0.0 + a) + c for a, c in zip((per[0]["mut"] + per[0]["exp"]), (per[2]["mut"] + per[2]["exp"]))])
    return r


# ---------------------------------------------------------------- selections, refusals, lifecycle
def check_selections(lib, name="a70", iters=2):
    """70 loci in chunks of 64: all of them (a full chunk and one of 6), 33 of them (a partial chunk), one locus, the last locus alone"""
    everything = check_case(lib, name, iters=iters, checkpoints=(1,))
    pk, samples = everything["pack"], everything["samples"]
    L = pk.L
    assert L > CHUNK and L % CHUNK
    for sel in (list(range(0, 66, 2)), [5], [L - 1]):
        r = run_chain(lib, name, iters, loci=sel, trees=False)
        e = r["mu"][iters]
        assert e["loci"].tolist() == sel and r["launches"] == iters
        sub = [[per[g] for g in sel] for per in samples]
        check_against_model(e, model_acc(sub, iters), iters, pk, f"{name} selection of {len(sel)}")
        for k in range(iters):
            assert hexes(r["rows"][1][k]) == hexes(model_row(sub[k])), f"{name} selection of {len(sel)}: row {k}"


def check_refusals(lib, capfd, name="j1"):
    """GPH_EARG with a message that names the cause, the sampler left as it was"""
    import gphocs_amd as G
    pk = load_pack(name)
    L = pk.L
    s = G.Sampler(pk, lib=lib)

    def refused(loci, *words):
        la = (ctypes.c_int64 * len(loci))(*loci)
        before = s._mutations_shape()
        capfd.readouterr()
        rc = s.lib.gph_engine_mutations_enable(s.engine, 4, la, len(loci), 0)
        err = capfd.readouterr().err
        assert rc == EARG and all(w in err for w in words), (loci, err)
        assert s._mutations_shape() == before
        with pytest.raises(ValueError):
            s.mutations_enable(4, loci)

    try:
        for on in (False, True):
            if on:
                s.mutations_enable(4, [1, 2])
                assert s._mutations_shape() == (2 * (pk.K + pk.n), CHUNK, 2, 0, 0)
            refused([0, L], f"locus {L}", "out of range")
            refused([-1], "locus -1", "out of range")
            refused([2, 2], "locus 2", "twice")
            refused([3, 2], "locus 2", "increasing")
        assert s.lib.gph_engine_mutations_enable(s.engine, -1, None, 0, 0) == EARG
    finally:
        s.close()


def check_lifecycle(lib, G, name="m3", iters=3):
    """reset, enable twice, a full row buffer, GPH_EFULL one byte short with the feature off, GPH_ESTATE, a rank without a
    selected locus"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    L, C, cap = pk.L, 2 * (pk.K + pk.n), 2 * iters
    need = L * C * 8 + ((L + CHUNK - 1) // CHUNK + cap) * (1 + C) * 8
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.mutations()                                  # not enabled
        assert s.lib.gph_engine_mutations_fetch_loci(s.engine, None, 0, 0) == ESTATE
        assert s.lib.gph_engine_mutations_sample(s.engine, 0) == ESTATE
        assert s._mutations_shape() == (0, 0, 0, 0, 0)
        s.mutations_enable(cap)
        assert s._mutations_shape() == (C, CHUNK, L, 0, 0)
        assert s.lib.gph_engine_mutations_sample(s.engine, 0) == ESTATE           # before initialize
        assert s.lib.gph_engine_mutations_enable(s.engine, cap, None, 0, need - 1) == FULL
        assert s._mutations_shape() == (0, 0, 0, 0, 0)     # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.mutations_enable(cap, max_bytes=need - 1)
        s.initialize()                                     # the engine is still usable
        with pytest.raises(RuntimeError):
            s.mutations_sample(0)
        s.mutations_enable(cap, [1, 2])                    # enable twice: another selection, then the real one
        assert s._mutations_shape() == (C, CHUNK, 2, 0, 0)
        s.mutations_enable(cap, max_bytes=need)
        before = s.mutations()
        assert before["samples"] == 0 and not before["mut"].any() and not before["expExt"].any()
        for it in range(iters):
            s.iteration(it)
            s.mutations_sample(it)
        first = s.mutations(reset=True)
        assert first["samples"] == iters and first["mut"].any() and first["exp"].any() and first["mutExt"].any() and first["expExt"].any()
        zero = s.mutations()
        assert zero["samples"] == 0 and not zero["mut"].any() and not zero["exp"].any()
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.mutations_sample(it)
        assert s._mutations_shape() == (C, CHUNK, L, iters, cap)
        with pytest.raises(BufferError):
            s.mutations_sample(99)                         # the row buffer is full
        second = s.mutations()
        its, rows = s.mutations_rows()
        assert its.tolist() == list(range(2 * iters)) and s._mutations_shape()[4] == 0
        s2 = G.Sampler(pk, lib=lib)                        # the same chain, sampled over the second half only
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.mutations_enable(cap)
                s2.iteration(it)
                if it >= iters:
                    s2.mutations_sample(it)
            fresh = s2.mutations()
            rows2 = s2.mutations_rows()[1]
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        for k in ("mut", "exp", "mutExt", "expExt"):
            assert second[k].tobytes() == fresh[k].tobytes()
        assert rows[iters:].tobytes() == rows2.tobytes()
        s.initialize()                                     # a new chain starts from zeroed accumulators and no rows
        again = s.mutations()
        assert again["samples"] == 0 and not again["mut"].any() and s._mutations_shape()[4] == 0
        s.mutations_enable(4, [])                          # no selected locus: the fold alone, rows of zeros
        s.mutations_sample(0)
        s.mutations_sample(1)
        e = s.mutations()
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["mut"].shape == (0, pk.K)
        its, rows = s.mutations_rows()
        assert its.tolist() == [0, 1] and rows.shape == (2, C) and not rows.any()
    finally:
        s.close()


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """records and final state dump with sampling on identical to a run with sampling off, and still the reference's records;
    launches of class 24 = the samples.  Returns the two runs"""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        r = run_chain(lib, name, full, sample=on, trees=False, record=rec, final=final, pack=G.Pack.load(os.path.join(GOLDEN, name + ".gpk")))
        out.append(dict(rec=rec, final=final, stats=r["stats"], launches=r["launches"], samples=r["mu"][full]["samples"] if on else 0))
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    return on, off


# ---------------------------------------------------------------- the program and the launcher
def _g(x):
    return "%.10g" % x


def expected_files(ctl_dir, ctl, lib=None, sampler_lib=None, loci=None):
    """the text of PREFIX.mutations.tsv and the head (header and rows) of PREFIX.mutations-genome.tsv the program must write,
    formatted from the output of an equivalent Sampler run (burn-in first, a sample wherever a trace line is written)"""
    import gphocs_amd as G
    from sampler_util import printed_names
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    its = [it for it in range(p.numSamplesMcmc) if it % (p.sampleSkip + 1) == 0]
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.mutations_enable(len(its), loci)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it in its:
                s.mutations_sample(it)
        e = s.mutations()
        got_its, rows = s.mutations_rows()
    finally:
        s.close()
    S, K, n = len(its), p.K, p.n
    assert e["samples"] == S and got_its.tolist() == its
    out = ["\t".join(["locus", "name", "samples", "sites"] + [f"{w}_{p.popName[q]}" for q in range(K) for w in ("mut", "exp")] + ["rel"])]
    for q, g in enumerate(e["loci"].tolist()):
        sites = int(sum(locus_rows(p, g)[2]))
        smut = sexp = 0.0
        cells = []
        for k in range(K):
            smut = smut + float(e["mut"][q, k])
            sexp = sexp + float(e["exp"][q, k])
            cells += [_g(float(e["mut"][q, k]) / float(S)), _g(float(e["exp"][q, k]) / float(S))]
        out.append("\t".join([str(g), p.locusNames[g], str(S), str(sites)] + cells + [_g(smut / sexp if sexp > 0.0 else 0.0)]))
    leaves = [f"{nm}.{i}" for i, nm in enumerate(printed_names(list(p.sampleNames)))] if hasattr(p, "sampleNames") else None
    return "\n".join(out) + "\n", its, rows, [p.popName[q] for q in range(K)], leaves, len(e["loci"])


def genome_rows(its, rows):
    return ["%7d" % it + "".join("\t" + _g(float(v)) for v in rows[k]) for k, it in enumerate(its)]


def summary_lines(gen_text, K, n, Q):
    """the "# rel" / "# ext" lines, the last line and the log line, recomputed from the file's own rows"""
    lines = gen_text.splitlines()
    head = lines[0].split("\t")
    rows = [[float(x) for x in ln.split("\t")[1:]] for ln in lines[1:] if not ln.startswith("#")]
    S = len(rows)
    assert len(head) == 1 + 2 * (K + n)
    pops = [h[4:] for h in head[1:1 + K]]
    leaves = [h[7:] for h in head[1 + 2 * K:1 + 2 * K + n]]
    assert head[1 + K:1 + 2 * K] == ["exp_" + nm for nm in pops] and head[1 + 2 * K + n:] == ["expExt_" + nm for nm in leaves]

    def stats(cm, ce):
        x = [(r[cm] / r[ce] if r[ce] != 0.0 else 0.0) for r in rows]
        tot = 0.0
        for v in x:
            tot = tot + v
        mean = tot / float(S) if S else 0.0
        ss = 0.0
        for v in x:
            ss = ss + (v - mean) * (v - mean)
        sd = math.sqrt(ss / float(S - 1)) if S > 1 else 0.0
        return mean, f"mean {_g(mean)} sd {_g(sd)} pHigh {_g(sum(v > 1.0 for v in x) / float(S) if S else 0.0)}"
    out, best = [], (-1.0, "none")
    for p, nm in enumerate(pops):
        mean, text = stats(p, K + p)
        out.append(f"# rel {nm} {text}")
        if mean > 0.0 and abs(math.log(mean)) > best[0]:
            best = (abs(math.log(mean)), f"{nm} {text}")
    for i, nm in enumerate(leaves):
        out.append(f"# ext {nm} {stats(2 * K + i, 2 * K + n + i)[1]}")
    return out + [f"# loci {Q} samples {S}"], "Mutations: " + best[1], pops, leaves


def check_program(lib_path, lib, tmp_path):
    """both files of a short m3 run against values recomputed from Sampler output and the "#" lines recomputed from the file's own
    rows; --mutations-loci and --mutations-rows; every other output of a run with -l -s --clades --triplets is the same bytes with
    and without; chain 0 of --mc3 / --replicates; the usage errors"""
    import subprocess
    import gphocs_amd as G
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import program_ctl
    name = "m3"
    ctl = name + ".ctl"
    a, b, c, d, e, m, r = (tmp_path / x for x in ("with", "without", "sel", "all", "rest", "mc3", "rep"))
    for x in (a, b, c, d, e, m, r):
        _copy_case(name, x, program_ctl(name))
    on = ["--mutations", "out"]
    run = _run(lib_path, a, on + [ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["mutations-genome.tsv", "mutations.tsv"]             # no part left behind
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    want_loci, its, rows, pops, _, Q = expected_files(str(a), ctl, lib, lib)
    assert got["mutations.tsv"] == want_loci
    tail, log, file_pops, leaves = summary_lines(got["mutations-genome.tsv"], pk.K, pk.n, Q)
    assert file_pops == pops and [lv.rsplit(".", 1)[1] for lv in leaves] == [str(i) for i in range(pk.n)]
    assert got["mutations-genome.tsv"].splitlines()[1:] == genome_rows(its, rows) + tail
    assert log in run.stdout.splitlines()
    # a selection, a row buffer of 3 rows that fills several times
    _run(lib_path, c, ["--mutations", "out", "--mutations-loci", "1-9:4", "--mutations-rows", "3", ctl])
    other = read_outputs(c, "out")
    want_loci2, its2, rows2, _, _, Q2 = expected_files(str(c), ctl, lib, lib, [1, 5, 9])
    assert other["mutations.tsv"] == want_loci2 and Q2 == 3
    assert other["mutations-genome.tsv"].splitlines()[1:] == genome_rows(its2, rows2) + summary_lines(other["mutations-genome.tsv"], pk.K, pk.n, Q2)[0]
    assert [ln for ln in got["mutations.tsv"].splitlines() if ln.split("\t")[0] in ("1", "5", "9")] == want_loci2.splitlines()[1:]
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "-s", "cs", "--clades", "cl", "--triplets", "tr"]
    _run(lib_path, d, on + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix in ("cs", "cl", "tr"):
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
    L = pk.L
    for args, words in ((["--mutations-loci", "0-3"], ["--mutations "]), (["--mutations-rows", "4"], ["--mutations "]),
                        (on + ["--mutations-loci", "5,5"], ["locus 5 ", "--mutations-loci"]), (on + ["--mutations-loci", f"3,{L}"], [f"locus {L} ", "--mutations-loci"]),
                        (on + ["--mutations-rows", "0"], ["usage"])):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and all(w in res.stderr for w in words), (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    cwd = os.getcwd()
    os.chdir(u)
    try:
        anylib = lib or G.load_library(dims=(pk.n, pk.K, pk.B))
        for kw in (dict(mutations_loci="0-3"), dict(mutations_rows=4), dict(mutations="out", mutations_rows=-1)):
            assert G.run_control_file(anylib, ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def part_rows(path):
    """(L lines, [(iteration, [floats])]) of a rank's part: the R lines carry the doubles' 64-bit patterns"""
    import struct
    L, R = [], []
    for ln in open(path).read().splitlines():
        if ln.startswith("L\t"):
            L.append(ln[2:])
        if ln.startswith("R\t"):
            f = ln.split("\t")
            R.append((int(f[1]), [struct.unpack("<d", struct.pack("<Q", int(x)))[0] for x in f[2:]]))
    return L, R


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, joined by gph_mutations_write: the per-locus rows are the one-rank rows (concatenated), every
    per-sample row is the fp64 sum of the two parts' rows in rank order -- for all loci and for a selection that lies wholly in rank
    1's block; the launcher does the same; a part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, mutations="out", mutations_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["mutations-genome.tsv", "mutations.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        assert [int(ln.split("\t")[0]) for ln in want["mutations.tsv"].splitlines()[1:]] == loci
        run_ranks(lib_path, name, 2, two, mutations="out", mutations_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.mutations.part0", "out.mutations.part1"]
        (L0, R0), (L1, R1) = part_rows(two / "out.mutations.part0"), part_rows(two / "out.mutations.part1")
        assert [it for it, _ in R0] == [it for it, _ in R1] and len(R0) > 0
        added = ["%7d" % it + "".join("\t" + _g((0.0 + x) + y) for x, y in zip(v0, v1)) for (it, v0), (_, v1) in zip(R0, R1)]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.mutations.part{r}", cut)
            text = open(cut / "out.mutations.part1").read().splitlines(True)
            open(cut / "out.mutations.part1", "w").write("".join(text[:-1]))
            assert lib.gph_mutations_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_mutations_write(str(two / "out").encode(), 2) == 0
        joined = read_outputs(two, "out")
        assert sorted(joined) == ["mutations-genome.tsv", "mutations.tsv"]      # no part among them
        assert joined["mutations.tsv"] == want["mutations.tsv"] and joined["mutations.tsv"].splitlines()[1:] == L0 + L1
        gen = joined["mutations-genome.tsv"].splitlines()
        assert gen[0] == want["mutations-genome.tsv"].splitlines()[0]
        assert [ln for ln in gen[1:] if not ln.startswith("#")] == added
        assert gen[1 + len(added):] == summary_lines(joined["mutations-genome.tsv"], pk.K, pk.n, len(loci))[0]
        if spec is not None:
            # every selected locus lies in rank 1's block: rank 0 adds zeros, the sums are the one-rank sums of one chunk
            assert joined == want
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--mutations", "out", "--mutations-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.mutations-genome.tsv must be
    written: status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.mutations-genome.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--mutations", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.mutations-genome.tsv"] and not os.listdir(d / "out.mutations-genome.tsv")
