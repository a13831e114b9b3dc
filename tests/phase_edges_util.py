"""What the phase-edge tests share (test_phase_edges.py on the host builds, test_phase_edges_gpu.py on the MI355X).

Summing over the phases of an unphased pattern is done by add_phases (csrc/gph_locus.h: a lane shift per round, behind lik_compute in
both forms, lik_private_t and lr_ref_eval) and, for loci of more than 64 rows, by root_sum_generic.  The goldens hold no group of
more than 16 rows in a locus of at most 64, none that ends in the wave's last lane, and no count that is not a power of two.  The
packs made here keep a golden's MODEL and make the loci up: random rows, any layout of groups.  A layout is the list of phase
counts of a locus in row order, [1, 64, 1] = a phased pattern, 64 phases of one pattern, a phased pattern (66 rows).

Three references, none of them the code under test: the oracle (oracle/gphocs_oracle, run live on the written pack), the identities
of power_posterior_util.py, and model_lnl() below: the likelihood of one gene tree in 60-digit decimal arithmetic."""
import copy
import os
from decimal import Decimal as D
from decimal import localcontext

import numpy as np

from conftest import GOLDEN
import power_posterior_util as PP

GT_O_DATALNL = 3        # gph_engine_gene_trees_shape: the offset of dataLnL in a record; FS_MUTRATE lies 4 doubles behind it (ess_util.py)
MODEL_TOL = 1e-10       # the project's parity bar (parity_util.REL_TOL) as a cap; measured: at most 5.6e-14 (the tests' docstrings)

# the layouts the narrow (P <= 64: lane path) and the wide paths must meet; NARROW[k] is named by its index below
NARROW = [
    [64],                           # 0: one group over the whole wave, 6 rounds of the shift
    [32, 32],                       # 1: two groups, the second ends in lane 63
    [1] * 48 + [16],                # 2: a group at lanes 48..63
    [1] * 30 + [32, 1],             # 3: P = 63, a group of 32 at lanes 30..61
    [1, 64, 1],                     # 4: P = 66, wide: the group straddles row 64
    [1] * 60 + [8],                 # 5: P = 68, wide: the group straddles row 64 and ends at the last row
    [3, 5, 6, 7, 12, 1, 2, 4],      # 6: counts that are no power of two: the prob / nc branch; the last group ends at P - 1 = 39
    [1, 2, 4, 8, 16],               # 7: every count a power of two: the ldexp branch; ends at P - 1 = 30
    [1],                            # 8
    [2],                            # 9
    [],                             # 10: P = 0
    [16, 1, 16, 1, 16, 1, 13],      # 11: P = 64, the last group (13: no power of two) ends in lane 63
    [1] * 62 + [2],                 # 12: a group of 2 at lanes 62..63
    [8, 8, 1, 4, 2, 1],             # 13: two adjacent groups from lane 0
    [2, 4, 1, 8, 16, 2, 3],         # 14: the only count that is no power of two is the last pattern's
    # 15: P = 158, wide, and past what GPH_HUGE_LDS=5200 leaves for a sequence block next to any variant's image (1.6 KB at 12
    # leaves): groups straddling rows 64 and 128 of a block that lies in HBM, the last one ending at the last row
    [1] * 20 + [64] + [1] * 9 + [32] + [5] * 6 + [3],
]
I_64, I_P63 = 0, 3
ALL_N_AT = (7, 0)       # (layout, row): the one row that is N in every sample
HUGE = [[1, 32768, 2], [16384, 1], [1, 1, 1]]      # phase words 0x8000 | 15 (the smallest encoded one) and 16384 (the largest plain one)


def _rows(rng, n, k, anc):
    """k distinct rows of n leaf codes: about 70 % the base `anc`, the rest uniform over T C A G, 8 % N; never N throughout"""
    seen, out = set(), []
    while len(out) < k:
        m = max(16, 2 * (k - len(out)))
        r = np.where(rng.random((m, n)) < 0.7, anc, rng.integers(0, 4, (m, n)))
        r = np.where(rng.random((m, n)) < 0.08, 4, r).astype(np.uint8)
        for row in r:
            t = row.tobytes()
            if t not in seen and not (row == 4).all():
                seen.add(t)
                out.append(row)
                if len(out) == k:
                    break
    return out


def build_pack(base, layouts, seed, big_count=False, all_n=None, first=0):
    """the model of golden `base` over made-up loci, one per layout (the list is rotated so that layouts[first] becomes locus 0: the
    reference locus of the locus-rate scan); counts 1..40 on first rows, 0 behind them; big_count: one count of 70000, beyond the
    16-bit count form; all_n = (layout, row): that row is N in every sample.  Deterministic from the seed."""
    import gphocs_amd as G
    p = G.Pack.load(os.path.join(GOLDEN, base + ".gpk"))
    rng = np.random.default_rng(seed)
    order = list(range(first, len(layouts))) + list(range(first))
    offs, leaf, ph, cnt = [0], [], [], []
    for li in order:
        lay = layouts[li]
        rows = _rows(rng, p.n, sum(lay), int(rng.integers(0, 4)))
        if all_n is not None and all_n[0] == li:
            rows[all_n[1]] = np.full(p.n, 4, np.uint8)
        leaf.extend(rows)
        for k in lay:
            ph.extend([k] + [0] * (k - 1))
            cnt.extend([int(rng.integers(1, 41))] + [0] * (k - 1))
        offs.append(offs[-1] + sum(lay))
    if big_count:
        cnt[next(i for i, k in enumerate(ph) if k > 0)] = 70000
    p.L = p.numLoci = len(layouts)
    p.layouts = [layouts[li] for li in order]
    p.pattern_offsets = np.array(offs, np.int64)
    p.leafcodes = np.array(leaf, np.uint8).reshape(-1, p.n)
    p.numPhases = G.encode_phases(ph)
    p.counts = np.array(cnt, np.int32)
    p.mutRates = np.ones(p.L)
    p.ftMixing = PP.FT_MIXING          # the goldens' own mixing step is never rejected (power_posterior_util.py)
    return p


def narrow_pack(base, seed=5, big_count=False, first=0):
    return build_pack(base, NARROW, seed, big_count=big_count, all_n=ALL_N_AT, first=first)


def huge_pack(seed=3):
    """three loci on the model of g1 (8 leaves): groups of 2^15 and 2^14 rows on the wide path"""
    return build_pack("g1", HUGE, seed)


def groups(pack, g):
    """(first row within the locus, phase count) of every group of locus g, from the pack's own arrays"""
    import gphocs_amd as G
    o0, o1 = int(pack.pattern_offsets[g]), int(pack.pattern_offsets[g + 1])
    ph = G.decode_phases(pack.numPhases[o0:o1])
    out, r = [], 0
    while r < o1 - o0:
        k = int(ph[r])
        assert k >= 1 and r + k <= o1 - o0 and not ph[r + 1:r + k].any()
        out.append((r, k))
        r += k
    return out


def covered(pack, iters=None, r=None, kinds=()):
    """the pack holds what it was made for -- read from its arrays, not from the layouts it was built from -- and, given the
    counters of a run (power_posterior_util.run's keys accept / tau / lrate), every proposal kind in `kinds` was both accepted
    and rejected"""
    P = np.diff(pack.pattern_offsets)
    G_ = [groups(pack, g) for g in range(pack.L)]
    def pow2(k):
        return k & (k - 1) == 0
    assert any(P[g] == 64 and (0, 64) in G_[g] for g in range(pack.L)), "a 64-phase group at P = 64"
    assert any(P[g] <= 64 and any(k > 1 and r0 + k - 1 == 63 for r0, k in G_[g]) for g in range(pack.L)), "a group ending at lane 63"
    assert any(P[g] < 64 and any(k > 1 and r0 + k == P[g] for r0, k in G_[g]) for g in range(pack.L)), "a group ending at P - 1 < 63"
    assert any(P[g] > 64 and any(k > 1 and r0 < 64 <= r0 + k - 1 for r0, k in G_[g]) for g in range(pack.L)), "a wide group straddling row 64"
    assert any(P[g] <= 64 and any(not pow2(k) for _, k in G_[g]) for g in range(pack.L)), "a locus with a count that is no power of two"
    assert any(0 < P[g] <= 64 and any(k > 1 for _, k in G_[g]) and all(pow2(k) for _, k in G_[g]) for g in range(pack.L)), "a locus of powers of two"
    assert any(P[g] <= 64 and any(k >= 32 for _, k in G_[g]) for g in range(pack.L)), "a group of 32 or more in the lane path"
    assert (P == 0).any(), "a locus without patterns"
    assert (pack.leafcodes == 4).all(axis=1).any(), "a row that is N in every sample"
    for g in range(pack.L):
        rows = pack.leafcodes[int(pack.pattern_offsets[g]):int(pack.pattern_offsets[g + 1])]
        assert len({row.tobytes() for row in rows}) == len(rows), "rows are distinct within a locus"
    if r is not None:
        PP.covered(pack, iters, r, kinds)


def kinds_for(pack):
    """the proposal kinds with a data term: every one of them reads the root sum"""
    return ("coal", "spr", "tau", "mixing") + (("lrate",) if int(getattr(pack, "mutRateMode", 0)) == 1 else ())


def run(G, lib, pack, iters, trace=None, state=None, env=None, with_cond=True):
    """one chain of `iters` iterations: records to `trace`, the state dump after the last one to `state`, the gene trees of every
    locus after the last one with the locus rates next to them, the counters covered() reads, debug_oob()"""
    import ctypes as C
    old = {}
    for k, v in (env or {}).items():
        old[k] = os.environ.get(k)
        os.environ[k] = v
    try:
        s = G.Sampler(pack, lib=lib)
        try:
            if trace:
                s.set_record_file(trace)
            s.initialize()
            s.enable_gene_trees(1)
            for it in range(iters):
                s.iteration(it)
            s.sample_gene_trees(iters - 1)
            off = s._gene_trees_shape()[3][GT_O_DATALNL]
            t = s.gene_trees(raw=True)
            rec = t["records"]
            rates = np.ascontiguousarray(rec[:, :, off + 32:off + 40]).view(np.float64)[0, :, 0].copy()
            if state:
                s.dump_state(state, with_cond)
            if trace:
                s.set_record_file(None)
            tau = (C.c_int64 * 64)()
            assert s.lib.gph_mcmc_tau_accept_counts(s.mcmc, tau) == 0
            lra, rv = C.c_int64(), C.c_double()
            assert s.lib.gph_mcmc_locus_rate_state(s.mcmc, C.byref(lra), C.byref(rv)) == 0
            return dict(accept=s.accept_counts(), tau=list(tau)[:pack.K], lrate=lra.value, trees=t, rates=rates, oob=s.debug_oob(),
                        dataLogLikelihood=s.state()["dataLogLikelihood"])
        finally:
            s.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_oracle(oracle_cli, path, iters, trace, state, with_cond=True):
    import subprocess
    subprocess.run([oracle_cli, "run", path, str(iters), trace, state, str(iters - 1), "1" if with_cond else "0"], check=True, timeout=600)


# ---------------------------------------------------------------- the independent model
def model_lnl(pack, g, age, left, right, root, rate):
    """ln p(D_g | gene tree) in 60-digit decimal arithmetic, by plain recursion over the tree: a leaf's conditional is 1 for its
    base (all four 1 for N); along an edge pe = (1 - exp(-4 rate dAge / 3)) / 4 (0 when rate dAge < 1e-100), a child's factor for
    base a is S pe + c_a (1 - 4 pe) with S the sum of the child's four values; a node is the product of its two children's
    factors; the locus is the sum over first rows of count ln(sum over the rows of the group and the four bases / (4 ph))"""
    n = pack.n
    o0 = int(pack.pattern_offsets[g])
    with localcontext() as ctx:
        ctx.prec = 60
        edge = {}
        for v in range(n, 2 * n - 1):
            for ch in (int(left[v]), int(right[v])):
                t = D(float(rate)) * (D(float(age[v])) - D(float(age[ch])))
                edge[ch] = (1 - (-4 * t / 3).exp()) / 4 if t >= D("1e-100") else D(0)

        def cond(v, row):
            if v < n:
                c = int(pack.leafcodes[row][v])
                return [D(1)] * 4 if c == 4 else [D(1) if a == c else D(0) for a in range(4)]
            out = [D(1)] * 4
            for ch in (int(left[v]), int(right[v])):
                cc, pe = cond(ch, row), edge[ch]
                S = sum(cc)
                out = [out[a] * (S * pe + cc[a] * (1 - 4 * pe)) for a in range(4)]
            return out
        tot = D(0)
        for r0, k in groups(pack, g):
            s = D(0)
            for j in range(k):
                s += sum(cond(int(root), o0 + r0 + j))
            tot += (s / (4 * k)).ln() * int(pack.counts[o0 + r0])
        return tot


def model_deviation(pack, r, max_rows=None):
    """the largest |engine - model| / |model| over the loci of a run (run() above); a locus without patterns must read 0.0.
    max_rows: loci with more rows are left to the oracle (the recursion is Python: 2^15 rows take minutes)"""
    t, worst, seen = r["trees"], 0.0, 0
    var = int(getattr(pack, "mutRateMode", 0)) == 1
    for q, g in enumerate(t["loci"]):
        g = int(g)
        got = float(t["dataLnL"][0, q])
        P = int(pack.pattern_offsets[g + 1] - pack.pattern_offsets[g])
        if P == 0:
            assert got == 0.0, (g, got)
            continue
        if max_rows is not None and P > max_rows:
            continue
        rate = float(r["rates"][q])
        assert var or rate == 1.0, (g, rate)
        want = model_lnl(pack, g, t["age"][0, q], t["left"][0, q], t["right"][0, q], t["root"][0, q], rate)
        assert want != 0
        worst = max(worst, float(abs((D(got) - want) / want)))
        seen += 1
    assert seen > 0
    return worst


# ---------------------------------------------------------------- the load boundary
def m3():
    import gphocs_amd as G
    return G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))


def _set(name, index, value):
    def f(p):
        getattr(p, name)[index] = value
    return f


def _two(p, row):
    p.numPhases[row], p.numPhases[row + 1] = 2, 0
    p.counts[row + 1] = 0


def malformed(p):
    """name: (locus that must be named, pattern of that locus, GPH_LOAD_* code, what to do to a copy of m3).  Every locus of m3 has
    at least two rows; locus g starts at row o[g]"""
    o = [int(x) for x in p.pattern_offsets]
    def inside_word(q):
        _two(q, o[5])
        q.numPhases[o[5] + 1] = 1
    def inside_count(q):
        _two(q, o[6])
        q.counts[o[6] + 1] = 3
    return {
        "overrun": (1, o[2] - o[1] - 1, -104, _set("numPhases", o[2] - 1, 2)),          # a count running one row past its locus
        "overrun-last-locus": (p.L - 1, o[p.L] - o[p.L - 1] - 1, -104, _set("numPhases", o[p.L] - 1, 2)),      # ... past the arrays
        "word-0x801f": (2, 0, -102, _set("numPhases", o[2], 0x801F)),
        "word-0x8003": (3, 1, -102, _set("numPhases", o[3] + 1, 0x8003)),
        "word-32768": (4, 0, -102, _set("numPhases", o[4], 32768)),
        "word-0x800e": (4, 0, -102, _set("numPhases", o[4], 0x800E)),                   # the legal exponents are 15 .. 24:
        "word-0x8019": (4, 0, -102, _set("numPhases", o[4], 0x8019)),                   # 14 and 25 are no counts,
        "word-0x800f-legal": (4, 0, -104, _set("numPhases", o[4], 0x800F)),             # 15 and 24 are, and only run past
        "word-0x8018-legal": (4, 0, -104, _set("numPhases", o[4], 0x8018)),             # the locus here
        "word-inside": (5, 1, -105, inside_word),
        "count-inside": (6, 1, -105, inside_count),
        "zero-leading": (7, 0, -103, _set("numPhases", o[7], 0)),
        "zero-later": (8, 1, -103, _set("numPhases", o[8] + 1, 0)),
        "negative-count": (9, 1, -106, _set("counts", o[9] + 1, -5)),
        "leaf-code-5": (10, 1, -107, _set("leafcodes", (o[10] + 1, 3), 5)),
    }


def check_refusal(lib, p, capfd, locus, code, pattern=None):
    """gph_engine_create and gph_engine_load_loci through Sampler(): refused with GPH_EARG, the locus (and the pattern) named on stderr
    and in what gph_engine_last_error / _text return; initialize is never called, nothing is launched"""
    import gphocs_amd as G
    import pytest
    with pytest.raises(RuntimeError) as ei:
        G.Sampler(p, lib=lib)           # (gph_engine_create and gph_engine_load_loci: initialize is never called)
    err = capfd.readouterr().err
    assert (ei.value.locus, ei.value.code) == (locus, code), str(ei.value)
    assert f"locus {locus}:" in ei.value.text and ei.value.text in err
    if pattern is not None:
        assert f"locus {locus}: pattern {pattern}:" in ei.value.text
    assert "status -1" in str(ei.value)            # GPH_EARG


def oversized(p, rows=1 << 25):
    """a copy of pack p cut to two loci whose offsets claim `rows` rows for the second one; the arrays stay as small as they are"""
    q = copy.deepcopy(p)
    o1 = int(p.pattern_offsets[1])
    q.L = q.numLoci = 2
    q.pattern_offsets = np.array([0, o1, o1 + rows], np.int64)
    q.mutRates = p.mutRates[:2].copy()
    return q
