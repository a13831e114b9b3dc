"""What the reduction tests share (test_reduce.py on the host builds, test_reduce_gpu.py on the MI355X).

k_reduce_stage (csrc/gph_engine.hip) folds the per-locus outputs (section 0) and the per-locus statistics (section 1) into the
reduced row every global decision is taken from.  gph_debug_reduce_ runs it with no engine around it: made-up values, any number
of loci and columns, several launches back to back through one partials buffer and one ticket.  On the host build the same entry
runs the serial loop the host engine sums with.

References, all here, none of them the code under test:
  exact_sums      integers of at most 2^30 in magnitude: every partial sum of 2^18 of them is below 2^49, so ANY order of
                  additions is exact and the row must EQUAL Python's integer sums;
  math.fsum       per column, with a bound derived from the longest addition path of the documented shape;
  shape_model     the documented fixed shape restated in numpy, vectorised over (block, sub-sequence, column): the device's sums
                  must have its bit patterns.

The shape (comments at reduce_run / reduce_partial_body / reduce_final_body): block b of GPH_RED_BLOCKS owns the loci
[b chunk, min((b + 1) chunk, L)), chunk = ceil(L / GPH_RED_BLOCKS).  Inside it Q sub-sequences q, q + Q, q + 2 Q, ... are each
folded in index order from +0.0 and then combined in the order of q from +0.0; Q = GPH_RED_SUBS * 64 / cw with cw = 16 / 32 / 64
for at most 16 / 32 / 64 columns and Q = GPH_RED_SUBS above.  The final pass folds the block partials as GPH_RED_SUBS runs of
consecutive blocks, each from +0.0, and combines the runs in order from +0.0.  Section 1 is folded window by window, 128 columns at
a time, and a column has the shape of ITS window's width: at 278 columns the first 256 have Q = 8 and the last 22 have Q = 16."""
import ctypes as C
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

from conftest import REPO

DP = C.POINTER(C.c_double)
EARG = -1                   # GPH_EARG (include/gphocs_hip.h)
WINDOW = 128                # columns of section 1 folded per call of reduce_partial_body / reduce_final_body
ERR_WORD = 7                # what the tests put into the error word

LOCI = (1, 2, 255, 256, 257, 511, 513, 2049)
# one width per cw class also gets: chunk 33 (a second step at Q = 32), chunk 129 (a second unroll trip at Q = 8), 257 (... at
# Q = 16), 513 (... at Q = 32: section 0), and the benchmark's count
LOCI_LARGE = (8193, 32769, 65537, 131073, 100000)
WIDTHS_0 = (1, 15, 16)
WIDTHS_128 = (1, 2, 15, 16, 17, 26, 32, 33, 63, 64, 65, 110, 127, 128)      # on a library with 128-column rows: dims (16, 9, 4)
WIDTHS_384 = (129, 144, 145, 256, 257, 278, 384)                            # on the many-band variant: dims (64, 39, 100)
DIMS_128, DIMS_384 = (16, 9, 4), (64, 39, 100)
# (section, width) of the cases that get LOCI_LARGE: cw 16 (section 0 as the engine folds it), 32, 64, 128, and the windows
LARGE_128 = ((0, 16), (1, 26), (1, 64), (1, 110))
LARGE_384 = ((1, 278),)


def host_library(wide=False):
    """the host build of the engine sources; wide: the one with the many-band capacities (384-column rows)"""
    sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))
    import run_hostemu as R
    import gphocs_amd as G
    return G.load_library(R.build_hostemu(big=wide))


def probe(lib, out0, stats1, L, nc0, nc1, nsets=1, launches=1, err_word=ERR_WORD, rows=None):
    """gph_debug_reduce_: (status, rows as float64 [launches][GPH_RED_ROW], info).  out0 [nsets][L][GPH_OUT_SLOTS] or None, stats1
    [nsets][L][nc1] or None.  `rows`: a buffer of the caller's (the refusals look at what is left in it)"""
    info = (C.c_int32 * 10)()
    if rows is None:
        i0 = constants(lib)
        rows = np.zeros((launches, i0.row))
    a = None if out0 is None else np.ascontiguousarray(out0, dtype=np.float64)
    b = None if stats1 is None else np.ascontiguousarray(stats1, dtype=np.float64)
    rc = lib.gph_debug_reduce_(None if a is None else a.ctypes.data_as(DP), None if b is None else b.ctypes.data_as(DP), L, nc0, nc1,
                               nsets, err_word, launches, rows.ctypes.data_as(DP), info, 0)
    return rc, rows, _info(info)


def _info(w):
    return SimpleNamespace(cols=w[0], stride=w[1], row=w[2], blocks=w[3], subs=w[4], unroll=w[5], out_slots=w[6], ticket=w[7],
                           poison=(w[8] & 0xFFFFFFFF) | ((w[9] & 0xFFFFFFFF) << 32))


_constants = {}


def constants(lib):
    """the library's own sizes, asked once per library with the smallest call there is"""
    key = id(lib)
    if key not in _constants:
        info = (C.c_int32 * 10)()
        one = np.ones(16 * 64)         # at least GPH_OUT_SLOTS doubles whatever the library's value
        rows = np.zeros(1 << 16)       # at least GPH_RED_ROW doubles
        assert lib.gph_debug_reduce_(one.ctypes.data_as(DP), None, 1, 1, 0, 1, 0, 1, rows.ctypes.data_as(DP), info, 0) == 0
        _constants[key] = _info(info)
        assert _constants[key].row <= len(rows) and _constants[key].out_slots <= len(one)
    return _constants[key]


# ---------------------------------------------------------------- the documented shape
def cw_of(ncols):
    return 16 if ncols <= 16 else 32 if ncols <= 32 else 64 if ncols <= 64 else 128


def windows(sec, ncols):
    """(first column, columns) of every call of the partial / final bodies for a section"""
    if sec == 0:
        return [(0, ncols)]
    return [(cb, min(WINDOW, ncols - cb)) for cb in range(0, ncols, WINDOW)]


def subsequences(info, wcols):
    """Q of a window of wcols columns"""
    cw = cw_of(wcols)
    return info.subs if cw == 128 else info.subs * 64 // cw


def chunk_of(info, L):
    return -(-L // info.blocks)


def path_length(info, L, wcols):
    """the longest chain of additions a column of a window of wcols columns goes through; the host build: L"""
    if info.subs == 0:
        return L
    Q = subsequences(info, wcols)
    return -(-chunk_of(info, L) // Q) + Q + info.blocks // info.subs + info.subs


def shape_model(info, x, sec):
    """sums of x [L][ncols] in the documented shape: float64 [ncols].  Vectorised over (block, sub-sequence, column); the loops run
    over the steps of a sub-sequence, the sub-sequences of a block, the blocks of a run and the runs"""
    L, ncols = x.shape
    chunk = chunk_of(info, L)
    out = np.empty(ncols)
    for cb, wc in windows(sec, ncols):
        Q = subsequences(info, wc)
        steps = -(-chunk // Q)
        pad = np.zeros((info.blocks, steps * Q, wc))
        flat = np.zeros((info.blocks * chunk, wc))
        flat[:L] = x[:, cb:cb + wc]
        pad[:, :chunk] = flat.reshape(info.blocks, chunk, wc)
        # element i of block b is locus b chunk + i: it exists below chunk and below L; sub-sequence q takes i = q, q + Q, ...
        i = np.arange(steps * Q)
        live = (i[None, :] < chunk) & (np.arange(info.blocks)[:, None] * chunk + i[None, :] < L)
        pad = pad.reshape(info.blocks, steps, Q, wc)
        live = live.reshape(info.blocks, steps, Q, 1)
        s = np.zeros((info.blocks, Q, wc))
        for t in range(steps):
            s = np.where(live[:, t], s + pad[:, t], s)
        part = np.zeros((info.blocks, wc))
        for q in range(Q):
            part = part + s[:, q]
        per = info.blocks // info.subs
        runs = np.zeros((info.subs, wc))
        part = part.reshape(info.subs, per, wc)
        for j in range(per):
            runs = runs + part[:, j]
        tot = np.zeros(wc)
        for k in range(info.subs):
            tot = tot + runs[k]
        out[cb:cb + wc] = tot
    return out


# ---------------------------------------------------------------- data
def section_arrays(info, sec, x):
    """x [nsets][L][ncols] as the probe's arguments (out0, stats1, nc0, nc1).  Section 0 rows have GPH_OUT_SLOTS slots whatever
    is folded: the slots behind ncols hold large values that must not reach any column"""
    nsets, L, ncols = x.shape
    if sec == 1:
        return None, x, 0, ncols
    o = np.full((nsets, L, info.out_slots), 3.0e9)
    o[:, :, :ncols] = x
    return o, None, ncols, 0


def integer_data(rng, nsets, L, ncols):
    """distinct per (set, locus, column) with overwhelming probability: uniform integers of [-2^30, 2^30] as doubles"""
    return rng.integers(-2 ** 30, 2 ** 30, (nsets, L, ncols), endpoint=True).astype(np.float64)


def float_data(rng, nsets, L, ncols):
    """u 10^k, u uniform in [-1, 1], k uniform in -3..3 per element"""
    u = rng.uniform(-1.0, 1.0, (nsets, L, ncols))
    k = rng.integers(0, 7, (nsets, L, ncols), dtype=np.uint8)
    u *= np.array([10.0 ** e for e in range(-3, 4)])[k]
    return u


def edge_loci(info, L, wcols):
    """where an extreme is easiest to lose: locus 0 and L - 1 (the last locus of the last chunk that is not empty), the first and
    the last locus of a middle chunk, an element of sub-sequence Q - 1, unroll slot GPH_RED_UNROLL - 1 of the first trip and slot 0
    of the second -- the last three where the chunk is long enough (and the build has sub-sequences at all)"""
    chunk = chunk_of(info, L)
    nb = -(-L // chunk)
    g0 = (nb // 2) * chunk
    e = [0, L - 1, g0, min(g0 + chunk, L) - 1]
    if info.subs:
        Q = subsequences(info, wcols)
        for i in (Q - 1, (info.unroll - 1) * Q, info.unroll * Q, info.unroll * Q + Q - 1):
            if i < chunk and g0 + i < L:
                e.append(g0 + i)
    return sorted(set(e))


# ---------------------------------------------------------------- what a row must hold
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def block(info, row, sec, kind, ncols=None):
    """sum (kind 0), minimum (1) or maximum (2) block of a section of a row; ncols: its first columns only"""
    o = sec * info.stride + kind * info.cols
    return row[o:o + (info.cols if ncols is None else ncols)]


def check_unwritten(info, row, nc0, nc1, err_word=ERR_WORD):
    """(e): columns from ncols on of each of the three blocks of a section keep the poison -- all of them where the section was not
    asked for; the trailing words of section 0 hold the error word and seven poisons (the final pass writes the error word whatever
    sections it folds), those of section 1 eight poisons; the ticket is back at 0"""
    b = bits(row)
    for sec, n in ((0, nc0), (1, nc1)):
        for kind in range(3):
            o = sec * info.stride + kind * info.cols
            assert np.all(b[o + n:o + info.cols] == info.poison), (sec, kind, n)
            assert not np.any(b[o:o + n] == info.poison), (sec, kind, n)
        tail = b[sec * info.stride + 3 * info.cols:(sec + 1) * info.stride]
        assert len(tail) == 8
        if sec == 0:
            assert row[3 * info.cols] == float(err_word) and np.all(tail[1:] == info.poison)
        else:
            assert np.all(tail == info.poison)
    assert info.ticket == 0


def exact_sums(x):
    """Python's integer sums of integer-valued doubles, per column"""
    xi = x.astype(np.int64)
    assert np.array_equal(xi.astype(np.float64), x)
    return [int(v) for v in xi.sum(axis=0, dtype=np.int64)]      # |sum| < 2^49: int64 adds integers exactly


def check_integers(lib, sec, ncols, L, seed):
    """(a): the sum columns equal the integer sums, the minima and maxima the columns' own"""
    info = constants(lib)
    rng = np.random.default_rng(seed)
    x = integer_data(rng, 1, L, ncols)
    o, s, nc0, nc1 = section_arrays(info, sec, x)
    rc, rows, got = probe(lib, o, s, L, nc0, nc1)
    assert rc == 0
    want = exact_sums(x[0])
    have = block(info, rows[0], sec, 0, ncols)
    assert [int(v) for v in have] == want and all(float(v).is_integer() for v in have), (sec, ncols, L)
    assert np.array_equal(block(info, rows[0], sec, 1, ncols), x[0].min(axis=0)), (sec, ncols, L)
    assert np.array_equal(block(info, rows[0], sec, 2, ncols), x[0].max(axis=0)), (sec, ncols, L)
    check_unwritten(got, rows[0], nc0, nc1)


def check_fsum(info, x, have, sec):
    """(b): |row - fsum| <= d 2^-53 sum|v| (1 + 1e-6) per column, d the longest addition path of the column's window.  Why d and
    no more: a path of d additions starts three times from +0.0 (sub-sequence, block, run), and x + 0.0 is exact, so at most d - 3
    of them round -- each by at most 2^-53 of a partial sum that is itself at most sum|v| (1 + d 2^-53); fsum's own rounding takes
    one of the three that are left.  The host build adds serially: d = L, the first addition exact.  Returns the worst ratio."""
    L, ncols = x.shape
    worst = 0.0
    xt = np.ascontiguousarray(x.T)
    for cb, wc in windows(sec, ncols):
        d = path_length(info, L, wc)
        for c in range(cb, cb + wc):
            ref = math.fsum(xt[c].tolist())
            # (sum|v| by numpy's pairwise sum: off by a few 2^-53 of itself, far inside the 1e-6)
            bound = d * 2.0 ** -53 * float(np.abs(xt[c]).sum()) * (1 + 1e-6)
            dist = abs(float(have[c]) - ref)
            assert dist <= bound, (sec, ncols, L, c, float(have[c]), ref, dist, bound)
            if bound > 0:
                worst = max(worst, dist / bound)
    return worst


def check_floats(lib, sec, ncols, L, seed, model=False):
    """(b), on the device (model=True) also (c): the sums have the bit patterns of shape_model; and (e)"""
    info = constants(lib)
    rng = np.random.default_rng(seed)
    x = float_data(rng, 1, L, ncols)
    o, s, nc0, nc1 = section_arrays(info, sec, x)
    rc, rows, got = probe(lib, o, s, L, nc0, nc1)
    assert rc == 0
    have = block(info, rows[0], sec, 0, ncols)
    ratio = check_fsum(info, x[0], have, sec)
    if model:
        want = shape_model(info, x[0], sec)
        bad = np.flatnonzero(bits(have) != bits(want))
        assert len(bad) == 0, (sec, ncols, L, bad[:8], have[bad[:8]], want[bad[:8]])
    assert np.array_equal(block(info, rows[0], sec, 1, ncols), x[0].min(axis=0))
    assert np.array_equal(block(info, rows[0], sec, 2, ncols), x[0].max(axis=0))
    check_unwritten(got, rows[0], nc0, nc1)
    return ratio


def check_extremes(lib, sec, ncols, L, seed):
    """(d): every column's minimum and maximum planted at the edge loci, taken cyclically; then three columns of special values.
    A column that holds a -inf: sum and minimum -inf.  A column of -0.0 only: sum +0.0 (every fold starts from +0.0).  A column
    that holds a NaN: the sum is NaN; nothing is asserted about its minimum and maximum.  What the kernel does with them: `v < mn`
    and `v > mx` are false for a NaN, so it is passed over and the column's minimum and maximum are those of its other elements
    (1e300 and -1e300, the starting values, for a column of NaN only) -- the serial loop of the host build does the same."""
    info = constants(lib)
    rng = np.random.default_rng(seed)
    x = float_data(rng, 1, L, ncols)
    for cb, wc in windows(sec, ncols):
        e = edge_loci(info, L, wc)
        for c in range(cb, cb + wc):
            lo, hi = e[c % len(e)], e[(c + 1) % len(e)]
            x[0, lo, c] = -(1.0e4 + c)          # beyond every |v| <= 1e3 of float_data
            if hi != lo:
                x[0, hi, c] = 1.0e4 + c
    o, s, nc0, nc1 = section_arrays(info, sec, x)
    rc, rows, got = probe(lib, o, s, L, nc0, nc1)
    assert rc == 0
    mn, mx = block(info, rows[0], sec, 1, ncols), block(info, rows[0], sec, 2, ncols)
    assert np.array_equal(mn, x[0].min(axis=0)) and np.array_equal(mx, x[0].max(axis=0)), (sec, ncols, L)
    assert np.all(mn == -(1.0e4 + np.arange(ncols))), (sec, ncols, L)
    if L > 1:
        assert np.all(mx == 1.0e4 + np.arange(ncols)), (sec, ncols, L)
    check_unwritten(got, rows[0], nc0, nc1)
    # the special columns: the last ones, as many of the three as the width has room for; the special element at an edge locus
    y = x           # the same array, the planted extremes and all: the references below are taken from the array itself
    e = edge_loci(info, L, windows(sec, ncols)[-1][1])
    c_inf, c_nan, c_zero = ncols - 1, ncols - 2, ncols - 3
    y[0, e[len(e) // 2], c_inf] = -np.inf
    if c_nan >= 0:
        y[0, e[-1], c_nan] = np.nan
    if c_zero >= 0:
        y[0, :, c_zero] = -0.0
    o, s, nc0, nc1 = section_arrays(info, sec, y)
    rc, rows, got = probe(lib, o, s, L, nc0, nc1)
    assert rc == 0
    sm, mn, mx = (block(info, rows[0], sec, k, ncols) for k in range(3))
    assert sm[c_inf] == -np.inf and mn[c_inf] == -np.inf, (sec, ncols, L)
    if c_nan >= 0:
        assert np.isnan(sm[c_nan]), (sec, ncols, L)
    if c_zero >= 0:
        assert bits(sm[c_zero:c_zero + 1])[0] == 0 and bits(mn[c_zero:c_zero + 1])[0] in (0, 1 << 63), (sec, ncols, L)
    plain = max(c_zero, 0)
    assert np.array_equal(mn[:plain], y[0, :, :plain].min(axis=0)) and np.array_equal(mx[:plain], y[0, :, :plain].max(axis=0))
    check_unwritten(got, rows[0], nc0, nc1)


def check_back_to_back(lib, sec, ncols, L, seed, model=False):
    """(f): six launches A, B, A, B, A, B through one partials buffer and one ticket, A and B different in every element: rows 0, 2,
    4 are the model of A bit for bit and rows 1, 3, 5 that of B (the host build: the rows of single launches); three launches
    of A alone give three identical rows"""
    info = constants(lib)
    rng = np.random.default_rng(seed)
    x = float_data(rng, 2, L, ncols)
    same = x[0] == x[1]
    x[1][same] += 1.0
    assert not np.any(x[0] == x[1])
    o, s, nc0, nc1 = section_arrays(info, sec, x)
    rc, rows, got = probe(lib, o, s, L, nc0, nc1, nsets=2, launches=6)
    assert rc == 0
    want = []
    for k in range(2):
        if model:
            want.append(bits(shape_model(info, x[k], sec)))
        else:
            ok, sk = (None if o is None else o[k:k + 1]), (None if s is None else s[k:k + 1])
            rc1, r1, _ = probe(lib, ok, sk, L, nc0, nc1)
            assert rc1 == 0
            want.append(bits(block(info, r1[0], sec, 0, ncols)).copy())
    for i in range(6):
        k = i % 2
        assert np.array_equal(bits(block(info, rows[i], sec, 0, ncols)), want[k]), (sec, ncols, L, i)
        assert np.array_equal(block(info, rows[i], sec, 1, ncols), x[k].min(axis=0)), (sec, ncols, L, i)
        assert np.array_equal(block(info, rows[i], sec, 2, ncols), x[k].max(axis=0)), (sec, ncols, L, i)
        check_unwritten(got, rows[i], nc0, nc1)
        assert np.array_equal(bits(rows[i]), bits(rows[k])), (sec, ncols, L, i)
    assert not np.any(want[0] == want[1])
    ok, sk = (None if o is None else o[:1]), (None if s is None else s[:1])
    rc, r3, got = probe(lib, ok, sk, L, nc0, nc1, launches=3)
    assert rc == 0
    assert np.array_equal(bits(r3[1]), bits(r3[0])) and np.array_equal(bits(r3[2]), bits(r3[0])), (sec, ncols, L)
    assert np.array_equal(bits(r3[0]), bits(rows[0]))


def check_fused(lib, nc1, L, seed):
    """sections 0 and 1 folded in one launch (what a resident iteration sends) give the bits of two launches"""
    info = constants(lib)
    rng = np.random.default_rng(seed)
    x0, x1 = float_data(rng, 1, L, info.out_slots), float_data(rng, 1, L, nc1)
    rc, both, got = probe(lib, x0, x1, L, info.out_slots, nc1)
    assert rc == 0
    check_unwritten(got, both[0], info.out_slots, nc1)
    rc, r0, _ = probe(lib, x0, None, L, info.out_slots, 0)
    assert rc == 0
    rc, r1, _ = probe(lib, None, x1, L, 0, nc1)
    assert rc == 0
    b = bits(both[0])
    assert np.array_equal(b[:info.stride], bits(r0[0])[:info.stride]), (nc1, L)
    assert np.array_equal(b[info.stride:], bits(r1[0])[info.stride:]), (nc1, L)


def check_refusals(lib):
    """every argument error: GPH_EARG, and the caller's rows are as they were"""
    info = constants(lib)
    L = 4
    o, s = np.ones((1, L, info.out_slots)), np.ones((1, L, info.cols))
    mark = 12345.0
    def refused(out0, stats1, L_, nc0, nc1, nsets=1, launches=1):
        rows = np.full((max(launches, 1), info.row), mark)
        rc, rows, _ = probe(lib, out0, stats1, L_, nc0, nc1, nsets=nsets, launches=launches, rows=rows)
        assert rc == EARG, (L_, nc0, nc1, nsets, launches, rc)
        assert np.all(rows == mark)
    refused(o, None, 0, 1, 0)
    refused(o, None, -1, 1, 0)
    refused(o, None, 2 ** 31, 1, 0)
    refused(o, None, 2 ** 40, 1, 0)
    refused(o, None, L, -1, 0)
    refused(o, s, L, -1, 4)
    refused(o, None, L, info.out_slots + 1, 0)
    refused(None, s, L, 0, -1)
    refused(o, s, L, 4, -1)
    refused(None, s, L, 0, info.cols + 1)
    refused(o, s, L, 0, 0)
    refused(None, s, L, 4, 0)
    refused(None, s, L, 4, 4)
    refused(o, None, L, 0, 4)
    refused(o, None, L, 4, 4)
    refused(o, None, L, 4, 0, nsets=0)
    refused(o, None, L, 4, 0, nsets=-1)
    refused(o, None, L, 4, 0, launches=0)
    refused(o, None, L, 4, 0, launches=-1)
    # and the same buffers are accepted when nothing is wrong
    rc, rows, got = probe(lib, o, s, L, 4, 4)
    assert rc == 0 and rows[0][0] == float(L) and rows[0][info.stride] == float(L)


def check_width(lib, sec, ncols, seed, model=False, loci=LOCI):
    """(a), (b), (c) on the device, (d), (e) for one width at every locus count of `loci`; (f) at the counts that fill more than one
    block and more than one step"""
    worst = 0.0
    for L in loci:
        check_integers(lib, sec, ncols, L, seed + L)
        worst = max(worst, check_floats(lib, sec, ncols, L, seed + 2 * L, model=model))
        check_extremes(lib, sec, ncols, L, seed + 3 * L)
    for L in loci:
        if L in (1, 257, 2049):
            check_back_to_back(lib, sec, ncols, L, seed + 5 * L, model=model)
    return worst
