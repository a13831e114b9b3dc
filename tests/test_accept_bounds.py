"""The sweep's accept test decided by bounds (gph_accept, g-phocs_amd/csrc/gph_math.h) takes exactly the decisions of the plain
`u < gph_exp(x)` for x < 0: more than 10^7 pairs through the host build of the engine sources (the debug entry next to the
math probe), aimed at where a bound could be wrong -- u within a few ulps of gph_exp(x) and of the two polynomial thresholds --
and 4 096 pairs on the device (-m gpu)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

M = 2.0 ** -40
ONE_BITS = int(np.array(1.0).view(np.int64))
DP = C.POINTER(C.c_double)


def run_entry(lib, x, u):
    """gph_accept(u, x), u < gph_exp(x), the bounds' verdict (0 undecided, 1 not below, 2 below)"""
    x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    n = len(x)
    out = np.zeros(3 * n)
    fn = lib.gph_debug_accept_
    fn.argtypes = [DP, DP, C.c_int32, DP, C.c_int32]
    assert fn(x.ctypes.data_as(DP), u.ctypes.data_as(DP), n, out.ctypes.data_as(DP), 0) == 0
    return out.reshape(3, n)


def exp_of(lib, x):
    """gph_exp(x) as the library evaluates it (bit-identical to glibc's: tests/test_math_vs_glibc.py)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    out = np.zeros(5 * n)
    assert lib.gph_debug_math(x.ctypes.data_as(DP), np.ones(n).ctypes.data_as(DP), n, out.ctypes.data_as(DP), 0) == 0
    return out[:n]


def thresholds(x):
    """the u at which each bound switches: (1 + m) / q and c / (1 + m), q and c as the fused Horner forms of gph_math.h
    (extended precision stands in for the fused operations: within an ulp, and the neighbourhoods below are +-8)"""
    with np.errstate(all="ignore"):
        xl = x.astype(np.longdouble)
        yl = -xl
        q = ((yl * (yl * np.longdouble(0.5) + 1).astype(np.float64) + 1)).astype(np.float64)
        a = (xl * np.longdouble(1.0 / 6.0) + np.longdouble(0.5)).astype(np.float64)
        b = (xl * a + 1).astype(np.float64)
        c = (xl * b + 1).astype(np.float64)
        return (1.0 + M) / q, c / (1.0 + M)


def around(v, k=8):
    """the doubles within +-k ulps of v, kept inside [0, 1): [len(v)][2k + 1]"""
    with np.errstate(all="ignore"):
        v = np.where(np.isfinite(v), np.clip(v, 0.0, 1.0), 0.0)
    bits = v.view(np.int64)[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]
    return np.clip(bits, 0, ONE_BITS - 1).view(np.float64)


def pairs_near_the_edges(lib, x):
    e = exp_of(lib, x)
    ur, ua = thresholds(x)
    u = np.concatenate([around(e), around(ur), around(ua)], axis=1)
    return np.repeat(x, u.shape[1]), u.ravel()


SPECIAL_X = np.array([-np.inf, np.nan, -0.0, -5e-324, -1e-320, -2.2250738585072014e-308, -1.1e-308, -745.0, -745.14, -746.0,
                      -708.0, -708.4, -709.0, -1e300, -1.7e308, -2.0, -1.0, -1.5960716379833215, -1e-12, -1e-17])
SPECIAL_U = np.array([0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 0.25, 0.5, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -41, 1.0 - 2.0 ** -39])


def special_pairs():
    return np.repeat(SPECIAL_X, len(SPECIAL_U)), np.tile(SPECIAL_U, len(SPECIAL_X))


@pytest.fixture(scope="module")
def host_lib():
    import run_hostemu as R
    import gphocs_amd as G
    return G.load_library(R.build_hostemu())


def undecided_cap(n):
    """share of uniform (x in [-10, 0], u in [0, 1)) pairs neither bound decides, from the bounds themselves: the strip between
    1 / (1 + y + y^2/2) and max(0, 1 - y + y^2/2 - y^3/6), y = -x:  integral of the first over [0, 10] = 2 (atan 11 - pi/4),
    of the second r - r^2/2 + r^3/6 - r^4/24 up to its root r; the margins m = 2^-40 widen the strip by less than 10^-11.
    + five standard deviations of a share counted on n pairs"""
    r = [z.real for z in np.roots([-1.0 / 6.0, 0.5, -1.0, 1.0]) if abs(z.imag) < 1e-12][0]
    p = (2.0 * (np.arctan(11.0) - np.pi / 4.0) - (r - r ** 2 / 2 + r ** 3 / 6 - r ** 4 / 24)) / 10.0 + 1e-10
    assert 0.065 < p < 0.067
    return p + 5.0 * np.sqrt(p * (1 - p) / n)


def test_same_decisions_as_the_plain_form(host_lib):
    rng = np.random.default_rng(20261020)
    total = 0
    sx, su = special_pairs()
    got = run_entry(host_lib, sx, su)
    assert np.array_equal(got[0], got[1]), "special values"
    total += len(sx)
    # x = -inf: the reject bound fires for u > 0; u = 0 and a NaN x fall through to the exact path
    inf = np.isneginf(sx)
    assert np.all(got[2][inf & (su > 0)] == 1) and np.all(got[2][inf & (su == 0)] == 0) and np.all(got[2][np.isnan(sx)] == 0)
    assert np.all(got[0][np.isnan(sx)] == 0)
    # the edges of every special x too
    ex, eu = pairs_near_the_edges(host_lib, SPECIAL_X)
    got = run_entry(host_lib, ex, eu)
    assert np.array_equal(got[0], got[1]), "edges of the special values"
    total += len(ex)
    for chunk in range(5):
        # x log-uniform in [-745, -1e-12]; per x the 51 u next to gph_exp(x) and to both thresholds, and 5 uniform ones
        x = -np.exp(rng.uniform(np.log(1e-12), np.log(745.0), 40000))
        ex, eu = pairs_near_the_edges(host_lib, x)
        ux, uu = np.repeat(x, 5), rng.random(5 * len(x))
        uu[::97] = 0.0
        xs, us = np.concatenate([ex, ux]), np.concatenate([eu, uu])
        got = run_entry(host_lib, xs, us)
        bad = np.flatnonzero(got[0] != got[1])
        assert len(bad) == 0, (xs[bad[:5]], us[bad[:5]], got[:, bad[:5]])
        # a verdict of the bounds is never against the plain form (the same statement, seen from the bounds)
        assert np.all(got[1][got[2] == 1] == 0) and np.all(got[1][got[2] == 2] == 1)
        total += len(xs)
    assert total >= 10_000_000, total


def test_share_the_bounds_leave_undecided(host_lib):
    rng = np.random.default_rng(7)
    n = 1_000_000
    x, u = -rng.uniform(0.0, 10.0, n), rng.random(n)
    got = run_entry(host_lib, x, u)
    assert np.array_equal(got[0], got[1])
    share = float(np.mean(got[2] == 0))
    print(f"undecided {share:.5f}, cap {undecided_cap(n):.5f}")
    assert share <= undecided_cap(n)


@pytest.mark.gpu
def test_device_decisions():
    """the same entry on the device, 4 096 pairs: special values, edges, uniform pairs; against the device's own plain form and
    against u < exp(x) of the C library"""
    import torch       # first, as the other device tests do: its HIP runtime has to be the one the process starts with
    assert torch.cuda.is_available(), "this test needs the MI355X"
    import gphocs_amd as G
    G.build()
    lib = G.load_library()
    rng = np.random.default_rng(11)
    x = np.concatenate([SPECIAL_X, -np.exp(rng.uniform(np.log(1e-12), np.log(745.0), 44))])
    ex, eu = pairs_near_the_edges(lib, x)            # 64 x 51 = 3 264
    sx, su = special_pairs()                         # 180
    n_u = 4096 - len(ex) - len(sx)
    ux, uu = -rng.uniform(0.0, 10.0, n_u), rng.random(n_u)
    xs, us = np.concatenate([ex, sx, ux]), np.concatenate([eu, su, uu])
    assert len(xs) == 4096
    got = run_entry(lib, xs, us)
    assert np.array_equal(got[0], got[1])
    libm = C.CDLL("libm.so.6")
    libm.exp.restype, libm.exp.argtypes = C.c_double, [C.c_double]
    with np.errstate(all="ignore"):
        ref = np.array([u < libm.exp(v) for v, u in zip(xs, us)], dtype=np.float64)
    assert np.array_equal(got[0], ref)
    assert np.mean(got[2][len(ex) + len(sx):] == 0) < 0.12       # the bounds are at work on the device (expected share 0.066)
