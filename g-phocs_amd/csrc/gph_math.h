// gph_math.h -- fp64 exp()/log() for the device that are BIT-IDENTICAL to the libm the
// reference links (glibc 2.35, x86-64 FMA variants __exp_fma / __log_fma).
//
// Why: G-PhoCS proposes a node age as reflect(t + finetune * N(0,1), lo, hi) with
// finetune (0.01) three orders of magnitude above the age window (1e-5): a 1-ulp
// difference in log() inside rndnormal (utils.c:459-472) becomes ~1e-13 relative in the
// age, and the summed log-likelihood drifts past 1e-10 within ~10 iterations.  The
// acceptance bar is 1e-10 relative against the reference for identical RNG streams, so
// the device evaluates exp/log with the same algorithm (Arm Optimized Routines exp/log,
// 128-entry tables, degree-5 polynomials), the same constants (gph_libm_tables.h, read
// from this image's libm) and the SAME fused-multiply-add placement as the compiled glibc
// code (transcribed from its instruction stream; every __builtin_fma below is one vfmadd,
// every other operation is an unfused IEEE operation; -ffp-contract=off).
// tests/test_math_vs_glibc.py checks bit-identity against glibc on millions of inputs.
#pragma once
#include <stdint.h>
#include "gph_libm_tables.h"
#include "gph_types.h"

#ifdef __HIPCC__
#define GPH_MATH_FN __host__ __device__ inline
#define GPH_MATH_TAB __device__ __constant__ static const
#else
#define GPH_MATH_FN static inline
#define GPH_MATH_TAB static const
#endif

// tables live in constant memory: the chain logic indexes them wave-uniformly (scalar
// loads); the per-pattern log() in the root reduction gathers through the vector L1
#ifdef __HIPCC__   /* both passes: the host side takes the tables' device addresses (hipGetSymbolAddress) */
__device__ __constant__ static const uint64_t gph_exp_t_d[256] = GPH_EXP_TAB;
__device__ __constant__ static const double gph_log_t_d[256] = GPH_LOG_TAB;
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// The polynomial / reduction constants and the table base addresses are READ from the kernel-argument segment
// (GphKargs, first argument of every kernel): a compile-time constant would be folded into the instruction stream as
// two 32-bit scalar moves per use (36 s_mov_b32 per log) and a __constant__ symbol costs a pc-relative (GOT) address
// computation per access, while the scalar unit is the scarce issue slot of the chain kernels; off the kernarg
// pointer the constants of one call arrive in a few wide scalar loads.
typedef __attribute__((address_space(4))) const double gph_cdbl;
typedef __attribute__((address_space(4))) const uint64_t gph_cu64;
#define GPH_KA ((__attribute__((address_space(4))) const GphKargs *)__builtin_amdgcn_kernarg_segment_ptr())
#define GPH_EXPC (&GPH_KA->mathc[0])
#define GPH_LOGC (&GPH_KA->mathc[8])
#define GPH_RNGC (&GPH_KA->mathc[26])
#define GPH_EXPT ((gph_cu64 *)GPH_KA->exp_t)
#define GPH_LOGT ((gph_cdbl *)GPH_KA->log_t)
#else
static const double gph_exp_c_h[8] = GPH_EXP_CONSTS;
static const uint64_t gph_exp_t_h[256] = GPH_EXP_TAB;
static const double gph_log_c_h[18] = GPH_LOG_CONSTS;
static const double gph_log_t_h[256] = GPH_LOG_TAB;
#define GPH_EXPC gph_exp_c_h
#define GPH_EXPT gph_exp_t_h
#define GPH_LOGC gph_log_c_h
#define GPH_LOGT gph_log_t_h
#endif

GPH_MATH_FN uint64_t gph_asu64(double x) { union { double d; uint64_t u; } v; v.d = x; return v.u; }
GPH_MATH_FN double gph_asf64(uint64_t u) { union { double d; uint64_t u; } v; v.u = u; return v.d; }

#if defined(__HIP_DEVICE_COMPILE__)
#define GPH_UIDX(i) (UNIFORM ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(i)) : (uint32_t)(i))
#else
#define GPH_UIDX(i) ((uint32_t)(i))
#endif
// UNIFORM = the argument is the same in every lane (chain logic): the table index goes through
// an SGPR so the two table words come from scalar loads instead of a vector gather
template <bool UNIFORM>
GPH_MATH_FN double gph_exp_t(double x)
{
  const auto *EC = GPH_EXPC;
  const double InvLn2N = EC[0], Shift = EC[1], NegLn2hiN = EC[2], NegLn2loN = EC[3];
  const double C2 = EC[4], C3 = EC[5], C4 = EC[6], C5 = EC[7];
  uint64_t ix = gph_asu64(x);
  uint32_t abstop = (uint32_t)(ix >> 52) & 0x7ff;
  if (abstop - 0x3c9u > 0x3eu) {
    if ((int32_t)(abstop - 0x3c9u) < 0) return 1.0 + x;          /* |x| < 2^-54 */
    if (abstop > 0x408u) {                                         /* |x| >= 1024, inf, nan */
      if (ix == 0xfff0000000000000ull) return 0.0;
      if (abstop == 0x7ffu) return 1.0 + x;
      if (ix >> 63) return 0.0;                                    /* underflow */
      return gph_asf64(0x7ff0000000000000ull);                     /* overflow */
    }
    abstop = 0;                                                    /* 512 <= |x| < 1024 */
  }
  double kds = __builtin_fma(x, InvLn2N, Shift);
  uint64_t ki = gph_asu64(kds);
  double kd = kds - Shift;
  double r = __builtin_fma(kd, NegLn2hiN, x);
  r = __builtin_fma(kd, NegLn2loN, r);
  uint32_t idx = GPH_UIDX(2 * (uint32_t)(ki & 0x7f));
  uint64_t top = ki << 45;
  double tail = gph_asf64(GPH_EXPT[idx]);
  uint64_t sbits = GPH_EXPT[idx + 1] + top;
  double p23 = __builtin_fma(r, C3, C2);
  double tr = r + tail;
  double r2 = r * r;
  double p45 = __builtin_fma(r, C5, C4);
  double t = __builtin_fma(p23, r2, tr);
  double r4 = r2 * r2;
  double tmp = __builtin_fma(r4, p45, t);
  if (abstop == 0) {
    /* specialcase(): the exponent of scale may have over/underflowed */
    if ((ki & 0x80000000ull) == 0) {
      sbits += 0xc0f0000000000000ull;                              /* -= 1009 << 52 */
      double scale = gph_asf64(sbits);
      double y = __builtin_fma(scale, tmp, scale);
      return y * 0x1p1009;
    }
    sbits += 0x3fe0000000000000ull;                                /* += 1022 << 52 */
    double scale = gph_asf64(sbits);
    double t1 = tmp * scale;
    double y = scale + t1;
    if (1.0 > y) {
      double hi = y + 1.0;
      double lo = scale - y;
      lo = lo + t1;
      double b = 1.0 - hi;
      b = b + y;
      b = b + lo;
      y = b + hi;
      y = y - 1.0;
      if (y == 0.0) y = 0.0;
    }
    return y * 0x1p-1022;
  }
  double scale = gph_asf64(sbits);
  return __builtin_fma(scale, tmp, scale);
}

GPH_MATH_FN double gph_exp(double x) { return gph_exp_t<false>(x); }
GPH_MATH_FN double gph_exp_u(double x) { return gph_exp_t<true>(x); }

// The Metropolis test `u < exp(x)` for x < 0, 0 <= u < 1, with EXACTLY the decisions of `u < gph_exp(x)`: two polynomial
// bounds decide most pairs in a dozen instructions, the rest evaluates gph_exp as before.  m = 2^-40, y = -x > 0,
// E = gph_exp(x), |E - e^x| < 1 ulp of e^x (glibc's exp stays below 0.52 ulp).  q and c below are the COMPUTED values.
//   reject:  q = fma(y, fma(y, 1/2, 1), 1): every term is positive, two roundings: q <= (1 + y + y^2/2) (1 + 2^-51)
//     <= e^y (1 + 2^-51).  fl(u q) >= 1 + m gives u q >= (1 + m) (1 - 2^-53), u >= e^x (1 + m) (1 - 2^-53) / (1 + 2^-51)
//     > e^x (1 + m/2), and E <= e^x (1 + 2^-52) where e^x is normal: u > E.  Where e^x is subnormal, E is one of the two
//     grid points next to it and u > e^x is a double too: u >= the grid point above e^x >= E.  Not (u < E) either way.
//     y = inf (x = -inf) or y^2 overflowing: q = inf, u q = inf for u > 0: reject, and E = 0.  u = 0: fl(0 q) is 0, or NaN
//     for q = inf: undecided.
//   accept:  T(x) = 1 + x + x^2/2 + x^3/6 <= e^x for x < 0 (Lagrange remainder e^xi x^4 / 24 >= 0, x < xi < 0), c = fma(x,
//     fma(x, fma(x, S, 1/2), 1), 1) with S = fl(1/6).  fl(u (1 + m)) < c gives u < c / ((1 + m) (1 - 2^-53)) < c (1 - m/2)
//     (u (1 + m) subnormal: u < 2^-1022 < E below, where c > 0 needs y <= 2).
//     y <= 2: the Horner values are 1/2 - y/6 in [1/6, 1/2], 1 - y (..) in [5/8, 1], 1 - y (..) in [-1/3, 1]: three roundings
//       of at most 2^-53 each, carried through factors y <= 2, and S off by 2^-56: |c - T| < 16 * 2^-53 = 2^-49.  For y <= 1
//       T >= 1/3, so c (1 - m/2) <= T + 2^-49 - 2^-43 < T (1 - 2^-52) <= e^x (1 - 2^-52) <= E.  For 1 < y <= 2 the remainder is
//       >= e^-2 / 24 > 2^-8: c (1 - m/2) <= c < T + 2^-49 < e^x - 2^-9 < E (c > 0 here: with c <= 0 the compare cannot hold
//       for u >= 0, nothing is decided).
//     y > 2: T <= T(-2) = -1/3 and T <= -y^3 / 24 (y^3/8 - y^2/2 + y - 1 is 0 at y = 2 and grows), while |c - T| <
//       2^-50 (1 + y + y^2 + y^3) < 2^-44 |T|: c < 0 <= u (c = -inf once y^3 overflows; x = -inf: 1/2 + x S = -inf, times
//       x = +inf, 1 + that = +inf, times x = -inf): undecided.
//   NaN x: q and c are NaN, both compares false: gph_exp decides, as it did.
// UNIFORM: wave-uniform arguments (chain logic), the compares are tested as lane masks on the scalar unit -- UNI of gph_rt.h,
// which includes this header and is not defined yet down here; GPH_UCMP is local to the functions below.
// CONTRACT: x < 0 (or NaN, -0.0) and 0 <= u < 1.  For x > 0 the polynomials bound nothing and the answer may be wrong: a
// caller handles x >= 0 before it draws u, as l_accept (gph_locus.h) does.
#if defined(__HIP_DEVICE_COMPILE__)
#define GPH_UCMP(c) (UNIFORM ? __builtin_amdgcn_ballot_w64((bool)(c)) != 0 : (bool)(c))
#else
#define GPH_UCMP(c) ((bool)(c))
#endif
#define GPH_ACC_M 0x1p-40
// 0: gph_exp has to decide, 1: certainly not below, 2: certainly below
template <bool UNIFORM>
GPH_MATH_FN int gph_accept_bounds_t(double u, double x)
{
  const double y = -x;
  const double q = __builtin_fma(y, __builtin_fma(y, 0.5, 1.0), 1.0);
  if (GPH_UCMP(u * q >= 1.0 + GPH_ACC_M)) return 1;
  const double c = __builtin_fma(x, __builtin_fma(x, __builtin_fma(x, 1.0 / 6.0, 0.5), 1.0), 1.0);
  if (GPH_UCMP(u * (1.0 + GPH_ACC_M) < c)) return 2;
  return 0;
}
template <bool UNIFORM>
GPH_MATH_FN bool gph_accept_t(double u, double x)
{
  const int b = gph_accept_bounds_t<UNIFORM>(u, x);
  if (b) return b == 2;
  return GPH_UCMP(u < gph_exp_t<UNIFORM>(x));
}
GPH_MATH_FN bool gph_accept(double u, double x) { return gph_accept_t<false>(u, x); }
GPH_MATH_FN bool gph_accept_u(double u, double x) { return gph_accept_t<true>(u, x); }
#undef GPH_UCMP
#undef GPH_ACC_M

template <bool UNIFORM>
GPH_MATH_FN double gph_log_t(double x)
{
  const auto *LC = GPH_LOGC;
  const double Ln2hi = LC[0], Ln2lo = LC[1];
  const double A0 = LC[2], A1 = LC[3], A2 = LC[4], A3 = LC[5], A4 = LC[6];
  uint64_t ix = gph_asu64(x);
  uint32_t top = (uint32_t)(ix >> 48);
  if (ix - 0x3fee000000000000ull <= 0x308ffffffffffull) {
    /* x within [1 - 2^-4, 1 + 0x1.09p-4): dedicated polynomial, log(1) == 0 exactly */
    const double B0 = LC[7], B1 = LC[8], B2 = LC[9], B3 = LC[10], B4 = LC[11],
                 B5 = LC[12], B6 = LC[13], B7 = LC[14], B8 = LC[15], B9 = LC[16],
                 B10 = LC[17];
    if (ix == 0x3ff0000000000000ull) return 0.0;
    double r = x - 1.0;
    double q1 = __builtin_fma(r, B2, B1);
    double q4 = __builtin_fma(r, B5, B4);
    double r2 = r * r;
    double q7 = __builtin_fma(r, B8, B7);
    q1 = __builtin_fma(r2, B3, q1);
    q4 = __builtin_fma(r2, B6, q4);
    double r3 = r * r2;
    double p = __builtin_fma(r2, B9, q7);
    p = __builtin_fma(r3, B10, p);
    p = __builtin_fma(p, r3, q4);
    p = __builtin_fma(p, r3, q1);
    double rw = __builtin_fma(r, 0x1p27, r);
    double rhi = __builtin_fma(-0x1p27, r, rw);
    double rhi2 = rhi * rhi;
    double rlo = r - rhi;
    double hi = __builtin_fma(rhi2, B0, r);
    double rmh = r - hi;
    double rs = r + rhi;
    double lo = __builtin_fma(rhi2, B0, rmh);
    double brl = B0 * rlo;
    lo = __builtin_fma(brl, rs, lo);
    double y = __builtin_fma(p, r3, lo);
    return hi + y;
  }
  if (top - 0x10u > 0x7fdfu) {
    if (ix * 2 == 0) return -gph_asf64(0x7ff0000000000000ull);   /* log(0) = -inf */
    if (ix == 0x7ff0000000000000ull) return x;                     /* log(inf) */
    if ((top & 0x8000u) || (top & 0x7ff0u) == 0x7ff0u) return gph_asf64(0x7ff8000000000000ull); /* x < 0, nan */
    ix = gph_asu64(x * 0x1p52);                                    /* subnormal: normalise */
    ix += 0xfcc0000000000000ull;                                   /* -= 52 << 52 */
  }
  uint64_t tmp = ix + 0xc01a000000000000ull;                       /* ix - OFF */
  uint32_t i = GPH_UIDX((uint32_t)(tmp >> 45) & 0x7f);
  int32_t k = (int32_t)((int64_t)tmp >> 52);
  uint64_t iz = ix - (tmp & 0xfff0000000000000ull);
  double kd = (double)k;
  double z = gph_asf64(iz);
  double invc = GPH_LOGT[2 * i], logc = GPH_LOGT[2 * i + 1];
  double r = __builtin_fma(z, invc, -1.0);
  double w = __builtin_fma(kd, Ln2hi, logc);
  double q12 = __builtin_fma(r, A2, A1);
  double hi = r + w;
  double r2 = r * r;
  double lo = w - hi;
  lo = lo + r;
  lo = __builtin_fma(kd, Ln2lo, lo);
  double r3 = r * r2;
  double q34 = __builtin_fma(r, A4, A3);
  lo = __builtin_fma(r2, A0, lo);
  q34 = __builtin_fma(q34, r2, q12);
  double y = __builtin_fma(r3, q34, lo);
  return y + hi;
}
GPH_MATH_FN double gph_log(double x) { return gph_log_t<false>(x); }
GPH_MATH_FN double gph_log_u(double x) { return gph_log_t<true>(x); }
