// gph_ess.h -- effective sample sizes: the batch-sum levels one series keeps (gph_ess_add), their read-out and the
// autocorrelation estimate (host: gph_ess_read, gph_ess), and k_ess, which keeps the levels of M series per selected locus on
// the device over the samples taken (include/gphocs_hip.h, gph_engine_ess_*).
//
// The levels.  J = GPH_ESS_LEVELS.  One series x_0 .. x_S-1 owns a[2 + 2J] doubles: a[0] = shift = x_0, a[1] = s1,
// a[2 + j] = run[j] (run[0] stays 0), a[2 + J + j] = sq[j].  Sample t (0-based) brings d = x_t - shift (t = 0: every word is
// zeroed first, d = 0); plain uncontracted fp64, in this order:
//   s1 = s1 + d;  sq[0] = sq[0] + d * d;  carry = d;
//   for j = 1 .. J - 1:  run[j] = run[j] + carry;  if ((t + 1) mod 2^j != 0) stop;
//                        carry = run[j];  sq[j] = sq[j] + carry * carry;  run[j] = 0;
// so sq[j] is the sum of squares of the completed batch SUMS of 2^j consecutive samples (a batch sum is a pairwise sum), and a
// sample touches two levels on average.  gph_ess_add is ONE text: the kernel's lanes and the host run it.
//
// Read-out (gph_ess_read, host), level j, b = 2^j, nb = floor(S / b):
//   T  = s1 - (((run[1] + run[2]) + ...) + run[j])          (j = 0: T = s1; the samples behind the last complete batch)
//   vx = (sq[0] - s1 * s1 / S) / (S - 1)                     vb = (sq[j] - T * T / nb) / (nb - 1)
//   mean = shift + s1 / S      sd = sqrt(max(vx, 0))
//   vx <= 0 (the series never changed): tau = 0, ess = 0 -- a stuck locus does not read as perfectly mixed
//   else tau = vb / (b * vx), ess = S / tau capped at S; tau <= 0 (or fewer than two batches): ess = S
// level < 0: j* = the largest j < J with 4^j <= S (b <= sqrt(S)).  S < 2: mean as above, everything else 0.
// out5 = mean, sd, tau, ess, level.
//
// gph_ess(x, S, max_lag, out8) (host): the levels of x by gph_ess_add, read at j*, and Geyer's initial positive sequence:
//   d_t = x_t - x_0 (d_0 = 0)      m = s1 / S      e_t = d_t - m
//   c_k = (sum_{t = k}^{S - 1} e_t * e_{t - k}, t ascending, from 0.0) / S
//   Kmax = min(S - 2, max_lag), max_lag <= 0: 2000       G_i = c_{2i} + c_{2i + 1}, computed as the sum reaches them
//   sum = G_0 (always taken: c_1 exists for S >= 2); i = 1, 2, ...: 2i + 1 > Kmax -> truncated = 1, stop; G_i <= 0 -> stop;
//   sum = sum + G_i   (no monotone adjustment)
//   c_0 == 0: tauAcf = 0, essAcf = 0.  else tauAcf = 2 * sum / c_0 - 1, essAcf = S / tauAcf capped at S, tauAcf <= 0: S
//   out8 = mean, sd, tauBatch, essBatch, tauAcf, essAcf, level, truncated
//
// k_ess.  Per selected locus q, M = 5 series (+ 1 under locus-mut-rate VAR) in this order: dataLnL (fs[FS_DATALNL]), genLnL
// (fs[FS_GENLNL]), tmrca (age[root]), numMigs (IS_NUM_MIGS clamped as gph_an_num_migs clamps it), topo, rate (fs[FS_MUTRATE]).
// topo: at the first sample since the accumulators were zeroed the n - 1 clade keys of the locus (gph_clades.h: the clade of an
// internal node as W 64-bit words), in node-index order, are stored as its FOCAL SET; x_topo of a sample is the number of
// internal nodes of the current tree whose key is in the focal set (n - 1 at the first sample, never below 1: the root's
// clade).  topoChanges: H_t = the sum over the internal nodes of gph_cl_key's hash, mod 2^64; changes += (H_t != H_t-1) for
// t >= 1 (two different clade sets collide with probability about 2^-64).
// Device memory per selected locus: acc[M][2 + 2J] doubles, focal[n - 1][W] u64, prev u64, changes u32 -- 1.5 KB at 16 leaves.
//
// Shape, as k_clades: workgroup w takes the G = max(1, 256 / n) consecutive records w G ... of the selection; fathers and
// internal ages are staged with 128-bit loads (gph_cl_stage), lane (g, i) climbs from leaf i (gph_cl_climb); after a barrier
// lane (g, k) forms its key and hash (gph_cl_key) and compares the key with the n - 1 keys of the locus's focal set in HBM
// (at t = 0 it writes its key there instead) and leaves a hit flag and the hash in LDS; after a second barrier lane (g, m),
// m < M, forms x_m (the topo count is an integer sum: exact in any order) and runs gph_ess_add on acc[q][m], and lane (g, M)
// adds the hashes and updates prev / changes.  Every accumulator word has one owner lane: no fp atomics, no global atomics.
// A sample reads the node records and four scalars of a page and, per locus, the focal set ((n - 1)^2 W key compares a
// locus: 225 at 16 leaves) and about two levels of each series.
// LDS: k_clades' G (4 N + (n - 1) (8 + 8 W + 4)) bytes + G (n - 1) 8 for the hashes -- 8.5 KB at 16 leaves (G = 16), 11.7 KB
// at 200 (G = 1, W = 4).
//
// The kernel has one text (the flat-kernel form, gph_sampler.h).  It writes no page, draws no random number and touches no
// chain state.
#pragma once
#include <stdint.h>

#ifndef GPH_SM_FN            /* a host translation unit that wants the estimator alone (gph_mcmc.cpp, gph_readtrace.cpp) */
#define GPH_SM_FN static inline
#define GPH_ESS_HOST_ONLY
#endif

#define GPH_ESS_LEVELS 16
#define GPH_ESS_WORDS (2 + 2 * GPH_ESS_LEVELS)

GPH_SM_FN void gph_ess_add(double *a, int64_t t, double x)
{
  if (t == 0) {
    for (int i = 0; i < GPH_ESS_WORDS; i++) a[i] = 0.0;
    a[0] = x;
  }
  const double d = t == 0 ? 0.0 : x - a[0];
  a[1] = a[1] + d;
  a[2 + GPH_ESS_LEVELS] = a[2 + GPH_ESS_LEVELS] + d * d;
  double carry = d;
  for (int j = 1; j < GPH_ESS_LEVELS; j++) {
    a[2 + j] = a[2 + j] + carry;
    if (((t + 1) & (((int64_t)1 << j) - 1)) != 0) break;
    carry = a[2 + j];
    a[2 + GPH_ESS_LEVELS + j] = a[2 + GPH_ESS_LEVELS + j] + carry * carry;
    a[2 + j] = 0.0;
  }
}

#ifdef GPH_ESS_HOST_ONLY
#include <math.h>
#include <vector>

// j*: the largest j < J with 4^j <= S
static inline int32_t gph_ess_level_(int64_t S)
{
  int32_t j = 0;
  while (j + 1 < GPH_ESS_LEVELS && ((int64_t)1 << (2 * (j + 1))) <= S) j++;
  return j;
}

// gph_ess_read (include/gphocs_hip.h): out5 = mean, sd, tau, ess, level
static int gph_ess_read_(const double *a, int64_t S, int32_t level, double *out5)
{
  if (!a || !out5 || S < 0 || level >= GPH_ESS_LEVELS) return GPH_EARG;
  const int32_t j = level < 0 ? gph_ess_level_(S) : level;
  for (int i = 0; i < 5; i++) out5[i] = 0.0;
  out5[4] = (double)j;
  if (S < 1) return 0;
  const double s1 = a[1], n = (double)S;
  out5[0] = a[0] + s1 / n;
  if (S < 2) return 0;
  const double vx = (a[2 + GPH_ESS_LEVELS] - s1 * s1 / n) / (double)(S - 1);
  out5[1] = sqrt(vx > 0.0 ? vx : 0.0);
  if (!(vx > 0.0)) return 0;                   /* the series never changed: tau = 0, ess = 0 */
  const int64_t b = (int64_t)1 << j, nb = S / b;
  double tau = 0.0;
  if (nb >= 2) {
    double tail = 0.0;
    for (int i = 1; i <= j; i++) tail = tail + a[2 + i];
    const double T = j == 0 ? s1 : s1 - tail;
    const double vb = (a[2 + GPH_ESS_LEVELS + j] - T * T / (double)nb) / (double)(nb - 1);
    tau = vb / ((double)b * vx);
  }
  double ess = n;
  if (tau > 0.0) { ess = n / tau; if (ess > n) ess = n; }
  out5[2] = tau; out5[3] = ess;
  return 0;
}

// gph_ess (include/gphocs_hip.h): out8 = mean, sd, tauBatch, essBatch, tauAcf, essAcf, level, truncated
static int gph_ess_(const double *x, int64_t S, int32_t max_lag, double *out8)
{
  if (!x || !out8 || S < 2) return GPH_EARG;
  double a[GPH_ESS_WORDS], r[5];
  for (int64_t t = 0; t < S; t++) gph_ess_add(a, t, x[t]);
  { int rc = gph_ess_read_(a, S, -1, r); if (rc) return rc; }
  const double n = (double)S, m = a[1] / n;
  std::vector<double> e((size_t)S);
  for (int64_t t = 0; t < S; t++) e[(size_t)t] = (t == 0 ? 0.0 : x[t] - x[0]) - m;
  auto cov = [&](int64_t k) {
    double s = 0.0;
    for (int64_t t = k; t < S; t++) s = s + e[(size_t)t] * e[(size_t)(t - k)];
    return s / n;
  };
  const int64_t lag = max_lag <= 0 ? 2000 : max_lag, Kmax = S - 2 < lag ? S - 2 : lag;
  const double c0 = cov(0);
  double sum = c0 + cov(1), truncated = 0.0;
  for (int64_t i = 1;; i++) {
    if (2 * i + 1 > Kmax) { truncated = 1.0; break; }
    const double G = cov(2 * i) + cov(2 * i + 1);
    if (!(G > 0.0)) break;
    sum = sum + G;
  }
  double tau = 0.0, ess = 0.0;
  if (c0 != 0.0) {
    tau = 2.0 * sum / c0 - 1.0;
    ess = n;
    if (tau > 0.0) { ess = n / tau; if (ess > n) ess = n; }
  }
  out8[0] = r[0]; out8[1] = r[1]; out8[2] = r[2]; out8[3] = r[3];
  out8[4] = tau; out8[5] = ess; out8[6] = r[4]; out8[7] = truncated;
  return 0;
}
#undef GPH_ESS_HOST_ONLY
#undef GPH_SM_FN
#else
#include "gph_ancestry.h"
#include "gph_clades.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 12

#define GPH_ES_MAXSERIES 6
enum { ES_DATALNL = 0, ES_GENLNL, ES_TMRCA, ES_NUMMIGS, ES_TOPO, ES_RATE };

GPH_SM_HD int32_t gph_es_lds_bytes(const GphLayout &y, const GphClShape &h) { return h.lds_bytes + h.G * (y.n > 1 ? y.n - 1 : 0) * 8; }

// the LDS of a workgroup: k_clades' arrays (cl.miss holds the HIT flags here: 1 = the node's key is in the focal set) behind
// the hashes of the internal nodes ([G][n - 1], first: 8-byte aligned whatever G and N are)
struct GphEsLds {
  uint64_t *hash;
  GphClLds cl;
};
GPH_SM_FN void gph_es_carve(char *base, const GphLayout &y, const GphClShape &h, GphEsLds &s)
{
  s.hash = (uint64_t *)base;
  gph_cl_carve(base + (size_t)h.G * (y.n - 1) * 8, y, h, s.cl);
}

// lane (g, k): internal node n + k against the focal set of its locus (first: the set is written instead)
GPH_SM_FN void gph_es_lookup(const GphEsLds &s, const GphLayout &y, const GphClShape &h, int g, int k, uint64_t *focal, bool first)
{
  const int ni = y.n - 1, c = GPH_IX(g * ni + k, h.G * ni);
  uint64_t key[GPH_CL_MAXW];
  s.hash[c] = gph_cl_key(s.cl, y, h, g, k, key);
  bool hit = first;
  if (first) {
    for (int w = 0; w < GPH_CL_MAXW; w++)
      if (w < h.W) focal[GPH_IX(k * h.W + w, ni * h.W)] = key[w];
  } else {
    for (int f = 0; f < ni && !hit; f++) {
      bool same = true;
      for (int w = 0; w < GPH_CL_MAXW; w++)
        if (w < h.W) same = same && focal[GPH_IX(f * h.W + w, ni * h.W)] == key[w];
      hit = same;
    }
  }
  s.cl.miss[c] = hit ? 1u : 0u;
}

// lane (g, m): series m of the locus in page pg
GPH_SM_FN double gph_es_value(const GphEsLds &s, const GphLayout &y, const GphClShape &h, int g, int m, const char *pg)
{
  const double *fs = (const double *)(pg + y.o_fscal);
  const int ni = y.n - 1;
  if (m == ES_DATALNL) return fs[FS_DATALNL];
  if (m == ES_GENLNL) return fs[FS_GENLNL];
  if (m == ES_RATE) return fs[FS_MUTRATE];
  if (m == ES_NUMMIGS) return (double)gph_an_num_migs(pg, y);
  if (m == ES_TMRCA) {
    const int root = ((const int32_t *)(pg + y.o_iscal))[IS_ROOT];
    return s.cl.age[GPH_IX(g * ni + GPH_IX(root - y.n, ni), h.G * ni)];
  }
  uint32_t hits = 0;
  for (int k = 0; k < ni; k++) hits += s.cl.miss[GPH_IX(g * ni + k, h.G * ni)];
  return (double)hits;
}

// one lane a locus: H_t, and whether it differs from H_t-1
GPH_SM_FN void gph_es_changes(const GphEsLds &s, const GphLayout &y, const GphClShape &h, int g, bool first, uint64_t *prev, uint32_t *changes)
{
  const int ni = y.n - 1;
  uint64_t H = 0;
  for (int k = 0; k < ni; k++) H += s.hash[GPH_IX(g * ni + k, h.G * ni)];
  if (!first && H != *prev) *changes = *changes + 1u;
  *prev = H;
}

// workgroup w = block bx; t: samples taken since the accumulators were zeroed; acc [nsel][M][GPH_ESS_WORDS], focal
// [nsel][n - 1][W], prev [nsel], changes [nsel]
GPH_FLAT(k_ess, GPH_CL_THREADS, GphLayout y, GphClShape h, const char *pages, const int32_t *sel_slot, int nsel, int L, int M, long long t,
         double *acc, uint64_t *focal, uint64_t *prev, uint32_t *changes)
{
  GPH_FLAT_BODY(GphNoLane);
  const int n = y.n, N = y.N, ni = n - 1, w = bx;
  if (ni < 1) return;
  GphEsLds s;
  gph_es_carve(lds, y, h, s);
  GPH_PHASE {
    for (int u = tid; u < h.G * ni * 2 * h.W; u += bd) s.cl.mask[GPH_IX(u, h.G * ni * 2 * h.W)] = 0u;
    for (int u = tid; u < h.G * N; u += bd) {
      const int g = u / N, v = u - g * N, j = gph_cl_slot(h, sel_slot, nsel, L, w, g);
      if (j >= 0) {
        GphNode rec;
        gph_copy16(&rec, pages + (size_t)j * y.page_bytes + y.o_nd + (size_t)v * 16);
        gph_cl_stage(s.cl, y, h, g, v, &rec);
      }
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < h.G * n; u += bd) {
      const int g = u / n, i = u - g * n;
      if (w * h.G + g < nsel) gph_cl_climb(s.cl, y, h, g, i);
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < h.G * ni; u += bd) {
      const int g = u / ni, k = u - g * ni, q = w * h.G + g;
      if (q < nsel) gph_es_lookup(s, y, h, g, k, focal + (size_t)q * ni * h.W, t == 0);
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < h.G * (M + 1); u += bd) {
      const int g = u / (M + 1), m = u - g * (M + 1), j = gph_cl_slot(h, sel_slot, nsel, L, w, g);
      if (j < 0) continue;
      const int q = w * h.G + g;
      if (m == M) gph_es_changes(s, y, h, g, t == 0, prev + GPH_IX(q, nsel), changes + GPH_IX(q, nsel));
      else gph_ess_add(acc + ((size_t)q * M + GPH_IX(m, M)) * GPH_ESS_WORDS, (int64_t)t, gph_es_value(s, y, h, g, m, pages + (size_t)j * y.page_bytes));
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
#endif
