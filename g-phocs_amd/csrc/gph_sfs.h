// gph_sfs.h -- k_sfs_tree and k_sfs_data: the site-frequency spectrum of every current population and the split of the
// variable sites of two populations into private, shared and fixed (Wakeley & Hey 1997) -- what the sampled genealogies expect
// (Fu 1995: the branch length under each frequency class) against what the data show; per selected locus and genome-wide per
// sample, on the device (include/gphocs_hip.h, gph_engine_sfs_*).
//
// Definitions.  Populations: the Kc CURRENT populations in model order; leaf i belongs to pop[i], n_p = the leaves of p.
//   SLOTS (NS)   for every p with n_p >= 2, in population order, the folded bins k = 1 .. n_p / 2 ("sfs_<p>:<k>"); then for every
//                pair P < Q taken (default: all with n_P, n_Q >= 1, lexicographic) the four classes privP, privQ, shared, fixed
//   GROUPS (NG)  what shares a denominator: one per population with bins, then one per pair
// Genealogy side, one locus at one sample: every non-root node v in node-index order, len_v = age[father v] - age[v] (leaf ages
// are the records': an ancient sample's branch starts at its age), c_v[p] = the leaves of p under v.
//   v is in sfs_p:k iff 0 < c_v[p] < n_p and min(c_v[p], n_p - c_v[p]) = k (c = n_p / 2 at even n_p: bin n_p / 2, once)
//   a = c_v[P], b = c_v[Q], "a inside" = 0 < a < n_P:  privP iff a inside and b in {0, n_Q};  privQ iff b inside and a in
//   {0, n_P};  shared iff both inside;  fixed iff (a, b) = (n_P, 0) or (0, n_Q);  else none of the four
//   per slot x = sum len_v over its nodes, plain uncontracted fp64 adds in node order from 0.0; e = rate x, one multiply
//   (rate = FS_MUTRATE of the page): the expected substitutions PER SITE that fall in the class.
// Data side, one locus, once at enable: a COLUMN is a row with a non-zero phase word and stands for `count` sites
// (gph_predictive.h); the codes are those of the column's own row (both haplotypes of a diploid lie in one population: the counts
// of a population do not depend on the phase row read).
//   p is USABLE at a column iff all n_p leaves have a code below 4 and show two distinct bases at most: use_p += count, and with
//   k >= 1 carriers of the rarer base obs[sfs_p:k] += count
//   a pair is usable iff all leaves of P and Q are non-missing and P u Q shows two bases at most: use_PQ += count, and count
//   goes to one class at most: polymorphic in P only, in Q only, in both, or monomorphic in each with different bases
//   u32 per (selected locus, slot or group), and `sites`; the host refuses a locus whose sites reach 2^32.
// Kept: per (selected locus, slot) one double, E = E + e: one plain add a sample by the lane that owns the slot -- rebuilt bit
// for bit.  Per sample one row of 1 + NS doubles: the iteration, then per slot sum_loci (double)use_group(slot) e, the expected
// number of SITES of the class among the usable ones: the loci of a workgroup added in selection order from 0.0 into the
// workgroup's partial row, the partial rows in workgroup order by k_rows_fold (gph_sampler.h).  No fp atomics.  The observed
// totals over the selected loci once, as uint64 (integer atomics: order-free).
//
// k_sfs_tree.  Workgroup w takes the G consecutive selected loci w G ...; the stage and the climbs are k_triplets' (gph_triplets.h:
// GphTrLds, gph_tr_carve, gph_tr_climb and gph_tr_count as they stand, through the GphTrShape this shape carries).
//   stage    the N node records of each locus with 128-bit loads: the father into a 16-bit LDS word (the only relation the
//            climbs and the walk need: the relation stride is 2 N, not 6 N), the age of EVERY node into a double; the locus
//            rate and the locus's NG `use` words; the counter words zeroed; once a workgroup: the leaf -> population bytes, n_p
//   phase 1  task (g, i): the climb from leaf i, one 32-bit LDS add of 1 << 8 (index % 4) a step (byte counts, n <= 255)
//   phase 2  task (g, slot), strided over the flattened index: the non-root nodes in index order, one byte read (a bin) or two
//            (a class) a node, x in a register; e = rate x; E[locus][slot] += e (slot fastest: neighbouring lanes write
//            neighbouring doubles); (double)use e into the LDS cell [g][slot]
//   phase 3  lane `slot`, strided: the cells g = 0 .. live - 1 in order from 0.0 into the workgroup's partial row in HBM
// The slot table (one packed word a slot: P | Q << 8 | k << 16 | kind << 24, kind 0 a bin, 1 .. 4 the classes) and the slot ->
// group table are kernel arguments in HBM, read once per task.
// LDS a locus: 8 N (ages) + 8 (rate) + 8 NS (cells) + 4 NG rounded to 8 (use) + N Kc rounded to 4 (counters) + 2 N rounded to 8
// (fathers); once: n + Kc bytes rounded to 16.  16 leaves, Kc = 5, n_p = 4, 4, 4, 2, 2 (8 bins, 10 pairs: NS = 48, NG = 15): 248 +
// 8 + 384 + 64 + 156 + 64 = 924 bytes a locus.  G = the loci that give both phases 256 tasks, ceil(256 / min(n, NS)), at most
// GPH_TR_MAXG = 32 and at most what GPH_TR_LDS_BUDGET = 40 KB holds, at least 1: 16 there (14.8 KB).
//
// k_sfs_data.  One workgroup a selected locus, the lanes stride over the locus's rows; a lane reads the nibbles of its column
// where they lie, keeps the base counts of population p as four byte counts of a lane-owned LDS word (gph_pd_bytesum's form; a
// population with a missing leaf is the one whose byte sum falls short of n_p), classifies every group and adds `count` into the
// locus's u32 sums in LDS (integer LDS adds); after a barrier lane c stores sum c -- one store per (locus, slot or group) -- and
// adds it into the observed totals (64-bit integer atomic).  256 lanes up to 8 current populations, 128 up to 16, 64 beyond
// (k_predictive's rule): 4 (NS + NG + 1) + 4 Kc lanes + n + Kc bytes of LDS.
// Both kernels have one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane.  They write
// no page, draw no random number and touch no chain state.
#pragma once
#include "gph_triplets.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 18

enum { SFS_BIN = 0, SFS_PRIVP, SFS_PRIVQ, SFS_SHARED, SFS_FIXED };

struct GphSfShape {
  GphTrShape tr;                // G, bd, cstride, rstride (2 N: fathers alone), o_age (ALL N nodes a locus), o_cnt, o_rel, o_pop, lds_bytes (T, slots: 0; o_row: -1)
  int32_t NS, NG;               // slots, groups
  int32_t ustride;              // `use` words a locus in LDS (NG rounded to 2)
  int32_t o_rate, o_cell, o_use;        // byte offsets in the dynamic LDS of k_sfs_tree: rate [G], cell [G][NS] doubles; use [G][ustride] u32
  int32_t dbd, d_lds;           // k_sfs_data: lanes, dynamic LDS
  int32_t o_dsum, o_dcnt, o_dpop;       // ... sums [NS + NG + 1] u32, cnt [Kc][dbd] u32, pop [n + Kc] bytes
};

// the word of a slot in the table (each of P, Q, k below 256)
GPH_SM_HD int32_t gph_sf_pack(int kind, int P, int Q, int k) { return (int32_t)((uint32_t)P | ((uint32_t)Q << 8) | ((uint32_t)k << 16) | ((uint32_t)kind << 24)); }

GPH_SM_HD void gph_sf_shape(const GphLayout &y, int NS, int NG, GphSfShape &s)
{
  GphTrShape &h = s.tr;
  const int n = y.n > 1 ? y.n : 2, N = y.N > 0 ? y.N : 1, Kc = y.Kc > 0 ? y.Kc : 1;
  s.NS = NS; s.NG = NG; s.ustride = (NG + 1) & ~1;
  h.T = 0; h.slots = 0;
  h.cstride = (N * Kc + 3) & ~3;
  h.rstride = (2 * N + 7) & ~7;
  const int popb = (n + Kc + 15) & ~15;
  const int per = 8 * N + 8 + 8 * NS + 4 * s.ustride + h.cstride + h.rstride, once = popb;
  const int least = NS > 0 && NS < n ? NS : n;
  int G = (GPH_TR_MAXTHREADS + least - 1) / least;
  if (G > GPH_TR_MAXG) G = GPH_TR_MAXG;
  if (G > (GPH_TR_LDS_BUDGET - once) / per) G = (GPH_TR_LDS_BUDGET - once) / per;
  if (G < 1) G = 1;
  h.G = G;
  int most = G * (NS > n ? NS : n);
  if (most > GPH_TR_MAXTHREADS) most = GPH_TR_MAXTHREADS;
  h.bd = (most + 63) / 64 * 64;
  int at = 0;
  h.o_age = at; at += G * 8 * N;
  s.o_rate = at; at += G * 8;
  s.o_cell = at; at += G * 8 * NS;
  s.o_use = at; at += G * 4 * s.ustride;
  h.o_cnt = at; at += G * h.cstride;
  h.o_rel = at; at += G * h.rstride;
  h.o_pop = at; at += popb;
  h.o_row = -1;
  h.lds_bytes = at;
  s.dbd = Kc <= 8 ? 256 : Kc <= 16 ? 128 : 64;
  at = 0;
  s.o_dsum = at; at += 4 * (NS + NG + 1);
  s.o_dcnt = at; at += 4 * Kc * s.dbd;
  s.o_dpop = at; at += popb;
  s.d_lds = at;
}

struct GphSfLds {
  GphTrLds t;         // age [G][N] (every node), counters, fathers, pop
  double *rate;       // [G]
  double *cell;       // [G][NS]
  uint32_t *use;      // [G][ustride]
};
GPH_SM_FN void gph_sf_carve(char *base, const GphSfShape &h, GphSfLds &s)
{
  gph_tr_carve(base, h.tr, s.t);
  s.rate = (double *)(base + h.o_rate); s.cell = (double *)(base + h.o_cell); s.use = (uint32_t *)(base + h.o_use);
}

// does a node with a leaves of P (of nP) and b leaves of Q (of nQ) below it belong to the slot?
GPH_SM_FN bool gph_sf_member(int kind, int k, uint32_t a, uint32_t nP, uint32_t b, uint32_t nQ)
{
  const bool ain = a > 0u && a < nP;
  if (kind == SFS_BIN) return ain && (a < nP - a ? a : nP - a) == (uint32_t)k;
  const bool bin = b > 0u && b < nQ;
  if (kind == SFS_PRIVP) return ain && !bin;
  if (kind == SFS_PRIVQ) return bin && !ain;
  if (kind == SFS_SHARED) return ain && bin;
  return (a == nP && b == 0u) || (a == 0u && b == nQ);
}

// workgroup w = block bx.  slot [NS] packed slots; sgrp [NS] slot -> group; pop [n + Kc] leaf -> population, then n_p; use
// [nsel][NG] of k_sfs_data; acc [nsel][NS]; part [workgroups][1 + NS] (column 0 is the fold's iteration column)
GPH_FLAT(k_sfs_tree, GPH_TR_MAXTHREADS, GphLayout y, GphSfShape hs, const char *pages, const int32_t *sel_slot, const int32_t *slot, const int32_t *sgrp,
         const uint8_t *pop, const uint32_t *use, int nsel, int L, double *acc, double *part)
{
  GPH_FLAT_BODY(GphNoLane);
  const GphTrShape &h = hs.tr;
  const int n = y.n, N = y.N, Kc = y.Kc, cw = h.cstride / 4, rw = h.rstride / 2, NS = hs.NS, NG = hs.NG, us = hs.ustride;
  const int q0 = bx * h.G, live = nsel - q0 < h.G ? nsel - q0 : h.G;      /* loci of this workgroup */
  if (live <= 0) return;
  GphSfLds sp;
  gph_sf_carve(lds, hs, sp);
  const GphTrLds &s = sp.t;
  GPH_PHASE {
    for (int u = tid; u < live * N; u += bd) {
      const int g = u / N, v = u - g * N;
      const int j = GPH_IX(sel_slot[GPH_IX(q0 + g, nsel)], L);
      const char *pg = pages + (size_t)j * y.page_bytes;
      GphNode rec;
      gph_copy16(&rec, pg + y.o_nd + (size_t)v * 16);
      s.rel[GPH_IX(g * rw + v, h.G * rw)] = rec.father;
      s.age[GPH_IX(g * N + v, h.G * N)] = rec.age;
      if (v == 0) sp.rate[GPH_IX(g, h.G)] = ((const double *)(pg + y.o_fscal))[FS_MUTRATE];
    }
    for (int u = tid; u < live * cw; u += bd) s.cnt[GPH_IX(u, h.G * cw)] = 0u;
    for (int u = tid; u < n + Kc; u += bd) s.pop[GPH_IX(u, n + Kc)] = pop[GPH_IX(u, n + Kc)];
    for (int u = tid; u < live * NG; u += bd) {
      const int g = u / NG, k = u - g * NG;
      sp.use[GPH_IX(g * us + k, h.G * us)] = use[(size_t)(q0 + g) * NG + GPH_IX(k, NG)];
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < live * n; u += bd) {
      const int g = u / n;
      gph_tr_climb(s, y, h, g, u - g * n);
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < live * NS; u += bd) {
      const int g = u / NS, sl = u - g * NS;
      const uint32_t word = (uint32_t)slot[GPH_IX(sl, NS)];
      const int P = (int)(word & 255u), Q = (int)((word >> 8) & 255u), k = (int)((word >> 16) & 255u), kind = (int)(word >> 24);
      const int grp = sgrp[GPH_IX(sl, NS)];
      double x = 0.0;
      if (P < Kc && Q < Kc) {
        const uint32_t nP = s.pop[GPH_IX(n + P, n + Kc)], nQ = s.pop[GPH_IX(n + Q, n + Kc)];
        for (int v = 0; v < N; v++) {
          const int f = s.rel[GPH_IX(g * rw + v, h.G * rw)];
          if ((unsigned)f >= (unsigned)N || f == v) continue;                 /* the root (or a damaged record): no branch */
          const uint32_t a = gph_tr_count(s, h, cw, g, v * Kc + P), b = kind == SFS_BIN ? 0u : gph_tr_count(s, h, cw, g, v * Kc + Q);
          if (!gph_sf_member(kind, k, a, nP, b, nQ)) continue;
          const double len = s.age[GPH_IX(g * N + f, h.G * N)] - s.age[GPH_IX(g * N + v, h.G * N)];
          x = x + len;
        }
      }
      const double e = sp.rate[GPH_IX(g, h.G)] * x;
      double *c = acc + (size_t)(q0 + g) * NS;
      c[GPH_IX(sl, NS)] = c[GPH_IX(sl, NS)] + e;
      const double used = (unsigned)grp < (unsigned)NG ? (double)sp.use[GPH_IX(g * us + grp, h.G * us)] : 0.0;
      sp.cell[GPH_IX(g * NS + sl, h.G * NS)] = used * e;
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    double *out = part + (size_t)bx * (1 + NS);
    if (tid == 0) out[0] = 0.0;
    for (int sl = tid; sl < NS; sl += bd) {
      double sum = 0.0;
      for (int g = 0; g < live; g++) sum = sum + sp.cell[GPH_IX(g * NS + sl, h.G * NS)];
      out[1 + GPH_IX(sl, NS)] = sum;
    }
  }
}

// the distinct bases of a word of four byte counts
GPH_SM_FN int gph_sf_shown(uint32_t w) { return ((w & 255u) != 0u) + (((w >> 8) & 255u) != 0u) + (((w >> 16) & 255u) != 0u) + ((w >> 24) != 0u); }
// the smallest non-zero byte of a word (0: none)
GPH_SM_FN uint32_t gph_sf_rarer(uint32_t w)
{
  uint32_t least = 0u;
  for (int b = 0; b < 4; b++) {
    const uint32_t c = (w >> (8 * b)) & 255u;
    if (c != 0u && (least == 0u || c < least)) least = c;
  }
  return least;
}

// workgroup bx = selected locus bx.  gdef [NG] packed groups (P | Q << 8 | pair << 24), gbase [NG] the first slot of each; pop
// [n + Kc]; obs [nsel][NS], use [nsel][NG], sites [nsel]; tot [NS + NG + 1]: the totals over the selection
GPH_FLAT(k_sfs_data, GPH_PD_MAXTHREADS, GphLayout y, GphSfShape hs, const char *seq, const uint64_t *seq_off, const int32_t *P2, const int32_t *sel_slot,
         const int32_t *gdef, const int32_t *gbase, const uint8_t *pop, int nsel, int L, uint32_t *obs, uint32_t *use, uint32_t *sites, uint64_t *tot)
{
  GPH_FLAT_BODY(GphNoLane);
  const int n = y.n, Kc = y.Kc, NH = GPH_Q_NH(n), NS = hs.NS, NG = hs.NG, W = NS + NG + 1, q = bx;
  if (q >= nsel) return;
  const int j = GPH_IX(sel_slot[GPH_IX(q, nsel)], L);
  const int P = P2[GPH_IX(2 * j, 2 * L)];
  const char *blk = seq + seq_off[GPH_IX(j, L + 1)];
  const int q_phases = GPH_Q_PHASES(P, n), q_count = GPH_Q_COUNT(P, n);
  uint32_t *sums = (uint32_t *)(lds + hs.o_dsum), *cnt = (uint32_t *)(lds + hs.o_dcnt);
  uint8_t *lpop = (uint8_t *)(lds + hs.o_dpop);
  GPH_PHASE {
    for (int c = tid; c < W; c += bd) sums[GPH_IX(c, W)] = 0u;
    for (int u = tid; u < n + Kc; u += bd) lpop[GPH_IX(u, n + Kc)] = pop[GPH_IX(u, n + Kc)];
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int r = tid; r < P; r += bd) {
      const uint32_t count = gph_pd_row_sites(blk, q_phases, q_count, y.cnt16, r, P);
      if (count == 0u) continue;                        /* a later row of a group of phases, or a column without a site */
      const uint8_t *row = (const uint8_t *)blk + GPH_Q_LEAF + (size_t)r * NH;
      for (int p = 0; p < Kc; p++) cnt[GPH_IX(p * bd + tid, Kc * bd)] = 0u;
      for (int i = 0; i < n; i++) {
        const int code = (row[GPH_IX(i >> 1, NH)] >> ((i & 1) << 2)) & 15, p = lpop[GPH_IX(i, n + Kc)];
        if (code >= 4 || p >= Kc) continue;
        cnt[GPH_IX(p * bd + tid, Kc * bd)] += 1u << (8 * code);
      }
      gph_lanes_add(sums + GPH_IX(NS + NG, W), count);
      for (int g = 0; g < NG; g++) {
        const uint32_t word = (uint32_t)gdef[GPH_IX(g, NG)];
        const int A = (int)(word & 255u), B = (int)((word >> 8) & 255u), base = gbase[GPH_IX(g, NG)];
        if (A >= Kc || B >= Kc) continue;
        const uint32_t wa = cnt[GPH_IX(A * bd + tid, Kc * bd)], nA = lpop[GPH_IX(n + A, n + Kc)];
        if (gph_pd_bytesum(wa) != nA) continue;         /* a leaf of A is missing */
        if ((word >> 24) == 0u) {
          const int shown = gph_sf_shown(wa);
          if (shown > 2) continue;
          gph_lanes_add(sums + GPH_IX(NS + g, W), count);
          if (shown == 2) {
            const int k = (int)gph_sf_rarer(wa);
            if (k >= 1 && 2 * k <= (int)nA) gph_lanes_add(sums + GPH_IX(base + k - 1, W), count);
          }
        } else {
          const uint32_t wb = cnt[GPH_IX(B * bd + tid, Kc * bd)], nB = lpop[GPH_IX(n + B, n + Kc)];
          if (gph_pd_bytesum(wb) != nB) continue;
          const int both = gph_sf_shown(wa + wb);       /* (a byte holds n_A + n_B <= n <= 255) */
          if (both > 2) continue;
          gph_lanes_add(sums + GPH_IX(NS + g, W), count);
          const bool pa = gph_sf_shown(wa) == 2, pb = gph_sf_shown(wb) == 2;
          const int cls = pa && pb ? SFS_SHARED : pa ? SFS_PRIVP : pb ? SFS_PRIVQ : both == 2 ? SFS_FIXED : 0;
          if (cls) gph_lanes_add(sums + GPH_IX(base + cls - 1, W), count);
        }
      }
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int c = tid; c < W; c += bd) {
      const uint32_t T = sums[GPH_IX(c, W)];
      if (c < NS) obs[(size_t)q * NS + GPH_IX(c, NS)] = T;
      else if (c < NS + NG) use[(size_t)q * NG + GPH_IX(c - NS, NG)] = T;
      else sites[GPH_IX(q, nsel)] = T;
      if (T) gph_lanes_add64(tot + GPH_IX(c, W), (uint64_t)T);
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
