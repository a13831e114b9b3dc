// gph_pairtimes.h -- k_pair_times: the distribution of the coalescence time of a lineage from population P and a lineage from
// population Q on an absolute time axis, per selected locus and genome-wide per sample, accumulated on the device
// (include/gphocs_hip.h, gph_engine_pair_times_*).
//
// Definitions.  Populations: the Kc CURRENT populations in model order; leaf i belongs to pop[i], n_p = the leaves of p.  A PAIR
// is (P, Q), P <= Q, with m_PQ >= 1 leaf pairs: m_PQ = n_P n_Q for P < Q, m_PP = n_P (n_P - 1) / 2 (default: all such pairs in
// lexicographic order); pair number k is SLOT k, NP their number.  The GRID is E = B - 1 edges e_0 < ... < e_{E-1}, finite
// positive doubles in the genealogy's own units, 1 <= E <= 127; bin(a) = the number of edges e <= a (an age equal to an edge lies
// in the upper bin), bin 0 = [0, e_0), bin B - 1 = [e_{E-1}, inf).
// One locus at one sample, v an internal node (n <= v < N) with children l, r, c_x[p] = the leaves of p under x:
//   w_v(P, Q) = c_l[P] c_r[Q] + c_r[P] c_l[Q]  (P < Q),    w_v(P, P) = c_l[P] c_r[P]
// = the leaf pairs of the slot whose lca is v: an integer <= 200^2, never enumerated.  split(P, Q), from popAge / popFather of the
// chain state at the sample: P < Q the age of the youngest population that is an ancestor of both, P = Q the age of P's father
// population, +inf when P has none.  Per sample and slot, all sums over the internal nodes in NODE-INDEX order, terms with
// w_v = 0 skipped, plain uncontracted fp64 (a multiply, then an add):
//   hist[k] = sum_{bin(age[v]) = k} w_v;  a = sum age[v] (double)w_v;  y = sum_{age[v] < split} w_v;  x = [y > 0];
//   tmin = the smallest age[v] with w_v > 0.            Invariants: sum_k hist[k] = m_PQ, y <= m_PQ.
// Per selected locus four doubles a slot, A += a, Y += y, X += x, M += tmin: one plain fp64 add a sample each, by the one lane
// that owns the slot -- rebuilt bit for bit; layout [locus][A | Y | X | M][slot].  Per sample one row of NP (B + 2) uint64 over
// the selected loci of the rank: per slot the B hist totals, then per slot the y total, then per slot the loci with x = 1 --
// integer atomics, order-free; the rows of different ranks add.
//
// Shape.  Workgroup w takes the G consecutive selected loci w G ...; stage and phase 1 are k_triplets' (gph_triplets.h: its
// GphTrLds, gph_tr_climb and gph_tr_count are used as they stand, through the GphTrShape this shape carries).
//   stage    the N node records of each locus with 128-bit loads; father / left / right into 16-bit LDS words, the ages of the
//            internal nodes into doubles; the counter words zeroed; once a workgroup: the leaf -> population bytes and n_p, the
//            E edges, popAge and popFather of the chain state, the row zeroed.
//   phase 1  task (g, i): the climb from leaf i, one 32-bit LDS add of 1 << 8 (index % 4) a step (byte counts, n <= 255).
//            Behind the climbs, lane `slot`, strided: split(slot) by a climb of popFather from P, and for every ancestor a climb
//            from Q, each guarded by K steps.
//   phase 2  task (g, slot), strided over the flattened index: the internal nodes in index order, w_v from four byte reads (two
//            for P = Q), the bin by a binary search over the edges in LDS (7 steps at most), w_v into hist by ONE 32-bit integer
//            LDS add into the workgroup's row (a sum is at most G n^2 < 2^32); a, y, tmin in registers; then the slot's own four
//            doubles (slot fastest: neighbouring lanes write neighbouring doubles), y and x into the LDS row.
//   phase 3  the workgroup's non-zero sums into the sample's row, one 64-bit integer atomic each.
// The LDS row is kept while it is at most GPH_TR_ROW_LDS = 8 KB (NP (B + 2) <= 2 048); beyond that phase 2 adds to the sample's
// row directly and there is no phase 3 (k_triplets' rule).  The pair table (one packed word a pair, P | Q << 8, a kernel
// argument in HBM) is read once per task into a register.
// LDS a locus: 8 (n - 1) (ages) + N Kc rounded to 4 (counters) + 6 N rounded to 8 (relations); once: 8 (E + K + NP) (edges,
// popAge, split), n + Kc bytes and 2 K bytes (popFather) rounded to 16, and the row, 4 NP (B + 2) bytes rounded to 16.
// 16 leaves, Kc = 5, B = 34: 468 bytes a locus, once 8 (33 + 9 + 15) + 32 + 32 + 2 160 = 2 680; the caps (N = 399, Kc = 39,
// K = 77, NP = 780, E = 127): 19.6 KB a locus, once 8 272 bytes, no row.
// G = the loci that give both phases 256 tasks, ceil(256 / min(n, NP)), at most GPH_TR_MAXG = 32 and at most what
// GPH_TR_LDS_BUDGET = 40 KB holds, at least 1: 18 at 16 leaves, Kc = 5 (15 slots; 11 KB), 1 at the caps.
// No fp atomics.  One text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane.  It writes no
// page, draws no random number and touches no chain state.
#pragma once
#include "gph_triplets.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 17

#define GPH_PT_MAXEDGES 127

struct GphPtShape {
  GphTrShape tr;                // G, bd, cstride, rstride, o_age, o_cnt, o_rel, o_pop, o_row, lds_bytes as k_triplets reads them (T, slots: 0)
  int32_t NP, B, E;             // slots, bins, edges
  int32_t W;                    // the numbers of a row: NP (B + 2)
  int32_t o_edge, o_page, o_split, o_pf;    // byte offsets in the dynamic LDS: edges [E], popAge [K], split [NP] doubles; popFather [K] 16-bit words
};

// the word of a pair in the table (P <= Q, each below 256)
GPH_SM_HD int32_t gph_pt_pack(int P, int Q) { return (int32_t)((uint32_t)P | ((uint32_t)Q << 8)); }

GPH_SM_HD void gph_pt_shape(const GphLayout &y, int NP, int E, GphPtShape &s)
{
  GphTrShape &h = s.tr;
  const int n = y.n > 1 ? y.n : 2, N = y.N > 0 ? y.N : 1, Kc = y.Kc > 0 ? y.Kc : 1, K = y.K > 0 ? y.K : 1;
  s.NP = NP; s.E = E; s.B = E + 1; s.W = NP * (E + 3);
  h.T = 0; h.slots = 0;
  h.cstride = (N * Kc + 3) & ~3;
  h.rstride = (6 * N + 7) & ~7;
  const int rowb = 4 * s.W <= GPH_TR_ROW_LDS ? (4 * s.W + 15) & ~15 : 0;
  const int dbl = 8 * (E + K + NP), popb = (n + Kc + 15) & ~15, pfb = (2 * K + 15) & ~15;
  const int per = 8 * (n - 1) + h.cstride + h.rstride, once = dbl + popb + pfb + rowb;
  const int least = NP > 0 && NP < n ? NP : n;
  int G = (GPH_TR_MAXTHREADS + least - 1) / least;
  if (G > GPH_TR_MAXG) G = GPH_TR_MAXG;
  if (G > (GPH_TR_LDS_BUDGET - once) / per) G = (GPH_TR_LDS_BUDGET - once) / per;
  if (G < 1) G = 1;
  h.G = G;
  int most = G * (NP > n ? NP : n);
  if (most > GPH_TR_MAXTHREADS) most = GPH_TR_MAXTHREADS;
  h.bd = (most + 63) / 64 * 64;
  int at = 0;
  h.o_age = at; at += G * 8 * (n - 1);
  s.o_edge = at; at += 8 * E;
  s.o_page = at; at += 8 * K;
  s.o_split = at; at += 8 * NP;
  h.o_cnt = at; at += G * h.cstride;
  h.o_rel = at; at += G * h.rstride;
  h.o_pop = at; at += popb;
  s.o_pf = at; at += pfb;
  h.o_row = rowb ? at : -1; at += rowb;
  h.lds_bytes = at;
}

struct GphPtLds {
  GphTrLds t;         // ages, counters, relations, pop, the workgroup's row [W] (null: none)
  double *edge;       // [E]
  double *page;       // [K] popAge of the chain state
  double *split;      // [NP]
  int16_t *pf;        // [K] popFather of the chain state
};
GPH_SM_FN void gph_pt_carve(char *base, const GphPtShape &h, GphPtLds &s)
{
  gph_tr_carve(base, h.tr, s.t);
  s.edge = (double *)(base + h.o_edge); s.page = (double *)(base + h.o_page); s.split = (double *)(base + h.o_split);
  s.pf = (int16_t *)(base + h.o_pf);
}

// split(P, Q) from the staged popAge / popFather; every climb guarded by K steps
GPH_SM_FN double gph_pt_split(const GphPtLds &s, int K, int P, int Q)
{
  int a = s.pf[GPH_IX(P, K)];
  if (P == Q) return (unsigned)a < (unsigned)K ? s.page[GPH_IX(a, K)] : __builtin_huge_val();
  for (int ga = 0; ga < K && (unsigned)a < (unsigned)K; ga++) {
    int b = s.pf[GPH_IX(Q, K)];
    for (int gb = 0; gb < K && (unsigned)b < (unsigned)K; gb++) {
      if (b == a) return s.page[GPH_IX(a, K)];
      b = s.pf[GPH_IX(b, K)];
    }
    a = s.pf[GPH_IX(a, K)];
  }
  return __builtin_huge_val();                /* (no common ancestor: a damaged population tree bounds nothing) */
}

// bin(a): the number of edges e <= a
GPH_SM_FN int gph_pt_bin(const GphPtLds &s, int E, double a)
{
  int lo = 0, hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s.edge[GPH_IX(mid, E)] <= a) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// workgroup w = block bx.  pair [NP] packed pairs; pop [n + Kc] leaf -> population, then n_p; edges [E]; acc [nsel][4][NP] (A, Y,
// X, M); row [NP (B + 2)]
GPH_FLAT(k_pair_times, GPH_TR_MAXTHREADS, GphKargs KA, GphPtShape hp, const char *pages, const int32_t *sel_slot, const int32_t *pair, const uint8_t *pop,
         const double *edges, int nsel, int L, double *acc, uint64_t *row)
{
  GPH_FLAT_BODY(GphNoLane);
  const GphLayout &y = KA.lay;
  const GphModel &model = KA.G->model;
  const GphTrShape &h = hp.tr;
  const int n = y.n, N = y.N, Kc = y.Kc, K = y.K, cw = h.cstride / 4, rw = h.rstride / 2, NP = hp.NP, B = hp.B, E = hp.E, W = hp.W;
  const int q0 = bx * h.G, live = nsel - q0 < h.G ? nsel - q0 : h.G;      /* loci of this workgroup */
  if (live <= 0) return;
  GphPtLds sp;
  gph_pt_carve(lds, hp, sp);
  const GphTrLds &s = sp.t;
  GPH_PHASE {
    for (int u = tid; u < live * N; u += bd) {
      const int g = u / N, v = u - g * N;
      const int j = GPH_IX(sel_slot[GPH_IX(q0 + g, nsel)], L);
      GphNode rec;
      gph_copy16(&rec, pages + (size_t)j * y.page_bytes + y.o_nd + (size_t)v * 16);
      s.rel[GPH_IX(g * rw + v, h.G * rw)] = rec.father;
      s.rel[GPH_IX(g * rw + N + v, h.G * rw)] = rec.left;
      s.rel[GPH_IX(g * rw + 2 * N + v, h.G * rw)] = rec.right;
      if (v >= n) s.age[GPH_IX(g * (n - 1) + (v - n), h.G * (n - 1))] = rec.age;
    }
    for (int u = tid; u < live * cw; u += bd) s.cnt[GPH_IX(u, h.G * cw)] = 0u;
    for (int u = tid; u < n + Kc; u += bd) s.pop[GPH_IX(u, n + Kc)] = pop[GPH_IX(u, n + Kc)];
    for (int u = tid; u < E; u += bd) sp.edge[GPH_IX(u, E)] = edges[GPH_IX(u, E)];
    for (int p = tid; p < K; p += bd) { sp.page[GPH_IX(p, K)] = model.popAge[GPH_IX(p, GPH_MAXK)]; sp.pf[GPH_IX(p, K)] = (int16_t)model.popFather[GPH_IX(p, GPH_MAXK)]; }
    if (s.row)
      for (int u = tid; u < W; u += bd) s.row[GPH_IX(u, W)] = 0u;
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < live * n; u += bd) {
      const int g = u / n;
      gph_tr_climb(s, y, h, g, u - g * n);
    }
    for (int sl = tid; sl < NP; sl += bd) {
      const uint32_t word = (uint32_t)pair[GPH_IX(sl, NP)];
      const int P = (int)(word & 255u), Q = (int)((word >> 8) & 255u);
      sp.split[GPH_IX(sl, NP)] = P < Kc && Q < Kc ? gph_pt_split(sp, K, P, Q) : __builtin_huge_val();
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < live * NP; u += bd) {
      const int g = u / NP, sl = u - g * NP;
      const uint32_t word = (uint32_t)pair[GPH_IX(sl, NP)];
      const int P = (int)(word & 255u), Q = (int)((word >> 8) & 255u);
      if (P >= Kc || Q >= Kc) continue;
      const double split = sp.split[GPH_IX(sl, NP)];
      double a = 0.0, tmin = __builtin_huge_val();
      uint32_t yy = 0u;
      for (int v = n; v < N; v++) {
        const int l = s.rel[GPH_IX(g * rw + N + v, h.G * rw)], r = s.rel[GPH_IX(g * rw + 2 * N + v, h.G * rw)];
        if ((unsigned)l >= (unsigned)N || (unsigned)r >= (unsigned)N) continue;     /* (a damaged record must not reach past the counters) */
        uint32_t w = gph_tr_count(s, h, cw, g, l * Kc + P) * gph_tr_count(s, h, cw, g, r * Kc + Q);
        if (P != Q) w += gph_tr_count(s, h, cw, g, r * Kc + P) * gph_tr_count(s, h, cw, g, l * Kc + Q);
        if (w == 0u) continue;
        const double t = s.age[GPH_IX(g * (n - 1) + (v - n), h.G * (n - 1))];
        const int k = gph_pt_bin(sp, E, t);
        if (s.row) gph_lanes_add(s.row + GPH_IX(sl * B + k, W), w);
        else gph_lanes_add64(row + GPH_IX(sl * B + k, W), (uint64_t)w);
        const double term = t * (double)w;
        a = a + term;
        if (t < split) yy += w;
        if (t < tmin) tmin = t;
      }
      double *c = acc + (size_t)(q0 + g) * 4 * NP;
      c[GPH_IX(sl, 4 * NP)] = c[GPH_IX(sl, 4 * NP)] + a;
      c[GPH_IX(NP + sl, 4 * NP)] = c[GPH_IX(NP + sl, 4 * NP)] + (double)yy;
      c[GPH_IX(2 * NP + sl, 4 * NP)] = c[GPH_IX(2 * NP + sl, 4 * NP)] + (yy ? 1.0 : 0.0);
      c[GPH_IX(3 * NP + sl, 4 * NP)] = c[GPH_IX(3 * NP + sl, 4 * NP)] + tmin;
      if (yy) {
        if (s.row) { gph_lanes_add(s.row + GPH_IX(NP * B + sl, W), yy); gph_lanes_add(s.row + GPH_IX(NP * B + NP + sl, W), 1u); }
        else { gph_lanes_add64(row + GPH_IX(NP * B + sl, W), (uint64_t)yy); gph_lanes_add64(row + GPH_IX(NP * B + NP + sl, W), (uint64_t)1); }
      }
    }
  }
  if (!s.row) return;                     /* (uniform over the workgroup) */
  GPH_BARRIER;
  GPH_PHASE {
    for (int u = tid; u < W; u += bd) {
      const uint32_t sum = s.row[GPH_IX(u, W)];
      if (sum) gph_lanes_add64(row + GPH_IX(u, W), (uint64_t)sum);
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
