// gph_triplets.h -- k_triplets: triplet topology weights (Martin & Van Belleghem 2017, "Twisst") per selected locus and
// genome-wide per sample, accumulated on the device (include/gphocs_hip.h, gph_engine_triplets_*).
//
// Definitions.  Populations: the Kc CURRENT populations in model order; leaf i belongs to pop[i] (the leaf -> current-population
// byte table k_predictive is handed), n_p = the leaves of p.  A TRIPLE is P < Q < R with n_P, n_Q, n_R >= 1 (default: all, in
// lexicographic order).  Its TOPOLOGIES are t = 0: PQ|R, 1: PR|Q, 2: QR|P; SLOT (triple, t) has number 3 triple + t.
// One locus at one sample, v an internal node (n <= v < N) with children l = left[v], r = right[v], c_x[p] = the leaves of p
// in the subtree of x (a leaf's own row: 1 at its population), tot[p] = n_p.  For slot XY|Z
//   w_v(XY|Z) = (c_l[X] c_r[Y] + c_r[X] c_l[Y]) (tot[Z] - c_l[Z] - c_r[Z])
// = the leaf triples (a in X, b in Y, c in Z) with lca(a, b) = v and c outside v's subtree: a and b sisters relative to c.
// An integer <= n_X n_Y n_Z (< 2^32 up to the caps of 200 leaves).  Per sample and slot:
//   cnt = sum_v w_v (integer);  age = sum_v age[v] (double)w_v over the internal nodes in NODE-INDEX order, terms with w_v = 0
//   skipped, plain uncontracted fp64: a multiply, then an add, no fma.
// Invariant: per triple sum_t cnt = n_P n_Q n_R at every sample (a binary tree gives each leaf triple exactly one topology).
// Per selected locus, two doubles a slot: W = W + cnt (exact while S n_P n_Q n_R < 2^53), A = A + age -- one plain fp64 add a
// sample, by the one lane that owns the slot: rebuilt bit for bit.  Per sample, one row of 3 T uint64 totals of cnt over the
// selected loci of the rank: integer atomics, order-free; the rows of different ranks add.
//
// Shape.  Workgroup w takes the G consecutive selected loci w G ...
//   stage    the N node records of each locus are read with 128-bit loads, consecutive lanes on consecutive records; father /
//            left / right go into 16-bit LDS words, the ages of the internal nodes into doubles; the counter words are zeroed;
//            the leaf -> population bytes and the n_p bytes are copied once per workgroup.
//   phase 1  task (g, i), strided over the lanes: climb from leaf i to the root (guarded by N steps, as gph_an_leaf is); on
//            every node of the path, the leaf's own row included, add 1 to the BYTE count c[g][v][pop(i)].  A count is at most
//            n_p <= n <= 200 < 256 (the host refuses more than 255 leaves): a byte cannot overflow, so four counts share a
//            32-bit LDS word and the add is ONE 32-bit integer LDS add of 1 << 8 (index % 4) that never carries into its
//            neighbour -- order-free.
//   phase 2  task (g, slot), strided over the lanes when G 3T exceeds them: walk the internal nodes in index order, form w_v from
//            six byte reads of the counters, sum cnt and age; then update its own W, A (layout [locus][W | A][slot]: slot
//            fastest, neighbouring lanes write neighbouring doubles) and add cnt into the WORKGROUP's row of 32-bit sums in LDS
//            (integer LDS add; a sum is at most G (n / 3)^3 < 2^32).
//   phase 3  lane `slot`, strided: the workgroup's non-zero sums into the sample's row, one 64-bit integer atomic each.  Every
//            locus adding its 3 T counts to the sample's row directly was measured first: 3 10^6 atomics a launch on 240 bytes
//            (two cache lines) took 3 ms at 100 000 loci, 16 leaves, T = 10 -- the atomics, not the tree walks.  Through LDS the
//            row sees G times fewer.  The LDS row is kept while it is at most GPH_TR_ROW_LDS = 8 KB (3 T <= 2 048); beyond that
//            (27 current populations and more, all triples) phase 2 adds to the sample's row directly and there is no phase 3.
//            The triple table (one packed word a triple, P | Q << 8 | R << 16, a kernel argument in HBM) is read once per task
//            into a register: at the caps it has 9 139 entries, which LDS has no room for next to the counters.
// Both task loops run over the flattened (g, task) index, so neither phase needs n or 3T to divide the lanes of a locus.
// LDS a locus: 8 (n - 1) (ages) + N Kc rounded to 4 (counters) + 6 N rounded to 8 (relations); once: n + Kc bytes rounded to 16
// and the row, 12 T bytes rounded to 16.
// 16 leaves, Kc = 5: 120 + 156 + 192 = 468 bytes a locus; the caps (N = 399, Kc = 39): 1 592 + 15 564 + 2 400 = 19.6 KB.
// G = the loci that give both phases 256 tasks, ceil(256 / min(n, 3T)), at most GPH_TR_MAXG = 32 (T = 1 would otherwise ask for
// 86 loci, whose climbs are 4 lanes' worth each) and at most what GPH_TR_LDS_BUDGET = 40 KB holds (4 workgroups a CU), at
// least 1: 16 at 16 leaves and Kc = 5 (7.5 KB: phase 1 has 256 tasks, phase 2 480), 1 at the caps.
// No fp atomics.  The kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane.
// It writes no page, draws no random number and touches no chain state.
#pragma once
#include "gph_sampler.h"
#include "gph_predictive.h"     /* gph_lanes_add64 */

#undef GPH_FILE_ID
#define GPH_FILE_ID 14

#define GPH_TR_MAXTHREADS 256
#define GPH_TR_MAXG 32
#define GPH_TR_LDS_BUDGET 40960
#define GPH_TR_ROW_LDS 8192

struct GphTrShape {
  int32_t G, bd;                // loci a workgroup, lanes
  int32_t T, slots;             // triples, 3 T
  int32_t cstride;              // counter bytes a locus (N Kc rounded to 4)
  int32_t rstride;              // relation bytes a locus (6 N rounded to 8)
  int32_t o_age, o_cnt, o_rel, o_pop;     // byte offsets in the dynamic LDS
  int32_t o_row;                // ... of the workgroup's row; -1: none, the counts go to the sample's row directly
  int32_t lds_bytes;
};

// the word of a triple in the table (P < Q < R, each below 256)
GPH_SM_HD int32_t gph_tr_pack(int P, int Q, int R) { return (int32_t)((uint32_t)P | ((uint32_t)Q << 8) | ((uint32_t)R << 16)); }

GPH_SM_HD void gph_tr_shape(const GphLayout &y, int T, GphTrShape &h)
{
  const int n = y.n > 1 ? y.n : 2, N = y.N > 0 ? y.N : 1, Kc = y.Kc > 0 ? y.Kc : 1;
  h.T = T; h.slots = 3 * T;
  h.cstride = (N * Kc + 3) & ~3;
  h.rstride = (6 * N + 7) & ~7;
  const int rowb = 4 * h.slots <= GPH_TR_ROW_LDS ? (4 * h.slots + 15) & ~15 : 0;
  const int per = 8 * (n - 1) + h.cstride + h.rstride, once = ((n + Kc + 15) & ~15) + rowb;
  const int least = h.slots > 0 && h.slots < n ? h.slots : n;
  int G = (GPH_TR_MAXTHREADS + least - 1) / least;
  if (G > GPH_TR_MAXG) G = GPH_TR_MAXG;
  if (G > (GPH_TR_LDS_BUDGET - once) / per) G = (GPH_TR_LDS_BUDGET - once) / per;
  if (G < 1) G = 1;
  h.G = G;
  int most = G * (h.slots > n ? h.slots : n);
  if (most > GPH_TR_MAXTHREADS) most = GPH_TR_MAXTHREADS;
  h.bd = (most + 63) / 64 * 64;
  int at = 0;
  h.o_age = at; at += G * 8 * (n - 1);
  h.o_cnt = at; at += G * h.cstride;
  h.o_rel = at; at += G * h.rstride;
  h.o_pop = at; at += once - rowb;
  h.o_row = rowb ? at : -1; at += rowb;
  h.lds_bytes = at;
}

struct GphTrLds {
  double *age;        // [G][n - 1] ages of the internal nodes n + k
  uint32_t *cnt;      // [G][cstride / 4] four byte counts a word: byte v Kc + p of a locus = c_v[p]
  int16_t *rel;       // [G][rstride / 2]: father [N], left [N], right [N]
  uint8_t *pop;       // [n] leaf -> current population, then [Kc] n_p
  uint32_t *row;      // [slots] the workgroup's sums of cnt (null: none)
};
GPH_SM_FN void gph_tr_carve(char *base, const GphTrShape &h, GphTrLds &s)
{
  s.age = (double *)(base + h.o_age); s.cnt = (uint32_t *)(base + h.o_cnt); s.rel = (int16_t *)(base + h.o_rel); s.pop = (uint8_t *)(base + h.o_pop);
  s.row = h.o_row >= 0 ? (uint32_t *)(base + h.o_row) : nullptr;
}

// task (g, i) of phase 1: 1 into c[g][v][pop(i)] for every node v on the path from leaf i to the root
GPH_SM_FN void gph_tr_climb(const GphTrLds &s, const GphLayout &y, const GphTrShape &h, int g, int i)
{
  const int n = y.n, N = y.N, Kc = y.Kc, cw = h.cstride / 4, rw = h.rstride / 2;
  const int p = s.pop[GPH_IX(i, n + Kc)];
  if (p >= Kc) return;                                /* (a damaged table must not reach past a node's row) */
  int v = i;
  for (int guard = 0; guard < N; guard++) {
    const int b = v * Kc + p;
    gph_lanes_add(s.cnt + GPH_IX(g * cw + (b >> 2), h.G * cw), 1u << (8 * (b & 3)));
    const int f = s.rel[GPH_IX(g * rw + v, h.G * rw)];
    if ((unsigned)f >= (unsigned)N) break;
    v = f;
  }
}

GPH_SM_FN uint32_t gph_tr_count(const GphTrLds &s, const GphTrShape &h, int cw, int g, int b)
{
  return (s.cnt[GPH_IX(g * cw + (b >> 2), h.G * cw)] >> (8 * (b & 3))) & 255u;
}

// task (g, slot) of phase 2: cnt and age of slot XY|Z over the internal nodes in index order
GPH_SM_FN void gph_tr_slot(const GphTrLds &s, const GphLayout &y, const GphTrShape &h, int g, int X, int Y, int Z, uint32_t &cnt, double &age)
{
  const int n = y.n, N = y.N, Kc = y.Kc, cw = h.cstride / 4, rw = h.rstride / 2;
  const uint32_t tot = s.pop[GPH_IX(n + Z, n + Kc)];
  cnt = 0u;
  age = 0.0;
  for (int v = n; v < N; v++) {
    const int l = s.rel[GPH_IX(g * rw + N + v, h.G * rw)], r = s.rel[GPH_IX(g * rw + 2 * N + v, h.G * rw)];
    if ((unsigned)l >= (unsigned)N || (unsigned)r >= (unsigned)N) continue;     /* (a damaged record must not reach past the counters) */
    const uint32_t lx = gph_tr_count(s, h, cw, g, l * Kc + X), ry = gph_tr_count(s, h, cw, g, r * Kc + Y);
    const uint32_t rx = gph_tr_count(s, h, cw, g, r * Kc + X), ly = gph_tr_count(s, h, cw, g, l * Kc + Y);
    const uint32_t pairs = lx * ry + rx * ly;
    if (pairs == 0u) continue;
    const uint32_t in = gph_tr_count(s, h, cw, g, l * Kc + Z) + gph_tr_count(s, h, cw, g, r * Kc + Z);
    if (in >= tot) continue;
    const uint32_t w = pairs * (tot - in);
    cnt += w;
    const double term = s.age[GPH_IX(g * (n - 1) + (v - n), h.G * (n - 1))] * (double)w;
    age = age + term;
  }
}

// workgroup w = block bx.  tri [T] packed triples; pop [n + Kc] leaf -> population, then n_p; acc [nsel][2][slots] (W, then A);
// row [slots]
GPH_FLAT(k_triplets, GPH_TR_MAXTHREADS, GphLayout y, GphTrShape h, const char *pages, const int32_t *sel_slot, const int32_t *tri, const uint8_t *pop,
         int nsel, int L, double *acc, uint64_t *row)
{
  GPH_FLAT_BODY(GphNoLane);
  const int n = y.n, N = y.N, Kc = y.Kc, cw = h.cstride / 4, rw = h.rstride / 2, slots = h.slots;
  const int q0 = bx * h.G, live = nsel - q0 < h.G ? nsel - q0 : h.G;      /* loci of this workgroup */
  if (live <= 0) return;
  GphTrLds s;
  gph_tr_carve(lds, h, s);
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
    if (s.row)
      for (int u = tid; u < slots; u += bd) s.row[GPH_IX(u, slots)] = 0u;
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
    for (int u = tid; u < live * slots; u += bd) {
      const int g = u / slots, sl = u - g * slots, k = sl / 3, t = sl - 3 * k;
      const uint32_t word = (uint32_t)tri[GPH_IX(k, h.T)];
      const int P = (int)(word & 255u), Q = (int)((word >> 8) & 255u), R = (int)((word >> 16) & 255u);
      if (P >= Kc || Q >= Kc || R >= Kc) continue;
      uint32_t cnt;
      double age;
      gph_tr_slot(s, y, h, g, t == 2 ? Q : P, t == 0 ? Q : R, t == 0 ? R : t == 1 ? Q : P, cnt, age);
      double *a = acc + (size_t)(q0 + g) * 2 * slots;
      a[GPH_IX(sl, 2 * slots)] = a[GPH_IX(sl, 2 * slots)] + (double)cnt;
      a[GPH_IX(slots + sl, 2 * slots)] = a[GPH_IX(slots + sl, 2 * slots)] + age;
      if (cnt) {
        if (s.row) gph_lanes_add(s.row + GPH_IX(sl, slots), cnt);
        else gph_lanes_add64(row + GPH_IX(sl, slots), (uint64_t)cnt);
      }
    }
  }
  if (!s.row) return;                     /* (uniform over the workgroup) */
  GPH_BARRIER;
  GPH_PHASE {
    for (int sl = tid; sl < slots; sl += bd) {
      const uint32_t sum = s.row[GPH_IX(sl, slots)];
      if (sum) gph_lanes_add64(row + GPH_IX(sl, slots), (uint64_t)sum);
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
