// gph_predictive.h -- posterior predictive checks: k_predictive simulates, per selected locus and per sample, one replicate
// alignment under the sampled genealogy and locus rate (JC69, the likelihood's own model) with the locus's own missing-data
// pattern, and sums integer discrepancy statistics over its sites; the same body in "observed" mode sums them over the data
// (include/gphocs_hip.h, gph_engine_predictive_*).
//
// Sites.  The rows of a locus's sequence block in order; a COLUMN is a row with a non-zero phase word (the first row of its
// group of phases; the other rows of the group carry phase word 0 and count 0 and own no site).  Column c owns count_c sites:
// site s belongs to c iff prefix_c <= s < prefix_c + count_c.  A leaf whose code in the column is 4 (N) is missing at the
// column's sites, in the data and in the replicate.
//
// Generator (64-bit unsigned, modulo 2^64): mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
// z ^= z >> 31.  Kl = mix(seed ^ mix(g + 0x9E3779B97F4A7C15)) for the GLOBAL locus index g (formed by the host at enable), K =
// mix(Kl + t) for sample t, h(s, v) = mix(K ^ ((s << 16) | v)) for site s and node v: a pure function of (seed, locus, sample,
// site, node) -- any assignment of sites to lanes gives the same replicate.
//
// Branches.  v != root: len = rate * (age[father v] - age[v]), q_v = len < 1e-100 ? 0 : 1 - exp(-4 len / 3.0) (4 x edge_prob,
// gph_locus.h), thr_v = (uint64)(q_v 2^53); v FIRES at s iff (h(s, v) >> 11) < thr_v; the root always fires.  The base of leaf i
// at s is h(s, a) & 3 for the first node a on the path i, father(i), ..., root that fires at s.
//
// Statistics, C = 1 + Kc (Kc + 1) / 2 integers per site with cnt[p][b] = the non-missing leaves of current population p that
// show base b, m_p = sum_b cnt[p][b]:  seg = 1 iff two bases or more are shown at all;  diff_p|p = (m_p^2 - sum_b cnt[p][b]^2) / 2;
// diff_p|q = m_p m_q - sum_b cnt[p][b] cnt[q][b] (p < q).  Order: seg, then (p, q), p <= q, p-major.  A locus's sums T fit 32 bits
// (the host refuses a locus whose sites x max n_p n_q reach 2^32).
//
// Accumulators per (selected locus, statistic): obs, gt, eq, s1, s2.  Observed mode: obs = T.  A sample: gt += (T > obs),
// eq += (T == obs), s1 = s1 + T, s2 = s2 + T * T -- plain fp64 in sample order, each word owned by one lane.  And the sample's
// row (the observed row): C u64 totals of T over the selected loci, integer atomics.
//
// k_predictive, one workgroup per selected locus:
//   the N node records are staged with 128-bit loads (age, father); lane v forms thr_v (one gph_exp) into LDS;
//   the rows of the locus are taken in TILES of h.TC rows: their code nibbles are copied into LDS with 128-bit loads, their
//   counts are turned into the prefix ends of the tile (a lane sums a chunk of rows, one lane scans the bd chunk sums, the lanes
//   add the chunk bases), then the lanes stride over the tile's sites: a lane keeps its row while the next site lies in it and
//   searches the prefix ends otherwise;
//   per site (replicate mode) a lane first hashes every node: where no branch fires every leaf shows the root's base and every
//   statistic is 0 -- most sites; otherwise it climbs from every leaf, keeps cnt[p] as four byte counts of a lane-owned LDS word,
//   and adds what is non-zero into the locus's u32 sums in LDS (integer LDS adds);
//   after a barrier lane c updates the five doubles of (locus, c) and adds T into the row.
// LDS: 18 N + n + 4 C + 8 bd + 16 (nodes, leaf -> population bytes, sums, chunk sums) + 4 Kc bd (cnt) + the tile, TC (4 + NH)
// bytes with NH = (n + 1) / 2: the tile gets what 40 KB leave, 16 rows at least.  bd = 256 lanes up to 8 current populations,
// 128 up to 16, 64 beyond.  The kernel writes no page, reads the sequence blocks read-only and touches no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 13

#define GPH_PD_MAXTHREADS 256
#define GPH_PD_WORDS 5
#define GPH_PD_LDS_BUDGET 40960
enum { PD_OBS = 0, PD_GT, PD_EQ, PD_S1, PD_S2 };

struct GphPdShape {
  int32_t bd;           // lanes of a workgroup
  int32_t C;            // statistics
  int32_t TC;           // rows of a tile (a multiple of 16)
  int32_t o_thr, o_age, o_up, o_pop, o_sums, o_chunk, o_meta, o_cnt, o_end, o_codes;   // byte offsets in the dynamic LDS
  int32_t lds_bytes;
};

GPH_SM_HD int32_t gph_pd_stats(int Kc) { return 1 + Kc * (Kc + 1) / 2; }
// statistic of the pair p <= q
GPH_SM_HD int32_t gph_pd_pair(int Kc, int p, int q) { return 1 + p * Kc - p * (p - 1) / 2 + (q - p); }

GPH_SM_HD void gph_pd_shape(const GphLayout &y, GphPdShape &h)
{
  const int n = y.n, N = y.N, Kc = y.Kc, NH = GPH_Q_NH(n);
  h.bd = Kc <= 8 ? 256 : Kc <= 16 ? 128 : 64;
  h.C = gph_pd_stats(Kc);
  int at = 0;
  h.o_thr = at; at += 8 * N;
  h.o_age = at; at += 8 * N;
  h.o_meta = at; at += 16;                          /* two u64: K, and the sites of the tile */
  h.o_sums = at; at += 4 * h.C;
  h.o_chunk = at; at += 2 * 4 * h.bd;               /* chunk sums and chunk bases */
  h.o_cnt = at; at += 4 * Kc * h.bd;
  h.o_up = at; at += (2 * N + 3) & ~3;
  h.o_pop = at; at += (n + 15) & ~15;
  at = (at + 15) & ~15;
  int tc = ((GPH_PD_LDS_BUDGET - at) / (4 + NH)) & ~15;
  if (tc > 4096) tc = 4096;
  if (tc < 16) tc = 16;
  h.TC = tc;
  h.o_codes = at; at += (tc * NH + 15) & ~15;
  h.o_end = at; at += 4 * tc;
  h.lds_bytes = at;
}

struct GphPdLds {
  uint64_t *thr;        // [N] a node fires where (h >> 11) < thr; the root: all ones
  double *age;          // [N]
  uint64_t *meta;       // [0] K of this locus and sample, [1] sites of the tile
  uint32_t *sums;       // [C]
  uint32_t *chunk;      // [2][bd] rows of a lane's chunk: their sites, and the sites in front of the chunk
  uint32_t *cnt;        // [Kc][bd] lane-owned: byte b of cnt[p][lane] = the leaves of p showing base b at the lane's site
  int16_t *up;          // [N] father (the root: -1)
  uint8_t *pop;         // [n] leaf -> current population
  uint8_t *codes;       // [TC][NH] the tile's code nibbles
  uint32_t *end;        // [TC] sites of the tile up to and including the row
};
GPH_SM_FN void gph_pd_carve(char *base, const GphPdShape &h, GphPdLds &s)
{
  s.thr = (uint64_t *)(base + h.o_thr); s.age = (double *)(base + h.o_age); s.meta = (uint64_t *)(base + h.o_meta);
  s.sums = (uint32_t *)(base + h.o_sums); s.chunk = (uint32_t *)(base + h.o_chunk); s.cnt = (uint32_t *)(base + h.o_cnt);
  s.up = (int16_t *)(base + h.o_up); s.pop = (uint8_t *)(base + h.o_pop); s.codes = (uint8_t *)(base + h.o_codes);
  s.end = (uint32_t *)(base + h.o_end);
}

GPH_SM_HD uint64_t gph_pd_mix(uint64_t z)
{
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27; z *= 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// Kl of global locus g (host, at enable)
GPH_SM_HD uint64_t gph_pd_locus_key(uint64_t seed, uint64_t g) { return gph_pd_mix(seed ^ gph_pd_mix(g + 0x9e3779b97f4a7c15ull)); }

// the 64-bit sibling of gph_lanes_add
GPH_SM_FN void gph_lanes_add64(uint64_t *p, uint64_t v)
{
#ifdef GPH_HOSTEMU
  *p += v;
#else
  (void)atomicAdd((unsigned long long *)p, (unsigned long long)v);
#endif
}

// thr of node v with father f (f outside 0 .. N - 1: the root)
GPH_SM_FN uint64_t gph_pd_threshold(const GphPdLds &s, int N, int v, int f, double rate)
{
  if (f < 0 || f >= N) return ~(uint64_t)0;
  const double len = rate * (s.age[GPH_IX(f, N)] - s.age[GPH_IX(v, N)]);
  if (len < 1e-100) return 0;
  const double q = 1 - gph_exp(gph_quot(-4 * len, 3.0, 1.0 / 3.0));      /* (the exact quotient, as edge_prob_v forms it) */
  if (!(q > 0.0)) return 0;                         /* (a NaN from a damaged record fires nowhere) */
  return (uint64_t)(q * 9007199254740992.0);
}

GPH_SM_FN uint32_t gph_pd_bytesum(uint32_t w) { return (w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24); }
GPH_SM_FN uint32_t gph_pd_dot(uint32_t a, uint32_t b)
{
  return (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
}

// one site of lane `tid`: global site index `site`, its column's nibbles `row` (LDS)
GPH_SM_FN void gph_pd_site(const GphPdLds &s, const GphLayout &y, const GphPdShape &h, int tid, uint64_t K, uint64_t site, const uint8_t *row, int NH,
                           bool observed)
{
  const int n = y.n, N = y.N, Kc = y.Kc, bd = h.bd;
  const uint64_t sv = site << 16;
  if (!observed) {
    uint32_t fired = 0;                             /* (counted, not short-circuited: a loop without a branch per node) */
    for (int v = 0; v < N; v++) fired += (uint32_t)((gph_pd_mix(K ^ (sv | (uint64_t)v)) >> 11) < s.thr[GPH_IX(v, N)]);
    if (fired < 2) return;                          /* the root alone: every leaf shows its base, every statistic is 0 */
  }
  for (int p = 0; p < Kc; p++) s.cnt[GPH_IX(p * bd + tid, Kc * bd)] = 0u;
  uint32_t tot = 0;
  for (int i = 0; i < n; i++) {
    const int code = (row[GPH_IX(i >> 1, NH)] >> ((i & 1) << 2)) & 15;
    if (code >= 4) continue;
    int b = code;
    if (!observed) {
      int v = i;
      uint64_t hv = 0;
      for (int guard = 0; guard < N; guard++) {
        hv = gph_pd_mix(K ^ (sv | (uint64_t)v));
        if ((hv >> 11) < s.thr[GPH_IX(v, N)]) break;
        const int f = s.up[GPH_IX(v, N)];
        if (f < 0 || f >= N) break;
        v = f;
      }
      b = (int)(hv & 3);
    }
    const uint32_t one = 1u << (8 * b);
    s.cnt[GPH_IX(s.pop[GPH_IX(i, n)] * bd + tid, Kc * bd)] += one;
    tot += one;
  }
  const int shown = ((tot & 255u) != 0) + (((tot >> 8) & 255u) != 0) + (((tot >> 16) & 255u) != 0) + ((tot >> 24) != 0);
  if (shown < 2) return;                            /* one base at most: no pair differs */
  gph_lanes_add(s.sums + 0, 1u);
  for (int p = 0; p < Kc; p++) {
    const uint32_t wp = s.cnt[GPH_IX(p * bd + tid, Kc * bd)], mp = gph_pd_bytesum(wp);
    if (mp == 0) continue;
    const uint32_t dpp = (mp * mp - gph_pd_dot(wp, wp)) / 2;
    if (dpp) gph_lanes_add(s.sums + GPH_IX(gph_pd_pair(Kc, p, p), h.C), dpp);
    for (int q = p + 1; q < Kc; q++) {
      const uint32_t wq = s.cnt[GPH_IX(q * bd + tid, Kc * bd)];
      const uint32_t dpq = mp * gph_pd_bytesum(wq) - gph_pd_dot(wp, wq);
      if (dpq) gph_lanes_add(s.sums + GPH_IX(gph_pd_pair(Kc, p, q), h.C), dpq);
    }
  }
}

// the sites a row owns: its count where its phase word is not 0
GPH_SM_FN uint32_t gph_pd_row_sites(const char *blk, int q_phases, int q_count, int cnt16, int r, int P)
{
  if (((const uint16_t *)(blk + q_phases))[GPH_IX(r, P)] == 0) return 0u;
  return cnt16 ? (uint32_t)((const uint16_t *)(blk + q_count))[GPH_IX(r, P)] : (uint32_t)((const int32_t *)(blk + q_count))[GPH_IX(r, P)];
}

// workgroup bx = selected locus bx.  observed != 0: the data's statistics into acc[.][.][PD_OBS] and the observed row (no page
// is read); else sample t.  P2: {phased, unphased} patterns per slot; key: Kl per selected locus; pop: leaf -> population;
// acc [nsel][C][5]; row [C].  The genealogy the sites are drawn on is handed over: recs == null, the sampled one (the node
// records of the page); else the replicate genealogies of k_simulate (gph_simulate.h), recs [nsel][rec_bytes] with the node
// records at rec_nodes and the root word at rec_root -- a replicate that failed (root < 0) is left out: no site, no word touched.
// The rate is the locus's own either way.  One site loop for both.
GPH_FLAT(k_predictive, GPH_PD_MAXTHREADS, GphKargs KA, GphPdShape h, const char *pages, const char *seq, const uint64_t *seq_off, const int32_t *P2,
         const int32_t *sel_slot, const uint64_t *key, const uint8_t *pop, int nsel, int L, long long t, int observed, double *acc, uint64_t *row,
         const char *recs, int rec_bytes, int rec_nodes, int rec_root)
{
  GPH_FLAT_BODY(GphNoLane);
  const GphLayout &y = KA.lay;
  const int n = y.n, N = y.N, NH = GPH_Q_NH(n), C = h.C, q = bx;
  if (q >= nsel) return;
  if (recs && !observed && *(const int32_t *)(recs + (size_t)q * rec_bytes + rec_root) < 0) return;
  const int j = GPH_IX(sel_slot[GPH_IX(q, nsel)], L);
  const int P = P2[GPH_IX(2 * j, 2 * L)];
  const char *blk = seq + seq_off[GPH_IX(j, L + 1)];
  const char *pg = pages + (size_t)j * y.page_bytes;
  const char *nodes = recs ? recs + (size_t)q * rec_bytes + rec_nodes : pg + y.o_nd;
  const int q_phases = GPH_Q_PHASES(P, n), q_count = GPH_Q_COUNT(P, n);
  GphPdLds s;
  gph_pd_carve(lds, h, s);
  GPH_PHASE {
    for (int c = tid; c < C; c += bd) s.sums[GPH_IX(c, C)] = 0u;
    for (int i = tid; i < n; i += bd) s.pop[GPH_IX(i, n)] = pop[GPH_IX(i, n)];
    if (tid == 0) s.meta[0] = gph_pd_mix(key[GPH_IX(q, nsel)] + (uint64_t)t);
    if (!observed)
      for (int v = tid; v < N; v += bd) {
        GphNode rec;
        gph_copy16(&rec, nodes + (size_t)v * 16);
        s.age[GPH_IX(v, N)] = rec.age;
        s.up[GPH_IX(v, N)] = rec.father;
      }
  }
  GPH_BARRIER;
  GPH_PHASE {
    if (!observed) {
      const double rate = ((const double *)(pg + y.o_fscal))[FS_MUTRATE];
      for (int v = tid; v < N; v += bd) s.thr[GPH_IX(v, N)] = gph_pd_threshold(s, N, v, s.up[GPH_IX(v, N)], rate);
    }
  }
  GPH_BARRIER;
  const uint64_t K = s.meta[0];
  uint64_t site0 = 0;                               /* the sites in front of the tile */
  for (int r0 = 0; r0 < P; r0 += h.TC) {
    const int rows = P - r0 < h.TC ? P - r0 : h.TC, per = (rows + bd - 1) / bd;
    GPH_PHASE {
      const int units = (rows * NH + 15) >> 4;      /* (r0 NH is a multiple of 16; the last unit ends inside the block) */
      for (int u = tid; u < units; u += bd) gph_copy16(s.codes + (size_t)GPH_IX(u, (h.TC * NH + 15) >> 4) * 16, blk + GPH_Q_LEAF + (size_t)r0 * NH + (size_t)u * 16);
      uint32_t sum = 0;
      for (int r = tid * per; r < rows && r < (tid + 1) * per; r++) {
        sum += gph_pd_row_sites(blk, q_phases, q_count, y.cnt16, r0 + r, P);
        s.end[GPH_IX(r, h.TC)] = sum;
      }
      s.chunk[GPH_IX(tid, 2 * bd)] = sum;
    }
    GPH_BARRIER;
    GPH_PHASE {
      if (tid == 0) {
        uint32_t run = 0;
        for (int l = 0; l < bd; l++) { s.chunk[GPH_IX(bd + l, 2 * bd)] = run; run += s.chunk[GPH_IX(l, 2 * bd)]; }
        s.meta[1] = run;
      }
    }
    GPH_BARRIER;
    GPH_PHASE {
      const uint32_t base = s.chunk[GPH_IX(bd + tid, 2 * bd)];
      for (int r = tid * per; r < rows && r < (tid + 1) * per; r++) s.end[GPH_IX(r, h.TC)] += base;
    }
    GPH_BARRIER;
    const uint32_t tile_sites = (uint32_t)s.meta[1];
    GPH_PHASE {
      int r = 0;
      for (uint32_t sl = (uint32_t)tid; sl < tile_sites; sl += (uint32_t)bd) {
        if (sl >= s.end[GPH_IX(r, h.TC)]) {         /* the first row behind r whose end lies beyond sl */
          int lo = r + 1, hi = rows - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sl >= s.end[GPH_IX(mid, h.TC)]) lo = mid + 1; else hi = mid;
          }
          r = lo;
        }
        gph_pd_site(s, y, h, tid, K, site0 + sl, s.codes + (size_t)GPH_IX(r, h.TC) * NH, NH, observed != 0);
      }
    }
    GPH_BARRIER;
    site0 += tile_sites;
  }
  GPH_PHASE {
    for (int c = tid; c < C; c += bd) {
      const uint32_t T = s.sums[GPH_IX(c, C)];
      double *a = acc + ((size_t)q * C + c) * GPH_PD_WORDS;
      const double x = (double)T;
      if (observed) a[PD_OBS] = x;
      else {
        if (x > a[PD_OBS]) a[PD_GT] = a[PD_GT] + 1.0;
        if (x == a[PD_OBS]) a[PD_EQ] = a[PD_EQ] + 1.0;
        a[PD_S1] = a[PD_S1] + x;
        a[PD_S2] = a[PD_S2] + x * x;
      }
      if (T) gph_lanes_add64(row + GPH_IX(c, C), (uint64_t)T);
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
