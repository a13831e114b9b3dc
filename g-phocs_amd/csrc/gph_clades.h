// gph_clades.h -- k_clades: per-locus clade tables over the samples taken, accumulated on the device (include/gphocs_hip.h,
// gph_engine_clades_*).
//
// What is computed.  For one locus at one sample let n be the leaves, N = 2n - 1 the nodes, W = ceil(n / 64).  The CLADE of
// internal node v is the set of leaves i whose path i, father(i), ..., root contains v, held as W 64-bit words (bit i % 64 of
// word i / 64); the root's clade is included, so a sample brings n - 1 pairwise distinct clades a locus.  Per selected locus
// a TABLE of P slots (a power of two) holds at most limit = 3P/4 distinct clades: an entry is key[W], cnt, age (the age's bit
// pattern), cnt = 0 marks an empty slot; two header words a locus, nkeys and dropped.  A sample takes the internal nodes
// v = n .. N - 1 in node-index order: key in the table -> cnt += 1, age = age + age[v] (one plain fp64 addition by the one lane
// that owns the cell: rebuilt bit for bit in sample order); else nkeys < limit -> insert with cnt = 1, age = age[v]; else
// dropped += 1.  That rule fixes the table's content whatever the hash function and the probe order; where an entry lies
// inside its table is no part of the contract.
//
// Layout.  Entries [q][slot][W + 2] u64, header [q][2] u32, q = 0 .. nsel - 1 over the selected loci of the rank in increasing
// locus index (what gph_engine_clades_fetch hands out, unchanged); record q comes from slot sel_slot[q] as in k_gene_trees.
//
// Shape.  Workgroup w takes the G = max(1, 256 / n) consecutive records w G ... of the selection.  The node records are read
// with 128-bit loads, consecutive lanes on consecutive records: the father goes into one 32-bit LDS word a node, the age of an
// internal node into one LDS double (ages are STAGED with the records, not read again at update time: the lane that loads
// record v is not the lane that later owns node v, and 8 (n - 1) bytes a locus are cheaper than a second trip to the page).
// Lane (g, i) then climbs from leaf i and ORs its bit into the mask of every ancestor ([G][n - 1][2W] u32, zeroed; a 32-bit LDS
// integer atomic -- order-free: gph_lanes_bits, gph_sampler.h), at most N steps, a father outside n .. N - 1 ends the climb.  After
// a barrier lane (g, v - n) hashes its key (a splitmix64 finaliser folded over the words: plain integer
// arithmetic) and probes the locus's table in HBM linearly: a hit updates the lane's own cell -- distinct nodes
// of a tree have distinct keys, no two lanes share a cell, and this phase writes no key -- a miss sets a flag in LDS.  After a
// second barrier one lane a locus takes the flagged nodes in node-index order and inserts or drops them by the rule (it
// probes again, for the key as well: a damaged record with two equal clades still follows the rule).  Misses are rare once a
// table has warmed up; a full table skips the probe.  Linear probing ends: at least P - limit >= 1 slots stay empty.
// No fp atomics, no global atomics: a locus has one owner workgroup.
// LDS: G (4 N + (n - 1) (8 + 8 W + 4)) bytes -- 6.6 KB at 16 leaves (G = 16), 10.1 KB at 200 (G = 1, W = 4).
//
// The kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane, phase by phase.
// It writes no page, draws no random number and touches no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 10      /* (9000xx is taken by the typed accessors of the dynamic LDS) */

#define GPH_CL_THREADS 256
#define GPH_CL_MAXW ((GPH_CAP_LEAVES + 63) / 64)

struct GphClShape {
  int32_t G;                  // records a workgroup
  int32_t W;                  // 64-bit words of a key
  int32_t P, limit;           // slots of a table, distinct clades it holds at most
  int32_t ew;                 // 64-bit words of an entry: W + 2
  int32_t lds_bytes;
};

// slots: a power of two >= 2 (the caller has checked)
GPH_SM_HD void gph_cl_shape(const GphLayout &y, int32_t slots, GphClShape &h)
{
  const int n = y.n > 0 ? y.n : 1;
  h.G = n < GPH_CL_THREADS ? GPH_CL_THREADS / n : 1;
  h.W = (n + 63) / 64;
  h.P = slots;
  h.limit = (int32_t)((int64_t)slots * 3 / 4);
  h.ew = h.W + 2;
  h.lds_bytes = h.G * (y.N * 4 + (n - 1) * (8 + 8 * h.W + 4));
}

// the smallest power of two >= 8 (n - 1), 2 at least
GPH_SM_HD int32_t gph_cl_default_slots(int n)
{
  int32_t p = 2;
  while (p < 8 * (n - 1)) p *= 2;
  return p;
}

// the LDS of a workgroup
struct GphClLds {
  double *age;      // [G][n - 1] ages of the internal nodes
  int32_t *up;      // [G][N] father
  uint32_t *mask;   // [G][n - 1][2W] clade of internal node n + k, 32 leaves a word
  uint32_t *miss;   // [G][n - 1] 1: the node's key was not in the table
};
GPH_SM_FN void gph_cl_carve(char *base, const GphLayout &y, const GphClShape &h, GphClLds &s)
{
  const int ni = y.n - 1;
  char *p = base;
  s.age = (double *)p; p += (size_t)h.G * ni * 8;
  s.mask = (uint32_t *)p; p += (size_t)h.G * ni * 2 * h.W * 4;
  s.up = (int32_t *)p; p += (size_t)h.G * y.N * 4;
  s.miss = (uint32_t *)p;
}

// record g of workgroup w -> its page slot; -1: beyond the last record
GPH_SM_FN int gph_cl_slot(const GphClShape &h, const int32_t *sel_slot, int nsel, int L, int w, int g)
{
  const int q = w * h.G + g;
  if (q >= nsel) return -1;
  return GPH_IX(sel_slot[GPH_IX(q, nsel)], L);
}

// the staged words of node record v (16 bytes, loaded as one unit)
GPH_SM_FN void gph_cl_stage(const GphClLds &s, const GphLayout &y, const GphClShape &h, int g, int v, const void *rec16)
{
  GphNode r;
  memcpy(&r, rec16, sizeof r);
  s.up[GPH_IX(g * y.N + v, h.G * y.N)] = (int32_t)r.father;
  if (v >= y.n) s.age[GPH_IX(g * (y.n - 1) + (v - y.n), h.G * (y.n - 1))] = r.age;
}

// lane (g, i): leaf i's bit into the mask of every ancestor
GPH_SM_FN void gph_cl_climb(const GphClLds &s, const GphLayout &y, const GphClShape &h, int g, int i)
{
  const int n = y.n, N = y.N, mw = 2 * h.W;
  int v = i;
  for (int guard = 0; guard < N; guard++) {
    const int f = s.up[GPH_IX(g * N + v, h.G * N)];
    if (f < n || f >= N) break;               /* the root's -1, or a damaged record: no ancestor's mask beyond the arrays */
    gph_lanes_bits(s.mask + GPH_IX((g * (n - 1) + (f - n)) * mw + (i >> 5), h.G * (n - 1) * mw), 1u << (i & 31));
    v = f;
  }
}

GPH_SM_FN uint64_t gph_cl_mix(uint64_t z)
{
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27; z *= 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the key of internal node n + k of record g, and its hash
GPH_SM_FN uint64_t gph_cl_key(const GphClLds &s, const GphLayout &y, const GphClShape &h, int g, int k, uint64_t *key)
{
  const int mw = 2 * h.W;
  uint64_t x = 0;
  for (int w = 0; w < GPH_CL_MAXW; w++) {
    if (w >= h.W) { key[w] = 0; continue; }
    const int at = (g * (y.n - 1) + k) * mw + 2 * w;
    key[w] = (uint64_t)s.mask[GPH_IX(at, h.G * (y.n - 1) * mw)] | (uint64_t)s.mask[GPH_IX(at + 1, h.G * (y.n - 1) * mw)] << 32;
    x = gph_cl_mix(x + 0x9e3779b97f4a7c15ull + key[w]);
  }
  return x;
}

// linear probe of one locus's table: the slot that holds `key`, or -1 - (the first empty slot met), or -1 - P (no empty slot:
// cannot happen below the limit)
GPH_SM_FN int gph_cl_find(const uint64_t *tab, const GphClShape &h, const uint64_t *key, uint64_t hash)
{
  const int P = h.P, ew = h.ew;
  int at = (int)(hash & (uint64_t)(P - 1));
  for (int probe = 0; probe < P; probe++) {
    const uint64_t *en = tab + (size_t)GPH_IX(at, P) * ew;
    if (en[h.W] == 0) return -1 - at;
    bool same = true;
    for (int w = 0; w < GPH_CL_MAXW; w++)
      if (w < h.W) same = same && en[w] == key[w];
    if (same) return at;
    at = (at + 1) & (P - 1);
  }
  return -1 - P;
}

// cnt += 1, age = age + a: one plain fp64 addition
GPH_SM_FN void gph_cl_hit(uint64_t *tab, const GphClShape &h, int at, double a)
{
  uint64_t *en = tab + (size_t)GPH_IX(at, h.P) * h.ew;
  double sum;
  memcpy(&sum, &en[h.W + 1], 8);
  sum = sum + a;
  en[h.W] = en[h.W] + 1;
  memcpy(&en[h.W + 1], &sum, 8);
}

// lane (g, k): look internal node n + k up in its locus's table; a miss is left to gph_cl_insert
GPH_SM_FN void gph_cl_lookup(const GphClLds &s, const GphLayout &y, const GphClShape &h, int g, int k, uint64_t *tab)
{
  uint64_t key[GPH_CL_MAXW];
  const uint64_t hash = gph_cl_key(s, y, h, g, k, key);
  const int at = gph_cl_find(tab, h, key, hash), c = GPH_IX(g * (y.n - 1) + k, h.G * (y.n - 1));
  if (at >= 0) gph_cl_hit(tab, h, at, s.age[c]);
  s.miss[c] = at >= 0 ? 0u : 1u;
}

// one lane a locus: the nodes that missed, in node-index order
GPH_SM_FN void gph_cl_insert(const GphClLds &s, const GphLayout &y, const GphClShape &h, int g, uint64_t *tab, uint32_t *hdr)
{
  uint32_t nkeys = hdr[0], dropped = hdr[1];
  bool any = false;
  for (int k = 0; k < y.n - 1; k++) {
    const int c = GPH_IX(g * (y.n - 1) + k, h.G * (y.n - 1));
    if (!s.miss[c]) continue;
    any = true;
    if (nkeys >= (uint32_t)h.limit) { dropped++; continue; }      /* a full table stays full: what missed it is not in it */
    uint64_t key[GPH_CL_MAXW];
    const uint64_t hash = gph_cl_key(s, y, h, g, k, key);
    const int at = gph_cl_find(tab, h, key, hash);
    if (at >= 0) { gph_cl_hit(tab, h, at, s.age[c]); continue; }  /* (inserted a moment ago: two equal clades in a damaged record) */
    if (at == -1 - h.P) { dropped++; continue; }
    uint64_t *en = tab + (size_t)GPH_IX(-1 - at, h.P) * h.ew;
    for (int w = 0; w < GPH_CL_MAXW; w++)
      if (w < h.W) en[w] = key[w];
    memcpy(&en[h.W + 1], &s.age[c], 8);
    en[h.W] = 1;
    nkeys++;
  }
  if (any) { hdr[0] = nkeys; hdr[1] = dropped; }
}

// workgroup w = block bx
GPH_FLAT(k_clades, GPH_CL_THREADS, GphLayout y, GphClShape h, const char *pages, const int32_t *sel_slot, int nsel, int L, uint64_t *ent,
         uint32_t *hdr)
{
  GPH_FLAT_BODY(GphNoLane);
  const int n = y.n, N = y.N, ni = n - 1, w = bx;
  if (ni < 1) return;
  GphClLds s;
  gph_cl_carve(lds, y, h, s);
  GPH_PHASE {
    for (int u = tid; u < h.G * ni * 2 * h.W; u += bd) s.mask[GPH_IX(u, h.G * ni * 2 * h.W)] = 0u;
    for (int u = tid; u < h.G * N; u += bd) {
      const int g = u / N, v = u - g * N, j = gph_cl_slot(h, sel_slot, nsel, L, w, g);
      if (j >= 0) {
        GphNode rec;
        gph_copy16(&rec, pages + (size_t)j * y.page_bytes + y.o_nd + (size_t)v * 16);
        gph_cl_stage(s, y, h, g, v, &rec);
      }
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int t = tid; t < h.G * n; t += bd) {
      const int g = t / n, i = t - g * n;
      if (w * h.G + g < nsel) gph_cl_climb(s, y, h, g, i);
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    for (int t = tid; t < h.G * ni; t += bd) {
      const int g = t / ni, k = t - g * ni, q = w * h.G + g;
      if (q < nsel) gph_cl_lookup(s, y, h, g, k, ent + (size_t)q * h.P * h.ew);
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    if (tid < h.G) {
      const int q = w * h.G + tid;
      if (q < nsel) gph_cl_insert(s, y, h, tid, ent + (size_t)q * h.P * h.ew, hdr + (size_t)q * 2);
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
