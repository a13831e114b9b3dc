// gph_cladecmp.h -- k_clades_compare: how far apart are the clade frequencies of R replicate chains, per locus, computed where
// the chains' clade tables lie (include/gphocs_hip.h, gph_engine_clades_compare).
//
// What is computed.  R = 2 .. GPH_CC_MAXR chains hold one clade table a selected locus each (gph_clades.h: entries [nsel][P][W + 2],
// header words [nsel][2]; same selection, P and W in every chain), chain r over S_r samples.  For locus q let U be the distinct
// keys kept in at least one of the R tables, the trivial clade (all n leaves) left out.  For k in U: c_r = the entry's cnt in
// table r, 0 where the table does not hold k (a full table that dropped k says 0 too: `dropped` in the row is the warning),
//   f_r = (double)c_r / (double)S_r          m = (((f_0 + f_1) + ...) + f_R-1) / R
//   v = (sum_r (f_r - m) (f_r - m), chain order) / (R - 1)          sd = sqrt(v)
// and k is COMPARED iff max_r f_r >= min_freq.  Row q, six fp64 columns: asdsf (sum of sd over the compared clades / their
// number, 0 without one), maxSd (0 without one), compared, distinct (|U|), shared (keys all R tables hold), dropped (sum over
// the chains of the tables' `dropped` words).  Every term is IEEE arithmetic in a fixed order; only the order in which the sds
// of a locus are added is the kernel's (lane partials, then lanes in lane order) -- fixed as well, so a row does not depend on
// which other loci are compared with it.
//
// Shape.  One 64-lane wavefront a locus, GPH_CC_THREADS = 256: workgroup w takes records 4 w .. 4 w + 3 of the selection,
// wavefronts beyond nsel do nothing.  For r = 0 .. R - 1 the locus's lanes stride the P slots of table r, consecutive lanes on
// consecutive entries.  A non-empty, non-trivial entry is probed for in tables 0 .. r - 1 (gph_cl_key's hash, gph_cl_find's
// linear probe: the lane lays its key down in the form k_clades keeps its masks in, one "record" of one "node" a lane, and
// calls them as they are): found there, the clade was counted when that table was walked -- skipped.  Otherwise tables
// r + 1 .. R - 1 are probed for their counts.  So every clade of U is owned by exactly one lane: no atomics, no duplicates.
// The loops over the chains run over GPH_CC_MAXR with a predicate, as gph_cl_find's over GPH_CL_MAXW: the counts stay in
// registers (32-bit; f_r is formed where it is used).  A lane keeps five partials -- sum, max, three counts --, writes them to
// LDS, and behind the barrier one lane a locus adds the 64 in lane order and writes the row.
// LDS: 256 (28 + 8 W) bytes -- 9 KB at W = 1, 15 KB at W = 4.
//
// The kernel writes no table, no page and no chain state, and waits for nothing: that the tables are complete when it reads
// them, and are not written while it does, is the host's ordering of the chains' streams (gph_backend.h: compare_order_*).
#pragma once
#include "gph_clades.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 11

#define GPH_CC_THREADS 256
#define GPH_CC_WAVE 64
#define GPH_CC_MAXR 16
#define GPH_CC_COLS 6

// the R tables, by value in the kernel-argument segment
struct GphCcTables {
  const uint64_t *ent[GPH_CC_MAXR];
  const uint32_t *hdr[GPH_CC_MAXR];
  int64_t samples[GPH_CC_MAXR];
};

GPH_SM_HD int32_t gph_cc_lds_bytes(int W) { return GPH_CC_THREADS * (8 + 8 + 3 * 4 + 2 * W * 4); }

// the LDS of a workgroup: the lanes' partials and, in key.mask, the key each lane is looking at ([threads][1][2W] u32)
struct GphCcLds {
  double *sum, *mx;       // [threads]
  uint32_t *cnt;          // [3][threads]: compared, distinct, shared
  GphClLds key;
};
GPH_SM_FN void gph_cc_carve(char *base, int W, GphCcLds &s)
{
  char *p = base;
  s.sum = (double *)p; p += (size_t)GPH_CC_THREADS * 8;
  s.mx = (double *)p; p += (size_t)GPH_CC_THREADS * 8;
  s.cnt = (uint32_t *)p; p += (size_t)GPH_CC_THREADS * 3 * 4;
  s.key.age = nullptr; s.key.up = nullptr; s.key.miss = nullptr;
  s.key.mask = (uint32_t *)p;
  (void)W;
}

// is this key the clade of all n leaves?
GPH_SM_FN bool gph_cc_trivial(const uint64_t *en, int W, int n)
{
  bool all = true;
  for (int w = 0; w < GPH_CL_MAXW; w++)
    if (w < W) {
      const int left = n - 64 * w;
      const uint64_t full = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1 : 0ull;
      all = all && en[w] == full;
    }
  return all;
}

// the five partials of a lane
struct GphCcPart {
  double sum = 0.0, mx = 0.0;
  uint32_t compared = 0, distinct = 0, shared = 0;
};

// lane `t` of its workgroup looks at entry `slot` of table r of locus q: counted into a iff this lane owns the clade
GPH_SM_FN void gph_cc_entry(const GphCcLds &s, const GphLayout &ky, const GphClShape &kh, const GphClShape &h, const GphCcTables &T, int R, int r,
                            size_t tab_off, int slot, int n, int t, double min_freq, GphCcPart &a)
{
  const uint64_t *en = T.ent[GPH_IX(r, GPH_CC_MAXR)] + tab_off + (size_t)GPH_IX(slot, h.P) * h.ew;
  const uint64_t own = en[h.W];
  if (own == 0 || gph_cc_trivial(en, h.W, n)) return;
  /* the key as k_clades holds a node's mask: "record" t, "node" 0 */
  const int mw = 2 * h.W;
  for (int w = 0; w < GPH_CL_MAXW; w++)
    if (w < h.W) {
      s.key.mask[GPH_IX(t * mw + 2 * w, GPH_CC_THREADS * mw)] = (uint32_t)en[w];
      s.key.mask[GPH_IX(t * mw + 2 * w + 1, GPH_CC_THREADS * mw)] = (uint32_t)(en[w] >> 32);
    }
  uint64_t key[GPH_CL_MAXW];
  const uint64_t hash = gph_cl_key(s.key, ky, kh, t, 0, key);
  uint32_t c[GPH_CC_MAXR];
  bool mine = true;
#pragma unroll
  for (int j = 0; j < GPH_CC_MAXR; j++) {
    c[j] = 0;
    if (j < R && j != r && mine) {
      const uint64_t *tab = T.ent[j] + tab_off;
      const int at = gph_cl_find(tab, h, key, hash);
      if (at >= 0) {
        if (j < r) mine = false;      /* counted when table j was walked */
        else c[j] = (uint32_t)tab[(size_t)GPH_IX(at, h.P) * h.ew + h.W];
      }
    }
    if (j == r) c[j] = (uint32_t)own;
  }
  if (!mine) return;
  double fsum = 0.0, fmax = 0.0;
  bool everywhere = true;
#pragma unroll
  for (int j = 0; j < GPH_CC_MAXR; j++)
    if (j < R) {
      const double f = (double)c[j] / (double)T.samples[j];
      fsum = fsum + f;
      fmax = f > fmax ? f : fmax;
      everywhere = everywhere && c[j] != 0;
    }
  const double m = fsum / (double)R;
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < GPH_CC_MAXR; j++)
    if (j < R) {
      const double d = (double)c[j] / (double)T.samples[j] - m;
      ss = ss + d * d;
    }
  const double sd = sqrt(ss / (double)(R - 1));
  a.distinct++;
  if (everywhere) a.shared++;
  if (fmax >= min_freq) {
    a.compared++;
    a.sum = a.sum + sd;
    a.mx = sd > a.mx ? sd : a.mx;
  }
}

// one lane a locus: the 64 partials in lane order -> the row
GPH_SM_FN void gph_cc_row(const GphCcLds &s, const GphCcTables &T, int R, int q, int t0, double *row)
{
  double sum = 0.0, mx = 0.0, compared = 0.0, distinct = 0.0, shared = 0.0, dropped = 0.0;
  for (int l = 0; l < GPH_CC_WAVE; l++) {
    const int t = GPH_IX(t0 + l, GPH_CC_THREADS);
    sum = sum + s.sum[t];
    mx = s.mx[t] > mx ? s.mx[t] : mx;
    compared += (double)s.cnt[t];
    distinct += (double)s.cnt[GPH_CC_THREADS + t];
    shared += (double)s.cnt[2 * GPH_CC_THREADS + t];
  }
  for (int j = 0; j < GPH_CC_MAXR; j++)
    if (j < R) dropped += (double)T.hdr[j][(size_t)q * 2 + 1];
  row[0] = compared > 0.0 ? sum / compared : 0.0;
  row[1] = mx;
  row[2] = compared; row[3] = distinct; row[4] = shared; row[5] = dropped;
}

// workgroup w = block bx; h: the shape the chains' tables share; n: leaves
GPH_FLAT(k_clades_compare, GPH_CC_THREADS, GphClShape h, GphCcTables T, int R, int n, int nsel, double min_freq, double *rows)
{
  GPH_FLAT_BODY(GphNoLane);
  GphCcLds s;
  gph_cc_carve(lds, h.W, s);
  /* gph_cl_key reads node k of record g at mask[(g (y.n - 1) + k) 2W ...]: one node a record, one record a lane */
  GphLayout ky = {};
  ky.n = 2;
  GphClShape kh = h;
  kh.G = GPH_CC_THREADS;
  GPH_PHASE {
    const int g = tid / GPH_CC_WAVE, l = tid - g * GPH_CC_WAVE, q = bx * (GPH_CC_THREADS / GPH_CC_WAVE) + g;
    GphCcPart a;
    if (q < nsel) {
      const size_t tab_off = (size_t)q * h.P * h.ew;
      for (int r = 0; r < R; r++)
        for (int slot = l; slot < h.P; slot += GPH_CC_WAVE) gph_cc_entry(s, ky, kh, h, T, R, r, tab_off, slot, n, tid, min_freq, a);
    }
    const int t = GPH_IX(tid, GPH_CC_THREADS);
    s.sum[t] = a.sum; s.mx[t] = a.mx;
    s.cnt[t] = a.compared; s.cnt[GPH_CC_THREADS + t] = a.distinct; s.cnt[2 * GPH_CC_THREADS + t] = a.shared;
  }
  GPH_BARRIER;
  GPH_PHASE {
    const int g = tid / GPH_CC_WAVE, q = bx * (GPH_CC_THREADS / GPH_CC_WAVE) + g;
    if (tid - g * GPH_CC_WAVE == 0 && q < nsel) gph_cc_row(s, T, R, q, g * GPH_CC_WAVE, rows + (size_t)q * GPH_CC_COLS);
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
