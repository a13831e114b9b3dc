// gph_ancestry.h -- k_ancestry: which sample's lineage went through which migration band, at which locus, accumulated on
// the device (include/gphocs_hip.h, gph_engine_ancestry_*).
//
// What is computed.  For one locus at one sample let n be the leaves, B the bands, and take the LIVE migration nodes: the
// IS_NUM_MIGS entries of `living` (the M line of a state dump).  The path of leaf i is i, father(i), ..., root; migration
// node m is on the path iff MG_BRANCH[m] is a node of the path.
//   hit[b][i]   = 1 iff some live m on the path of i has MG_BAND[m] == b
//   first[b][i] = the smallest mig_age[m] among those (the youngest such migration: the first one met going back in time)
//   any[i]      = 1 iff some hit[b][i] is 1
// Per locus, over the samples taken: one fp64 row of n (2B + 1) columns, cnt.<b>.<i> += hit, age.<b>.<i> = age.<b>.<i> +
// first where hit (one plain uncontracted fp64 addition a sample, by the one lane that owns the cell: rebuilt bit for bit
// from state dumps), any.<i> += any.  Counts are integers held as doubles.  Per sample, over the loci of the rank: one row
// of n (B + 1) 32-bit integers, any.<i> then hit.<b>.<i>: the number of loci with any[i] / hit[b][i] = 1.
//
// Layout.  Accumulators: [slot][column], column = b n + i (cnt), B n + b n + i (age), 2 B n + i (any): the leaf is the
// fastest index, and lane (g, i) of a workgroup owns leaf i of the g-th locus of its group, so the lanes of neighbouring
// leaves write neighbouring doubles (and neighbouring loci neighbouring rows).  A sample's row: [i] any, [(1 + b) n + i].
//
// Shape.  Workgroup w takes the G = max(1, 256 / n) consecutive slots w G ... of the rank.  Lane g < G reads the
// IS_NUM_MIGS word of its slot -- four bytes a locus, nothing else -- and the workgroup votes: with no live migration in
// the whole group it returns there, having staged nothing and touched no accumulator (most groups of most samples).
// Otherwise, for the loci of the group WITH migrations only: the node records are read with 128-bit loads, consecutive
// lanes on consecutive records, and the father of each goes into the low half of one 32-bit LDS word a node (`up`, high
// half 0); mig_age, the mig_i words and `living` are copied into LDS with 128-bit loads (GphAnImg: three 16-byte-aligned
// byte ranges of a page, packed).  One lane a locus then ORs bit 16 + k into up[MG_BRANCH[living[k]]] for its k-th live
// migration (at most GPH_MAX_MIGS = 10: the mask has room), and lane (g, i) climbs from leaf i to the root with ONE
// 32-bit LDS read a node (lanes on different nodes are on different banks), ORing the masks.  A lane whose mask is not
// empty updates its own columns of the accumulator row and adds 1 to the sample's row with 32-bit integer atomics
// (integer addition is order-free: the row does not depend on scheduling).  No fp atomics.
// LDS: G (4 N + about 260) bytes -- 2.5 KB at 16 leaves, 1.9 KB at 200 (G = 1): neither leaves nor bands need tiling in
// any capacity variant; a lane holds a 10-bit mask, not a set of B bands.
//
// The kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane, phase by phase.
// It writes no page, draws no random number and touches no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 6

#define GPH_AN_MAXTHREADS 256
#define GPH_AN_RANGES 3

static_assert(GPH_MAX_MIGS <= 16, "the path mask of k_ancestry is the high half of a 32-bit word");

// mig_age, mig_i and living of a page, packed (gph_sampler.h); a_*: image offsets of the arrays themselves
struct GphAnImg : GphPackedImg {
  int32_t a_mage, a_migi, a_living;
};
struct GphAnShape {
  int32_t G, bd, lds_bytes;
  GphAnImg img;
};

GPH_SM_HD int gph_an_locus_columns(int n, int B) { return n * (2 * B + 1); }
GPH_SM_HD int gph_an_row_ints(int n, int B) { return n * (B + 1); }

GPH_SM_HD void gph_an_shape(const GphLayout &y, GphAnShape &h)
{
  const int lo[GPH_AN_RANGES] = {y.o_mig_age, y.o_mig_i, y.o_living};
  const int sz[GPH_AN_RANGES] = {GPH_MAX_MIGS * 8, GPH_MAX_MIGS * MG_COUNT * 2, GPH_MAX_MIGS * 2};
  int a[GPH_AN_RANGES];
  gph_pack_ranges(y, lo, sz, GPH_AN_RANGES, h.img, a);
  h.img.a_mage = a[0]; h.img.a_migi = a[1]; h.img.a_living = a[2];
  const int n = y.n > 0 ? y.n : 1;
  h.G = n < GPH_AN_MAXTHREADS ? GPH_AN_MAXTHREADS / n : 1;
  h.bd = (h.G * n + 63) / 64 * 64;
  h.lds_bytes = h.G * h.img.bytes + h.G * y.N * 4 + h.G * 4;
}

// the LDS of a workgroup
struct GphAnLds {
  char *img;        // [G][img.bytes]
  uint32_t *up;     // [G][N]: father (low half, as int16) | mask of the live migrations on the node's branch << 16
  int32_t *nm;      // [G] live migrations of the locus (0: not staged)
};
GPH_SM_FN void gph_an_carve(char *base, int N, const GphAnShape &h, GphAnLds &s)
{
  char *p = base;
  s.img = p; p += (size_t)h.G * h.img.bytes;
  s.up = (uint32_t *)p; p += (size_t)h.G * N * 4;
  s.nm = (int32_t *)p;
}

// live migrations of the locus in page pg, from the IS_NUM_MIGS word alone
GPH_SM_FN int gph_an_num_migs(const char *pg, const GphLayout &y)
{
  const int nm = ((const int32_t *)(pg + y.o_iscal))[IS_NUM_MIGS];
  return nm < 0 ? 0 : nm > GPH_MAX_MIGS ? GPH_MAX_MIGS : nm;
}

// the staged word of a node record (16 bytes, loaded as one unit): its father, no migration yet
GPH_SM_FN uint32_t gph_an_up_word(const void *rec16)
{
  GphNode r;
  memcpy(&r, rec16, sizeof r);
  return (uint32_t)(uint16_t)r.father;
}

// one lane a locus: bit 16 + k on the branch of the k-th live migration
GPH_SM_FN void gph_an_mark(const GphAnLds &s, const GphLayout &y, const GphAnShape &h, int g)
{
  const char *im = s.img + (size_t)GPH_IX(g, h.G) * h.img.bytes;
  const int16_t *migi = (const int16_t *)(im + h.img.a_migi), *living = (const int16_t *)(im + h.img.a_living);
  const int nm = s.nm[GPH_IX(g, h.G)];
  for (int k = 0; k < nm; k++) {
    const int m = living[GPH_IX(k, GPH_MAX_MIGS)];
    if ((unsigned)m >= (unsigned)GPH_MAX_MIGS) continue;      /* (a damaged record must not reach past the arrays) */
    const int br = migi[GPH_IX(m * MG_COUNT + MG_BRANCH, GPH_MAX_MIGS * MG_COUNT)];
    if ((unsigned)br >= (unsigned)y.N) continue;
    const int at = GPH_IX(g * y.N + br, h.G * y.N);
    s.up[at] = s.up[at] | (1u << (16 + k));
  }
}

// lane (g, i): climb from leaf i to the root of the staged locus g (slot j), then the lane's own columns of the locus's
// accumulator row `a` and of the sample's row
GPH_SM_FN void gph_an_leaf(const GphAnLds &s, const GphLayout &y, const GphAnShape &h, int g, int i, double *a, uint32_t *row)
{
  const int n = y.n, N = y.N, B = y.B, ncol = gph_an_locus_columns(n, B), nrow = gph_an_row_ints(n, B);
  uint32_t mask = 0;
  int v = i;
  for (int guard = 0; guard < N; guard++) {
    const uint32_t w = s.up[GPH_IX(g * N + v, h.G * N)];
    mask |= w >> 16;
    const int f = (int16_t)(w & 0xffffu);
    if ((unsigned)f >= (unsigned)N) break;
    v = f;
  }
  if (!mask) return;
  const char *im = s.img + (size_t)GPH_IX(g, h.G) * h.img.bytes;
  const double *mage = (const double *)(im + h.img.a_mage);
  const int16_t *migi = (const int16_t *)(im + h.img.a_migi), *living = (const int16_t *)(im + h.img.a_living);
  int band[GPH_MAX_MIGS];
  double age[GPH_MAX_MIGS];
  for (int k = 0; k < GPH_MAX_MIGS; k++) {
    band[k] = -1;
    age[k] = 0.0;
    if (!((mask >> k) & 1u)) continue;
    const int m = living[GPH_IX(k, GPH_MAX_MIGS)];
    if ((unsigned)m >= (unsigned)GPH_MAX_MIGS) continue;
    const int b = migi[GPH_IX(m * MG_COUNT + MG_BAND, GPH_MAX_MIGS * MG_COUNT)];
    if ((unsigned)b >= (unsigned)B) continue;
    band[k] = b;
    age[k] = mage[GPH_IX(m, GPH_MAX_MIGS)];
  }
  bool anyhit = false;
  for (int k = 0; k < GPH_MAX_MIGS; k++) {
    const int b = band[k];
    if (b < 0) continue;
    bool seen = false;
    for (int q = 0; q < k; q++) seen = seen || band[q] == b;
    if (seen) continue;                       /* the band's cell was updated at its first migration of the list */
    double first = age[k];
    for (int q = k + 1; q < GPH_MAX_MIGS; q++)
      if (band[q] == b && age[q] < first) first = age[q];
    const int c = GPH_IX(b * n + i, ncol);
    a[c] = a[c] + 1.0;
    a[GPH_IX(B * n + b * n + i, ncol)] = a[GPH_IX(B * n + b * n + i, ncol)] + first;
    gph_lanes_add(row + GPH_IX((1 + b) * n + i, nrow), 1u);
    anyhit = true;
  }
  if (anyhit) {
    a[GPH_IX(2 * B * n + i, ncol)] = a[GPH_IX(2 * B * n + i, ncol)] + 1.0;
    gph_lanes_add(row + GPH_IX(i, nrow), 1u);
  }
}

// what a lane keeps across the barriers: lane g < G the live migrations of the g-th locus of the group
struct GphAnLane {
  int mine = 0;
};

// workgroup w = block bx
GPH_FLAT(k_ancestry, GPH_AN_MAXTHREADS, GphLayout y, GphAnShape h, const char *pages, double *acc, uint32_t *row, int L)
{
  GPH_FLAT_BODY(GphAnLane);
  const int n = y.n, N = y.N, ncol = gph_an_locus_columns(n, y.B), upl = h.img.bytes / 16;
  const int j0 = bx * h.G;
  GphAnLds s;
  gph_an_carve(lds, N, h, s);
  GPH_PHASE {
    if (tid < h.G) {
      if (j0 + tid < L) ln.mine = gph_an_num_migs(pages + (size_t)(j0 + tid) * y.page_bytes, y);
      s.nm[tid] = ln.mine;
    }
  }
  if (!GPH_BLOCK_OR(mine)) return;       /* no live migration in the group: nothing staged, nothing touched (uniform over the workgroup) */
  GPH_PHASE {
    for (int u = tid; u < h.G * N; u += bd) {
      const int g = u / N, v = u - g * N;
      if (s.nm[GPH_IX(g, h.G)] > 0) {
        GphNode rec;
        gph_copy16(&rec, pages + (size_t)(j0 + g) * y.page_bytes + y.o_nd + (size_t)v * 16);
        s.up[GPH_IX(u, h.G * N)] = gph_an_up_word(&rec);
      }
    }
    for (int u = tid; u < h.G * upl; u += bd) {
      const int g = u / upl, o = (u - g * upl) * 16;
      if (s.nm[GPH_IX(g, h.G)] > 0)
        gph_copy16(s.img + (size_t)g * h.img.bytes + GPH_IX(o, h.img.bytes), pages + (size_t)(j0 + g) * y.page_bytes + gph_pack_unit_src(h.img, o));
    }
  }
  GPH_BARRIER;
  GPH_PHASE {
    if (tid < h.G && ln.mine > 0) gph_an_mark(s, y, h, tid);
  }
  GPH_BARRIER;
  GPH_PHASE {
    const int g = tid / n, i = tid - g * n;
    if (g < h.G && s.nm[g] > 0) gph_an_leaf(s, y, h, g, i, acc + (size_t)(j0 + g) * ncol, row);
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
