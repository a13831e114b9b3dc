// gph_coalstats.h -- k_coal_stats (+ k_rows_fold, gph_sampler.h): the genome-wide coalescent statistics ("coal stats") and sample-pair
// statistics ("node stats") of one MCMC sample, computed on the device (include/gphocs_hip.h, gph_engine_coal_stats_*).
//
// What is computed restates code the reference carries but never reaches (the call is guarded by
// `if (recordCoalStats && 0)`, GPhoCS.c:1771):
//   computeNodeStats, patch.c:2172-2270 (with computePairwiseLCAs, LocusDataLikelihood.c:1685-1830): for every locus
//     and every unordered pair of leaves (i, j), l = lca(i, j), P = pop(l): cnt[i,j,P] += 1, agesum[i,j,P] += age(l), and
//     first[i,j,P] += 1 when l is the first coalescence of population P in this locus -- the internal node of P with
//     the smallest age, the lowest node index among equal ages (patch.c:2217-2224: a strict `<` in index order).
//   computeFlatStats, patch.c:2278-2320 (with getSortedAges, LocusDataLikelihood.c:1216-1260): the n - 1 internal ages
//     of a locus sorted ascending, a[0..n-2]; with k = n, n-1, ..., 2 lineages and dT = a[0], then a[i] - a[i-1]:
//     migStat += dT * k, coalStat += (dT * k) * (k - 1).  Sample ages are ignored, as upstream: an ancient sample
//     counts as a lineage from time 0.
//   numCoal / numMig: the pages' coalescence counts per population / migration counts per band, summed; and the sums of
//     the loci's genealogy and data log-likelihoods.
//
// Shape.  The L slots of a rank are cut into contiguous chunks of `chunk` slots (GPH_CS_CHUNK unless the engine was told
// otherwise, gph_engine_coal_stats_set_chunk); workgroup (c, t) of k_coal_stats walks chunk c locus by locus for tile t of the pairs.  Per locus it
// stages only the node records (GphNode[N], N * 16 bytes of the page) in LDS -- the records of the next locus are
// already on their way in registers -- then
//   * every lane that owns an internal node v counts the internal nodes ordered before v by (age, index): the count is
//     v's rank among the sorted ages, and "no node of v's population before v" makes v its population's first
//     coalescence (one loop of broadcast LDS reads serves both);
//   * every lane owns ONE pair for the whole chunk (pair p = t * blockDim + lane, row-major over i < j) and finds its
//     LCA by climbing father links from whichever of the two nodes is younger (at most N steps);
//   * lane i of tile 0 owns term i of the flat statistics (the i-th sorted age) for the whole chunk.
// The accumulators of a lane live in LDS as [population][lane] (cnt and first as u32, agesum as f64): whatever
// populations the lanes of a wavefront hit, lane l stays in bank l (mod 64) of the u32 arrays and in the word pair
// 2l, 2l + 1 of the f64 array (a 64-bit access serves half a wavefront at a time), so the updates are conflict-free.
// blockDim is 64..256 lanes, the largest multiple of 64 whose accumulators (16 * K bytes a lane) fit GPH_CS_LDS_ACC =
// 48 KB: the whole allocation stays below 64 KB, so two workgroups and more are resident per CU (160 KB of LDS).  With
// more pairs than lanes the pairs are tiled over blockIdx.y (200 leaves: 19 900 pairs in 311 tiles of 64 at 40
// populations); every tile stages the node records itself.
//
// Summation order (what makes a row bitwise reproducible for a given locus count, chunk size and rank count): inside a
// chunk every accumulator is owned by one lane and grows in slot order; at the end of the chunk the n - 1 flat terms are
// added by one lane in term order i = 0 .. n-2, and the log-likelihoods were added by one lane in slot order.  The chunk's
// partial row goes to HBM; k_rows_fold, one lane per column, then adds the partials in chunk order 0, 1, ... into the
// sample's row.  No atomics, no dependence on how workgroups are scheduled.  Counts are integers held as doubles (exact
// below 2^53).  Ranks: each rank's row covers its own loci; the rows are added in rank order by whoever combines them
// (INTEGRATION.md).
//
// Each kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane, phase by phase.
// The kernels write no page, draw no random number and touch no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 4

// raw row: iteration, the four flat statistics, the two log-likelihood sums, then cnt, first, agesum as [pair][pop]
enum { CS_ITER = 0, CS_COALSTAT, CS_NUMCOAL, CS_MIGSTAT, CS_NUMMIG, CS_GENLNL, CS_DATALNL, CS_FIXED };
static_assert(CS_ITER == 0, "gph_fold_column writes the iteration into column 0");

#define GPH_CS_CHUNK 128        // slots per chunk (default)
#define GPH_CS_LDS_ACC 49152    // LDS bytes of a workgroup's pair accumulators at most
#define GPH_CS_MAXTHREADS 256

GPH_SM_HD int gph_cs_pairs(int n) { return n * (n - 1) / 2; }
GPH_SM_HD int gph_cs_row_doubles(int n, int K) { return CS_FIXED + 3 * gph_cs_pairs(n) * K; }
// lanes of a workgroup = pairs of a tile
GPH_SM_HD int gph_cs_block(int n, int K)
{
  int bd = (gph_cs_pairs(n) + 63) / 64 * 64;
  if (bd > GPH_CS_MAXTHREADS) bd = GPH_CS_MAXTHREADS;
  const int fit = GPH_CS_LDS_ACC / (16 * (K > 0 ? K : 1)) / 64 * 64;
  if (bd > fit) bd = fit;
  return bd < 64 ? 64 : bd;
}

// the LDS of a workgroup
struct GphCsLds {
  GphNode *nd;          // [N] node records of the current locus
  double *agesum;       // [K][bd]
  double *sorted;       // [n - 1] internal ages of the current locus, ascending
  double *flat_m, *flat_c;   // [n - 1] term i of migStat / coalStat, summed over the chunk's loci
  uint32_t *cnt, *first;     // [K][bd]
  int32_t *isf;         // [N] 1: the node is the first coalescence of its population in the current locus
  int32_t *evt;         // [K + B] coalescence / migration counts summed over the chunk's loci
};
GPH_SM_HD size_t gph_cs_lds_bytes(int n, int K, int B, int bd)
{
  const int N = 2 * n - 1;
  return (size_t)N * 16 + (size_t)K * bd * 8 + (size_t)(n - 1) * 24 + (size_t)K * bd * 8 + (size_t)N * 4 + (size_t)(K + B) * 4;
}
GPH_SM_FN void gph_cs_carve(char *base, int n, int K, int B, int bd, GphCsLds &s)
{
  const int N = 2 * n - 1;
  char *p = base;
  s.nd = (GphNode *)p; p += (size_t)N * 16;
  s.agesum = (double *)p; p += (size_t)K * bd * 8;
  s.sorted = (double *)p; p += (size_t)(n - 1) * 8;
  s.flat_m = (double *)p; p += (size_t)(n - 1) * 8;
  s.flat_c = (double *)p; p += (size_t)(n - 1) * 8;
  s.cnt = (uint32_t *)p; p += (size_t)K * bd * 4;
  s.first = (uint32_t *)p; p += (size_t)K * bd * 4;
  s.isf = (int32_t *)p; p += (size_t)N * 4;
  s.evt = (int32_t *)p;
}

// pair p (row-major over i < j) -> its two leaves
GPH_SM_FN void gph_cs_pair(int p, int n, int &i, int &j)
{
  int r = 0;
  while (r < n - 2 && p >= n - 1 - r) { p -= n - 1 - r; r++; }
  i = r;
  j = r + 1 + p;
}

// internal node v of the staged locus: its rank among the internal ages (ties: the lower index first) puts its age into
// the sorted array, and it is its population's first coalescence when no internal node of that population comes before it
// (patch.c:2217-2224)
GPH_SM_FN void gph_cs_rank_first(const GphCsLds &s, int n, int N, int v)
{
  const double av = s.nd[GPH_IX(v, N)].age;
  const int pv = s.nd[GPH_IX(v, N)].npop;
  int rank = 0, firstv = 1;
  for (int u = n; u < N; u++) {
    const double au = s.nd[GPH_IX(u, N)].age;
    const int before = au < av || (au == av && u < v);
    rank += before;
    if (before && s.nd[GPH_IX(u, N)].npop == pv) firstv = 0;
  }
  s.sorted[GPH_IX(rank, n - 1)] = av;
  s.isf[GPH_IX(v, N)] = firstv;
}

// lowest common ancestor of nodes a and b: when one is the other's father, that one is the answer's side and the child
// climbs (so a zero-length branch cannot send an ancestor past the LCA); otherwise the younger of the two climbs to its
// father, and with equal ages, where neither is then the other's father, the lower index.  At most 2N steps
GPH_SM_FN int gph_cs_lca(const GphCsLds &s, int N, int a, int b)
{
  for (int guard = 0; a != b && guard < 2 * N; guard++) {
    const GphNode &na = s.nd[GPH_IX(a, N)], &nb = s.nd[GPH_IX(b, N)];
    bool ca = na.father == b ? true : nb.father == a ? false : na.age < nb.age || (na.age == nb.age && a < b);
    if (ca && na.father < 0) ca = false;
    else if (!ca && nb.father < 0) ca = true;
    const int up = ca ? na.father : nb.father;
    if (up < 0 || up >= N) break;
    if (ca) a = up;
    else b = up;
  }
  return a;
}

// the pair owned by `lane` coalesces in node l in the staged locus
GPH_SM_FN void gph_cs_pair_add(const GphCsLds &s, int N, int K, int bd, int lane, int l)
{
  const GphNode &nl = s.nd[GPH_IX(l, N)];
  const int pop = GPH_IX(nl.npop, K);
  if ((unsigned)pop >= (unsigned)K) return;     /* (a damaged record must not reach past the accumulators) */
  const int at = pop * bd + lane;
  s.cnt[at] = s.cnt[at] + 1u;
  s.first[at] = s.first[at] + (uint32_t)s.isf[GPH_IX(l, N)];
  s.agesum[at] = s.agesum[at] + nl.age;
}

// term i of the flat statistics of the staged locus (patch.c:2307-2311): k = n - i lineages over the i-th interval
GPH_SM_FN void gph_cs_flat_add(const GphCsLds &s, int n, int i)
{
  const double dT = i == 0 ? s.sorted[0] : s.sorted[GPH_IX(i, n - 1)] - s.sorted[GPH_IX(i - 1, n - 1)];
  const double k = (double)(n - i);
  const double m = dT * k;
  s.flat_m[GPH_IX(i, n - 1)] = s.flat_m[GPH_IX(i, n - 1)] + m;
  s.flat_c[GPH_IX(i, n - 1)] = s.flat_c[GPH_IX(i, n - 1)] + m * (k - 1.0);
}

// the fixed columns of a chunk's partial row, by ONE lane: flat terms in term order, event counts
GPH_SM_FN void gph_cs_chunk_fixed(const GphCsLds &s, int n, int K, int B, double sgen, double sdata, double *out)
{
  double cs = 0.0, ms = 0.0;
  for (int i = 0; i < n - 1; i++) { ms = ms + s.flat_m[GPH_IX(i, n - 1)]; cs = cs + s.flat_c[GPH_IX(i, n - 1)]; }
  long long nc = 0, nm = 0;
  for (int p = 0; p < K; p++) nc += s.evt[GPH_IX(p, K + B)];
  for (int b = 0; b < B; b++) nm += s.evt[GPH_IX(K + b, K + B)];
  out[CS_ITER] = 0.0;
  out[CS_COALSTAT] = cs;
  out[CS_NUMCOAL] = (double)nc;
  out[CS_MIGSTAT] = ms;
  out[CS_NUMMIG] = (double)nm;
  out[CS_GENLNL] = sgen;
  out[CS_DATALNL] = sdata;
}

// entry q of a tile's pair accumulators (q = pair-in-tile * K + population) into the chunk's partial row
GPH_SM_FN void gph_cs_chunk_pair_out(const GphCsLds &s, int n, int K, int bd, int tile, int q, double *out)
{
  const int pr = q / K, pop = q - pr * K;
  const int npk = gph_cs_pairs(n) * K;
  const int col = GPH_IX((tile * bd + pr) * K + pop, npk);
  const int at = pop * bd + pr;
  out[CS_FIXED + col] = (double)s.cnt[at];
  out[CS_FIXED + npk + col] = (double)s.first[at];
  out[CS_FIXED + 2 * npk + col] = s.agesum[at];
}

// what a lane keeps across the barriers: its pair, the node record of the next locus (on its way while this one is worked on),
// the LCA of its pair, and (lane 0 of tile 0) the log-likelihoods of the locus and their sums over the chunk
struct GphCsLane {
  int la = 0, lb = 1, l = 0;
  GphNode pre = {0.0, -1, -1, -1, 0};
  double lg = 0.0, ld = 0.0, sgen = 0.0, sdata = 0.0;
};

// workgroup (ch, tile) = block (bx, by)
GPH_FLAT(k_coal_stats, GPH_CS_MAXTHREADS, GphLayout y, const char *pages, double *part, int L, int chunk)
{
  GPH_FLAT_BODY(GphCsLane);
  const int n = y.n, N = y.N, K = y.K, B = y.B, np = gph_cs_pairs(n), rd = gph_cs_row_doubles(n, K);
  const int ch = bx, tile = by;
  GphCsLds s;
  gph_cs_carve(lds, n, K, B, bd, s);
  const int valid = np - tile * bd < bd ? np - tile * bd : bd;
  const int j0 = ch * chunk, j1 = j0 + chunk < L ? j0 + chunk : L;
  GPH_PHASE {
    if (tid < valid) gph_cs_pair(tile * bd + tid, n, ln.la, ln.lb);
    for (int q = tid; q < K * bd; q += bd) { s.agesum[q] = 0.0; s.cnt[q] = 0u; s.first[q] = 0u; }
    for (int q = tid; q < n - 1; q += bd) { s.flat_m[q] = 0.0; s.flat_c[q] = 0.0; }
    for (int q = tid; q < K + B; q += bd) s.evt[q] = 0;
    if (tid < N && j0 < j1) ln.pre = ((const GphNode *)(pages + (size_t)j0 * y.page_bytes + y.o_nd))[tid];
  }
  for (int j = j0; j < j1; j++) {
    const char *pg = pages + (size_t)j * y.page_bytes;
    GPH_BARRIER;        /* everybody is done with the previous locus's records (first pass: with zeroing) */
    GPH_PHASE {
      if (tid < N) s.nd[tid] = ln.pre;
      for (int v = tid + bd; v < N; v += bd) s.nd[v] = ((const GphNode *)(pg + y.o_nd))[v];
      if (tid < N && j + 1 < j1) ln.pre = ((const GphNode *)(pg + y.page_bytes + y.o_nd))[tid];
      ln.lg = 0.0; ln.ld = 0.0;
      if (tile == 0 && tid == 0) { const double *fs = (const double *)(pg + y.o_fscal); ln.lg = fs[FS_GENLNL]; ln.ld = fs[FS_DATALNL]; }
    }
    GPH_BARRIER;
    GPH_PHASE {
      for (int v = n + tid; v < N; v += bd) gph_cs_rank_first(s, n, N, v);
      ln.l = tid < valid ? gph_cs_lca(s, N, ln.la, ln.lb) : 0;
    }
    GPH_BARRIER;        /* the first-coalescence flags and the sorted ages are complete */
    GPH_PHASE {
      if (tid < valid) gph_cs_pair_add(s, N, K, bd, tid, ln.l);
      if (tile == 0) {
        for (int i = tid; i < n - 1; i += bd) gph_cs_flat_add(s, n, i);
        const int16_t *ncoal = (const int16_t *)(pg + y.o_ncoal), *nmig = (const int16_t *)(pg + y.o_nmig);
        for (int q = tid; q < K + B; q += bd) s.evt[q] += q < K ? ncoal[q] : nmig[q - K];
        ln.sgen = ln.sgen + ln.lg;
        ln.sdata = ln.sdata + ln.ld;
      }
    }
  }
  GPH_BARRIER;
  double *out = part + (size_t)ch * rd;
  GPH_PHASE {
    for (int q = tid; q < valid * K; q += bd) gph_cs_chunk_pair_out(s, n, K, bd, tile, q, out);
    if (tile == 0 && tid == 0) gph_cs_chunk_fixed(s, n, K, B, ln.sgen, ln.sdata, out);
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
