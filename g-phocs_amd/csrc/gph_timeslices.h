// gph_timeslices.h -- k_time_slices (+ k_rows_fold, gph_sampler.h): the coalescence and migration statistics of one MCMC sample cut
// into S equal time slices per population branch and per migration band, genome-wide, computed on the device
// (include/gphocs_hip.h, gph_engine_time_slices_*).
//
// What is computed.  The population half restates code the reference carries but never reaches: recalcStats_partitioned /
// computeGenetreeStats_partitioned (patch.c:2357-2694) behind the numCoal_<pop>:<k> / deltaT_<pop>:<k> columns of
// printCoalStats (GPhoCS.c:927-935, 1000-1009).  The migration half is commented out upstream (patch.c:2527-2529,
// 2592-2596, 2606-2611) and is defined here.  Every event record of a chain carries (type, node, nlin, time): `time` the
// time elapsed since the previous event of the chain, `nlin` the lineages during that interval.  All arithmetic is IEEE
// double in the order written (the build has no contraction); u * t with an integer u is one multiplication.
//   population p, S slices:  a = popAge[p]; the root has ONE slice (patch.c:2541-2543), every other population S of width
//     w = (popAge[father(p)] - a) / S, the first boundary at end = a + w.  For every event e in chain order: t = e.time,
//     a += t; while a boundary lies below a (and the slice is not the last): t -= a - end, D[p][s] += nlin (nlin - 1) t,
//     s++, t = a - end, end += w; then D[p][s] += nlin (nlin - 1) t and, for a coalescence, C[p][s] += 1.
//   band b into population q:  the same walk over q's chain from popAge[q]; the band is live from its MIG_BAND_START
//     event (s = 0, w = (bandEnd[b] - bandStart[b]) / S, end = bandStart[b] + w) to its MIG_BAND_END event, inclusive;
//     while live M[b][s] += nlin t with the same splitting, and N[b][s] += 1 for an IN_MIG event whose migration node
//     belongs to band b.
// ONE deliberate difference from the reference: upstream drops a residue of at most 1e-7 that falls past the last boundary
// and aborts on a larger one (Fatal Error 9001); here the last slice takes whatever is left, so the slices of a branch add
// up to the page's own statistic (up to summation order) and no new abort exists.
//
// The chain as synchronizeEvents leaves it.  The engine defers the synchronizeEvents pass of an iteration into the head of
// the next sweep kernel (gph_engine.hip: sync_pending).  A sample taken in between sees event times that pass has not
// corrected yet.  The walker then applies the pass's own arithmetic (synchronize_events, gph_locus.h; patch.c:3548-3633) to
// every event it reads -- age += time; time' = time + (realAge - age), a negative time' above -1e-7 is 0; age = realAge --
// and uses time' (`vsync`): bit for bit the times the deferred pass will write, without writing them.  This needs the node
// ages and the migration ages of the locus next to the events.
//
// Shape.  The L slots of a rank are cut into contiguous chunks of `chunk` slots (GPH_TS_CHUNK unless told otherwise,
// gph_engine_time_slices_set_chunk).  Workgroup (c, t) of k_time_slices takes chunk c and tile t of the K + B walkers
// (walker W < K: population W; otherwise band W - K).  It goes through the chunk in groups of G loci: the group's event
// pools, node records, migration ages, chain heads and migration-node words are copied from the pages into LDS with
// 128-bit loads, consecutive lanes on consecutive 16-byte units (GphTsImg: five 16-byte-aligned byte ranges of a page, packed), then lane
// (g, w) = (tid / wt, tid % wt) walks the chain of walker t * wt + w of locus g out of LDS.  The accumulators of a lane
// live in LDS as [slice][lane], D / M as f64 and C / N as u32: whatever slice the lanes of a wavefront are in, lane l
// stays in bank l (mod 64) of the u32 array and in the word pair 2l, 2l + 1 of the f64 array (blockDim is a multiple of
// 64), so the updates are conflict-free, as in gph_coalstats.h.
// Sizes follow from K, B, S and the layout (gph_ts_shape): wt = all K + B walkers when one locus image and their
// accumulators (12 S bytes a lane) fit GPH_TS_LDS_MAX, otherwise the walkers are tiled over blockIdx.y; G = as many loci
// as keep the workgroup within GPH_TS_MAXTHREADS lanes and GPH_TS_LDS_PREF bytes (40 KB: four workgroups per CU of 160 KB).
//
// Summation order (what makes a row bitwise reproducible for a given locus count, chunk size and rank count): a lane's
// accumulator grows term by term in chain order, locus after locus (the loci g, g + G, g + 2G, ... of the chunk); at the
// end of the chunk ONE lane per (walker, slice) adds the G copies in the order g = 0, 1, ..., G - 1 into the chunk's
// partial row; k_rows_fold, one lane per column, adds the partial rows in chunk order.  No atomics, nothing
// depends on how workgroups are scheduled.  Counts are integers held as doubles.
//
// Each kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane, phase by phase.
// The kernels write no page, draw no random number and touch no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 5

#define GPH_TS_CHUNK 128          // slots per chunk (default)
#define GPH_TS_MAXS 32            // slices at most
#define GPH_TS_MAXTHREADS 256
#define GPH_TS_LDS_PREF 40960     // LDS bytes of a workgroup the group size G is grown to
#define GPH_TS_LDS_MAX 61440      // LDS bytes of a workgroup at most (one locus image + one wavefront of accumulators must fit)
#define GPH_TS_RANGES 5

// the part of a page a walk needs, packed (gph_sampler.h); a_*: image offsets of the arrays themselves
struct GphTsImg : GphPackedImg {
  int32_t a_ev, a_nd, a_mage, a_first, a_migi;
};
struct GphTsShape {
  int32_t S, G, wt, bd, ntiles, lds_bytes;
  GphTsImg img;
};

GPH_SM_HD int gph_ts_row_doubles(int K, int B, int S) { return 1 + 2 * S * (K + B); }
GPH_SM_HD int gph_ts_up64(int x) { return (x + 63) / 64 * 64; }
// LDS bytes beside the images and the accumulators: the model tables (4 f64 + 2 i32 arrays), padded
GPH_SM_HD int gph_ts_model_bytes(int K, int B) { return ((2 * K + 2 * B) * 8 + (K + B) * 4 + 15) / 16 * 16; }
GPH_SM_HD int gph_ts_lds_bytes(int K, int B, int S, int G, int bd, int img) { return G * img + gph_ts_model_bytes(K, B) + bd * S * 12; }

GPH_SM_HD void gph_ts_image(const GphLayout &y, GphTsImg &m)
{
  const int lo[GPH_TS_RANGES] = {y.o_ev, y.o_nd, y.o_mig_age, y.o_first, y.o_mig_i};
  const int sz[GPH_TS_RANGES] = {y.E * 16, y.N * 16, GPH_MAX_MIGS * 8, y.K * 2, GPH_MAX_MIGS * MG_COUNT * 2};
  int a[GPH_TS_RANGES];
  gph_pack_ranges(y, lo, sz, GPH_TS_RANGES, m, a);
  m.a_ev = a[0]; m.a_nd = a[1]; m.a_mage = a[2]; m.a_first = a[3]; m.a_migi = a[4];
}

// walkers per tile, loci per group, lanes: from K, B, S and the layout alone.  0: fine; 1: S out of range
GPH_SM_HD int gph_ts_shape(const GphLayout &y, int S, GphTsShape &h)
{
  if (S < 1 || S > GPH_TS_MAXS) return 1;
  const int K = y.K, B = y.B, W = K + B, per_lane = 12 * S, fixed = gph_ts_model_bytes(K, B);
  gph_ts_image(y, h.img);
  const int img = h.img.bytes;
  int wt = W < GPH_TS_MAXTHREADS ? W : GPH_TS_MAXTHREADS;
  while (wt > 1 && img + fixed + gph_ts_up64(wt) * per_lane > GPH_TS_LDS_MAX) wt = (wt + 1) / 2;
  const int ntiles = (W + wt - 1) / wt;
  wt = (W + ntiles - 1) / ntiles;
  int G = 1;
  while ((G + 1) * wt <= GPH_TS_MAXTHREADS && (G + 1) * img + fixed + gph_ts_up64((G + 1) * wt) * per_lane <= GPH_TS_LDS_PREF) G++;
  h.S = S; h.G = G; h.wt = wt; h.ntiles = ntiles; h.bd = gph_ts_up64(G * wt);
  h.lds_bytes = gph_ts_lds_bytes(K, B, S, G, h.bd, img);
  return 0;
}

// the LDS of a workgroup
struct GphTsLds {
  char *img;                 // [G][img.bytes]
  double *popAge, *sampleAge, *bandStart, *bandEnd;   // [K] [K] [B] [B]
  double *accD;              // [S][bd]
  int32_t *popFather, *bandTgt;                       // [K] [B]
  uint32_t *accC;            // [S][bd]
};
GPH_SM_FN void gph_ts_carve(char *base, int K, int B, const GphTsShape &h, GphTsLds &s)
{
  char *p = base;
  s.img = p; p += (size_t)h.G * h.img.bytes;
  s.popAge = (double *)p; p += (size_t)K * 8;
  s.sampleAge = (double *)p; p += (size_t)K * 8;
  s.bandStart = (double *)p; p += (size_t)B * 8;
  s.bandEnd = (double *)p; p += (size_t)B * 8;
  s.accD = (double *)p; p += (size_t)h.S * h.bd * 8;
  s.popFather = (int32_t *)p; p += (size_t)K * 4;
  s.bandTgt = (int32_t *)p; p += (size_t)B * 4;
  s.accC = (uint32_t *)p;
}

// entry q of the model tables (q < 2K + 2B: the f64 arrays, then the two i32 arrays) from the chain state
GPH_SM_FN void gph_ts_load_model(const GphTsLds &s, const GphModel &m, int K, int B, int q)
{
  if (q < K) s.popAge[GPH_IX(q, K)] = m.popAge[GPH_IX(q, GPH_MAXK)];
  else if (q < 2 * K) s.sampleAge[GPH_IX(q - K, K)] = m.sampleAge[GPH_IX(q - K, GPH_MAXK)];
  else if (q < 2 * K + B) s.bandStart[GPH_IX(q - 2 * K, B)] = m.bandStart[GPH_IX(q - 2 * K, GPH_MAXB)];
  else if (q < 2 * K + 2 * B) s.bandEnd[GPH_IX(q - 2 * K - B, B)] = m.bandEnd[GPH_IX(q - 2 * K - B, GPH_MAXB)];
  else if (q < 3 * K + 2 * B) s.popFather[GPH_IX(q - 2 * K - 2 * B, K)] = m.popFather[GPH_IX(q - 2 * K - 2 * B, GPH_MAXK)];
  else s.bandTgt[GPH_IX(q - 3 * K - 2 * B, B)] = m.bandTgt[GPH_IX(q - 3 * K - 2 * B, GPH_MAXB)];
}

// lane `lane` walks the chain of walker W in the staged image of locus g of the group
GPH_SM_FN void gph_ts_walk(const GphTsLds &s, const GphLayout &y, const GphTsShape &h, int lane, int g, int W, int vsync)
{
  const int K = y.K, B = y.B, S = h.S, bd = h.bd;
  const char *im = s.img + (size_t)GPH_IX(g, h.G) * h.img.bytes;
  const GphEv *evs = (const GphEv *)(im + h.img.a_ev);
  const GphNode *nd = (const GphNode *)(im + h.img.a_nd);
  const double *mage = (const double *)(im + h.img.a_mage);
  const int16_t *first = (const int16_t *)(im + h.img.a_first), *migi = (const int16_t *)(im + h.img.a_migi);
  const bool isband = W >= K;
  const int b = W - K;
  const int pop = isband ? s.bandTgt[GPH_IX(b, B)] : W;
  if ((unsigned)pop >= (unsigned)K) return;       /* (a damaged model must not reach past the tables) */
  const int father = s.popFather[GPH_IX(pop, K)];
  const bool root = pop == y.rootPop || (unsigned)father >= (unsigned)K;
  const double PREC = 0.0000001;
  double a = s.popAge[GPH_IX(pop, K)], age = a, w = 0.0, end = 0.0;
  int Sp = S, sl = 0;
  bool live = !isband;
  if (!isband) {
    if (root) Sp = 1;
    else { w = (s.popAge[GPH_IX(father, K)] - a) / (double)S; end = a + w; }
  }
  int e = first[GPH_IX(pop, K)];
  for (int guard = 0; e >= 0 && e < y.E && guard < y.E; guard++) {
    const GphEv R = evs[GPH_IX(e, y.E)];
    const int id = R.node;
    double t = R.time;
    if (vsync) {
      /* synchronize_events' arithmetic on this event, not written back */
      double real;
      age = age + R.time;
      switch (R.type) {
      case GPH_SAMPLES_START: real = s.sampleAge[GPH_IX(pop, K)]; break;
      case GPH_COAL: real = (unsigned)id < (unsigned)y.N ? nd[GPH_IX(id, y.N)].age : age; break;
      case GPH_IN_MIG:
      case GPH_OUT_MIG: real = (unsigned)id < (unsigned)GPH_MAX_MIGS ? mage[GPH_IX(id, GPH_MAX_MIGS)] : age; break;
      case GPH_MIG_BAND_START: real = (unsigned)id < (unsigned)B ? s.bandStart[GPH_IX(id, B)] : age; break;
      case GPH_MIG_BAND_END: real = (unsigned)id < (unsigned)B ? s.bandEnd[GPH_IX(id, B)] : age; break;
      case GPH_END_CHAIN: real = root ? age : s.popAge[GPH_IX(father, K)]; break;
      default: real = age; break;
      }
      t = R.time + (real - age);
      if (!(t < -PREC) && t < 0.0) t = 0.0;
      age = real;
    }
    a = a + t;
    if (live) {
      const int nl = R.nlin;
      const double u = isband ? (double)nl : (double)(nl * (nl - 1));
      while (sl < Sp - 1 && a > end) {
        t = t - (a - end);
        const int at = GPH_IX(sl * bd + lane, S * bd);
        s.accD[at] = s.accD[at] + u * t;
        sl++;
        t = a - end;
        end = end + w;
      }
      const int at = GPH_IX(sl * bd + lane, S * bd);
      s.accD[at] = s.accD[at] + u * t;
      if (!isband) {
        if (R.type == GPH_COAL) s.accC[at] = s.accC[at] + 1u;
      } else {
        if (R.type == GPH_IN_MIG && (unsigned)id < (unsigned)GPH_MAX_MIGS && migi[GPH_IX(id * MG_COUNT + MG_BAND, GPH_MAX_MIGS * MG_COUNT)] == b)
          s.accC[at] = s.accC[at] + 1u;
        if (R.type == GPH_MIG_BAND_END && id == b) break;
      }
    } else if (R.type == GPH_MIG_BAND_START && id == b) {
      live = true;
      sl = 0;
      w = (s.bandEnd[GPH_IX(b, B)] - s.bandStart[GPH_IX(b, B)]) / (double)S;
      end = s.bandStart[GPH_IX(b, B)] + w;
    }
    e = R.next;
  }
}

// cell q = (walker-in-tile, slice) of a tile into the chunk's partial row: the G copies in the order g = 0 .. G - 1
GPH_SM_FN void gph_ts_chunk_out(const GphTsLds &s, const GphLayout &y, const GphTsShape &h, int tile, int q, double *out)
{
  const int S = h.S, w = q / S, sl = q - w * S, W = tile * h.wt + w;
  if (W >= y.K + y.B) return;
  double d = 0.0;
  uint32_t c = 0;
  for (int g = 0; g < h.G; g++) {
    const int at = GPH_IX(sl * h.bd + g * h.wt + w, S * h.bd);
    d = d + s.accD[at];
    c += s.accC[at];
  }
  const int col = 1 + 2 * GPH_IX(W * S + sl, (y.K + y.B) * S);
  out[col] = (double)c;
  out[col + 1] = d;
}

// what a lane keeps across the barriers: which locus of a group and which walker it is
struct GphTsLane {
  int g = 0, Wk = 0;
  bool walker = false;
};

// workgroup (ch, tile) = block (bx, by)
GPH_FLAT(k_time_slices, GPH_TS_MAXTHREADS, GphLayout y, GphTsShape h, const GphGlobal *G, const char *pages, double *part, int L, int chunk,
         int rd, int vsync)
{
  GPH_FLAT_BODY(GphTsLane);
  const int K = y.K, B = y.B, W = K + B, ch = bx, tile = by;
  GphTsLds s;
  gph_ts_carve(lds, K, B, h, s);
  const int j0 = ch * chunk, j1 = j0 + chunk < L ? j0 + chunk : L, upl = h.img.bytes / 16;
  GPH_PHASE {
    for (int q = tid; q < h.S * bd; q += bd) { s.accD[q] = 0.0; s.accC[q] = 0u; }
    for (int q = tid; q < 3 * K + 3 * B; q += bd) gph_ts_load_model(s, G->model, K, B, q);
    ln.g = tid / h.wt; ln.Wk = tile * h.wt + (tid - ln.g * h.wt);
    ln.walker = ln.g < h.G && ln.Wk < W;
  }
  for (int jg = j0; jg < j1; jg += h.G) {
    const int nl = j1 - jg < h.G ? j1 - jg : h.G;
    GPH_BARRIER;        /* everybody is done with the previous group's images (first pass: with zeroing and the tables) */
    GPH_PHASE {
      for (int u = tid; u < nl * upl; u += bd) {
        const int loc = u / upl, o = (u - loc * upl) * 16;
        gph_copy16(s.img + (size_t)GPH_IX(loc, h.G) * h.img.bytes + GPH_IX(o, h.img.bytes),
                   pages + (size_t)(jg + loc) * y.page_bytes + gph_pack_unit_src(h.img, o));
      }
    }
    GPH_BARRIER;
    GPH_PHASE {
      if (ln.walker && ln.g < nl) gph_ts_walk(s, y, h, tid, ln.g, ln.Wk, vsync);
    }
  }
  GPH_BARRIER;
  double *out = part + (size_t)ch * rd;
  GPH_PHASE {
    for (int q = tid; q < h.wt * h.S; q += bd) gph_ts_chunk_out(s, y, h, tile, q, out);
    if (tile == 0 && tid == 0) out[0] = 0.0;
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
