// gph_sampler.h -- what the flat kernels share (the statistics samplers gph_coalstats.h, gph_timeslices.h, gph_ancestry.h,
// gph_genetrees.h, gph_clades.h, gph_summary.h, and k_apply_list / k_debug_math in gph_engine.hip): the ONE form a flat kernel
// is written in, the fold of per-chunk partial rows into a sample's row, and the packed image of a few byte ranges of a page
// that a workgroup stages in LDS.
#pragma once
#include "gph_kernels.h"
#ifdef GPH_HOSTEMU
#include <vector>
#endif

#undef GPH_FILE_ID
#define GPH_FILE_ID 7

// ---- the flat-kernel form.  A flat kernel has one text.  For gfx950 it is a __global__ function; in the host-emulation
// build it is a plain function that launch_grid (gph_backend.h) calls once per block, and the same text runs lane by lane,
// phase by phase:
//   GPH_FLAT(name, maxthreads, args...) { GPH_FLAT_BODY(Lane); ...   bd, bx, by (blockDim.x, blockIdx.x / .y) and `lds`, the
//                                  dynamic LDS, are block-uniform and visible in the whole kernel
//   GPH_PHASE { ... }              what the lanes do between two barriers; `tid` exists only here.  gfx950: a plain scope; host:
//                                  the loop over the bd lanes.  No `return` inside
//   GPH_BARRIER;                   stands between two phases: __syncthreads() / nothing
//   ln                             what a lane keeps from one phase to a later one: a per-kernel struct `Lane` (GphNoLane: nothing)
//                                  whose default member initialisers are the values at entry.  gfx950: a local; host: one of bd
//   GPH_BLOCK_OR(member)           barrier + whether ln.member is nonzero in any lane (between phases)
// Whatever stands outside a phase is block-uniform (the loop over the loci of a chunk, the carving of the LDS, pointers, an
// early return): every thread executes it on the device, the host executes it once.  The host launch hands over zeroed LDS;
// a kernel zeroes what it needs all the same.
// NOT in this form, on purpose: k_rng_ahead (gph_engine.hip) -- its device form works with wavefront shuffles, an LDS
// transpose and FMA quotients, its host form is the plain-division statement the tests pin; k_reduce_stage / k_global exist
// for the device only; the per-locus kernels have their own single text (GPH_KERNEL, GphCtx), and gph_emu64.h runs those.
struct GphNoLane {};
#ifdef GPH_HOSTEMU
#define GPH_SM_HD static inline
#define GPH_SM_FN static inline
#define GPH_FLAT(name, maxthreads, ...) static inline void name(GphBlk gph_blk, __VA_ARGS__)
#define GPH_FLAT_BODY(Lane) \
  const int bd = gph_blk.dim, bx = gph_blk.x, by = gph_blk.y; char *const lds = gph_blk.lds; \
  typedef Lane gph_lane_t; std::vector<gph_lane_t> gph_lanes((size_t)bd); (void)bx; (void)by; (void)lds
#define GPH_PHASE for (int tid = 0; tid < bd; tid++) if (gph_lane_t &ln = gph_lanes[(size_t)tid]; ((void)ln, true))
#define GPH_BARRIER ((void)0)
#define GPH_BLOCK_OR(member) gph_lanes_or(gph_lanes, &gph_lane_t::member)
template <class T, class M> static inline bool gph_lanes_or(const std::vector<T> &lanes, M T::*member)
{
  bool any = false;
  for (const T &l : lanes) any = any || l.*member != 0;
  return any;
}
#else
#define GPH_SM_HD __host__ __device__ inline     /* sizes and shapes: the host needs them to allocate and launch */
#define GPH_SM_FN __device__ inline
#define GPH_FLAT(name, maxthreads, ...) __global__ void __launch_bounds__(maxthreads) name(__VA_ARGS__)
#define GPH_FLAT_BODY(Lane) \
  extern __shared__ __attribute__((aligned(16))) char lds[]; \
  const int bd = blockDim.x, bx = blockIdx.x, by = blockIdx.y; Lane ln; (void)bx; (void)by; (void)ln
#define GPH_PHASE if (const int tid = threadIdx.x; true)
#define GPH_BARRIER __syncthreads()
#define GPH_BLOCK_OR(member) __syncthreads_or(ln.member)
#endif

// one 16-byte unit, both sides 16-byte aligned: one 128-bit load and one 128-bit store on the device
GPH_SM_FN void gph_copy16(void *dst, const void *src)
{
#ifdef GPH_HOSTEMU
  memcpy(dst, src, 16);
#else
  *(uint4 *)dst = *(const uint4 *)src;
#endif
}
// the order-free integer updates of a word that several lanes of a launch may hit: atomic on the device, plain on the host
// (one lane at a time there)
GPH_SM_FN void gph_lanes_add(uint32_t *p, uint32_t v)
{
#ifdef GPH_HOSTEMU
  *p += v;
#else
  (void)atomicAdd(p, v);
#endif
}
GPH_SM_FN void gph_lanes_bits(uint32_t *p, uint32_t bits)
{
#ifdef GPH_HOSTEMU
  *p |= bits;
#else
  (void)atomicOr(p, bits);
#endif
}

// ---- the fold.  A chunked sampler (coal stats, time slices) leaves one partial row of rd doubles per chunk of slots in
// HBM; column c of the sample's row is the partials added in chunk order 0, 1, ..., column 0 the sample's iteration
#define GPH_FOLD_THREADS 256
#define GPH_FOLD_AHEAD 16        // partial rows whose loads are in flight at once

GPH_SM_FN void gph_fold_column(const double *part, int nchunks, int rd, int c, double iteration, double *row)
{
  /* the adds stay one chain in chunk order; the loads of GPH_FOLD_AHEAD chunks are issued before the first of them is added
     (one load at a time left the lane waiting a memory latency per chunk: 1.49 ms for the 6 250 partial rows of k_sfs_tree) */
  double sum = 0.0;
  int ch = 0;
  for (; ch + GPH_FOLD_AHEAD <= nchunks; ch += GPH_FOLD_AHEAD) {
    double v[GPH_FOLD_AHEAD];
    for (int k = 0; k < GPH_FOLD_AHEAD; k++) v[k] = part[(size_t)(ch + k) * rd + c];
    for (int k = 0; k < GPH_FOLD_AHEAD; k++) sum = sum + v[k];
  }
  for (; ch < nchunks; ch++) sum = sum + part[(size_t)ch * rd + c];
  row[c] = c == 0 ? iteration : sum;
}

// one lane per column
GPH_FLAT(k_rows_fold, GPH_FOLD_THREADS, const double *part, int nchunks, int rd, double iteration, double *row)
{
  GPH_FLAT_BODY(GphNoLane);
  GPH_PHASE {
    const int c = bx * bd + tid;
    if (c < rd) gph_fold_column(part, nchunks, rd, c, iteration, row);
  }
}

// ---- the packed image.  The part of a page a kernel needs, copied into LDS with 128-bit loads, consecutive lanes on
// consecutive 16-byte units: range r < R = len[r] bytes from page offset src[r] at image offset dst[r] (all multiples of 16)
#define GPH_PACK_RANGES 5

struct GphPackedImg {
  int32_t src[GPH_PACK_RANGES], dst[GPH_PACK_RANGES], len[GPH_PACK_RANGES];
  int32_t R, bytes;
};

// R arrays of a page, sz[r] bytes at page offset lo[r]: each widened to 16-byte boundaries (and clamped to the page), one
// after the other; a[r] = image offset of array r itself
GPH_SM_HD void gph_pack_ranges(const GphLayout &y, const int *lo, const int *sz, int R, GphPackedImg &m, int *a)
{
  int at = 0;
  for (int r = 0; r < GPH_PACK_RANGES; r++) {
    m.src[r] = m.len[r] = 0;
    m.dst[r] = at;
    if (r >= R) continue;
    const int s = lo[r] & ~15;
    int e = (lo[r] + sz[r] + 15) & ~15;
    if (e > y.page_bytes) e = y.page_bytes;
    m.src[r] = s; m.len[r] = e - s;
    a[r] = at + (lo[r] - s);
    at += e - s;
  }
  m.R = R;
  m.bytes = at;
}

// the 16-byte unit at image offset o < bytes -> where it lies in the page (the unused ranges are empty and start at `bytes`:
// the search stops before them, and its trip count is a constant)
GPH_SM_FN int gph_pack_unit_src(const GphPackedImg &m, int o)
{
  int r = 0;
  while (r < GPH_PACK_RANGES - 1 && o >= m.dst[r] + m.len[r]) r++;
  return m.src[r] + (o - m.dst[r]);
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
