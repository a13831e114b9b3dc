// gph_sampler.h -- what the kernels of the statistics samplers (gph_coalstats.h, gph_timeslices.h, gph_ancestry.h) share:
// the function qualifiers of their two build forms, the fold of per-chunk partial rows into a sample's row, and the packed
// image of a few byte ranges of a page that a workgroup stages in LDS.
#pragma once
#include "gph_kernels.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 7

#ifdef GPH_HOSTEMU
#define GPH_SM_HD static inline
#define GPH_SM_FN static inline
#else
#define GPH_SM_HD __host__ __device__ inline     /* sizes and shapes: the host needs them to allocate and launch */
#define GPH_SM_FN __device__ inline
#endif

// ---- the fold.  A chunked sampler (coal stats, time slices) leaves one partial row of rd doubles per chunk of slots in
// HBM; column c of the sample's row is the partials added in chunk order 0, 1, ..., column 0 the sample's iteration
#define GPH_FOLD_THREADS 256

GPH_SM_FN void gph_fold_column(const double *part, int nchunks, int rd, int c, double iteration, double *row)
{
  double sum = 0.0;
  for (int ch = 0; ch < nchunks; ch++) sum = sum + part[(size_t)ch * rd + c];
  row[c] = c == 0 ? iteration : sum;
}

#ifndef GPH_HOSTEMU
// one lane per column
__global__ void __launch_bounds__(GPH_FOLD_THREADS) k_rows_fold(const double *part, int nchunks, int rd, double iteration, double *row)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < rd) gph_fold_column(part, nchunks, rd, c, iteration, row);
}
#else
static inline void k_rows_fold(GphBlk blk, const double *part, int nchunks, int rd, double iteration, double *row)
{
  for (int c = blk.x * blk.dim; c < (blk.x + 1) * blk.dim && c < rd; c++) gph_fold_column(part, nchunks, rd, c, iteration, row);
}
#endif

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
