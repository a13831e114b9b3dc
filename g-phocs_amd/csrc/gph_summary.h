// gph_summary.h -- k_locus_summary: per-locus posterior summaries accumulated on the device (include/gphocs_hip.h,
// gph_engine_locus_summary_*).  One lane per locus slot reads a few dozen bytes of its page (the values
// gph_engine_dump_loci prints) and updates fp64 accumulators in HBM.  The accumulators are column-major, [ncol][L] in
// slot order, so that every column's reads and writes coalesce across the lanes.  The kernel has one text (the flat-kernel
// form, gph_sampler.h); it writes no page, draws no random number and touches no chain state.
//
// Columns: 0-2 dataLnL, 3-5 genLnL, 6-8 TMRCA (shift, s1, s2 each), then per band the summed migration count and the
// number of samples with a migration (nmig.b at 9 + b, pmig.b at 9 + B + b), per population the summed coalescence count
// (9 + 2B + p), and under `locus-mut-rate VAR` the locus rate's shift, s1, s2 last.  shift is the value at the first
// sample; a later sample x adds d = x - shift to s1 and d * d to s2, in sample order, with plain (uncontracted) fp64
// operations: the sums can be rebuilt bit for bit from state dumps.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 3

enum { LS_DATALNL = 0, LS_GENLNL = 3, LS_TMRCA = 6, LS_FIXED = 9 };

GPH_SM_HD int gph_ls_columns(int K, int B, int var) { return LS_FIXED + 2 * B + K + (var ? 3 : 0); }

// one locus: pg = its page, a = its first accumulator (column c at a[c * L]); first = the first sample since the
// accumulators were zeroed
GPH_SM_FN void locus_summary_slot(const char *pg, const GphLayout &y, double *a, size_t L, int ncol, int first, int var)
{
  const double *fs = (const double *)(pg + y.o_fscal);
  const int32_t *is = (const int32_t *)(pg + y.o_iscal);
  const GphNode *nd = (const GphNode *)(pg + y.o_nd);
  const int16_t *nmig = (const int16_t *)(pg + y.o_nmig);
  const int16_t *ncoal = (const int16_t *)(pg + y.o_ncoal);
  auto col = [&](int c) -> double & { return a[(size_t)GPH_IX(c, ncol) * L]; };
  auto moment = [&](int c, double x) {
    if (first) { col(c) = x; col(c + 1) = 0.0; col(c + 2) = 0.0; return; }
    const double d = x - col(c);
    col(c + 1) = col(c + 1) + d;
    col(c + 2) = col(c + 2) + d * d;
  };
  moment(LS_DATALNL, fs[FS_DATALNL]);
  moment(LS_GENLNL, fs[FS_GENLNL]);
  moment(LS_TMRCA, nd[GPH_IX(is[IS_ROOT], y.N)].age);
  const int B = y.B, K = y.K;
  for (int b = 0; b < B; b++) {
    const double m = (double)nmig[GPH_IX(b, B)];
    const double hit = m > 0.0 ? 1.0 : 0.0;
    if (first) { col(LS_FIXED + b) = m; col(LS_FIXED + B + b) = hit; }
    else { col(LS_FIXED + b) = col(LS_FIXED + b) + m; col(LS_FIXED + B + b) = col(LS_FIXED + B + b) + hit; }
  }
  for (int p = 0; p < K; p++) {
    const double c = (double)ncoal[GPH_IX(p, K)];
    if (first) col(LS_FIXED + 2 * B + p) = c;
    else col(LS_FIXED + 2 * B + p) = col(LS_FIXED + 2 * B + p) + c;
  }
  if (var) moment(LS_FIXED + 2 * B + K, fs[FS_MUTRATE]);
}

#define GPH_LS_THREADS 256
// one lane per locus slot
GPH_FLAT(k_locus_summary, GPH_LS_THREADS, GphLayout y, const char *pages, double *acc, int L, int ncol, int first, int var)
{
  GPH_FLAT_BODY(GphNoLane);
  GPH_PHASE {
    const int j = bx * bd + tid;
    if (j < L) locus_summary_slot(pages + (size_t)j * y.page_bytes, y, acc + j, (size_t)L, ncol, first, var);
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
