// gph_engine.hip -- host side of the engine + __global__ wrappers (C ABI: include/gphocs_hip.h).
//
// Launch geometry: one 64-lane workgroup (one wavefront) per locus, grid = loci; the
// per-wave dynamic LDS holds the whole mutable state of the locus, so the number of
// resident waves per CU is LDS-bound (160 KiB / lds_bytes) -- L >> 256 CUs x waves/CU
// keeps every XCD busy and needs no blockIdx remap (loci are independent, nothing is
// shared between workgroups, so L2 affinity is irrelevant).
//
// An MCMC iteration is ONE stream of launches (gph_engine_iteration_): per-locus kernel -> fixed-shape reduction
// -> [RCCL all-gather of the reduced row, on the same stream] -> k_global (the decision above the loci, one
// wavefront, gph_global.h) -> predicated commit / revert kernel -> ... and a single host synchronisation at its end.
#include <stdio.h>
#include <stdlib.h>
#include <stddef.h>
#include <stdarg.h>
#include <string.h>
#include <vector>
#include <string>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <set>
#if defined(GPH_HOSTEMU) && defined(GPH_EMU64)
#define GPH_EMU64_IMPL      /* this translation unit holds the micro-wave scheduler (gph_emu64.h; test builds only) */
#endif
#include "gph_kernels.h"
#include "gph_global.h"
#include "gph_summary.h"
#include "gph_coalstats.h"
#include "gph_timeslices.h"
#include "gph_ancestry.h"
#include "gph_genetrees.h"
#include "gph_clades.h"
#include "gph_ess.h"
#include "gph_predictive.h"
#include "gph_simulate.h"
#include "gph_triplets.h"
#include "gph_pairtimes.h"
#include "gph_sfs.h"
#include "gph_mutations.h"
#include "gph_cladecmp.h"
#include "gph_comm.h"
#include "../../include/gphocs_hip.h"

#ifdef GPH_HOSTEMU
thread_local char *gph_sm = nullptr;
thread_local GphLds gph_lds;
GphLayout g_lay;
GphModel g_model;
GphGlobal *gph_G_emu = nullptr;
#ifdef GPH_BOUNDS
int gph_oob_word = 0;
#endif
#define GPH_KERNEL(name, ...) static void name(int gph_blk, __VA_ARGS__)
#define GPH_SWEEP_WAVES_ 6
#define GPH_SWEEP_ATTR
#define GPH_BLK gph_blk
#else
#define GPH_KERNEL(name, ...) __global__ __launch_bounds__(GPH_WAVE) void name(__VA_ARGS__)
#define GPH_BLK ((int)blockIdx.x)
// wavefronts per SIMD the sweep kernel is compiled for (the build passes it per capacity variant): 6 = 80 VGPRs, which
// every variant reaches without a spill -- beyond that LDS decides how many loci are resident; variant s is built for 8
#ifndef GPH_SWEEP_WAVES
#define GPH_SWEEP_WAVES 6
#endif
#define GPH_SWEEP_ATTR __attribute__((amdgpu_waves_per_eu(GPH_SWEEP_WAVES, GPH_SWEEP_WAVES)))
#define GPH_SWEEP_WAVES_ GPH_SWEEP_WAVES
#endif

// j0 = first slot of the launch group (see GphDev).  GphCtx reads the model from the kernel-argument segment (the host
// knows it when it launches: the genealogy sweep at the head of an iteration, the locus-rate kernels), GphCtxG from the
// device-resident chain state KA.G (everything launched after a decision the host has not seen yet)
GPH_KERNEL(k_init, GphKargs KA, GphDev D, int j0, uint32_t seedz, const double *mutRate, int preDraws) { GphCtxG lx; lx.kb_init(D, j0 + GPH_BLK, seedz, mutRate ? mutRate[j0 + GPH_BLK] : 1.0, preDraws); }
GPH_SWEEP_ATTR GPH_KERNEL(k_sweep, GphKargs KA, GphDev D, int j0, int flags, double ftCoal, double ftMig, double mix_c, double mix_lnc) { GphCtx lx; lx.kb_sweep<false>(D, j0 + GPH_BLK, flags, ftCoal, ftMig, mix_c, mix_lnc, 1.0); }
// the sweep of a heated chain (beta != 1, gph_engine_set_beta): a kernel of its own, chosen at launch, so that the sweep of the posterior carries no factor
GPH_SWEEP_ATTR GPH_KERNEL(k_sweep_heated, GphKargs KA, GphDev D, int j0, int flags, double ftCoal, double ftMig, double mix_c, double mix_lnc, double beta) { GphCtx lx; lx.kb_sweep<true>(D, j0 + GPH_BLK, flags, ftCoal, ftMig, mix_c, mix_lnc, beta); }
GPH_KERNEL(k_tau_eval, GphKargs KA, GphDev D, int j0, int fuse) { GphCtxG lx; lx.kb_tau_eval(D, j0 + GPH_BLK, GPH_G->tau, fuse); }
GPH_KERNEL(k_tau_finish, GphKargs KA, GphDev D, int j0, int unused) { (void)unused; GphCtxG lx; lx.kb_tau_finish(D, j0 + GPH_BLK); }
GPH_KERNEL(k_mix_eval, GphKargs KA, GphDev D, int j0, int fuse) { GphCtxG lx; lx.kb_mix_eval(D, j0 + GPH_BLK, GPH_G->mix_c, fuse); }
GPH_KERNEL(k_mix_finish, GphKargs KA, GphDev D, int j0, int unused) { (void)unused; GphCtxG lx; lx.kb_mix_finish(D, j0 + GPH_BLK); }
GPH_KERNEL(k_sync, GphKargs KA, GphDev D, int j0, int refresh) { GphCtxG lx; lx.kb_sync(D, j0 + GPH_BLK, refresh); }
GPH_KERNEL(k_check, GphKargs KA, GphDev D, int j0, int unused) { (void)unused; GphCtxG lx; lx.kb_check(D, j0 + GPH_BLK); }
GPH_KERNEL(k_unit, GphKargs KA, GphDev D, int j0, int op, int arg, double *out, int stride) { GphCtxG lx; lx.kb_unit(D, j0 + GPH_BLK, op, arg, out, stride); }
GPH_KERNEL(k_lrate_prep, GphKargs KA, GphDev D, int j0, double finetune, GphLrPre *pre) { GphCtx lx; lx.kb_lrate_prep(D, j0 + GPH_BLK, finetune, pre); }
GPH_KERNEL(k_lrate_scan, GphKargs KA, GphDev D, int j0, GphLrArgs A) { (void)j0; GphCtx lx; lx.kb_lrate_scan(D, A); }
GPH_KERNEL(k_lrate_apply, GphKargs KA, GphDev D, int j0, const GphLrRec *rec) { GphCtx lx; lx.kb_lrate_apply(D, j0 + GPH_BLK, rec); }

// ---------------------------------------------------------------- small elementwise / reduction kernels
#ifndef GPH_RED_BLOCKS
#define GPH_RED_BLOCKS 256
#endif
static_assert(2 * GPH_CAP_K + 2 * GPH_CAP_B <= GPH_RED_COLS && GPH_OUT_SLOTS <= 64, "the reduction kernels fold at most GPH_RED_COLS columns");

// UpdateTheta / UpdateMigRates accepted: the genLogLikelihood touch-ups of GPhoCS.c:3084-3093 and :3192-3200, every
// accepted proposal of the iteration in the order it was accepted (the list is in the chain state); one thread per locus
GPH_HD void apply_list_locus(char *pg, const GphLayout &y, const GphApply *ap, int na)
{
  double *fs = (double *)(pg + y.o_fscal);
  double v = fs[FS_GENLNL];
  for (int i = 0; i < na; i++) {
    const int idx = ap[i].idx;
    if (ap[i].kind == 0) {
      const int nc = ((int16_t *)(pg + y.o_ncoal))[idx];
      const double cs = ((double *)(pg + y.o_coal))[idx];
      v -= (ap[i].lnc * nc + ap[i].diff * cs);
    } else {
      const int nm = ((int16_t *)(pg + y.o_nmig))[idx];
      const double ms = ((double *)(pg + y.o_migst))[idx];
      v += (ap[i].lnc * nm - ap[i].diff * ms);
    }
  }
  fs[FS_GENLNL] = v;
}
// (a flat kernel: one text for both builds, gph_sampler.h)
#define GPH_FLAT_THREADS 256
GPH_FLAT(k_apply_list, GPH_FLAT_THREADS, GphKargs KA, GphDev D)
{
  GPH_FLAT_BODY(GphNoLane);
  const int na = KA.G->napply;
  GPH_PHASE {
    const int g = bx * bd + tid;
    if (g < D.L && na != 0) apply_list_locus(D.pages + (size_t)g * KA.lay.page_bytes, KA.lay, KA.G->apply, na);
  }
}
#ifndef GPH_HOSTEMU
// the stage above the loci (gph_global.h): one wavefront, every lane runs the same scalar code, lane 0's stores count
// ---- the stage(s) above the loci (gph_global.h) and the reductions that feed them, as ONE launch.
// The chain state (12 KB) and the ranks' reduced rows are staged through LDS by the whole block -- coalesced copies
// instead of a chain of dependent HBM round trips of a lone thread; thread 0 runs the stages in order.
struct GphStageList { int n; int stage[6]; int arg[6]; };
#define GPH_RED_SUBS 8
#define GPH_RED_THREADS (GPH_RED_SUBS * 64)
struct alignas(16) GphStageShared {
  char g[sizeof(GphGlobal)];
  double r[GPH_RED_ROW];
};
__device__ void stages_body(GphKargs &KA, const double *rows, int world, const GphStageList &SL, int iteration, GphStageShared &sh)
{
  typedef uint32_t gu32x4 __attribute__((ext_vector_type(4)));
  static_assert(sizeof(GphGlobal) % 16 == 0, "the chain state is copied in 16-byte units");
  const int tid = threadIdx.x, nt = blockDim.x;
  const gu32x4 *src = (const gu32x4 *)KA.G;
  gu32x4 *dst = (gu32x4 *)sh.g;
  for (int i = tid; i < (int)(sizeof(GphGlobal) / 16); i += nt) dst[i] = src[i];
  /* the ranks' rows combined in rank order (the same additions on every rank), one column per thread step */
  for (int c = tid; c < GPH_RED_ROW; c += nt) {
    const int within = c % GPH_RED_STRIDE, kind = within < 3 * GPH_RED_COLS ? within / GPH_RED_COLS : 3;
    double v = rows[c];
    for (int r = 1; r < world; r++) {
      const double w = rows[(size_t)r * GPH_RED_ROW + c];
      v = kind == 0 ? v + w : kind == 1 ? (w < v ? w : v) : (w > v ? w : v);
    }
    sh.r[c] = v;
  }
  __syncthreads();
  if (tid == 0) {
    GphGlobal &G = *(GphGlobal *)sh.g;
    G.iteration = iteration;
    GphRed R;
    R.rows = sh.r; R.world = 1;
    for (int k = 0; k < SL.n; k++) gg_stage(G, R, SL.stage[k], SL.arg[k]);
  }
  __syncthreads();
  gu32x4 *out = (gu32x4 *)KA.G;
  for (int i = tid; i < (int)(sizeof(GphGlobal) / 16); i += nt) out[i] = dst[i];
}
__global__ void __launch_bounds__(GPH_RED_THREADS) k_global(GphKargs KA, const double *rows, int world, GphStageList SL, int iteration)
{
  __shared__ __attribute__((aligned(16))) GphStageShared sh;
  stages_body(KA, rows, world, SL, iteration, sh);
}

// fixed-shape two-level reduction (deterministic run to run): block b owns a contiguous chunk of
// loci; inside it Q = 8 * (64 / column width) sub-sequences (g = g0+q, g0+q+Q, ...) are summed in index
// order and combined in sub-sequence order; the final pass adds the 256 block partials in a fixed shape.
// mode 0 = per-locus outputs (GPH_OUT_SLOTS columns), mode 1 = compact statistics (2K+2B columns)
// part: [3][GPH_RED_BLOCKS][GPH_RED_COLS] (sum, min, max) per section
// one sub-sequence of a column (g, g + step, ... below g1) folded in index order.  The loads of GPH_RED_UNROLL steps are
// issued together and folded as they arrive: one load in flight per thread made these loops a chain of memory
// latencies (a dozen to fifty of them per reduction, six reductions per iteration)
#define GPH_RED_UNROLL 16
__device__ __forceinline__ void reduce_run(const double *src, int stride, int col, int g, int g1, int step, double &s, double &mn, double &mx)
{
  for (; g < g1; g += step * GPH_RED_UNROLL) {
    double v[GPH_RED_UNROLL];
#pragma unroll
    for (int u = 0; u < GPH_RED_UNROLL; u++) {
      const int gg = g + u * step;
      v[u] = gg < g1 ? src[(size_t)gg * stride + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < GPH_RED_UNROLL; u++)
      if (g + u * step < g1) { s += v[u]; mn = v[u] < mn ? v[u] : mn; mx = v[u] > mx ? v[u] : mx; }
  }
}
// cbase: first column of the window this call folds (at most 128 columns a call; the many-band build's statistics row is
// folded window by window).  A column's additions have the shape of ITS window's width, not of the row's: Q = 8 sub-sequences
// in a full window of 128, and in the last window whatever its own width gives -- at 278 columns the first 256 are folded with
// Q = 8 and the last 22 (a window of 22: cw = 32) with Q = 16.  Fixed for a given column count, so still the same run to run;
// tests/reduce_util.py restates the shape and the probe gph_debug_reduce_ holds the kernel to it bit for bit
__device__ void reduce_partial_body(const GphDev &D, int mode, int ncols, int cbase, int stride_cols, double *part, double (*sh)[GPH_RED_SUBS * 4][16])
{
  /* a wavefront covers 64 / cw loci at a time (cw = columns rounded up to 16, 32 or 64): every lane has work */
  const int cw = ncols <= 16 ? 16 : ncols <= 32 ? 32 : ncols <= 64 ? 64 : 128;
  const int b = blockIdx.x;
  const int chunk = (D.L + GPH_RED_BLOCKS - 1) / GPH_RED_BLOCKS;
  const int g0 = b * chunk, g1 = g0 + chunk < D.L ? g0 + chunk : D.L;
  const double *src = (mode == 0 ? D.out : D.stats) + cbase;
  const int stride = mode == 0 ? GPH_OUT_SLOTS : stride_cols;
  part += cbase;
  if (cw == 128) {
    /* more than 64 columns (the largest capacity variant): two columns per lane, one locus per wavefront step */
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    for (int half = 0; half < 2; half++) {
      const int col = lane + 64 * half;
      double s = 0.0, mn = 1e300, mx = -1e300;
      if (col < ncols) reduce_run(src, stride, col, g0 + q, g1, GPH_RED_SUBS, s, mn, mx);
      for (int c0 = 64 * half; c0 < ncols && c0 < 64 * (half + 1); c0 += 16) {
        __syncthreads();
        if (col >= c0 && col < c0 + 16) { sh[0][q][col - c0] = s; sh[1][q][col - c0] = mn; sh[2][q][col - c0] = mx; }
        __syncthreads();
        if (threadIdx.x < 16 && c0 + (int)threadIdx.x < ncols) {
          const int c = threadIdx.x;
          double ts = 0.0, tmn = 1e300, tmx = -1e300;
          for (int k = 0; k < GPH_RED_SUBS; k++) {
            ts += sh[0][k][c];
            tmn = sh[1][k][c] < tmn ? sh[1][k][c] : tmn;
            tmx = sh[2][k][c] > tmx ? sh[2][k][c] : tmx;
          }
          part[(0 * GPH_RED_BLOCKS + b) * GPH_RED_COLS + c0 + c] = ts;
          part[(1 * GPH_RED_BLOCKS + b) * GPH_RED_COLS + c0 + c] = tmn;
          part[(2 * GPH_RED_BLOCKS + b) * GPH_RED_COLS + c0 + c] = tmx;
        }
      }
    }
    __syncthreads();
    return;
  }
  const int ng = 64 / cw, Q = GPH_RED_SUBS * ng;
  const int lane = threadIdx.x & 63, col = lane % cw, q = (threadIdx.x >> 6) * ng + lane / cw;
  double s = 0.0, mn = 1e300, mx = -1e300;
  if (col < ncols) reduce_run(src, stride, col, g0 + q, g1, Q, s, mn, mx);
  /* combine the Q sub-sequences of a column in sub-sequence order; 16 columns at a time through shared memory */
  for (int c0 = 0; c0 < ncols; c0 += 16) {
    __syncthreads();
    if (col >= c0 && col < c0 + 16) { sh[0][q][col - c0] = s; sh[1][q][col - c0] = mn; sh[2][q][col - c0] = mx; }
    __syncthreads();
    if (threadIdx.x < 16 && c0 + (int)threadIdx.x < ncols) {
      const int c = threadIdx.x;
      double ts = 0.0, tmn = 1e300, tmx = -1e300;
      for (int k = 0; k < Q; k++) {
        ts += sh[0][k][c];
        tmn = sh[1][k][c] < tmn ? sh[1][k][c] : tmn;
        tmx = sh[2][k][c] > tmx ? sh[2][k][c] : tmx;
      }
      part[(0 * GPH_RED_BLOCKS + b) * GPH_RED_COLS + c0 + c] = ts;
      part[(1 * GPH_RED_BLOCKS + b) * GPH_RED_COLS + c0 + c] = tmn;
      part[(2 * GPH_RED_BLOCKS + b) * GPH_RED_COLS + c0 + c] = tmx;
    }
  }
  __syncthreads();
}
// final pass: column c's block partials in block order, as GPH_RED_SUBS contiguous runs combined in run order -- a
// fixed shape, so the result does not depend on scheduling.  Up to 64 columns (every variant but the largest): thread
// (run, column), one run each; beyond: thread (h, column) folds runs h and h + 4.  A run's 3 x 32 partials are fetched
// 48 loads at a time: these are reads of other XCDs' writes, a microsecond or two each
__device__ void reduce_final_body(int ncols, int cbase, const double *part, double *red, double (*sh)[GPH_RED_SUBS][128])
{
  part += cbase; red += cbase;
  const int cw = ncols <= 64 ? 64 : 128;
  const int col = threadIdx.x % cw, h = threadIdx.x / cw;
  const int per = GPH_RED_BLOCKS / GPH_RED_SUBS;
  static_assert((GPH_RED_BLOCKS / GPH_RED_SUBS) % 16 == 0, "the final pass folds sixteen block partials per step");
  for (int sub = h; sub < GPH_RED_SUBS; sub += GPH_RED_THREADS / cw) {
    double s = 0.0, mn = 1e300, mx = -1e300;
    if (col < ncols)
      for (int b0 = sub * per; b0 < (sub + 1) * per; b0 += 16) {
        double vs[16], vn[16], vx[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
          vs[u] = part[(0 * GPH_RED_BLOCKS + b0 + u) * GPH_RED_COLS + col];
          vn[u] = part[(1 * GPH_RED_BLOCKS + b0 + u) * GPH_RED_COLS + col];
          vx[u] = part[(2 * GPH_RED_BLOCKS + b0 + u) * GPH_RED_COLS + col];
        }
#pragma unroll
        for (int u = 0; u < 16; u++) { s += vs[u]; mn = vn[u] < mn ? vn[u] : mn; mx = vx[u] > mx ? vx[u] : mx; }
      }
    if (col < 128) { sh[0][sub][col] = s; sh[1][sub][col] = mn; sh[2][sub][col] = mx; }
  }
  __syncthreads();
  if (h == 0 && col < ncols) {
    double s = 0.0, mn = 1e300, mx = -1e300;
    for (int k = 0; k < GPH_RED_SUBS; k++) {
      s += sh[0][k][col];
      mn = sh[1][k][col] < mn ? sh[1][k][col] : mn;
      mx = sh[2][k][col] > mx ? sh[2][k][col] : mx;
    }
    red[col] = s;
    red[GPH_RED_COLS + col] = mn;
    red[2 * GPH_RED_COLS + col] = mx;
  }
  __syncthreads();
}
// reduction of section 0 (nc0 columns of the per-locus outputs) and / or section 1 (nc1 columns of the statistics) into
// this rank's row; the LAST block to finish its partials (ticket) does the final pass and -- do_stage: a single rank, whose
// row is everybody's -- runs the stages that consume the row in the same launch.  Several ranks gather their rows on the
// stream behind this kernel and run the stages in k_global (gph_backend.h: flush_pending); the kernel waits for nobody
__global__ void __launch_bounds__(GPH_RED_THREADS) k_reduce_stage(GphKargs KA, GphDev D, int nc0, int nc1, double *part, unsigned *ticket, double *red,
                                                                  int do_stage, GphStageList SL, int iteration)
{
  __shared__ union { double p[3][GPH_RED_SUBS * 4][16]; double f[3][GPH_RED_SUBS][128]; GphStageShared st; } sh;
  __shared__ int s_last;
  if (nc0 > 0) reduce_partial_body(D, 0, nc0, 0, nc0, part, sh.p);
  for (int cb = 0; cb < nc1; cb += 128) reduce_partial_body(D, 1, nc1 - cb < 128 ? nc1 - cb : 128, cb, nc1, part + 3 * GPH_RED_BLOCKS * GPH_RED_COLS, sh.p);
  __syncthreads();
  /* ONE release per block (thread 0, after the block barrier: cumulative over the block's stores) -- an agent-scope
   * fence writes the L2 back, and 2048 wavefronts doing it cost more than the reduction itself */
  if (threadIdx.x == 0) { __threadfence(); s_last = atomicAdd(ticket, 1u) == gridDim.x - 1; }
  __syncthreads();
  if (!s_last) return;
  /* every wavefront of the last block acquires for itself before it reads the other blocks' partials (they were
   * written through other XCDs' L2s): one agent-scope fence per wavefront of ONE block -- the memory model asks for
   * it, the cache-wide invalidate of thread 0's fence only happened to cover the other waves */
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (nc0 > 0) reduce_final_body(nc0, 0, part, red, sh.f);
  for (int cb = 0; cb < nc1; cb += 128) reduce_final_body(nc1 - cb < 128 ? nc1 - cb : 128, cb, part + 3 * GPH_RED_BLOCKS * GPH_RED_COLS, red + GPH_RED_STRIDE, sh.f);
  if (threadIdx.x == 0) { red[3 * GPH_RED_COLS] = (double)*D.err; *ticket = 0; }
  __syncthreads();
  /* (ONE call site in this kernel: with two the compiler stops inlining the stage body, the by-reference kernel arguments go
   * through a 72-byte stack frame, and the kernel faults at address 0 on its first launch with stages -- measured, round 5) */
  if (do_stage) stages_body(KA, red, 1, SL, iteration, sh.st);
}
#endif

// parity probe: the device's exp/log (gph_math.h) and its native sqrt / divide / floor
GPH_FLAT(k_debug_math, GPH_FLAT_THREADS, GphKargs KA, const double *x, const double *y, int n, double *o)
{
  GPH_FLAT_BODY(GphNoLane);
  (void)KA;
  GPH_PHASE {
    const int i = bx * bd + tid;
    if (i < n) {
      o[i] = gph_exp(x[i]);
      o[n + i] = gph_log(x[i]);
      o[2 * n + i] = sqrt(fabs(x[i]));
      o[3 * n + i] = x[i] / y[i];
      o[4 * n + i] = floor(x[i]);
    }
  }
}
// ... and the sweep's accept test: gph_accept(u = y, x) next to the plain y < gph_exp(x), and what the bounds alone said
GPH_FLAT(k_debug_accept, GPH_FLAT_THREADS, GphKargs KA, const double *x, const double *y, int n, double *o)
{
  GPH_FLAT_BODY(GphNoLane);
  (void)KA;
  GPH_PHASE {
    const int i = bx * bd + tid;
    if (i < n) {
      o[i] = (double)gph_accept(y[i], x[i]);
      o[n + i] = (double)(y[i] < gph_exp(x[i]));
      o[2 * n + i] = (double)gph_accept_bounds_t<false>(y[i], x[i]);
    }
  }
}

// ---------------------------------------------------------------- the sweep's uniforms, generated ahead of it
// One lane per locus slot: the three Wichmann-Hill recurrences of the slot's stream from the generator state in its page
// (read only) and the draws exactly as l_rndu(GphRng &) forms them -- serial per locus, 64 loci per instruction here, where
// k_sweep spent 5.7 % of its dependent instruction stream on them.  Per slot: the first n_ahead = min(M, roundup64(k_prev + 64))
// draws (k_prev: what the locus consumed in its previous sweep), the state after every C of them and after the last one.
// The consumer is GphRngA (gph_locus.h), which goes on by itself where the draws end.
GPH_HD int rng_ahead_count(int kprev, int M)
{
  int n = (kprev + 64 + 63) & ~63;
  return n < 0 ? 0 : n > M ? M : n;
}
// Two forms on purpose (not the flat-kernel form of gph_sampler.h): the host form below is the plain-division statement of
// l_rndu that the tests pin, the device form reaches the same bits with shuffles, an LDS transpose and FMA quotients.
#ifdef GPH_HOSTEMU
static void k_rng_ahead(GphBlk b, GphKargs KA, GphDev D)
{
  const int cs = D.ra_cshift, nck = (D.ra_M >> cs) + 1;
  for (int slot = b.x * b.dim; slot < (b.x + 1) * b.dim && slot < D.L; slot++) {
    const int32_t *is = (const int32_t *)(D.pages + (size_t)slot * KA.lay.page_bytes + KA.lay.o_iscal);
    uint32_t x = (uint32_t)is[IS_RX], y = (uint32_t)is[IS_RY], z = (uint32_t)is[IS_RZ];
    const int n = rng_ahead_count(D.ra_kprev[slot], D.ra_M);
    for (int d = 0; d <= n; d++) {
      if ((d & ((1 << cs) - 1)) == 0) {
        uint32_t *c = D.ra_ckpt + 4 * ((size_t)GPH_IX(d >> cs, nck) * D.L + slot);
        c[0] = x; c[1] = y; c[2] = z; c[3] = 0;
      }
      if (d == n) break;
      GPH_RNG_STEP(x, y, z);
      const double r = x / 30269.0 + y / 30307.0 + z / 30323.0;
      D.ra_draws[(size_t)slot * D.ra_M + GPH_IX(d, D.ra_M)] = r - (int)r;
    }
    uint32_t *t = D.ra_tail + 4 * (size_t)slot;
    t[0] = x; t[1] = y; t[2] = z; t[3] = (uint32_t)n;
  }
}
#else
// A tile of 64 loci x 16 draws goes through LDS so that a store instruction writes whole 128-byte lines: 16 lanes per
// locus, 4 loci per instruction (a lane-strided store would be 64 separate 8-byte transactions).  The checkpoints and the
// tail are laid out with the slot as the fastest index: lane-consecutive 16-byte stores.
#define GPH_RA_TILE 16
__global__ void __launch_bounds__(GPH_WAVE) k_rng_ahead(GphKargs KA, GphDev D)
{
  typedef uint32_t gu32x4 __attribute__((ext_vector_type(4)));
  __shared__ double tile[GPH_WAVE][GPH_RA_TILE + 1];
  __shared__ int n_of[GPH_WAVE];
  const int lane = threadIdx.x, slot0 = blockIdx.x * GPH_WAVE, slot = slot0 + lane;
  const bool live = slot < D.L;
  const int cs = D.ra_cshift, nck = (D.ra_M >> cs) + 1;
  const double rx = KA.mathc[26], ry = KA.mathc[27], rz = KA.mathc[28], mx = KA.mathc[29], my = KA.mathc[30], mz = KA.mathc[31];
  uint32_t x = 0, y = 0, z = 0;
  int n = 0;
  gu32x4 *ckpt = (gu32x4 *)D.ra_ckpt;
  if (live) {
    const int32_t *is = (const int32_t *)(D.pages + (size_t)slot * KA.lay.page_bytes + KA.lay.o_iscal);
    x = (uint32_t)is[IS_RX]; y = (uint32_t)is[IS_RY]; z = (uint32_t)is[IS_RZ];
    n = rng_ahead_count(D.ra_kprev[slot], D.ra_M);
    ckpt[slot] = gu32x4{x, y, z, 0u};
  }
  n_of[lane] = n;
  int nmax = n;
  for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(nmax, o, GPH_WAVE); nmax = w > nmax ? w : nmax; }
  __syncthreads();
  for (int d0 = 0; d0 < nmax; d0 += GPH_RA_TILE) {
    if (d0 < n) {      /* (n is a multiple of 64, the tile divides 64: a tile is generated in full or not at all) */
#pragma unroll
      for (int t = 0; t < GPH_RA_TILE; t++) {
        GPH_RNG_STEP(x, y, z);
        /* x / 30269.0 + y / 30307.0 + z / 30323.0 with the exact quotients of l_rndu (gph_locus.h) */
        const double xd = (double)x, yd = (double)y, zd = (double)z;
        double q;
        q = xd * rx; const double qx = __builtin_fma(__builtin_fma(-q, mx, xd), rx, q);
        q = yd * ry; const double qy = __builtin_fma(__builtin_fma(-q, my, yd), ry, q);
        q = zd * rz; const double qz = __builtin_fma(__builtin_fma(-q, mz, zd), rz, q);
        tile[lane][t] = __builtin_amdgcn_fract(qx + qy + qz);
      }
      const int d1 = d0 + GPH_RA_TILE;
      if ((d1 & ((1 << cs) - 1)) == 0) ckpt[(size_t)GPH_IX(d1 >> cs, nck) * D.L + slot] = gu32x4{x, y, z, 0u};
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < GPH_WAVE / 4; i++) {
      const int r = (lane >> 4) + 4 * i, c = lane & 15;
      if (slot0 + r < D.L && d0 < n_of[r]) D.ra_draws[(size_t)(slot0 + r) * D.ra_M + GPH_IX(d0 + c, D.ra_M)] = tile[r][c];
    }
    __syncthreads();
  }
  if (live) ((gu32x4 *)D.ra_tail)[slot] = gu32x4{x, y, z, (uint32_t)n};
}
#endif

// ---------------------------------------------------------------- engine object
#define GPH_NCLS 29     // (18: k_rng_ahead, 19: k_clades, 20: k_clades_compare, 21: k_ess, 22: k_predictive, 23: k_triplets, 24: k_mutations, 25: k_simulate, 26: k_pair_times, 27: k_sfs_tree, 28: k_sfs_data) kernel classes of gph_engine_last_kernel_ms (the chain state counts evaluations for the first 16)
// the two buffers the statistics samplers keep on the device (alloc / free / fetch: sampler scaffold below)
struct SmRows {      // the rows of the samples taken since the last fetch: [cap][n] elements of esz bytes, `fill` of them taken
  char *d = nullptr;
  size_t esz = 0;
  int32_t n = 0, cap = 0, fill = 0;
};
struct SmParts {     // one partial row of rd doubles per chunk of `chunk` slots, folded into a sample's row by k_rows_fold
  double *d_part = nullptr;
  int32_t rd = 0, chunk = 0, nchunks = 0;
  int32_t chunk_next = 0;      // slots per chunk of the next alloc (the _set_chunk entry points; 0: the default)
};

struct SmSel {       // a selection of loci: those of this rank, global indices in increasing order, and the page slot of each in HBM
  std::vector<int64_t> loci;
  int32_t *d_slot = nullptr;
};
struct SmSelected {  // a sampler over a selection: what gene trees, clades, ESS, predictive checks and triplet weights keep alike
  bool on = false;
  SmSel sel;
  int64_t samples = 0;                    // since the accumulators were last zeroed
  char *d = nullptr;                      // its block on the device, in selection order
  size_t bytes = 0;
  SmRows rows;                            // per-sample rows with their iterations, where the sampler takes any
  std::vector<int32_t> iters;
  int (*zero)(gph_engine *) = nullptr;    // the accumulators back to zero, queued: the sampler's own step (selected_on sets it)
};

// what both builds keep of an engine; gph_backend.h completes it (struct gph_engine) with the members only one has
struct gph_engine_state {
  gph_config cfg;
  std::vector<int32_t> samplesPerPop, popFather, popSon0, popSon1, bandSrc, bandTgt;
  GphLayout lay;
  GphDev dev;
  // chain state above the loci (gph_types.h: GphGlobal): host mirror (pinned) and the copy in HBM the kernels read.
  // Between iterations both are equal; inside an iteration the device copy leads (resident mode) or the host
  // mirror does (host mode: a caller-supplied all-reduce hook forces a synchronisation per reduction anyway)
  GphGlobal *G_h = nullptr, *G_d = nullptr;
  bool G_dirty = true;               // the host mirror was changed since it was last pushed
  int64_t n_huge = 0;                // loci whose sequence block stays in HBM (the first slots)
  int32_t last_error_code = 0;       // the last fatal error check_error reported (gph_engine_last_error)
  long long last_error_locus = -1;
  char last_error_text[288] = "";    // the line a refused gph_engine_load_loci printed (gph_engine_last_error_text)
  bool in_error_dump = false;
  int64_t L = 0;
  size_t cond_bytes = 0, pages_bytes = 0, seq_bytes_total = 0;
  std::vector<uint64_t> h_cond_off;
  std::vector<int32_t> h_P;          // per slot (sorted order)
  std::vector<int32_t> h_orig;       // slot -> original local index
  std::vector<int64_t> h_sites;      // per local locus: the alignment columns it stands for (the counts of its unphased patterns)
  struct Bucket { int j0, count, lds_bytes; };   // a launch group: slots [j0, j0+count), dynamic LDS per wave
  std::vector<Bucket> buckets;
  double *d_mutRate = nullptr;
  int init_predraws = 0;             // rndu() draws every locus spent before its genealogy is sampled (VAR start-up: 1)
  bool var_rates = false;            // locus rates are part of the state (dumped as "R" lines)
  // UpdateLocusRate: per-slot records, input-order -> slot map, result scalars, scratch for pattern-rich loci
  GphLrRec *d_lrec = nullptr;
  GphLrPre *d_lpre = nullptr;
  double lr_hits = 0;                // proposals of the last update decided with the prepared likelihood
  int32_t *d_slot_of = nullptr;
  double *d_lr_result = nullptr, *d_lr_gscr = nullptr;
  char *d_ref_page = nullptr, *d_ref_seq = nullptr;   // the reference locus's node records / scalars and sequence block on this rank
  std::vector<uint64_t> h_seq_off;
  GphLrArgs lr;
  int lr_lds_bytes = 0;
  int lds_pad[16] = {0};             // GPH_LDS_PAD="class:bytes,...": extra dynamic LDS per kernel class (occupancy experiments)
  // reductions: block partials, this rank's reduced row (GPH_RED_ROW doubles) and every rank's row after the all-gather
  double *d_part = nullptr, *d_red = nullptr, *d_gather = nullptr;
  double *h_red = nullptr;                       // pinned: this rank's row (host mode)
  // several ranks, one process per GPU: a native communicator (RCCL all-gather on the engine's stream, or -- ranks
  // sharing one GPU, tests only -- a host shared-memory exchange) or a caller-supplied hook
  gph_comm *comm = nullptr;
  gph_allreduce_fn allreduce = nullptr;
  void *allreduce_user = nullptr;
  bool force_host = false;           // GPH_HOST_DECISIONS=1: decisions on the host although nothing requires it (tests)
  int64_t n_syncs = 0, n_collectives = 0, n_launches = 0;   // host synchronisations / cross-rank exchanges / kernel launches so far
  uint32_t seedz = 0;
  bool loaded = false, seeded = false, model_set = false, initialized = false;
  GphKargs ka;                 // first argument of every kernel: model, layout, math constants, table addresses
  bool sync_pending = false;   // synchronizeEvents of the finished iteration rides at the head of the next sweep kernel
  bool fin_owed = false;       // the commit / revert of the last decided tau / sample-age proposal has not run yet
  bool mix_owed = false;       // the commit of the last decided mixing proposal has not run yet (it rides at the head of the next sweep kernel)
  int32_t slog_sel = 0;        // loci selected for the decision-level transcript (GPH_LOGSTEPS builds)
  bool mirror_current = true;  // the host mirror G_h holds what the device-side stages last wrote (false between a queued stage and pull_G)
  bool no_fuse = false;        // GPH_NO_FUSE=1 (tests): every finish as a kernel of its own; read once in gph_engine_create
  // the sweep's uniforms generated ahead of it (k_rng_ahead); read once in gph_engine_create:
  // GPH_RNG_AHEAD=0 off, GPH_RNG_AHEAD_DRAWS=<M> draws kept per locus at most (a multiple of 64), GPH_RNG_AHEAD_CKPT=16|64 draws
  // between two checkpoints, GPH_RNG_AHEAD_FIRST=<n> draws generated for a locus's first sweep
  bool rng_ahead = true;
  // placement of the pass: B (resident mode: the pass for the next sweep goes out behind this one's kernel on a stream of its
  // own and overlaps the tau / mixing kernels) or A (GPH_RNG_AHEAD_PLACE=A, and whenever B's draws cannot be trusted: right in
  // front of the sweep kernel).  B's draws are those of the pages as the sweep left them: they hold for the next sweep of the
  // chained iterations only, and only while ra_b_valid stands: whatever else steps a locus's generator or rewrites the pages'
  // generator states (k_init, the locus-rate kernels, k_unit, a stepwise sweep, the tests' hook) takes it down
  bool ra_place_b = true, ra_b_valid = false;
  int32_t ra_M = 512, ra_C = 16, ra_first = 320;
  size_t ra_bytes = 0;
  gph_counters counters = {0, 0, 0.0, 0};
  // the statistics samplers; all null / 0 while a feature is off
  // per-locus summaries (gph_summary.h): [ncol][L] accumulators in slot order, samples since they were last zeroed
  struct { double *d = nullptr; int32_t ncol = 0; int64_t samples = 0; std::vector<std::string> names; } ls;
  // genome-wide coalescent / sample-pair statistics (gph_coalstats.h)
  struct { SmParts part; SmRows rows; int32_t bd = 0; std::string name; } cs;
  // time-sliced coalescence / migration statistics (gph_timeslices.h)
  struct { SmParts part; SmRows rows; GphTsShape shape = {}; std::string name; } ts;
  // per-locus, per-sample migration ancestry (gph_ancestry.h): fp64 accumulators [L][ncol] in slot order, the integer rows
  // of the samples and their iterations
  struct { double *d_acc = nullptr; SmRows rows; int32_t ncol = 0; int64_t samples = 0; GphAnShape shape = {}; std::vector<int32_t> iters; std::string name; } an;
  // sampled genealogies of selected loci (gph_genetrees.h): the rows of records, the selected loci of this rank (global indices,
  // increasing) with their slots in HBM, and the iterations of the rows held
  struct : SmSelected { GphGtShape shape = {}; } gt;       // (no block, no accumulators: on while it has a row buffer)
  // clade tables of selected loci (gph_clades.h): entries [nsel][P][W + 2] (the block) and header words [nsel][2] in selection order
  // d_cmp: the rows of the last gph_engine_clades_compare this engine led ([nsel][GPH_CC_COLS], allocated by the first one)
  struct : SmSelected { uint32_t *d_hdr = nullptr; GphClShape shape = {}; double *d_cmp = nullptr;
                        uint64_t *ent() const { return (uint64_t *)d; } } cl;
  // effective sample sizes of selected loci (gph_ess.h): ONE buffer in selection order -- acc [nsel][M][GPH_ESS_WORDS] doubles,
  // focal [nsel][n - 1][W] u64, prev [nsel] u64, changes [nsel] u32 (one buffer: a fetch is one copy and one synchronisation)
  struct : SmSelected { size_t o_focal = 0, o_prev = 0, o_changes = 0; GphClShape shape = {}; int32_t M = 0; int64_t max_bytes = 0; } es;
  // posterior predictive checks of selected loci (gph_predictive.h): ONE buffer in selection order -- acc [nsel][C][5] doubles,
  // observed [C] u64 (the data's totals), key [nsel] u64 (Kl of each locus), pop [n] bytes (leaf -> current population) --, the
  // per-sample rows [cap][C] u64 with their iterations, the sites of each selected locus
  struct : SmSelected { size_t o_obs = 0, o_key = 0, o_pop = 0; GphPdShape shape = {}; std::vector<int64_t> sites; uint64_t seed = 0; std::string name; } pd;
  // triplet topology weights of selected loci (gph_triplets.h): ONE buffer in selection order -- acc [nsel][2][3 T] doubles (W,
  // then A, of every slot), tri [T] packed triples, pop [n + Kc] bytes (leaf -> current population, then n_p) --, the per-sample
  // rows [cap][3 T] u64 with their iterations, the triples as the caller sees them
  struct : SmSelected { size_t o_tri = 0, o_pop = 0; GphTrShape shape = {}; std::vector<int32_t> tri; std::string name; } tr;
  // expected substitutions of selected loci (gph_mutations.h): the block is acc [nsel][C] doubles in selection order; one partial
  // row of 1 + C doubles per chunk of selected loci, folded into the per-sample rows [cap][1 + C] (column 0: the iteration)
  struct : SmSelected { SmParts part; GphMuShape shape = {}; std::string name; } mu;
  // replicate genealogies of selected loci (gph_simulate.h): ONE buffer in selection order -- acc [nsel][W] doubles, then (with
  // sites) sacc [nsel][C][5] doubles and sobs [C] u64 as the predictive checks keep them; behind them key [nsel] u64, skey [nsel]
  // u64 (the site level's Kl), pop [n] bytes, recs [nsel][record]: the latest sample's replicates --, the per-sample rows
  // [cap][RC + C] u64 with their iterations
  struct : SmSelected { size_t o_sacc = 0, o_sobs = 0, o_key = 0, o_skey = 0, o_pop = 0, o_rec = 0; GphSiShape shape = {}; GphGtShape gshape = {};
                        GphPdShape pshape = {}; int32_t C = 0; std::vector<int64_t> sites; std::string name; } si;
  // pairwise coalescence-time distributions of selected loci (gph_pairtimes.h): ONE buffer in selection order -- acc [nsel][4][NP]
  // doubles (A, Y, X, M of every slot), pair [NP] packed pairs, edges [E] doubles, pop [n + Kc] bytes --, the per-sample rows
  // [cap][NP (B + 2)] u64 with their iterations, the pairs and edges as the caller sees them
  struct : SmSelected { size_t o_pair = 0, o_edge = 0, o_pop = 0; GphPtShape shape = {}; std::vector<int32_t> pairs; std::vector<double> edges; std::string name; } pt;
  // site-frequency spectra of selected loci (gph_sfs.h): ONE buffer in selection order -- acc [nsel][NS] doubles (E of every slot);
  // behind it the data side, formed once at enable: obs [nsel][NS], use [nsel][NG], sites [nsel] u32, tot [NS + NG + 1] u64 (their
  // totals over the selection); then the tables: slot [NS], sgrp [NS], gdef [NG], gbase [NG] i32, pop [n + Kc] bytes --, one partial
  // row of 1 + NS doubles per workgroup of G selected loci, folded into the per-sample rows [cap][1 + NS] (column 0: the iteration)
  struct : SmSelected { SmParts part; size_t o_obs = 0, o_use = 0, o_sites = 0, o_tot = 0, o_slot = 0, o_sgrp = 0, o_gdef = 0, o_gbase = 0, o_pop = 0;
                        GphSfShape shape = {}; std::vector<int32_t> slot, sgrp, gdef, gbase; std::string name; } sf;
  // the samplers with accumulators over a selection, in the order gph_engine_init_genealogies zeroes them
  std::vector<SmSelected *> selected() { return {&cl, &es, &pd, &tr, &mu, &si, &pt, &sf}; }
  double last_ms[GPH_NCLS] = {0};
  // per kernel class: launches, summed HIP-event ms; evaluations / bytes / nodes live in the chain state
  double cls_launches[GPH_NCLS] = {0}, cls_ms[GPH_NCLS] = {0};
  double cls_evals0[16] = {0}, cls_bytes0[16] = {0}, cls_nodes0[16] = {0};   // offsets of the last reset
  int last_which = 0;
  uint32_t timing_mask = 0xffffffffu;   // classes whose launches are bracketed by HIP events
};

static int align_up(int x, int a) { return (x + a - 1) / a * a; }

// page + LDS layout for (n, K, B): everything sized by the ACTUAL dimensions, not by the
// reference's MAX_* caps (sizeof(Locus_SuperStruct) alone is 9.7 KB there)
static void build_layout(GphLayout &y, int n, int Kc, int K, int B, int rootPop, int Pmax, int cnt16)
{
  memset(&y, 0, sizeof y);
  y.n = n; y.N = 2 * n - 1; y.K = K; y.Kc = Kc; y.B = B; y.rootPop = rootPop;
  y.E = 2 * n + 4 * GPH_MAX_MIGS + 3 * B + K + 10;   // event pool, patch.c:92
  y.RB = GPH_MAX_MIGS + 2 * B;
  // the HBM page IS the page part of the static LDS image (GphLds, capacity-sized arrays):
  // staging is one fully coalesced 16-B/lane copy
#define OFS(f) ((int32_t)offsetof(GphLds, f))
  y.o_ev = OFS(ev); y.o_nd = OFS(nd); y.o_sv = OFS(sv); y.o_mig_age = OFS(mig_age);
  y.o_coal = OFS(coal); y.o_migst = OFS(migst); y.o_rb_age = OFS(rb_age); y.o_fscal = OFS(fscal);
  y.o_iscal = OFS(iscal);
  y.o_nev = OFS(nev);
  y.o_first = OFS(first);
  y.o_mig_i = OFS(mig_i); y.o_living = OFS(living); y.o_ncoal = OFS(ncoal); y.o_nmig = OFS(nmig); y.o_rb_i = OFS(rb_i);
  y.page_bytes = align_up(OFS(s_dcoal), 16);
#undef OFS
  // dynamic LDS: the locus' sequence block (same bytes as its HBM block, laid out by its own P: GPH_Q_* in
  // gph_types.h) + per-pattern terms of the root reduction for loci with more than one pattern per lane
  y.Pmax = Pmax;
  y.cnt16 = cnt16;
  y.dyn_bytes = 0;
  y.lds_bytes = GPH_Q_TERMS(Pmax, n, cnt16) + (Pmax > GPH_WAVE ? 8 * Pmax : 8 * GPH_WAVE);
  y.huge_P = 0x7fffffff;
}

static void build_model_static(gph_engine_state *e)
{
  GphModel &m = e->G_h->model;
  const gph_config &c = e->cfg;
  memset(&m, 0, sizeof m);
  for (int p = 0; p < c.K; p++) {
    m.popFather[p] = e->popFather[p];
    m.popSon0[p] = e->popSon0[p];
    m.popSon1[p] = e->popSon1[p];
    gph_popmask mask = 0;
    for (int d = 0; d < c.K; d++) {           // isAncestralTo, self-inclusive (MCMCcontrol.c:851,977,1015-1024)
      int x = d;
      while (x >= 0) { if (x == p) { mask |= (gph_popmask)1 << d; break; } x = e->popFather[x]; }
    }
    m.isAnc[p] = mask;
  }
  int cum = 0;
  for (int p = 0; p < c.Kc; p++) { m.samplesPerPop[p] = e->samplesPerPop[p]; cum += e->samplesPerPop[p]; m.cumSamples[p] = cum; }
  for (int b = 0; b < c.B; b++) { m.bandSrc[b] = e->bandSrc[b]; m.bandTgt[b] = e->bandTgt[b]; m.bandsInto[e->bandTgt[b]][b >> 5] |= 1u << (b & 31); }
  for (int p = 0; p < c.K; p++)
    for (int b = 0; b < c.B; b++) if ((m.isAnc[e->bandTgt[b]] >> p) & 1) m.bandsOver[p][b >> 5] |= 1u << (b & 31);
  // populationPostOrder(rootPop), patch.c:1936-1951
  std::vector<int> order;
  struct Rec { static void go(gph_engine_state *e, int pop, std::vector<int> &o) {
    if (pop >= e->cfg.Kc) { go(e, e->popSon0[pop], o); go(e, e->popSon1[pop], o); }
    o.push_back(pop); } };
  Rec::go(e, c.rootPop, order);
  for (size_t i = 0; i < order.size(); i++) m.postOrder[i] = order[i];
  GphGlobal &G = *e->G_h;
  G.n = c.n; G.K = c.K; G.Kc = c.Kc; G.B = c.B; G.rootPop = c.rootPop; G.Ltot = (double)c.L_total;
  G.tau_limit = (long long)1 << 62;
}

#ifdef GPH_ACCSTAT
// host build with -DGPH_ACCSTAT: the sweep's accept tests by site (l_accept, gph_locus.h), printed when the library is unloaded
long long gph_as[3][3];
struct GphAsPrint { ~GphAsPrint() { static const char *site[3] = {"internal node", "migration node", "SPR"};
  for (int s = 0; s < 3; s++) fprintf(stderr, "ACCSTAT %s: tests %lld, lnacc < 0 %lld, decided by the bounds %lld\n", site[s], gph_as[s][0], gph_as[s][1], gph_as[s][2]); } } gph_as_print;
#endif
#ifdef GPH_WALKSTAT
long long gph_ws[4];
struct GphWsPrint { ~GphWsPrint() { fprintf(stderr, "WALKSTAT proposals %lld: prune steps %.2f, regraft steps %.2f, common prefix %.2f per proposal\n", gph_ws[3], (double)gph_ws[0] / gph_ws[3], (double)gph_ws[1] / gph_ws[3], (double)gph_ws[2] / gph_ws[3]); } } gph_ws_print;
#endif
// ---------------------------------------------------------------- the backend
// the model in the kernel-argument segment (every build but the many-band one, whose kernels all read G->model)
#if GPH_BIG_BANDS
#define GPH_KA_MODEL(ka, e) ((void)0)
#else
#define GPH_KA_MODEL(ka, e) ((ka).model = (e)->G_h->model)
#endif
// exp/log/rndu constants of gph_math.h / gph_locus.h (GphKargs::mathc); the device build adds the addresses of the two
// 128-entry libm tables
static void fill_math_constants(GphKargs &ka)
{
  const double ec[8] = GPH_EXP_CONSTS, lc[18] = GPH_LOG_CONSTS;
  const double rc[6] = {1.0 / 30269.0, 1.0 / 30307.0, 1.0 / 30323.0, 30269.0, 30307.0, 30323.0};
  memcpy(&ka.mathc[0], ec, sizeof ec);
  memcpy(&ka.mathc[8], lc, sizeof lc);
  memcpy(&ka.mathc[26], rc, sizeof rc);
}
static int world_of(const gph_engine *e);
// memory and stream, the chain state's two copies (push_G: host mirror -> HBM after the host changed settings or, in host
// mode, took a decision; pull_G: back), the engine's resources, the reductions, the launch functions: one form per build
#include "gph_backend.h"
static int world_of(const gph_engine *e) { return e->comm ? gph_comm_world(e->comm) : 1; }
static int push_if_dirty(gph_engine *e) { return e->G_dirty ? push_G(e) : 0; }

static int reduce_stats(gph_engine *e) { return reduce_local(e, 1, 2 * e->cfg.K + 2 * e->cfg.B); }

// which columns of the reduced row a stage consumes (host mode with a caller-supplied all-reduce hook: only these
// travel): sums / minima / maxima as (section, column) pairs; every stage that follows a locus kernel also takes the
// counters and the error words
struct StageCols { int ns = 0, nm = 0, nx = 0; int s[GPH_RED_COLS + 32][2], m[8][2], x[8][2]; };
static void stage_columns(const gph_engine *e, int stage, StageCols &c)
{
  const int C = 2 * e->cfg.K + 2 * e->cfg.B;
  auto S = [&](int sec, int col) { c.s[c.ns][0] = sec; c.s[c.ns][1] = col; c.ns++; };
  auto M = [&](int sec, int col) { c.m[c.nm][0] = sec; c.m[c.nm][1] = col; c.nm++; };
  auto X = [&](int sec, int col) { c.x[c.nx][0] = sec; c.x[c.nx][1] = col; c.nx++; };
  auto counters = [&]() { S(0, 8); S(0, 9); S(0, 10); S(0, 13); X(0, 11); X(0, -1); };
  auto totals = [&]() { for (int k = 0; k < C; k++) S(1, k); };
  switch (stage) {
  case GS_INIT_DONE: counters(); S(0, 0); S(0, 1); totals(); break;
  case GS_SWEEP_DONE: counters(); for (int k = 0; k < 8; k++) S(0, k); S(0, 12); M(0, 15); totals(); break;
  case GS_TOTALS: totals(); break;
  case GS_TAU_DECIDE: case GS_SAGE_DECIDE: counters(); S(0, 0); S(0, 1); S(0, 3); S(0, 4); M(0, 14); break;
  case GS_MIX_DECIDE: counters(); S(0, 0); break;
  case GS_REFRESH_DONE: counters(); M(0, 0); S(0, 1); S(0, 2); break;
  case GS_CHECK_DONE: counters(); M(0, 0); S(0, 1); S(0, 2); totals(); break;
  case GS_COUNT_ONLY: counters(); S(0, 0); S(0, 1); S(0, 3); S(0, 4); M(0, 14); break;   /* + what the stepwise evaluate calls return */
  default: break;
  }
}
static bool stage_reads_row(int stage)
{
  switch (stage) {
  case GS_INIT_DONE: case GS_SWEEP_DONE: case GS_TOTALS: case GS_TAU_DECIDE: case GS_SAGE_DECIDE: case GS_MIX_DECIDE:
  case GS_REFRESH_DONE: case GS_CHECK_DONE: case GS_COUNT_ONLY: return true;
  default: return false;
  }
}
static double *colp(double *row, const int sc[2], int kind)   /* kind 0 sum, 1 min, 2 max; column -1 = the error word */
{
  if (sc[1] < 0) return row + 3 * GPH_RED_COLS;
  return row + sc[0] * GPH_RED_STRIDE + kind * GPH_RED_COLS + sc[1];
}

// one stage above the loci (gph_global.h: gg_stage) on the reduced row(s) of the launch(es) before it.
// resident mode: [all-gather on the stream] + k_global, no host synchronisation.
// host mode: synchronise, fetch this rank's row, combine it over the ranks (hook or shared-memory exchange), run
// gg_stage on the host mirror and push the mirror.
static int run_stage(gph_engine *e, int stage, int arg, int iteration)
{
  int rc;
  bool queued;
  if ((rc = stage_defer(e, stage, arg, iteration, queued)) || queued) return rc;
  GphRed R;
  R.rows = e->h_red; R.world = 1;
  if (stage_reads_row(stage)) {
    if ((rc = pull_row(e))) return rc;
    if (e->allreduce || e->comm) {
      StageCols c;
      stage_columns(e, stage, c);
      double sums[GPH_RED_COLS + 32], mins[16];
      for (int k = 0; k < c.ns; k++) sums[k] = *colp(e->h_red, c.s[k], 0);
      for (int k = 0; k < c.nm; k++) mins[k] = *colp(e->h_red, c.m[k], 1);
      for (int k = 0; k < c.nx; k++) mins[c.nm + k] = -*colp(e->h_red, c.x[k], 2);   /* a maximum as the minimum of the negatives */
      if (e->allreduce) rc = e->allreduce(e->allreduce_user, sums, c.ns, mins, c.nm + c.nx);
      else rc = gph_comm_allreduce_host(e->comm, sums, c.ns, mins, c.nm + c.nx);
      if (rc) return GPH_EHIP;
      e->n_collectives++;
      for (int k = 0; k < c.ns; k++) *colp(e->h_red, c.s[k], 0) = sums[k];
      for (int k = 0; k < c.nm; k++) *colp(e->h_red, c.m[k], 1) = mins[k];
      for (int k = 0; k < c.nx; k++) *colp(e->h_red, c.x[k], 2) = -mins[c.nm + k];
    }
  }
  e->G_h->iteration = iteration;
  gg_stage(*e->G_h, R, stage, arg);
  return push_G(e);
}

// one locus in the canonical text form (same format as oracle/gphocs_oracle_io.c go_dump_state's per-locus part): pg = its
// page, cb = its conditionals (or null)
static void dump_one_locus(const gph_engine *e, FILE *f, long long global_locus, const char *pg, const char *cb, int P)
{
  const GphLayout &y = e->lay;
  const double *fs = (const double *)(pg + y.o_fscal);
  const int32_t *is = (const int32_t *)(pg + y.o_iscal);
  const GphNode *nd = (const GphNode *)(pg + y.o_nd);
  const int16_t *ne = (const int16_t *)(pg + y.o_nev);
  const int16_t *first = (const int16_t *)(pg + y.o_first);
  const GphEv *evr = (const GphEv *)(pg + y.o_ev);
  fprintf(f, "LOCUS %lld root %d dataLnL %a genLnL %a rng %u %u %u\n", (long long)global_locus, is[IS_ROOT],
          fs[FS_DATALNL], fs[FS_GENLNL], (unsigned)is[IS_RX], (unsigned)is[IS_RY], (unsigned)is[IS_RZ]);
  if (e->var_rates) fprintf(f, "R %a\n", fs[FS_MUTRATE]);
  for (int i = 0; i < y.N; i++)
    fprintf(f, "N %d %d %d %d %a %d %d\n", i, nd[i].father, nd[i].left, nd[i].right, nd[i].age, nd[i].npop, i < y.n ? -1 : ne[i]);
  for (int pop = 0; pop < y.K; pop++) {
    fprintf(f, "C %d", pop);
    int guard = 0;
    for (int ev = first[pop]; ev >= 0 && guard++ < y.E; ev = evr[ev].next)
      fprintf(f, " %d:%d:%d:%d:%a", ev, evr[ev].type, evr[ev].node, evr[ev].nlin, evr[ev].time);
    fprintf(f, "\n");
  }
  fprintf(f, "S");
  for (int pop = 0; pop < y.K; pop++)
    fprintf(f, " %a %d", ((const double *)(pg + y.o_coal))[pop], ((const int16_t *)(pg + y.o_ncoal))[pop]);
  for (int b = 0; b < y.B; b++)
    fprintf(f, " %a %d", ((const double *)(pg + y.o_migst))[b], ((const int16_t *)(pg + y.o_nmig))[b]);
  fprintf(f, "\n");
  fprintf(f, "M %d", is[IS_NUM_MIGS]);
  for (int i = 0; i < is[IS_NUM_MIGS]; i++) {
    int mg = ((const int16_t *)(pg + y.o_living))[i];
    const int16_t *mi = (const int16_t *)(pg + y.o_mig_i) + mg * MG_COUNT;
    fprintf(f, " %d:%d:%d:%d:%d:%d:%d:%a", mg, mi[MG_BRANCH], mi[MG_BAND], mi[MG_SPOP], mi[MG_TPOP], mi[MG_SEV],
            mi[MG_TEV], ((const double *)(pg + y.o_mig_age))[mg]);
  }
  fprintf(f, "\n");
  if (cb) {
    for (int i = y.n; i < y.N; i++) {
      const double *c = (const double *)(cb + ((size_t)((int)(((uint32_t)is[IS_CBIT0 + (i >> 5)] >> (i & 31)) & 1) * (y.n - 1) + (i - y.n)) * P) * 32);
      fprintf(f, "K %d", i);
      for (int k = 0; k < 4 * P; k++) fprintf(f, " %a", c[k]);
      fprintf(f, "\n");
    }
  }
}

// after a host synchronisation: the error the stages recorded, the counters
static int check_error(gph_engine *e)
{
  const int code = e->G_h->error;
  if (code != 0) {
    const long long gl = e->G_h->error_locus;      /* -1: not a per-locus error (every gg_* path that raises one says so) */
    e->last_error_code = code;
    e->last_error_locus = gl;
    if (code == 75) fprintf(stderr, "gphocs_hip: synchronizeEvents found an inconsistency (Fatal Error 0075/0076)\n");
    else if (code == 9999) fprintf(stderr, "gphocs_hip: checkAll failed at iteration %d\n", e->G_h->iteration);
    else if (gl >= 0) fprintf(stderr, "gphocs_hip: Fatal Error %04d reported by a locus kernel, first in locus %lld (iteration %d)\n", code, gl, e->G_h->iteration);
    else fprintf(stderr, "gphocs_hip: Fatal Error %04d reported by a locus kernel\n", code);
    /* what printGenealogyAndExit prints upstream (GPhoCS.c:660-676: the locus's genealogy and its event chains), in the
     * canonical dump format, when the failing locus is one of this rank's; the state is the one the kernel left behind */
    const long long lo = gl - e->cfg.locus_begin;
    if (gl >= 0 && lo >= 0 && lo < e->L && !e->in_error_dump) {
      e->in_error_dump = true;
      int64_t slot = -1;
      for (int64_t j = 0; j < e->L; j++) if (e->h_orig[j] == lo) { slot = j; break; }
      std::vector<char> pg(e->lay.page_bytes);
      if (slot >= 0 && !d2h(e, pg.data(), (const char *)e->dev.pages + (size_t)slot * e->lay.page_bytes, e->lay.page_bytes)) {
        fprintf(stderr, "gphocs_hip: genealogy and event chains of locus %lld:\n", gl);
        dump_one_locus(e, stderr, gl, pg.data(), nullptr, 0);
      }
      e->in_error_dump = false;
    }
    return GPH_EKERNEL;
  }
  return 0;
}
// the mirror is current (host mode: always; resident mode: after pull_G)
static int finish_sync(gph_engine *e)
{
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  if (resident(e)) { int rc = pull_G(e); if (rc) return rc; }
  return check_error(e);
}

static int run_stage_now(gph_engine *e, int stage, int arg);
// the commit of a decided mixing proposal that was left for the next sweep kernel: as a kernel of its own, now (something
// other than the sweep is about to read or write the pages)
static int mix_finish_owed(gph_engine *e)
{
  if (!e->mix_owed) return 0;
  e->mix_owed = false;
  return launch_loci(e, 7, k_mix_finish, 0);
}
// run a deferred synchronizeEvents pass now (anything but the next genealogy sweep is about to touch the pages).
// now = the caller is a stepwise entry point that goes on to edit the host mirror of the chain state and push it: the
// stage that checks the pass (Fatal Error 0075/0076, the class-8 counters) must then have run -- on the host, result
// checked -- before that, or the push would overwrite what a queued device-side stage wrote
static int flush_sync(gph_engine *e, bool now)
{
  int rc;
  if ((rc = mix_finish_owed(e))) return rc;     /* a mixing commit left for the next sweep kernel goes first */
  if (!e->sync_pending) return 0;
  e->sync_pending = false;
  if ((rc = push_if_dirty(e))) return rc;
  if ((rc = launch_loci(e, 8, k_sync, 0))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if (now) return run_stage_now(e, GS_REFRESH_DONE, 0);
  return run_stage(e, GS_REFRESH_DONE, 0, e->G_h->iteration);
}

// a stage whose result the CALLER needs now (the stepwise entry points of the C ABI): host path whatever the mode
static int run_stage_now(gph_engine *e, int stage, int arg)
{
  const bool fh = e->force_host;
  e->force_host = true;
  int rc = run_stage(e, stage, arg, e->G_h->iteration);
  e->force_host = fh;
  if (rc) return rc;
  return check_error(e);
}

// the buffers of k_rng_ahead, by slot.  Not getting them is not an error: the sweep then generates its draws itself (and a
// data set at the edge of the device's memory still loads)
static int rng_ahead_alloc(gph_engine *e)
{
  const size_t L = (size_t)e->L, nck = (size_t)(e->ra_M / e->ra_C) + 1;
  const size_t b_draws = sizeof(double) * L * e->ra_M, b_ckpt = 16 * nck * L, b_tail = 16 * L, b_kprev = sizeof(int32_t) * L;
  GphDev &d = e->dev;
  /* GPH_RNG_AHEAD_FAIL_ALLOC=1 (tests): as if the last of them had not been had */
  const bool forced = getenv("GPH_RNG_AHEAD_FAIL_ALLOC") && atoi(getenv("GPH_RNG_AHEAD_FAIL_ALLOC")) != 0;
  if (dev_alloc((void **)&d.ra_draws, b_draws) || dev_alloc((void **)&d.ra_ckpt, b_ckpt) || dev_alloc((void **)&d.ra_tail, b_tail) ||
      forced || dev_alloc((void **)&d.ra_kprev, b_kprev)) {
    dev_clear_error();
    fprintf(stderr, "gphocs_hip: no memory for %d draws ahead of the sweep per locus (%.1f MB): the sweep kernel generates its own\n",
            e->ra_M, (double)(b_draws + b_ckpt + b_tail + b_kprev) / 1e6);
    dev_free(d.ra_draws); dev_free(d.ra_ckpt); dev_free(d.ra_tail); dev_free(d.ra_kprev);
    d.ra_draws = nullptr; d.ra_ckpt = nullptr; d.ra_tail = nullptr; d.ra_kprev = nullptr;
    e->rng_ahead = false;
    return 0;
  }
  /* n_ahead of a locus's first sweep = ra_first rounded up to 64 (rng_ahead_count) */
  std::vector<int32_t> kp(L, ((e->ra_first + 63) & ~63) - 64);
  if (h2d(e, d.ra_kprev, kp.data(), b_kprev)) return GPH_EHIP;
  d.ra_M = e->ra_M;
  d.ra_cshift = e->ra_C == 64 ? 6 : 4;
  e->ra_bytes = b_draws + b_ckpt + b_tail + b_kprev;
  return 0;
}

// the engines this library has made and not yet destroyed: a call that takes several engines (gph_engine_clades_compare) is
// handed pointers it cannot look into before it knows they are its own -- every capacity variant has its own gph_engine
static std::mutex g_engines_lock;
static std::set<const gph_engine *> g_engines;
static bool engine_is_ours(const gph_engine *e)
{
  std::lock_guard<std::mutex> hold(g_engines_lock);
  return g_engines.count(e) != 0;
}

// ---------------------------------------------------------------- C ABI
extern "C" {
static void rng_ahead_dirty(gph_engine *e);

int gph_engine_create(const gph_config *cfg, gph_engine **out)
{
  if (!cfg || !out) return GPH_EARG;
  if (cfg->n > 200 || cfg->K > 39 || cfg->B > 100)
    fprintf(stderr, "gphocs_hip: n=%d K=%d B=%d exceed even the reference's compile-time caps (NS 200, 2*NSPECIES-1 = 39, MAX_MIG_BANDS 100: upstream src/patch.h:17-22)\n", cfg->n, cfg->K, cfg->B);
  if (cfg->n < 2 || cfg->n > GPH_CAP_LEAVES || cfg->K > GPH_CAP_K || cfg->B > GPH_CAP_B || cfg->K != 2 * cfg->Kc - 1) {
    fprintf(stderr, "gphocs_hip: unsupported dimensions n=%d K=%d B=%d (this library variant: n<=%d leaves, K<=%d populations, B<=%d bands; the largest variant covers the reference's own caps 200 / 39 / 100, upstream src/patch.h:17-22)\n",
            cfg->n, cfg->K, cfg->B, GPH_CAP_LEAVES, GPH_CAP_K, GPH_CAP_B);
    return GPH_EARG;
  }
  gph_engine *e = new gph_engine();
  e->cfg = *cfg;
  e->samplesPerPop.assign(cfg->samplesPerPop, cfg->samplesPerPop + cfg->Kc);
  e->popFather.assign(cfg->popFather, cfg->popFather + cfg->K);
  e->popSon0.assign(cfg->popSon0, cfg->popSon0 + cfg->K);
  e->popSon1.assign(cfg->popSon1, cfg->popSon1 + cfg->K);
  if (cfg->B > 0) { e->bandSrc.assign(cfg->bandSrc, cfg->bandSrc + cfg->B); e->bandTgt.assign(cfg->bandTgt, cfg->bandTgt + cfg->B); }
  e->cfg.samplesPerPop = e->samplesPerPop.data();
  e->cfg.popFather = e->popFather.data();
  e->cfg.popSon0 = e->popSon0.data();
  e->cfg.popSon1 = e->popSon1.data();
  e->cfg.bandSrc = e->bandSrc.data();
  e->cfg.bandTgt = e->bandTgt.data();
  memset(&e->dev, 0, sizeof e->dev);
  memset(&e->ka, 0, sizeof e->ka);
  fill_math_constants(e->ka);
  if (const char *fh = getenv("GPH_HOST_DECISIONS")) e->force_host = atoi(fh) != 0;
  if (const char *nf = getenv("GPH_NO_FUSE")) e->no_fuse = atoi(nf) != 0;
  if (const char *ra = getenv("GPH_RNG_AHEAD")) e->rng_ahead = atoi(ra) != 0;
  if (const char *ra = getenv("GPH_RNG_AHEAD_DRAWS")) e->ra_M = atoi(ra);
  if (const char *ra = getenv("GPH_RNG_AHEAD_PLACE")) e->ra_place_b = ra[0] == 'B' || ra[0] == 'b';
  if (const char *ra = getenv("GPH_RNG_AHEAD_CKPT")) e->ra_C = atoi(ra);
  if (const char *ra = getenv("GPH_RNG_AHEAD_FIRST")) e->ra_first = atoi(ra);
  if (e->rng_ahead && (e->ra_M < 64 || e->ra_M % 64 != 0 || e->ra_M > (1 << 20) || (e->ra_C != 16 && e->ra_C != 64) || e->ra_first < 0)) {
    fprintf(stderr, "gphocs_hip: GPH_RNG_AHEAD_DRAWS must be a multiple of 64 (up to 2^20), GPH_RNG_AHEAD_CKPT 16 or 64, GPH_RNG_AHEAD_FIRST >= 0\n");
    delete e;
    return GPH_EARG;
  }
  if (int rc = backend_open(e)) { gph_engine_destroy(e); return rc; }
  memset(e->G_h, 0, sizeof(GphGlobal));
  e->G_h->error_locus = -1;          /* (0 is a locus: an error that is not per-locus must not name it -- ADVICE round 5) */
  e->G_h->beta = 1.0;                /* the posterior itself */
  build_model_static(e);
  { std::lock_guard<std::mutex> hold(g_engines_lock); g_engines.insert(e); }
  *out = e;
  return 0;
}

void gph_engine_destroy(gph_engine *e)
{
  if (!e) return;
  { std::lock_guard<std::mutex> hold(g_engines_lock); g_engines.erase(e); }
  rng_ahead_drain(e);
  dev_free(e->dev.pages); dev_free(e->dev.shadow); dev_free(e->dev.cond); dev_free((void *)e->dev.cond_off);
  dev_free((void *)e->dev.seq); dev_free((void *)e->dev.seq_off); dev_free((void *)e->dev.orig); dev_free((void *)e->dev.P); dev_free(e->dev.out); dev_free(e->dev.stats); dev_free(e->d_mutRate);
  dev_free(e->d_lrec); dev_free(e->d_lpre); dev_free(e->d_slot_of); dev_free(e->d_lr_result); dev_free(e->d_lr_gscr); dev_free(e->d_ref_page); dev_free(e->d_ref_seq);
  dev_free(e->d_part); dev_free(e->dev.err);
  dev_free(e->dev.ra_draws); dev_free(e->dev.ra_ckpt); dev_free(e->dev.ra_tail); dev_free(e->dev.ra_kprev);
  dev_free(e->ls.d); dev_free(e->cs.part.d_part); dev_free(e->cs.rows.d); dev_free(e->ts.part.d_part); dev_free(e->ts.rows.d);
  dev_free(e->an.d_acc); dev_free(e->an.rows.d);
  dev_free(e->gt.rows.d); dev_free(e->gt.sel.d_slot);
  dev_free(e->cl.d_hdr); dev_free(e->cl.d_cmp); dev_free(e->mu.part.d_part); dev_free(e->sf.part.d_part);
  for (SmSelected *s : e->selected()) { dev_free(s->d); dev_free(s->sel.d_slot); dev_free(s->rows.d); }
  dev_free((void *)e->dev.slog_map); dev_free(e->dev.slog); dev_free(e->dev.slog_n);
  if (e->d_gather != e->d_red) dev_free(e->d_gather);
  dev_free(e->d_red);
  backend_close(e);
  delete e;
}

int gph_engine_set_allreduce(gph_engine *e, gph_allreduce_fn fn, void *user)
{
  if (!e) return GPH_EARG;
  e->allreduce = fn;
  e->allreduce_user = user;
  return 0;
}

// native communicator (gph_comm.h): RCCL over xGMI, one rank per GPU, all-gathers queued on the engine's stream; or the
// host shared-memory exchange for ranks that share a GPU.  The engine does not own it.
int gph_engine_set_comm(gph_engine *e, gph_comm *c)
{
  if (!e) return GPH_EARG;
  SETDEV(e);
  e->comm = c;
  if (e->d_gather != e->d_red) { dev_free(e->d_gather); e->d_gather = e->d_red; }
  if (c && gph_comm_world(c) > 1 && gph_comm_on_stream(c)) {
    if (gph_comm_world(c) > 64) return GPH_EARG;
    if (dev_alloc((void **)&e->d_gather, sizeof(double) * GPH_RED_ROW * gph_comm_world(c))) return GPH_EHIP;
  }
  return 0;
}

GphGlobal *gph_engine_global_(gph_engine *e) { if (!e) return nullptr; e->G_dirty = true; return e->G_h; }
const GphGlobal *gph_engine_global_ro_(gph_engine *e) { return e ? e->G_h : nullptr; }

// power posterior (include/gphocs_hip.h): from the next proposal on, the data term of every acceptance ratio is beta * its change
int gph_engine_set_beta(gph_engine *e, double beta)
{
  if (!e || !(beta >= 0.0 && beta <= 64.0)) return GPH_EARG;    /* (a NaN fails both comparisons) */
  if (e->G_h->beta != beta) { e->G_h->beta = beta; e->G_dirty = true; }
  return 0;
}
int gph_engine_get_beta(gph_engine *e, double *beta)
{
  if (!e || !beta) return GPH_EARG;
  *beta = e->G_h->beta;
  return 0;
}

// What gph_engine_load_loci accepts (include/gphocs_hip.h says it to the caller).  The first violation is refused with GPH_EARG and
// a line on stderr that names the locus (global index) and the pattern (row of the locus); gph_engine_last_error then returns that
// locus with one of the GPH_LOAD_* codes, gph_engine_last_error_text the line.  The sizes of ALL loci are judged first, from
// the offsets alone: a caller whose offsets are wrong is told so before a row is read.
static int refuse_loci(gph_engine *e, int64_t g, int32_t code, const char *fmt, ...)
{
  char what[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(what, sizeof what, fmt, ap);
  va_end(ap);
  e->last_error_locus = (long long)e->cfg.locus_begin + g;
  e->last_error_code = code;
  snprintf(e->last_error_text, sizeof e->last_error_text, "gphocs_hip: gph_engine_load_loci: locus %lld: %s", e->last_error_locus, what);
  fprintf(stderr, "%s\n", e->last_error_text);
  return GPH_EARG;
}

static int check_loci(gph_engine *e, int64_t L, const int64_t *poff, const uint8_t *leafcodes, const uint16_t *numPhases, const int32_t *counts)
{
  const int n = e->cfg.n;
  const int64_t lim = (int64_t)1 << 31;
  /* the device code indexes a locus's conditionals ((half * (n - 1) + node - n) * P + p) * 4 + base and its sequence block with
   * 32-bit integers */
  for (int64_t g = 0; g < L; g++) {
    const int64_t P = poff[g + 1] - poff[g];
    if (P < 0) return refuse_loci(e, g, GPH_LOAD_SIZE, "pattern_offsets decrease (%lld patterns)", (long long)P);
    if (P >= lim || (int64_t)8 * (n - 1) * P >= lim || (int64_t)GPH_Q_BYTES(P, (int64_t)n, 1) >= lim)     /* (the block with 16-bit counts: the smaller form; load_loci judges the other once it knows the form) */
      return refuse_loci(e, g, GPH_LOAD_SIZE, "%lld phased patterns at %d leaves: 8 (n - 1) P or the sequence block reaches 2^31", (long long)P, n);
  }
  for (int64_t g = 0; g < L; g++) {
    const int64_t P = poff[g + 1] - poff[g], r0 = poff[g];
    for (int64_t p = 0; p < P; ) {
      const int w = numPhases[r0 + p];
      if (w == 0) return refuse_loci(e, g, GPH_LOAD_NO_GROUP, "pattern %lld: phase word 0 on a row that belongs to no group of phases", (long long)p);
      if (w >= GPH_PHASES_ENCODE_MIN && ((w & 0x7fff) < 15 || (w & 0x7fff) > 24))
        return refuse_loci(e, g, GPH_LOAD_WORD, "pattern %lld: phase word 0x%04x is no count (0x8000 | exponent takes exponents 15 .. 24)", (long long)p, w);
      const int64_t k = GPH_PHASES(w);
      if (k > P - p) return refuse_loci(e, g, GPH_LOAD_OVERRUN, "pattern %lld: %lld phases run past the locus's last row (%lld patterns)", (long long)p, (long long)k, (long long)P);
      if (counts[r0 + p] < 0) return refuse_loci(e, g, GPH_LOAD_COUNT, "pattern %lld: negative count %d", (long long)p, (int)counts[r0 + p]);
      for (int64_t q = p + 1; q < p + k; q++)
        if (numPhases[r0 + q] != 0 || counts[r0 + q] != 0)
          return refuse_loci(e, g, GPH_LOAD_INSIDE, "pattern %lld: phase word 0x%04x and count %d inside the %lld phases of pattern %lld (both are 0 there)",
                             (long long)q, (int)numPhases[r0 + q], (int)counts[r0 + q], (long long)k, (long long)p);
      p += k;
    }
    for (int64_t p = 0; p < P; p++)
      for (int i = 0; i < n; i++)
        if (leafcodes[(size_t)(r0 + p) * n + i] > 4)
          return refuse_loci(e, g, GPH_LOAD_LEAF, "pattern %lld: leaf code %d of sample %d (0 .. 3 = T C A G, 4 = N)", (long long)p, (int)leafcodes[(size_t)(r0 + p) * n + i], i);
  }
  return 0;
}

int gph_engine_load_loci(gph_engine *e, int64_t L, const int64_t *poff, const uint8_t *leafcodes,
                         const uint16_t *numPhases, const int32_t *counts, const double *mutRates)
{
  if (!e || L <= 0 || !poff || !leafcodes || !numPhases || !counts) return GPH_EARG;
  if (e->loaded) { fprintf(stderr, "gphocs_hip: gph_engine_load_loci called twice on one engine\n"); return GPH_ESTATE; }
  { int rcv = check_loci(e, L, poff, leafcodes, numPhases, counts); if (rcv) return rcv; }      /* before anything is allocated */
  SETDEV(e);
  const int n = e->cfg.n;
  int Pmax = 1;
  for (int64_t g = 0; g < L; g++) { int P = (int)(poff[g + 1] - poff[g]); if (P > Pmax) Pmax = P; }   /* P == 0: a locus with no informative column (all N) is legal upstream */
  /* pattern counts as 16-bit words when every count of the data set allows it (a count is at most the length of its
   * locus): 2 bytes per pattern of every resident sequence block */
  int cnt16 = 1;
  for (int64_t i = 0; i < poff[L]; i++) if (counts[i] < 0 || counts[i] > 65535) { cnt16 = 0; break; }
  if (const char *ov = getenv("GPH_CNT16")) cnt16 = cnt16 && atoi(ov) != 0;     /* tests: the 32-bit form */
  if (!cnt16)       /* (check_loci judged the block with 16-bit counts; with 32-bit counts it is the larger limit only where n == 1) */
    for (int64_t g = 0; g < L; g++)
      if ((int64_t)GPH_Q_BYTES(poff[g + 1] - poff[g], (int64_t)n, 0) >= ((int64_t)1 << 31))
        return refuse_loci(e, g, GPH_LOAD_SIZE, "%lld phased patterns at %d leaves: the sequence block reaches 2^31", (long long)(poff[g + 1] - poff[g]), n);
  build_layout(e->lay, n, e->cfg.Kc, e->cfg.K, e->cfg.B, e->cfg.rootPop, Pmax, cnt16);
  /* A locus whose sequence block does not fit the LDS budget of a launch group keeps it in HBM ("huge": its own launch
   * group, the generic (pattern, base) paths read the block through GphSeq -- gph_rt.h; the reference mallocs any P,
   * LocusDataLikelihood.c:251).  The budget is what ONE pattern-rich locus may cost every other one in resident
   * wavefronts: the whole group is launched with the LDS of its largest block (default 32 KB = 5 wavefronts per CU, or
   * the image + 16 KB for the big-tree builds;
   * GPH_HUGE_LDS=bytes -- tests force the HBM path on small loci with it). */
  {
    int budget = 32 * 1024;
    if (budget < (int)sizeof(GphLds) + 16 * 1024) budget = (int)sizeof(GphLds) + 16 * 1024;     /* (the big-tree builds' images alone are 9 - 44 KB) */
    if (const char *ov = getenv("GPH_HUGE_LDS")) {
      budget = atoi(ov);
      if (budget <= 0) { fprintf(stderr, "gphocs_hip: GPH_HUGE_LDS=%s is not a byte count\n", ov); return GPH_EARG; }
    }
    /* the budget covers image + block: what a workgroup can have at all is the CU's 160 KB */
    if (budget > 160 * 1024) budget = 160 * 1024;
    int hp = GPH_WAVE;     /* (a block of up to GPH_WAVE patterns always fits: the lane-per-pattern paths read LDS directly) */
    while (hp < Pmax && (int)sizeof(GphLds) + GPH_Q_BYTES(hp + 1, n, cnt16) <= budget) hp++;
    e->lay.huge_P = hp >= Pmax ? 0x7fffffff : hp;
  }
  e->L = L;
  // slots in decreasing P (stable): within a dispatch the longest wavefronts start first; loci with more
  // than one pattern per lane (P > 64) form their own launch group
  e->h_orig.resize(L);
  for (int64_t g = 0; g < L; g++) e->h_orig[g] = (int32_t)g;
  std::stable_sort(e->h_orig.begin(), e->h_orig.end(), [&](int32_t a, int32_t b) {
    return (poff[a + 1] - poff[a]) > (poff[b + 1] - poff[b]); });
  e->buckets.clear();
  {
    int64_t nwide = 0, nhuge = 0;
    while (nhuge < L && (poff[e->h_orig[nhuge] + 1] - poff[e->h_orig[nhuge]]) > e->lay.huge_P) nhuge++;
    nwide = nhuge;
    while (nwide < L && (poff[e->h_orig[nwide] + 1] - poff[e->h_orig[nwide]]) > GPH_WAVE) nwide++;
    e->n_huge = nhuge;
    if (nhuge > 0 && e->cfg.locus_begin == 0)
      fprintf(stderr, "gphocs_hip: %lld loci with more than %d phased patterns (up to %d) keep their sequence block in HBM\n",
              (long long)nhuge, e->lay.huge_P, Pmax);
    if (nhuge > 0) {        /* sequence block in HBM: no dynamic LDS beyond a token allocation */
      gph_engine::Bucket bk;
      bk.j0 = 0; bk.count = (int)nhuge;
      bk.lds_bytes = 64;
      e->buckets.push_back(bk);
    }
    if (nwide > nhuge) {    /* the generic (pattern, base) mapping, block in LDS (the root sum needs no terms array on the device) */
      const int pw = (int)(poff[e->h_orig[nhuge] + 1] - poff[e->h_orig[nhuge]]);
      gph_engine::Bucket bk;
      bk.j0 = (int)nhuge; bk.count = (int)(nwide - nhuge);
      bk.lds_bytes = GPH_Q_TERMS(pw, n, cnt16) + wide_terms_bytes(pw);
      e->buckets.push_back(bk);
    }
    if (nwide < L) {
      const int pn = (int)(poff[e->h_orig[nwide] + 1] - poff[e->h_orig[nwide]]);
      gph_engine::Bucket bk;
      bk.j0 = (int)nwide; bk.count = (int)(L - nwide);
      bk.lds_bytes = GPH_Q_BYTES(pn, n, cnt16);
      /* the per-lane terms of the root reduction through LDS (ordered_sum64_lds: one vector instruction per pattern
       * instead of three) take 8 bytes per pattern behind a locus's block: never at the price of a resident workgroup.
       * LDS is handed out in 1280-byte granules (160 KB / 128, measured: profiles/HISTORY.md, round 1) and the sweep kernel keeps
       * at most GPH_SWEEP_WAVES workgroups per SIMD: the group gets the room of the granules its largest block needs
       * anyway, or -- when even the largest locus's terms do not cost a workgroup -- room for everybody's; a locus takes
       * the LDS form when its terms end inside the allocation (gph_locus.h: lik_compute) */
      {
        auto resident = [](int bytes) { const int g = (bytes + 1279) / 1280; const int w = 128 / g; return w < 4 * GPH_SWEEP_WAVES_ ? w : 4 * GPH_SWEEP_WAVES_; };
        const int base = (int)sizeof(GphLds) + bk.lds_bytes;
        const int full = 8 * ((pn + 7) & ~7);
        e->lay.lds_sum = 1;
        if (resident(base + full) == resident(base)) bk.lds_bytes += full;
        else {
          /* the largest size with as many resident workgroups as the bare block: granules first, then the step of the
           * wavefront cap (4 * GPH_SWEEP_WAVES workgroups per CU do not need whole granules to themselves) */
          int room = (base + 1279) / 1280 * 1280;
          while (resident(room + 1280) == resident(base)) room += 1280;
          bk.lds_bytes = (room - (int)sizeof(GphLds)) & ~15;
        }
        if (const char *ov = getenv("GPH_LDS_SUM")) {     /* tests: force either form for every locus */
          e->lay.lds_sum = atoi(ov) != 0;
          bk.lds_bytes = GPH_Q_BYTES(pn, n, cnt16) + (e->lay.lds_sum ? full : 0);
        }
      }
      e->buckets.push_back(bk);
    }
  }
  /* (a group that was given the rest of its granules for the root sum's terms can be larger than block + 512 bytes) */
  e->lay.lds_bytes = 0;
  for (auto &bk : e->buckets) if (bk.lds_bytes > e->lay.lds_bytes) e->lay.lds_bytes = bk.lds_bytes;
  e->h_cond_off.resize(L + 1);
  e->h_P.resize(L);
  std::vector<uint64_t> seq_off(L + 1);
  std::vector<double> rates(L, 1.0);
  uint64_t off = 0, soff = 0;
  for (int64_t j = 0; j < L; j++) {
    int64_t g = e->h_orig[j];
    int P = (int)(poff[g + 1] - poff[g]);
    e->h_P[j] = P;
    e->h_cond_off[j] = off;
    off += (uint64_t)2 * (n - 1) * P * 32;
    seq_off[j] = soff;
    soff += GPH_Q_BYTES(P, n, cnt16);
    if (P > e->lay.huge_P) soff += (uint64_t)8 * ((P + 1) & ~1);     /* the root reduction's terms of the host build behind a block that lies in HBM */
    if (mutRates) rates[j] = mutRates[g];
  }
  e->h_cond_off[L] = off;
  seq_off[L] = soff;
  e->h_seq_off = seq_off;
  e->h_sites.assign(L, 0);
  for (int64_t g = 0; g < L; g++)
    for (int64_t p = poff[g]; p < poff[g + 1]; p++) if (numPhases[p] != 0) e->h_sites[g] += counts[p];
  std::vector<char> seq(soff, 0);
  for (int64_t j = 0; j < L; j++) {
    int64_t g = e->h_orig[j];
    int P = e->h_P[j];
    char *blk = seq.data() + seq_off[j];
    for (int p = 0; p < P; p++) {
      for (int i = 0; i < n; i++) {
        uint8_t c = leafcodes[(size_t)(poff[g] + p) * n + i];
        blk[GPH_Q_LEAF + p * GPH_Q_NH(n) + (i >> 1)] |= (char)(c << ((i & 1) << 2));
      }
      ((uint16_t *)(blk + GPH_Q_PHASES(P, n)))[p] = numPhases[poff[g] + p];
      if (cnt16) ((uint16_t *)(blk + GPH_Q_COUNT(P, n)))[p] = (uint16_t)counts[poff[g] + p];
      else ((int32_t *)(blk + GPH_Q_COUNT(P, n)))[p] = counts[poff[g] + p];
    }
  }
  e->cond_bytes = off;
  e->seq_bytes_total = soff;
  e->pages_bytes = (size_t)L * e->lay.page_bytes;
  int rc = 0;
  rc |= dev_alloc((void **)&e->dev.pages, e->pages_bytes);
  rc |= dev_alloc((void **)&e->dev.shadow, e->pages_bytes);
  rc |= dev_alloc((void **)&e->dev.cond, e->cond_bytes);
  rc |= dev_alloc((void **)&e->dev.cond_off, sizeof(uint64_t) * (L + 1));
  rc |= dev_alloc((void **)&e->dev.seq, seq.size());
  rc |= dev_alloc((void **)&e->dev.seq_off, sizeof(uint64_t) * (L + 1));
  rc |= dev_alloc((void **)&e->dev.P, sizeof(int32_t) * 2 * L);
  rc |= dev_alloc((void **)&e->dev.orig, sizeof(int32_t) * L);
  rc |= dev_alloc((void **)&e->dev.out, sizeof(double) * GPH_OUT_SLOTS * L);
  rc |= dev_alloc((void **)&e->dev.stats, sizeof(double) * (2 * e->cfg.K + 2 * e->cfg.B) * L);
  rc |= dev_alloc((void **)&e->d_part, sizeof(double) * 2 * 3 * GPH_RED_BLOCKS * GPH_RED_COLS);
  rc |= dev_alloc((void **)&e->dev.err, sizeof(int32_t));
  if (!rc) rc = zero_error_word(e);
  if (mutRates) rc |= dev_alloc((void **)&e->d_mutRate, sizeof(double) * L);
  if (rc) { fprintf(stderr, "gphocs_hip: device allocation failed\n"); return GPH_EHIP; }
  rc |= h2d(e, (void *)e->dev.cond_off, e->h_cond_off.data(), sizeof(uint64_t) * (L + 1));
  rc |= h2d(e, (void *)e->dev.seq, seq.data(), seq.size());
  rc |= h2d(e, (void *)e->dev.seq_off, seq_off.data(), sizeof(uint64_t) * (L + 1));
  {
    std::vector<int32_t> pu((size_t)2 * L);      /* {phased, unphased} patterns per slot */
    for (int64_t j = 0; j < L; j++) {
      const int64_t g = e->h_orig[j];
      int U = 0;
      for (int64_t p = poff[g]; p < poff[g + 1]; p++) U += numPhases[p] > 0;
      pu[2 * j] = e->h_P[j]; pu[2 * j + 1] = U;
    }
    rc |= h2d(e, (void *)e->dev.P, pu.data(), sizeof(int32_t) * 2 * L);
  }
  rc |= h2d(e, (void *)e->dev.orig, e->h_orig.data(), sizeof(int32_t) * L);
  if (mutRates) rc |= h2d(e, e->d_mutRate, rates.data(), sizeof(double) * L);
  if (rc) return GPH_EHIP;
  e->dev.L = (int32_t)L;
  if (e->rng_ahead && rng_ahead_alloc(e)) return GPH_EHIP;
  e->dev.Ltot = (int32_t)e->cfg.L_total;
  e->dev.locus_begin = e->cfg.locus_begin;
  e->loaded = true;
  return loci_loaded(e);
}

int gph_engine_set_model(gph_engine *e, const double *theta, const double *popAge, const double *sampleAge,
                         const double *migRate, const double *bandStart, const double *bandEnd)
{
  if (!e || !theta || !popAge || !sampleAge) return GPH_EARG;
  GphModel &m = e->G_h->model;
  for (int p = 0; p < e->cfg.K; p++) { gg_set_theta(*e->G_h, p, theta[p]); m.popAge[p] = popAge[p]; m.sampleAge[p] = sampleAge[p]; }
  for (int b = 0; b < e->cfg.B; b++) { gg_set_mig(*e->G_h, b, migRate[b]); m.bandStart[b] = bandStart[b]; m.bandEnd[b] = bandEnd[b]; }
  e->model_set = true;
  e->G_dirty = true;
  return 0;
}

int gph_engine_seed(gph_engine *e, uint32_t seed)
{
  if (!e) return GPH_EARG;
  e->seedz = 170u * (seed % 178u) + 137u;   // utils.c:421
  e->seeded = true;
  return 0;
}

int gph_engine_init_genealogies(gph_engine *e, double *sumGen, double *sumData)
{
  if (!e || !e->loaded || !e->seeded || !e->model_set) return GPH_ESTATE;
  SETDEV(e);
  /* the pages are rewritten from scratch: nothing decided on the old chain is owed to them any more (a commit left for the
   * next sweep kernel would stage in the OLD chain's shadow page over the fresh genealogies) */
  rng_ahead_dirty(e);
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  e->mix_owed = e->fin_owed = e->sync_pending = false;
  if (e->G_h->mix_flag || e->G_h->tau_flag) { e->G_h->mix_flag = 0; e->G_h->tau_flag = 0; e->G_dirty = true; }
  { int rcp = push_if_dirty(e); if (rcp) return rcp; }
  /* summaries of the old chain do not carry over; the locus-rate columns come and go with `locus-mut-rate VAR` */
  if (e->ls.d && e->ls.ncol != gph_ls_columns(e->cfg.K, e->cfg.B, e->var_rates)) { int rce = gph_engine_locus_summary_enable(e, 1); if (rce) return rce; }
  e->ls.samples = e->an.samples = e->cl.samples = 0;
  e->cs.rows.fill = e->ts.rows.fill = e->an.rows.fill = e->gt.rows.fill = 0;
  e->an.iters.clear();
  e->gt.iters.clear();
  { int rcz = acc_zero(e, e->ls.d, sizeof(double) * (size_t)e->ls.ncol * e->L); if (rcz) return rcz; }
  { int rcz = acc_zero(e, e->an.d_acc, sizeof(double) * (size_t)e->an.ncol * e->L); if (rcz) return rcz; }
  for (SmSelected *s : e->selected()) {
    if (s == &e->es && e->es.on && e->es.M != (e->var_rates ? 6 : 5)) {       /* the rate series comes and goes with `locus-mut-rate VAR` */
      std::vector<int64_t> sel = e->es.sel.loci;
      sel.push_back(0);                                         /* (a non-null pointer for an empty selection too) */
      int rce = gph_engine_ess_enable(e, sel.data(), (int64_t)sel.size() - 1, e->es.max_bytes);
      if (rce) return rce;
    }
    s->rows.fill = 0;
    s->iters.clear();
    if (s->on) { s->samples = 0; int rcz = s->zero(e); if (rcz) return rcz; }
  }
  int rc = launch_loci(e, 3, k_init, e->seedz, e->d_mutRate, e->init_predraws);
  if (!rc) rc = reduce_local(e, 0, GPH_OUT_SLOTS);
  if (!rc) rc = reduce_stats(e);
  if (rc) return rc;
  e->G_h->nrec = 0;
  e->G_h->iteration = -1;
  if ((rc = run_stage_now(e, GS_INIT_DONE, 0))) return rc;
  { GphRed R; R.rows = e->h_red; R.world = 1;
    if (sumGen) *sumGen = R.sum(0, 0);
    if (sumData) *sumData = R.sum(0, 1); }
  e->initialized = true;
  return rc;
}

// the draws of every slot's next sweep (k_rng_ahead), on the engine's stream right in front of the sweep kernel -- ahead of
// the fork of its launch groups, so every group finds its draws -- from the generator states the pages hold now
// a pass that is still in flight on its own stream and whose draws will not be used must be over before the next one writes
// the same buffers
static void rng_ahead_drain_if(gph_engine *e, bool stale) { if (stale && e->ra_b_valid) rng_ahead_drain(e); }
// something other than the chained sweep is about to step the loci's generators: a pass made behind the last sweep (it may
// still be running) is void
static void rng_ahead_dirty(gph_engine *e) { rng_ahead_drain_if(e, true); e->ra_b_valid = false; }
static int rng_ahead_launch(gph_engine *e)
{
  if (e->dev.ra_M <= 0) return 0;
  int rc;
  if ((rc = flush_pending(e))) return rc;
  launch_pre(e);
  const int tms = tm_begin(e, 18);
  if ((rc = launch_grid(e, GphGrid{(int)((e->L + GPH_WAVE - 1) / GPH_WAVE), 1}, GPH_WAVE, 0, k_rng_ahead, e->ka, e->dev))) return rc;
  tm_end(e, tms);
  e->cls_launches[18] += 1; e->n_launches++;
  return 0;
}

// The three genealogy proposals fused in one launch (GPhoCS.c:1495-1538; flags: which of them) and the reductions of its
// outputs.  Two things decided earlier ride at the kernel's head: the deferred synchronizeEvents of the finished iteration
// (flag 8; with_sync tells the stage that follows) and the commit of an accepted mixing proposal (flag 16) -- its flag and
// factor travel as kernel arguments off the host mirror, which must then be what the decision stage wrote
static int sweep_launch(gph_engine *e, int flags, double ftCoal, double ftMig, int &with_sync, bool chained = false)
{
  int rc;
  /* chained: the sweep of gph_engine_iteration_.  The draws the pass made behind the previous iteration's sweep are this
   * sweep's unless something stepped a generator since (rng_ahead_dirty) */
  const bool side = chained && e->ra_place_b && e->dev.ra_M > 0 && resident(e);
  const bool have = side && e->ra_b_valid;
  rng_ahead_drain_if(e, !have);
  e->ra_b_valid = false;
  with_sync = e->sync_pending ? 8 : 0;
  e->sync_pending = false;
  int with_mix = 0;
  if (e->mix_owed) {
    if (!e->mirror_current && (rc = finish_sync(e))) return rc;
    e->mix_owed = false;
    if (e->G_h->mix_flag) with_mix = 16;
  }
  if (have) { if ((rc = flush_pending(e)) || (rc = rng_ahead_wait(e))) return rc; }
  else if ((rc = rng_ahead_launch(e))) return rc;
  /* beta is a setting: the mirror's value is the chain's (as the step sizes, which the callers read from it) */
  if (e->G_h->beta == 1.0) rc = launch_loci(e, 0, k_sweep, flags | with_sync | with_mix, ftCoal, ftMig, e->G_h->mix_c, e->G_h->mix_lnc);
  else rc = launch_loci(e, 0, k_sweep_heated, flags | with_sync | with_mix, ftCoal, ftMig, e->G_h->mix_c, e->G_h->mix_lnc, e->G_h->beta);
  if (rc) return rc;
  if (side) {
    launch_pre(e);
    if ((rc = rng_ahead_side(e, GphGrid{(int)((e->L + GPH_WAVE - 1) / GPH_WAVE), 1}))) return rc;
    e->cls_launches[18] += 1; e->n_launches++;
    e->ra_b_valid = true;
  }
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  return reduce_stats(e);
}

// ---- the stepwise entry points: one reference proposal function each (include/gphocs_hip.h), the result is on the
// host when the call returns.  gph_engine_iteration_() below runs the same launches without the round trips.
int gph_engine_genealogy_sweep(gph_engine *e, int32_t flags, double ftCoal, double ftMig, gph_sweep_result *out)
{
  if (!e || !e->initialized || !out) return GPH_ESTATE;
  SETDEV(e);
  int rc, with_sync;
  if ((rc = push_if_dirty(e))) return rc;
  GphGlobal &G = *e->G_h;
  const int64_t a0 = G.acc[0], a1 = G.acc[1], a2 = G.acc[2], a7 = G.acc[7];
  if ((rc = sweep_launch(e, flags, ftCoal, ftMig, with_sync))) return rc;
  if ((rc = run_stage_now(e, GS_SWEEP_DONE, with_sync))) return rc;
  /* the per-class deltas, as the caller adds them (GPhoCS.c:1495-1545) */
  GphRed R; R.rows = e->h_red; R.world = 1;
  out->accepted_internal = G.acc[0] - a0;
  out->accepted_mignode = G.acc[1] - a1;
  out->accepted_spr = G.acc[2] - a2;
  out->total_mig_nodes = G.acc[7] - a7;
  out->dData_internal = R.sum(0, 3);
  out->dLog_internal = R.sum(0, 4);
  out->dLog_mignode = R.sum(0, 5);
  out->dData_spr = R.sum(0, 6);
  out->dLog_spr = R.sum(0, 7);
  return 0;
}

int gph_engine_tau_evaluate(gph_engine *e, const gph_tau_args *a, gph_tau_result *out)
{
  if (!e || !e->initialized || !a || !out) return GPH_ESTATE;
  if (a->num_aff > 2 * GPH_MAXB) return GPH_EARG;
  SETDEV(e);
  { int rcs = flush_sync(e, true); if (rcs) return rcs; }
  GphTauArgs &A = e->G_h->tau;
  memset(&A, 0, sizeof A);
  A.ap = a->ap; A.son0 = a->son0; A.son1 = a->son1; A.isRoot = a->isRoot; A.num_aff = a->num_aff; A.mode = a->mode;
  A.tauold = a->tauold; A.taunew = a->taunew; A.taub0 = a->taub0; A.taub1 = a->taub1;
  A.taufactor0 = a->taufactor0; A.taufactor1 = a->taufactor1;
  for (int i = 0; i < a->num_aff; i++) {
    A.aff_bands[i] = a->aff_bands[i];
    A.start_or_end[i] = a->start_or_end[i];
    A.new_band_ages[i] = a->new_band_ages[i];
  }
  int rc = push_G(e);
  if (rc) return rc;
  if ((rc = launch_loci(e, 1, k_tau_eval, 0))) return rc;     /* stepwise: the finish of the previous proposal was a call of its own */
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = run_stage_now(e, GS_COUNT_ONLY, 1))) return rc;
  // first conflicting locus in serial (input) order: loci after it were never touched by
  // the reference; slot 14 holds the global index of a conflicting locus (1e300 = none)
  GphRed R; R.rows = e->h_red; R.world = 1;   /* the row as combined over the ranks by run_stage */
  out->ntj0 = (int64_t)R.sum(0, 0);
  out->ntj1 = (int64_t)R.sum(0, 1);
  out->genDelta = R.sum(0, 3);
  out->dataDelta = R.sum(0, 4);
  out->first_conflict_locus = R.mn(0, 14) < 1e299 ? (int64_t)R.mn(0, 14) : -1;
  return 0;
}

// the commit (flag 1) or revert (flag 0: of the loci before `limit`, the first conflicting one) of the evaluated tau proposal
static int tau_finish_now(gph_engine *e, int flag, long long limit)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  e->G_h->tau_flag = flag;
  e->G_h->tau_limit = limit;
  gg_fill_fin(*e->G_h, flag, limit);
  int rc = push_G(e);
  if (rc) return rc;
  return launch_loci(e, 5, k_tau_finish, 0);
}
int gph_engine_tau_commit(gph_engine *e) { return tau_finish_now(e, 1, (long long)1 << 62); }
int gph_engine_tau_revert(gph_engine *e, int64_t first_conflict)
{
  return tau_finish_now(e, 0, first_conflict >= 0 ? (long long)first_conflict : (long long)1 << 62);
}

int gph_engine_mixing_evaluate(gph_engine *e, double c, double *dataDelta)
{
  if (!e || !e->initialized || !dataDelta) return GPH_ESTATE;
  SETDEV(e);
  { int rcs = flush_sync(e, true); if (rcs) return rcs; }
  e->G_h->mix_c = c;
  int rc = push_G(e);
  if (rc) return rc;
  if ((rc = launch_loci(e, 2, k_mix_eval, 0))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = run_stage_now(e, GS_COUNT_ONLY, 2))) return rc;
  GphRed R; R.rows = e->h_red; R.world = 1;
  *dataDelta = R.sum(0, 0);
  return 0;
}

int gph_engine_mixing_commit(gph_engine *e, double c, double lnc)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  e->G_h->mix_flag = 1; e->G_h->mix_c = c; e->G_h->mix_lnc = lnc;
  int rc = push_G(e);
  if (rc) return rc;
  return launch_loci(e, 7, k_mix_finish, 0);
}

// mixing reject (GPhoCS.c:4881-4887): revertToSaved restores every locus exactly, and
// the evaluated state only ever lived in the shadow pages -- nothing to do.
int gph_engine_mixing_revert(gph_engine *e) { return e ? 0 : GPH_EARG; }

static int finish_owed(gph_engine *e);
// every finish that has been left for a later kernel, now (the caller is about to edit the main pages by other means)
static int owed_finishes(gph_engine *e)
{
  int rc = finish_owed(e);
  if (!rc) rc = mix_finish_owed(e);
  return rc;
}
static int apply_list(gph_engine *e)
{
  int rc;
  if ((rc = owed_finishes(e))) return rc;
  if ((rc = flush_pending(e))) return rc;
  launch_pre(e);
  if ((rc = launch_grid(e, GphGrid{(int)((e->L + GPH_FLAT_THREADS - 1) / GPH_FLAT_THREADS), 1}, GPH_FLAT_THREADS, 0, k_apply_list, e->ka, e->dev))) return rc;
  flat_launched(e, -1, 1);
  return 0;
}

// one accepted UpdateTheta (kind 0, population idx, diff = 1/new - 1/old) or UpdateMigRates (kind 1, band idx, diff = new -
// old rate) proposal as a touch-up list of its own
static int apply_one(gph_engine *e, int kind, int idx, int limit, double lnc, double diff)
{
  if (!e || !e->initialized || idx < 0 || idx >= limit) return GPH_EARG;
  SETDEV(e);
  { int rco = owed_finishes(e); if (rco) return rco; }    /* the touch-up edits the MAIN page: a commit that still sits in the shadow page goes first */
  GphGlobal &G = *e->G_h;
  G.napply = 1;
  G.apply[0].kind = kind; G.apply[0].idx = idx; G.apply[0].lnc = lnc; G.apply[0].diff = diff;
  int rc = push_G(e);
  if (rc) return rc;
  return apply_list(e);
}
int gph_engine_apply_theta(gph_engine *e, int32_t pop, double lnc, double thetaold, double thetanew)
{
  return apply_one(e, 0, pop, e ? e->cfg.K : 0, lnc, (1 / thetanew - 1 / thetaold));
}
int gph_engine_apply_migrate(gph_engine *e, int32_t band, double lnc, double old_rate, double new_rate)
{
  return apply_one(e, 1, band, e ? e->cfg.B : 0, lnc, (new_rate - old_rate));
}

int gph_engine_get_totals(gph_engine *e, double *cs, double *nc, double *ms, double *nm)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  const int K = e->cfg.K, B = e->cfg.B;
  int rc;
  if ((rc = push_if_dirty(e))) return rc;
  if ((rc = mix_finish_owed(e))) return rc;    /* the statistics of an accepted mixing proposal are scaled by its commit */
  if ((rc = reduce_stats(e))) return rc;
  if ((rc = run_stage_now(e, GS_TOTALS, 0))) return rc;
  const GphGlobal &G = *e->G_h;
  for (int p = 0; p < K; p++) { if (cs) cs[p] = G.tot_coal[p]; if (nc) nc[p] = G.tot_ncoal[p]; }
  for (int b = 0; b < B; b++) { if (ms) ms[b] = G.tot_mig[b]; if (nm) nm[b] = G.tot_nmig[b]; }
  return rc;
}

int gph_engine_synchronize(gph_engine *e, int32_t refresh, double *oldGen, double *newGen)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  if (!refresh) {
    /* nothing is returned without a refresh: the pass is deferred into the next sweep kernel (one page
     * round trip less per iteration); any other page-touching call runs it first */
    e->sync_pending = true;
    if (oldGen) *oldGen = 0.0;
    if (newGen) *newGen = 0.0;
    return 0;
  }
  int rc;
  if ((rc = flush_sync(e, true))) return rc;
  if ((rc = push_if_dirty(e))) return rc;
  if ((rc = launch_loci(e, 8, k_sync, refresh))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = run_stage_now(e, GS_REFRESH_DONE, 0))) return rc;   /* arg 0: the caller applies the difference */
  GphRed R; R.rows = e->h_red; R.world = 1;
  if (oldGen) *oldGen = R.sum(0, 1);
  if (newGen) *newGen = R.sum(0, 2);
  return rc;
}

int gph_engine_check_all(gph_engine *e, int32_t *ok, double *sumData, double *sumGen)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  int rc;
  if ((rc = flush_sync(e, true))) return rc;
  if ((rc = push_if_dirty(e))) return rc;
  if ((rc = launch_loci(e, 4, k_check, 0))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = reduce_stats(e))) return rc;
  e->G_h->nrec = 0;
  rc = run_stage_now(e, GS_CHECK_DONE, 0);
  if (ok) *ok = e->G_h->error != 9999;
  if (e->G_h->error == 9999) { e->G_h->error = 0; e->G_h->error_locus = -1; e->G_dirty = true; rc = 0; }
  { GphRed R; R.rows = e->h_red; R.world = 1;
    if (sumData) *sumData = R.sum(0, 1);
    if (sumGen) *sumGen = R.sum(0, 2); }
  return rc;
}

int gph_engine_get_counters(gph_engine *e, gph_counters *out, int32_t reset)
{
  if (!e || !out) return GPH_EARG;
  /* summed over ALL ranks (the counters ride in the reduced rows); e->counters = the values at the last reset */
  const GphGlobal &G = *e->G_h;
  double ev = 0, nd = 0, by = 0;
  for (int k = 0; k < 16; k++) { ev += G.cls_evals[k]; nd += G.cls_nodes[k]; by += G.cls_bytes[k]; }
  out->evals = (int64_t)ev - e->counters.evals;
  out->eval_nodes = (int64_t)nd - e->counters.eval_nodes;
  out->eval_bytes = by - e->counters.eval_bytes;
  out->not_enough_migs = (int64_t)G.cnt_notenough - e->counters.not_enough_migs;
  if (reset) { e->counters.evals = (int64_t)ev; e->counters.eval_nodes = (int64_t)nd; e->counters.eval_bytes = by; e->counters.not_enough_migs = (int64_t)G.cnt_notenough; }
  return 0;
}

int gph_engine_last_kernel_ms(gph_engine *e, int32_t which, double *ms)
{
  if (!e || !ms || which < 0 || which >= GPH_NCLS) return GPH_EARG;
  *ms = e->last_ms[which];
  return 0;
}

int64_t gph_engine_num_loci(gph_engine *e) { return e ? e->L : 0; }

int gph_engine_class_stats(gph_engine *e, int32_t which, double *out5, int32_t reset)
{
  if (!e || !out5 || which < 0 || which >= GPH_NCLS) return GPH_EARG;
  const GphGlobal &G = *e->G_h;
  if (which >= 16) {   /* (classes the chain state keeps no evaluation counters for) */
    out5[0] = e->cls_launches[which]; out5[1] = e->cls_ms[which]; out5[2] = out5[3] = out5[4] = 0.0;
    if (reset) e->cls_launches[which] = e->cls_ms[which] = 0;
    return 0;
  }
  out5[0] = e->cls_launches[which]; out5[1] = e->cls_ms[which]; out5[2] = G.cls_evals[which] - e->cls_evals0[which];
  out5[3] = G.cls_bytes[which] - e->cls_bytes0[which]; out5[4] = G.cls_nodes[which] - e->cls_nodes0[which];
  if (reset) {
    e->cls_launches[which] = e->cls_ms[which] = 0;
    e->cls_evals0[which] = G.cls_evals[which]; e->cls_bytes0[which] = G.cls_bytes[which]; e->cls_nodes0[which] = G.cls_nodes[which];
  }
  return 0;
}

// host synchronisations, cross-rank exchanges and kernel launches since the engine was created
int gph_engine_host_stats(gph_engine *e, int64_t *syncs, int64_t *collectives, int64_t *launches, int32_t *resident_mode)
{
  if (!e) return GPH_EARG;
  if (syncs) *syncs = e->n_syncs;
  if (collectives) *collectives = e->n_collectives;
  if (launches) *launches = e->n_launches;
  if (resident_mode) *resident_mode = resident(e) ? 1 : 0;
  return 0;
}
// classes whose launches are bracketed by HIP events (bit k = class k of gph_engine_last_kernel_ms); default all
int gph_engine_set_timing(gph_engine *e, uint32_t class_mask)
{
  if (!e) return GPH_EARG;
  e->timing_mask = class_mask;
  return 0;
}

// out[5n]: exp(x), log(x), sqrt(|x|), x/y, floor(x) evaluated ON THE DEVICE
int gph_debug_math(const double *x, const double *y, int32_t n, double *out, int32_t device)
{
  if (!x || !y || !out || n <= 0) return GPH_EARG;
  return debug_math(x, y, n, out, device);
}
// tests only (not part of include/gphocs_hip.h): out[3n] = gph_accept(u, x), u < gph_exp(x), gph_accept_bounds_t(u, x)
int gph_debug_accept_(const double *x, const double *u, int32_t n, double *out, int32_t device)
{
  if (!x || !u || !out || n <= 0) return GPH_EARG;
  return debug_math(x, u, n, out, device, 1);
}
// tests only (not part of include/gphocs_hip.h): the cross-locus reduction on its own, no engine.  out0: [nsets][L][GPH_OUT_SLOTS]
// (section 0, nc0 columns of it folded), stats1: [nsets][L][nc1] (section 1); launch i of `launches` folds set i % nsets into
// rows[i][GPH_RED_ROW], back to back as the reductions of an iteration (gph_backend.h: debug_reduce); err_word: what the error
// word holds.  rows start as the poison, so what a launch did not write reads as that.  info[10] (may be null): GPH_RED_COLS,
// _STRIDE, _ROW, _BLOCKS, _SUBS, _UNROLL (the last two 0 in the host build: a serial loop), GPH_OUT_SLOTS, the ticket word after
// the last launch, the poison's low and high words.  Refused before anything is allocated, launched or written: GPH_EARG
int gph_debug_reduce_(const double *out0, const double *stats1, int64_t L, int32_t nc0, int32_t nc1, int32_t nsets, int32_t err_word,
                      int32_t launches, double *rows, int32_t *info, int32_t device)
{
  if (L < 1 || L > INT32_MAX || nc0 < 0 || nc0 > GPH_OUT_SLOTS || nc1 < 0 || nc1 > GPH_RED_COLS || (nc0 == 0 && nc1 == 0)) return GPH_EARG;
  if ((nc0 > 0 && !out0) || (nc1 > 0 && !stats1) || nsets < 1 || launches < 1 || !rows) return GPH_EARG;
  return debug_reduce(out0, stats1, L, nc0, nc1, nsets, err_word, launches, rows, info, device);
}

// tests only (not part of include/gphocs_hip.h): the pass ahead of the sweep.  info[4] = on, M, C, bytes per locus;
// kprev (may be null): the per-locus counts in input order -- what each locus consumed in its last sweep -- read
// (set = 0) or written (set != 0: the next pass generates min(M, roundup64(kprev + 64)) draws for the locus)
int gph_engine_rng_ahead_(gph_engine *e, int32_t *info, int32_t *kprev, int32_t set)
{
  if (!e || !e->loaded) return GPH_EARG;
  SETDEV(e);
  if (info) { if (set < 0) { info[0] = e->ra_place_b && e->dev.ra_M > 0 && resident(e); info[1] = e->ra_b_valid; return 0; }
    info[0] = e->dev.ra_M > 0; info[1] = e->dev.ra_M; info[2] = 1 << e->dev.ra_cshift; info[3] = (int32_t)(e->ra_bytes / (size_t)e->L); }
  if (!kprev) return 0;
  if (e->dev.ra_M <= 0) return GPH_ESTATE;
  if (e->initialized) { int rcs = finish_sync(e); if (rcs) return rcs; }
  std::vector<int32_t> by_slot((size_t)e->L);
  if (set) {
    rng_ahead_dirty(e);         /* (a pass made behind the last sweep used the old counts) */
    for (int64_t j = 0; j < e->L; j++) by_slot[j] = kprev[e->h_orig[j]];
    return h2d(e, e->dev.ra_kprev, by_slot.data(), sizeof(int32_t) * e->L);
  }
  if (d2h(e, by_slot.data(), e->dev.ra_kprev, sizeof(int32_t) * e->L)) return GPH_EHIP;
  for (int64_t j = 0; j < e->L; j++) kprev[e->h_orig[j]] = by_slot[j];
  return 0;
}
// tests only (not part of include/gphocs_hip.h): the buffers of the last pass as they stand, in input order (any of them may
// be null): draws[L][M], ckpt[L][M / C + 1][4] (the device keeps them with the slot as the fastest index), tail[L][4].
// Only reads: a pass made behind the last sweep stays valid (it is waited for, its draws are what the buffers then hold)
int gph_engine_rng_ahead_fetch_(gph_engine *e, double *draws, uint32_t *ckpt, uint32_t *tail)
{
  if (!e || !e->loaded) return GPH_EARG;
  SETDEV(e);
  if (e->dev.ra_M <= 0) return GPH_ESTATE;
  if (e->initialized) { int rcs = finish_sync(e); if (rcs) return rcs; }
  if (e->ra_b_valid) rng_ahead_drain(e);
  const size_t L = (size_t)e->L, M = (size_t)e->dev.ra_M, nck = (M >> e->dev.ra_cshift) + 1;
  if (draws) {
    std::vector<double> by_slot(L * M);
    if (d2h(e, by_slot.data(), e->dev.ra_draws, sizeof(double) * L * M)) return GPH_EHIP;
    for (size_t j = 0; j < L; j++) memcpy(draws + (size_t)e->h_orig[j] * M, by_slot.data() + j * M, sizeof(double) * M);
  }
  if (ckpt) {
    std::vector<uint32_t> by_slot(4 * nck * L);
    if (d2h(e, by_slot.data(), e->dev.ra_ckpt, 16 * nck * L)) return GPH_EHIP;
    for (size_t j = 0; j < L; j++)
      for (size_t c = 0; c < nck; c++) memcpy(ckpt + 4 * ((size_t)e->h_orig[j] * nck + c), by_slot.data() + 4 * (c * L + j), 16);
  }
  if (tail) {
    std::vector<uint32_t> by_slot(4 * L);
    if (d2h(e, by_slot.data(), e->dev.ra_tail, 16 * L)) return GPH_EHIP;
    for (size_t j = 0; j < L; j++) memcpy(tail + 4 * (size_t)e->h_orig[j], by_slot.data() + 4 * j, 16);
  }
  return 0;
}

#ifndef GPH_BUILD_ID
#define GPH_BUILD_ID "unidentified"
#endif
const char *gph_build_id(void) { return GPH_BUILD_ID; }
const char *gph_build_compiler(void)
{
#ifdef __clang_version__
  return "clang " __clang_version__;
#else
  return "g++ " __VERSION__;
#endif
}
const char *gph_runtime_version(void)
{
  static char buf[96];
  runtime_version(buf, sizeof buf);
  return buf;
}

// Decision-level transcript (upstream -DLOG_STEPS: GPhoCS.c:2363-2401, 2540-2577, 2654-2718, patch.c:1451-1454):
// the three genealogy sweeps append one record per printed fragment for the selected loci -- kind 1 node-age proposal
// {node, t, tnew}, 2 considerEventMove {event, source pop, target pop, old age, new age, new event}, 3 decision {accepted,
// lnacceptance}, 4 migration-node proposal {migration node, t, tnew}, 5 SPR {node, father, father's population}.  Compiled
// into the test builds only (GPH_LOGSTEPS: the host build of tests/hostemu and libgphocs_hip_plain.so).
int gph_engine_steplog_enable(gph_engine *e, const int64_t *loci, int32_t n, int32_t cap)
{
#if !defined(GPH_LOGSTEPS) && !defined(GPH_BBCOUNT)    /* (GPH_BBCOUNT: tools/bbcount.sh borrows the record buffer for basic-block counters) */
  (void)e; (void)loci; (void)n; (void)cap;
  return GPH_EARG;      /* not compiled into this build of the library */
#else
  if (!e || !e->loaded || n < 0 || cap < 1 || (n > 0 && !loci)) return GPH_EARG;
  SETDEV(e);
  /* (before the first initialisation nothing is in flight, and the host mirror of the chain state -- not yet pushed -- must
   * not be overwritten by a read-back) */
  if (e->initialized) { int rcs = flush_sync(e, true); if (!rcs) rcs = finish_sync(e); if (rcs) return rcs; }
  dev_free((void *)e->dev.slog_map); dev_free(e->dev.slog); dev_free(e->dev.slog_n);
  e->dev.slog_map = nullptr; e->dev.slog = nullptr; e->dev.slog_n = nullptr; e->dev.slog_cap = 0;
  e->slog_sel = n;
  if (n == 0) return 0;
  std::vector<int32_t> map((size_t)e->L, -1);
  for (int64_t j = 0; j < e->L; j++)
    for (int k = 0; k < n; k++)
      if (e->h_orig[j] + e->cfg.locus_begin == loci[k]) map[j] = k;
  std::vector<int32_t> zero((size_t)n, 0);
  /* allocate into locals and publish them to the kernels' view only when every copy has succeeded: a partial failure
   * must not leave dev.slog_map pointing at uninitialised memory */
  int32_t *d_map = nullptr, *d_n = nullptr;
  double *d_log = nullptr;
  if (dev_alloc((void **)&d_map, sizeof(int32_t) * e->L) || dev_alloc((void **)&d_log, sizeof(double) * 8 * (size_t)n * cap) ||
      dev_alloc((void **)&d_n, sizeof(int32_t) * n) ||
      h2d(e, d_map, map.data(), sizeof(int32_t) * e->L) || h2d(e, d_n, zero.data(), sizeof(int32_t) * n)) {
    dev_free(d_map); dev_free(d_log); dev_free(d_n);
    e->slog_sel = 0;
    return GPH_EHIP;
  }
  e->dev.slog_map = d_map; e->dev.slog = d_log; e->dev.slog_n = d_n;
  e->dev.slog_cap = cap;
  return 0;
#endif
}
// records of selected locus `idx` so far (out: 8 doubles per record, at most max_records of them; *nrec = records
// written by the kernels, which may exceed the capacity given to _enable); reset != 0 empties the buffer
int gph_engine_steplog_fetch(gph_engine *e, int32_t idx, double *out, int32_t max_records, int32_t *nrec, int32_t reset)
{
#if !defined(GPH_LOGSTEPS) && !defined(GPH_BBCOUNT)
  (void)e; (void)idx; (void)out; (void)max_records; (void)nrec; (void)reset;
  return GPH_EARG;
#else
  if (!e || !e->dev.slog || idx < 0 || idx >= e->slog_sel || !nrec) return GPH_EARG;
  SETDEV(e);
  { int rcs = finish_sync(e); if (rcs) return rcs; }
  int32_t n = 0;
  if (d2h(e, &n, e->dev.slog_n + idx, sizeof n)) return GPH_EHIP;
  *nrec = n;
#ifdef GPH_BBCOUNT
  n = e->dev.slog_cap;       /* the whole buffer: it holds counters, not records */
#endif
  const int32_t m = std::min(std::min(n, e->dev.slog_cap), max_records);
  if (out && m > 0 && d2h(e, out, e->dev.slog + (size_t)idx * e->dev.slog_cap * 8, sizeof(double) * 8 * (size_t)m)) return GPH_EHIP;
  if (reset) { const int32_t z = 0; if (h2d(e, e->dev.slog_n + idx, &z, sizeof z)) return GPH_EHIP; }
  return 0;
#endif
}

int gph_engine_hbm_bytes(gph_engine *e, double *bytes)
{
  if (!e || !bytes) return GPH_EARG;
  *bytes = 2.0 * e->pages_bytes + (double)e->cond_bytes + (double)e->seq_bytes_total + 8.0 * GPH_OUT_SLOTS * e->L + (double)e->ra_bytes;
  return 0;
}

// starting locus rates in input order (VAR start-up or any caller-supplied rates); `draws` = rndu() draws every
// locus's stream has spent producing them.  Before gph_engine_init_genealogies.
int gph_engine_set_locus_rates(gph_engine *e, const double *rates, int32_t draws, int32_t variable)
{
  if (!e || !e->loaded || e->initialized || !rates || draws < 0) return GPH_ESTATE;
  SETDEV(e);
  std::vector<double> r(e->L);
  for (int64_t j = 0; j < e->L; j++) r[j] = rates[e->h_orig[j]];
  if (!e->d_mutRate && dev_alloc((void **)&e->d_mutRate, sizeof(double) * e->L)) return GPH_EHIP;
  if (h2d(e, e->d_mutRate, r.data(), sizeof(double) * e->L)) return GPH_EHIP;
  e->init_predraws = draws;
  e->var_rates = variable != 0;
  return 0;
}

// UpdateLocusRate (GPhoCS.c:4598-4680): a serial scan by one wavefront + a parallel write-back (gph_kernels.h)
// one vector of doubles from the rank that owns it to every rank, through the sum all-reduce (the others add
// zeros: exact), in pieces small enough for any caller-supplied hook (<= 24 doubles a call)
static int xreduce(gph_engine *e, double *sums, int nsum, double *mins, int nmin)
{
  int rc = 0;
  if (e->allreduce) rc = e->allreduce(e->allreduce_user, sums, nsum, mins, nmin);
  else if (e->comm) rc = gph_comm_allreduce_host(e->comm, sums, nsum, mins, nmin);
  else return 0;
  e->n_collectives++;
  return rc ? GPH_EHIP : 0;
}
static bool multi_rank(const gph_engine *e) { return e->allreduce || (e->comm && gph_comm_world(e->comm) > 1); }
static int lr_share(gph_engine *e, bool mine, std::vector<double> &v)
{
  if (!multi_rank(e)) return 0;
  for (size_t off = 0; off < v.size(); off += 24) {
    double buf[24];
    const int nn = (int)(v.size() - off < 24 ? v.size() - off : 24);
    for (int i = 0; i < nn; i++) buf[i] = mine ? v[off + i] : 0.0;
    int rc = xreduce(e, buf, nn, nullptr, 0);
    if (rc) return rc;
    for (int i = 0; i < nn; i++) v[off + i] = buf[i];
  }
  return 0;
}

int gph_engine_locus_rate_update(gph_engine *e, double finetune, double alpha, gph_locus_rate_result *io)
{
  if (!e || !e->initialized || !io) return GPH_ESTATE;
  io->accepted = 0;
  if (finetune <= 0.0) return 0;                       /* GPhoCS.c:4606 */
  rng_ahead_dirty(e);
  const bool owner = e->cfg.locus_begin == 0;          /* this rank holds the reference locus (genRateRef = 0) */
  SETDEV(e);
  if (!multi_rank(e) && (!owner || e->cfg.L_total != e->L)) {
    fprintf(stderr, "gphocs_hip: UpdateLocusRate over a shard of the loci needs the all-reduce hook (gph_engine_set_allreduce)\n");
    return GPH_EARG;
  }
  int rc = 0;
  if ((rc = flush_sync(e, true))) return rc;
  if ((rc = push_if_dirty(e))) return rc;
  const GphLayout &y = e->lay;
  const int n = e->cfg.n, N = 2 * n - 1;
  /* ---- the reference locus as every rank needs it: node records + rate, likelihood, root (every call), sequence
   * block (first call: it never changes).  32-bit words travel as doubles */
  std::vector<char> refpg(y.page_bytes, 0);
  int jr = -1;
  if (owner) {
    for (int64_t j = 0; j < e->L; j++) if (e->h_orig[j] == 0) jr = (int)j;
    if ((rc = d2h(e, refpg.data(), e->dev.pages + (size_t)jr * y.page_bytes, y.page_bytes))) return rc;
  }
  {
    std::vector<double> v(4 * N + 4, 0.0);
    if (owner) {
      const uint32_t *w = (const uint32_t *)(refpg.data() + y.o_nd);
      for (int i = 0; i < 4 * N; i++) v[i] = (double)w[i];
      v[4 * N] = ((const double *)(refpg.data() + y.o_fscal))[FS_MUTRATE];
      v[4 * N + 1] = ((const double *)(refpg.data() + y.o_fscal))[FS_DATALNL];
      v[4 * N + 2] = (double)((const int32_t *)(refpg.data() + y.o_iscal))[IS_ROOT];
      v[4 * N + 3] = (double)e->h_P[jr];
    }
    if ((rc = lr_share(e, owner, v))) return rc;
    if (!owner) {
      uint32_t *w = (uint32_t *)(refpg.data() + y.o_nd);
      for (int i = 0; i < 4 * N; i++) w[i] = (uint32_t)v[i];
      ((double *)(refpg.data() + y.o_fscal))[FS_MUTRATE] = v[4 * N];
      ((double *)(refpg.data() + y.o_fscal))[FS_DATALNL] = v[4 * N + 1];
      ((int32_t *)(refpg.data() + y.o_iscal))[IS_ROOT] = (int32_t)v[4 * N + 2];
    }
    e->lr.ref_P = (int32_t)v[4 * N + 3];
    e->lr.rref0 = v[4 * N];
    e->lr.likref0 = v[4 * N + 1];
  }
  const int Pr = e->lr.ref_P, Pmax = y.Pmax > Pr ? y.Pmax : Pr;
  if (!e->d_lrec) {
    std::vector<int32_t> slot_of(e->L);
    for (int64_t j = 0; j < e->L; j++) slot_of[e->h_orig[j]] = (int32_t)j;
    // dynamic LDS of the scan: guest sequence block | reference sequence block | guest nodes | reference nodes | scratch
    const int seqb = align_up(GPH_Q_TERMS(Pmax, n, y.cnt16) + (Pmax > GPH_WAVE ? 8 * Pmax : 0), 16), ndb = N * (int)sizeof(GphNode);
    const int fixed = 2 * seqb + 2 * ndb;
    /* the compiled program of the reference locus is a lane-per-node construction: not in the big-tree variant */
    const int progb = GPH_BIG_TREE ? 0 : (n - 1) * GPH_WAVE * 16;
    const int lfb = !GPH_BIG_TREE && Pr >= 1 && Pr <= GPH_WAVE ? n * Pr * 32 : 0;      // the reference locus's leaves as conditional arrays
    const int budget = 96 * 1024 - (int)sizeof(GphLds) - progb - align_up(N * 8, 16) - lfb;
    int Pscr = (budget - fixed) / ((n - 1) * 32);
    if (const char *ov = getenv("GPH_LR_PSCR")) Pscr = atoi(ov) < Pscr ? atoi(ov) : Pscr;   /* tests: force the global-scratch path */
    if (Pscr > Pmax) Pscr = Pmax;
    if (Pscr < 0) Pscr = 0;
    const double finetune0 = e->lr.finetune; (void)finetune0;
    const int32_t refP = e->lr.ref_P; const double r0 = e->lr.rref0, l0 = e->lr.likref0;
    memset(&e->lr, 0, sizeof e->lr);
    e->lr.ref_P = refP; e->lr.rref0 = r0; e->lr.likref0 = l0;
    e->lr.o_rseq = seqb; e->lr.o_gnd = 2 * seqb; e->lr.o_rnd = 2 * seqb + ndb; e->lr.o_scr = fixed; e->lr.Pscr = Pscr;
    // behind the scratch: the reference locus's compiled program (one 16-byte entry per step and lane) and edge probabilities
    e->lr.o_prog = fixed + (n - 1) * Pscr * 32;
    e->lr.o_pe = e->lr.o_prog + progb;
    e->lr.o_lf = lfb ? e->lr.o_pe + align_up(N * 8, 16) : 0;
    e->lr_lds_bytes = e->lr.o_pe + align_up(N * 8, 16) + lfb;
    /* The scan keeps TWO sequence blocks in its dynamic LDS (the reference locus's, and the one it re-evaluates), each sized for
     * the largest locus of the rank; loci whose block stays in HBM for the per-locus kernels ("huge", round 5) are staged here like
     * any other (lr_load copies from HBM).  What does not fit next to the static image cannot run: ALL ranks learn it in one
     * exchange and fail together before any kernel of the update (a rank returning alone would leave the others in the next
     * collective -- ADVICE round 5). */
    {
      const int lds_max = 160 * 1024;
      double too_big[1] = {e->lr_lds_bytes + (int)sizeof(GphLds) > lds_max ? 1.0 : 0.0};
      if (multi_rank(e) && (rc = xreduce(e, too_big, 1, nullptr, 0))) return rc;
      if (too_big[0] != 0.0) {
        if (e->lr_lds_bytes + (int)sizeof(GphLds) > lds_max)
          fprintf(stderr, "gphocs_hip: locus-mut-rate VAR: the serial scan of UpdateLocusRate needs %d bytes of LDS for two sequence "
                          "blocks of up to %d phased patterns (%d bytes each) next to the %d-byte image; the CU has %d\n",
                  e->lr_lds_bytes, Pmax, seqb, (int)sizeof(GphLds), lds_max);
        memset(&e->lr, 0, sizeof e->lr);
        return GPH_EARG;
      }
    }
    e->lr.ref_seq_bytes = GPH_Q_BYTES(Pr, n, y.cnt16);
    rc |= dev_alloc((void **)&e->d_lrec, sizeof(GphLrRec) * e->L);
    rc |= dev_alloc((void **)&e->d_lpre, sizeof(GphLrPre) * e->L);
    rc |= dev_alloc((void **)&e->d_slot_of, sizeof(int32_t) * e->L);
    rc |= dev_alloc((void **)&e->d_lr_result, sizeof(double) * 16);
    rc |= dev_alloc((void **)&e->d_lr_gscr, Pmax > Pscr ? sizeof(double) * 4 * (size_t)(n - 1) * Pmax : 16);
    rc |= dev_alloc((void **)&e->d_ref_page, y.page_bytes);
    rc |= dev_alloc((void **)&e->d_ref_seq, e->lr.ref_seq_bytes + 16);
    if (rc) return GPH_EHIP;
    if (h2d(e, e->d_slot_of, slot_of.data(), sizeof(int32_t) * e->L)) return GPH_EHIP;
    e->lr.result = e->d_lr_result; e->lr.rec = e->d_lrec; e->lr.pre = e->d_lpre; e->lr.slot_of = e->d_slot_of; e->lr.gscr = e->d_lr_gscr;
    /* the reference locus's sequence block: the owner's copy goes round once */
    std::vector<char> seqblk(e->lr.ref_seq_bytes + 16, 0);
    if (owner && e->lr.ref_seq_bytes > 0 &&
        (rc = d2h(e, seqblk.data(), e->dev.seq + e->h_seq_off[jr], e->lr.ref_seq_bytes))) return rc;
    {
      std::vector<double> v(e->lr.ref_seq_bytes / 4, 0.0);
      if (owner) for (size_t i = 0; i < v.size(); i++) v[i] = (double)((const uint32_t *)seqblk.data())[i];
      if ((rc = lr_share(e, owner, v))) return rc;
      if (!owner) for (size_t i = 0; i < v.size(); i++) ((uint32_t *)seqblk.data())[i] = (uint32_t)v[i];
    }
    if (e->lr.ref_seq_bytes > 0 && h2d(e, e->d_ref_seq, seqblk.data(), e->lr.ref_seq_bytes)) return GPH_EHIP;
    e->lr.ref_seq = e->d_ref_seq;
    e->lr.ref_page = e->d_ref_page;
    if ((rc = scan_lds_limit(e))) return rc;
  }
  if (h2d(e, e->d_ref_page, refpg.data(), y.page_bytes)) return GPH_EHIP;
  e->lr.finetune = finetune; e->lr.alpha = alpha; e->lr.beta = e->G_h->beta;
  e->lr.first = owner ? 1 : 0;
  if ((rc = launch_loci(e, 11, k_lrate_prep, finetune, e->d_lpre))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = run_stage_now(e, GS_COUNT_ONLY, 11))) return rc;
  /* ---- the scan, rank after rank in locus order: state = {next locus, rref, likref, dataLogLikelihood,
   * logLikelihood, rateVar, accepted, prepared rates used}; the rank whose block starts at `next` scans and
   * publishes the state, the others add zeros */
  double st[8] = {0.0, e->lr.rref0, e->lr.likref0, io->dataLogLikelihood, io->logLikelihood, io->rateVar, 0.0, 0.0};
  double res[16] = {0};
  for (int guard = 0; (int64_t)st[0] < e->cfg.L_total; guard++) {
    if (guard > 1 << 20) return GPH_ESTATE;
    const bool mine = (int64_t)st[0] == e->cfg.locus_begin;
    double nx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mine) {
      e->lr.rref0 = st[1]; e->lr.likref0 = st[2];
      e->lr.dataLnL = st[3]; e->lr.logL = st[4]; e->lr.rateVar = st[5];
      if ((rc = launch_wave(e, 9, k_lrate_scan, e->lr_lds_bytes, e->lr))) return rc;
      if ((rc = d2h(e, res, e->d_lr_result, sizeof res))) return rc;
      collect_times(e);
      if (res[4] != 0.0) { fprintf(stderr, "gphocs_hip: Fatal Error %04d reported by the locus-rate scan\n", (int)res[4]); return GPH_EKERNEL; }
      nx[0] = (double)(e->cfg.locus_begin + e->L); nx[1] = res[13]; nx[2] = res[14];
      nx[3] = res[1]; nx[4] = res[2]; nx[5] = res[3]; nx[6] = st[6] + res[0]; nx[7] = st[7] + res[5];
    }
    if (multi_rank(e)) { if ((rc = xreduce(e, nx, 8, nullptr, 0))) return rc; }
    else if (!mine) return GPH_ESTATE;
    if (nx[0] <= st[0]) { fprintf(stderr, "gphocs_hip: the ranks' locus blocks do not tile 0..L_total\n"); return GPH_EARG; }
    memcpy(st, nx, sizeof st);
  }
  if (owner) {
    /* the reference locus's record: its last accepted rate / likelihood and the number of accepted proposals */
    GphLrRec r;
    const int32_t *is = (const int32_t *)(refpg.data() + y.o_iscal);
    r.rate = st[1]; r.lnl = st[2]; r.rx = (uint32_t)is[IS_RX]; r.ry = (uint32_t)is[IS_RY]; r.rz = (uint32_t)is[IS_RZ];
    r.flag = (int32_t)st[6] << 2;
    if (h2d(e, e->d_lrec + jr, &r, sizeof r)) return GPH_EHIP;
  }
  if ((rc = launch_loci(e, 10, k_lrate_apply, e->d_lrec))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = run_stage_now(e, GS_COUNT_ONLY, 10))) return rc;
  io->accepted = (int64_t)st[6];
  io->dataLogLikelihood = st[3];
  io->logLikelihood = st[4];
  io->rateVar = st[5];
  e->lr_hits = st[7];
#ifdef GPH_LRSTAMP
  fprintf(stderr, "evaluator stamps: setup+exp %.0f, nodes %.0f, root %.0f cycles per call (%.0f calls, %.1f steps)\n", res[8] / res[11], res[9] / res[11], res[10] / res[11], res[11], res[12] / res[11]);
#endif
  if (getenv("GPH_LR_VERBOSE"))
    fprintf(stderr, "gphocs_hip: locus-rate scan: %.0f of %lld proposals decided with the prepared likelihood; %.3g shader cycles in %.3g s (%.0f MHz)\n",
            st[7], (long long)(e->cfg.L_total - 1), res[6], res[7] / 1e8, res[7] > 0 ? res[6] / (res[7] / 1e8) / 1e6 : 0.0);
  return 0;
}

// The parts of an iteration, one per function performMCMC calls (GPhoCS.c:1495-1821).  gph_engine_iteration_ queues them
// all and synchronises once; gph_engine_part_ runs ONE and returns with its result on the host (the reference's own
// performMCMC driving the engine through the functions of GPhoCS.h:84-100: oracle/integration_binding.c).
// e->fin_owed: the commit / revert of the last decided UpdateTau / UpdateSampleAge proposal has not run yet -- it rides
// at the head of the next evaluate kernel (the next population's, or mixing's): the decision stage froze what it needs
// in the chain state (GphTauFin), and the stage that proposes the next move goes out in the same launch as the decision.
// GPH_NO_FUSE=1 (tests) runs every finish as a kernel of its own, as the stepwise entry points do.
static int finish_owed(gph_engine *e)
{
  if (!e->fin_owed) return 0;
  e->fin_owed = false;
  return launch_loci(e, 5, k_tau_finish, 0);
}
// an evaluate kernel of the iteration and the reduction of its outputs; the finish that is owed rides at the kernel's head
// (GPH_NO_FUSE: goes first, as a kernel of its own)
static int evaluate_fused(gph_engine *e, int cls, decltype(&k_tau_eval) kernel)
{
  int rc;
  if (e->no_fuse && (rc = finish_owed(e))) return rc;
  const int fuse = e->fin_owed;
  e->fin_owed = false;
  if ((rc = launch_loci(e, cls, kernel, fuse))) return rc;
  return reduce_local(e, 0, GPH_OUT_SLOTS);
}
static int part_sweep(gph_engine *e, int32_t iteration, double ftCoal, double ftMig, bool chained = false)
{
  int rc, with_sync;
  if ((rc = sweep_launch(e, 7, ftCoal, ftMig, with_sync, chained))) return rc;
  return run_stage(e, GS_SWEEP_DONE, with_sync, iteration);
}
static int part_lrate(gph_engine *e, int32_t iteration, const double *lr_alpha_finetune, int64_t *lr_accepted, double *lr_rateVar)
{
  // UpdateLocusRate, GPhoCS.c:1554-1563, 4598-4680 (host-driven: resident() is false with variable rates)
  int rc;
  GphGlobal &Gh = *e->G_h;
  gph_locus_rate_result R;
  R.accepted = 0; R.dataLogLikelihood = Gh.dataLogLikelihood; R.logLikelihood = Gh.logLikelihood; R.rateVar = *lr_rateVar;
  if ((rc = gph_engine_locus_rate_update(e, lr_alpha_finetune[1], lr_alpha_finetune[0], &R))) return rc;
  Gh.dataLogLikelihood = R.dataLogLikelihood; Gh.logLikelihood = R.logLikelihood; *lr_rateVar = R.rateVar;
  *lr_accepted += R.accepted;
  gg_rec(Gh, REC_LRATE, 0, (long long)R.accepted);
  if ((rc = push_G(e))) return rc;
  if ((rc = reduce_stats(e))) return rc;
  return run_stage(e, GS_TOTALS, 0, iteration);
}
static int part_tau(gph_engine *e, int32_t iteration, bool first_proposed)
{
  int rc;
  const GphGlobal &Gh = *e->G_h;
  const int K = Gh.K, Kc = Gh.Kc;
  for (int ap = Kc; ap < K; ++ap) {
    if ((ap > Kc || !first_proposed) && (rc = run_stage(e, GS_TAU_PROPOSE, ap, iteration))) return rc;
    if ((rc = evaluate_fused(e, 1, k_tau_eval))) return rc;
    if ((rc = run_stage(e, GS_TAU_DECIDE, ap, iteration))) return rc;
    e->fin_owed = true;
  }
  return run_stage(e, GS_TAU_END, 0, iteration);
}
static int part_sage(gph_engine *e, int32_t iteration)
{
  int rc;
  const GphGlobal &Gh = *e->G_h;
  for (int pop = 0; pop < Gh.Kc; ++pop) {
    if (!Gh.updateSampleAge[pop]) continue;
    if ((rc = run_stage(e, GS_SAGE_PROPOSE, pop, iteration))) return rc;
    if ((rc = evaluate_fused(e, 1, k_tau_eval))) return rc;
    if ((rc = run_stage(e, GS_SAGE_DECIDE, pop, iteration))) return rc;
    e->fin_owed = true;
  }
  return run_stage(e, GS_SAGE_END, 0, iteration);
}
static int part_mix(gph_engine *e, int32_t iteration)
{
  int rc;
  const GphGlobal &Gh = *e->G_h;
  if ((rc = run_stage(e, GS_MIX_PROPOSE, 0, iteration))) return rc;
  if (Gh.ftMixing > 0.0) {
    if ((rc = evaluate_fused(e, 2, k_mix_eval))) return rc;
    if ((rc = run_stage(e, GS_MIX_DECIDE, 0, iteration))) return rc;
    e->mix_owed = true;        /* at the head of the next sweep kernel (sweep_launch), or mix_finish_owed() -- GPH_NO_FUSE: now */
    if (e->no_fuse) return mix_finish_owed(e);
  }
  return 0;
}
// the genLogLikelihood refresh of every locus after sampleMigRates (GPhoCS.c:1749-1757), inside synchronizeEvents' pass
static int part_refresh(gph_engine *e, int32_t iteration)
{
  int rc;
  if ((rc = launch_loci(e, 8, k_sync, 1))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  return run_stage(e, GS_REFRESH_DONE, 1, iteration);
}
// checkAll, patch.c:2745-2884: consistency checks + accumulator resynchronisation
static int part_check(gph_engine *e, int32_t iteration)
{
  int rc;
  if ((rc = flush_sync(e, false))) return rc;
  if ((rc = launch_loci(e, 4, k_check, 0))) return rc;
  if ((rc = reduce_local(e, 0, GPH_OUT_SLOTS))) return rc;
  if ((rc = reduce_stats(e))) return rc;
  return run_stage(e, GS_CHECK_DONE, 0, iteration);
}

// ---------------------------------------------------------------- one MCMC iteration, device-resident
// The iteration body of performMCMC (GPhoCS.c:1476-1821) as ONE stream of launches: every per-locus loop is a kernel
// over the loci, every `omp atomic` accumulation a fixed-shape reduction (+ one RCCL all-gather of the reduced row over
// several GPUs), everything the reference does on its main thread between two loops a k_global stage (gph_global.h)
// that reads the reduced rows in HBM and leaves the model, the pending proposal and the accept flag in the chain
// state for the next kernel.  The host synchronises ONCE, at the end, to read the chain state back (trace writer,
// next sweep's kernel arguments).  In host mode (caller-supplied all-reduce hook, ranks sharing a GPU, UpdateLocusRate,
// host emulation) the same launches run with a synchronisation per stage and gg_stage on the host mirror.
// lr: UpdateLocusRate's settings and running state (`locus-mut-rate VAR`), NULL = constant / fixed rates.
int gph_engine_iteration_(gph_engine *e, int32_t iteration, const double *lr_alpha_finetune, int64_t *lr_accepted, double *lr_rateVar)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  int rc;
  GphGlobal &Gh = *e->G_h;    /* settings only: the running state is on the device until finish_sync */
  if ((rc = push_if_dirty(e))) return rc;
  if ((rc = part_sweep(e, iteration, Gh.ftCoalTime, Gh.ftMigTime, true))) return rc;
  if (lr_alpha_finetune && (rc = part_lrate(e, iteration, lr_alpha_finetune, lr_accepted, lr_rateVar))) return rc;
  if ((rc = run_stage(e, GS_THETA, 0, iteration))) return rc;
  /* the first tau proposal touches no locus: its stage rides in the launch of the stages before it, ahead of the
   * per-locus touch-ups of the accepted theta / migration-rate proposals */
  if (Gh.Kc < Gh.K && (rc = run_stage(e, GS_TAU_PROPOSE, Gh.Kc, iteration))) return rc;
  if ((rc = apply_list(e))) return rc;
  if ((rc = part_tau(e, iteration, true))) return rc;
  if ((rc = part_sage(e, iteration))) return rc;
  if (Gh.doMixing && (rc = part_mix(e, iteration))) return rc;
  if ((rc = finish_owed(e))) return rc;    /* no evaluate kernel followed the last decision */
  if ((iteration == Gh.startMig || (iteration + 1) % Gh.samplesPerLog == 0) && (rc = mix_finish_owed(e))) return rc;   /* the refresh / checkAll pass reads the pages */
  if (iteration == Gh.startMig) {
    // sampleMigRates, then the genLogLikelihood refresh of every locus (GPhoCS.c:1738-1757) inside synchronizeEvents' pass
    if ((rc = run_stage(e, GS_STARTMIG, 0, iteration))) return rc;
    if ((rc = part_refresh(e, iteration))) return rc;
  } else {
    e->sync_pending = true;   /* synchronizeEvents (GPhoCS.c:1705-1714): at the head of the next sweep kernel */
  }
  if ((iteration + 1) % Gh.samplesPerLog == 0 && (rc = part_check(e, iteration))) return rc;
  return finish_sync(e);
}

// ONE part of an iteration, its result on the host when this returns: what a caller that keeps the reference's own
// performMCMC runs behind each of the functions of GPhoCS.h:84-100 (gph_mcmc_update_* below; the caller has set the
// step size(s) of the part in the chain state and, for GPH_PART_REFRESH, the freshly sampled migration rates)
int gph_engine_part_(gph_engine *e, int32_t part, int32_t iteration, const double *lr_alpha_finetune, int64_t *lr_accepted, double *lr_rateVar)
{
  if (!e || !e->initialized) return GPH_ESTATE;
  SETDEV(e);
  int rc = 0;
  GphGlobal &Gh = *e->G_h;
  rng_ahead_dirty(e);      /* (the stepwise driver: every pass in front of its sweep) */
  if ((rc = push_if_dirty(e))) return rc;
  if (part != GPH_PART_SWEEP && part != GPH_PART_SYNC) { int rcm = mix_finish_owed(e); if (rcm) return rcm; }
  if (part == GPH_PART_LRATE || part == GPH_PART_TAU || part == GPH_PART_SAGE || part == GPH_PART_MIX) {
    int rcs = flush_sync(e, true);    /* a deferred synchronizeEvents pass must not be overtaken by a kernel that edits the pages */
    if (rcs) return rcs;
  }
  switch (part) {
  case GPH_PART_SWEEP: rc = part_sweep(e, iteration, Gh.ftCoalTime, Gh.ftMigTime); break;
  case GPH_PART_LRATE: rc = lr_alpha_finetune ? part_lrate(e, iteration, lr_alpha_finetune, lr_accepted, lr_rateVar) : GPH_EARG; break;
  case GPH_PART_THETA: rc = run_stage(e, GS_THETA_ONLY, 0, iteration); if (!rc) rc = apply_list(e); break;
  case GPH_PART_MIGR: rc = run_stage(e, GS_MIGR_ONLY, 0, iteration); if (!rc) rc = apply_list(e); break;
  case GPH_PART_TAU: rc = part_tau(e, iteration, false); break;
  case GPH_PART_SAGE: rc = part_sage(e, iteration); break;
  case GPH_PART_MIX: rc = part_mix(e, iteration); break;
  case GPH_PART_SYNC: e->sync_pending = true; break;
  case GPH_PART_REFRESH: e->sync_pending = false; rc = part_refresh(e, iteration); break;
  case GPH_PART_CHECK: Gh.nrec = 0; e->G_dirty = true; rc = push_if_dirty(e); if (!rc) rc = part_check(e, iteration); break;
  default: return GPH_EARG;
  }
  if (rc) return rc;
  if ((rc = finish_owed(e))) return rc;
  if (part != GPH_PART_MIX && (rc = mix_finish_owed(e))) return rc;    /* (after GPH_PART_MIX the commit may wait for GPH_PART_SWEEP) */
  return finish_sync(e);
}

// kernel-level fixtures (gph_kernels.h: kb_unit): single calls of the per-locus functions on the current chain state,
// every call undone.  out: [local loci][stride] doubles in input order, stride >= 3 (n - 1).
//   op 0: per internal node tnew, lnLd, dprior;  op 1: full recompute value;  op 2: rubber band (pre) of ancestral
//   population `arg`: delta, n0, n1, lik -- the proposal (bounds, factors) is derived from the model exactly as
//   oracle/ref_harness.c `unit` derives it;  ops 3-6 (ref_harness.c `unit2`): executeGenSPR of node arg onto a fixed list
//   of branches (stride >= 1 + 5 N: calls, then target, age, return code, value, root per call), scaleAllNodeAges by
//   1 + arg / 1000 + revert + full recompute (delta, value), rubberBandRipple do / undo (moved events, two deltas),
//   traceLineage(arg, 0 / 1) + evaluation (stride >= 13: 1, res, target, father's new population, old / new migration
//   events, both prior deltas, father's new age, data delta, generator state);  op 7 (`unit2` H): rubberBandRipple do / undo over
//   the MIG_BAND_START / MIG_BAND_END events of every band (UpdateTau's start_or_end list): moved events, two deltas
int gph_engine_unit(gph_engine *e, int32_t op, int32_t arg, double *out, int32_t stride)
{
  if (!e || !e->initialized || !out || op < 0 || op > 8 || stride < 3 * (e->cfg.n - 1) || stride < 4) return GPH_EARG;
  if ((op == 3 && stride < 1 + 5 * (2 * e->cfg.n - 1)) || (op == 6 && stride < 13)) return GPH_EARG;
  if ((op == 3 || op == 6) && (arg < 0 || arg >= 2 * e->cfg.n - 1)) return GPH_EARG;
  if (op == 8 && (arg < 0 || arg > 100000)) return GPH_EARG;      /* (the checked build's self-test: arg = a node index, possibly out of range) */
  SETDEV(e);
  rng_ahead_dirty(e);
  { int rcs = flush_sync(e, true); if (!rcs) rcs = finish_sync(e); if (rcs) return rcs; }
  if (op == 2) {
    if (arg < e->cfg.Kc || arg >= e->cfg.K) return GPH_EARG;
    GphGlobal &G = *e->G_h;
    const GphModel &M = G.model;
    GphTauArgs &A = G.tau;
    memset(&A, 0, sizeof A);
    const int ap = arg, s0 = M.popSon0[ap], s1 = M.popSon1[ap], isRoot = ap == e->cfg.rootPop;
    const double tauold = M.popAge[ap];
    double taub0 = gg_max2(M.popAge[s0], M.popAge[s1]);
    taub0 = gg_max2(taub0, M.sampleAge[s0]);
    taub0 = gg_max2(taub0, M.sampleAge[s1]);
    const double taub1 = isRoot ? GG_OLDAGE : M.popAge[M.popFather[ap]];
    const double taunew = taub0 + 0.55 * (gg_min2(taub1, tauold * 1.4) - taub0);
    A.ap = ap; A.son0 = s0; A.son1 = s1; A.isRoot = isRoot;
    A.tauold = tauold; A.taunew = taunew; A.taub0 = taub0; A.taub1 = taub1;
    A.taufactor0 = (taunew - taub0) / (tauold - taub0);
    A.taufactor1 = isRoot ? A.taufactor0 : (taunew - taub1) / (tauold - taub1);
    e->G_dirty = true;
  }
  { int rcp = push_if_dirty(e); if (rcp) return rcp; }
  double *d_out = nullptr;
  const size_t bytes = sizeof(double) * (size_t)stride * e->L;
  if (dev_alloc((void **)&d_out, bytes)) return GPH_EHIP;
  int rc = acc_zero(e, d_out, bytes);
  if (!rc) rc = launch_loci(e, 12, k_unit, op, arg, d_out, stride);
  if (!rc) rc = reduce_local(e, 0, GPH_OUT_SLOTS);
  if (!rc) rc = run_stage_now(e, GS_COUNT_ONLY, 12);
  if (!rc) rc = d2h(e, out, d_out, bytes);
  dev_free(d_out);
  return rc;
}

// the last fatal error a call returned GPH_EKERNEL for: the reference's "Fatal Error NNNN" code and the global index of the
// first locus that reported it (-1: not attributable to one locus, e.g. checkAll's accumulator test); 0 / -1 if none
int gph_engine_last_error(gph_engine *e, int64_t *locus, int32_t *code)
{
  if (!e) return GPH_EARG;
  if (locus) *locus = e->last_error_locus;
  if (code) *code = e->last_error_code;
  return 0;
}

const char *gph_engine_last_error_text(gph_engine *e) { return e ? e->last_error_text : ""; }

// tests only: break the event chain of population `pop` of one locus (the `next` link of its first event becomes -1), so
// that the next kernel's bounded chain walks raise a fatal code for exactly that locus (tests/test_host_logic.py,
// tests/test_gpu_parity.py: the failure must name the locus and print its genealogy)
int gph_engine_debug_break_chain(gph_engine *e, int64_t global_locus, int32_t pop)
{
  if (!e || !e->initialized || pop < 0 || pop >= e->cfg.K) return GPH_EARG;
  SETDEV(e);
  /* (several ranks: EVERY rank calls this -- a deferred synchronizeEvents pass runs here, with its exchange; the rank that
   * does not hold the locus returns GPH_EARG after it) */
  { int rcs = flush_sync(e, true); if (!rcs) rcs = finish_sync(e); if (rcs) return rcs; }
  const long long lo = global_locus - e->cfg.locus_begin;
  if (lo < 0 || lo >= e->L) return GPH_EARG;
  int64_t slot = -1;
  for (int64_t j = 0; j < e->L; j++) if (e->h_orig[j] == lo) { slot = j; break; }
  if (slot < 0) return GPH_ESTATE;
  const GphLayout &y = e->lay;
  std::vector<char> pg(y.page_bytes);
  char *dp = (char *)e->dev.pages + (size_t)slot * y.page_bytes;
  int rc = d2h(e, pg.data(), dp, y.page_bytes);
  if (rc) return rc;
  const int16_t *first = (const int16_t *)(pg.data() + y.o_first);
  GphEv *evr = (GphEv *)(pg.data() + y.o_ev);
  if (first[pop] < 0) return GPH_ESTATE;
  evr[first[pop]].next = -1;
  return h2d(e, dp, pg.data(), y.page_bytes);
}

// tests only: the CHECKED build's first out-of-range index (gph_rt.h: GPH_BOUNDS): source line + 100000 x file (1 gph_locus.h,
// 2 gph_kernels.h), 8000xx the typed accessors of the image, 9000xx those of the dynamic LDS; 0 = none so far.  *checked = 0 in
// a build without the checks (every product library).
int gph_engine_debug_oob(gph_engine *e, int32_t *where, int32_t *checked)
{
  if (!e || !where || !checked) return GPH_EARG;
  *where = 0;
#ifndef GPH_BOUNDS
  *checked = 0;
  return 0;
#else
  *checked = 1;
  SETDEV(e);
  if (e->initialized) { int rcs = flush_sync(e, true); if (!rcs) rcs = finish_sync(e); if (rcs) return rcs; }
  /* read and clear: the word belongs to the library (every engine of the process), a report must not be seen twice */
  return oob_take(where);
#endif
}

#if defined(GPH_HOSTEMU) && defined(GPH_EMU64)
// tests only (the wave64 host build): micro-waves started and rendezvous passed by the calling thread so far
int gph_debug_emu64_stats(long long *waves, long long *rendezvous)
{
  if (waves) *waves = gph_emu::tw.waves_total;
  if (rendezvous) *rendezvous = gph_emu::tw.rendezvous_total;
  return gph_emu::g_enabled;
}
#endif

// canonical text dump (same format as oracle/gphocs_oracle_io.c go_dump_state's per-locus part)
int gph_engine_dump_loci(gph_engine *e, const char *path, int32_t withCond, int32_t append)
{
  if (!e || !e->initialized || !path) return GPH_ESTATE;
  SETDEV(e);
  { int rcs = flush_sync(e, true); if (!rcs) rcs = finish_sync(e); if (rcs) return rcs; }
  const GphLayout &y = e->lay;
  std::vector<char> pages(e->pages_bytes), cond(withCond ? e->cond_bytes : 0);
  int rc = d2h(e, pages.data(), e->dev.pages, e->pages_bytes);
  if (!rc && withCond) rc = d2h(e, cond.data(), e->dev.cond, e->cond_bytes);
  if (rc) return rc;
  FILE *f = fopen(path, append ? "a" : "w");
  if (!f) return GPH_EARG;
  std::vector<int32_t> slot_of(e->L);
  for (int64_t j = 0; j < e->L; j++) slot_of[e->h_orig[j]] = (int32_t)j;
  /* GPH_DUMP_STRIDE=k: every k-th locus (global index) only -- full-size parity runs */
  const int dstride = getenv("GPH_DUMP_STRIDE") && atoi(getenv("GPH_DUMP_STRIDE")) > 0 ? atoi(getenv("GPH_DUMP_STRIDE")) : 1;
  for (int64_t go = 0; go < e->L; go++) {
    if ((go + e->cfg.locus_begin) % dstride != 0) continue;
    const int64_t g = slot_of[go];
    dump_one_locus(e, f, go + e->cfg.locus_begin, pages.data() + (size_t)g * y.page_bytes, withCond ? cond.data() + e->h_cond_off[g] : nullptr, e->h_P[g]);
  }
  fclose(f);
  return 0;
}

// ---- the statistics samplers: one scaffold under nine features
//   sample_settle, sample_run   what every _sample function does around its launches: the state settled, the row taken, what is
//                               pending flushed, the timing events, the counters
//   SmRows, SmParts             the row buffer and the chunked partials (coal stats, time slices)
//   SmSel, SmSelected           a selection of loci, and the state of a sampler over one: selected_out, selected_free,
//                               selected_on / selected_zero (zeroing itself stays each sampler's own step), over_limit
//   rows_iters_fetch            the rows taken since the last fetch with their iterations
//   leaf_pops                   the leaf -> current population bytes two kernels read
// A sample reads the current state from the device, so whatever is still owed to it runs first; how much depends on what
// the sampler's kernels read.  A deferred synchronizeEvents pass STAYS deferred at every level: it corrects event times only
// (the one sampler that reads them applies the pass's arithmetic itself: vsync, gph_timeslices.h).
//   SETTLE_PAGES (summary, coal stats: node records and per-page scalars).  The commit of an accepted mixing proposal still
//     owed to the next sweep kernel changes the pages, so it runs now (k_mix_finish) -- unless the proposal was rejected (the
//     host mirror of the chain state, current after an iteration, says so): then there is nothing to commit, as part_sweep
//     finds too.
//   SETTLE_PAGES_AND_AGES (ancestry: the migration ages too).  First the commit / revert of a decided tau or sample-age
//     proposal still owed to the next evaluate kernel (k_tau_finish: one more launch; never owed after a whole
//     gph_engine_iteration_, only between the parts of a stepwise caller).
//   SETTLE_CHAIN (time slices: event times and the model in the chain state).  Before both, a host-side change of the chain
//     state is pushed.
enum { SETTLE_PAGES, SETTLE_PAGES_AND_AGES, SETTLE_CHAIN };
static int sample_settle(gph_engine *e, int level)
{
  if (level == SETTLE_CHAIN) { int rcp = push_if_dirty(e); if (rcp) return rcp; }
  if (level != SETTLE_PAGES) { int rcw = finish_owed(e); if (rcw) return rcw; }
  if (e->mix_owed && e->mirror_current && !e->G_h->mix_flag) e->mix_owed = false;
  return mix_finish_owed(e);
}

// the launch bookkeeping of one sample, k launches of timing class cls queued on the engine's stream between the two:
// what is pending on the stream goes first, HIP events bracket the launches (tms: their slot); what is counted: gph_backend.h
static int sample_begin(gph_engine *e, int cls, int &tms)
{
  tms = -1;
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  tms = tm_begin(e, cls);
  return 0;
}
static void sample_end(gph_engine *e, int cls, int k, int tms)
{
  tm_end(e, tms);
  flat_launched(e, cls, k);
  e->cls_launches[cls] += 1;
}

static void *rows_next(const SmRows &b) { return b.d + b.esz * (size_t)b.n * b.fill; }
// what a sample leaves behind: a row of `rows` (zero: set to 0 first, outside the timing events), its iteration, one more sample
struct SmTaken {
  SmRows *rows = nullptr;
  bool zero = false;
  std::vector<int32_t> *iters = nullptr;
  int32_t iteration = 0;
  int64_t *samples = nullptr;
};
// one sample of a sampler that is on: the state settled to `level`, then k launches of timing class cls -- launch(row) queues
// them; k == 0: a rank with nothing to launch, which takes its (empty or zero) row all the same -- then what the sample leaves
extern "C++" { template <class Launch> static int sample_run(gph_engine *e, int level, int cls, int k, const SmTaken &t, Launch launch)
{
  if (t.rows && t.rows->fill >= t.rows->cap) return GPH_EFULL;
  SETDEV(e);
  { int rcs = sample_settle(e, level); if (rcs) return rcs; }
  void *row = t.rows ? rows_next(*t.rows) : nullptr;
  if (t.zero) { int rcz = acc_zero(e, row, t.rows->esz * (size_t)t.rows->n); if (rcz) return rcz; }
  if (k > 0) {
    int tms;
    { int rcb = sample_begin(e, cls, tms); if (rcb) return rcb; }
    { int rcl = launch(row); if (rcl) return rcl; }
    sample_end(e, cls, k, tms);
  }
  if (t.iters) t.iters->push_back(t.iteration);
  if (t.rows) t.rows->fill++;
  if (t.samples) ++*t.samples;
  return 0;
} }

static void rows_free(SmRows &b) { dev_free(b.d); b = SmRows{}; }
static int rows_alloc(SmRows &b, size_t esz, int32_t n, int32_t cap)
{
  if (dev_alloc((void **)&b.d, esz * (size_t)n * cap)) { b.d = nullptr; return GPH_EHIP; }
  b.esz = esz; b.n = n; b.cap = cap; b.fill = 0;
  return 0;
}
// every row taken since the last fetch into out, contiguous, and the buffer empty again
static int rows_fetch(gph_engine *e, SmRows &b, void *out, int32_t *rows)
{
  *rows = b.fill;
  if (b.fill > 0) { int rc = d2h(e, out, b.d, b.esz * (size_t)b.n * b.fill); if (rc) return rc; }
  b.fill = 0;
  return 0;
}
// the same with the rows' iterations (`its`, emptied too), behind an entry point's own checks of its arguments: out[rows][ld]
// elements, ld 0: the rows packed, copied straight into out (the ABI has no ld).  counted: the copy is the call's host synchronisation as the
// counters see it (pull_rows) or the plain copy of rows_fetch -- the entry points differ in that, and keep differing
static int rows_iters_fetch(gph_engine *e, SmRows &b, std::vector<int32_t> &its, int32_t *iters, void *out, int64_t ld, bool counted, int32_t *rows)
{
  SETDEV(e);
  const size_t row = b.esz * (size_t)b.n, held = (size_t)b.fill;
  if (held > 0 && row > 0) {       /* (rows without records: nothing to copy) */
    std::vector<char> tmp(ld ? row * held : 0);
    void *to = ld ? (void *)tmp.data() : out;
    int rc = counted ? pull_rows(e, to, b.d, row * held) : d2h(e, to, b.d, row * held);
    if (rc) return rc;
    for (size_t r = 0; ld && r < held; r++) memcpy((char *)out + r * (size_t)ld * b.esz, tmp.data() + r * row, row);
  }
  for (size_t r = 0; r < held; r++) iters[r] = its[r];
  *rows = b.fill;
  b.fill = 0;
  its.clear();
  return 0;
}

static void parts_free(SmParts &p) { dev_free(p.d_part); p.d_part = nullptr; p.rd = p.chunk = p.nchunks = 0; }
static int parts_alloc(gph_engine *e, SmParts &p, int32_t rd, int32_t default_chunk)
{
  const int chunk = p.chunk_next > 0 ? p.chunk_next : default_chunk;
  const int nchunks = (int)((e->L + chunk - 1) / chunk);
  if (dev_alloc((void **)&p.d_part, sizeof(double) * (size_t)rd * nchunks)) { p.d_part = nullptr; return GPH_EHIP; }
  p.rd = rd; p.chunk = chunk; p.nchunks = nchunks;
  return 0;
}
// the partial rows of a sample into its row, in chunk order (one launch)
static int parts_fold(gph_engine *e, const SmParts &p, int32_t iteration, double *row)
{
  return launch_grid(e, GphGrid{(p.rd + GPH_FOLD_THREADS - 1) / GPH_FOLD_THREADS, 1}, GPH_FOLD_THREADS, 0, k_rows_fold,
                     p.d_part, p.nchunks, p.rd, iteration, row);
}
// a chunked sampler's two buffers: partial rows for its L slots, `capacity` rows of rd doubles
static int chunked_alloc(gph_engine *e, SmParts &p, SmRows &b, int32_t rd, int32_t default_chunk, int32_t capacity)
{
  if (parts_alloc(e, p, rd, default_chunk)) return GPH_EHIP;
  if (rows_alloc(b, sizeof(double), rd, capacity)) { parts_free(p); return GPH_EHIP; }
  return 0;
}
// a caller's selection of loci: nothing (null: every locus) or global indices, strictly increasing
static bool sel_valid(const int64_t *loci, int64_t nloci)
{
  if (loci && nloci < 0) return false;
  if (loci)
    for (int64_t k = 0; k < nloci; k++)
      if (loci[k] < 0 || (k > 0 && loci[k] <= loci[k - 1])) return false;
  return true;
}
static void sel_free(SmSel &s) { dev_free(s.d_slot); s = SmSel{}; }
// the loci of the selection that this rank holds, and their slots in HBM: slots are sorted by decreasing pattern count, h_orig[j]
// is the local locus slot j holds
static int sel_alloc(gph_engine *e, SmSel &s, const int64_t *loci, int64_t nloci)
{
  const int64_t L = e->L, lb = e->cfg.locus_begin;
  if (!loci) for (int64_t g = 0; g < L; g++) s.loci.push_back(lb + g);
  else for (int64_t k = 0; k < nloci; k++) if (loci[k] >= lb && loci[k] < lb + L) s.loci.push_back(loci[k]);
  std::vector<int32_t> slot_of((size_t)L), slot(s.loci.size());
  for (int64_t j = 0; j < L; j++) slot_of[(size_t)e->h_orig[j]] = (int32_t)j;
  for (size_t q = 0; q < slot.size(); q++) slot[q] = slot_of[(size_t)(s.loci[q] - lb)];
  int rc = dev_alloc((void **)&s.d_slot, sizeof(int32_t) * slot.size());
  if (rc) s.d_slot = nullptr;
  else if (!slot.empty()) rc = h2d(e, s.d_slot, slot.data(), sizeof(int32_t) * slot.size());
  if (rc) sel_free(s);
  return rc;
}
// the selected loci of this rank into out (count alone with out == null)
static int sel_copy_out(const SmSel &s, int64_t *out, int64_t max_loci, int64_t *count)
{
  *count = (int64_t)s.loci.size();
  if (max_loci < *count) return out ? GPH_EARG : 0;
  for (size_t q = 0; q < s.loci.size(); q++) out[q] = s.loci[q];
  return 0;
}
// gph_engine_*_selected: the selected loci of this rank of a sampler that is on (s null with e)
static int selected_out(const gph_engine *e, const SmSelected *s, int64_t *out, int64_t max_loci, int64_t *count)
{
  if (!e || !count || max_loci < 0 || (!out && max_loci > 0)) return GPH_EARG;
  if (!s->on) return GPH_ESTATE;
  return sel_copy_out(s->sel, out, max_loci, count);
}
// off, everything on the device released (more: a sampler's further blocks) and every member as in a fresh engine
extern "C++" { template <class S> static void selected_free(S &s, std::initializer_list<void *> more = {})
{
  dev_free(s.d);
  for (void *p : more) dev_free(p);
  rows_free(s.rows);
  sel_free(s.sel);
  s = S{};
} }
// the accumulators of a sampler back to zero, the sample count with them; and the end of an _enable: on, zeroed by `zero`
static int selected_zero(gph_engine *e, SmSelected &s)
{
  if (!s.on) return 0;
  s.samples = 0;
  return s.zero(e);
}
static int selected_on(gph_engine *e, SmSelected &s, int (*zero)(gph_engine *))
{
  s.on = true;
  s.zero = zero;
  return selected_zero(e, s);
}
// the byte limit of a sampler's device memory, the caller's or 1 GiB: whether `need` exceeds it, then said on stderr as
// "gphocs_hip: <what> need <need> bytes (<detail>), the limit is <limit>"
__attribute__((format(printf, 4, 5))) static bool over_limit(int64_t need, int64_t max_bytes, const char *what, const char *detail, ...)
{
  const int64_t limit = max_bytes > 0 ? max_bytes : (int64_t)1 << 30;
  if (need <= limit) return false;
  char text[256];
  va_list ap;
  va_start(ap, detail);
  vsnprintf(text, sizeof text, detail, ap);
  va_end(ap);
  fprintf(stderr, "gphocs_hip: %s need %lld bytes (%s), the limit is %lld\n", what, (long long)need, text, (long long)limit);
  return true;
}
// leaf -> current population, one byte a leaf (leaves stand in population order), behind it with_counts ? the samples of each
// population : nothing; padded to 16 bytes
static std::vector<uint8_t> leaf_pops(const gph_engine *e, bool with_counts)
{
  const int n = e->cfg.n, Kc = e->cfg.Kc;
  std::vector<uint8_t> pop(((size_t)n + (with_counts ? Kc : 0) + 15) & ~(size_t)15, 0);
  for (int p = 0, i = 0; p < Kc; p++) {
    for (int k = 0; k < e->samplesPerPop[p] && i < n; k++) pop[(size_t)i++] = (uint8_t)p;
    if (with_counts) pop[(size_t)n + p] = (uint8_t)e->samplesPerPop[p];
  }
  return pop;
}
// per-locus accumulators [L][ncol] in slot order -> out, row h_orig[j] (the local locus slot j holds) of leading dimension ld
static int fetch_by_locus(gph_engine *e, const double *d_acc, int ncol, bool column_major, double *out, int64_t ld)
{
  const int64_t L = e->L;
  std::vector<double> acc((size_t)ncol * L);
  int rc = d2h(e, acc.data(), d_acc, sizeof(double) * acc.size());
  if (rc) return rc;
  for (int64_t j = 0; j < L; j++) {
    double *row = out + (size_t)e->h_orig[j] * ld;
    for (int c = 0; c < ncol; c++) row[c] = column_major ? acc[(size_t)c * L + j] : acc[(size_t)j * ncol + c];
  }
  return 0;
}

// ---- per-locus posterior summaries (gph_summary.h)
int gph_engine_locus_summary_enable(gph_engine *e, int32_t on)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  SETDEV(e);
  dev_free(e->ls.d);
  e->ls = {};
  if (!on) return 0;
  const int K = e->cfg.K, B = e->cfg.B, var = e->var_rates;
  const int ncol = gph_ls_columns(K, B, var);
  if (dev_alloc((void **)&e->ls.d, sizeof(double) * (size_t)ncol * e->L)) { e->ls.d = nullptr; return GPH_EHIP; }
  e->ls.ncol = ncol;
  for (const char *q : {"dataLnL", "genLnL", "tmrca"})
    for (const char *m : {".shift", ".s1", ".s2"}) e->ls.names.push_back(std::string(q) + m);
  for (int b = 0; b < B; b++) e->ls.names.push_back("nmig." + std::to_string(b));
  for (int b = 0; b < B; b++) e->ls.names.push_back("pmig." + std::to_string(b));
  for (int p = 0; p < K; p++) e->ls.names.push_back("ncoal." + std::to_string(p));
  if (var) for (const char *m : {".shift", ".s1", ".s2"}) e->ls.names.push_back(std::string("rate") + m);
  return acc_zero(e, e->ls.d, sizeof(double) * (size_t)ncol * e->L);
}

// one sample of the current state, queued on the engine's stream
int gph_engine_locus_summary_sample(gph_engine *e)
{
  if (!e || !e->initialized || !e->ls.d) return GPH_ESTATE;
  const int first = e->ls.samples == 0;
  const int L = (int)e->L, ncol = e->ls.ncol, var = e->var_rates;
  SmTaken t;
  t.samples = &e->ls.samples;
  return sample_run(e, SETTLE_PAGES, 13, 1, t, [&](void *) {
    return launch_grid(e, GphGrid{(L + GPH_LS_THREADS - 1) / GPH_LS_THREADS, 1}, GPH_LS_THREADS, 0, k_locus_summary,
                       e->lay, e->dev.pages, e->ls.d, L, ncol, first, var);
  });
}

int gph_engine_locus_summary_columns(gph_engine *e, int32_t *ncol, int64_t *samples)
{
  if (!e) return GPH_EARG;
  if (ncol) *ncol = e->ls.ncol;
  if (samples) *samples = e->ls.samples;
  return 0;
}

int gph_engine_locus_summary_fetch(gph_engine *e, double *out, int64_t ld, int32_t reset)
{
  if (!e || !out) return GPH_EARG;
  if (!e->ls.d) return GPH_ESTATE;
  if (ld < e->ls.ncol) return GPH_EARG;
  SETDEV(e);
  int rc = fetch_by_locus(e, e->ls.d, e->ls.ncol, true, out, ld);
  if (rc || !reset) return rc;
  e->ls.samples = 0;
  return acc_zero(e, e->ls.d, sizeof(double) * (size_t)e->ls.ncol * e->L);
}

const char *gph_engine_locus_summary_column_name(gph_engine *e, int32_t col)
{
  if (!e || col < 0 || col >= (int32_t)e->ls.names.size()) return nullptr;
  return e->ls.names[col].c_str();
}

// ---- genome-wide coalescent and sample-pair statistics per sample (gph_coalstats.h)
int gph_engine_coal_stats_enable(gph_engine *e, int32_t capacity)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity < 0) return GPH_EARG;
  SETDEV(e);
  parts_free(e->cs.part);
  rows_free(e->cs.rows);
  e->cs.bd = 0;
  if (capacity == 0) return 0;
  const int n = e->cfg.n, K = e->cfg.K;
  if (chunked_alloc(e, e->cs.part, e->cs.rows, gph_cs_row_doubles(n, K), GPH_CS_CHUNK, capacity)) return GPH_EHIP;
  e->cs.bd = gph_cs_block(n, K);
  return 0;
}

// tests: the slots per chunk the next _enable uses (0: the default), so that a data set of a few loci runs the fold over
// several partial rows.  The chunk size is part of the summation order: it changes the last bits of the fp64 sums
int gph_engine_coal_stats_set_chunk(gph_engine *e, int32_t slots)
{
  if (!e || slots < 0) return GPH_EARG;
  e->cs.part.chunk_next = slots;
  return 0;
}

// one sample of the current state into the next free row, queued on the engine's stream
int gph_engine_coal_stats_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->cs.rows.d) return GPH_ESTATE;
  const SmParts &p = e->cs.part;
  const int L = (int)e->L, n = e->cfg.n, K = e->cfg.K, B = e->cfg.B, bd = e->cs.bd;
  const int ntiles = (gph_cs_pairs(n) + bd - 1) / bd;
  SmTaken t;
  t.rows = &e->cs.rows;
  return sample_run(e, SETTLE_PAGES, 14, 2, t, [&](void *row) {
    int rcl = launch_grid(e, GphGrid{p.nchunks, ntiles}, bd, gph_cs_lds_bytes(n, K, B, bd), k_coal_stats,
                          e->lay, e->dev.pages, p.d_part, L, p.chunk);
    return rcl ? rcl : parts_fold(e, p, iteration, (double *)row);
  });
}

int gph_engine_coal_stats_shape(gph_engine *e, int32_t *row_doubles, int32_t *filled, int32_t *n, int32_t *K)
{
  if (!e) return GPH_EARG;
  if (row_doubles) *row_doubles = e->cs.rows.n;
  if (filled) *filled = e->cs.rows.fill;
  if (n) *n = e->cfg.n;
  if (K) *K = e->cfg.K;
  return 0;
}

int gph_engine_coal_stats_fetch(gph_engine *e, double *out, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || (!out && max_rows > 0)) return GPH_EARG;
  if (!e->cs.rows.d) return GPH_ESTATE;
  if (max_rows < e->cs.rows.fill) return GPH_EARG;
  SETDEV(e);
  return rows_fetch(e, e->cs.rows, out, rows);
}

const char *gph_engine_coal_stats_column_name(gph_engine *e, int32_t col)
{
  static const char *fixed[CS_FIXED] = {"iter", "coalStat", "numCoal", "migStat", "numMig", "genLnL", "dataLnL"};
  if (!e || col < 0) return nullptr;
  if (col < CS_FIXED) return fixed[col];
  const int n = e->cfg.n, K = e->cfg.K, npk = gph_cs_pairs(n) * K;
  if (K < 1 || col >= CS_FIXED + 3 * npk) return nullptr;
  const int block = (col - CS_FIXED) / npk, q = (col - CS_FIXED) % npk;
  int i = 0, p = q / K;
  while (i < n - 2 && p >= n - 1 - i) { p -= n - 1 - i; i++; }
  e->cs.name = std::string(block == 0 ? "cnt." : block == 1 ? "first." : "agesum.") + std::to_string(i) + "." + std::to_string(i + 1 + p) + "." + std::to_string(q % K);
  return e->cs.name.c_str();
}

// ---- coalescence and migration statistics per time slice, per sample (gph_timeslices.h)
int gph_engine_time_slices_enable(gph_engine *e, int32_t slices, int32_t capacity)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity < 0) return GPH_EARG;
  SETDEV(e);
  parts_free(e->ts.part);
  rows_free(e->ts.rows);
  e->ts.shape = GphTsShape{};
  if (capacity == 0) return 0;
  GphTsShape h;
  if (gph_ts_shape(e->lay, slices, h)) {
    fprintf(stderr, "gphocs_hip: time slices: %d slices requested, 1 to %d are supported\n", (int)slices, GPH_TS_MAXS);
    return GPH_EARG;
  }
  if (h.lds_bytes > 65536) {
    fprintf(stderr, "gphocs_hip: time slices: %d slices need %d bytes of LDS a workgroup, 65536 at most\n", (int)slices, (int)h.lds_bytes);
    return GPH_EARG;
  }
  /* (every cell of a partial row is written by its chunk's workgroups, the root's zero slices included) */
  if (chunked_alloc(e, e->ts.part, e->ts.rows, gph_ts_row_doubles(e->cfg.K, e->cfg.B, slices), GPH_TS_CHUNK, capacity)) return GPH_EHIP;
  e->ts.shape = h;
  return 0;
}

// tests: the slots per chunk the next _enable uses (0: the default).  The chunk size is part of the summation order
int gph_engine_time_slices_set_chunk(gph_engine *e, int32_t slots)
{
  if (!e || slots < 0) return GPH_EARG;
  e->ts.part.chunk_next = slots;
  return 0;
}

// one sample of the current state into the next free row, queued on the engine's stream.  A deferred synchronizeEvents pass
// stays deferred: the walkers apply its arithmetic to the event times they read (vsync), so the row is that of the chain as
// the pass will leave it
int gph_engine_time_slices_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->ts.rows.d) return GPH_ESTATE;
  const SmParts &p = e->ts.part;
  const GphTsShape &h = e->ts.shape;
  SmTaken t;
  t.rows = &e->ts.rows;
  return sample_run(e, SETTLE_CHAIN, 15, 2, t, [&](void *row) {
    const int L = (int)e->L, vsync = e->sync_pending ? 1 : 0;       /* (read behind the settling) */
    int rcl = launch_grid(e, GphGrid{p.nchunks, h.ntiles}, h.bd, (size_t)h.lds_bytes, k_time_slices,
                          e->lay, h, e->G_d, e->dev.pages, p.d_part, L, p.chunk, p.rd, vsync);
    return rcl ? rcl : parts_fold(e, p, iteration, (double *)row);
  });
}

int gph_engine_time_slices_shape(gph_engine *e, int32_t *row_doubles, int32_t *filled, int32_t *slices, int32_t *K, int32_t *B,
                                 int32_t *staged_bytes_per_locus)
{
  if (!e) return GPH_EARG;
  if (row_doubles) *row_doubles = e->ts.rows.n;
  if (filled) *filled = e->ts.rows.fill;
  if (slices) *slices = e->ts.shape.S;
  if (staged_bytes_per_locus) *staged_bytes_per_locus = e->ts.shape.img.bytes;
  if (K) *K = e->cfg.K;
  if (B) *B = e->cfg.B;
  return 0;
}

int gph_engine_time_slices_fetch(gph_engine *e, double *out, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || (!out && max_rows > 0)) return GPH_EARG;
  if (!e->ts.rows.d) return GPH_ESTATE;
  if (max_rows < e->ts.rows.fill) return GPH_EARG;
  SETDEV(e);
  return rows_fetch(e, e->ts.rows, out, rows);
}

const char *gph_engine_time_slices_column_name(gph_engine *e, int32_t col)
{
  if (!e || col < 0 || col >= e->ts.rows.n) return nullptr;
  if (col == 0) return "iter";
  const int S = e->ts.shape.S, K = e->cfg.K, q = (col - 1) / 2, W = q / S, k = q % S + 1, second = (col - 1) & 1;
  const char *what = W < K ? (second ? "deltaT." : "numCoal.") : (second ? "migT." : "numMig.");
  e->ts.name = std::string(what) + std::to_string(W < K ? W : W - K) + "." + std::to_string(k);
  return e->ts.name.c_str();
}

// ---- per-locus, per-sample migration ancestry (gph_ancestry.h)
int gph_engine_ancestry_enable(gph_engine *e, int32_t capacity_rows, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0) return GPH_EARG;
  SETDEV(e);
  dev_free(e->an.d_acc);
  e->an.d_acc = nullptr;
  rows_free(e->an.rows);
  e->an.ncol = 0; e->an.samples = 0;
  e->an.iters.clear();
  e->an.shape = GphAnShape{};
  if (capacity_rows == 0) return 0;
  const int n = e->cfg.n, B = e->cfg.B;
  const int ncol = gph_an_locus_columns(n, B);
  const int64_t need = (int64_t)e->L * ncol * 8;
  if (over_limit(need, max_bytes, "ancestry: the per-locus accumulators", "%lld loci x %d leaves x %d columns x 8", (long long)e->L, n, 2 * B + 1)) return GPH_EFULL;
  if (dev_alloc((void **)&e->an.d_acc, (size_t)need)) { e->an.d_acc = nullptr; return GPH_EHIP; }
  if (rows_alloc(e->an.rows, sizeof(uint32_t), gph_an_row_ints(n, B), capacity_rows)) {
    dev_free(e->an.d_acc);
    e->an.d_acc = nullptr;
    return GPH_EHIP;
  }
  e->an.ncol = ncol;
  gph_an_shape(e->lay, e->an.shape);
  return acc_zero(e, e->an.d_acc, (size_t)need);
}

// one sample of the current state, queued on the engine's stream
int gph_engine_ancestry_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->an.rows.d) return GPH_ESTATE;
  const int L = (int)e->L;
  const GphAnShape &h = e->an.shape;
  const int groups = (L + h.G - 1) / h.G;
  const size_t row_bytes = sizeof(uint32_t) * (size_t)e->an.rows.n;
  /* (this sampler zeroes its row between the timing events, as it always did: not SmTaken's zero, which goes in front) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 16, 1, SmTaken{&e->an.rows, false, &e->an.iters, iteration, &e->an.samples}, [&](void *row) {
    int rcl = acc_zero(e, row, row_bytes);
    return rcl ? rcl : launch_grid(e, GphGrid{groups, 1}, h.bd, (size_t)h.lds_bytes, k_ancestry, e->lay, h, e->dev.pages, e->an.d_acc, (uint32_t *)row, L);
  });
}

int gph_engine_ancestry_shape(gph_engine *e, int32_t *locus_columns, int32_t *row_ints, int64_t *samples, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  if (locus_columns) *locus_columns = e->an.ncol;
  if (row_ints) *row_ints = e->an.rows.n;
  if (samples) *samples = e->an.samples;
  if (rows_held) *rows_held = e->an.rows.fill;
  return 0;
}

int gph_engine_ancestry_fetch_loci(gph_engine *e, double *out, int64_t ld, int32_t reset)
{
  if (!e || !out) return GPH_EARG;
  if (!e->an.d_acc) return GPH_ESTATE;
  if (ld < e->an.ncol) return GPH_EARG;
  SETDEV(e);
  int rc = fetch_by_locus(e, e->an.d_acc, e->an.ncol, false, out, ld);
  if (rc || !reset) return rc;
  e->an.samples = 0;
  return acc_zero(e, e->an.d_acc, sizeof(double) * (size_t)e->an.ncol * e->L);
}

int gph_engine_ancestry_fetch_rows(gph_engine *e, int32_t *iters, int32_t *out, int64_t ld, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || ((!out || !iters) && max_rows > 0)) return GPH_EARG;
  const SmRows &b = e->an.rows;
  if (!b.d) return GPH_ESTATE;
  if (max_rows < b.fill || (b.fill > 0 && ld < b.n)) return GPH_EARG;
  return rows_iters_fetch(e, e->an.rows, e->an.iters, iters, out, ld, false, rows);
}

const char *gph_engine_ancestry_column_name(gph_engine *e, int32_t which, int32_t col)
{
  if (!e || col < 0 || e->an.rows.cap == 0) return nullptr;
  const int n = e->cfg.n, B = e->cfg.B;
  if (which == 0) {
    if (col >= e->an.ncol) return nullptr;
    const int blk = col / n, i = col % n;
    e->an.name = blk >= 2 * B ? "any." + std::to_string(i)
                              : std::string(blk < B ? "cnt." : "age.") + std::to_string(blk % (B > 0 ? B : 1)) + "." + std::to_string(i);
  } else if (which == 1) {
    if (col >= e->an.rows.n) return nullptr;
    const int blk = col / n, i = col % n;
    e->an.name = blk == 0 ? "any." + std::to_string(i) : "hit." + std::to_string(blk - 1) + "." + std::to_string(i);
  } else return nullptr;
  return e->an.name.c_str();
}

// ---- sampled genealogies of selected loci (gph_genetrees.h)
static_assert((int)GT_O_COUNT == (int)GPH_GT_O_COUNT && (int)GT_O_LIVING == (int)GPH_GT_O_LIVING && GPH_MAX_MIGS == GPH_GT_MAX_MIGS && MG_COUNT == 6,
              "the record layout include/gphocs_hip.h documents");
int gph_engine_gene_trees_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || !sel_valid(loci, nloci)) return GPH_EARG;
  SETDEV(e);
  selected_free(e->gt);
  if (capacity_rows == 0) return 0;
  { int rcs = sel_alloc(e, e->gt.sel, loci, nloci); if (rcs) return rcs; }
  const int64_t nsel = (int64_t)e->gt.sel.loci.size();
  GphGtShape h;
  gph_gt_shape(e->lay, h);
  const int64_t limit = max_bytes > 0 ? max_bytes : (int64_t)256 << 20;
  const int64_t need = (int64_t)capacity_rows * nsel * h.img.bytes;
  if (need > limit) {
    fprintf(stderr, "gphocs_hip: gene trees: the row buffer needs %lld bytes (%d rows x %lld loci x %d bytes a record), the limit is %lld\n",
            (long long)need, (int)capacity_rows, (long long)nsel, (int)h.img.bytes, (long long)limit);
    sel_free(e->gt.sel);
    return GPH_EFULL;
  }
  if (rows_alloc(e->gt.rows, (size_t)h.img.bytes, (int32_t)nsel, capacity_rows)) { sel_free(e->gt.sel); return GPH_EHIP; }
  e->gt.shape = h;
  e->gt.on = true;
  return 0;
}

// one sample of the current state, queued on the engine's stream
int gph_engine_gene_trees_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->gt.on) return GPH_ESTATE;
  const GphGtShape &h = e->gt.shape;
  const int nsel = e->gt.rows.n, L = (int)e->L;
  const int groups = (nsel + h.G - 1) / h.G;
  /* (a rank without a selected locus launches nothing: a grid of no blocks is no legal launch) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 17, groups > 0, SmTaken{&e->gt.rows, false, &e->gt.iters, iteration, nullptr}, [&](void *row) {
    return launch_grid(e, GphGrid{groups, 1}, GPH_GT_THREADS, 0, k_gene_trees, e->lay, h, e->dev.pages, e->gt.sel.d_slot, nsel, L, (char *)row);
  });
}

int gph_engine_gene_trees_shape(gph_engine *e, int64_t *selected, int32_t *nodes, int32_t *record_bytes, int32_t *offsets, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  const bool on = e->gt.on;
  if (selected) *selected = on ? (int64_t)e->gt.sel.loci.size() : 0;
  if (nodes) *nodes = on ? e->lay.N : 0;
  if (record_bytes) *record_bytes = on ? e->gt.shape.img.bytes : 0;
  if (offsets) for (int k = 0; k < GT_O_COUNT; k++) offsets[k] = on ? e->gt.shape.off[k] : 0;
  if (rows_held) *rows_held = e->gt.rows.fill;
  return 0;
}

int gph_engine_gene_trees_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->gt : nullptr, out, max_loci, count); }

int gph_engine_gene_trees_fetch(gph_engine *e, int32_t *iters, void *out, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || (!iters && max_rows > 0)) return GPH_EARG;
  SmRows &b = e->gt.rows;
  if (!e->gt.on) return GPH_ESTATE;
  if (max_rows < b.fill || (!out && b.fill > 0 && b.n > 0)) return GPH_EARG;       /* (rows without records need no `out`) */
  return rows_iters_fetch(e, b, e->gt.iters, iters, out, 0, false, rows);
}

// ---- clade tables of selected loci (gph_clades.h)
static int clades_zero(gph_engine *e)
{
  { int rcz = acc_zero(e, e->cl.d, e->cl.bytes); if (rcz) return rcz; }
  return acc_zero(e, e->cl.d_hdr, sizeof(uint32_t) * 2 * e->cl.sel.loci.size());
}
static void clades_free(gph_engine *e) { selected_free(e->cl, {e->cl.d_hdr, e->cl.d_cmp}); }

int gph_engine_clades_enable(gph_engine *e, int32_t slots, const int64_t *loci, int64_t nloci, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (slots != 0 && (slots < 2 || (slots & (slots - 1)) != 0)) return GPH_EARG;
  if (!sel_valid(loci, nloci)) return GPH_EARG;
  SETDEV(e);
  clades_free(e);
  { int rcs = sel_alloc(e, e->cl.sel, loci, nloci); if (rcs) return rcs; }
  const size_t nsel = e->cl.sel.loci.size();
  GphClShape h;
  gph_cl_shape(e->lay, slots ? slots : gph_cl_default_slots(e->cfg.n), h);
  const int64_t per = (int64_t)h.P * h.ew * 8 + 8, need = (int64_t)nsel * per;
  if (over_limit(need, max_bytes, "clades: the tables", "%lld loci x (%d slots x %d words x 8 + 8)", (long long)nsel, (int)h.P, (int)h.ew)) {
    clades_free(e);
    return GPH_EFULL;
  }
  const size_t bytes = sizeof(uint64_t) * nsel * (size_t)h.P * h.ew;
  if (dev_alloc((void **)&e->cl.d, bytes) || dev_alloc((void **)&e->cl.d_hdr, sizeof(uint32_t) * 2 * nsel)) {
    dev_clear_error();
    clades_free(e);
    return GPH_EHIP;
  }
  e->cl.shape = h;
  e->cl.bytes = bytes;
  return selected_on(e, e->cl, clades_zero);
}

// one sample of the current state, queued on the engine's stream
int gph_engine_clades_sample(gph_engine *e)
{
  if (!e || !e->initialized || !e->cl.on) return GPH_ESTATE;
  const GphClShape &h = e->cl.shape;
  const int nsel = (int)e->cl.sel.loci.size(), L = (int)e->L;
  const int groups = (nsel + h.G - 1) / h.G;
  SmTaken t;
  t.samples = &e->cl.samples;
  /* (a rank without a selected locus launches nothing; one leaf has no clade) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 19, groups > 0 && e->cfg.n > 1, t, [&](void *) {
    return launch_grid(e, GphGrid{groups, 1}, GPH_CL_THREADS, (size_t)h.lds_bytes, k_clades, e->lay, h, e->dev.pages, e->cl.sel.d_slot, nsel, L,
                       e->cl.ent(), e->cl.d_hdr);
  });
}

int gph_engine_clades_shape(gph_engine *e, int64_t *selected, int32_t *slots, int32_t *words, int32_t *limit, int64_t *samples)
{
  if (!e) return GPH_EARG;
  const bool on = e->cl.on;
  if (selected) *selected = on ? (int64_t)e->cl.sel.loci.size() : 0;
  if (slots) *slots = on ? e->cl.shape.P : 0;
  if (words) *words = on ? e->cl.shape.W : 0;
  if (limit) *limit = on ? e->cl.shape.limit : 0;
  if (samples) *samples = on ? e->cl.samples : 0;
  return 0;
}

int gph_engine_clades_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->cl : nullptr, out, max_loci, count); }

int gph_engine_clades_fetch(gph_engine *e, uint64_t *entries, uint32_t *nkeys, uint32_t *dropped, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->cl.on) return GPH_ESTATE;
  const size_t nsel = e->cl.sel.loci.size();
  if (nsel > 0 && (!entries || !nkeys || !dropped)) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) {
    std::vector<uint32_t> hdr(2 * nsel);
    { int rc = d2h(e, entries, e->cl.d, e->cl.bytes); if (rc) return rc; }
    { int rc = d2h(e, hdr.data(), e->cl.d_hdr, sizeof(uint32_t) * 2 * nsel); if (rc) return rc; }
    for (size_t q = 0; q < nsel; q++) { nkeys[q] = hdr[2 * q]; dropped[q] = hdr[2 * q + 1]; }
  }
  return reset ? selected_zero(e, e->cl) : 0;
}

// ---- the clade tables of R replicate chains compared where they lie (gph_cladecmp.h); engines[0] leads: its stream runs the
// kernel, its counters count it, its host thread waits for the rows
int gph_engine_clades_compare(gph_engine *const *engines, int32_t R, double min_freq, double *rows, int64_t max_loci, int64_t *count)
{
  if (!engines || !count || R < 2 || R > GPH_CC_MAXR || max_loci < 0 || (!rows && max_loci > 0)) return GPH_EARG;
  if (!(min_freq >= 0.0 && min_freq <= 1.0)) return GPH_EARG;       /* (a NaN fails both) */
  for (int r = 0; r < R; r++) {
    if (!engines[r] || !engine_is_ours(engines[r])) return GPH_EARG;
    for (int j = 0; j < r; j++) if (engines[j] == engines[r]) return GPH_EARG;
  }
  gph_engine *e = engines[0];
  for (int r = 1; r < R; r++)
    if (engines[r]->cfg.device != e->cfg.device || engines[r]->cfg.n != e->cfg.n) return GPH_EARG;
  for (int r = 0; r < R; r++) if (!engines[r]->cl.on) return GPH_ESTATE;
  const GphClShape &h = e->cl.shape;
  for (int r = 1; r < R; r++) {
    const auto &c = engines[r]->cl;
    if (c.shape.P != h.P || c.shape.W != h.W || c.shape.ew != h.ew || c.sel.loci != e->cl.sel.loci) return GPH_EARG;
  }
  const int64_t nsel = (int64_t)e->cl.sel.loci.size();
  if (max_loci < nsel) return GPH_EARG;
  for (int r = 0; r < R; r++) if (engines[r]->cl.samples < 1) return GPH_ESTATE;
  *count = nsel;
  if (nsel == 0) return 0;           /* (a rank without a selected locus launches nothing) */
  SETDEV(e);
  if (!e->cl.d_cmp && dev_alloc((void **)&e->cl.d_cmp, sizeof(double) * GPH_CC_COLS * (size_t)nsel)) {
    dev_clear_error();
    e->cl.d_cmp = nullptr;
    return GPH_EHIP;
  }
  GphCcTables T;
  memset(&T, 0, sizeof T);
  for (int r = 0; r < R; r++) { T.ent[r] = engines[r]->cl.ent(); T.hdr[r] = engines[r]->cl.d_hdr; T.samples[r] = engines[r]->cl.samples; }
  const int groups = (int)((nsel + GPH_CC_THREADS / GPH_CC_WAVE - 1) / (GPH_CC_THREADS / GPH_CC_WAVE));
  int tms, rc;
  if ((rc = compare_order_before(engines, R))) return rc;      /* (in front of the timing events: the kernel's time, not the wait) */
  if ((rc = sample_begin(e, 20, tms))) return rc;
  if ((rc = launch_grid(e, GphGrid{groups, 1}, GPH_CC_THREADS, (size_t)gph_cc_lds_bytes(h.W), k_clades_compare, h, T, (int)R, (int)e->cfg.n, (int)nsel,
                        min_freq, e->cl.d_cmp))) return rc;
  sample_end(e, 20, 1, tms);
  if ((rc = compare_order_after(engines, R))) return rc;
  return pull_rows(e, rows, e->cl.d_cmp, sizeof(double) * GPH_CC_COLS * (size_t)nsel);
}

// ---- effective sample sizes of selected loci (gph_ess.h)
static int ess_zero(gph_engine *e) { return acc_zero(e, e->es.d, e->es.bytes); }
static void ess_free(gph_engine *e) { selected_free(e->es); }

int gph_engine_ess_enable(gph_engine *e, const int64_t *loci, int64_t nloci, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (!sel_valid(loci, nloci)) return GPH_EARG;
  SETDEV(e);
  ess_free(e);
  { int rcs = sel_alloc(e, e->es.sel, loci, nloci); if (rcs) return rcs; }
  const size_t nsel = e->es.sel.loci.size();
  GphClShape h;
  gph_cl_shape(e->lay, 2, h);            /* (G, W and the LDS bytes of the climb; there is no table) */
  const int M = e->var_rates ? 6 : 5, ni = e->cfg.n > 1 ? e->cfg.n - 1 : 0;
  const size_t o_focal = nsel * (size_t)M * GPH_ESS_WORDS * 8, o_prev = o_focal + nsel * (size_t)ni * h.W * 8, o_changes = o_prev + nsel * 8,
               bytes = o_changes + nsel * 4;
  if (over_limit((int64_t)bytes, max_bytes, "ess: the accumulators", "%lld loci x (%d series x %d doubles + %d focal keys of %d words + 12)",
                 (long long)nsel, M, GPH_ESS_WORDS, ni, (int)h.W)) {
    ess_free(e);
    return GPH_EFULL;
  }
  if (dev_alloc((void **)&e->es.d, bytes)) {
    dev_clear_error();
    e->es.d = nullptr;
    ess_free(e);
    return GPH_EHIP;
  }
  e->es.shape = h;
  e->es.M = M;
  e->es.max_bytes = max_bytes;
  e->es.o_focal = o_focal; e->es.o_prev = o_prev; e->es.o_changes = o_changes; e->es.bytes = bytes;
  return selected_on(e, e->es, ess_zero);
}

// one sample of the current state, queued on the engine's stream
int gph_engine_ess_sample(gph_engine *e)
{
  if (!e || !e->initialized || !e->es.on) return GPH_ESTATE;
  const GphClShape &h = e->es.shape;
  const int nsel = (int)e->es.sel.loci.size(), L = (int)e->L;
  const int groups = (nsel + h.G - 1) / h.G;
  SmTaken t;
  t.samples = &e->es.samples;
  /* (a rank without a selected locus launches nothing; one leaf has no clade) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 21, groups > 0 && e->cfg.n > 1, t, [&](void *) {
    return launch_grid(e, GphGrid{groups, 1}, GPH_CL_THREADS, (size_t)gph_es_lds_bytes(e->lay, h), k_ess, e->lay, h, e->dev.pages,
                       e->es.sel.d_slot, nsel, L, (int)e->es.M, (long long)e->es.samples, (double *)e->es.d,
                       (uint64_t *)(e->es.d + e->es.o_focal), (uint64_t *)(e->es.d + e->es.o_prev), (uint32_t *)(e->es.d + e->es.o_changes));
  });
}

int gph_engine_ess_shape(gph_engine *e, int64_t *selected, int32_t *series, int32_t *levels, int32_t *words, int64_t *samples)
{
  if (!e) return GPH_EARG;
  const bool on = e->es.on;
  if (selected) *selected = on ? (int64_t)e->es.sel.loci.size() : 0;
  if (series) *series = on ? e->es.M : 0;
  if (levels) *levels = on ? GPH_ESS_LEVELS : 0;
  if (words) *words = on ? e->es.shape.W : 0;
  if (samples) *samples = on ? e->es.samples : 0;
  return 0;
}

int gph_engine_ess_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->es : nullptr, out, max_loci, count); }

// acc [selected][series][2 + 2 levels], changes [selected], focal [selected][n - 1][words] (changes / focal may be null)
int gph_engine_ess_fetch(gph_engine *e, double *acc, uint32_t *changes, uint64_t *focal, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->es.on) return GPH_ESTATE;
  const size_t nsel = e->es.sel.loci.size();
  if (nsel > 0 && !acc) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) {
    std::vector<char> all(e->es.bytes);
    { int rc = pull_rows(e, all.data(), e->es.d, e->es.bytes); if (rc) return rc; }
    memcpy(acc, all.data(), e->es.o_focal);
    if (focal) memcpy(focal, all.data() + e->es.o_focal, e->es.o_prev - e->es.o_focal);
    if (changes) memcpy(changes, all.data() + e->es.o_changes, nsel * 4);
  }
  return reset ? selected_zero(e, e->es) : 0;
}

// ---- posterior predictive checks of selected loci (gph_predictive.h)
// k_predictive over the selection: the data's statistics (observed) or sample t of the current state
static int predictive_launch(gph_engine *e, int observed, uint64_t *row)
{
  const int nsel = (int)e->pd.sel.loci.size();
  launch_pre(e);
  return launch_grid(e, GphGrid{nsel, 1}, e->pd.shape.bd, (size_t)e->pd.shape.lds_bytes, k_predictive, e->ka, e->pd.shape, (const char *)e->dev.pages,
                     e->dev.seq, e->dev.seq_off, e->dev.P, (const int32_t *)e->pd.sel.d_slot, (const uint64_t *)(e->pd.d + e->pd.o_key),
                     (const uint8_t *)(e->pd.d + e->pd.o_pop), nsel, (int)e->L, (long long)e->pd.samples, observed, (double *)e->pd.d, row,
                     (const char *)nullptr, 0, 0, 0);
}
// the accumulators back to zero, t back to 0, and the data's statistics formed again (they live in the same words)
static int predictive_zero(gph_engine *e)
{
  { int rcz = acc_zero(e, e->pd.d, e->pd.o_key); if (rcz) return rcz; }
  if (e->pd.sel.loci.empty()) return 0;          /* (a rank without a selected locus launches nothing) */
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  { int rcl = predictive_launch(e, 1, (uint64_t *)(e->pd.d + e->pd.o_obs)); if (rcl) return rcl; }
  flat_launched(e, -1, 1);
  return 0;
}
static void predictive_free(gph_engine *e) { selected_free(e->pd); }

int gph_engine_predictive_enable(gph_engine *e, uint64_t seed, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || !sel_valid(loci, nloci)) return GPH_EARG;
  SETDEV(e);
  predictive_free(e);
  if (capacity_rows == 0) return 0;
  const int n = e->cfg.n, Kc = e->cfg.Kc;
  GphPdShape h;
  gph_pd_shape(e->lay, h);
  if (n > 255 || h.lds_bytes > 65536) {
    fprintf(stderr, "gphocs_hip: predictive: %d leaves in %d current populations need byte counts above 255 or %d bytes of LDS a workgroup (65536 at most)\n",
            n, Kc, (int)h.lds_bytes);
    return GPH_EARG;
  }
  { int rcs = sel_alloc(e, e->pd.sel, loci, nloci); if (rcs) return rcs; }
  const size_t nsel = e->pd.sel.loci.size();
  int64_t maxpair = 1;
  for (int p = 0; p < Kc; p++) if ((int64_t)e->samplesPerPop[p] * e->samplesPerPop[p] > maxpair) maxpair = (int64_t)e->samplesPerPop[p] * e->samplesPerPop[p];
  for (size_t q = 0; q < nsel; q++) {
    const int64_t g = e->pd.sel.loci[q], sites = e->h_sites[(size_t)(g - e->cfg.locus_begin)];
    if (sites >= ((int64_t)1 << 31) || sites * maxpair >= ((int64_t)1 << 32)) {
      fprintf(stderr, "gphocs_hip: predictive: locus %lld: %lld sites x %lld sample pairs reach 2^32: its statistics do not fit 32 bits\n",
              (long long)g, (long long)sites, (long long)maxpair);
      predictive_free(e);
      return GPH_EARG;
    }
    e->pd.sites.push_back(sites);
  }
  const size_t o_obs = nsel * (size_t)h.C * GPH_PD_WORDS * 8, o_key = o_obs + (size_t)h.C * 8, o_pop = o_key + nsel * 8, bytes = o_pop + (((size_t)n + 15) & ~(size_t)15);
  const int64_t need = (int64_t)bytes + (int64_t)capacity_rows * h.C * 8;
  if (over_limit(need, max_bytes, "predictive: the accumulators and rows", "%lld loci x (%d statistics x 40 + 8) + %d rows x %d x 8 + %d",
                 (long long)nsel, (int)h.C, (int)capacity_rows, (int)h.C, (int)(h.C * 8 + ((n + 15) & ~15)))) {
    predictive_free(e);
    return GPH_EFULL;
  }
  if (dev_alloc((void **)&e->pd.d, bytes)) { dev_clear_error(); e->pd.d = nullptr; predictive_free(e); return GPH_EHIP; }
  if (rows_alloc(e->pd.rows, sizeof(uint64_t), h.C, capacity_rows)) { dev_clear_error(); predictive_free(e); return GPH_EHIP; }
  std::vector<uint64_t> key(nsel + 1);
  for (size_t q = 0; q < nsel; q++) key[q] = gph_pd_locus_key(seed, (uint64_t)e->pd.sel.loci[q]);
  const std::vector<uint8_t> pop = leaf_pops(e, false);
  int rc = 0;
  if (nsel > 0) rc = h2d(e, e->pd.d + o_key, key.data(), nsel * 8);
  if (!rc) rc = h2d(e, e->pd.d + o_pop, pop.data(), pop.size());
  if (rc) { predictive_free(e); return rc; }
  e->pd.shape = h;
  e->pd.seed = seed;
  e->pd.o_obs = o_obs; e->pd.o_key = o_key; e->pd.o_pop = o_pop; e->pd.bytes = bytes;
  return selected_on(e, e->pd, predictive_zero);
}

// one sample of the current state, queued on the engine's stream
int gph_engine_predictive_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->pd.on) return GPH_ESTATE;
  /* (a rank without a selected locus launches nothing: its row stays 0) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 22, !e->pd.sel.loci.empty(), SmTaken{&e->pd.rows, true, &e->pd.iters, iteration, &e->pd.samples},
                    [&](void *row) { return predictive_launch(e, 0, (uint64_t *)row); });
}

int gph_engine_predictive_shape(gph_engine *e, int64_t *selected, int32_t *stats, int64_t *samples, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  const bool on = e->pd.on;
  if (selected) *selected = on ? (int64_t)e->pd.sel.loci.size() : 0;
  if (stats) *stats = on ? e->pd.shape.C : 0;
  if (samples) *samples = on ? e->pd.samples : 0;
  if (rows_held) *rows_held = on ? e->pd.rows.fill : 0;
  return 0;
}

int gph_engine_predictive_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->pd : nullptr, out, max_loci, count); }

// acc [selected][C][5] (obs, gt, eq, s1, s2), sites [selected] (may be null)
int gph_engine_predictive_fetch_loci(gph_engine *e, double *acc, int64_t *sites, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->pd.on) return GPH_ESTATE;
  const size_t nsel = e->pd.sel.loci.size();
  if (nsel > 0 && !acc) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) { int rc = pull_rows(e, acc, e->pd.d, e->pd.o_obs); if (rc) return rc; }
  if (sites) for (size_t q = 0; q < nsel; q++) sites[q] = e->pd.sites[q];
  return reset ? selected_zero(e, e->pd) : 0;
}

// the rows taken since the last fetch ([rows][C], with their iterations) and the data's totals (observed [C], may be null);
// the row buffer is empty again
int gph_engine_predictive_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *rows_out, uint64_t *observed, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || ((!rows_out || !iters) && max_rows > 0)) return GPH_EARG;
  if (!e->pd.on) return GPH_ESTATE;
  SmRows &b = e->pd.rows;
  if (max_rows < b.fill) return GPH_EARG;
  SETDEV(e);
  if (observed) { int rc = pull_rows(e, observed, e->pd.d + e->pd.o_obs, (size_t)b.n * 8); if (rc) return rc; }
  /* (no ld in this entry point: the rows arrive packed) */
  return rows_iters_fetch(e, b, e->pd.iters, iters, rows_out, 0, true, rows);
}

// seg, then diff_<p>|<q> for the current populations p <= q (model order), p-major
const char *gph_engine_predictive_column_name(gph_engine *e, int32_t col)
{
  if (!e || !e->pd.on || col < 0 || col >= e->pd.shape.C) return nullptr;
  if (col == 0) return "seg";
  const int Kc = e->cfg.Kc;
  for (int p = 0; p < Kc; p++)
    for (int q = p; q < Kc; q++)
      if (gph_pd_pair(Kc, p, q) == col) { e->pd.name = "diff_" + std::to_string(p) + "|" + std::to_string(q); return e->pd.name.c_str(); }
  return nullptr;
}

// ---- triplet topology weights of selected loci (gph_triplets.h)
// the accumulators back to zero, the sample count with them
static int triplets_zero(gph_engine *e) { return acc_zero(e, e->tr.d, e->tr.o_tri); }
static void triplets_free(gph_engine *e) { selected_free(e->tr); }
static int triplets_refuse(const char *fmt, long long a, long long b, long long c, long long d)
{
  fprintf(stderr, "gphocs_hip: triplets: ");
  fprintf(stderr, fmt, a, b, c, d);
  fputc('\n', stderr);
  return GPH_EARG;
}

int gph_engine_triplets_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, const int32_t *triples, int32_t ntriples, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || (loci && nloci < 0) || (triples && ntriples < 0)) return GPH_EARG;
  SETDEV(e);
  if (capacity_rows == 0) { triplets_free(e); return 0; }
  const int n = e->cfg.n, Kc = e->cfg.Kc;
  /* every refusal before anything is freed or allocated: a refused call leaves the sampler as it was.  (The other samplers
   * free first, and refuse a selection through sel_valid without a message; this one says what is wrong with it and also
   * holds it against the loci of all ranks) */
  if (Kc < 3) return triplets_refuse("%lld current population(s): a triple needs three", Kc, 0, 0, 0);
  if (n > 255) return triplets_refuse("%lld leaves: the byte counts of k_triplets hold 255 at most", n, 0, 0, 0);
  if (loci)
    for (int64_t k = 0; k < nloci; k++) {
      if (loci[k] < 0 || loci[k] >= e->cfg.L_total) return triplets_refuse("locus %lld is out of range (0 .. %lld)", loci[k], e->cfg.L_total - 1, 0, 0);
      if (k > 0 && loci[k] == loci[k - 1]) return triplets_refuse("locus %lld is named twice", loci[k], 0, 0, 0);
      if (k > 0 && loci[k] < loci[k - 1]) return triplets_refuse("locus %lld stands behind locus %lld: the selection is not increasing", loci[k], loci[k - 1], 0, 0);
    }
  std::vector<int32_t> tri;
  if (!triples) {
    for (int P = 0; P < Kc; P++)
      for (int Q = P + 1; Q < Kc; Q++)
        for (int R = Q + 1; R < Kc; R++)
          if (e->samplesPerPop[P] >= 1 && e->samplesPerPop[Q] >= 1 && e->samplesPerPop[R] >= 1) tri.push_back(gph_tr_pack(P, Q, R));
  } else {
    for (int32_t k = 0; k < ntriples; k++) {
      int m[3] = {triples[3 * k], triples[3 * k + 1], triples[3 * k + 2]};
      for (int a = 0; a < 3; a++)
        if (m[a] < 0 || m[a] >= Kc) return triplets_refuse("triple %lld names population %lld: the current populations are 0 .. %lld", k, m[a], Kc - 1, 0);
      std::sort(m, m + 3);
      if (m[0] == m[1] || m[1] == m[2]) return triplets_refuse("triple %lld (%lld, %lld, %lld) repeats a population", k, triples[3 * k], triples[3 * k + 1], triples[3 * k + 2]);
      for (int a = 0; a < 3; a++)
        if (e->samplesPerPop[m[a]] < 1) return triplets_refuse("triple %lld names population %lld, which has no sample", k, m[a], 0, 0);
      const int32_t word = gph_tr_pack(m[0], m[1], m[2]);
      for (int32_t q = 0; q < k; q++)
        if (tri[(size_t)q] == word) return triplets_refuse("triple %lld (%lld, %lld, %lld) is named twice", k, m[0], m[1], m[2]);
      tri.push_back(word);
    }
  }
  if (tri.empty()) return triplets_refuse("no triple of populations with samples", 0, 0, 0, 0);
  const int T = (int)tri.size();
  GphTrShape h;
  gph_tr_shape(e->lay, T, h);
  if (h.lds_bytes > 65536) return triplets_refuse("%lld leaves in %lld current populations need %lld bytes of LDS a workgroup (65536 at most)", n, Kc, h.lds_bytes, 0);
  triplets_free(e);
  int64_t nsel = 0;
  if (!loci) nsel = e->L;
  else for (int64_t k = 0; k < nloci; k++) nsel += loci[k] >= e->cfg.locus_begin && loci[k] < e->cfg.locus_begin + e->L;
  const std::vector<uint8_t> pop = leaf_pops(e, true);
  const size_t o_tri = (size_t)nsel * 2 * h.slots * 8, o_pop = (o_tri + (size_t)T * 4 + 15) & ~(size_t)15, bytes = o_pop + pop.size();
  const int64_t need = (int64_t)bytes + (int64_t)capacity_rows * h.slots * 8;
  /* (nothing to free behind this refusal: the sampler is off already) */
  if (over_limit(need, max_bytes, "triplets: the accumulators and rows", "%lld loci x %d triples x 48 + %d rows x %d x 8 + %lld",
                 (long long)nsel, T, (int)capacity_rows, (int)h.slots, (long long)(bytes - o_tri))) return GPH_EFULL;
  { int rcs = sel_alloc(e, e->tr.sel, loci, nloci); if (rcs) return rcs; }
  if (dev_alloc((void **)&e->tr.d, bytes)) { dev_clear_error(); e->tr.d = nullptr; triplets_free(e); return GPH_EHIP; }
  if (rows_alloc(e->tr.rows, sizeof(uint64_t), h.slots, capacity_rows)) { dev_clear_error(); triplets_free(e); return GPH_EHIP; }
  int rc = h2d(e, e->tr.d + o_tri, tri.data(), (size_t)T * 4);
  if (!rc) rc = h2d(e, e->tr.d + o_pop, pop.data(), pop.size());
  if (rc) { triplets_free(e); return rc; }
  e->tr.shape = h;
  e->tr.tri = tri;
  e->tr.o_tri = o_tri; e->tr.o_pop = o_pop; e->tr.bytes = bytes;
  return selected_on(e, e->tr, triplets_zero);
}

// one sample of the current state, queued on the engine's stream
int gph_engine_triplets_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->tr.on) return GPH_ESTATE;
  const GphTrShape &h = e->tr.shape;
  const int nsel = (int)e->tr.sel.loci.size(), groups = (nsel + h.G - 1) / h.G;
  /* (a rank without a selected locus launches nothing: its row stays 0) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 23, groups > 0, SmTaken{&e->tr.rows, true, &e->tr.iters, iteration, &e->tr.samples}, [&](void *row) {
    return launch_grid(e, GphGrid{groups, 1}, h.bd, (size_t)h.lds_bytes, k_triplets, e->lay, h, (const char *)e->dev.pages, (const int32_t *)e->tr.sel.d_slot,
                       (const int32_t *)(e->tr.d + e->tr.o_tri), (const uint8_t *)(e->tr.d + e->tr.o_pop), nsel, (int)e->L, (double *)e->tr.d, (uint64_t *)row);
  });
}

int gph_engine_triplets_shape(gph_engine *e, int32_t *triples, int32_t *slots, int64_t *selected, int64_t *samples, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  const bool on = e->tr.on;
  if (triples) *triples = on ? e->tr.shape.T : 0;
  if (slots) *slots = on ? e->tr.shape.slots : 0;
  if (selected) *selected = on ? (int64_t)e->tr.sel.loci.size() : 0;
  if (samples) *samples = on ? e->tr.samples : 0;
  if (rows_held) *rows_held = on ? e->tr.rows.fill : 0;
  return 0;
}

int gph_engine_triplets_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->tr : nullptr, out, max_loci, count); }

// out [selected][ld], ld >= 2 slots: W of every slot, then A of every slot
int gph_engine_triplets_fetch_loci(gph_engine *e, double *out, int64_t ld, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->tr.on) return GPH_ESTATE;
  const size_t nsel = e->tr.sel.loci.size(), w = 2 * (size_t)e->tr.shape.slots;
  if ((nsel > 0 && !out) || ld < (int64_t)w) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) {
    std::vector<double> acc(nsel * w);
    { int rc = pull_rows(e, acc.data(), e->tr.d, e->tr.o_tri); if (rc) return rc; }
    for (size_t q = 0; q < nsel; q++) memcpy(out + q * (size_t)ld, acc.data() + q * w, w * 8);
  }
  return reset ? selected_zero(e, e->tr) : 0;
}

// the rows taken since the last fetch (iters[rows], out[rows][ld], ld >= slots); the row buffer is empty again
int gph_engine_triplets_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *out, int64_t ld, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || ((!out || !iters) && max_rows > 0)) return GPH_EARG;
  if (!e->tr.on) return GPH_ESTATE;
  SmRows &b = e->tr.rows;
  if (max_rows < b.fill || (b.fill > 0 && ld < b.n)) return GPH_EARG;
  return rows_iters_fetch(e, b, e->tr.iters, iters, out, ld, true, rows);
}

// slot 3 k + t of triple k = (P, Q, R): "<P>,<Q>|<R>", "<P>,<R>|<Q>", "<Q>,<R>|<P>" with the indices of the current populations
const char *gph_engine_triplets_column_name(gph_engine *e, int32_t col)
{
  if (!e || !e->tr.on || col < 0 || col >= e->tr.shape.slots) return nullptr;
  const uint32_t word = (uint32_t)e->tr.tri[(size_t)(col / 3)];
  const int m[3] = {(int)(word & 255u), (int)((word >> 8) & 255u), (int)((word >> 16) & 255u)}, t = col % 3;
  const int x = t == 2 ? m[1] : m[0], y = t == 0 ? m[1] : m[2], z = t == 0 ? m[2] : t == 1 ? m[1] : m[0];
  e->tr.name = std::to_string(x) + "," + std::to_string(y) + "|" + std::to_string(z);
  return e->tr.name.c_str();
}

// ---- expected substitutions per population branch and per sample, of selected loci (gph_mutations.h)
static int mutations_zero(gph_engine *e) { return acc_zero(e, e->mu.d, e->mu.bytes); }
static void mutations_free(gph_engine *e) { selected_free(e->mu, {e->mu.part.d_part}); }
static int mutations_refuse(const char *fmt, long long a, long long b)
{
  fprintf(stderr, "gphocs_hip: mutations: ");
  fprintf(stderr, fmt, a, b);
  fputc('\n', stderr);
  return GPH_EARG;
}

int gph_engine_mutations_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || (loci && nloci < 0)) return GPH_EARG;
  SETDEV(e);
  if (capacity_rows == 0) { mutations_free(e); return 0; }
  /* every refusal before anything is freed or allocated, as the triplet weights do: a refused call leaves the sampler as it was */
  if (loci)
    for (int64_t k = 0; k < nloci; k++) {
      if (loci[k] < 0 || loci[k] >= e->cfg.L_total) return mutations_refuse("locus %lld is out of range (0 .. %lld)", loci[k], e->cfg.L_total - 1);
      if (k > 0 && loci[k] == loci[k - 1]) return mutations_refuse("locus %lld is named twice", loci[k], 0);
      if (k > 0 && loci[k] < loci[k - 1]) return mutations_refuse("locus %lld stands behind locus %lld: the selection is not increasing", loci[k], loci[k - 1]);
    }
  GphMuShape h;
  gph_mu_shape(e->lay, h);
  if (h.lds_bytes > GPH_MU_LDS_BUDGET) return mutations_refuse("%lld leaves need %lld bytes of LDS a workgroup for one row of a locus (40960 at most, the samplers' budget)", e->cfg.n, h.lds_bytes);
  mutations_free(e);
  int64_t nsel = 0;
  if (!loci) nsel = e->L;
  else for (int64_t k = 0; k < nloci; k++) nsel += loci[k] >= e->cfg.locus_begin && loci[k] < e->cfg.locus_begin + e->L;
  const int rd = 1 + h.C, nchunks = (int)((nsel + h.chunk - 1) / h.chunk);
  const size_t bytes = (size_t)nsel * h.C * 8, pbytes = (size_t)(nchunks > 0 ? nchunks : 1) * rd * 8;
  const int64_t need = (int64_t)bytes + (int64_t)pbytes + (int64_t)capacity_rows * rd * 8;
  /* (nothing to free behind this refusal: the sampler is off already) */
  if (over_limit(need, max_bytes, "mutations: the accumulators and rows", "%lld loci x %d x 8 + (%d chunks + %d rows) x %d x 8",
                 (long long)nsel, (int)h.C, nchunks > 0 ? nchunks : 1, (int)capacity_rows, rd)) return GPH_EFULL;
  { int rcs = sel_alloc(e, e->mu.sel, loci, nloci); if (rcs) return rcs; }
  if (dev_alloc((void **)&e->mu.d, bytes > 0 ? bytes : 8)) { dev_clear_error(); e->mu.d = nullptr; mutations_free(e); return GPH_EHIP; }
  if (dev_alloc((void **)&e->mu.part.d_part, pbytes)) { dev_clear_error(); e->mu.part.d_part = nullptr; mutations_free(e); return GPH_EHIP; }
  if (rows_alloc(e->mu.rows, sizeof(double), rd, capacity_rows)) { dev_clear_error(); mutations_free(e); return GPH_EHIP; }
  e->mu.part.rd = rd; e->mu.part.chunk = h.chunk; e->mu.part.nchunks = nchunks;
  e->mu.shape = h;
  e->mu.bytes = bytes;
  return selected_on(e, e->mu, mutations_zero);
}

// one sample of the current state into the accumulators and the next free row, queued on the engine's stream.  The settle level
// is that of the time slices: the population ages and fathers are read from the chain state
int gph_engine_mutations_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->mu.on) return GPH_ESTATE;
  const GphMuShape &h = e->mu.shape;
  const SmParts &p = e->mu.part;
  const int nsel = (int)e->mu.sel.loci.size();
  SmTaken t;
  t.rows = &e->mu.rows;
  t.samples = &e->mu.samples;
  /* (a rank without a selected locus launches the fold alone: its row is the iteration and zeros) */
  return sample_run(e, SETTLE_CHAIN, 24, p.nchunks > 0 ? 2 : 1, t, [&](void *row) {
    if (p.nchunks > 0) {
      launch_pre(e);
      int rcl = launch_grid(e, GphGrid{p.nchunks, 1}, h.bd, (size_t)h.lds_bytes, k_mutations, e->ka, h, (const char *)e->dev.pages, (const char *)e->dev.cond,
                            e->dev.cond_off, e->dev.seq, e->dev.seq_off, e->dev.P, (const int32_t *)e->mu.sel.d_slot, nsel, (int)e->L, (double *)e->mu.d, p.d_part);
      if (rcl) return rcl;
    }
    return parts_fold(e, p, iteration, (double *)row);
  });
}

int gph_engine_mutations_shape(gph_engine *e, int32_t *columns, int32_t *chunk, int64_t *selected, int64_t *samples, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  const bool on = e->mu.on;
  if (columns) *columns = on ? e->mu.shape.C : 0;
  if (chunk) *chunk = on ? e->mu.shape.chunk : 0;
  if (selected) *selected = on ? (int64_t)e->mu.sel.loci.size() : 0;
  if (samples) *samples = on ? e->mu.samples : 0;
  if (rows_held) *rows_held = on ? e->mu.rows.fill : 0;
  return 0;
}

int gph_engine_mutations_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->mu : nullptr, out, max_loci, count); }

// out [selected][ld] doubles, the C columns of gph_engine_mutations_column_name
int gph_engine_mutations_fetch_loci(gph_engine *e, double *out, int64_t ld, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->mu.on) return GPH_ESTATE;
  const size_t nsel = e->mu.sel.loci.size(), w = (size_t)e->mu.shape.C;
  if (nsel > 0 && (!out || ld < (int64_t)w)) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) {
    std::vector<double> acc(nsel * w);
    { int rc = pull_rows(e, acc.data(), e->mu.d, e->mu.bytes); if (rc) return rc; }
    for (size_t q = 0; q < nsel; q++) memcpy(out + q * (size_t)ld, acc.data() + q * w, w * 8);
  }
  return reset ? selected_zero(e, e->mu) : 0;
}

// the rows taken since the last fetch, [rows][1 + C] doubles (column 0: the iteration); the row buffer is empty again
int gph_engine_mutations_fetch_rows(gph_engine *e, double *out, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || (!out && max_rows > 0)) return GPH_EARG;
  if (!e->mu.on) return GPH_ESTATE;
  if (max_rows < e->mu.rows.fill) return GPH_EARG;
  SETDEV(e);
  return rows_fetch(e, e->mu.rows, out, rows);
}

// mut.<p>, exp.<p> for the K populations (model order), then mutExt.<i>, expExt.<i> for the n leaves
const char *gph_engine_mutations_column_name(gph_engine *e, int32_t col)
{
  if (!e || !e->mu.on || col < 0 || col >= e->mu.shape.C) return nullptr;
  const int K = e->cfg.K, n = e->cfg.n;
  if (col < 2 * K) e->mu.name = std::string(col < K ? "mut." : "exp.") + std::to_string(col % K);
  else e->mu.name = std::string(col - 2 * K < n ? "mutExt." : "expExt.") + std::to_string((col - 2 * K) % n);
  return e->mu.name.c_str();
}

// ---- pairwise coalescence-time distributions of selected loci (gph_pairtimes.h)
// the accumulators back to zero, the sample count with them
static int pair_times_zero(gph_engine *e) { return acc_zero(e, e->pt.d, e->pt.o_pair); }
static void pair_times_free(gph_engine *e) { selected_free(e->pt); }
static int pair_times_refuse(const char *fmt, long long a, long long b, long long c, long long d)
{
  fprintf(stderr, "gphocs_hip: pair times: ");
  fprintf(stderr, fmt, a, b, c, d);
  fputc('\n', stderr);
  return GPH_EARG;
}
// the leaf pairs of slot (P, Q), P <= Q
static int64_t pair_times_m(const gph_engine *e, int P, int Q)
{
  const int64_t a = e->samplesPerPop[P], b = e->samplesPerPop[Q];
  return P == Q ? a * (a - 1) / 2 : a * b;
}

int gph_engine_pair_times_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, const int32_t *pairs, int32_t npairs,
                                 const double *edges, int32_t nedges, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || (loci && nloci < 0) || (pairs && npairs < 0)) return GPH_EARG;
  SETDEV(e);
  if (capacity_rows == 0) { pair_times_free(e); return 0; }
  const int n = e->cfg.n, Kc = e->cfg.Kc;
  /* every refusal before anything is freed or allocated, as the triplet weights do: a refused call leaves the sampler as it was */
  if (n > 255) return pair_times_refuse("%lld leaves: the byte counts of k_pair_times hold 255 at most", n, 0, 0, 0);
  if (loci)
    for (int64_t k = 0; k < nloci; k++) {
      if (loci[k] < 0 || loci[k] >= e->cfg.L_total) return pair_times_refuse("locus %lld is out of range (0 .. %lld)", loci[k], e->cfg.L_total - 1, 0, 0);
      if (k > 0 && loci[k] == loci[k - 1]) return pair_times_refuse("locus %lld is named twice", loci[k], 0, 0, 0);
      if (k > 0 && loci[k] < loci[k - 1]) return pair_times_refuse("locus %lld stands behind locus %lld: the selection is not increasing", loci[k], loci[k - 1], 0, 0);
    }
  std::vector<int32_t> pr;
  if (!pairs) {
    for (int P = 0; P < Kc; P++)
      for (int Q = P; Q < Kc; Q++)
        if (pair_times_m(e, P, Q) >= 1) pr.push_back(gph_pt_pack(P, Q));
  } else {
    for (int32_t k = 0; k < npairs; k++) {
      int m[2] = {pairs[2 * k], pairs[2 * k + 1]};
      for (int a = 0; a < 2; a++)
        if (m[a] < 0 || m[a] >= Kc) return pair_times_refuse("pair %lld names population %lld: the current populations are 0 .. %lld", k, m[a], Kc - 1, 0);
      if (m[0] > m[1]) std::swap(m[0], m[1]);
      if (m[0] == m[1] && e->samplesPerPop[m[0]] < 2) return pair_times_refuse("pair %lld: population %lld has fewer than two samples", k, m[0], 0, 0);
      for (int a = 0; a < 2; a++)
        if (e->samplesPerPop[m[a]] < 1) return pair_times_refuse("pair %lld names population %lld, which has no sample", k, m[a], 0, 0);
      const int32_t word = gph_pt_pack(m[0], m[1]);
      for (int32_t q = 0; q < k; q++)
        if (pr[(size_t)q] == word) return pair_times_refuse("pair %lld (%lld, %lld) is named twice", k, m[0], m[1], 0);
      pr.push_back(word);
    }
  }
  if (pr.empty()) return pair_times_refuse("no pair of populations with a pair of samples", 0, 0, 0, 0);
  if (nedges < 1 || nedges > GPH_PT_MAXEDGES || !edges) return pair_times_refuse("%lld edges: a grid has 1 .. %lld", edges ? nedges : 0, GPH_PT_MAXEDGES, 0, 0);
  for (int32_t k = 0; k < nedges; k++) {
    if (!std::isfinite(edges[k]) || !(edges[k] > 0.0)) return pair_times_refuse("edge %lld is not a finite positive number", k, 0, 0, 0);
    if (k > 0 && !(edges[k] > edges[k - 1])) return pair_times_refuse("edge %lld does not lie above edge %lld", k, k - 1, 0, 0);
  }
  const int NP = (int)pr.size();
  GphPtShape h;
  gph_pt_shape(e->lay, NP, nedges, h);
  if (h.tr.lds_bytes > 65536) return pair_times_refuse("%lld leaves in %lld current populations need %lld bytes of LDS a workgroup (65536 at most)", n, Kc, h.tr.lds_bytes, 0);
  pair_times_free(e);
  int64_t nsel = 0;
  if (!loci) nsel = e->L;
  else for (int64_t k = 0; k < nloci; k++) nsel += loci[k] >= e->cfg.locus_begin && loci[k] < e->cfg.locus_begin + e->L;
  const std::vector<uint8_t> pop = leaf_pops(e, true);
  const size_t o_pair = (size_t)nsel * 4 * NP * 8, o_edge = (o_pair + (size_t)NP * 4 + 15) & ~(size_t)15,
               o_pop = (o_edge + (size_t)nedges * 8 + 15) & ~(size_t)15, bytes = o_pop + pop.size();
  const int64_t need = (int64_t)bytes + (int64_t)capacity_rows * h.W * 8;
  /* (nothing to free behind this refusal: the sampler is off already) */
  if (over_limit(need, max_bytes, "pair times: the accumulators and rows", "%lld loci x %d pairs x 32 + %d rows x %d x 8 + %lld",
                 (long long)nsel, NP, (int)capacity_rows, (int)h.W, (long long)(bytes - o_pair))) return GPH_EFULL;
  { int rcs = sel_alloc(e, e->pt.sel, loci, nloci); if (rcs) return rcs; }
  if (dev_alloc((void **)&e->pt.d, bytes)) { dev_clear_error(); e->pt.d = nullptr; pair_times_free(e); return GPH_EHIP; }
  if (rows_alloc(e->pt.rows, sizeof(uint64_t), h.W, capacity_rows)) { dev_clear_error(); pair_times_free(e); return GPH_EHIP; }
  int rc = h2d(e, e->pt.d + o_pair, pr.data(), (size_t)NP * 4);
  if (!rc) rc = h2d(e, e->pt.d + o_edge, edges, (size_t)nedges * 8);
  if (!rc) rc = h2d(e, e->pt.d + o_pop, pop.data(), pop.size());
  if (rc) { pair_times_free(e); return rc; }
  e->pt.shape = h;
  e->pt.pairs = pr;
  e->pt.edges.assign(edges, edges + nedges);
  e->pt.o_pair = o_pair; e->pt.o_edge = o_edge; e->pt.o_pop = o_pop; e->pt.bytes = bytes;
  return selected_on(e, e->pt, pair_times_zero);
}

// one sample of the current state, queued on the engine's stream.  The settle level is that of the time slices: the population
// ages and fathers are read from the chain state
int gph_engine_pair_times_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->pt.on) return GPH_ESTATE;
  const GphPtShape &h = e->pt.shape;
  const int nsel = (int)e->pt.sel.loci.size(), groups = (nsel + h.tr.G - 1) / h.tr.G;
  /* (a rank without a selected locus launches nothing: its row stays 0) */
  return sample_run(e, SETTLE_CHAIN, 26, groups > 0, SmTaken{&e->pt.rows, true, &e->pt.iters, iteration, &e->pt.samples}, [&](void *row) {
    launch_pre(e);
    return launch_grid(e, GphGrid{groups, 1}, h.tr.bd, (size_t)h.tr.lds_bytes, k_pair_times, e->ka, h, (const char *)e->dev.pages, (const int32_t *)e->pt.sel.d_slot,
                       (const int32_t *)(e->pt.d + e->pt.o_pair), (const uint8_t *)(e->pt.d + e->pt.o_pop), (const double *)(e->pt.d + e->pt.o_edge), nsel,
                       (int)e->L, (double *)e->pt.d, (uint64_t *)row);
  });
}

// pairs: NP; bins: B; group: the loci a workgroup takes; edges_out [B - 1] (may be null): the grid as given
int gph_engine_pair_times_shape(gph_engine *e, int32_t *pairs, int32_t *bins, int32_t *group, int64_t *selected, int64_t *samples, int32_t *rows_held, double *edges_out)
{
  if (!e) return GPH_EARG;
  const bool on = e->pt.on;
  if (pairs) *pairs = on ? e->pt.shape.NP : 0;
  if (bins) *bins = on ? e->pt.shape.B : 0;
  if (group) *group = on ? e->pt.shape.tr.G : 0;
  if (selected) *selected = on ? (int64_t)e->pt.sel.loci.size() : 0;
  if (samples) *samples = on ? e->pt.samples : 0;
  if (rows_held) *rows_held = on ? e->pt.rows.fill : 0;
  if (edges_out && on) for (size_t k = 0; k < e->pt.edges.size(); k++) edges_out[k] = e->pt.edges[k];
  return 0;
}

int gph_engine_pair_times_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->pt : nullptr, out, max_loci, count); }

// out [selected][ld], ld >= 4 NP: A of every slot, then Y, X, M
int gph_engine_pair_times_fetch_loci(gph_engine *e, double *out, int64_t ld, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->pt.on) return GPH_ESTATE;
  const size_t nsel = e->pt.sel.loci.size(), w = 4 * (size_t)e->pt.shape.NP;
  if ((nsel > 0 && !out) || ld < (int64_t)w) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) {
    std::vector<double> acc(nsel * w);
    { int rc = pull_rows(e, acc.data(), e->pt.d, e->pt.o_pair); if (rc) return rc; }
    for (size_t q = 0; q < nsel; q++) memcpy(out + q * (size_t)ld, acc.data() + q * w, w * 8);
  }
  return reset ? selected_zero(e, e->pt) : 0;
}

// the rows taken since the last fetch (iters[rows], out[rows][ld], ld >= NP (B + 2)); the row buffer is empty again
int gph_engine_pair_times_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *out, int64_t ld, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || ((!out || !iters) && max_rows > 0)) return GPH_EARG;
  if (!e->pt.on) return GPH_ESTATE;
  SmRows &b = e->pt.rows;
  if (max_rows < b.fill || (b.fill > 0 && ld < b.n)) return GPH_EARG;
  return rows_iters_fetch(e, b, e->pt.iters, iters, out, ld, true, rows);
}

// "<P>|<Q>:<k>" per slot and bin, then "below_<P>|<Q>" per slot, then "loci_<P>|<Q>" per slot, with the indices of the current populations
const char *gph_engine_pair_times_column_name(gph_engine *e, int32_t col)
{
  if (!e || !e->pt.on || col < 0 || col >= e->pt.shape.W) return nullptr;
  const int NP = e->pt.shape.NP, B = e->pt.shape.B;
  const int sl = col < NP * B ? col / B : (col - NP * B) % NP;
  const uint32_t word = (uint32_t)e->pt.pairs[(size_t)sl];
  const std::string pq = std::to_string((int)(word & 255u)) + "|" + std::to_string((int)((word >> 8) & 255u));
  e->pt.name = col < NP * B ? pq + ":" + std::to_string(col % B) : (col < NP * B + NP ? "below_" : "loci_") + pq;
  return e->pt.name.c_str();
}

// ---- site-frequency spectra of selected loci, data against sampled genealogies (gph_sfs.h)
// the accumulators E back to zero, the sample count with them (the data side stays: it is formed once, at enable)
static int sfs_zero(gph_engine *e) { return acc_zero(e, e->sf.d, e->sf.o_obs); }
static void sfs_free(gph_engine *e) { selected_free(e->sf, {e->sf.part.d_part}); }
static int sfs_refuse(const char *fmt, long long a, long long b, long long c)
{
  fprintf(stderr, "gphocs_hip: sfs: ");
  fprintf(stderr, fmt, a, b, c);
  fputc('\n', stderr);
  return GPH_EARG;
}

int gph_engine_sfs_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, const int32_t *pairs, int32_t npairs, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || (loci && nloci < 0) || (pairs && npairs < 0)) return GPH_EARG;
  SETDEV(e);
  if (capacity_rows == 0) { sfs_free(e); return 0; }
  const int n = e->cfg.n, Kc = e->cfg.Kc;
  /* every refusal before anything is freed or allocated, as the triplet weights do: a refused call leaves the sampler as it was */
  if (n > 255) return sfs_refuse("%lld leaves: the byte counts of k_sfs_tree hold 255 at most", n, 0, 0);
  int64_t nsel = 0;
  for (int64_t k = 0; k < (loci ? nloci : e->L); k++) {
    const int64_t g = loci ? loci[k] : e->cfg.locus_begin + k;
    if (g < 0 || g >= e->cfg.L_total) return sfs_refuse("locus %lld is out of range (0 .. %lld)", g, e->cfg.L_total - 1, 0);
    if (k > 0 && loci && g == loci[k - 1]) return sfs_refuse("locus %lld is named twice", g, 0, 0);
    if (k > 0 && loci && g < loci[k - 1]) return sfs_refuse("locus %lld stands behind locus %lld: the selection is not increasing", g, loci[k - 1], 0);
    if (g < e->cfg.locus_begin || g >= e->cfg.locus_begin + e->L) continue;
    const int64_t sites = e->h_sites[(size_t)(g - e->cfg.locus_begin)];
    if (sites >= ((int64_t)1 << 32)) return sfs_refuse("locus %lld: %lld sites reach 2^32: its counts do not fit 32 bits", g, sites, 0);
    nsel++;
  }
  std::vector<int32_t> pr;                          /* [pair][2], P < Q */
  if (!pairs) {
    for (int P = 0; P < Kc; P++)
      for (int Q = P + 1; Q < Kc; Q++)
        if (e->samplesPerPop[P] >= 1 && e->samplesPerPop[Q] >= 1) { pr.push_back(P); pr.push_back(Q); }
  } else {
    for (int32_t k = 0; k < npairs; k++) {
      int m[2] = {pairs[2 * k], pairs[2 * k + 1]};
      for (int a = 0; a < 2; a++)
        if (m[a] < 0 || m[a] >= Kc) return sfs_refuse("pair %lld names population %lld: the current populations are 0 .. %lld", k, m[a], Kc - 1);
      if (m[0] == m[1]) return sfs_refuse("pair %lld names population %lld twice: a pair has two populations", k, m[0], 0);
      if (m[0] > m[1]) std::swap(m[0], m[1]);
      for (int a = 0; a < 2; a++)
        if (e->samplesPerPop[m[a]] < 1) return sfs_refuse("pair %lld names population %lld, which has no sample", k, m[a], 0);
      for (size_t q = 0; q < pr.size(); q += 2)
        if (pr[q] == m[0] && pr[q + 1] == m[1]) return sfs_refuse("pair %lld (%lld, %lld) is named twice", k, m[0], m[1]);
      pr.push_back(m[0]); pr.push_back(m[1]);
    }
  }
  std::vector<int32_t> slot, sgrp, gdef, gbase;
  for (int p = 0; p < Kc; p++) {
    if (e->samplesPerPop[p] < 2) continue;
    gdef.push_back(gph_sf_pack(0, p, p, 0)); gbase.push_back((int32_t)slot.size());
    for (int k = 1; k <= e->samplesPerPop[p] / 2; k++) { slot.push_back(gph_sf_pack(SFS_BIN, p, p, k)); sgrp.push_back((int32_t)gdef.size() - 1); }
  }
  for (size_t q = 0; q < pr.size(); q += 2) {
    gdef.push_back(gph_sf_pack(1, pr[q], pr[q + 1], 0)); gbase.push_back((int32_t)slot.size());
    for (int c = SFS_PRIVP; c <= SFS_FIXED; c++) { slot.push_back(gph_sf_pack(c, pr[q], pr[q + 1], 0)); sgrp.push_back((int32_t)gdef.size() - 1); }
  }
  if (slot.empty()) return sfs_refuse("no population has two samples and no pair is taken: there is no slot", 0, 0, 0);
  const int NS = (int)slot.size(), NG = (int)gdef.size(), W = NS + NG + 1;
  GphSfShape h;
  gph_sf_shape(e->lay, NS, NG, h);
  if (h.tr.lds_bytes > 65536 || h.d_lds > 65536)
    return sfs_refuse("%lld leaves in %lld current populations need %lld bytes of LDS a workgroup (65536 at most)", n, Kc, h.tr.lds_bytes > h.d_lds ? h.tr.lds_bytes : h.d_lds);
  sfs_free(e);
  const std::vector<uint8_t> pop = leaf_pops(e, true);
  const int rd = 1 + NS, groups = (int)((nsel + h.tr.G - 1) / h.tr.G);
  const size_t o_obs = (size_t)nsel * NS * 8, o_use = o_obs + (size_t)nsel * NS * 4, o_sites = o_use + (size_t)nsel * NG * 4,
               o_tot = (o_sites + (size_t)nsel * 4 + 7) & ~(size_t)7, o_slot = o_tot + (size_t)W * 8, o_sgrp = o_slot + (size_t)NS * 4,
               o_gdef = o_sgrp + (size_t)NS * 4, o_gbase = o_gdef + (size_t)NG * 4, o_pop = (o_gbase + (size_t)NG * 4 + 15) & ~(size_t)15,
               bytes = o_pop + pop.size(), pbytes = (size_t)(groups > 0 ? groups : 1) * rd * 8;
  const int64_t need = (int64_t)bytes + (int64_t)pbytes + (int64_t)capacity_rows * rd * 8;
  /* (nothing to free behind this refusal: the sampler is off already) */
  if (over_limit(need, max_bytes, "sfs: the accumulators and rows", "%lld loci x (%d slots x 12 + %d groups x 4 + 4) + (%d workgroups + %d rows) x %d x 8 + %lld",
                 (long long)nsel, NS, NG, groups > 0 ? groups : 1, (int)capacity_rows, rd, (long long)(bytes - o_tot))) return GPH_EFULL;
  { int rcs = sel_alloc(e, e->sf.sel, loci, nloci); if (rcs) return rcs; }
  if (dev_alloc((void **)&e->sf.d, bytes)) { dev_clear_error(); e->sf.d = nullptr; sfs_free(e); return GPH_EHIP; }
  if (dev_alloc((void **)&e->sf.part.d_part, pbytes)) { dev_clear_error(); e->sf.part.d_part = nullptr; sfs_free(e); return GPH_EHIP; }
  if (rows_alloc(e->sf.rows, sizeof(double), rd, capacity_rows)) { dev_clear_error(); sfs_free(e); return GPH_EHIP; }
  int rc = h2d(e, e->sf.d + o_slot, slot.data(), (size_t)NS * 4);
  if (!rc) rc = h2d(e, e->sf.d + o_sgrp, sgrp.data(), (size_t)NS * 4);
  if (!rc) rc = h2d(e, e->sf.d + o_gdef, gdef.data(), (size_t)NG * 4);
  if (!rc) rc = h2d(e, e->sf.d + o_gbase, gbase.data(), (size_t)NG * 4);
  if (!rc) rc = h2d(e, e->sf.d + o_pop, pop.data(), pop.size());
  /* the data side, once: one workgroup a selected locus (a rank without one keeps the zeros) */
  if (!rc) rc = acc_zero(e, e->sf.d + o_obs, o_slot - o_obs);
  if (!rc && nsel > 0) {
    int tms;
    rc = sample_begin(e, 28, tms);
    if (!rc) rc = launch_grid(e, GphGrid{(int)nsel, 1}, h.dbd, (size_t)h.d_lds, k_sfs_data, e->lay, h, e->dev.seq, e->dev.seq_off, e->dev.P,
                              (const int32_t *)e->sf.sel.d_slot, (const int32_t *)(e->sf.d + o_gdef), (const int32_t *)(e->sf.d + o_gbase),
                              (const uint8_t *)(e->sf.d + o_pop), (int)nsel, (int)e->L, (uint32_t *)(e->sf.d + o_obs), (uint32_t *)(e->sf.d + o_use),
                              (uint32_t *)(e->sf.d + o_sites), (uint64_t *)(e->sf.d + o_tot));
    if (!rc) sample_end(e, 28, 1, tms);
  }
  if (rc) { sfs_free(e); return rc; }
  e->sf.part.rd = rd; e->sf.part.chunk = h.tr.G; e->sf.part.nchunks = groups;
  e->sf.shape = h;
  e->sf.slot = slot; e->sf.sgrp = sgrp; e->sf.gdef = gdef; e->sf.gbase = gbase;
  e->sf.o_obs = o_obs; e->sf.o_use = o_use; e->sf.o_sites = o_sites; e->sf.o_tot = o_tot; e->sf.o_slot = o_slot; e->sf.o_sgrp = o_sgrp;
  e->sf.o_gdef = o_gdef; e->sf.o_gbase = o_gbase; e->sf.o_pop = o_pop; e->sf.bytes = bytes;
  return selected_on(e, e->sf, sfs_zero);
}

// one sample of the current state into the accumulators and the next free row, queued on the engine's stream: k_sfs_tree, then
// the fold of its partial rows
int gph_engine_sfs_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->sf.on) return GPH_ESTATE;
  const GphSfShape &h = e->sf.shape;
  const SmParts &p = e->sf.part;
  const int nsel = (int)e->sf.sel.loci.size();
  SmTaken t;
  t.rows = &e->sf.rows;
  t.samples = &e->sf.samples;
  /* (a rank without a selected locus launches the fold alone: its row is the iteration and zeros) */
  return sample_run(e, SETTLE_PAGES_AND_AGES, 27, p.nchunks > 0 ? 2 : 1, t, [&](void *row) {
    if (p.nchunks > 0) {
      int rcl = launch_grid(e, GphGrid{p.nchunks, 1}, h.tr.bd, (size_t)h.tr.lds_bytes, k_sfs_tree, e->lay, h, (const char *)e->dev.pages,
                            (const int32_t *)e->sf.sel.d_slot, (const int32_t *)(e->sf.d + e->sf.o_slot), (const int32_t *)(e->sf.d + e->sf.o_sgrp),
                            (const uint8_t *)(e->sf.d + e->sf.o_pop), (const uint32_t *)(e->sf.d + e->sf.o_use), nsel, (int)e->L, (double *)e->sf.d, p.d_part);
      if (rcl) return rcl;
    }
    return parts_fold(e, p, iteration, (double *)row);
  });
}

// slots: NS; groups: NG; group: the loci a workgroup takes (a partial row sums)
int gph_engine_sfs_shape(gph_engine *e, int32_t *slots, int32_t *groups, int32_t *group, int64_t *selected, int64_t *samples, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  const bool on = e->sf.on;
  if (slots) *slots = on ? e->sf.shape.NS : 0;
  if (groups) *groups = on ? e->sf.shape.NG : 0;
  if (group) *group = on ? e->sf.shape.tr.G : 0;
  if (selected) *selected = on ? (int64_t)e->sf.sel.loci.size() : 0;
  if (samples) *samples = on ? e->sf.samples : 0;
  if (rows_held) *rows_held = on ? e->sf.rows.fill : 0;
  return 0;
}

int gph_engine_sfs_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->sf : nullptr, out, max_loci, count); }

// out [NS][5]: the slot's group, its kind (0: a bin, 1 .. 4: privP, privQ, shared, fixed), P, Q (P again for a bin), k (0 for a class)
int gph_engine_sfs_slots(gph_engine *e, int32_t *out)
{
  if (!e || !out) return GPH_EARG;
  if (!e->sf.on) return GPH_ESTATE;
  for (size_t s = 0; s < e->sf.slot.size(); s++) {
    const uint32_t word = (uint32_t)e->sf.slot[s];
    out[5 * s] = e->sf.sgrp[s]; out[5 * s + 1] = (int32_t)(word >> 24); out[5 * s + 2] = (int32_t)(word & 255u);
    out[5 * s + 3] = (int32_t)((word >> 8) & 255u); out[5 * s + 4] = (int32_t)((word >> 16) & 255u);
  }
  return 0;
}

// out [selected][ld], ld >= NS: E of every slot
int gph_engine_sfs_fetch_loci(gph_engine *e, double *out, int64_t ld, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->sf.on) return GPH_ESTATE;
  const size_t nsel = e->sf.sel.loci.size(), w = (size_t)e->sf.shape.NS;
  if ((nsel > 0 && !out) || ld < (int64_t)w) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) {
    std::vector<double> acc(nsel * w);
    { int rc = pull_rows(e, acc.data(), e->sf.d, e->sf.o_obs); if (rc) return rc; }
    for (size_t q = 0; q < nsel; q++) memcpy(out + q * (size_t)ld, acc.data() + q * w, w * 8);
  }
  return reset ? selected_zero(e, e->sf) : 0;
}

// the data side as k_sfs_data left it at enable: out [selected][ld], ld >= NS + NG + 1: obs of the NS slots, use of the NG groups,
// sites; totals [NS + NG + 1] (may be null): the same over the selection.  One copy, one host synchronisation
int gph_engine_sfs_fetch_observed(gph_engine *e, uint32_t *out, int64_t ld, uint64_t *totals)
{
  if (!e) return GPH_EARG;
  if (!e->sf.on) return GPH_ESTATE;
  const size_t nsel = e->sf.sel.loci.size(), NS = (size_t)e->sf.shape.NS, NG = (size_t)e->sf.shape.NG, W = NS + NG + 1;
  if ((nsel > 0 && !out) || ld < (int64_t)W) return GPH_EARG;
  SETDEV(e);
  std::vector<char> all(e->sf.o_slot - e->sf.o_obs);
  { int rc = pull_rows(e, all.data(), e->sf.d + e->sf.o_obs, all.size()); if (rc) return rc; }
  const char *obs = all.data(), *use = all.data() + (e->sf.o_use - e->sf.o_obs), *sites = all.data() + (e->sf.o_sites - e->sf.o_obs);
  for (size_t q = 0; q < nsel; q++) {
    uint32_t *row = out + q * (size_t)ld;
    memcpy(row, obs + q * NS * 4, NS * 4);
    memcpy(row + NS, use + q * NG * 4, NG * 4);
    memcpy(row + NS + NG, sites + q * 4, 4);
  }
  if (totals) memcpy(totals, all.data() + (e->sf.o_tot - e->sf.o_obs), W * 8);
  return 0;
}

// the rows taken since the last fetch, [rows][1 + NS] doubles (column 0: the iteration); the row buffer is empty again
int gph_engine_sfs_fetch_rows(gph_engine *e, double *out, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || (!out && max_rows > 0)) return GPH_EARG;
  if (!e->sf.on) return GPH_ESTATE;
  if (max_rows < e->sf.rows.fill) return GPH_EARG;
  SETDEV(e);
  return rows_fetch(e, e->sf.rows, out, rows);
}

// the NS slots, "sfs_<p>:<k>" per bin and "privP_<P>|<Q>", "privQ_", "shared_", "fixed_" per pair, then the NG groups, "<p>" or
// "<P>|<Q>", with the indices of the current populations
const char *gph_engine_sfs_column_name(gph_engine *e, int32_t col)
{
  if (!e || !e->sf.on || col < 0 || col >= e->sf.shape.NS + e->sf.shape.NG) return nullptr;
  static const char *const cls[5] = {"sfs_", "privP_", "privQ_", "shared_", "fixed_"};
  const int NS = e->sf.shape.NS;
  const uint32_t word = (uint32_t)(col < NS ? e->sf.slot[(size_t)col] : e->sf.gdef[(size_t)(col - NS)]);
  const int kind = (int)(word >> 24);
  const std::string P = std::to_string((int)(word & 255u)), Q = std::to_string((int)((word >> 8) & 255u));
  if (col >= NS) e->sf.name = kind ? P + "|" + Q : P;
  else if (kind == SFS_BIN) e->sf.name = cls[0] + P + ":" + std::to_string((int)((word >> 16) & 255u));
  else e->sf.name = cls[kind] + P + "|" + Q;
  return e->sf.name.c_str();
}

// ---- replicate genealogies of selected loci, simulated from the sampled parameters (gph_simulate.h)
// the site level: k_predictive's site loop over the selection, on the data (observed) or on the replicate records of sample t
static int simulate_sites_launch(gph_engine *e, int observed, uint64_t *row)
{
  const int nsel = (int)e->si.sel.loci.size();
  const GphGtShape &g = e->si.gshape;
  launch_pre(e);
  return launch_grid(e, GphGrid{nsel, 1}, e->si.pshape.bd, (size_t)e->si.pshape.lds_bytes, k_predictive, e->ka, e->si.pshape, (const char *)e->dev.pages,
                     e->dev.seq, e->dev.seq_off, e->dev.P, (const int32_t *)e->si.sel.d_slot, (const uint64_t *)(e->si.d + e->si.o_skey),
                     (const uint8_t *)(e->si.d + e->si.o_pop), nsel, (int)e->L, (long long)e->si.samples, observed, (double *)(e->si.d + e->si.o_sacc), row,
                     (const char *)(e->si.d + e->si.o_rec), (int)g.img.bytes, (int)g.off[GT_O_NODES], (int)g.off[GT_O_ROOT]);
}
// the accumulators back to zero, t back to 0, and (with sites) the data's statistics formed again
static int simulate_zero(gph_engine *e)
{
  { int rcz = acc_zero(e, e->si.d, e->si.o_key); if (rcz) return rcz; }
  if (e->si.C == 0 || e->si.sel.loci.empty()) return 0;
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  { int rcl = simulate_sites_launch(e, 1, (uint64_t *)(e->si.d + e->si.o_sobs)); if (rcl) return rcl; }
  flat_launched(e, -1, 1);
  return 0;
}
static void simulate_free(gph_engine *e) { selected_free(e->si); }

int gph_engine_simulate_enable(gph_engine *e, uint64_t seed, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int32_t with_sites, int64_t max_bytes)
{
  if (!e || !e->loaded) return GPH_ESTATE;
  if (capacity_rows < 0 || !sel_valid(loci, nloci)) return GPH_EARG;
  SETDEV(e);
  simulate_free(e);
  if (capacity_rows == 0) return 0;
  const int n = e->cfg.n, Kc = e->cfg.Kc;
  GphSiShape h;
  GphGtShape g;
  GphPdShape ph;
  gph_si_shape(e->lay, h);
  gph_gt_shape(e->lay, g);
  gph_pd_shape(e->lay, ph);
  if (n > 255 || h.lds_bytes > 65536 || (with_sites && ph.lds_bytes > 65536)) {
    fprintf(stderr, "gphocs_hip: simulate: %d leaves in %d populations need byte counts above 255 or %d bytes of LDS a workgroup (65536 at most)\n",
            n, (int)e->cfg.K, (int)(h.lds_bytes > ph.lds_bytes ? h.lds_bytes : ph.lds_bytes));
    return GPH_EARG;
  }
  { int rcs = sel_alloc(e, e->si.sel, loci, nloci); if (rcs) return rcs; }
  const size_t nsel = e->si.sel.loci.size();
  const int C = with_sites ? ph.C : 0;
  int64_t maxpair = 1;
  for (int p = 0; p < Kc; p++) if ((int64_t)e->samplesPerPop[p] * e->samplesPerPop[p] > maxpair) maxpair = (int64_t)e->samplesPerPop[p] * e->samplesPerPop[p];
  for (size_t q = 0; q < nsel; q++) {
    const int64_t gl = e->si.sel.loci[q], sites = e->h_sites[(size_t)(gl - e->cfg.locus_begin)];
    if (with_sites && (sites >= ((int64_t)1 << 31) || sites * maxpair >= ((int64_t)1 << 32))) {
      fprintf(stderr, "gphocs_hip: simulate: locus %lld: %lld sites x %lld sample pairs reach 2^32: its statistics do not fit 32 bits\n",
              (long long)gl, (long long)sites, (long long)maxpair);
      simulate_free(e);
      return GPH_EARG;
    }
    e->si.sites.push_back(sites);
  }
  const size_t o_sacc = nsel * (size_t)h.W * 8, o_sobs = o_sacc + nsel * (size_t)C * GPH_PD_WORDS * 8, o_key = o_sobs + (size_t)C * 8, o_skey = o_key + nsel * 8,
               o_pop = o_skey + nsel * 8, o_rec = (o_pop + (size_t)n + 15) & ~(size_t)15, bytes = o_rec + nsel * (size_t)g.img.bytes;
  const int RC = h.RC + C;
  const int64_t need = (int64_t)bytes + (int64_t)capacity_rows * RC * 8;
  if (over_limit(need, max_bytes, "simulate: the accumulators, records and rows", "%lld loci x (%d doubles x 8 + %d statistics x 40 + 16 + %d bytes a record) + %d rows x %d x 8 + %d",
                 (long long)nsel, (int)h.W, C, (int)g.img.bytes, (int)capacity_rows, RC, (int)(C * 8 + ((n + 15) & ~15)))) {
    simulate_free(e);
    return GPH_EFULL;
  }
  if (dev_alloc((void **)&e->si.d, bytes > 0 ? bytes : 16)) { dev_clear_error(); e->si.d = nullptr; simulate_free(e); return GPH_EHIP; }
  if (rows_alloc(e->si.rows, sizeof(uint64_t), RC, capacity_rows)) { dev_clear_error(); simulate_free(e); return GPH_EHIP; }
  std::vector<uint64_t> key(2 * nsel + 1);
  for (size_t q = 0; q < nsel; q++) {
    key[q] = gph_si_locus_key(seed, (uint64_t)e->si.sel.loci[q]);
    key[nsel + q] = gph_si_locus_key(seed ^ GPH_SI_SITES, (uint64_t)e->si.sel.loci[q]);
  }
  const std::vector<uint8_t> pop = leaf_pops(e, false);
  int rc = acc_zero(e, e->si.d, bytes);                /* (the records too: a fetch before the first sample reads zeros) */
  if (!rc && nsel > 0) rc = h2d(e, e->si.d + o_key, key.data(), 2 * nsel * 8);
  if (!rc) rc = h2d(e, e->si.d + o_pop, pop.data(), (size_t)n);
  if (rc) { simulate_free(e); return rc; }
  e->si.shape = h; e->si.gshape = g; e->si.pshape = ph; e->si.C = C;
  e->si.o_sacc = o_sacc; e->si.o_sobs = o_sobs; e->si.o_key = o_key; e->si.o_skey = o_skey; e->si.o_pop = o_pop; e->si.o_rec = o_rec; e->si.bytes = bytes;
  return selected_on(e, e->si, simulate_zero);
}

// one replicate of every selected locus under the current state, queued on the engine's stream: k_simulate, then (with sites)
// the site loop on the replicate records.  The settle level is that of the time slices: the model is read from the chain state
int gph_engine_simulate_sample(gph_engine *e, int32_t iteration)
{
  if (!e || !e->initialized || !e->si.on) return GPH_ESTATE;
  const GphSiShape &h = e->si.shape;
  const int nsel = (int)e->si.sel.loci.size(), groups = (nsel + h.bd - 1) / h.bd, k = groups > 0 ? (e->si.C > 0 ? 2 : 1) : 0;
  /* (a rank without a selected locus launches nothing: its row stays 0) */
  return sample_run(e, SETTLE_CHAIN, 25, k, SmTaken{&e->si.rows, true, &e->si.iters, iteration, &e->si.samples}, [&](void *row) {
    launch_pre(e);
    int rcl = launch_grid(e, GphGrid{groups, 1}, h.bd, (size_t)h.lds_bytes, k_simulate, e->ka, h, e->si.gshape, (const char *)e->dev.pages,
                          (const int32_t *)e->si.sel.d_slot, (const uint64_t *)(e->si.d + e->si.o_key), (const uint8_t *)(e->si.d + e->si.o_pop), nsel, (int)e->L,
                          (long long)e->si.samples, (double *)e->si.d, e->si.d + e->si.o_rec, (uint64_t *)row);
    if (rcl || e->si.C == 0) return rcl;
    return simulate_sites_launch(e, 0, (uint64_t *)row + h.RC);
  });
}

int gph_engine_simulate_shape(gph_engine *e, int64_t *selected, int32_t *stats, int32_t *site_stats, int32_t *row_columns, int32_t *record_bytes,
                              int64_t *samples, int32_t *rows_held)
{
  if (!e) return GPH_EARG;
  const bool on = e->si.on;
  if (selected) *selected = on ? (int64_t)e->si.sel.loci.size() : 0;
  if (stats) *stats = on ? e->si.shape.M : 0;
  if (site_stats) *site_stats = on ? e->si.C : 0;
  if (row_columns) *row_columns = on ? e->si.shape.RC + e->si.C : 0;
  if (record_bytes) *record_bytes = on ? e->si.gshape.img.bytes : 0;
  if (samples) *samples = on ? e->si.samples : 0;
  if (rows_held) *rows_held = on ? e->si.rows.fill : 0;
  return 0;
}

int gph_engine_simulate_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count) { return selected_out(e, e ? &e->si : nullptr, out, max_loci, count); }

// acc [selected][5 M + 1] (gt, eq, sx, sy, sy2 per statistic, then the failed replicates), site_acc [selected][C][5] (obs, gt, eq,
// s1, s2; may be null), sites [selected] (may be null)
int gph_engine_simulate_fetch_loci(gph_engine *e, double *acc, double *site_acc, int64_t *sites, int32_t reset)
{
  if (!e) return GPH_EARG;
  if (!e->si.on) return GPH_ESTATE;
  const size_t nsel = e->si.sel.loci.size();
  if (nsel > 0 && !acc) return GPH_EARG;
  SETDEV(e);
  if (nsel > 0) { int rc = pull_rows(e, acc, e->si.d, e->si.o_sacc); if (rc) return rc; }
  if (nsel > 0 && site_acc && e->si.C > 0) { int rc = d2h(e, site_acc, e->si.d + e->si.o_sacc, e->si.o_sobs - e->si.o_sacc); if (rc) return rc; }
  if (sites) for (size_t q = 0; q < nsel; q++) sites[q] = e->si.sites[q];
  return reset ? selected_zero(e, e->si) : 0;
}

// the rows taken since the last fetch ([rows][RC + C], with their iterations) and the data's totals (observed [C], may be null);
// the row buffer is empty again
int gph_engine_simulate_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *rows_out, uint64_t *observed, int32_t max_rows, int32_t *rows)
{
  if (!e || !rows || max_rows < 0 || ((!rows_out || !iters) && max_rows > 0)) return GPH_EARG;
  if (!e->si.on) return GPH_ESTATE;
  SmRows &b = e->si.rows;
  if (max_rows < b.fill) return GPH_EARG;
  SETDEV(e);
  if (observed && e->si.C > 0) { int rc = pull_rows(e, observed, e->si.d + e->si.o_sobs, (size_t)e->si.C * 8); if (rc) return rc; }
  return rows_iters_fetch(e, b, e->si.iters, iters, rows_out, 0, true, rows);
}

// the replicate records of the latest sample, out [selected][record_bytes] in the layout of a gene-trees record; offsets as
// gph_engine_gene_trees_shape hands them out (may be null)
int gph_engine_simulate_fetch_records(gph_engine *e, void *out, int32_t *offsets)
{
  if (!e) return GPH_EARG;
  if (!e->si.on) return GPH_ESTATE;
  const size_t nsel = e->si.sel.loci.size();
  if (nsel > 0 && !out) return GPH_EARG;
  SETDEV(e);
  if (offsets) for (int k = 0; k < GT_O_COUNT; k++) offsets[k] = e->si.gshape.off[k];
  if (nsel > 0) return pull_rows(e, out, e->si.d + e->si.o_rec, nsel * (size_t)e->si.gshape.img.bytes);
  return 0;
}

// which 0: the M statistics -- tmrca, length, genLnL, coal_<p>, mig_<b>; 1: the columns of a row -- s.coal_<p>, s.mig_<b>, r.coal_<p>,
// r.mig_<b>, gt.tmrca, gt.length, gt.genLnL, failed, then r.<site statistic>; 2: the C site statistics (gph_engine_predictive_column_name)
const char *gph_engine_simulate_column_name(gph_engine *e, int32_t which, int32_t col)
{
  if (!e || !e->si.on || col < 0) return nullptr;
  const int K = e->cfg.K, B = e->cfg.B, Kc = e->cfg.Kc;
  static const char *const fixed[SI_FIXED] = {"tmrca", "length", "genLnL"};
  auto stat = [&](int c) { return c < SI_FIXED ? std::string(fixed[c]) : c < SI_FIXED + K ? "coal_" + std::to_string(c - SI_FIXED) : "mig_" + std::to_string(c - SI_FIXED - K); };
  auto site = [&](int c) {
    if (c == 0) return std::string("seg");
    for (int p = 0; p < Kc; p++)
      for (int q = p; q < Kc; q++)
        if (gph_pd_pair(Kc, p, q) == c) return "diff_" + std::to_string(p) + "|" + std::to_string(q);
    return std::string("?");
  };
  if (which == 0) {
    if (col >= e->si.shape.M) return nullptr;
    e->si.name = stat(col);
  } else if (which == 1) {
    if (col >= e->si.shape.RC + e->si.C) return nullptr;
    const int KB = K + B;
    if (col < 2 * KB) e->si.name = std::string(col < KB ? "s." : "r.") + stat(SI_FIXED + col % KB);
    else if (col < 2 * KB + SI_FIXED) e->si.name = std::string("gt.") + fixed[col - 2 * KB];
    else if (col == 2 * KB + SI_FIXED) e->si.name = "failed";
    else e->si.name = "r." + site(col - e->si.shape.RC);
  } else if (which == 2) {
    if (col >= e->si.C) return nullptr;
    e->si.name = site(col);
  } else return nullptr;
  return e->si.name.c_str();
}

// ---- two engines exchange their chain states (Metropolis-coupled chains)
#include "gph_exchange.h"

} // extern "C"
