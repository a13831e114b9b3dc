// gph_backend.h -- the one place in the engine's host code that knows which build it is in.
//
// gph_engine.hip serves two builds from one text: the gfx950 library, and the host-emulation library (-DGPH_HOSTEMU,
// tests/hostemu: the CPU parity suite and the sanitizer builds).  Host emulation is a fake that the tests substitute for
// the GPU; this file is its interface.  Both halves of the one conditional below define the same names with the same
// signatures -- memory and stream, the chain state's two copies, the engine's own resources, the reduction / stage paths
// (a fixed-shape tree with a last-block ticket on the device, a serial loop on the host) and the launch functions -- and
// everything below the include in gph_engine.hip is one text for both.
//
// Included by gph_engine.hip after the kernels and gph_engine_state; it completes the engine object (struct gph_engine)
// with the members only one build has.
#pragma once

// blocks of a flat launch (launch_grid): x, and y for the samplers that tile a chunk
struct GphGrid { int x, y; };
// what the reduction probe (debug_reduce, tests only) fills its buffers with before anything is folded: a quiet NaN with a
// recognisable payload (info[8], info[9] of the probe: its low and high words)
static const uint64_t GPH_RED_POISON = 0x7FF8DEADBEEF0BADull;

// What a launch counts -- host_stats(), class_stats() and last_kernel_ms are asserted by tests, so the rules are kept as
// they grew, and they are not the same in the two builds:
//
//   site                          device build                           host build
//   launch_loci                   n_launches += one per launch group     n_launches += one per call
//   launch_wave                   not added to n_launches                not added to n_launches
//   sample_end (k launches)       n_launches += k, sets last_which       neither
//   apply_list (flat_launched)    n_launches += 1                        nothing
//   rng_ahead_launch / _side      n_launches += 1, cls_launches[18] += 1 n_launches += 1, cls_launches[18] += 1
//                                 (last_which is left alone: the sweep that follows sets it)
//   cls_launches[cls]             += 1 per call                          += 1 per call
//
// launch_loci and launch_wave set last_which in both builds; launch_grid itself counts nothing (its callers do, above);
// the reduction and stage kernels of the device build add one to n_launches each.

#ifdef GPH_HOSTEMU
// ================================================================ host emulation
#define SETDEV(e) ((void)0)

struct gph_engine : gph_engine_state {
  std::vector<char> lds;             // the dynamic LDS of the block that is running
};

static int dev_alloc(void **p, size_t bytes) { *p = calloc(1, bytes ? bytes : 1); return *p ? 0 : GPH_EHIP; }
static void dev_free(void *p) { free(p); }
static int h2d(gph_engine *, void *d, const void *h, size_t n) { memcpy(d, h, n); return 0; }
static int d2h(gph_engine *, void *h, const void *d, size_t n) { memcpy(h, d, n); return 0; }
static int acc_zero(gph_engine *, void *p, size_t bytes) { if (p) memset(p, 0, bytes); return 0; }
static int stream_sync(gph_engine *e) { e->n_syncs++; return 0; }
static int collect_times(gph_engine *) { return 0; }
static int tm_begin(gph_engine *, int) { return -1; }
static void tm_end(gph_engine *, int) {}
static int push_G(gph_engine *e) { e->G_dirty = false; return 0; }     /* one copy of the chain state: G_d == G_h */
static int pull_G(gph_engine *e) { e->n_syncs++; return 0; }
static int pull_row(gph_engine *e) { memcpy(e->h_red, e->d_red, sizeof(double) * GPH_RED_ROW); e->n_syncs++; return 0; }
static bool resident(const gph_engine *) { return false; }
static int flush_pending(gph_engine *) { return 0; }
static int stage_defer(gph_engine *, int, int, int, bool &queued) { queued = false; return 0; }
static void flat_launched(gph_engine *, int, int) {}     /* k flat launches of class cls (-1: none) went out: not counted here */
static void dev_clear_error() {}
// placement B of k_rng_ahead needs resident mode: never here
static int rng_ahead_side(gph_engine *, GphGrid) { return 0; }
static int rng_ahead_wait(gph_engine *) { return 0; }
static void rng_ahead_drain(gph_engine *) {}
// two engines exchange their pages (gph_exchange.h): one thread of launches here, nothing to order
static int exchange_order(gph_engine *, gph_engine *) { return 0; }
// R engines' clade tables are read by one kernel of engines[0] (gph_engine_clades_compare): nothing to order here either
static int compare_order_before(gph_engine *const *, int) { return 0; }
static int compare_order_after(gph_engine *const *, int) { return 0; }
// a sampler's result -> the caller's buffer, with the call's one host synchronisation
static int pull_rows(gph_engine *e, void *h, const void *d, size_t n) { memcpy(h, d, n); e->n_syncs++; return 0; }

// the serial fold of one section over L loci into `red` (that section of a reduced row): sum, minimum and maximum per column,
// the loci in index order.  The engine (reduce_local) and the reduction probe (debug_reduce) both run this text
static void reduce_serial(const double *out, const double *stats, int64_t L, int sec, int ncols, double *red)
{
  for (int c = 0; c < ncols; c++) {
    double s = 0, mn = 1e300, mx = -1e300;
    for (int64_t g = 0; g < L; g++) {
      double v;
      if (sec == 0) v = out[(size_t)g * GPH_OUT_SLOTS + c];
      else v = stats[(size_t)g * ncols + c];
      s += v; mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    }
    red[c] = s; red[GPH_RED_COLS + c] = mn; red[2 * GPH_RED_COLS + c] = mx;
  }
}
static int reduce_local(gph_engine *e, int sec, int ncols)
{
  double *red = e->d_red + sec * GPH_RED_STRIDE;
  reduce_serial(e->dev.out, e->dev.stats, e->L, sec, ncols, red);
  red[3 * GPH_RED_COLS] = (double)*e->dev.err;
  return 0;
}
// the reduction probe (gph_debug_reduce_ in gph_engine.hip): launch i folds input set i % nsets into row i with the engine's
// serial loop; the error word goes where the device's final pass puts it (section 0's first trailing word)
static int debug_reduce(const double *out0, const double *stats1, int64_t L, int nc0, int nc1, int nsets, int err_word, int launches,
                        double *rows, int32_t *info, int)
{
  for (size_t i = 0; i < (size_t)launches * GPH_RED_ROW; i++) memcpy(rows + i, &GPH_RED_POISON, 8);
  for (int i = 0; i < launches; i++) {
    const size_t set = (size_t)(i % nsets);
    double *red = rows + (size_t)i * GPH_RED_ROW;
    if (nc0 > 0) reduce_serial(out0 + set * L * GPH_OUT_SLOTS, nullptr, L, 0, nc0, red);
    if (nc1 > 0) reduce_serial(nullptr, stats1 + set * L * nc1, L, 1, nc1, red + GPH_RED_STRIDE);
    red[3 * GPH_RED_COLS] = (double)err_word;
  }
  if (info) {     /* no tree here: no sub-sequences, no unroll, no ticket */
    const int32_t v[10] = {GPH_RED_COLS, GPH_RED_STRIDE, GPH_RED_ROW, GPH_RED_BLOCKS, 0, 0, GPH_OUT_SLOTS, 0,
                           (int32_t)(uint32_t)GPH_RED_POISON, (int32_t)(uint32_t)(GPH_RED_POISON >> 32)};
    memcpy(info, v, sizeof v);
  }
  return 0;
}

// ---- engine resources
static int backend_open(gph_engine *e)
{
  e->G_h = (GphGlobal *)calloc(1, sizeof(GphGlobal));
  e->G_d = e->G_h;
  e->h_red = (double *)calloc(GPH_RED_ROW, sizeof(double));
  e->d_red = (double *)calloc(GPH_RED_ROW, sizeof(double));
  e->d_gather = e->d_red;
  return 0;
}
static void backend_close(gph_engine *e) { free(e->h_red); free(e->G_h); }
static int wide_terms_bytes(int P) { return 8 * P; }     /* the host form keeps the root reduction's per-pattern terms behind the block */
static int zero_error_word(gph_engine *e) { if (e->dev.err) *e->dev.err = 0; return 0; }
static int loci_loaded(gph_engine *) { return 0; }
static int scan_lds_limit(gph_engine *) { return 0; }
static void runtime_version(char *buf, size_t n) { snprintf(buf, n, "host emulation (no HIP runtime)"); }
#ifdef GPH_BOUNDS
static int oob_take(int32_t *where) { *where = gph_oob_word; gph_oob_word = 0; return 0; }
#endif

// ---- launches: on the host a kernel takes its block first (GPH_KERNEL: the block index; a flat kernel, GPH_FLAT in
// gph_sampler.h: GphBlk) and is called once per block, one block after the other, with a zeroed scratch buffer for its dynamic
// LDS.  A flat kernel is the device text itself, run lane by lane between its barriers; only k_rng_ahead has a host form of its own
static void launch_pre(gph_engine *e)
{
  g_model = e->G_h->model; g_lay = e->lay; gph_G_emu = e->G_h;
  GPH_KA_MODEL(e->ka, e); e->ka.lay = e->lay; e->ka.G = e->G_h;
}
template <class... P, class... A>
static int launch_loci(gph_engine *e, int cls, void (*kernel)(int, GphKargs, GphDev, int, P...), A &&...args)
{
  launch_pre(e);
  for (auto &bk : e->buckets) {
    e->lds.assign(bk.lds_bytes + 8 * e->lay.Pmax + 64, 0);     /* the host form keeps per-pattern terms for every P */
    gph_sm = e->lds.data();
    for (int b = 0; b < bk.count; b++) kernel(b, e->ka, e->dev, bk.j0, static_cast<P>(args)...);
  }
  e->last_which = cls; e->cls_launches[cls] += 1; e->n_launches++;
  return 0;
}
template <class... P, class... A>
static int launch_wave(gph_engine *e, int cls, void (*kernel)(int, GphKargs, GphDev, int, P...), size_t lds_bytes, A &&...args)
{
  launch_pre(e);
  e->lds.assign(lds_bytes + 64, 0);
  gph_sm = e->lds.data();
  kernel(0, e->ka, e->dev, 0, static_cast<P>(args)...);
  e->last_which = cls; e->cls_launches[cls] += 1;
  return 0;
}
template <class... P, class... A>
static int run_blocks(std::vector<char> &lds, GphGrid grid, int block, size_t lds_bytes, void (*kernel)(GphBlk, P...), A &&...args)
{
  for (int x = 0; x < grid.x; x++)
    for (int y = 0; y < grid.y; y++) {
      lds.assign(lds_bytes + 64, 0);
      kernel(GphBlk{x, y, block, lds.data()}, static_cast<P>(args)...);
    }
  return 0;
}
template <class... P, class... A>
static int launch_grid(gph_engine *e, GphGrid grid, int block, size_t lds_bytes, void (*kernel)(GphBlk, P...), A &&...args)
{
  return run_blocks(e->lds, grid, block, lds_bytes, kernel, args...);
}

static int debug_math(const double *x, const double *y, int n, double *out, int, int which = 0)
{
  GphKargs ka;
  memset(&ka, 0, sizeof ka);
  fill_math_constants(ka);
  std::vector<char> lds;
  return run_blocks(lds, GphGrid{(n + GPH_FLAT_THREADS - 1) / GPH_FLAT_THREADS, 1}, GPH_FLAT_THREADS, 0, which ? k_debug_accept : k_debug_math, ka, x, y, n, out);
}

#else
// ================================================================ gfx950
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "gphocs_hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); return GPH_EHIP; } } while (0)
#define SETDEV(e) do { if (hipSetDevice((e)->cfg.device) != hipSuccess) return GPH_EHIP; } while (0)

struct gph_engine : gph_engine_state {
  unsigned *d_ticket = nullptr;                  // last-block ticket of the fused reduction
  // resident mode: reductions and stages requested since the last launch; they go out as ONE kernel when the next
  // per-locus kernel is launched (or the host needs the result)
  int pend_nc0 = 0, pend_nc1 = 0;
  GphStageList pend_sl = {0, {0}, {0}};
  int pend_iteration = 0;
  hipStream_t stream = nullptr;
  // the launch group of the pattern-rich loci (P > 64: a few per cent of a data set, long wavefronts) runs NEXT TO the
  // main group on a stream of its own, forked from and joined to the engine's stream with two events per launch point:
  // one after the other, the small group cost a wavefront lifetime of its own per kernel class (configs[4]: 5 % of a sweep)
  hipStream_t stream_wide = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_stream = true;            // GPH_SIDE_STREAM=0: the groups one after the other on the engine's stream (A/B, tests)
  // k_rng_ahead for the NEXT sweep (placement B): on a stream of its own behind the sweep kernel, next to the tau / mixing
  // kernels; the next sweep kernel waits for ev_ra_done
  hipStream_t stream_ra = nullptr;
  hipEvent_t ev_ra_go = nullptr, ev_ra_done = nullptr;
  hipEvent_t ev_xchg = nullptr;       // what this engine's stream held when its pages went to another engine (gph_exchange.h)
  hipEvent_t ev_cmp = nullptr;        // gph_engine_clades_compare: what this engine's stream held in front of / behind the kernel
  struct Tm { hipEvent_t a, b; int which; };
  std::vector<Tm> tm;                // event pairs of the launches since the last synchronisation
  size_t tm_used = 0;
};

static int dev_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 16) == hipSuccess ? 0 : GPH_EHIP; }
static void dev_free(void *p) { if (p) (void)hipFree(p); }
// a failed allocation that the caller survives: the runtime keeps its last error until somebody takes it, and the check
// after the next launch (launch_on) would report it
static void dev_clear_error() { (void)hipGetLastError(); }
// elapsed times of the launches bracketed since the last synchronisation (the stream is idle: every event is complete)
static int collect_times(gph_engine *e)
{
  for (size_t i = 0; i < e->tm_used; i++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->tm[i].a, e->tm[i].b) == hipSuccess) { e->last_ms[e->tm[i].which] = ms; e->cls_ms[e->tm[i].which] += ms; }
  }
  e->tm_used = 0;
  return 0;
}
static int stream_sync(gph_engine *e)
{
  HIPCHK(hipStreamSynchronize(e->stream));
  e->n_syncs++;
  return collect_times(e);
}
static int h2d(gph_engine *e, void *d, const void *h, size_t n)
{
  HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}
static int d2h(gph_engine *e, void *h, const void *d, size_t n)
{
  HIPCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}
// a buffer on the device back to zero, queued on the engine's stream (nothing for a null pointer: a sampler that is off)
static int acc_zero(gph_engine *e, void *p, size_t bytes)
{
  if (p) HIPCHK(hipMemsetAsync(p, 0, bytes, e->stream));
  return 0;
}
// HIP events on the engine's own stream bracket the launches of a timed class; no host synchronisation here
static int tm_begin(gph_engine *e, int which)
{
  if (!((e->timing_mask >> which) & 1)) return -1;
  if (e->tm_used == e->tm.size()) {
    gph_engine::Tm t;
    if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) return -1;
    e->tm.push_back(t);
  }
  e->tm[e->tm_used].which = which;
  (void)hipEventRecord(e->tm[e->tm_used].a, e->stream);
  return (int)e->tm_used++;
}
static void tm_end(gph_engine *e, int slot) { if (slot >= 0) (void)hipEventRecord(e->tm[slot].b, e->stream); }
// host mirror -> HBM: a synchronous copy, the mirror may be modified again as soon as this returns
static int push_G(gph_engine *e)
{
  e->G_dirty = false;
  return h2d(e, e->G_d, e->G_h, sizeof(GphGlobal));
}
// HBM -> host mirror, with a host synchronisation (the end of an iteration in resident mode)
static int pull_G(gph_engine *e)
{
  HIPCHK(hipMemcpyAsync(e->G_h, e->G_d, sizeof(GphGlobal), hipMemcpyDeviceToHost, e->stream));
  { int rcs = stream_sync(e); if (rcs) return rcs; }
  e->mirror_current = true;
  return 0;
}
// this rank's reduced row -> its pinned copy, with a host synchronisation (host mode)
static int pull_row(gph_engine *e)
{
  HIPCHK(hipMemcpyAsync(e->h_red, e->d_red, sizeof(double) * GPH_RED_ROW, hipMemcpyDeviceToHost, e->stream));
  return stream_sync(e);
}
// are the decisions above the loci taken on the device?  Yes unless something forces a host synchronisation at every
// reduction point anyway: a caller-supplied all-reduce hook, the host shared-memory exchange of ranks that share a
// GPU, or GPH_HOST_DECISIONS=1 (tests compare the two modes); never in the host-emulation build
static bool resident(const gph_engine *e)
{
  if (e->force_host || e->allreduce || e->var_rates) return false;
  if (e->comm && !gph_comm_on_stream(e->comm)) return false;
  return true;
}
// k flat launches of class cls (-1: none, apply_list) went out
static void flat_launched(gph_engine *e, int cls, int k) { e->n_launches += k; if (cls >= 0) e->last_which = cls; }

template <class... P, class... A>
static int launch_on(hipStream_t stream, GphGrid grid, int block, size_t lds_bytes, void (*kernel)(P...), A &&...args)
{
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid.x, (unsigned)grid.y), dim3((unsigned)block), lds_bytes, stream, static_cast<P>(args)...);
  HIPCHK(hipGetLastError());
  return 0;
}
static void launch_pre(gph_engine *e) { GPH_KA_MODEL(e->ka, e); e->ka.lay = e->lay; e->ka.G = e->G_d; }
// k_rng_ahead for the sweep AFTER the one just launched on the engine's stream: forked behind it onto its own stream
static int rng_ahead_side(gph_engine *e, GphGrid grid)
{
  if (!e->stream_ra) {
    if (hipStreamCreateWithFlags(&e->stream_ra, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_ra_go, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_ra_done, hipEventDisableTiming) != hipSuccess) return GPH_EHIP;
  }
  HIPCHK(hipEventRecord(e->ev_ra_go, e->stream));
  HIPCHK(hipStreamWaitEvent(e->stream_ra, e->ev_ra_go, 0));
  { int rcl = launch_on(e->stream_ra, grid, GPH_WAVE, 0, k_rng_ahead, e->ka, e->dev); if (rcl) return rcl; }
  HIPCHK(hipEventRecord(e->ev_ra_done, e->stream_ra));
  return 0;
}
// the engine's stream goes on when that pass has finished
static int rng_ahead_wait(gph_engine *e) { HIPCHK(hipStreamWaitEvent(e->stream, e->ev_ra_done, 0)); return 0; }
// nothing of it in flight any more (before its buffers or the pages are released)
static void rng_ahead_drain(gph_engine *e) { if (e->stream_ra) (void)hipStreamSynchronize(e->stream_ra); }
// two engines are about to exchange their pages (gph_exchange.h): whatever either stream still holds for the pages it gives
// away -- a finish kernel just queued, a pass of k_rng_ahead reading them on its own stream -- comes before the first launch
// of the engine that receives them.  Events only: the host does not wait, and no kernel of one engine waits for a kernel of
// the other.  Both records go out before either wait, so neither stream waits for work queued behind the exchange.  A pass of
// k_rng_ahead whose draws are dropped also comes before its own engine's next pass, which writes the same buffers.
static int exchange_order(gph_engine *a, gph_engine *b)
{
  gph_engine *const p[2] = {a, b};
  for (gph_engine *x : p) {
    if (!x->ev_xchg) HIPCHK(hipEventCreateWithFlags(&x->ev_xchg, hipEventDisableTiming));
    HIPCHK(hipEventRecord(x->ev_xchg, x->stream));
  }
  for (int i = 0; i < 2; i++) {
    gph_engine *x = p[i], *y = p[1 - i];
    HIPCHK(hipStreamWaitEvent(y->stream, x->ev_xchg, 0));
    if (x->ra_b_valid) {
      HIPCHK(hipStreamWaitEvent(y->stream, x->ev_ra_done, 0));
      HIPCHK(hipStreamWaitEvent(x->stream, x->ev_ra_done, 0));
    }
  }
  return 0;
}
// R engines' clade tables are read by one kernel on the stream of p[0] (gph_engine_clades_compare).  Before it: what every other
// stream holds -- a k_clades that is still writing its tables -- comes first.  Behind it: the others' next k_clades waits until
// the tables have been read.  Events only, as above: the host does not wait here, no kernel waits for another engine's kernel,
// and the device is never synchronised as a whole.
static int compare_event(gph_engine *x)
{
  if (!x->ev_cmp) HIPCHK(hipEventCreateWithFlags(&x->ev_cmp, hipEventDisableTiming));
  HIPCHK(hipEventRecord(x->ev_cmp, x->stream));
  return 0;
}
static int compare_order_before(gph_engine *const *p, int R)
{
  for (int r = 1; r < R; r++) { int rc = compare_event(p[r]); if (rc) return rc; }
  for (int r = 1; r < R; r++) HIPCHK(hipStreamWaitEvent(p[0]->stream, p[r]->ev_cmp, 0));
  return 0;
}
static int compare_order_after(gph_engine *const *p, int R)
{
  { int rc = compare_event(p[0]); if (rc) return rc; }
  for (int r = 1; r < R; r++) HIPCHK(hipStreamWaitEvent(p[r]->stream, p[0]->ev_cmp, 0));
  return 0;
}
// a sampler's result -> the caller's buffer, with the call's one host synchronisation (and the times of what it waited for)
static int pull_rows(gph_engine *e, void *h, const void *d, size_t n)
{
  HIPCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, e->stream));
  return stream_sync(e);
}
// a flat kernel on the engine's stream; what is pending and what is counted is the caller's business (sample_begin / _end,
// apply_list, the reductions below)
template <class... P, class... A>
static int launch_grid(gph_engine *e, GphGrid grid, int block, size_t lds_bytes, void (*kernel)(P...), A &&...args)
{
  return launch_on(e->stream, grid, block, lds_bytes, kernel, args...);
}

// ---- the reductions and the stages above the loci
// resident mode: everything requested since the last per-locus launch -- the reduction(s) of its outputs and the stages
// above the loci -- as one kernel (single rank), or reduction -> RCCL all-gather -> stages (several ranks)
static int flush_pending(gph_engine *e)
{
  const bool red = e->pend_nc0 > 0 || e->pend_nc1 > 0;
  if (!red && e->pend_sl.n == 0) return 0;
  const GphStageList sl = e->pend_sl;
  const int nc0 = e->pend_nc0, nc1 = e->pend_nc1;
  e->pend_nc0 = e->pend_nc1 = 0;
  e->pend_sl.n = 0;
  const bool multi = e->comm && gph_comm_world(e->comm) > 1;
  int rc;
  launch_pre(e);
  if (red) {
    const int fuse = sl.n > 0 && !multi;
    if ((rc = launch_grid(e, GphGrid{GPH_RED_BLOCKS, 1}, GPH_RED_THREADS, 0, k_reduce_stage, e->ka, e->dev, nc0, nc1, e->d_part, e->d_ticket,
                          e->d_red, fuse, sl, e->pend_iteration))) return rc;
    e->n_launches++;
    if (e->comm) {     /* (a one-rank communicator too: its row is already everybody's, the collective is counted all the same) */
      if (gph_comm_allgather_stream(e->comm, e->d_red, e->d_gather, GPH_RED_ROW, (void *)e->stream)) return GPH_EHIP;
      e->n_collectives++;
    }
    if (fuse) return 0;
  }
  if (sl.n > 0) {
    const double *rows = e->comm ? e->d_gather : e->d_red;
    if ((rc = launch_grid(e, GphGrid{1, 1}, GPH_RED_THREADS, 0, k_global, e->ka, rows, world_of(e), sl, e->pend_iteration))) return rc;
    e->n_launches++;
  }
  return 0;
}
// reduce the per-locus outputs (section 0) or the page statistics (section 1) over the local loci into this rank's row
static int reduce_local(gph_engine *e, int sec, int ncols)
{
  if (resident(e)) {
    /* lazily: fused with the stages that consume the row (flush_pending) */
    if (e->pend_sl.n > 0) { int rcf = flush_pending(e); if (rcf) return rcf; }
    if (sec == 0) e->pend_nc0 = ncols; else e->pend_nc1 = ncols;
    return 0;
  }
  int rc;
  if ((rc = flush_pending(e))) return rc;
  GphStageList none = {0, {0}, {0}};
  launch_pre(e);
  if ((rc = launch_grid(e, GphGrid{GPH_RED_BLOCKS, 1}, GPH_RED_THREADS, 0, k_reduce_stage, e->ka, e->dev, sec == 0 ? ncols : 0, sec == 1 ? ncols : 0,
                        e->d_part, e->d_ticket, e->d_red, 0, none, 0))) return rc;
  e->n_launches += 1;
  return 0;
}
// a stage above the loci in resident mode: queued, it goes out fused with the reduction before it (and the stages next to
// it) at the next launch.  Host mode (queued = false): what is pending goes out, the caller runs the stage on the mirror
static int stage_defer(gph_engine *e, int stage, int arg, int iteration, bool &queued)
{
  queued = resident(e);
  if (!queued) return flush_pending(e);
  if (e->pend_sl.n == 6) { int rcf = flush_pending(e); if (rcf) return rcf; }
  e->pend_sl.stage[e->pend_sl.n] = stage;
  e->pend_sl.arg[e->pend_sl.n] = arg;
  e->pend_sl.n++;
  e->pend_iteration = iteration;
  e->mirror_current = false;     /* the stage writes the chain state on the device: the mirror is stale until pull_G */
  return 0;
}

// ---- launches of the per-locus kernels.  One dispatch covers every locus with at most one pattern per lane (slots in
// decreasing P: longest wavefronts first), a second one the rare loci with more (they also need the per-pattern terms
// array in LDS), forked onto the side stream and joined again.  What is pending goes first; no host synchronisation here.
template <class... P, class... A>
static int launch_loci(gph_engine *e, int cls, void (*kernel)(GphKargs, GphDev, int, P...), A &&...args)
{
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  launch_pre(e);
  const int tms = tm_begin(e, cls);
  const size_t nb = e->buckets.size();
  const bool fork = e->side_stream && nb >= 2;
  if (fork) { HIPCHK(hipEventRecord(e->ev_fork, e->stream)); HIPCHK(hipStreamWaitEvent(e->stream_wide, e->ev_fork, 0)); }
  for (size_t bi = 0; bi < nb; bi++) {
    const gph_engine::Bucket &bk = e->buckets[bi];
    e->ka.lay.dyn_bytes = bk.lds_bytes;
    { int rcl = launch_on(fork && bi + 1 < nb ? e->stream_wide : e->stream, GphGrid{bk.count, 1}, GPH_WAVE, bk.lds_bytes + e->lds_pad[cls],
                          kernel, e->ka, e->dev, bk.j0, args...); if (rcl) return rcl; }
    e->n_launches++;
  }
  if (fork) { HIPCHK(hipEventRecord(e->ev_join, e->stream_wide)); HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0)); }
  tm_end(e, tms);
  e->last_which = cls; e->cls_launches[cls] += 1;
  return 0;
}
// one single-wave workgroup with its own dynamic-LDS size (the serial scan of UpdateLocusRate)
template <class... P, class... A>
static int launch_wave(gph_engine *e, int cls, void (*kernel)(GphKargs, GphDev, int, P...), size_t lds_bytes, A &&...args)
{
  { int rcf = flush_pending(e); if (rcf) return rcf; }
  launch_pre(e);
  const int tms = tm_begin(e, cls);
  { int rcl = launch_on(e->stream, GphGrid{1, 1}, GPH_WAVE, lds_bytes, kernel, e->ka, e->dev, 0, args...); if (rcl) return rcl; }
  tm_end(e, tms);
  e->last_which = cls; e->cls_launches[cls] += 1;
  return 0;
}

// ---- engine resources
static int fill_math_tables(GphKargs &ka)
{
  void *p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(gph_log_t_d)) != hipSuccess) return 1;
  ka.log_t = (const double *)p;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(gph_exp_t_d)) != hipSuccess) return 1;
  ka.exp_t = (const uint64_t *)p;
  return 0;
}
// streams, events, the pinned mirror of the chain state and of the reduced row, their copies in HBM, the ticket
static int backend_open(gph_engine *e)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= e->cfg.device) {
    fprintf(stderr, "gphocs_hip: no usable HIP device %d (found %d) -- this library has no CPU path\n", e->cfg.device, ndev);
    return GPH_EHIP;
  }
  if (hipSetDevice(e->cfg.device) != hipSuccess || fill_math_tables(e->ka)) {
    fprintf(stderr, "gphocs_hip: cannot resolve the device math tables\n");
    return GPH_EHIP;
  }
  if (const char *ov = getenv("GPH_SIDE_STREAM")) e->side_stream = atoi(ov) != 0;
  if (hipStreamCreate(&e->stream) != hipSuccess ||
      hipStreamCreateWithFlags(&e->stream_wide, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc((void **)&e->G_h, sizeof(GphGlobal), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void **)&e->G_d, sizeof(GphGlobal)) != hipSuccess ||
      hipHostMalloc((void **)&e->h_red, sizeof(double) * GPH_RED_ROW * 64, hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void **)&e->d_red, sizeof(double) * GPH_RED_ROW) != hipSuccess ||
      hipMemset(e->d_red, 0, sizeof(double) * GPH_RED_ROW) != hipSuccess ||
      hipMalloc((void **)&e->d_ticket, 64) != hipSuccess || hipMemset(e->d_ticket, 0, 64) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) return GPH_EHIP;
  e->d_gather = e->d_red;
  return 0;
}
static void backend_close(gph_engine *e)
{
  dev_free(e->G_d);
  dev_free(e->d_ticket);
  if (e->h_red) (void)hipHostFree(e->h_red);
  if (e->G_h) (void)hipHostFree(e->G_h);
  for (auto &t : e->tm) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  if (e->ev_xchg) (void)hipEventDestroy(e->ev_xchg);
  if (e->ev_cmp) (void)hipEventDestroy(e->ev_cmp);
  if (e->ev_ra_go) (void)hipEventDestroy(e->ev_ra_go);
  if (e->ev_ra_done) (void)hipEventDestroy(e->ev_ra_done);
  if (e->stream_ra) (void)hipStreamDestroy(e->stream_ra);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->stream_wide) (void)hipStreamDestroy(e->stream_wide);
  if (e->stream) (void)hipStreamDestroy(e->stream);
}
static int wide_terms_bytes(int) { return 0; }     /* the root sum of the pattern-rich loci needs no terms array on the device */
static int zero_error_word(gph_engine *e)
{
  return hipMemset(e->dev.err, 0, sizeof(int32_t)) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess ? GPH_EHIP : 0;
}
// the loci are in HBM: the per-locus kernels use up to the wide group's dynamic LDS size; allow > 64 KiB
static int loci_loaded(gph_engine *e)
{
  const void *ks[] = {(const void *)k_init, (const void *)k_sweep, (const void *)k_sweep_heated, (const void *)k_tau_eval, (const void *)k_tau_finish,
                      (const void *)k_mix_eval, (const void *)k_mix_finish,
                      (const void *)k_sync, (const void *)k_check, (const void *)k_lrate_apply, (const void *)k_lrate_prep,
                      (const void *)k_unit};
  int pad_max = 0;
  if (const char *pe = getenv("GPH_LDS_PAD")) {
    for (const char *q = pe; *q;) {
      int w = -1, by = 0;
      if (sscanf(q, "%d:%d", &w, &by) == 2 && w >= 0 && w < 16 && by >= 0) { e->lds_pad[w] = by; pad_max = by > pad_max ? by : pad_max; }
      while (*q && *q != ',') q++;
      if (*q == ',') q++;
    }
  }
  /* image + the largest launch group's block (+ an experiment's padding) must fit the CU's LDS: said with the numbers, whatever
   * made it too big (the message used to blame GPH_LDS_PAD for a block that was too large by itself) */
  if (e->lay.lds_bytes + pad_max + (int)sizeof(GphLds) > 160 * 1024) {
    fprintf(stderr, "gphocs_hip: %d-byte image + %d-byte sequence block%s = %d bytes of LDS per locus, the CU has %d%s\n", (int)sizeof(GphLds),
            e->lay.lds_bytes, pad_max ? " + GPH_LDS_PAD" : "", e->lay.lds_bytes + pad_max + (int)sizeof(GphLds), 160 * 1024,
            getenv("GPH_HUGE_LDS") ? " (GPH_HUGE_LDS is set: lower it, the block then stays in HBM)" : "");
    return GPH_EARG;
  }
  for (auto k : ks) HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, e->lay.lds_bytes + pad_max));
  return 0;
}
static int scan_lds_limit(gph_engine *e)
{
  HIPCHK(hipFuncSetAttribute((const void *)k_lrate_scan, hipFuncAttributeMaxDynamicSharedMemorySize, e->lr_lds_bytes));
  return 0;
}
static void runtime_version(char *buf, size_t n)
{
  int rt = 0, dr = 0;
  if (hipRuntimeGetVersion(&rt) != hipSuccess) rt = -1;
  if (hipDriverGetVersion(&dr) != hipSuccess) dr = -1;
  snprintf(buf, n, "HIP runtime %d, driver %d", rt, dr);
}
#ifdef GPH_BOUNDS
static int oob_take(int32_t *where)
{
  int w = 0, z = 0;
  HIPCHK(hipMemcpyFromSymbol(&w, HIP_SYMBOL(gph_oob_word), sizeof(int)));
  if (w != 0) HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gph_oob_word), &z, sizeof(int)));
  *where = w;
  return 0;
}
#endif
// the parity probe's round trip: no engine, the null stream of `device`
// which: 0 k_debug_math (out[5n]), 1 k_debug_accept (out[3n])
static int debug_math(const double *x, const double *y, int n, double *out, int device, int which = 0)
{
  double *dx = nullptr, *dy = nullptr, *dout = nullptr;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc((void **)&dx, sizeof(double) * n));
  HIPCHK(hipMalloc((void **)&dy, sizeof(double) * n));
  HIPCHK(hipMalloc((void **)&dout, sizeof(double) * 5 * n));
  HIPCHK(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy, y, sizeof(double) * n, hipMemcpyHostToDevice));
  GphKargs ka;
  memset(&ka, 0, sizeof ka);
  fill_math_constants(ka);
  if (fill_math_tables(ka)) return GPH_EHIP;
  { int rcl = launch_on(nullptr, GphGrid{(n + GPH_FLAT_THREADS - 1) / GPH_FLAT_THREADS, 1}, GPH_FLAT_THREADS, 0, which ? k_debug_accept : k_debug_math, ka, dx, dy, n, dout); if (rcl) return rcl; }
  HIPCHK(hipMemcpy(out, dout, sizeof(double) * (which ? 3 : 5) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dout);
  return 0;
}
// the reduction probe (gph_debug_reduce_ in gph_engine.hip): k_reduce_stage itself, no engine.  `launches` launches back to
// back on one stream of its own, no host synchronisation between them; launch i folds input set i % nsets into row i, all of
// them through ONE partials buffer and ONE ticket sized as the engine's (gph_engine_load_loci, backend_open) -- what an
// iteration's six reductions share.  The partials and the rows start as GPH_RED_POISON; no stage runs (do_stage = 0)
struct GphRedProbe {
  double *out = nullptr, *stats = nullptr, *part = nullptr, *rows = nullptr;
  unsigned *ticket = nullptr;
  int32_t *err = nullptr;
  hipStream_t stream = nullptr;
  ~GphRedProbe()
  {
    dev_free(out); dev_free(stats); dev_free(part); dev_free(rows); dev_free(ticket); dev_free(err);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
static int debug_reduce(const double *out0, const double *stats1, int64_t L, int nc0, int nc1, int nsets, int err_word, int launches,
                        double *rows, int32_t *info, int device)
{
  HIPCHK(hipSetDevice(device));
  GphRedProbe p;
  const size_t n0 = nc0 > 0 ? (size_t)nsets * L * GPH_OUT_SLOTS : 0, n1 = nc1 > 0 ? (size_t)nsets * L * nc1 : 0;
  const size_t npart = (size_t)2 * 3 * GPH_RED_BLOCKS * GPH_RED_COLS, nrows = (size_t)launches * GPH_RED_ROW;
  std::vector<uint64_t> poison(npart > nrows ? npart : nrows, GPH_RED_POISON);
  HIPCHK(hipStreamCreate(&p.stream));
  if (n0) { HIPCHK(hipMalloc((void **)&p.out, sizeof(double) * n0)); HIPCHK(hipMemcpy(p.out, out0, sizeof(double) * n0, hipMemcpyHostToDevice)); }
  if (n1) { HIPCHK(hipMalloc((void **)&p.stats, sizeof(double) * n1)); HIPCHK(hipMemcpy(p.stats, stats1, sizeof(double) * n1, hipMemcpyHostToDevice)); }
  HIPCHK(hipMalloc((void **)&p.part, sizeof(double) * npart));
  HIPCHK(hipMalloc((void **)&p.rows, sizeof(double) * nrows));
  HIPCHK(hipMalloc((void **)&p.ticket, 64));
  HIPCHK(hipMalloc((void **)&p.err, sizeof(int32_t)));
  HIPCHK(hipMemcpy(p.part, poison.data(), sizeof(double) * npart, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p.rows, poison.data(), sizeof(double) * nrows, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(p.ticket, 0, 64));
  HIPCHK(hipMemcpy(p.err, &err_word, sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  GphKargs ka;
  memset(&ka, 0, sizeof ka);
  GphDev dev;
  memset(&dev, 0, sizeof dev);
  dev.L = (int32_t)L;
  dev.err = p.err;
  const GphStageList none = {0, {0}, {0}};
  for (int i = 0; i < launches; i++) {
    const size_t set = (size_t)(i % nsets);
    dev.out = n0 ? p.out + set * L * GPH_OUT_SLOTS : nullptr;
    dev.stats = n1 ? p.stats + set * L * nc1 : nullptr;
    { int rcl = launch_on(p.stream, GphGrid{GPH_RED_BLOCKS, 1}, GPH_RED_THREADS, 0, k_reduce_stage, ka, dev, nc0, nc1, p.part, p.ticket,
                          p.rows + (size_t)i * GPH_RED_ROW, 0, none, 0); if (rcl) return rcl; }
  }
  HIPCHK(hipStreamSynchronize(p.stream));
  unsigned ticket = 0;
  HIPCHK(hipMemcpy(rows, p.rows, sizeof(double) * nrows, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&ticket, p.ticket, sizeof ticket, hipMemcpyDeviceToHost));
  if (info) {
    const int32_t v[10] = {GPH_RED_COLS, GPH_RED_STRIDE, GPH_RED_ROW, GPH_RED_BLOCKS, GPH_RED_SUBS, GPH_RED_UNROLL, GPH_OUT_SLOTS, (int32_t)ticket,
                           (int32_t)(uint32_t)GPH_RED_POISON, (int32_t)(uint32_t)(GPH_RED_POISON >> 32)};
    memcpy(info, v, sizeof v);
  }
  return 0;
}
#endif
