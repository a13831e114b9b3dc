/*
 * gphocs_hip.h -- C ABI of libgphocs_hip.so, the MI355X-native per-locus likelihood
 * engine for G-PhoCS-style MCMC (drop-in for the reference's per-locus hot path).
 *
 * The reference has no plugin/FFI layer: the seam is the set of plain C entry points
 * performMCMC() calls (upstream src/GPhoCS.h:84-100) operating on process-wide
 * globals.  This ABI exports the same granularity -- batched over loci, an opaque
 * handle instead of globals, an int status instead of exit(-1):
 *
 *   reference (file:line)                              this library
 *   ------------------------------------------------   --------------------------------
 *   processAlignments/createLocusData/initializeLocusData
 *     GPhoCS.c:260-438, LocusDataLikelihood.c:142,239   gph_engine_load_loci
 *   GetMem  patch.c:28                                  gph_engine_create
 *   initRandomGenerator  utils.c:411                    gph_engine_seed
 *   initializeMCMC per-locus loop  GPhoCS.c:1197-1214   gph_engine_init_genealogies
 *   UpdateGB_InternalNode  GPhoCS.c:2287   \
 *   UpdateGB_MigrationNode GPhoCS.c:2439    }           gph_engine_genealogy_sweep
 *   UpdateGB_MigSPR        GPhoCS.c:2598   /
 *   UpdateTau loop 1       GPhoCS.c:3491-3833           gph_engine_tau_evaluate
 *   UpdateTau loop 2       GPhoCS.c:3885-3936           gph_engine_tau_commit
 *   UpdateTau loops 3/4    GPhoCS.c:3965-3989           gph_engine_tau_revert
 *   mixing loops           GPhoCS.c:4793-4801,4818-4848 gph_engine_mixing_evaluate/_commit
 *   UpdateTheta/UpdateMigRates per-locus touch-ups
 *     GPhoCS.c:3084-3093, 3192-3200                     gph_engine_apply_theta/_migrate
 *   computeTotalStats  patch.c:2134                     gph_engine_get_totals
 *   synchronizeEvents  patch.c:3548                     gph_engine_synchronize
 *   checkAll           patch.c:2745                     gph_engine_check_all
 *   performMCMC iteration body GPhoCS.c:1476-1821       gph_mcmc_iteration (host driver)
 *
 * All pointers are plain host pointers unless named *_dev.  Every function returns 0
 * on success or a negative GPH_E* code; the HIP path is the only path -- there is no
 * CPU fallback, and creation fails loudly when no gfx950 device is usable.
 * Not re-entrant per handle (as the reference: called serially from one thread).
 */
#ifndef GPHOCS_HIP_H
#define GPHOCS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPH_OK 0
#define GPH_EARG (-1)      /* bad argument / unsupported size */
#define GPH_EHIP (-2)      /* HIP runtime failure (no device, OOM, launch error) */
#define GPH_EKERNEL (-3)   /* a locus reported a fatal consistency error (reference: "Fatal Error NNNN") */
#define GPH_ESTATE (-4)    /* call out of order */
#define GPH_EFULL (-5)     /* gph_engine_coal_stats_sample / _time_slices_sample / _ancestry_sample / _gene_trees_sample: every row of the
                            * device buffer is taken; fetch first.  gph_engine_ancestry_enable / _gene_trees_enable: the accumulators /
                            * the row buffer would exceed the byte limit */

typedef struct gph_engine gph_engine;
typedef struct gph_mcmc gph_mcmc;

typedef struct {
  int32_t n;              /* haploid leaves per locus (dataSetup.numSamples) */
  int32_t Kc, K, B;       /* current pops, all pops, migration bands */
  int32_t rootPop;
  const int32_t *samplesPerPop;                 /* [Kc] haploid leaves per current pop */
  const int32_t *popFather, *popSon0, *popSon1; /* [K], -1 = none */
  const int32_t *bandSrc, *bandTgt;             /* [B] */
  int32_t device;         /* HIP device ordinal */
  int64_t L_total;        /* loci over all ranks (dataSetup.numLoci) */
  int64_t locus_begin;    /* global index of this rank's first locus */
} gph_config;

/* cross-rank reduction hook (one process per GPU): sums[0..nsum) are summed, mins[0..nmin)
 * minimised, in place, over all ranks.  NULL = single rank (or a native communicator, below).
 * nsum + nmin <= 16 + 2K + 2B: one call per reduction point, 6 + #ancestral populations per MCMC iteration.
 * A hook forces a host synchronisation at every reduction point; the native RCCL communicator does not. */
typedef int (*gph_allreduce_fn)(void *user, double *sums, int32_t nsum, double *mins, int32_t nmin);

/* ------------------------------------------------------------------------------------
 * native cross-rank exchange (csrc/gph_comm.cpp), one process per GPU, loci sharded over the ranks.  Replaces the
 * `omp atomic` accumulations of the reference's per-locus loops across GPUs:
 *   RCCL: ncclAllGather of the reduced row over xGMI, queued on the engine's stream -- no host synchronisation;
 *         librccl is dlopen()ed on first use.  RCCL refuses two ranks on one GPU.
 *   shm:  host shared-memory exchange for ranks that share a GPU (tests on a 1-GPU box).
 *   local: the ranks are THREADS of one process that share a device (tests on a 1-GPU box): the all-gather runs on
 *         the engines' streams (HIP events order the device-to-device copies), so the device-resident world > 1
 *         path -- reduction, gather, rank-order combine in k_global -- runs exactly as it does under RCCL.
 * rank 0 makes the id and hands it to the other ranks by any means (pipe, file, torch.distributed). */
typedef struct gph_comm gph_comm;
#define GPH_COMM_ID_BYTES 128
int gph_device_count(void);   /* HIP devices this process sees (the first GPU call of a freshly forked rank) */
int gph_comm_unique_id(void *id128);
gph_comm *gph_comm_create_rccl(const void *id128, int32_t rank, int32_t world, int32_t device);
gph_comm *gph_comm_create_shm(const char *name, int32_t rank, int32_t world);   /* name "/unique-per-run", same on every rank */
gph_comm *gph_comm_attach_shm(void *zeroed_shared_mapping, int32_t rank, int32_t world);
/* thread ranks of one process on one device: one group per job, one communicator per rank (thread); the group is
 * released with its last communicator */
typedef struct gph_comm_group gph_comm_group;
gph_comm_group *gph_comm_local_group(int32_t world, int32_t device);
gph_comm *gph_comm_create_local(gph_comm_group *group, int32_t rank);
size_t gph_comm_shm_bytes(int32_t world);
void gph_comm_destroy(gph_comm *c);
int gph_comm_world(const gph_comm *c);
int gph_comm_rank(const gph_comm *c);
int gph_comm_on_stream(const gph_comm *c);
const char *gph_comm_kind(const gph_comm *c);
int gph_comm_allgather_stream(gph_comm *c, const double *d_in, double *d_out, int32_t count, void *hip_stream);
int gph_comm_allreduce_host(gph_comm *c, double *sums, int32_t nsum, double *mins, int32_t nmin);

typedef struct {
  int64_t accepted_internal, accepted_mignode, accepted_spr;
  double dData_internal, dLog_internal, dLog_mignode, dData_spr, dLog_spr;
  int64_t total_mig_nodes;    /* sum of num_migs after the migration-node sweep (GPhoCS.c:1517-1520) */
} gph_sweep_result;

/* host part of UpdateTau (GPhoCS.c:3224-3461) or, with mode = 1, of UpdateSampleAge
 * (GPhoCS.c:4006-4128; ap = the current population whose sample age moves, son0 = son1 = -1,
 * taub0 = 0, taub1 = father age, tauold/taunew = old/new sample age) */
typedef struct {
  int32_t ap, son0, son1, isRoot, num_aff, mode;
  double tauold, taunew, taub0, taub1, taufactor0, taufactor1;
  int32_t aff_bands[200];     /* 2 * MAX_MIG_BANDS (patch.h:17): a band can enter with its start and its end */
  int32_t start_or_end[200];
  double new_band_ages[200];
} gph_tau_args;

typedef struct {
  int64_t ntj0, ntj1;
  int64_t first_conflict_locus;   /* global locus index, -1 = no migration conflict */
  double genDelta, dataDelta;
} gph_tau_result;

typedef struct {           /* summed over ALL ranks */
  int64_t evals;          /* computeLocusDataLikelihood(useOld=1)-equivalents since last reset */
  int64_t eval_nodes;     /* recomputed internal nodes (R) */
  double eval_bytes;      /* algorithmic bytes 96*R*P + 20*N + 8*U + 8 per evaluation */
  int64_t not_enough_migs;
} gph_counters;

int gph_engine_create(const gph_config *cfg, gph_engine **out);
void gph_engine_destroy(gph_engine *e);
int gph_engine_set_allreduce(gph_engine *e, gph_allreduce_fn fn, void *user);
/* native communicator (not owned by the engine; destroy it after the engine) */
int gph_engine_set_comm(gph_engine *e, gph_comm *c);
/* leafcodes: [Ptot][n] with 0..3 = T,C,A,G and 4 = N; numPhases non-zero on the first phase
 * of each unphased pattern (the reference keeps an int, 2^hets; here a 16-bit word: a count below 2^15 as it is, a count of 2^15 or
 * more -- always a power of two -- as 0x8000 | exponent, GPH_NUMPHASES below); counts on the same rows; pattern_offsets[L+1]
 *
 * What is legal is checked before anything is allocated; the first violation returns GPH_EARG, prints one line to stderr that
 * names the locus (global index) and the pattern (row of the locus), and leaves that locus and its GPH_LOAD_* code for
 * gph_engine_last_error and the line for gph_engine_last_error_text.  The sizes come first, from pattern_offsets alone, then
 * the rows locus by locus:
 *   GPH_LOAD_SIZE      a locus of P rows with 8 (n - 1) P >= 2^31 or a sequence block of 2^31 bytes or more (the device code
 *                      indexes a locus's conditionals and its block with 32-bit integers), or pattern_offsets that decrease
 *   GPH_LOAD_WORD      a phase word >= 0x8000 whose low 15 bits are not an exponent of 15 .. 24 (0x8003, 0x801f, a raw 32768)
 *   GPH_LOAD_NO_GROUP  a row with word 0 that no first row's count covers (a locus's first row among them)
 *   GPH_LOAD_OVERRUN   a first row whose decoded count runs past the last row of its locus
 *   GPH_LOAD_INSIDE    a non-zero word or a non-zero count on one of the count - 1 rows behind a first row
 *   GPH_LOAD_COUNT     a negative count
 *   GPH_LOAD_LEAF      a leaf code above 4
 * A count below 2^15 need not be a power of two (3, 5, 12 phases are legal); a locus of 0 rows is legal. */
#define GPH_NUMPHASES(w) ((int)(w) < 0x8000 ? (int)(w) : (1 << ((int)(w) & 31)))
#define GPH_LOAD_SIZE     (-101)
#define GPH_LOAD_WORD     (-102)
#define GPH_LOAD_NO_GROUP (-103)
#define GPH_LOAD_OVERRUN  (-104)
#define GPH_LOAD_INSIDE   (-105)
#define GPH_LOAD_COUNT    (-106)
#define GPH_LOAD_LEAF     (-107)
int gph_engine_load_loci(gph_engine *e, int64_t L, const int64_t *pattern_offsets, const uint8_t *leafcodes,
                         const uint16_t *numPhases, const int32_t *counts, const double *mutRates);
/* the line the last refused gph_engine_load_loci printed ("" if none); valid until the engine is destroyed */
const char *gph_engine_last_error_text(gph_engine *e);
int gph_engine_set_model(gph_engine *e, const double *theta, const double *popAge, const double *sampleAge,
                         const double *migRate, const double *bandStart, const double *bandEnd);
int gph_engine_seed(gph_engine *e, uint32_t seed);
int gph_engine_init_genealogies(gph_engine *e, double *sumGenLnL, double *sumDataLnL);
/* flags: 1 = internal-node ages, 2 = migration-node ages, 4 = SPR; fused in one launch */
int gph_engine_genealogy_sweep(gph_engine *e, int32_t flags, double finetuneCoalTime, double finetuneMigTime,
                               gph_sweep_result *out);
int gph_engine_tau_evaluate(gph_engine *e, const gph_tau_args *a, gph_tau_result *out);
int gph_engine_tau_commit(gph_engine *e);
int gph_engine_tau_revert(gph_engine *e, int64_t first_conflict_locus);
int gph_engine_mixing_evaluate(gph_engine *e, double c, double *dataDelta);
int gph_engine_mixing_commit(gph_engine *e, double c, double lnc);
int gph_engine_mixing_revert(gph_engine *e);
/* UpdateLocusRate (GPhoCS.c:4598-4680; `locus-mut-rate VAR alpha`).  The reference loop is serial over loci (each
 * proposal also moves the rate of the reference locus, genRateRef = 0): one wavefront scans the loci in input
 * order with a stateless evaluator, the accepted loci are then rewritten in parallel.  in/out: the three
 * accumulators the reference updates per accepted proposal (dataState.dataLogLikelihood, .logLikelihood,
 * .rateVar); returns the accept count.  finetune <= 0 returns 0 accepted at once (:4606).  With loci sharded over
 * ranks the scan is chained through the ranks in locus order over the all-reduce hook (same additions in the same
 * order: bit-identical to one rank); every rank gets the same result. */
typedef struct gph_locus_rate_result {
  int64_t accepted;
  double dataLogLikelihood, logLikelihood, rateVar;
} gph_locus_rate_result;
int gph_engine_locus_rate_update(gph_engine *e, double finetune, double varRatesAlpha, gph_locus_rate_result *io);
/* starting rates of the local loci in input order, before gph_engine_init_genealogies (initializeMCMC's VAR
 * branch, GPhoCS.c:1157-1178: the host draws and normalises, `draws` = rndu() draws each locus's stream spent
 * on it -- 1 there); variable != 0 makes the rates part of the dumped state */
int gph_engine_set_locus_rates(gph_engine *e, const double *rates, int32_t draws, int32_t variable);
int gph_engine_apply_theta(gph_engine *e, int32_t pop, double lnc, double thetaold, double thetanew);
int gph_engine_apply_migrate(gph_engine *e, int32_t band, double lnc, double old_rate, double new_rate);
/* sums over ALL ranks; num_* returned as doubles holding exact integers */
int gph_engine_get_totals(gph_engine *e, double *coal_stats, double *num_coals, double *mig_stats,
                          double *num_migs);
int gph_engine_synchronize(gph_engine *e, int32_t refresh_genealogy_lnl, double *sumOldGenLnL,
                           double *sumNewGenLnL);
int gph_engine_check_all(gph_engine *e, int32_t *ok, double *sumDataLnL, double *sumGenLnL);
int gph_engine_get_counters(gph_engine *e, gph_counters *out, int32_t reset);
/* After a call returned GPH_EKERNEL: the reference's "Fatal Error NNNN" code and the global index of the FIRST locus that
 * reported it (-1 when the failure is not one locus's: checkAll's accumulator test, synchronizeEvents' flag).  The engine
 * has then already printed, to stderr, the code, the locus and -- what printGenealogyAndExit(gen, ...) prints upstream,
 * GPhoCS.c:660-676 -- that locus's genealogy and event chains in the canonical dump format. */
int gph_engine_last_error(gph_engine *e, int64_t *locus, int32_t *code);
/* tests only: break the event chain of population `pop` of one locus, so that the next kernel raises a fatal code for it
 * (with several ranks every rank calls it: it completes a deferred synchronizeEvents pass first, which is a collective;
 * GPH_EARG on the ranks that do not hold the locus) */
int gph_engine_debug_break_chain(gph_engine *e, int64_t global_locus, int32_t pop);
/* tests only: libgphocs_hip_chk.so is the same library compiled with -DGPH_BOUNDS -- every index the per-locus device code puts
 * into an array of a locus's LDS image, into its dynamic LDS or into its conditional arrays is compared with the array's extent.
 * *checked = 1 in such a build (0 in every product library); *where = 0, or the first violation's source line + 100000 x file
 * (read and cleared).  gph_engine_unit op 8 is the check's self-test: it reads node record `arg`. */
int gph_engine_debug_oob(gph_engine *e, int32_t *where, int32_t *checked);
/* debug / parity: canonical text dump of every local locus (same format as the oracle's) */
int gph_engine_dump_loci(gph_engine *e, const char *path, int32_t withConditionals, int32_t append);
/* debug / parity, kernel level: single calls of the per-locus functions with deterministic arguments on the current
 * chain state, every call undone -- what oracle/ref_harness.c `unit` does with the reference's own functions
 * (tests/golden/ *.unit).  out[local loci][stride] in input order.  op 0: per internal node i (stride >= 3 (n-1)):
 * tnew, lnLd, dprior of adjustGenNodeAge + computeLocusDataLikelihood(1) + considerEventMove (GPhoCS.c:2316-2381);
 * op 1: computeLocusDataLikelihood(useOld=0); op 2: rubberBand(pre) x3 of ancestral population arg + evaluation
 * (GPhoCS.c:3705-3831): delta, n0, n1, lik.  Second set (`unit2`, tests/golden/ *.unit2): op 3: executeGenSPR of node arg
 * (LocusDataLikelihood.c:931-1012; return codes 0 / 1 / 2) onto its father's, its sibling's, the root's and every fifth other
 * legal branch + computeLocusDataLikelihood(1) + revertToSaved (stride >= 1 + 5 (2n-1): calls, then target, age, code, value,
 * root); op 4: scaleAllNodeAges(1 + arg / 1000) (LocusDataLikelihood.c:895-917) + revertToSaved + full recompute: delta,
 * value; op 5: rubberBandRipple(do) + (undo) (patch.c:815-869) over every migration event's source-side event moved 0.01 %
 * up: events, two deltas; op 6: traceLineage(arg, 0) + traceLineage(arg, 1) (patch.c:886-1331) + evaluation (stride >= 13:
 * 1, res, target, father's new population, migration events removed / created, both prior deltas, father's new age, data
 * delta, the locus's generator state); op 7: rubberBandRipple(do) + (undo) over the MIG_BAND_START / MIG_BAND_END events of
 * every band, moved 30 % into the neighbouring gap (the entries UpdateTau adds with start_or_end 1 / 0, GPhoCS.c:3708-3745):
 * events, two deltas */
int gph_engine_unit(gph_engine *e, int32_t op, int32_t arg, double *out, int32_t stride);
/* timing of the last launch of a named kernel class, measured with HIP events on the
 * engine's own stream: which = 0 sweep, 1 tau_eval, 2 mix_eval, 3 init, 4 check,
 * 5 tau_finish (commit or revert, by the decision flag), 7 mix_finish, 8 sync, 9 locus-rate scan, 10 locus-rate apply,
 * 11 locus-rate prepare, 13 locus summary (gph_engine_locus_summary_sample), 14 coalescent / sample-pair statistics
 * (gph_engine_coal_stats_sample: k_coal_stats + k_rows_fold together), 15 time-sliced statistics
 * (gph_engine_time_slices_sample: k_time_slices + k_rows_fold together), 16 migration ancestry
 * (gph_engine_ancestry_sample: k_ancestry), 17 sampled genealogies (gph_engine_gene_trees_sample: k_gene_trees), 18 the
 * sweep's draws generated ahead of it (k_rng_ahead), 19 clade tables (gph_engine_clades_sample: k_clades), 20 the clade
 * tables of replicate chains compared (gph_engine_clades_compare: k_clades_compare, counted on engines[0]), 21 effective
 * sample sizes per locus (gph_engine_ess_sample: k_ess), 22 posterior predictive checks (gph_engine_predictive_sample:
 * k_predictive), 23 triplet topology weights (gph_engine_triplets_sample: k_triplets), 24 expected substitutions
 * (gph_engine_mutations_sample: k_mutations + k_rows_fold together), 25 replicate genealogies (gph_engine_simulate_sample),
 * 26 pairwise coalescence-time distributions (gph_engine_pair_times_sample: k_pair_times), 27 site-frequency spectra, the
 * genealogy side (gph_engine_sfs_sample: k_sfs_tree + k_rows_fold together), 28 their data side (gph_engine_sfs_enable: k_sfs_data) */
int gph_engine_last_kernel_ms(gph_engine *e, int32_t which, double *ms);
/* classes whose launches are bracketed by HIP events (bit k = class k); default all */
int gph_engine_set_timing(gph_engine *e, uint32_t class_mask);
/* host synchronisations, cross-rank exchanges and kernel launches since the engine was created; resident_mode = 1 when
 * the decisions above the loci are taken on the device (one host synchronisation per iteration) */
int gph_engine_host_stats(gph_engine *e, int64_t *syncs, int64_t *collectives, int64_t *launches, int32_t *resident_mode);
/* accumulated per class: out5 = {launches, summed ms, evaluations, algorithmic bytes, recomputed nodes} */
int gph_engine_class_stats(gph_engine *e, int32_t which, double *out5, int32_t reset);
int64_t gph_engine_num_loci(gph_engine *e);
/* parity probe: out[5n] = exp(x), log(x), sqrt(|x|), x/y, floor(x) evaluated on the device */
int gph_debug_math(const double *x, const double *y, int32_t n, double *out5n, int32_t device);
int gph_engine_hbm_bytes(gph_engine *e, double *bytes);
/* identity of this build of the library: hash of its sources and compiler flags (measurement files under profiles/
 * carry it, and bench.py drops a committed counter measurement that was taken with another build) */
const char *gph_build_id(void);
/* the compiler that built this library (its __clang_version__) and the HIP runtime / driver it is running on
 * ("runtime <hipRuntimeGetVersion>, driver <hipDriverGetVersion>"): both go into the bench line -- a library built by one
 * ROCm release may well run on another */
/* TEST BUILDS ONLY (libgphocs_hip_plain.so and the host build of tests/hostemu; every other build returns GPH_EARG):
 * decision-level transcript of the three genealogy sweeps for the selected loci (global locus indices), the engine's
 * counterpart of upstream's -DLOG_STEPS debug file (GPhoCS.c:2363-2401, 2540-2577, 2654-2718; patch.c:1451-1454).
 * Records are 8 doubles: kind, then  1 node-age proposal: node, t, tnew | 2 considerEventMove: event, source pop, target
 * pop, old age, new age, new event | 3 decision: accepted, lnacceptance | 4 migration-node proposal: node, t, tnew |
 * 5 SPR: node, father, father's population.  tests/test_logsteps.py formats them as upstream prints them. */
int gph_engine_steplog_enable(gph_engine *e, const int64_t *loci, int32_t n, int32_t cap);
int gph_engine_steplog_fetch(gph_engine *e, int32_t idx, double *out, int32_t max_records, int32_t *nrec, int32_t reset);
const char *gph_build_compiler(void);
const char *gph_runtime_version(void);
/* per-locus posterior summaries, accumulated on the device (k_locus_summary, csrc/gph_summary.h).  One sample reads, from
 * every local locus's page, the data and genealogy log-likelihoods, the TMRCA (age of the root node), the locus rate
 * (`locus-mut-rate VAR` only), the migration count of every band and the coalescence count of every population, and
 * adds them to fp64 accumulators in HBM.  Moments are kept as shift (the value at the first sample) + sums of d and d^2,
 * d = x - shift, in sample order; counts as sums, and for every band the number of samples with a migration.
 *   _enable(on)     allocates and zeroes the accumulators (on = 1) or frees them (on = 0); gph_engine_init_genealogies
 *                   zeroes them again
 *   _sample         queues one sample on the engine's stream (no host synchronisation); a mixing commit still owed to
 *                   the next sweep kernel runs first
 *   _columns        raw columns per locus and samples taken since the accumulators were last zeroed
 *   _fetch          out[local locus][ld >= ncol], rows in global locus order (row i = global locus locus_begin + i);
 *                   reset = 1 zeroes the accumulators afterwards
 *   _column_name    stable machine name of raw column col ("dataLnL.shift", "dataLnL.s1", "dataLnL.s2", "genLnL.*",
 *                   "tmrca.*", "nmig.<band>", "pmig.<band>", "ncoal.<pop>", "rate.*"), NULL if out of range */
int gph_engine_locus_summary_enable(gph_engine *e, int32_t on);
int gph_engine_locus_summary_sample(gph_engine *e);
int gph_engine_locus_summary_columns(gph_engine *e, int32_t *ncol, int64_t *samples);
int gph_engine_locus_summary_fetch(gph_engine *e, double *out, int64_t ld, int32_t reset);
const char *gph_engine_locus_summary_column_name(gph_engine *e, int32_t col);
/* genome-wide coalescent statistics and sample-pair statistics of one MCMC sample, computed on the device (k_coal_stats,
 * k_rows_fold: csrc/gph_coalstats.h, gph_sampler.h).  They replace code the reference carries but never reaches (`coal-stats-file`,
 * GPhoCS.c:1771 `if (recordCoalStats && 0)`): computeNodeStats (patch.c:2172-2270) over computePairwiseLCAs
 * (LocusDataLikelihood.c:1685-1830), computeFlatStats (patch.c:2278-2320) over getSortedAges
 * (LocusDataLikelihood.c:1216-1260), and the numbers printCoalStats prints (GPhoCS.c:911-1040).
 * A raw row of row_doubles = 7 + 3 * n(n-1)/2 * K doubles, over THIS rank's loci:
 *   [0] iteration  [1] coalStat  [2] numCoal  [3] migStat  [4] numMig  [5] sum of genealogy log-likelihoods
 *   [6] sum of data log-likelihoods, then three blocks [pair][population], pairs (i, j), i < j, row-major:
 *   cnt (loci in which the pair coalesces in the population), first (... and that coalescence is the population's first
 *   in the locus), agesum (summed age of those coalescences).  Counts are doubles holding integers.
 * Derived as printCoalStats / computeNodeStats do (patch.c:2256-2266): probCoal = cnt / L, probFirstCoal = first / L,
 * meanCoal = agesum / cnt where cnt > 0, else 0, with L the loci of all ranks; logGenLikelihood = [5] + [6]
 * (GPhoCS.c:997 prints dataState.logLikelihood * numLoci, data + genealogy), logDataLikelihood = [6].  logPrior
 * (getLogPrior, GPhoCS.c:858-898) is a function of the parameters alone and is added by the caller.  Several ranks: the
 * ranks' raw rows are added in rank order before anything is derived.
 *   _enable(capacity)  allocates a device buffer of `capacity` rows (capacity 0: frees everything, the feature is off);
 *                      gph_engine_init_genealogies empties it
 *   _sample(iteration) queues one sample on the engine's stream (no host synchronisation) into the next free row; a
 *                      mixing commit still owed to the next sweep kernel runs first.  GPH_EFULL when no row is free:
 *                      nothing is overwritten
 *   _shape             doubles per row, rows filled since the last fetch, leaves, populations
 *   _fetch             copies the filled rows to out[max_rows >= filled][row_doubles], *rows = their number, and
 *                      empties the buffer
 *   _column_name       machine name of raw column col: "iter", "coalStat", "numCoal", "migStat", "numMig", "genLnL",
 *                      "dataLnL", "cnt.<i>.<j>.<pop>", "first.<i>.<j>.<pop>", "agesum.<i>.<j>.<pop>"; NULL if out of
 *                      range; the string is valid until the next call on this engine */
int gph_engine_coal_stats_enable(gph_engine *e, int32_t capacity);
int gph_engine_coal_stats_sample(gph_engine *e, int32_t iteration);
int gph_engine_coal_stats_shape(gph_engine *e, int32_t *row_doubles, int32_t *filled, int32_t *n, int32_t *K);
int gph_engine_coal_stats_fetch(gph_engine *e, double *out, int32_t max_rows, int32_t *rows);
const char *gph_engine_coal_stats_column_name(gph_engine *e, int32_t col);
/* tests: slots per chunk used by the next _enable (0 = the default, 128).  The chunk size is part of the summation order
 * of the fp64 sums (csrc/gph_coalstats.h): rows are bitwise reproducible for a given locus count, chunk size and rank
 * count */
int gph_engine_coal_stats_set_chunk(gph_engine *e, int32_t slots);
/* coalescence and migration statistics per TIME SLICE of one MCMC sample, genome-wide, computed on the device
 * (k_time_slices, k_rows_fold: csrc/gph_timeslices.h, where the statistic is defined line by line).  Every
 * population's branch and every migration band's life is cut into `slices` equal time slices; per slice: the number of
 * coalescences C and the coalescent exposure D = sum of n(n-1) t (the sufficient statistics of theta within the slice),
 * the number of migrations N into the band's target through the band and the migration exposure M = sum of n t.  The
 * population half restates recalcStats_partitioned / computeGenetreeStats_partitioned (patch.c:2357-2694; the columns
 * numCoal_<pop>:<k> / deltaT_<pop>:<k> of printCoalStats, GPhoCS.c:927-935, 1000-1009), which the reference never reaches;
 * the migration half is commented out upstream and defined here.  The root population has one slice (its other columns
 * stay 0, as upstream prints them).  Unlike upstream the last slice takes whatever lies past the last boundary (upstream
 * drops up to 1e-7 and aborts with Fatal Error 9001 beyond): the slices of a branch add up to the pages' own statistic.
 * A raw row of row_doubles = 1 + 2 * slices * (K + B) doubles, over THIS rank's loci:
 *   [0] iteration, then for every population in model order and every slice C, D, then for every band in control-file
 *   order and every slice N, M.  Counts are doubles holding integers.  Several ranks: the rows are added in rank order.
 *   _enable(slices, capacity)  a device buffer of `capacity` rows (capacity 0: frees everything, the feature is off);
 *                      slices outside 1 .. 32 is GPH_EARG (with a message); gph_engine_init_genealogies empties the buffer
 *   _sample(iteration) queues one sample on the engine's stream (two kernels, no host synchronisation, no exchange) into
 *                      the next free row; a commit still owed to the next kernel runs first (k_mix_finish after an
 *                      accepted mixing proposal; k_tau_finish between the parts of a stepwise caller); a deferred synchronizeEvents
 *                      pass stays deferred (the kernel reads the event times as that pass will leave them).  GPH_EFULL
 *                      when no row is free: nothing is overwritten
 *   _shape             doubles per row, rows filled since the last fetch, slices, populations, bands, and the bytes of a
 *                      page the kernel copies into LDS per locus and sample (any pointer may be NULL)
 *   _fetch             copies the filled rows to out[max_rows >= filled][row_doubles], *rows = their number, and empties
 *                      the buffer
 *   _column_name       machine name of raw column col: "iter", "numCoal.<pop>.<k>", "deltaT.<pop>.<k>", "numMig.<band>.<k>",
 *                      "migT.<band>.<k>", k = 1 .. slices; NULL if out of range; valid until the next call on this engine
 *   _set_chunk         tests: slots per chunk used by the next _enable (0 = the default, 128); the chunk size is part of
 *                      the summation order: rows are bitwise reproducible for a given locus count, chunk size and rank count */
int gph_engine_time_slices_enable(gph_engine *e, int32_t slices, int32_t capacity);
int gph_engine_time_slices_sample(gph_engine *e, int32_t iteration);
int gph_engine_time_slices_shape(gph_engine *e, int32_t *row_doubles, int32_t *filled, int32_t *slices, int32_t *K, int32_t *B,
                                 int32_t *staged_bytes_per_locus);
int gph_engine_time_slices_fetch(gph_engine *e, double *out, int32_t max_rows, int32_t *rows);
const char *gph_engine_time_slices_column_name(gph_engine *e, int32_t col);
int gph_engine_time_slices_set_chunk(gph_engine *e, int32_t slots);
/* per-locus, per-sample MIGRATION ANCESTRY accumulated on the device (k_ancestry: csrc/gph_ancestry.h): which sample's
 * lineage went through which migration band, at which locus.  For one locus at one sample, with n leaves and B bands in
 * control-file order, take the live migration nodes (the IS_NUM_MIGS entries of `living`; the M line of a state dump prints
 * mg:branch:band:spop:tpop:sev:tev:age).  The path of leaf i is i, father(i), ..., root; migration node m is on the path
 * iff its branch is a node of the path.  hit[b][i] = 1 iff some live m on the path of i belongs to band b; first[b][i] =
 * the smallest age among those (the first one met going back in time); any[i] = 1 iff some hit[b][i] is 1.
 * Per local locus, over the samples taken: a row of locus_columns = n (2B + 1) doubles, column b n + i: cnt.<b>.<i> += hit;
 * B n + b n + i: age.<b>.<i> = age.<b>.<i> + first where hit (one plain fp64 addition a sample: rebuilt bit for bit from
 * state dumps); 2 B n + i: any.<i> += any.  Counts are doubles holding integers.
 * Per sample, over THIS rank's loci: a row of row_ints = n (B + 1) integers, column i: the loci with any[i] = 1; (1 + b) n
 * + i: the loci with hit[b][i] = 1.  Several ranks: the per-locus rows concatenate in rank order, the per-sample rows add.
 *   _enable(capacity_rows, max_bytes)  accumulators (zeroed) and a device buffer of capacity_rows per-sample rows;
 *                      capacity_rows 0 frees everything, the feature is off.  GPH_EFULL (with a message that names the
 *                      size) when the accumulators, L_local n (2B + 1) 8 bytes, exceed max_bytes (<= 0: 1 GiB); the
 *                      engine stays usable.  B = 0: only the any columns exist (all zero).  gph_engine_init_genealogies
 *                      zeroes the accumulators and empties the buffer
 *   _sample(iteration) queues one sample on the engine's stream (one kernel, no host synchronisation, no exchange); the
 *                      pages are made current as for gph_engine_locus_summary_sample (a commit still owed to the next
 *                      kernel runs first).  A group of loci without a live migration costs one 4-byte read a locus.
 *                      GPH_EFULL when no per-sample row is free: nothing is overwritten, nothing accumulated
 *   _shape             doubles per per-locus row, integers per per-sample row, samples accumulated since the accumulators
 *                      were last zeroed, per-sample rows held (any pointer may be NULL)
 *   _fetch_loci        out[L_local][ld >= locus_columns] in global locus order (as gph_engine_locus_summary_fetch);
 *                      reset != 0 zeroes the accumulators and the sample count afterwards
 *   _fetch_rows        copies the held rows to iters[max_rows >= held] and out[held][ld >= row_ints], *rows = their number,
 *                      and empties the buffer
 *   _column_name(which, col)  which 0: a per-locus column, "cnt.<b>.<i>", "age.<b>.<i>", "any.<i>"; which 1: a per-sample
 *                      column, "any.<i>", "hit.<b>.<i>"; NULL if out of range or off; valid until the next call */
int gph_engine_ancestry_enable(gph_engine *e, int32_t capacity_rows, int64_t max_bytes);
int gph_engine_ancestry_sample(gph_engine *e, int32_t iteration);
int gph_engine_ancestry_shape(gph_engine *e, int32_t *locus_columns, int32_t *row_ints, int64_t *samples, int32_t *rows_held);
int gph_engine_ancestry_fetch_loci(gph_engine *e, double *out, int64_t ld, int32_t reset);
int gph_engine_ancestry_fetch_rows(gph_engine *e, int32_t *iters, int32_t *out, int64_t ld, int32_t max_rows, int32_t *rows);
const char *gph_engine_ancestry_column_name(gph_engine *e, int32_t which, int32_t col);
/* SAMPLED GENEALOGIES of selected loci, gathered on the device (k_gene_trees: csrc/gph_genetrees.h).  One RECORD describes
 * one locus at one sample -- what the LOCUS, N and M lines of a state dump print at the same point of the chain, every field
 * equal and the ages equal as bit patterns.  With n leaves and N = 2n - 1 nodes it is record_bytes bytes (about 16 N + 300)
 * copied verbatim from the locus's page, and holds at the offsets _shape hands out (GPH_GT_O_*):
 *   NODES     N node records of 16 bytes: age (fp64), father, left, right, npop (int16 each)
 *   ROOT, NUM_MIGS  two int32: the root node and the number of live migrations
 *   DATALNL, GENLNL two fp64
 *   MIG_AGE   GPH_GT_MAX_MIGS fp64, by migration node
 *   MIG_I     GPH_GT_MAX_MIGS x 6 int16, by migration node: branch, band, source population, target population, 2 event ids
 *   LIVING    GPH_GT_MAX_MIGS int16: the live migration nodes, NUM_MIGS of them, in the order of a state dump's M line
 * gph_gene_trees_decode (below) turns records into plain arrays.  A SELECTION is a strictly increasing list of global 0-based
 * locus indices in sequence-file order; a ROW is one sample: the records of the selected loci THIS rank holds, in increasing
 * locus index (not slot order: the kernel goes through a selected -> slot table).
 *   _enable(capacity_rows, loci, nloci, max_bytes)  a device buffer of capacity_rows rows for the selection; loci NULL: all
 *                      loci of the rank.  GPH_ESTATE before gph_engine_load_loci.  GPH_EARG for a negative index or a list
 *                      that is not strictly increasing; indices outside this rank's block [locus_begin, locus_begin + L_local)
 *                      are not this rank's and are ignored (a rank may end up with no selected locus).  capacity_rows 0 frees
 *                      everything, the feature is off.  GPH_EFULL (with a message that names the numbers) when capacity_rows x
 *                      selected x record_bytes exceeds max_bytes (<= 0: 256 MB); the engine stays usable, the feature is off.
 *                      gph_engine_init_genealogies empties the buffer
 *   _sample(iteration) GPH_ESTATE when not enabled or not initialised, GPH_EFULL when no row is free (nothing is overwritten).
 *                      Otherwise queues one sample on the engine's stream: one kernel (none on a rank without a selected
 *                      locus, which still counts the sample), no host synchronisation, no exchange.  The pages and the
 *                      migration ages are made current as for gph_engine_ancestry_sample; a deferred synchronizeEvents pass
 *                      stays deferred (a record holds no event time)
 *   _shape             selected loci of this rank, N, bytes of a record, the GPH_GT_O_COUNT offsets inside a record, rows
 *                      held (any pointer may be NULL; all 0 while the feature is off)
 *   _selected          out[max_loci >= *count]: the global indices of this rank's selected loci; out NULL with max_loci 0:
 *                      the count only.  GPH_ESTATE while off
 *   _fetch             copies the rows taken since the last fetch to iters[max_rows >= held] and out[held][selected x
 *                      record_bytes], *rows = their number, and empties the buffer (one host synchronisation; out may be
 *                      NULL on a rank without a selected locus).  GPH_ESTATE while off, GPH_EARG when max_rows is too small */
#define GPH_GT_MAX_MIGS 10
enum { GPH_GT_O_NODES = 0, GPH_GT_O_ROOT, GPH_GT_O_NUM_MIGS, GPH_GT_O_DATALNL, GPH_GT_O_GENLNL, GPH_GT_O_MIG_AGE, GPH_GT_O_MIG_I,
       GPH_GT_O_LIVING, GPH_GT_O_COUNT };
int gph_engine_gene_trees_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int64_t max_bytes);
int gph_engine_gene_trees_sample(gph_engine *e, int32_t iteration);
int gph_engine_gene_trees_shape(gph_engine *e, int64_t *selected, int32_t *nodes, int32_t *record_bytes, int32_t *offsets, int32_t *rows_held);
int gph_engine_gene_trees_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_gene_trees_fetch(gph_engine *e, int32_t *iters, void *out, int32_t max_rows, int32_t *rows);
/* CLADE TABLES per selected locus, accumulated on the device over the samples taken (k_clades: csrc/gph_clades.h).  With n
 * leaves, N = 2n - 1 nodes and W = ceil(n / 64): the clade of internal node v is the set of leaves whose path to the root
 * contains v, as W 64-bit words (bit i % 64 of word i / 64), the root's clade (all leaves) included.  A locus's TABLE has
 * `slots` physical slots (a power of two >= 2) and holds at most limit = 3 slots / 4 distinct clades; an entry is key[W],
 * cnt, age (the bit pattern of an fp64), cnt = 0 marks an empty slot; nkeys and dropped are kept per locus.  A sample takes
 * the internal nodes v = n .. N - 1 in node-index order: key in the table -> cnt += 1, age = age + age[v] (one plain fp64
 * addition: the sums can be rebuilt bit for bit in sample order); else nkeys < limit -> insert with cnt = 1, age = age[v],
 * nkeys += 1; else dropped += 1.  Hence: counts of kept clades are exact; a table never leaves the full state and a clade
 * dropped once is never inserted later; the root key has cnt = samples; sum of cnt + dropped = samples x (n - 1).  Where an
 * entry lies inside its table is unspecified.
 *   _enable(slots, loci, nloci, max_bytes)  slots 0: the smallest power of two >= 8 (n - 1); any other value that is no
 *                      power of two or below 2 is GPH_EARG.  The selection as for gph_engine_gene_trees_enable (loci NULL:
 *                      all loci of the rank).  GPH_EFULL (with a message, nothing allocated, the feature off) when the tables
 *                      exceed max_bytes (<= 0: 1 GiB).  Everything is allocated here and freed with the engine;
 *                      gph_engine_init_genealogies zeroes the tables and the sample count
 *   _sample            GPH_ESTATE when not enabled or not initialised.  One kernel (none on a rank without a selected locus,
 *                      which still counts the sample), no host synchronisation, no exchange; the state is settled as for
 *                      gph_engine_ancestry_sample
 *   _shape             selected loci of this rank, slots, W, limit, samples since the tables were last zeroed (any pointer
 *                      may be NULL; all 0 while the feature is off)
 *   _selected          as gph_engine_gene_trees_selected
 *   _fetch             entries[selected][slots][W + 2] in selection order, nkeys[selected], dropped[selected] (one host
 *                      synchronisation); reset != 0 then zeroes tables, header words and the sample count */
int gph_engine_clades_enable(gph_engine *e, int32_t slots, const int64_t *loci, int64_t nloci, int64_t max_bytes);
int gph_engine_clades_sample(gph_engine *e);
int gph_engine_clades_shape(gph_engine *e, int64_t *selected, int32_t *slots, int32_t *words, int32_t *limit, int64_t *samples);
int gph_engine_clades_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_clades_fetch(gph_engine *e, uint64_t *entries, uint32_t *nkeys, uint32_t *dropped, int32_t reset);
/* REPLICATE CHAINS COMPARED: how far apart are the clade frequencies of R = 2 .. 16 chains, per selected locus, computed on
 * the device from the chains' clade tables where they lie (k_clades_compare: csrc/gph_cladecmp.h); only the rows leave it.
 * All engines belong to this library and one device, and their tables share the selection, the slots and W; chain r has taken
 * S_r >= 1 samples.  For locus q let U be the distinct keys kept in at least one of the R tables; the trivial clade (all n
 * leaves) is left out everywhere.  For k in U: c_r = the entry's cnt in table r, 0 where table r does not hold k (a clade
 * that a FULL table dropped counts as frequency 0 in that chain -- that is what the table says, and dropped > 0 in the row is
 * the warning, as for the tables themselves), and in plain fp64, in this operand order,
 *   f_r = (double)c_r / (double)S_r        m = (((f_0 + f_1) + ...) + f_{R-1}) / R
 *   v = (sum_r (f_r - m) (f_r - m), added in chain order) / (R - 1)        sd = sqrt(v)
 * k is COMPARED iff max_r f_r >= min_freq.  rows[q][6], q over the selected loci of the rank in increasing locus index:
 *   asdsf     sum of sd over the compared clades / their number, 0 when there are none (the average standard deviation of
 *             split frequencies); the sds are added in an order of the kernel's own that does not depend on the other loci
 *   maxSd     max sd over the compared clades, 0 when there are none
 *   compared  their number            distinct  |U|
 *   shared    keys held by all R tables            dropped   sum over the chains of the tables' `dropped` words
 * (counts are exact in fp64).  *count = the selected loci of the rank; none: nothing is launched.  Order: engines[0]'s stream
 * waits, through events, for what the other engines' streams hold (their last k_clades), runs the one kernel (timing class
 * 20, counted on engines[0]), and the other streams wait for it before they go on, so a later sample cannot write a table
 * that is still being read; then one copy of the rows and ONE host synchronisation, on engines[0].  No device-wide
 * synchronisation, no kernel waits for another stream.  No table, page or chain state is written.
 * GPH_EARG, nothing changed: R outside 2 .. 16; a null, foreign (another library variant's) or repeated engine; min_freq not
 * in [0, 1] or not finite; engines on different devices; different selections, slots or key words; max_loci below the
 * selection.  GPH_ESTATE: clade tables not enabled on some engine; a sample count of 0. */
int gph_engine_clades_compare(gph_engine *const *engines, int32_t R, double min_freq, double *rows /* [max_loci][6] */, int64_t max_loci,
                              int64_t *count);
/* the potential scale reduction factor (Gelman & Rubin 1992) of one quantity over R >= 2 chains of S >= 2 samples each,
 * x[R][S]; host code, plain fp64 in this operand order (a loop in the same order reproduces every bit):
 *   m_r = (sum_s x[r][s], added in sample order) / S        v_r = (sum_s (x[r][s] - m_r)^2, added in sample order) / (S - 1)
 *   Wv = (sum_r v_r, added in chain order) / R              M = (sum_r m_r, added in chain order) / R
 *   Bn = (sum_r (m_r - M)^2, added in chain order) / (R - 1)        V = ((double)(S - 1) / (double)S) * Wv + Bn
 *   out = {mean M, sdWithin sqrt(Wv), sdBetween sqrt(Bn), psrf sqrt(V / Wv)};  Wv == 0: psrf = 1 if Bn == 0, else +inf
 * R < 2, S < 2 or a null pointer: GPH_EARG. */
int gph_psrf(const double *x /* [R][S] */, int32_t R, int64_t S, double *out /* mean, sdWithin, sdBetween, psrf */);
/* EFFECTIVE SAMPLE SIZES.  One estimator, two users (csrc/gph_ess.h): the batch-sum LEVELS of a series, kept by binary carry.
 * J = 16 levels; a series x_0 .. x_S-1 owns a[2 + 2J] doubles: a[0] = shift = x_0, a[1] = s1, a[2 + j] = run[j] (run[0] stays
 * 0), a[2 + J + j] = sq[j].  Sample t (0-based) brings d = x_t - shift (t = 0: every word is zeroed first, d = 0); plain
 * uncontracted fp64 in this order (a loop in the same order reproduces every bit):
 *   s1 = s1 + d;  sq[0] = sq[0] + d * d;  carry = d;
 *   for j = 1 .. J - 1:  run[j] = run[j] + carry;  if ((t + 1) mod 2^j != 0) stop;
 *                        carry = run[j];  sq[j] = sq[j] + carry * carry;  run[j] = 0;
 * so sq[j] is the sum of squares of the completed batch sums of 2^j consecutive samples.
 * gph_ess_read(a, S, level, out5), host: with b = 2^j, nb = floor(S / b),
 *   T = s1 - (((run[1] + run[2]) + ...) + run[j])   (j = 0: T = s1)
 *   vx = (sq[0] - s1 * s1 / S) / (S - 1)            vb = (sq[j] - T * T / nb) / (nb - 1)
 *   mean = shift + s1 / S     sd = sqrt(max(vx, 0))
 *   vx <= 0 (the series never changed): tau = 0 and ess = 0 -- a stuck series does not read as perfectly mixed;
 *   else tau = vb / (b * vx) (0 with fewer than two batches), ess = S / tau capped at S, tau <= 0: ess = S.
 * level < 0: j* = the largest j < J with 4^j <= S (b <= sqrt(S)).  S < 2: sd = tau = ess = 0 (S = 0: mean = 0 too).
 * out5 = mean, sd, tau, ess, the level used.  GPH_EARG: a null pointer, S < 0, level >= J.
 * gph_ess(x, S, max_lag, out8), host: the levels of x by the rule above read at j*, and the autocorrelation estimate (Geyer's
 * initial positive sequence, no monotone adjustment): d_t = x_t - x_0 (d_0 = 0), m = s1 / S, e_t = d_t - m,
 *   c_k = (sum_{t = k}^{S - 1} e_t * e_{t - k}, added from 0.0 with t ascending) / S
 *   Kmax = min(S - 2, max_lag), max_lag <= 0: 2000;  G_i = c_{2i} + c_{2i+1}, computed as the sum reaches them
 *   sum = G_0 (always taken); for i = 1, 2, ..: 2i + 1 > Kmax: truncated = 1, stop; G_i <= 0: stop; sum = sum + G_i
 *   c_0 = 0: tauAcf = essAcf = 0; else tauAcf = 2 * sum / c_0 - 1, essAcf = S / tauAcf capped at S, tauAcf <= 0: essAcf = S
 * out8 = mean, sd, tauBatch, essBatch, tauAcf, essAcf, level, truncated.  S < 2 or a null pointer: GPH_EARG. */
int gph_ess_read(const double *a /* [2 + 2 * 16] */, int64_t S, int32_t level, double *out5);
int gph_ess(const double *x, int64_t S, int32_t max_lag, double *out8);
/* ... PER SELECTED LOCUS, accumulated on the device over the samples taken (k_ess: csrc/gph_ess.h; timing class 21).  Per
 * locus M = 5 series, + 1 under `locus-mut-rate VAR`, in this order: dataLnL, genLnL, tmrca (age[root]), numMigs (clamped to
 * 0 .. GPH_GT_MAX_MIGS as a gene-tree record clamps it), topo, rate.  topo: at the first sample since the accumulators were
 * zeroed the n - 1 clade keys of the locus (W = ceil(n / 64) words each, as for the clade tables), in node-index order, are
 * stored as its FOCAL SET; x_topo of a sample = the number of internal nodes of the current tree whose clade is in the focal
 * set (1 .. n - 1, n - 1 at the first sample): the distance-to-a-focal-tree series of Lanfear et al. 2016, its ESS the
 * topological ESS.  changes[q] counts the samples t >= 1 whose clade set differs from that of sample t - 1, decided by a 64-bit
 * hash of the set (the sum of the clades' hashes): two different sets collide with probability about 2^-64.
 * Device memory per selected locus: M (2 + 2J) doubles, (n - 1) W + 1 64-bit words and one 32-bit word (1.5 KB at 16 leaves).
 *   _enable   the selection as for gph_engine_gene_trees_enable (loci NULL: all loci of the rank); GPH_EFULL, with a message and
 *             nothing allocated, above max_bytes (<= 0: 1 GiB); GPH_ESTATE before the loci are loaded.  Enabling again frees
 *             and starts over.  gph_engine_init_genealogies zeroes the accumulators and the sample count.
 *   _sample   one kernel on the engine's stream, no host synchronisation; a rank without a selected locus launches nothing
 *             and still counts the sample.  GPH_ESTATE when not enabled or before gph_engine_init_genealogies.
 *   _shape    selected loci of the rank, M, J, W, samples since the accumulators were zeroed (all 0 while off)
 *   _selected as gph_engine_gene_trees_selected
 *   _fetch    acc[selected][M][2 + 2J] (levels as above), changes[selected], focal[selected][n - 1][W] (either may be NULL),
 *             one copy and ONE host synchronisation; reset != 0 zeroes everything and the sample count afterwards.
 * The kernel writes no page, draws no random number and touches no chain state. */
int gph_engine_ess_enable(gph_engine *e, const int64_t *loci, int64_t nloci, int64_t max_bytes);
int gph_engine_ess_sample(gph_engine *e);
int gph_engine_ess_shape(gph_engine *e, int64_t *selected, int32_t *series, int32_t *levels, int32_t *words, int64_t *samples);
int gph_engine_ess_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_ess_fetch(gph_engine *e, double *acc /* [selected][series][2 + 2 levels] */, uint32_t *changes, uint64_t *focal, int32_t reset);

/* POSTERIOR PREDICTIVE CHECKS of selected loci, simulated on the device (k_predictive: csrc/gph_predictive.h; timing class 22).
 * At every sample one replicate alignment of each selected locus is drawn under the sampled genealogy (the settled node
 * records a gene-tree record holds) and locus rate (FS_MUTRATE) with JC69, the likelihood's model, and the locus's own
 * missing-data pattern, and C = 1 + Kc (Kc + 1) / 2 integer statistics are summed over its sites; the same statistics of the
 * data are formed once.  All arithmetic is uncontracted fp64 and 64-bit unsigned integers modulo 2^64.
 *   columns   the pattern rows of the locus as gph_engine_load_loci received them, in order; a column is the FIRST row of a
 *             group of phases (non-zero phase word), the others are skipped (the statistics do not depend on the order of the
 *             leaves within a population).  Column c stands for count_c sites: site s = 0, 1, ... belongs to c iff
 *             prefix_c <= s < prefix_c + count_c; a leaf with code 4 (N) is missing at them, in the data and in the replicate
 *   generator mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *             Kl = mix(seed ^ mix(g + 0x9E3779B97F4A7C15)), g the GLOBAL locus index;  K = mix(Kl + t), t = samples taken since
 *             _enable / a reset (0-based);  h(s, v) = mix(K ^ ((s << 16) | v)), site s < 2^31, node v < 2^16
 *   branches  v != root: len = rate * (age[father v] - age[v]); q_v = 0 when len < 1e-100, else 1 - exp(-4 len / 3.0) (glibc's
 *             exp); thr_v = (uint64)(q_v * 2^53); v FIRES at s iff (h(s, v) >> 11) < thr_v; the root always fires
 *   replicate the base of leaf i at s = h(s, a) & 3, a the first node on the path i, father(i), ..., root that fires at s
 *   statistics per site, cnt[p][b] = the non-missing leaves of current population p showing base b, m_p = sum_b cnt[p][b]:
 *             seg = 1 iff at least two bases b are shown by some leaf; diff_p|p = (m_p^2 - sum_b cnt[p][b]^2) / 2;
 *             diff_p|q (p < q) = m_p m_q - sum_b cnt[p][b] cnt[q][b].  Order: seg, then (p, q), p <= q, p-major
 *             (gph_engine_predictive_column_name: "seg", "diff_<p>|<q>")
 *   accumulators per (selected locus, statistic), five doubles: obs = T of the data; per sample with the replicate's T:
 *             gt += (T > obs), eq += (T == obs), s1 = s1 + T, s2 = s2 + T * T, in sample order
 *   rows      per sample the iteration and C uint64 totals of T over the rank's selected loci; the data's totals once
 *   _enable   capacity_rows per-sample rows; 0 frees everything, the feature is off.  The selection as for
 *             gph_engine_gene_trees_enable.  GPH_EARG with a message that names the locus for a selected locus whose
 *             sites x max n_p n_q reach 2^32 (or whose sites reach 2^31); GPH_EFULL, with a message and nothing allocated, above
 *             max_bytes (<= 0: 1 GiB); GPH_ESTATE before the loci are loaded.  Enabling again frees and starts over.
 *             gph_engine_init_genealogies zeroes the accumulators, the sample count and the rows held
 *   _sample   one kernel on the engine's stream, no host synchronisation; a rank without a selected locus launches nothing and
 *             still takes the (zero) row.  GPH_EFULL when the row buffer is full; GPH_ESTATE when off or before
 *             gph_engine_init_genealogies
 *   _shape    selected loci of the rank, C, samples since the accumulators were zeroed, rows held (all 0 while off)
 *   _fetch_loci  acc[selected][C][5] (obs, gt, eq, s1, s2), sites[selected] (may be NULL); one copy and one host
 *             synchronisation; reset != 0 zeroes the accumulators afterwards and restarts t at 0 (obs is formed again)
 *   _fetch_rows  the rows taken since the last call (iters[rows], rows[rows][C]) and observed[C] (may be NULL); the row buffer
 *             is empty again
 * The kernel writes no page, reads the sequence blocks read-only, and touches neither the chain state nor a locus generator. */
int gph_engine_predictive_enable(gph_engine *e, uint64_t seed, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int64_t max_bytes);
int gph_engine_predictive_sample(gph_engine *e, int32_t iteration);
int gph_engine_predictive_shape(gph_engine *e, int64_t *selected, int32_t *stats, int64_t *samples, int32_t *rows_held);
int gph_engine_predictive_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_predictive_fetch_loci(gph_engine *e, double *acc /* [selected][C][5] */, int64_t *sites, int32_t reset);
int gph_engine_predictive_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *rows_out, uint64_t *observed, int32_t max_rows, int32_t *rows);
const char *gph_engine_predictive_column_name(gph_engine *e, int32_t col);

/* TRIPLET TOPOLOGY WEIGHTS of selected loci and genome-wide per sample (k_triplets: csrc/gph_triplets.h; timing class 23): for
 * three populations P, Q, R, how often are P and Q sisters, how often P and R, how often Q and R -- the topology weighting of
 * Martin & Van Belleghem (2017, "Twisst"), the gene-tree form of the ABBA-BABA asymmetry: lineage sorting alone makes the two
 * minority topologies equally frequent, an excess of one is the signature of gene flow.
 *   populations  the Kc CURRENT populations in model order; leaf i belongs to the population whose samples hold it; n_p = its leaves
 *   triples      P < Q < R (indices of current populations) with n_P, n_Q, n_R >= 1; default all, in lexicographic order
 *   topologies   t = 0: PQ|R, 1: PR|Q, 2: QR|P; SLOT (triple, t) has number 3 triple + t
 *   per node     one locus at one sample, v an internal node with children l = left[v], r = right[v], c_x[p] = the leaves of p in
 *                the subtree of x (a leaf's own row: 1 at its population), tot[p] = n_p; for slot XY|Z
 *                    w_v(XY|Z) = (c_l[X] c_r[Y] + c_r[X] c_l[Y]) (tot[Z] - c_l[Z] - c_r[Z])
 *                = the leaf triples (a in X, b in Y, c in Z) with lca(a, b) = v and c outside v's subtree (a and b sisters
 *                relative to c); an integer <= n_X n_Y n_Z < 2^32
 *   per sample   of a slot: cnt = sum_v w_v (integer); age = sum_v age[v] (double)w_v over the internal nodes in NODE-INDEX order,
 *                terms with w_v = 0 skipped, plain uncontracted fp64 (a multiply, then an add, no fma): the summed age of the
 *                sister coalescence -- introgression makes it young, lineage sorting leaves it old
 *   invariant    per triple sum_t cnt = n_P n_Q n_R at every sample (a binary tree gives each leaf triple exactly one topology)
 *   accumulators per (selected locus, slot) two doubles: W = W + cnt (exact while S n_P n_Q n_R < 2^53), A = A + age, one plain
 *                fp64 add a sample in sample order
 *   rows         per sample the iteration and 3 T uint64 totals of cnt over the rank's selected loci (integer atomics: order-free;
 *                the rows of the ranks add); a triple's three totals sum to (selected loci) n_P n_Q n_R
 *   input        the settled node records a gene-tree record holds at that point of the chain
 *   _enable      capacity_rows per-sample rows; 0 frees everything, the feature is off.  loci: NULL = all loci of the rank, else
 *                nloci global indices, strictly increasing (those of other ranks' blocks are ignored).  triples: NULL = all, else
 *                ntriples x 3 population indices (P, Q, R) in any order; the members are sorted, the triples keep the caller's
 *                order.  GPH_EARG with a message that names the cause, nothing freed or allocated: fewer than 3 current
 *                populations; a triple that repeats a population, names an index >= Kc or a population without samples, or is
 *                named twice; a locus index >= the number of loci, negative, named twice or out of order.  GPH_EFULL, with the
 *                size in the message and the feature off, when accumulators and rows exceed max_bytes (<= 0: 1 GiB): 48 T bytes a
 *                selected locus.  GPH_ESTATE before the loci are loaded.  Enabling again frees and starts over.
 *                gph_engine_init_genealogies zeroes the accumulators, the sample count and the rows held
 *   _sample      one kernel on the engine's stream, no host synchronisation; a rank without a selected locus launches nothing and
 *                still takes the (zero) row.  GPH_EFULL when the row buffer is full; GPH_ESTATE when off or before
 *                gph_engine_init_genealogies
 *   _shape       T, 3 T, selected loci of the rank, samples since the accumulators were zeroed, rows held (all 0 while off)
 *   _fetch_loci  out[selected][ld], ld >= 6 T: W of the 3 T slots, then A of the 3 T slots; one copy and one host
 *                synchronisation; reset != 0 zeroes the accumulators and the sample count afterwards
 *   _fetch_rows  the rows taken since the last call (iters[rows], out[rows][ld], ld >= 3 T); the row buffer is empty again
 *   _column_name slot col as "<X>,<Y>|<Z>" with the indices of the current populations: X and Y are the sisters
 * The kernel writes no page, draws no random number and touches no chain state. */
int gph_engine_triplets_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, const int32_t *triples /* [ntriples][3] */,
                               int32_t ntriples, int64_t max_bytes);
int gph_engine_triplets_sample(gph_engine *e, int32_t iteration);
int gph_engine_triplets_shape(gph_engine *e, int32_t *triples, int32_t *slots, int64_t *selected, int64_t *samples, int32_t *rows_held);
int gph_engine_triplets_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_triplets_fetch_loci(gph_engine *e, double *out /* [selected][ld] */, int64_t ld, int32_t reset);
int gph_engine_triplets_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *out /* [rows][ld] */, int64_t ld, int32_t max_rows, int32_t *rows);
const char *gph_engine_triplets_column_name(gph_engine *e, int32_t col);

/* EXPECTED SUBSTITUTIONS per population branch and per sample, of selected loci and genome-wide per sample (k_mutations:
 * csrc/gph_mutations.h; timing class 24): where on the population tree the data put their mutations.  The model has one clock --
 * one rate in every population, every locus scaled by its own factor; a lineage with another rate, or a sample whose private
 * differences are errors, shows as a ratio mut / exp away from 1.  mut is the posterior expected number of substitutions given
 * the data and the sampled genealogy (partial likelihoods from below AND from above), exp what the clock expects on the same
 * exposure.  THE DEFINITION; all arithmetic is plain uncontracted fp64 in the order written, exp is gph_exp, a quotient is IEEE
 * division.
 *   locus        at one sample: n leaves, N = 2n - 1 nodes, rows 0 .. P - 1 of its sequence block.  A COLUMN is a row with a
 *                non-zero phase word together with the ph - 1 rows behind it; it stands for `count` sites (as for the predictive
 *                checks); sites = sum count; rate = FS_MUTRATE.  Node records, live migrations and log-likelihoods are the settled
 *                ones a gene-tree record holds; population ages and fathers come from the chain state (settled as for time slices)
 *   branch       above v != root with father f: t_v = age[f] - age[v], len = rate t_v, a = 4 len / 3.0,
 *                u = len < 1e-100 ? 0 : 1 - exp(-4 len / 3.0), pe = u / 4.0, qe = 1 - 4.0 pe (edge_prob and the likelihood's qe),
 *                    E_diff = (a qe) / u + 0.75 a          E_same = ((0.75 a) u) / (1 + 3 qe)
 *                the expected number of real substitutions of a JC69 path whose ends differ / are equal: exact by uniformisation,
 *                and the conditional density of substitutions along the branch is uniform, which allows splitting a branch by
 *                time.  u == 0: the branch contributes nothing
 *   per row      I_v(y) the inside conditional of v: an internal node's CURRENT half (IS_CBIT) of the conditional arrays, a leaf's
 *                one-hot vector, all ones for code 4.  Top down: O_root(x) = 1.0; for a child c of v with sibling s
 *                    U_c(x) = O_v(x) f_s(x)       f_s = child_factor of the sibling as the likelihood forms it (S >= 4 -> 1.0)
 *                    SU = ((U_c(0) + U_c(1)) + U_c(2)) + U_c(3)        O_c(y) = pe_c SU + qe_c U_c(y)
 *                with J_x = the sum of I_c(y) over y != x in increasing y
 *                    D_c(row) = pe_c (((U_c(0) J_0 + U_c(1) J_1) + U_c(2) J_2) + U_c(3) J_3)
 *                the posterior mass of "the ends of the branch differ" (every term positive: no cancellation);
 *                R(row) = ((r0 + r1) + r2) + r3 of the root's conditionals
 *   per column   j and branch: DD = sum D, RR = sum R over the column's rows in row order; d = DD / RR (0 where RR == 0);
 *                Dv = sum_j (double)count_j d in column order; M_v = E_same (sites - Dv) + E_diff Dv.  A missing leaf needs no
 *                special case: its all-ones vector gives the prior expectation
 *   segments     of the branch above v: cur = npop[v], t = age[v]; the events are the live migrations whose branch is v by
 *                increasing age (equal ages in `living` order), then age[f].  Before an event at age b: while cur has a father
 *                population F with popAge[F] <= b, close (cur, popAge[F] - t), cur = F, t = popAge[F]; then close (cur, b - t),
 *                t = b; at a migration cur = the band's source population (below the migration node the lineage is in the target
 *                population, above it in the source).  Every loop is bounded: a record that does not fit still terminates.
 *                Segment (p, dt): mut_p = mut_p + M_v (dt / t_v), exp_p = exp_p + (rate dt) sites; nodes in index order, then
 *                segments in time order.  Leaf i: mutExt_i = M_i, expExt_i = (rate t_i) sites
 *   columns      C = 2 (K + n): mut_p and exp_p of the K populations (model order), then mutExt_i and expExt_i of the n leaves
 *   accumulators per selected locus C doubles, acc = acc + value, one plain fp64 add a sample in sample order
 *   rows         per sample 1 + C doubles: the iteration, then the C columns summed over the rank's selected loci WITHOUT fp
 *                atomics -- the loci of a chunk of `chunk` selected loci in selection order (from 0.0), the chunks in chunk order
 *                (from 0.0; k_rows_fold): a row is rebuilt bit for bit for a given selection and rank count.  Ranks' rows add in
 *                rank order
 *   _enable      capacity_rows per-sample rows; 0 frees everything, the feature is off.  loci as gph_engine_triplets_enable, with
 *                its refusals (GPH_EARG with a message that names the cause, nothing freed or allocated) and its limit: GPH_EFULL,
 *                with the size in the message and the feature off, when accumulators, partial rows and rows exceed max_bytes
 *                (<= 0: 1 GiB).  GPH_EARG with a message where one row of a locus no longer fits the samplers' 40 KB of LDS (more than
 *                about 180 leaves).  GPH_ESTATE before the loci are loaded.  gph_engine_init_genealogies zeroes the accumulators,
 *                the sample count and the rows held
 *   _sample      k_mutations and the fold on the engine's stream, no host synchronisation; a rank without a selected locus
 *                launches the fold alone.  GPH_EFULL when the row buffer is full; GPH_ESTATE when off or before
 *                gph_engine_init_genealogies
 *   _shape       C, the chunk size, selected loci of the rank, samples since the accumulators were zeroed, rows held (0 while off)
 *   _fetch_loci  out[selected][ld], ld >= C; one copy and one host synchronisation; reset != 0 zeroes the accumulators and the
 *                sample count afterwards
 *   _fetch_rows  the rows taken since the last call, out[rows][1 + C]; the row buffer is empty again
 *   _column_name column col of the C: "mut.<p>", "exp.<p>", "mutExt.<i>", "expExt.<i>"
 * The kernel writes no page, draws no random number and touches no chain state. */
int gph_engine_mutations_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int64_t max_bytes);
int gph_engine_mutations_sample(gph_engine *e, int32_t iteration);
int gph_engine_mutations_shape(gph_engine *e, int32_t *columns, int32_t *chunk, int64_t *selected, int64_t *samples, int32_t *rows_held);
int gph_engine_mutations_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_mutations_fetch_loci(gph_engine *e, double *out /* [selected][ld] */, int64_t ld, int32_t reset);
int gph_engine_mutations_fetch_rows(gph_engine *e, double *out /* [rows][1 + C] */, int32_t max_rows, int32_t *rows);
const char *gph_engine_mutations_column_name(gph_engine *e, int32_t col);

/* REPLICATE GENEALOGIES simulated from the sampled parameters, of selected loci and genome-wide per sample (k_simulate:
 * csrc/gph_simulate.h; timing class 25).  The predictive checks above redraw the data ON the sampled genealogy and so test the
 * mutation process alone; here the replicate is drawn from the parameters, G_rep ~ p(G | Theta_s) by direct simulation of the
 * structured coalescent with migration, and D_rep ~ p(D | G_rep) on it: the check of the demographic model against the data, the
 * realized discrepancy T(G_s, Theta_s) against T(G_rep, Theta_s) of the sampled genealogies against their prior, and -- at beta 0,
 * where G_s and G_rep are exchangeable -- a check of the sampler itself: every mid-p must centre on 0.5.
 * THE DEFINITION; all arithmetic is plain uncontracted fp64 in the order written, log is the engine's own (glibc's log bit for bit), x / theta_p the
 * correctly rounded quotient, every other quotient IEEE division.
 *   model      theta, popAge, sampleAge, popFather, migRate, bandStart, bandEnd, bandSrc, bandTgt of the chain state (settled as for
 *              the time slices); leaf i belongs to the current population whose samples hold it
 *   generator  mix as for the predictive checks.  Kl = mix((seed ^ 0x53494D554C415445) ^ mix(g + 0x9E3779B97F4A7C15)), g the GLOBAL
 *              locus index; Ks = mix(Kl + t), t = samples taken since _enable / a reset; Ka = mix(Ks + (a + 1) 0xD1B54A32D192ED03)
 *              for attempt a = 0 .. 15; draw d = 0, 1, ... of the attempt: u_d = ((mix(Ka ^ d) >> 12) + 0.5) 2^-52, in (0, 1)
 *   lineages   a list of (node, population).  enter(t): every current population p in index order that has not entered and has
 *              sampleAge[p] <= t enters -- its leaves are appended in leaf order, each in p, leaf age sampleAge[p] --; then every
 *              lineage in list order climbs: while its population has a father F with popAge[F] <= t it moves to F
 *   start      t = 0; enter(0)
 *   step       one lineage left and every population entered: the end; the root is node N - 1.  Else with c[p] = the lineages in p:
 *              rates in this order -- p = 0 .. K - 1 with c[p] >= 2: r = (c (c - 1)) / theta_p; b = 0 .. B - 1 with bandStart[b] <= t
 *              < bandEnd[b] and c[tgt b] >= 1: r = c[tgt b] migRate[b] --, R = R + r from 0.0 in that order.  nb = the smallest of
 *              popAge[p] (p >= Kc), sampleAge[p] (p < Kc), bandStart[b], bandEnd[b] that is > t (none: infinity).  u = the next
 *              draw (spent whatever follows); w = -log(u) / R.  If !(R > 0) or t + w >= nb: t' = nb (a BOUNDARY), else t' = t + w.
 *              t' infinite: the attempt fails.  dt = t' - t; exposures: coal_p = coal_p + (c (c - 1)) dt for c[p] >= 2, mig_b =
 *              mig_b + c[tgt b] dt for the bands live at t with c >= 1.  t = t'.  A boundary: enter(t), next step.  Else x = u' R
 *              with the next draw u'; walking the non-zero rates in the same order, acc = acc + r from 0.0, the event is the first
 *              with x < acc; the last non-zero rate takes the rounding residue
 *   coalescence in p, c = c[p]: two further draws u, u': a = min(int(u c), c - 1), b = min(int(u' (c - 1)), c - 2), b += (b >= a);
 *              the a-th and b-th lineages of p in list order.  Node v = n + (coalescences so far): age t, npop p, left = the one
 *              earlier in the list, right = the later; v takes the earlier slot, the later slot is removed, the order is kept
 *   migration  in b: with GPH_GT_MAX_MIGS migrations recorded already the attempt is ABANDONED and redrawn with the next a (the
 *              chain's prior is truncated there, so the rejection is exact).  One further draw u: k = min(int(u c[tgt b]), c - 1);
 *              the k-th lineage of tgt b in list order moves to bandSrc[b]; migration m = (migrations so far): branch = its node,
 *              band b, spop = bandSrc[b], tpop = bandTgt[b], age t, living[m] = m
 *   failed     after 16 attempts: the replicate of the locus at that sample is FAILED -- counted per locus and in the row's
 *              `failed` column, left out of every statistic; its record is all zero with root -1
 *   record     the layout of a gene-trees record (gph_engine_gene_trees_shape's offsets; gph_gene_trees_decode and
 *              gph_gene_tree_newick read it unchanged); dataLnL = 0; genLnL as the engine's gtree_lnl forms it, every population
 *              and band, no constant: lnL = 0.0; p = 0 .. K - 1: lnL += n_p log(2 / theta_p) - coal_p / theta_p; b = 0 .. B - 1 with
 *              migRate[b] > 0: lnL += m_b log(migRate[b]) - mig_b migRate[b], n_p / m_b the replicate's coalescences / migrations
 *   statistics M = 3 + K + B: tmrca (the root's age), length (the sum over the nodes v != root in node order of age[father v] -
 *              age[v]), genLnL, coal_<p>, mig_<b>.  x on the sampled genealogy (settled node records, the page's counts and
 *              genLnL), y on the replicate.  Per (selected locus, statistic) five doubles in sample order: gt += (y > x), eq +=
 *              (y == x), sx = sx + x, sy = sy + y, sy2 = sy2 + y y; behind the 5 M one double: the failed replicates
 *   sites      (with_sites) the replicate alignment is drawn on the replicate genealogy with the locus's rate and missing-data
 *              pattern by the predictive checks' own site loop -- everything as defined there with K = mix(Kl' + t), Kl' =
 *              mix((seed ^ 0x53494D554C415445 ^ 0x5349544553) ^ mix(g + 0x9E3779B97F4A7C15)) --: C statistics a locus, five
 *              doubles obs, gt, eq, s1, s2 each.  A failed replicate adds nothing
 *   rows       per sample the iteration and 2 (K + B) + 4 + C uint64 totals over the rank's selected loci (integer atomics; the
 *              rows of the ranks add): the sampled coal_p, mig_b, the replicate's coal_p, mig_b, the loci with y > x for tmrca,
 *              length, genLnL, `failed`, then the replicate's C site totals; the data's site totals once
 *   _enable    capacity_rows per-sample rows; 0 frees everything, the feature is off.  The selection, the refusals and the limits
 *              as for gph_engine_predictive_enable (the 2^32 bound only with_sites); GPH_EFULL above max_bytes (<= 0: 1 GiB)
 *   _sample    k_simulate, then (with_sites) the site loop, on the engine's stream, no host synchronisation; a rank without a
 *              selected locus launches nothing and still takes the (zero) row.  GPH_EFULL when the row buffer is full
 *   _shape     selected loci of the rank, M, C (0 without sites), the columns of a row, the bytes of a record, samples since the
 *              accumulators were zeroed, rows held (all 0 while off)
 *   _fetch_loci   acc[selected][5 M + 1], site_acc[selected][C][5] (may be NULL), sites[selected] (may be NULL); reset != 0 zeroes
 *              the accumulators afterwards and restarts t at 0
 *   _fetch_rows   as gph_engine_predictive_fetch_rows, observed[C]
 *   _fetch_records  the latest sample's replicates, out[selected][record bytes]; offsets[GPH_GT_O_COUNT] (may be NULL)
 *   _column_name  which 0: statistic col; 1: row column col ("s.", "r." for sampled / replicate, "gt.", "failed"); 2: site statistic
 * The kernels write no page and touch neither the chain state nor a locus generator. */
int gph_engine_simulate_enable(gph_engine *e, uint64_t seed, int32_t capacity_rows, const int64_t *loci, int64_t nloci, int32_t with_sites,
                               int64_t max_bytes);
int gph_engine_simulate_sample(gph_engine *e, int32_t iteration);
int gph_engine_simulate_shape(gph_engine *e, int64_t *selected, int32_t *stats, int32_t *site_stats, int32_t *row_columns, int32_t *record_bytes,
                              int64_t *samples, int32_t *rows_held);
int gph_engine_simulate_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_simulate_fetch_loci(gph_engine *e, double *acc /* [selected][5 M + 1] */, double *site_acc /* [selected][C][5] */, int64_t *sites,
                                   int32_t reset);
int gph_engine_simulate_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *rows_out, uint64_t *observed, int32_t max_rows, int32_t *rows);
int gph_engine_simulate_fetch_records(gph_engine *e, void *out /* [selected][record bytes] */, int32_t *offsets);
const char *gph_engine_simulate_column_name(gph_engine *e, int32_t which, int32_t col);

/* PAIRWISE COALESCENCE-TIME DISTRIBUTIONS per population pair, of selected loci and genome-wide per sample (k_pair_times:
 * csrc/gph_pairtimes.h; timing class 26): the distribution of the coalescence time of a lineage from population P and a lineage
 * from population Q on an ABSOLUTE time axis -- the curve set next to an MSMC or Relate cross-coalescence curve: it shows when two
 * populations stopped exchanging lineages, whether the model has a band for it or not.  In a model without gene flow a P-Q
 * coalescence cannot be younger than the split of P and Q, so "the youngest P-Q coalescence of this locus lies below the split"
 * is a statement about the locus that needs no band index.
 *   populations  the Kc CURRENT populations in model order; n_p = the leaves of p
 *   pairs        (P, Q), P <= Q, with m_PQ >= 1 leaf pairs: m_PQ = n_P n_Q for P < Q, m_PP = n_P (n_P - 1) / 2; default all such
 *                pairs in lexicographic order; pair number k is SLOT k, NP their number
 *   grid         E = B - 1 EDGES e_0 < e_1 < ... < e_{E-1}, finite positive doubles in the genealogy's own units (as tmrca),
 *                1 <= E <= 127; bin(a) = the number of edges e <= a: an age equal to an edge lies in the upper bin; bin 0 is
 *                [0, e_0), bin B - 1 is [e_{E-1}, inf).  The engine takes the edges as given
 *   per node     one locus at one sample, v an internal node with children l, r, c_x[p] = the leaves of p under x:
 *                    w_v(P, Q) = c_l[P] c_r[Q] + c_r[P] c_l[Q]   (P < Q),      w_v(P, P) = c_l[P] c_r[P]
 *                = the leaf pairs of the slot whose lca is v; an integer <= 200^2, never enumerated
 *   split        from popAge and popFather of the chain state at the sample: P < Q the age of the youngest population that is an
 *                ancestor of both; P = Q the age of P's father population, +inf when P has none
 *   per sample   of a slot, all sums over the internal nodes in NODE-INDEX order, terms with w_v = 0 skipped, plain uncontracted
 *                fp64 (a multiply, then an add):
 *                    hist[k] = sum_{bin(age[v]) = k} w_v        a = sum age[v] (double)w_v        y = sum_{age[v] < split} w_v
 *                    x = [y > 0]                                tmin = the smallest age[v] with w_v > 0
 *   invariants   sum_k hist[k] = m_PQ and y <= m_PQ at every sample
 *   accumulators per (selected locus, slot) four doubles: A += a, Y += y, X += x, M += tmin, one plain fp64 add a sample in sample
 *                order; layout [locus][A | Y | X | M][slot]: 32 NP bytes a locus.  There are no per-locus histograms
 *   rows         per sample the iteration and NP (B + 2) uint64 over the rank's selected loci: per slot the B hist totals, then per
 *                slot the y total, then per slot the number of loci with x = 1 (integer atomics: order-free; the rows of the ranks add)
 *   input        the settled node records a gene-tree record holds at that point of the chain, and the chain state's popAge
 *   _enable      capacity_rows per-sample rows; 0 frees everything, the feature is off.  loci as gph_engine_triplets_enable.  pairs:
 *                NULL = all, else npairs x 2 population indices in any order; the members are sorted, the pairs keep the caller's
 *                order.  edges [nedges].  GPH_EARG with a message that names the cause, nothing freed or allocated: a locus index
 *                out of range, named twice or out of order; a pair that names an index outside 0 .. Kc - 1, is named twice (after
 *                sorting) or has no leaf pair ("population p has fewer than two samples" for P = Q); nedges outside 1 .. 127; an
 *                edge that is non-finite, <= 0 or not above its predecessor, by index; more than 255 leaves; more than 64 KB of
 *                LDS at one locus a workgroup.  GPH_EFULL, with the size in the message and the feature off, when accumulators and
 *                rows exceed max_bytes (<= 0: 1 GiB).  GPH_ESTATE before the loci are loaded.  Enabling again frees and starts
 *                over.  gph_engine_init_genealogies zeroes the accumulators, the sample count and the rows held
 *   _sample      one kernel on the engine's stream, no host synchronisation; a rank without a selected locus launches nothing and
 *                still takes the (zero) row.  GPH_EFULL when the row buffer is full; GPH_ESTATE when off or before
 *                gph_engine_init_genealogies
 *   _shape       NP, B, the loci a workgroup takes, selected loci of the rank, samples since the accumulators were zeroed, rows
 *                held (all 0 while off); edges_out [B - 1] (may be NULL): the grid as given
 *   _fetch_loci  out[selected][ld], ld >= 4 NP: A of the NP slots, then Y, X, M; one copy and one host synchronisation; reset != 0
 *                zeroes the accumulators and the sample count afterwards
 *   _fetch_rows  the rows taken since the last call (iters[rows], out[rows][ld], ld >= NP (B + 2)); the row buffer is empty again
 *   _column_name column col of a row: "<P>|<Q>:<k>" per slot and bin, then "below_<P>|<Q>" per slot, then "loci_<P>|<Q>" per slot,
 *                with the indices of the current populations
 * The kernel writes no page, draws no random number and touches no chain state; there are no fp atomics.  Not built: coalescence
 * rates / hazard estimates and a relative cross-coalescence ratio, per-locus histograms, pairs of ancestral populations. */
int gph_engine_pair_times_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, const int32_t *pairs /* [npairs][2] */,
                                 int32_t npairs, const double *edges, int32_t nedges, int64_t max_bytes);
int gph_engine_pair_times_sample(gph_engine *e, int32_t iteration);
int gph_engine_pair_times_shape(gph_engine *e, int32_t *pairs, int32_t *bins, int32_t *group, int64_t *selected, int64_t *samples, int32_t *rows_held,
                                double *edges_out);
int gph_engine_pair_times_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_pair_times_fetch_loci(gph_engine *e, double *out /* [selected][ld] */, int64_t ld, int32_t reset);
int gph_engine_pair_times_fetch_rows(gph_engine *e, int32_t *iters, uint64_t *out /* [rows][ld] */, int64_t ld, int32_t max_rows, int32_t *rows);
const char *gph_engine_pair_times_column_name(gph_engine *e, int32_t col);

/* SITE-FREQUENCY SPECTRA, data against sampled genealogies, of selected loci and genome-wide per sample (k_sfs_tree, k_sfs_data:
 * csrc/gph_sfs.h; timing classes 27 and 28): the folded site-frequency spectrum of every current population and the split of the
 * variable sites of two populations into private, shared and fixed (Wakeley & Hey 1997) -- what the data show next to what the
 * sampled genealogies expect (Fu 1995: the branch length under each frequency class).  Growth or a bottleneck on a branch, or a
 * sample whose singletons are errors, changes the SHAPE of the spectrum far more than the mean pairwise difference.
 *   populations  the Kc CURRENT populations in model order; n_p = the leaves of p
 *   slots        NS of them.  For every p with n_p >= 2, in population order, the folded bins k = 1 .. n_p / 2 ("sfs_<p>:<k>");
 *                then for every pair P < Q taken, four classes in this order: privP, privQ, shared, fixed.  Default: all pairs
 *                with n_P, n_Q >= 1 in lexicographic order
 *   groups       NG of them: what shares a denominator, one per population with bins, then one per pair
 *   genealogy    one locus at one sample, from the settled node records a gene-tree record holds and the locus rate of the page:
 *                every non-root node v in NODE-INDEX order, len_v = age[father v] - age[v] (leaf ages are the records': an
 *                ancient sample's branch starts at its age), c_v[p] = the leaves of p under v (a leaf counts for its own
 *                population whatever migrations lie on the branch).
 *                    v is in sfs_p:k iff 0 < c_v[p] < n_p and min(c_v[p], n_p - c_v[p]) = k (c = n_p / 2 at even n_p: once)
 *                    a = c_v[P], b = c_v[Q], "a inside" = 0 < a < n_P:
 *                    privP iff a inside and b in {0, n_Q};  privQ iff b inside and a in {0, n_P};  shared iff both inside;
 *                    fixed iff (a, b) = (n_P, 0) or (0, n_Q);  otherwise none of the four
 *                per slot x = sum len_v over its nodes, plain uncontracted fp64 adds in node order from 0.0; e = rate x, one
 *                multiply: the expected substitutions PER SITE that fall in the class
 *   data         one locus, once at enable.  Its columns are the rows with a non-zero phase word, each standing for `count`
 *                sites, as the predictive checks define them; the codes read are the column's own row (both haplotypes of a
 *                diploid lie in one population, so a population's counts do not depend on the phase row read).
 *                    p is USABLE at a column iff all n_p leaves have a code below 4 and show two distinct bases at most: the
 *                    column adds count to use_p and, with k >= 1 carriers of the rarer base, to obs[sfs_p:k]
 *                    a pair is usable iff all leaves of P and Q are non-missing and P u Q shows two bases at most: count to
 *                    use_PQ and to one class at most: polymorphic in P only, in Q only, in both, or monomorphic in each with
 *                    different bases
 *                u32 per (selected locus, slot or group), and `sites`; a selected locus whose sites reach 2^32 is refused
 *   accumulators per (selected locus, slot) one double, E = E + e: one plain add a sample, rebuilt bit for bit
 *   rows         per sample 1 + NS doubles: the iteration, then per slot sum_loci (double)use_group(slot) e -- the expected
 *                number of SITES of the class among the usable ones; the loci of a workgroup's G consecutive selected loci are
 *                added in selection order from 0.0, the workgroups' partial rows then in workgroup order from 0.0 (no fp atomics)
 *   observed     the totals of obs, use and sites over the rank's selected loci, uint64
 *   meaning      under the model and infinite sites obs / expected is 1 per slot; JC69 multiple hits lower the observed counts by
 *                a relative amount of the order of the tree's length in substitutions per site.  No exactness is claimed beyond
 *                the definitions above
 *   _enable      capacity_rows per-sample rows; 0 frees everything, the feature is off.  loci as gph_engine_triplets_enable.
 *                pairs: NULL = all, else npairs x 2 population indices in any order (npairs 0 with a non-null pointer: none); the
 *                members are sorted, the pairs keep the caller's order.  GPH_EARG with a message that names the cause, nothing
 *                freed or allocated: a locus index out of range, named twice or out of order; a locus whose sites reach 2^32; a
 *                pair that names an index outside 0 .. Kc - 1, one population twice, a population without a sample, or is named
 *                twice (after sorting); no slot at all (no population has two samples and no pair is taken); more than 255
 *                leaves; more than 64 KB of LDS at one locus a workgroup.  GPH_EFULL, with the size in the message and the
 *                feature off, when accumulators, tables and rows exceed max_bytes (<= 0: 1 GiB).  GPH_ESTATE before the loci are
 *                loaded.  Enabling again frees and starts over.  k_sfs_data runs here, once.  gph_engine_init_genealogies zeroes
 *                E, the sample count and the rows held; the data side stays
 *   _sample      k_sfs_tree and the fold on the engine's stream, no host synchronisation; a rank without a selected locus
 *                launches the fold alone.  GPH_EFULL when the row buffer is full; GPH_ESTATE when off or before
 *                gph_engine_init_genealogies
 *   _shape       NS, NG, G, selected loci of the rank, samples since E was zeroed, rows held (all 0 while off)
 *   _slots       out[NS][5]: group, kind (0 a bin, 1 .. 4 privP, privQ, shared, fixed), P, Q (P again for a bin), k (0 for a class)
 *   _fetch_loci  out[selected][ld], ld >= NS: E; reset != 0 zeroes E and the sample count afterwards
 *   _fetch_observed  out[selected][ld], ld >= NS + NG + 1: obs per slot, use per group, sites; totals[NS + NG + 1] (may be NULL)
 *   _fetch_rows  the rows taken since the last call, [rows][1 + NS]; the row buffer is empty again
 *   _column_name col < NS: "sfs_<p>:<k>" or "privP_<P>|<Q>", "privQ_", "shared_", "fixed_"; NS <= col < NS + NG: the group, "<p>"
 *                or "<P>|<Q>"; with the indices of the current populations
 * The kernels write no page, draw no random number and touch no chain state.  Not built: a replicate-based (exact, p-valued)
 * spectrum check through k_predictive's generator, unfolded spectra, joint spectra beyond the four classes. */
int gph_engine_sfs_enable(gph_engine *e, int32_t capacity_rows, const int64_t *loci, int64_t nloci, const int32_t *pairs /* [npairs][2] */, int32_t npairs,
                          int64_t max_bytes);
int gph_engine_sfs_sample(gph_engine *e, int32_t iteration);
int gph_engine_sfs_shape(gph_engine *e, int32_t *slots, int32_t *groups, int32_t *group, int64_t *selected, int64_t *samples, int32_t *rows_held);
int gph_engine_sfs_selected(gph_engine *e, int64_t *out, int64_t max_loci, int64_t *count);
int gph_engine_sfs_slots(gph_engine *e, int32_t *out /* [NS][5] */);
int gph_engine_sfs_fetch_loci(gph_engine *e, double *out /* [selected][ld] */, int64_t ld, int32_t reset);
int gph_engine_sfs_fetch_observed(gph_engine *e, uint32_t *out /* [selected][ld] */, int64_t ld, uint64_t *totals);
int gph_engine_sfs_fetch_rows(gph_engine *e, double *out /* [rows][1 + NS] */, int32_t max_rows, int32_t *rows);
const char *gph_engine_sfs_column_name(gph_engine *e, int32_t col);

/* ------------------------------------------------------------------------------------
 * host MCMC driver: the iteration body of performMCMC (GPhoCS.c:1476-1821) above the
 * engine: general-slot RNG, priors, accept decisions of the global proposals
 * (UpdateTheta GPhoCS.c:3037, UpdateMigRates :3115, UpdateTau :3224 host part,
 * UpdateSampleAge :4006 host part, mixing :4688 host part), accumulators dataState.{logLikelihood,dataLogLikelihood}. */
typedef struct {
  const double *thetaAlpha, *thetaBeta, *thetaStart;   /* [K] */
  const double *ageAlpha, *ageBeta, *ageStart;         /* [K] (ancestral pops) */
  const double *sampleAge;                             /* [K] */
  const int32_t *updateSampleAge;                      /* [K] 1 = estimated ("age x e"), NULL = none */
  const double *mrAlpha, *mrBeta;                      /* [B] */
  double ftCoalTime, ftMigTime, ftTheta, ftMigRate, ftMixing;
  const double *ftTaus;                                /* [K] */
  int32_t seed, startMig, doMixing, samplesPerLog;
  int32_t numParameters;
  const double *printFactors;                          /* [numParameters] */
  int32_t mutRateMode;                                 /* 0 CONST, 1 VAR (UpdateLocusRate runs, GPhoCS.c:1554), 2 FIXED */
  double varRatesAlpha, ftLocusRate;                   /* locus-mut-rate VAR <alpha>, finetune-locus-rate */
} gph_mcmc_config;

int gph_mcmc_create(gph_engine *e, const gph_config *cfg, const gph_mcmc_config *mc, gph_mcmc **out);
void gph_mcmc_destroy(gph_mcmc *m);
int gph_mcmc_initialize(gph_mcmc *m, int64_t *totalCoals);
/* optional record file: one "IT <iter> <proposal> <accepted> <dataLnL %a> <logL %a>" line per
 * proposal call and one TRACE line per iteration (the unchanged trace-file row format) */
int gph_mcmc_set_record_file(gph_mcmc *m, const char *path);
int gph_mcmc_iteration(gph_mcmc *m, int32_t iteration);
int gph_mcmc_get_state(gph_mcmc *m, double *logLikelihood, double *dataLogLikelihood, double *theta,
                       double *popAge, double *migRate);
int gph_mcmc_dump_state(gph_mcmc *m, const char *path, int32_t withConditionals);
int gph_mcmc_accept_counts(gph_mcmc *m, int64_t *counts9);
/* cumulative accepted UpdateTau (ancestral) / UpdateSampleAge (current, estimated age) proposals per population [K] */
int gph_mcmc_tau_accept_counts(gph_mcmc *m, int64_t *perPop);
/* new step sizes (the find-finetunes search of performMCMC, GPhoCS.c:1896-2180, changes them between log periods);
 * taus [K] or NULL = unchanged */
int gph_mcmc_set_finetunes(gph_mcmc *m, double coalTime, double migTime, double theta, double migRate, double mixing,
                           const double *taus);
/* iterations between two checkAll() resynchronisations (= the log period, GPhoCS.c:1811-1821; the find-finetunes
 * phase uses find-finetunes-samples-per-step instead of iterations-per-log) */
int gph_mcmc_set_log_period(gph_mcmc *m, int32_t iterations);
/* finetune-locus-rate (changed by the find-finetunes search), and the running state of UpdateLocusRate:
 * cumulative accept count and dataState.rateVar */
int gph_mcmc_set_locus_rate_finetune(gph_mcmc *m, double locusRate);
int gph_mcmc_locus_rate_state(gph_mcmc *m, int64_t *accepted, double *rateVar);
/* recordParamVals (GPhoCS.c:802-849) of the last iteration: thetas, taus, migration rates, sample ages */
int gph_mcmc_param_vals(gph_mcmc *m, double *vals, int32_t n);
/* Power posterior (heated chain): the chain samples p(D | G)^beta p(G | Theta) p(Theta).  beta multiplies the change of the
 * data log-likelihood in every acceptance ratio that has one -- UpdateGB_InternalNode, UpdateGB_MigSPR, UpdateLocusRate,
 * UpdateTau / UpdateSampleAge, mixing -- and nothing else: not the draws or their order, not the genealogy term, the priors
 * or the Hastings factors.  beta = 1 (the default) is the posterior, bit for bit the chain without this call; beta = 0 samples
 * the prior.  Finite and in [0, 64], else GPH_EARG.  It takes effect from the next proposal call, gph_mcmc_iteration and every
 * proposal-level call of the drop-in boundary below included (gph_engine_genealogy_sweep and gph_engine_locus_rate_update,
 * which decide on the device, too).  What the chain RECORDS stays unheated: dataLogLikelihood / logLikelihood, the trace
 * columns, the per-locus values, checkAll are those of the plain likelihood.  With several ranks every rank must be given the
 * same beta (nothing is exchanged for it): ranks that differ take different decisions and the chain is undefined. */
int gph_engine_set_beta(gph_engine *e, double beta);
int gph_engine_get_beta(gph_engine *e, double *beta);
int gph_mcmc_set_beta(gph_mcmc *m, double beta);
int gph_mcmc_get_beta(gph_mcmc *m, double *beta);

/* Metropolis-coupled chains (MC3) on one device.
 * gph_engine_exchange_state / gph_mcmc_exchange_state: afterwards a holds the chain STATE b held and the reverse -- per locus
 * the genealogies, event chains, statistics, generator triples, likelihoods, conditional arrays and (locus-mut-rate VAR) rates;
 * above the loci everything gph_chain_state carries (below), and at the gph_mcmc level rateVar and the recorded parameter
 * values.  Each side KEEPS its beta, step sizes, priors, accept counters, log period, record file, samplers and counters.
 * Device pointers change hands, nothing is copied; the host does not wait for the device; the two engines' streams are
 * ordered through events.  A commit the engine still owed to its pages runs first (one launch at most).  GPH_EARG, and nothing
 * changed, unless: a != b, both initialised and without a recorded error, same device, same library variant, the same loci in
 * the same layout and slot order (two engines loaded from the same arrays), no communicator and no all-reduce hook on either.
 * gph_mcmc_exchange_state is the call for chains driven by gph_mcmc_iteration; the engine-level call is its per-locus and
 * chain-state part for a caller with a driver of its own.
 *
 * gph_mc3: a group of C = 2 .. 16 chains the caller created and initialised, and goes on owning.  _create gives chain c
 * betas[c] (gph_mcmc_set_beta) for good.  _iteration is call number t = 0, 1, ... and does two things in this order.  (1) When
 * swap_every > 0, t > 0 and t % swap_every == 0: two uniforms u1, u2 from the group's own generator -- the general slot's
 * generator (utils.c:421-426, 459-470) seeded with swap_seed -- pick the pair j = min((int)(u1 (C - 1)), C - 2) and decide:
 * with l_c chain c's dataLogLikelihood (unheated, as gph_mcmc_get_state gives it), lnr = (beta_j - beta_j+1) (l_j+1 - l_j);
 * the swap is accepted iff lnr >= 0 or log(u2) < lnr, and then chains j and j + 1 exchange their states.  One gph_mc3_swap is
 * appended to the log either way (u = u2).  (2) gph_mcmc_iteration(chains[c], iteration) for every c, one host thread a chain,
 * joined before the call returns; the first failure is returned (with the chain's index on stderr) and stops the group.
 * Chain 0 holds beta_0 throughout, so with beta_0 = 1 its trace, samplers and outputs describe the posterior.
 * _swap_counts: attempts and accepted swaps of pair (c, c + 1), C - 1 values each (either may be NULL).  _swap_log: *count =
 * decisions so far; with out != NULL they are copied (GPH_EARG when max is too small). */
typedef struct gph_mc3 gph_mc3;
typedef struct { int32_t call, lower; double beta_lower, beta_upper, l_lower, l_upper, lnr, u; int32_t accepted, pad; } gph_mc3_swap;
int gph_engine_exchange_state(gph_engine *a, gph_engine *b);
int gph_mcmc_exchange_state(gph_mcmc *a, gph_mcmc *b);
int gph_mc3_create(gph_mcmc *const *chains, int32_t C, const double *betas, int32_t swap_every, uint32_t swap_seed, gph_mc3 **out);
void gph_mc3_destroy(gph_mc3 *g);                       /* the chains stay the caller's */
int gph_mc3_iteration(gph_mc3 *g, int32_t iteration);
int gph_mc3_swap_counts(gph_mc3 *g, int64_t *attempts, int64_t *accepted);
int gph_mc3_swap_log(gph_mc3 *g, gph_mc3_swap *out, int64_t max, int64_t *count);

/* ------------------------------------------------------------------------------------
 * input front end (host only, no GPU): the reference's file formats, unchanged.
 *   gph_control_read   readControlFile + readSecondaryControlFile + checkSettings +
 *                      finalizeNumParameters              (MCMCcontrol.c:118-463, 575-1478)
 *   gph_loci_read      readSeqFile + processLocusAlignment + processHetPatterns
 *                      (AlignmentProcessor.c:468-1158, 1595-1894, 2242-2339) and readRateFile
 *                      (GPhoCS.c:491-579); the result is what gph_engine_load_loci takes
 *   gph_run_control_file   main() + the trace-file side of performMCMC (GPhoCS.c:84-238, 1232-1330,
 *                      1763-1769): same control file, same sequence file, same trace file */
typedef struct gph_control gph_control;
typedef struct gph_loci gph_loci;
typedef struct {
  const char *seqFile, *traceFile, *rateFile;
  int32_t numLoci;          /* num-loci of the control file, -1 = all loci of the sequence file */
  int32_t burnin, numSamples, sampleSkip, logsPerLine;
  int32_t mutRateMode;      /* 0 CONST, 1 VAR, 2 FIXED */
  int32_t findFinetunes, findFinetunesNumSteps, findFinetunesSamplesPerStep;
  int32_t numSampleSlots;   /* haploid leaves per locus (a diploid sample takes two) */
  double varRatesAlpha, ftLocusRate;
} gph_control_info;
int gph_control_read(const char *ctl_path, const char *secondary_ctl_path_or_null, gph_control **out);
void gph_control_free(gph_control *c);
/* fills any non-NULL output; pointers inside stay owned by (and valid as long as) the control object */
int gph_control_get(const gph_control *c, gph_config *cfg, gph_mcmc_config *mc, gph_control_info *info);
const char *gph_control_pop_name(const gph_control *c, int32_t pop);
const char *gph_control_sample_name(const gph_control *c, int32_t slot);   /* "" = second haploid of a diploid */
/* seq_path NULL = the control file's seq-file; threads <= 0 = all host threads; err receives the
 * reference's error text when the file is rejected */
int gph_loci_read(const gph_control *c, const char *seq_path, int32_t threads, gph_loci **out, char *err, int32_t errlen);
void gph_loci_free(gph_loci *l);
int gph_loci_arrays(const gph_loci *l, int64_t *L, int32_t *n, const int64_t **pattern_offsets, const uint8_t **leafcodes,
                    const uint16_t **numPhases, const int32_t **counts, const double **mutRates, const int32_t **unphased);
/* name of locus g (0-based, sequence-file order) as the sequence file gives it; NULL if g is out of range */
const char *gph_loci_name(const gph_loci *l, int64_t g);
int gph_run_control_file(const char *ctl_path, const char *secondary_ctl_path_or_null, int32_t device, int32_t verbose);
/* the same chain over `world` processes, one per GPU: every rank reads the files, holds the contiguous block
 * rank*ceil(L/world) .. of the loci, runs the same host code on the same general RNG stream and combines the
 * reduced vectors through `allreduce` (see gph_engine_set_allreduce); rank 0 writes the trace file */
int gph_run_control_file_ranked(const char *ctl_path, const char *secondary_ctl_path_or_null, int32_t device,
                                int32_t verbose, int32_t rank, int32_t world, gph_allreduce_fn allreduce, void *user);
/* ------------------------------------------------------------------------------------
 * The reference's proposal functions, ONE CALL EACH -- the drop-in boundary at the granularity performMCMC calls them
 * (upstream src/GPhoCS.h:84-100): a host program that keeps the reference's own performMCMC (trace writer, finetune
 * search, log lines) replaces the BODIES of those functions by these calls and mirrors the handful of process-wide
 * globals the reference keeps on its main thread through gph_chain_state.  oracle/integration_binding.c is that
 * replacement written out, linked with the reference's own objects and run (tests/test_boundary_run.py).
 *   reference function                                  call
 *   UpdateGB_InternalNode + _MigrationNode + _MigSPR    gph_mcmc_update_gb        (GPhoCS.c:2287, 2439, 2598; one fused launch)
 *   UpdateLocusRate        GPhoCS.c:4598                gph_mcmc_update_locus_rate
 *   UpdateTheta            GPhoCS.c:3037                gph_mcmc_update_theta
 *   UpdateMigRates         GPhoCS.c:3115                gph_mcmc_update_mig_rates
 *   UpdateTau              GPhoCS.c:3224                gph_mcmc_update_tau        (accepted[ancestral pop], as upstream)
 *   UpdateSampleAge        GPhoCS.c:4006                gph_mcmc_update_sample_age (accepted[current pop])
 *   mixing                 GPhoCS.c:4688                gph_mcmc_mixing
 *   synchronizeEvents loop GPhoCS.c:1705-1714           gph_mcmc_synchronize_events(refresh = 0)
 *   sampleMigRates' genLogLikelihood loop :1749-1757    gph_mcmc_synchronize_events(refresh = 1), after set_chain
 *   checkAll               patch.c:2745                 gph_mcmc_check_all
 * Conventions as upstream: a step size <= 0 makes the call return 0 accepted without drawing anything; errors are a
 * non-zero status (upstream prints "Fatal Error NNNN" and exits). */
#define GPH_ABI_MAXK 40     /* 2 * NSPECIES - 1 = 39 populations upstream (patch.h:19) */
#define GPH_ABI_MAXB 100    /* MAX_MIG_BANDS (patch.h:17) */
typedef struct {
  double theta[GPH_ABI_MAXK], popAge[GPH_ABI_MAXK], sampleAge[GPH_ABI_MAXK];   /* Population.{theta,age,sampleAge}, PopulationTree.h:60-101 */
  double migRate[GPH_ABI_MAXB], bandStart[GPH_ABI_MAXB], bandEnd[GPH_ABI_MAXB]; /* MigrationBand.{migRate,startTime,endTime} */
  uint32_t rng[3];                                       /* the general slot of RndCtx (utils.h:34): rndu_x, rndu_y, rndu_z */
  double logLikelihood, dataLogLikelihood, rateVar;      /* dataState, GPhoCS.h:35-50 */
  double coal_stats[GPH_ABI_MAXK], num_coals[GPH_ABI_MAXK], mig_stats[GPH_ABI_MAXB], num_migs[GPH_ABI_MAXB];   /* genetree_stats_total, patch.h:121 */
  int64_t rubberband_mig_conflicts;                      /* misc_stats, patch.h */
} gph_chain_state;
int gph_mcmc_get_chain(gph_mcmc *m, gph_chain_state *out);
int gph_mcmc_set_chain(gph_mcmc *m, const gph_chain_state *in);
int gph_mcmc_update_gb(gph_mcmc *m, int32_t iteration, double ftCoalTime, double ftMigTime, int64_t accepted[3], int64_t *total_mig_nodes);
int gph_mcmc_update_locus_rate(gph_mcmc *m, int32_t iteration, double finetune, int64_t *accepted);
int gph_mcmc_update_theta(gph_mcmc *m, int32_t iteration, double finetune, int64_t *accepted);
int gph_mcmc_update_mig_rates(gph_mcmc *m, int32_t iteration, double finetune, int64_t *accepted);
int gph_mcmc_update_tau(gph_mcmc *m, int32_t iteration, const double *finetunes, int32_t *accepted);
int gph_mcmc_update_sample_age(gph_mcmc *m, int32_t iteration, const double *finetunes, int32_t *accepted);
int gph_mcmc_mixing(gph_mcmc *m, int32_t iteration, double finetune, int64_t *accepted);
int gph_mcmc_synchronize_events(gph_mcmc *m, int32_t iteration, int32_t refresh);
int gph_mcmc_check_all(gph_mcmc *m, int32_t iteration, int32_t *ok);
/* initializeMCMC's per-locus loop (GPhoCS.c:1197-1214) for a caller that has sampled the population parameters itself
 * (samplePopParameters) and handed them over with gph_mcmc_set_chain: genealogies, event chains, statistics,
 * likelihoods; the chain state then holds dataLogLikelihood / logLikelihood as :1216-1224 leave them */
int gph_mcmc_initialize_genealogies(gph_mcmc *m);

/* the same with a native communicator (RCCL or shared memory): what `G-PhoCS-hip -g N <control-file>` runs in each of
 * its N child processes */
int gph_run_control_file_comm(const char *ctl_path, const char *secondary_ctl_path_or_null, int32_t device,
                              int32_t verbose, gph_comm *comm);

/* ------------------------------------------------------------------------------------
 * gph_run: any of the three above plus the outputs of the program, each switched on by its own field.  `size` is
 * sizeof(gph_run_options) AS THE CALLER COMPILED IT: a library that knows more fields reads the missing tail as 0 / NULL
 * (the smallest size accepted ends behind `comm`); a larger size than the library's own, or a NULL struct, is GPH_EARG.
 * A later output adds a field at the end, not a function.
 * Every output takes its sample wherever a trace line is written (never in the burn-in), into a device buffer of <rows>
 * rows; whenever that buffer is full, and at the end, rank r appends the rows to a binary part file PREFIX.<kind>.part<r>.
 * gph_run_finish(o, ranks, failed), called once after the last rank has returned, makes the files of the parts and removes
 * the parts (failed == 0: gph_ess_write, gph_clades_write, gph_gene_trees_write, gph_ancestry_write, gph_time_slices_write, gph_coal_stats_write, in this
 * order; everything is discarded at the first failure) or only discards, parts and files.  A one-rank run calls it itself.
 * Either way a run that did not finish leaves neither parts nor files, and a part that is missing, damaged or was not
 * closed by its rank is an error.  The outputs compose freely. */
typedef struct gph_run_options {
  uint32_t size;                   /* sizeof(gph_run_options) of the caller */
  const char *ctl, *ctl2;          /* control file; secondary control file or NULL */
  int32_t device, verbose;
  gph_comm *comm;                  /* NULL, or the communicator whose rank this process is (gph_run_control_file_comm) */
  int32_t rank, world;             /* without comm: 0, 0 or 0, 1 = one rank, else gph_run_control_file_ranked with ... */
  gph_allreduce_fn allreduce; void *user;   /* ... this exchange and its argument */
  /* `-l FILE`: the per-locus summary table, written once after the last iteration and only on success.  One rank writes
   * the file; of several, rank r writes FILE.part<r> with its own loci (rank 0's part holds the header) and the caller
   * concatenates the parts in rank order (gph_run_finish leaves them alone). */
  const char *locus_summary_path;
  /* `-s PREFIX`: the coalescent / sample-pair statistics (printCoalStats, GPhoCS.c:911-1040).  rows <= 0: 64, fewer when 64
   * rows of 7 + 3 * n(n-1)/2 * K doubles would exceed 256 MB.  Parts PREFIX.coal.part<r>, every raw row followed by logPrior.
   * gph_coal_stats_write adds the parts in rank order and writes PREFIX.coal.tsv and, per population,
   * PREFIX.<pop>.probCoal.tsv / .probFirstCoal.tsv / .meanCoal.tsv. */
  const char *coal_stats_prefix;
  int32_t coal_stats_rows;
  /* `--time-slices S` (needs coal_stats_prefix: GPH_EARG without one): a sample of gph_engine_time_slices_* wherever a
   * coal-stats sample is, into a device buffer of as many rows; parts PREFIX.slices.part<r>.  gph_time_slices_write adds them
   * in rank order, sample by sample, and writes PREFIX.slices.tsv -- header iter, numCoal_<pop>:<k> deltaT_<pop>:<k> (k = 1 .. S,
   * GPhoCS.c:933), numMig_<src>-><tgt>:<k> migT_<src>-><tgt>:<k>; rows "%7d" then "\t%9d\t%8f" per pair (GPhoCS.c:1005). */
  int32_t time_slices;
  /* `--ancestry PREFIX`: the migration ancestry (gph_engine_ancestry_*), rows <= 0: 64.  The part PREFIX.ancestry.part<r>
   * holds the rank's per-sample rows as they are flushed and, once the last iteration is done, its rows of the per-locus
   * table.  gph_ancestry_write writes, from the parts,
   *   PREFIX.loci.tsv     header locus name leaf sample samples pAny, then per band p_<src>-><tgt> age_<src>-><tgt>; one row
   *                       per (locus, leaf) with any.<i> > 0 (all-zero rows are omitted), in sequence-file order, then leaf
   *                       order; sample = the leaf's name as the header of PREFIX.<pop>.probCoal.tsv names it; pAny = any / S,
   *                       p = cnt / S, age = age_sum / cnt (0 where cnt = 0) in the genealogy's own units, all "%.10g"; the
   *                       ranks' rows concatenated in rank order
   *   PREFIX.samples.tsv  header iter, any_<sample>#<i> per leaf, <src>-><tgt>|<sample>#<i> per band and leaf; rows "%7d" then
   *                       "\t%9d" per count; the ranks' rows added sample by sample */
  const char *ancestry_prefix;
  int32_t ancestry_rows;
  /* `--gene-trees PREFIX [--gene-trees-loci SPEC] [--gene-trees-rows N]`: the sampled genealogies (gph_engine_gene_trees_*).
   * gene_trees_loci: NULL or "all", or a comma list of i, i-j (both ends included) or i-j:step, 0-based indices in
   * sequence-file order; an index named twice or >= the number of loci is refused, with a message that names it, before the
   * first iteration (GPH_EARG), and so is a population or sample name that holds white space or one of ()[],:;'=& ; a
   * selection or a row count without a prefix is GPH_EARG.  The row buffer holds min(gene_trees_rows or 64, 256 MB / bytes of a
   * row) rows; a single row above 256 MB stops the run before the first iteration (GPH_EFULL, with a message).  Parts
   * PREFIX.trees.part<r>.  gph_gene_trees_write writes, from the parts, PREFIX.trees.tsv:
   *   header  iter locus name dataLnL genLnL tmrca numMigs tree
   *   one line per (sample, selected locus), sample order then locus order (the ranks' records of one sample in rank order);
   *   iter, locus (0-based), numMigs "%d"; name from the sequence file; dataLnL, genLnL, tmrca = age[root] in the genealogy's
   *   own units "%.10g"; tree: gph_gene_tree_newick with leaf labels <sample>.<i>, <sample> as PREFIX.<pop>.probCoal.tsv
   *   names leaf i */
  const char *gene_trees_prefix, *gene_trees_loci;
  int32_t gene_trees_rows;
  /* `--clades PREFIX [--clades-loci SPEC] [--clades-slots P] [--clades-min-support F]`: the clade tables
   * (gph_engine_clades_*).  clades_loci as gene_trees_loci, with the same refusals (names included); clades_slots 0: the
   * default, else a power of two >= 2; clades_min_support: 0 = the default F = 0.5, a negative value = F = 0 (every kept
   * clade), else F in (0, 1]; a selection, a slot count or a threshold without a prefix, slots that are no power of two and a
   * threshold above 1 are GPH_EARG before anything is read.  The tables stay on the device during the run; rank r writes its
   * part PREFIX.clades.part<r> once, at the end.  gph_clades_write concatenates the parts in rank order into
   *   PREFIX.clades.tsv     header locus name samples dropped size support meanAge members; one row per (locus, kept clade)
   *                         with cnt / S >= F, in sequence-file order, then decreasing cnt, then increasing size, then the
   *                         key compared from word W - 1 down to word 0; support = cnt / S, meanAge = age / cnt in the
   *                         genealogy's own units, both "%.10g"; members: the comma list of the leaf labels <sample>.<i> in
   *                         leaf order, labels as PREFIX.trees.tsv prints them
   *   PREFIX.consensus.tsv  header locus name samples distinct dropped resolved tree; one row per selected locus;
   *                         distinct = nkeys, resolved and tree: gph_clades_consensus */
  const char *clades_prefix, *clades_loci;
  int32_t clades_slots;
  double clades_min_support;
  /* `--beta B`: the whole chain, burn-in and finetune search included, samples the power posterior
   * p(D | G)^B p(G | Theta) p(Theta) (gph_mcmc_set_beta); B = 0 is the prior.  Here 0 = not given = the posterior (B = 1), any
   * NEGATIVE value = B = 0, else B itself, in (0, 64] (GPH_EARG beyond).  The trace file and every other output keep their
   * formats; they describe the power posterior (the log-likelihood columns stay those of the plain likelihood), and the log on
   * stdout says so once.  Not together with marginal_prefix (GPH_EARG). */
  double beta;
  /* `--marginal-likelihood PREFIX [--ml-steps K] [--ml-burnin b] [--ml-samples s] [--ml-alpha a]`: the marginal likelihood
   * ln Z = ln p(D) by stepping-stone sampling and thermodynamic integration.  The run itself happens first, exactly as without
   * the option (its trace and every other output are the same bytes, and their parts are closed before anything below starts).
   * Then the chain goes on from where it ended, with the step sizes it ended with, down the ladder beta_k = (k / K)^(1 / a),
   * k = K, K - 1, .., 0: at each rung b iterations are discarded, then after each of s iterations the chain's total data
   * log-likelihood l (over all loci and ranks: gph_mcmc_get_state's dataLogLikelihood) is recorded.  With d_k = beta_{k+1} - beta_k:
   *   lnZ_ss = sum_{k<K} [ m + ln( (1/s) sum_j exp(d_k l_j(k) - m) ) ],  m = max_j d_k l_j(k)       (Xie et al. 2011)
   *   lnZ_ti = sum_{k<K} d_k (mean_k + mean_{k+1}) / 2                                              (trapezoid)
   * in fp64 on rank 0, which alone writes, once, at the end and only on success, PREFIX.marginal.tsv (tab-separated, numbers
   * "%.10g"): the header
   *   rung beta samples meanLnL sdLnL lnRatio accCoal accMig accSpr accTheta accMigRate accTau accMixing
   * one row per rung in the order visited (rung = k; sdLnL: the sample standard deviation; lnRatio: the rung's stepping-stone
   * term, 0 for k = K; acc*: accepted fractions over the rung's b + s iterations, accMig per migration node visited, accTau
   * over ancestral populations and estimated sample ages), then one line "# lnZ_ss <v> lnZ_ti <v> steps K alpha a".  The two
   * values also go into one line of the log on stdout, and every rung's acceptance into one line each.  A failed run leaves
   * no such file (gph_run_finish removes it).  Step sizes are not re-tuned per rung.
   * marginal_steps K: 0 = 32; marginal_samples s: 0 = 2000; marginal_alpha a: 0 = 0.3; negative values of these three are
   * GPH_EARG (what the program passes for `--ml-steps 0`, `--ml-samples 0`, `--ml-alpha 0`: usage errors).  marginal_burnin b:
   * 0 = the control file's burn-in if positive, else 1000; any negative value = no burn-in.  Any of the four without
   * marginal_prefix is GPH_EARG.  Every refusal comes with a message that names the option, before anything is read. */
  const char *marginal_prefix;
  int32_t marginal_steps, marginal_burnin, marginal_samples;
  double marginal_alpha;
  /* `--mc3 C [--mc3-heat h] [--mc3-swap-every k] [--mc3-report PREFIX]`: Metropolis-coupled chains (gph_mc3_* above), all on
   * this device.  mc3_chains C: 0 = off, 2 .. 16, anything else GPH_EARG.  Chain c has beta_c = 1 / (1 + h c) (mc3_heat h: 0 =
   * 0.1, negative GPH_EARG) and the seed random-seed + c; the swap generator gets random-seed + C.  Chain 0 is the control
   * file's chain: the trace, the log lines, the finetune search and every output above are its, exactly as without the option,
   * and because a swap exchanges states it stays the cold chain -- they describe the posterior.  The heated chains are further
   * engines loaded from the same host arrays (C times gph_engine_hbm_bytes of device memory; a chain that cannot be allocated
   * stops the run before the first iteration, with a message).  They are given every step size chain 0 is given (the search
   * reads chain 0's acceptance only).  A swap of two neighbours is attempted in front of every k-th iteration (mc3_swap_every
   * k: 0 = 1, negative = never).  The log on stdout states the ladder before the first iteration and attempts / accepted per
   * pair after the last.  With mc3_report_prefix, rank 0 writes PREFIX.mc3.tsv once, at the end and only on success
   * (gph_run_finish removes it after a failure; tab-separated, numbers "%.10g"): the header
   *   chain beta seed swapAttempts swapAccepted accCoal accMig accSpr accTheta accMigRate accTau accMixing meanLnL
   * one row a chain (the swap columns: pair (c, c + 1), 0 in the last row; acc*: as in PREFIX.marginal.tsv, over all
   * iterations; meanLnL: the chain's dataLogLikelihood over the iterations >= 0), then "# heat h every k attempted A accepted B".
   * GPH_EARG, with a message that names the option and before anything is read: mc3_heat, mc3_swap_every or mc3_report_prefix
   * without mc3_chains; mc3_chains with world > 1, a communicator or an all-reduce hook, with beta, or with marginal_prefix. */
  int32_t mc3_chains;
  double mc3_heat;
  int32_t mc3_swap_every;
  const char *mc3_report_prefix;
  /* `--replicates R --replicates-out PREFIX [--replicates-min-freq F] [--replicates-every k]`: R = 2 .. 16 INDEPENDENT chains on
   * this device, all at beta = 1, chain r seeded with random-seed + r, and the convergence diagnostics across them.  Chain 0 is
   * the control file's chain: its trace and every other output are the bytes of the run without the option.  The chains run
   * through gph_mc3 with every beta = 1 and no swaps (a host thread and a stream each); chain 0's step sizes and log period are
   * pushed to all of them, none is tuned by itself; they take R times the device memory, and a chain that cannot be allocated
   * stops the run before the first iteration with a message.  At every sample point (the rule of the summary table) chain
   * r >= 1 writes its trace line to PREFIX.chain<r>.trace (the trace file's header and formats; the files behave like the
   * trace file), every chain samples its clade tables when clades_prefix is given (chains r >= 1 with chain 0's selection and
   * slots), and the values every chain's trace line prints are kept on the host, before formatting: vals[i] * printFactors[i],
   * then Full-ld-ln, then Data-ld-ln.  After the last iteration, on success only (gph_run_finish removes both after a failure):
   *   PREFIX.psrf.tsv    header param mean sdWithin sdBetween psrf; one row per trace column in trace order, named as the
   *                      trace header names it, numbers "%.10g" (gph_psrf); last line "# chains R samples S maxPsrf v"
   *   PREFIX.asdsf.tsv   with clades_prefix only: header locus name samples asdsf maxSd compared distinct shared dropped; one
   *                      row per selected locus in sequence-file order (gph_engine_clades_compare with min_freq F; locus,
   *                      samples and the four counts "%d", the rest "%.10g"); last line
   *                      "# chains R minfreq F loci Q meanAsdsf v maxAsdsf v", the mean over the rows in file order
   * replicates_min_freq F: 0 = 0.1, negative = 0, else F in (0, 1].  replicates_every k >= 1 (0: off; clades_prefix only): after
   * every k-th sample and after the last, one line "Replicates: sample <S>: ASDSF mean <v> max <v> over <Q> loci" on stdout,
   * each at the cost of one kernel and one host synchronisation; the last line's values are the file's.  Conventionally an
   * ASDSF below 0.01 and a PSRF below 1.1 are read as agreement between the chains; nothing here guarantees either.
   * GPH_EARG, with a message that names the option and before anything is read: replicates outside 2 .. 16; no
   * replicates_prefix; any other replicates_* field without replicates; F above 1 or not finite; k < 0; replicates_every
   * without clades_prefix; replicates with world > 1, a communicator or an all-reduce hook, mc3_chains, beta or
   * marginal_prefix. */
  int32_t replicates;
  const char *replicates_prefix;
  double replicates_min_freq;
  int32_t replicates_every;
  /* `--ess PREFIX [--ess-loci SPEC]`: effective sample sizes, of every trace column and of every selected locus (gph_ess,
   * gph_engine_ess_* above).  A sample is taken wherever a trace line is written.  ess_loci as gene_trees_loci (an index named
   * twice or >= the number of loci is refused by name before the first iteration); ess_loci without ess_prefix is GPH_EARG
   * before anything is read.  The values every trace line prints are kept on the host before formatting (vals[i] *
   * printFactors[i], then the two log-likelihood columns) and the per-locus levels stay on the device during the run; rank r
   * writes its part PREFIX.ess.part<r> once, at the end.  gph_ess_write makes of the parts (numbers "%.10g")
   *   PREFIX.ess.tsv        (rank 0's) header param samples mean sd essBatch essAcf tauAcf truncated; one row per trace column
   *                         in trace order, named as the trace header names it (gph_ess with max_lag 0; fewer than two
   *                         samples: zeros); last line "# samples S level j batch b minEssAcf v (<param>)", the minimum over
   *                         the columns that were not constant ("-" and 0 when all were)
   *   PREFIX.locus-ess.tsv  header locus name samples essDataLnL essGenLnL essTmrca essNumMigs essTopo [essRate] topoChanges
   *                         minEss; one row per selected locus in sequence-file order, the ranks' rows concatenated in rank
   *                         order; ESS = gph_ess_read at the level with batch <= sqrt(samples); minEss over the series that
   *                         were not constant, 0 when all were; last line
   *                         "# loci Q level j batch b medianMinEss v minMinEss v (locus <i>)" (the median of an even number of
   *                         rows is the mean of the two in the middle; no row: 0 0 (locus -1))
   * and prints both summary lines as one line "ESS: ...; ..." on stdout.  With mc3_chains, replicates and marginal_prefix the
   * files describe chain 0 and the run proper, as the clade tables do; every other output is the same bytes with and without. */
  const char *ess_prefix, *ess_loci;
  /* `--predictive PREFIX [--predictive-loci SPEC] [--predictive-seed N] [--predictive-rows N]`: posterior predictive checks
   * (gph_engine_predictive_* above).  A sample is taken wherever a trace line is written.  predictive_loci as gene_trees_loci
   * (an index named twice or >= the number of loci is refused by name before the first iteration); predictive_seed: the seed as
   * decimal text (NULL: the control file's random-seed); predictive_rows: the rows of the device buffer (0: a default), fetched
   * when it is full and at the end.  Any of the three without predictive_prefix, a seed that is no unsigned number and negative
   * rows are GPH_EARG with a message, before anything is read.  Rank r writes its part PREFIX.predictive.part<r> once, at the end.
   * gph_predictive_write makes of the parts (numbers "%.10g")
   *   PREFIX.predictive.tsv         header locus name samples sites, then per statistic s obs_<s> mean_<s> sd_<s> p_<s>, then minP
   *                                 stat; one row per selected locus in sequence-file order (the ranks' rows concatenated); <s> =
   *                                 seg, diff_<P>|<Q> with the populations' names; mean = s1 / S, sd = sqrt(max((s2 - s1^2 / S) /
   *                                 (S - 1), 0)) (0 for S < 2), p = (gt + eq / 2) / S (upper-tail mid-p), minP = the smallest
   *                                 2 min(p, 1 - p) over the statistics, stat its name (the first of equal ones); last line
   *                                 "# loci Q samples S seed N minMinP v (locus <i>)" (no row: 0 (locus -1))
   *   PREFIX.predictive-genome.tsv  header iter and the statistics' names; one row per sample, "%7d" and "\t%llu" per statistic:
   *                                 the totals over the selected loci (the ranks' rows added); then "# observed", "# mean",
   *                                 "# p" (the same mid-p, over the samples), each with one tab-separated value per statistic, and
   *                                 "# loci Q samples S seed N"
   * and prints "Predictive: " and the "# p" line without its "# " on stdout.  Both files are written once, on success only; a
   * failed run leaves neither parts nor files.  With mc3_chains, replicates and marginal_prefix they describe chain 0 and the run
   * proper; every other output is the same bytes with and without. */
  const char *predictive_prefix, *predictive_loci, *predictive_seed;
  int32_t predictive_rows;
  /* `--triplets PREFIX [--triplets-pops "A,B,C;D,E,F"] [--triplets-loci SPEC] [--triplets-rows N]`: triplet topology weights
   * (gph_engine_triplets_* above).  A sample is taken wherever a trace line is written.  triplets_pops: the triples as names of
   * current populations of the control file, three a triple, triples separated by ';' (NULL: all triples); triplets_loci as
   * gene_trees_loci; triplets_rows: the rows of the device buffer (0: a default), fetched when it is full and at the end.  Any of
   * the three without triplets_prefix and negative rows are GPH_EARG with a message, before anything is read; an unknown or
   * repeated name, a triple named twice and a model with fewer than three current populations are GPH_EARG with a message that
   * names the option, once the control file is read and before the sequence file is.  Rank r writes its part
   * PREFIX.triplets.part<r> once, at the end.  gph_triplets_write makes of the parts (numbers "%.10g")
   *   PREFIX.triplets.tsv         header locus name samples P Q R w_PQ|R w_PR|Q w_QR|P age_PQ|R age_PR|Q age_QR|P top; one row per
   *                               (selected locus, triple) in sequence-file order, then triple order (the ranks' rows
   *                               concatenated); P Q R the populations' names; w = W / (S n_P n_Q n_R); age = A / W (0 where
   *                               W = 0) in the genealogy's own units; top = the label "<X>,<Y>|<Z>" of the slot with the largest
   *                               W (ties: the lowest t)
   *   PREFIX.triplets-genome.tsv  header iter, then per triple the labels "<X>,<Y>|<Z>" of its three slots (names); one row per
   *                               sample, "%7d" and "\t%llu" per slot: the totals over the selected loci (the ranks' rows
   *                               added); then per triple
   *                                   # asym <P>,<Q>,<R> major <label> minorA <label> minorB <label> wMajor <v> D <mean> sd <v> pPos <v>
   *                               major = the slot with the largest total over all samples (ties: the lowest t), the minors the
   *                               other two in slot order with totals a and b per sample; wMajor = the major's share of the
   *                               triple's total over all samples; D_s = (a - b) / (a + b) (0 when a + b = 0); D and sd the mean
   *                               and the sample sd (divisor S - 1; 0 for S = 1) over the samples in sample order; pPos the
   *                               fraction of samples with D_s > 0; and a last line "# loci Q samples S triples T"
   * and prints "Triplets: " and the "# asym" values of the triple with the largest |D| (the first of equal ones) on stdout.  Both
   * files are written once, on success only; a failed run leaves neither parts nor files.  With mc3_chains, replicates and
   * marginal_prefix they describe chain 0 and the run proper; every other output is the same bytes with and without. */
  const char *triplets_prefix, *triplets_pops, *triplets_loci;
  int32_t triplets_rows;
  /* `--mutations PREFIX [--mutations-loci SPEC] [--mutations-rows N]`: expected substitutions per population branch and per
   * sample (gph_engine_mutations_* above).  A sample is taken wherever a trace line is written.  mutations_loci as
   * gene_trees_loci; mutations_rows: the rows of the device buffer (0: a default), fetched when it is full and at the end.  Either
   * without mutations_prefix and negative rows are GPH_EARG with a message, before anything is read.  Rank r writes its part
   * PREFIX.mutations.part<r> once, at the end; the part carries the per-sample rows as the doubles' 64-bit patterns, so the ranks' doubles add
   * without loss.  gph_mutations_write makes of the parts (numbers "%.10g")
   *   PREFIX.mutations.tsv         header locus name samples sites, then per population mut_<pop> exp_<pop>, then rel; one row per
   *                                selected locus in sequence-file order (the ranks' rows concatenated); mut and exp are the means
   *                                over the samples (accumulator / S), rel = (sum_p mut accumulators) / (sum_p exp accumulators),
   *                                both sums in population order (0 where the second is 0)
   *   PREFIX.mutations-genome.tsv  header iter, mut_<pop> and exp_<pop> of every population, mutExt_<sample>.<i> and
   *                                expExt_<sample>.<i> of every leaf; one row per sample, "%7d" and "\t%.10g" per column: the
   *                                sums over the selected loci (the ranks' rows added in rank order); then
   *                                    # rel <pop> mean <v> sd <v> pHigh <v>            per population
   *                                    # ext <sample>.<i> mean <v> sd <v> pHigh <v>     per leaf
   *                                with, per sample, the ratio mut / exp of the row's values as printed (0 where exp is 0), mean
   *                                and the sample sd (divisor S - 1; 0 for S = 1) over the samples in sample order, pHigh the
   *                                share of samples with a ratio above 1; and a last line "# loci Q samples S"
   * and prints "Mutations: " and the "# rel" values of the population with the largest |ln mean| (the first of equal ones) on
   * stdout.  Both files are written once, on success only; a failed run leaves neither parts nor files.  With mc3_chains,
   * replicates and marginal_prefix they describe chain 0 and the run proper; every other output is the same bytes with and
   * without. */
  const char *mutations_prefix, *mutations_loci;
  int32_t mutations_rows;
  /* `--simulate PREFIX [--simulate-loci SPEC] [--simulate-seed N] [--simulate-rows N] [--simulate-no-sites]`: replicate genealogies
   * simulated from the sampled parameters (gph_engine_simulate_* above).  A sample is taken wherever a trace line is written.
   * simulate_loci as gene_trees_loci; simulate_seed: an unsigned decimal number (NULL: the control file's random-seed);
   * simulate_rows: the rows of the device buffer (0: a default); simulate_no_sites != 0: the genealogy level alone.  Any of them
   * without simulate_prefix, a seed that is no number and negative rows are GPH_EARG with a message, before anything is read.
   * Rank r writes its part PREFIX.simulate.part<r> once, at the end; gph_simulate_write makes of the parts (numbers "%.10g")
   *   PREFIX.simulate.tsv         header locus name samples failed sites; per genealogy statistic -- tmrca, length, genLnL,
   *                               coal_<pop>, mig_<src>-><tgt> -- s_<stat> mean_<stat> sd_<stat> p_<stat>: the sampled genealogies'
   *                               mean sx / V, the replicates' mean sy / V and sd sqrt((sy2 - sy sy / V) / (V - 1)) (0 for V < 2
   *                               or a negative radicand), the mid-p (gt + eq / 2) / V, V = samples - failed (all 0 for V = 0);
   *                               with sites per site statistic obs_ mean_ sd_ p_ as PREFIX.predictive.tsv prints them, over V;
   *                               then minP = the smallest 2 min(p, 1 - p) and the statistic that has it (the first of equal
   *                               ones).  One row per selected locus, ranks in rank order; a last line
   *                               "# loci Q samples S seed N failed F minMinP v (locus g)"
   *   PREFIX.simulate-genome.tsv  header iter and the columns of a row (gph_engine_simulate_column_name, which 1, with the
   *                               populations' and bands' names); one row per sample, the ranks' rows added; then
   *                                   # observed   "-" per genealogy column, the data's total per site column
   *                                   # mean       the column's mean over the samples
   *                                   # p          "-" for s.* and failed; r.coal_* / r.mig_*: the mid-p of the replicates'
   *                                                total against the sampled total of the same sample; gt.*: sum gt / sum (Q -
   *                                                failed) over the samples; site columns: the mid-p against the observed total
   *                               and a last line "# loci Q samples S seed N"
   * and prints "Simulate: " and the p line on stdout.  Both files are written once, on success only; a failed run leaves
   * neither parts nor files.  With mc3_chains, replicates and marginal_prefix they describe chain 0 and the run proper, with
   * beta that chain.  Not built: a file of the replicate trees (gph_engine_simulate_fetch_records hands them out), replicates
   * per heated or replicate chain, models other than the run's own. */
  const char *simulate_prefix, *simulate_loci, *simulate_seed;
  int32_t simulate_rows, simulate_no_sites;
  /* `--pair-times PREFIX [--pair-times-pops "A,B;A,A"] [--pair-times-grid LO,HI,B] [--pair-times-loci SPEC] [--pair-times-rows N]`:
   * pairwise coalescence-time distributions (gph_engine_pair_times_* above).  A sample is taken wherever a trace line is written.
   * pair_times_pops: the pairs as names of current populations of the control file, two a pair, pairs separated by ';' (NULL: all
   * pairs with a leaf pair); pair_times_grid "LO,HI,B": B bins with E = B - 1 edges e_k = LO (HI / LO)^(k / (E - 1)), computed on
   * the host as LO * pow(HI / LO, (double)k / (double)(E - 1)), e_0 = LO and e_{E-1} = HI exactly (NULL: "1e-6,1e-2,34");
   * pair_times_loci as gene_trees_loci; pair_times_rows: the rows of the device buffer (0: a default).  Any of the four without
   * pair_times_prefix and negative rows are GPH_EARG with a message, before anything is read; LO <= 0, HI <= LO, B outside 3 .. 128,
   * an unknown population name, a pair named twice and a pair without a leaf pair are GPH_EARG with a message that names the
   * option, once the control file is read and before the sequence file is.  Rank r writes its part PREFIX.pair-times.part<r>
   * once, at the end; its H line carries every edge as used as its 64-bit pattern.  gph_pair_times_write makes of the parts
   * (numbers "%.10g")
   *   PREFIX.pair-times.tsv         header locus name samples P Q pairs meanAge minAge pBelow fBelow; one row per (selected locus,
   *                                 pair) in sequence-file order, then slot order (the ranks' rows concatenated); P Q the
   *                                 populations' names, pairs = m_PQ, meanAge = A / (S m), minAge = M / S, pBelow = X / S,
   *                                 fBelow = Y / (S m); a last line "# loci Q samples S pairs NP bins B"
   *   PREFIX.pair-times-genome.tsv  header iter, then "<P>|<Q>:<k>" per slot and bin, then "below_<P>|<Q>" per slot, then
   *                                 "loci_<P>|<Q>" per slot (names); one row of integers per sample, "%7d" and "\t%llu" (the
   *                                 ranks' rows added); then "# edges" and the E edges as "%.17g"; then per slot, with
   *                                 F_s[k] = sum_{j <= k} hist_s[j] / (Q m) the sample's cumulative share (integer partial sums, one
   *                                 division) and b_s = below_s / (Q m):
   *                                     # cdf <P>|<Q> v_0 ... v_{B-1}        the means of F_s[k] over the samples
   *                                     # sd <P>|<Q> v_0 ... v_{B-1}         their sample sd (divisor S - 1; 0 for S = 1)
   *                                     # below <P>|<Q> mean <v> sd <v> loci <v>     mean and sd of b_s, mean of loci_s / Q
   *                                 sums in sample order from 0.0, mean = sum / S, sd = sqrt(sum (v - mean)^2 / (S - 1))
   * and prints "PairTimes: " and the "# below" values of the P < Q pair with the largest mean b (the first of equal ones; "none"
   * without a P < Q pair) on stdout.  Both files are written once, on success only; a failed run leaves neither parts nor files.
   * With mc3_chains, replicates and marginal_prefix they describe chain 0 and the run proper; every other output is the same bytes
   * with and without.  Not built: coalescence rates / hazard estimates and a relative cross-coalescence ratio, per-locus
   * histograms, pairs of ancestral populations, the output per heated or replicate chain, a control-file keyword. */
  const char *pair_times_prefix, *pair_times_pops, *pair_times_grid, *pair_times_loci;
  int32_t pair_times_rows;
  /* `--sfs PREFIX [--sfs-pairs "A,B;C,D"|none] [--sfs-loci SPEC] [--sfs-rows N]`: site-frequency spectra, data against sampled
   * genealogies (gph_engine_sfs_* above).  A sample is taken wherever a trace line is written.  sfs_pairs: the pairs as names of
   * current populations of the control file, two a pair, pairs separated by ';', in any order; "none": no pair (NULL: all pairs);
   * sfs_loci as gene_trees_loci; sfs_rows: the rows of the device buffer (0: a default).  Any of the three without sfs_prefix and
   * negative rows are GPH_EARG with a message, before anything is read; an unknown population name, a pair that names one
   * population twice, a pair named twice, and a model in which no population has two samples and no pair is taken are GPH_EARG
   * with a message that names the option, once the control file is read and before the sequence file is.  Rank r writes its part
   * PREFIX.sfs.part<r> once, at the end.  gph_sfs_write makes of the parts (numbers "%.10g"; S the samples)
   *   PREFIX.sfs.tsv         header locus name samples sites, then use_<g> per group, then obs_<slot> exp_<slot> per slot with
   *                          exp = (double)use E / S (0 for S = 0), then rel = sum obs / sum exp over the SPECTRUM slots (sums
   *                          in slot order from 0.0; 0 where the denominator is 0); one row per selected locus in sequence-file
   *                          order (the ranks' rows concatenated); names: "sfs_<p>:<k>", "privP_<P>|<Q>", "privQ_", "shared_",
   *                          "fixed_" and "<p>", "<P>|<Q>" with the populations' names; a last line "# loci Q samples S slots NS"
   *   PREFIX.sfs-genome.tsv  header iter and the slot names; one row of expected counts per sample, "%7d" and "\t%.10g" (the
   *                          ranks' rows added in rank order from their doubles' 64-bit patterns); then, per slot and over the
   *                          samples' rows as added,
   *                              # observed   the data's totals (integers, the ranks' added)
   *                              # mean       sum / S, the sum in sample order from 0.0
   *                              # sd         sqrt(sum (v - mean)^2 / (S - 1)), 0 for S = 1
   *                              # ratio      observed / mean, 0 where mean is 0
   *                              # z          (observed - mean) / sqrt(mean + sd^2), 0 where the denominator is 0
   *                          then "# loci Q samples S"
   * and prints "SFS: <slot> observed <v> mean <v> ratio <v> z <v>" for the slot with the largest |z| (the first of equal ones)
   * on stdout.  Both files are written once, on success only; a failed run leaves neither parts nor files.  With mc3_chains,
   * replicates and marginal_prefix they describe chain 0 and the run proper; every other output is the same bytes with and
   * without.  Not built: a replicate-based (exact, p-valued) spectrum check through k_predictive's generator, unfolded spectra,
   * the output per heated or replicate chain, a control-file keyword. */
  const char *sfs_prefix, *sfs_pairs, *sfs_loci;
  int32_t sfs_rows;
} gph_run_options;
int gph_run(const gph_run_options *o);
int gph_run_finish(const gph_run_options *o, int32_t ranks, int32_t failed);
/* what gph_run_finish calls, one output at a time: _write makes the files of the parts of `ranks` ranks and removes the
 * parts; _discard removes the parts and the output's files should they exist; _combined hands out the records _write would
 * print: *rows samples of *row_doubles doubles (the ranks' raw rows added in rank order; coal stats: then logPrior) into
 * out[max_rows >= *rows]; out NULL: the two counts only. */
int gph_coal_stats_write(const char *prefix, int32_t ranks);
int gph_coal_stats_combined(const char *prefix, int32_t ranks, double *out, int64_t max_rows, int64_t *rows, int32_t *row_doubles);
int gph_coal_stats_discard(const char *prefix, int32_t ranks);
int gph_time_slices_write(const char *prefix, int32_t ranks);
int gph_time_slices_combined(const char *prefix, int32_t ranks, double *out, int64_t max_rows, int64_t *rows, int32_t *row_doubles);
int gph_time_slices_discard(const char *prefix, int32_t ranks);
int gph_ancestry_write(const char *prefix, int32_t ranks);
int gph_ancestry_discard(const char *prefix, int32_t ranks);
int gph_gene_trees_write(const char *prefix, int32_t ranks);
int gph_gene_trees_discard(const char *prefix, int32_t ranks);
int gph_clades_write(const char *prefix, int32_t ranks);
int gph_clades_discard(const char *prefix, int32_t ranks);
int gph_ess_write(const char *prefix, int32_t ranks);
int gph_ess_discard(const char *prefix, int32_t ranks);
int gph_predictive_write(const char *prefix, int32_t ranks);
int gph_predictive_discard(const char *prefix, int32_t ranks);
int gph_triplets_write(const char *prefix, int32_t ranks);
int gph_triplets_discard(const char *prefix, int32_t ranks);
int gph_mutations_write(const char *prefix, int32_t ranks);
int gph_mutations_discard(const char *prefix, int32_t ranks);
int gph_simulate_write(const char *prefix, int32_t ranks);
int gph_simulate_discard(const char *prefix, int32_t ranks);
int gph_pair_times_write(const char *prefix, int32_t ranks);
int gph_pair_times_discard(const char *prefix, int32_t ranks);
int gph_sfs_write(const char *prefix, int32_t ranks);
int gph_sfs_discard(const char *prefix, int32_t ranks);
/* records of gph_engine_gene_trees_fetch as plain arrays (host only; any output pointer may be NULL).  Record r of `count`,
 * record_bytes apart, with the offsets and N of _shape: age[r][N] (copied, the bit patterns intact), father / left / right /
 * npop[r][N], root / num_migs[r] (num_migs clamped to 0 .. GPH_GT_MAX_MIGS), dataLnL / genLnL[r], and per live migration
 * k < num_migs in `living` order mig_branch / mig_band / mig_spop / mig_tpop / mig_age[r][GPH_GT_MAX_MIGS]; entries
 * k >= num_migs (and those of a damaged `living` word) are -1 and age 0. */
int gph_gene_trees_decode(const void *records, int64_t count, int32_t record_bytes, const int32_t *offsets, int32_t nodes,
                          double *age, int32_t *father, int32_t *left, int32_t *right, int32_t *npop, int32_t *root, int32_t *num_migs,
                          double *dataLnL, double *genLnL, int32_t *mig_branch, int32_t *mig_band, int32_t *mig_spop, int32_t *mig_tpop,
                          double *mig_age);
/* one genealogy as one line of extended Newick (host only: no GPU, no engine).  n leaves, N = 2n - 1 nodes, arrays as
 * gph_gene_trees_decode fills them; pop_names[K], band_names[B] ("<src>-><tgt>"), leaf_labels[n].
 *   tree    := sub(root) ";"
 *   body(v) := label(v) "[&pop=" POP(npop[v]) "]"                                 v a leaf
 *            | "(" sub(left[v]) "," sub(right[v]) ")" "[&pop=" POP(npop[v]) "]"   v internal
 * For v != root let m_1 .. m_k be the live migrations on the branch of v sorted by age ascending (equal ages keep `living`
 * order), a_0 = age[v], a_j = the age of m_j: s_0 = body(v), s_j = "(" s_{j-1} ":" LEN(a_j - a_{j-1}) ")" "[&mig=" BAND "]",
 * sub(v) = s_k ":" LEN(age[father[v]] - a_k); sub(root) = body(root).  LEN is "%.10g" of the fp64 difference.
 * Returns 0 with the text in out (NUL-terminated, *out_len = its length; out NULL: the length only), 2 when out_cap is too
 * small, GPH_EARG for a record that is no tree (an index out of range, a cycle) or a name that holds white space or one of
 * ()[],:;'=& (with a message). */
int gph_gene_tree_newick(int32_t n, const double *age, const int32_t *father, const int32_t *left, const int32_t *right,
                         const int32_t *npop, int32_t root, int32_t num_migs, const int32_t *mig_branch, const int32_t *mig_band,
                         const double *mig_age, const char *const *pop_names, int32_t K, const char *const *band_names, int32_t B,
                         const char *const *leaf_labels, char *out, size_t out_cap, size_t *out_len);
/* the majority-rule consensus of one locus's clade table as one line of Newick without branch lengths (host only).
 * entries[slots][W + 2] as gph_engine_clades_fetch hands them out (W = ceil(n / 64)), `samples` the samples they were
 * accumulated over, leaf_labels[n].  The consensus holds the kept clades with 2 cnt > samples: pairwise nested or disjoint by
 * construction; a set that is not, or an entry that is no clade of n leaves (fewer than two leaves, a bit beyond leaf n - 1), is
 * refused with GPH_EARG and a message -- never a wrong tree.  *resolved = their number, the root's clade included.
 *   tree    := node(all leaves) ";"
 *   node(c) := "(" child "," child ... ")" "[&support=" cnt / samples ",age=" age / cnt "]"      both "%.10g"
 *   child   := node(c') for the largest clades c' inside c | the label of a leaf of c that lies in none of them
 * children in the order of their smallest leaf index.  Mean ages of nested clades are conditional on different sample sets and
 * need not nest: no branch lengths.  A table that does not hold the clade of all leaves (a full table dropped it) gives the top
 * level without annotation; one leaf gives its label.  Returns as gph_gene_tree_newick does, label rules included. */
int gph_clades_consensus(int32_t n, int32_t slots, const uint64_t *entries, int64_t samples, const char *const *leaf_labels,
                         char *out, size_t out_cap, size_t *out_len, int32_t *resolved);

/* ------------------------------------------------------------------------------------
 * post-run summary of a trace file (host only): block means per column, the output of the reference's
 * stand-alone `readTrace` tool (src/readTrace.c:41-291: `-b` block size, default the whole file = -1;
 * `-d` samples to discard).  The text that tool prints goes to out (NUL-terminated, *out_len = its
 * length; out may be NULL to ask for the length), its error text to err.  Returns 0, the tool's exit
 * code on error, or 2 when out_cap was too small. */
int gph_read_trace(const char *trace_file, int block_size, int discard, char *out, size_t out_cap, size_t *out_len,
                   char *err, size_t err_cap);
/* `readTrace <trace-file> --ess [-d N]`: the table of PREFIX.ess.tsv (gph_run_options: ess_prefix) for any trace file -- the
 * reference's own, a chain<r>.trace -- its summary line included: the first column is dropped, the first N samples are
 * discarded, the values are parsed as doubles and every column goes through gph_ess with max_lag 0.  Buffers and status as
 * gph_read_trace. */
int gph_read_trace_ess(const char *trace_file, int discard, char *out, size_t out_cap, size_t *out_len, char *err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif
