// gph_main.cpp -- G-PhoCS-hip: the reference's command line (GPhoCS.c:84-238)
//   G-PhoCS-hip [-v] [-d device] [-g gpus] [-l locus-summary-file] [-s coal-stats-prefix [--coal-stats-rows N] [--time-slices S]] [--ancestry ancestry-prefix] [--gene-trees trees-prefix [--gene-trees-loci SPEC] [--gene-trees-rows N]] [--clades clades-prefix [--clades-loci SPEC] [--clades-slots P] [--clades-min-support F]] [--ess ess-prefix [--ess-loci SPEC]] [--predictive pp-prefix [--predictive-loci SPEC] [--predictive-seed N] [--predictive-rows N]] [--triplets tw-prefix [--triplets-pops "A,B,C;D,E,F"] [--triplets-loci SPEC] [--triplets-rows N]] [--mutations mutations-prefix [--mutations-loci SPEC] [--mutations-rows N]] [--simulate sim-prefix [--simulate-loci SPEC] [--simulate-seed N] [--simulate-rows N] [--simulate-no-sites]] [--beta B] [--marginal-likelihood ml-prefix [--ml-steps K] [--ml-burnin b] [--ml-samples s] [--ml-alpha a]] [--mc3 C [--mc3-heat h] [--mc3-swap-every k] [--mc3-report mc3-prefix]] [--replicates R --replicates-out rep-prefix [--replicates-min-freq F] [--replicates-every k]] <control-file> [secondary-control-file]
// over libgphocs_hip.  The library comes in capacity variants (tighter LDS image = more
// wavefronts per CU); the control file is read once with the default build to learn the model
// dimensions, then the tightest variant that fits runs the chain.
//
// -g N: ONE chain over N GPUs (the analogue of the reference's `-n threads`, GPhoCS.c:95, 116-145: a static split
// of the loci, MultiCoreUtils.h:8).  The launcher forks N children BEFORE anything touches a GPU; child r loads the
// library, takes device r, holds the r-th contiguous block of loci and runs the same chain; the reduced vectors of
// the per-locus loops travel by RCCL all-gather on each child's stream (the id of the communicator goes from child
// 0 to the others through a shared page).  With fewer devices than ranks (tests on a 1-GPU box) the ranks share
// devices and exchange through that shared page instead -- RCCL refuses two ranks on one GPU.
//
// The outputs (gph_run_options in include/gphocs_hip.h says what each writes): -l FILE, the per-locus posterior summary
// table; -s PREFIX, the coalescent / sample-pair statistics of every sample (--coal-stats-rows N: rows of the device buffer
// between two flushes, default 64), with --time-slices S additionally per time slice; --ancestry PREFIX, which sample's
// lineage went through which migration band at which locus; --gene-trees PREFIX, the sampled genealogy of every selected
// locus at every sample as a line of extended Newick (--gene-trees-loci SPEC: a comma list of i, i-j or i-j:step, 0-based in
// sequence-file order, default all; --gene-trees-rows N: rows of the device buffer, default 64, fewer when a row is large);
// --clades PREFIX, per selected locus the clades its sampled genealogies support, with posterior probability and mean age,
// and its majority-rule consensus tree, from tables accumulated on the device (--clades-loci SPEC as --gene-trees-loci;
// --clades-slots P: slots of a locus's table, a power of two, default the smallest one >= 8 (leaves - 1); --clades-min-support
// F: the clades listed have support >= F, default 0.5, 0 lists every kept clade).
// --ess PREFIX writes the effective sample size of every trace column to PREFIX.ess.tsv (batch means and Geyer's initial
// positive sequence) and, per selected locus (--ess-loci SPEC as --gene-trees-loci, default all), the effective sample sizes
// of its log-likelihoods, TMRCA, migration count and topology (the distance to the first sampled tree) with the number of
// topology changes to PREFIX.locus-ess.tsv, from batch sums kept on the device.
// --predictive PREFIX writes posterior predictive checks: per selected locus (--predictive-loci SPEC as --gene-trees-loci, default
// all) the observed value, the replicates' mean and sd and the mid-p of every discrepancy statistic to PREFIX.predictive.tsv, and
// the genome-wide totals per sample to PREFIX.predictive-genome.tsv; one replicate alignment per sample and locus is simulated
// on the device (--predictive-seed N, default the control file's random-seed; --predictive-rows N: rows of the device buffer).
// --triplets PREFIX writes triplet topology weights (Twisst): per selected locus (--triplets-loci SPEC as --gene-trees-loci,
// default all) and triple of current populations (--triplets-pops "A,B,C;D,E,F", default all triples) the share of each of the
// three topologies and the mean age of the sister coalescence to PREFIX.triplets.tsv, and the genome-wide totals per sample with
// the asymmetry of the two minority topologies to PREFIX.triplets-genome.tsv (--triplets-rows N: rows of the device buffer).
// --mutations PREFIX writes the posterior expected number of substitutions inside each population and on each sample's terminal
// branch next to what the clock expects on the same exposure: per selected locus (--mutations-loci SPEC, default all) to
// PREFIX.mutations.tsv, genome-wide per sample with the ratios' summary to PREFIX.mutations-genome.tsv (--mutations-rows N).
// --simulate PREFIX confronts the demographic model itself: per sample and selected locus (--simulate-loci SPEC, default all) one
// replicate genealogy is simulated on the device from the sampled parameters (the structured coalescent with migration), and,
// unless --simulate-no-sites, a replicate alignment on it; the sampled genealogies' statistics against the replicates' and the
// data's against the replicate alignments' go to PREFIX.simulate.tsv, the genome-wide totals per sample to
// PREFIX.simulate-genome.tsv (--simulate-seed N, default the control file's random-seed; --simulate-rows N).
// --pair-times PREFIX writes the distribution of the coalescence time between the lineages of two current populations on an
// absolute time axis: per selected locus (--pair-times-loci SPEC, default all) and pair (--pair-times-pops "A,B;A,A", default all
// pairs) the mean and the youngest age and how often a coalescence lies below the populations' split to PREFIX.pair-times.tsv, and
// per sample the genome-wide histograms over the grid (--pair-times-grid LO,HI,B, default 1e-6,1e-2,34: B bins, geometric edges)
// with their cumulative curves to PREFIX.pair-times-genome.tsv (--pair-times-rows N: rows of the device buffer).
// --sfs PREFIX writes the site-frequency spectrum of every current population and, per pair of populations (--sfs-pairs "A,B;C,D",
// default all pairs, `none`: none), the private, shared and fixed variable sites, as the data show them next to what the sampled
// genealogies expect: per selected locus (--sfs-loci SPEC, default all) to PREFIX.sfs.tsv, genome-wide per sample with the observed
// totals, ratios and z scores to PREFIX.sfs-genome.tsv (--sfs-rows N: rows of the device buffer).
// --beta B runs the whole chain on the power posterior p(D|G)^B p(G|Theta) p(Theta), B in [0, 64], 0 = the prior;
// --marginal-likelihood PREFIX runs, behind the unchanged run, the ladder beta_k = (k/K)^(1/a) from 1 down to 0 (--ml-steps K,
// default 32; --ml-alpha a, default 0.3; per rung --ml-burnin b discarded iterations, default the control file's burn-in or
// 1000, and --ml-samples s recorded ones, default 2000) and writes the stepping-stone and thermodynamic-integration estimates
// of the log marginal likelihood to PREFIX.marginal.tsv (rank 0 alone: no parts).  The two exclude each other.
// --mc3 C runs C = 2 .. 16 Metropolis-coupled chains on the one GPU: chain c on the power posterior with beta_c = 1 / (1 + h c)
// (--mc3-heat h, default 0.1) and the seed random-seed + c; in front of every k-th iteration (--mc3-swap-every k, default 1,
// negative: never) two neighbouring chains are proposed to exchange their states.  Chain 0 is the control file's chain and stays
// the cold one, so the trace and every output above describe the posterior as before; --mc3-report PREFIX writes the ladder,
// the swap counts and every chain's acceptance to PREFIX.mc3.tsv.  Not with -g N > 1, --beta or --marginal-likelihood.
// --replicates R --replicates-out PREFIX runs R = 2 .. 16 independent chains on the one GPU (chain r seeded with random-seed + r,
// chain 0 the control file's own, its outputs unchanged) and writes the convergence diagnostics across them: the potential
// scale reduction factor of every trace column to PREFIX.psrf.tsv, with --clades the per-locus average standard deviation of
// split frequencies to PREFIX.asdsf.tsv (over the clades some chain holds with frequency >= F, --replicates-min-freq F, default
// 0.1), the other chains' traces to PREFIX.chain<r>.trace; --replicates-every k prints the ASDSF after every k-th sample.  Not
// with -g N > 1, --mc3, --beta or --marginal-likelihood.
// They compose freely.  Under -g N every child leaves parts: of the summary table FILE.part<r>, which the launcher
// concatenates in rank order into FILE once every child has exited 0; of the others the library's own, which gph_run_finish
// turns into the files (the launcher itself has not touched a GPU).  A run that did not finish leaves neither parts nor files.
#include "gphocs_hip.h"
#include <dlfcn.h>
#include <libgen.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <cerrno>
#include <unistd.h>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct Variant { const char *file; int leaves, pops, bands; };
static const Variant VARIANTS[] = {{"libgphocs_hip_s.so", 16, 9, 4}, {"libgphocs_hip_l.so", 20, 13, 4}, {"libgphocs_hip.so", 24, 16, 8},
                                   {"libgphocs_hip_x.so", 32, 32, 16}, {"libgphocs_hip_g.so", 48, 16, 8}, {"libgphocs_hip_h.so", 64, 40, 16},
                                   {"libgphocs_hip_b.so", 64, 40, 100}, {"libgphocs_hip_n.so", 200, 40, 100}};
/* the library whose gph_control_read reads the control file BEFORE the capacity variant is chosen: the control parser has
 * no compile-time capacities (it keeps the reference's own caps, patch.h:17-22, in every build), so any variant can read
 * any control file; the dimensions it returns then select the tightest variant above */
static const int DEFAULT_VARIANT = 5;

template <class F> static F sym(void *h, const char *name)
{
  void *p = dlsym(h, name);
  if (!p) { fprintf(stderr, "G-PhoCS-hip: %s is missing from the engine library\n", name); exit(2); }
  return (F)p;
}

struct Mailbox {                       // first bytes of the page the ranks share
  std::atomic<int> id_ready, ndev;
  char id[GPH_COMM_ID_BYTES];
};

static void *load_engine(const std::string &dir, const char *ctl, const char *ctl2)
{
  const char *forced = getenv("GPHOCS_HIP_LIB");
  std::string path = forced ? forced : dir + "/" + VARIANTS[DEFAULT_VARIANT].file;
  void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!h && !forced) { path = dir + "/" + VARIANTS[2].file; h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL); }
  if (!h) { fprintf(stderr, "G-PhoCS-hip: cannot load %s: %s\n", path.c_str(), dlerror()); exit(2); }
  if (forced) return h;
  gph_control *c = nullptr;
  gph_config cfg;
  if (sym<decltype(&gph_control_read)>(h, "gph_control_read")(ctl, ctl2, &c)) exit(1);
  sym<decltype(&gph_control_get)>(h, "gph_control_get")(c, &cfg, nullptr, nullptr);
  const int n = cfg.n, K = cfg.K, B = cfg.B;
  sym<decltype(&gph_control_free)>(h, "gph_control_free")(c);
  for (const Variant &v : VARIANTS)
    if (n <= v.leaves && K <= v.pops && B <= v.bands) {
      std::string p2 = dir + "/" + v.file;
      if (p2 != path) { void *h2 = dlopen(p2.c_str(), RTLD_NOW | RTLD_LOCAL); if (h2) h = h2; }
      break;
    }
  return h;
}

// the launcher's children, for the signal handler: a launcher that is told to stop takes its ranks with it
static pid_t g_kids[64];
static volatile sig_atomic_t g_nkids = 0;
static void forward_signal(int sig)
{
  for (int r = 0; r < g_nkids; r++) if (g_kids[r] > 0) kill(g_kids[r], sig);
  _exit(128 + sig);
}

static int usage(const char *a0)
{
  fprintf(stderr, "usage: %s [-v] [-d device] [-g gpus] [-l locus-summary-file] [-s coal-stats-prefix [--coal-stats-rows N] [--time-slices S]] [--ancestry ancestry-prefix] [--gene-trees trees-prefix [--gene-trees-loci SPEC] [--gene-trees-rows N]] [--clades clades-prefix [--clades-loci SPEC] [--clades-slots P] [--clades-min-support F]] [--ess ess-prefix [--ess-loci SPEC]] [--predictive pp-prefix [--predictive-loci SPEC] [--predictive-seed N] [--predictive-rows N]] [--triplets tw-prefix [--triplets-pops \"A,B,C;D,E,F\"] [--triplets-loci SPEC] [--triplets-rows N]] [--mutations mutations-prefix [--mutations-loci SPEC] [--mutations-rows N]] [--pair-times pt-prefix [--pair-times-pops \"A,B;A,A\"] [--pair-times-grid LO,HI,B] [--pair-times-loci SPEC] [--pair-times-rows N]] [--sfs sfs-prefix [--sfs-pairs \"A,B;C,D\"|none] [--sfs-loci SPEC] [--sfs-rows N]] [--beta B] [--marginal-likelihood ml-prefix [--ml-steps K] [--ml-burnin b] [--ml-samples s] [--ml-alpha a]] [--mc3 C [--mc3-heat h] [--mc3-swap-every k] [--mc3-report mc3-prefix]] [--replicates R --replicates-out rep-prefix [--replicates-min-freq F] [--replicates-every k]] <control-file> [secondary-control-file]\n", a0);
  return 1;
}

int main(int argc, char **argv)
{
  int gpus = 1, i = 1;
  gph_run_options o;
  memset(&o, 0, sizeof o);
  o.size = sizeof o;
  for (; i < argc && argv[i][0] == '-'; i++) {
    if (!strcmp(argv[i], "-v") || !strcmp(argv[i], "--verbose")) o.verbose = 1;
    else if (!strcmp(argv[i], "-d") && i + 1 < argc) o.device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-g") && i + 1 < argc) gpus = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-l") && i + 1 < argc) o.locus_summary_path = argv[++i];
    else if (!strcmp(argv[i], "-s") && i + 1 < argc) o.coal_stats_prefix = argv[++i];
    else if (!strcmp(argv[i], "--coal-stats-rows") && i + 1 < argc) o.coal_stats_rows = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--time-slices") && i + 1 < argc) { o.time_slices = atoi(argv[++i]); if (o.time_slices < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--ancestry") && i + 1 < argc) o.ancestry_prefix = argv[++i];
    else if (!strcmp(argv[i], "--gene-trees") && i + 1 < argc) o.gene_trees_prefix = argv[++i];
    else if (!strcmp(argv[i], "--gene-trees-loci") && i + 1 < argc) o.gene_trees_loci = argv[++i];
    else if (!strcmp(argv[i], "--gene-trees-rows") && i + 1 < argc) { o.gene_trees_rows = atoi(argv[++i]); if (o.gene_trees_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--ess") && i + 1 < argc) o.ess_prefix = argv[++i];
    else if (!strcmp(argv[i], "--ess-loci") && i + 1 < argc) o.ess_loci = argv[++i];
    else if (!strcmp(argv[i], "--predictive") && i + 1 < argc) o.predictive_prefix = argv[++i];
    else if (!strcmp(argv[i], "--predictive-loci") && i + 1 < argc) o.predictive_loci = argv[++i];
    else if (!strcmp(argv[i], "--predictive-seed") && i + 1 < argc) o.predictive_seed = argv[++i];
    else if (!strcmp(argv[i], "--predictive-rows") && i + 1 < argc) { o.predictive_rows = atoi(argv[++i]); if (o.predictive_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--triplets") && i + 1 < argc) o.triplets_prefix = argv[++i];
    else if (!strcmp(argv[i], "--triplets-pops") && i + 1 < argc) o.triplets_pops = argv[++i];
    else if (!strcmp(argv[i], "--triplets-loci") && i + 1 < argc) o.triplets_loci = argv[++i];
    else if (!strcmp(argv[i], "--triplets-rows") && i + 1 < argc) { o.triplets_rows = atoi(argv[++i]); if (o.triplets_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--mutations") && i + 1 < argc) o.mutations_prefix = argv[++i];
    else if (!strcmp(argv[i], "--mutations-loci") && i + 1 < argc) o.mutations_loci = argv[++i];
    else if (!strcmp(argv[i], "--mutations-rows") && i + 1 < argc) { o.mutations_rows = atoi(argv[++i]); if (o.mutations_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--simulate") && i + 1 < argc) o.simulate_prefix = argv[++i];
    else if (!strcmp(argv[i], "--simulate-loci") && i + 1 < argc) o.simulate_loci = argv[++i];
    else if (!strcmp(argv[i], "--simulate-seed") && i + 1 < argc) o.simulate_seed = argv[++i];
    else if (!strcmp(argv[i], "--simulate-rows") && i + 1 < argc) { o.simulate_rows = atoi(argv[++i]); if (o.simulate_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--simulate-no-sites")) o.simulate_no_sites = 1;
    else if (!strcmp(argv[i], "--pair-times") && i + 1 < argc) o.pair_times_prefix = argv[++i];
    else if (!strcmp(argv[i], "--pair-times-pops") && i + 1 < argc) o.pair_times_pops = argv[++i];
    else if (!strcmp(argv[i], "--pair-times-grid") && i + 1 < argc) o.pair_times_grid = argv[++i];
    else if (!strcmp(argv[i], "--pair-times-loci") && i + 1 < argc) o.pair_times_loci = argv[++i];
    else if (!strcmp(argv[i], "--pair-times-rows") && i + 1 < argc) { o.pair_times_rows = atoi(argv[++i]); if (o.pair_times_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--sfs") && i + 1 < argc) o.sfs_prefix = argv[++i];
    else if (!strcmp(argv[i], "--sfs-pairs") && i + 1 < argc) o.sfs_pairs = argv[++i];
    else if (!strcmp(argv[i], "--sfs-loci") && i + 1 < argc) o.sfs_loci = argv[++i];
    else if (!strcmp(argv[i], "--sfs-rows") && i + 1 < argc) { o.sfs_rows = atoi(argv[++i]); if (o.sfs_rows < 1) return usage(argv[0]); }
    else if (!strcmp(argv[i], "--clades") && i + 1 < argc) o.clades_prefix = argv[++i];
    else if (!strcmp(argv[i], "--clades-loci") && i + 1 < argc) o.clades_loci = argv[++i];
    else if (!strcmp(argv[i], "--clades-slots") && i + 1 < argc) {
      o.clades_slots = atoi(argv[++i]);
      if (o.clades_slots < 2 || (o.clades_slots & (o.clades_slots - 1))) { fprintf(stderr, "%s: --clades-slots takes a power of two >= 2\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--clades-min-support") && i + 1 < argc) {
      char *end = nullptr;
      const double F = strtod(argv[++i], &end);
      if (end == argv[i] || *end || !(F >= 0.0 && F <= 1.0)) { fprintf(stderr, "%s: --clades-min-support takes a number in [0, 1]\n", argv[0]); return usage(argv[0]); }
      o.clades_min_support = F == 0.0 ? -1.0 : F;      /* (0 in the options struct means the default) */
    }
    else if (!strcmp(argv[i], "--beta") && i + 1 < argc) {
      char *end = nullptr;
      const double B = strtod(argv[++i], &end);
      if (end == argv[i] || *end || !(B >= 0.0 && B <= 64.0)) { fprintf(stderr, "%s: --beta takes a number in [0, 64]\n", argv[0]); return usage(argv[0]); }
      o.beta = B == 0.0 ? -1.0 : B;                    /* (0 in the options struct means not given) */
    }
    else if (!strcmp(argv[i], "--marginal-likelihood") && i + 1 < argc) o.marginal_prefix = argv[++i];
    else if (!strcmp(argv[i], "--ml-steps") && i + 1 < argc) {
      o.marginal_steps = atoi(argv[++i]);
      if (o.marginal_steps < 1) { fprintf(stderr, "%s: --ml-steps takes a number of steps K >= 1\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--ml-burnin") && i + 1 < argc) {
      o.marginal_burnin = atoi(argv[++i]);
      if (o.marginal_burnin < 0) { fprintf(stderr, "%s: --ml-burnin takes a number of iterations b >= 0\n", argv[0]); return usage(argv[0]); }
      if (o.marginal_burnin == 0) o.marginal_burnin = -1;     /* (0 in the options struct means the default) */
    }
    else if (!strcmp(argv[i], "--ml-samples") && i + 1 < argc) {
      o.marginal_samples = atoi(argv[++i]);
      if (o.marginal_samples < 1) { fprintf(stderr, "%s: --ml-samples takes a number of samples s >= 1\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--ml-alpha") && i + 1 < argc) {
      char *end = nullptr;
      o.marginal_alpha = strtod(argv[++i], &end);
      if (end == argv[i] || *end || !(o.marginal_alpha > 0.0) || o.marginal_alpha > 1e300) { fprintf(stderr, "%s: --ml-alpha takes a finite number a > 0\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--mc3") && i + 1 < argc) {
      o.mc3_chains = atoi(argv[++i]);
      if (o.mc3_chains < 2 || o.mc3_chains > 16) { fprintf(stderr, "%s: --mc3 takes a number of chains C in 2 .. 16\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--mc3-heat") && i + 1 < argc) {
      char *end = nullptr;
      o.mc3_heat = strtod(argv[++i], &end);
      if (end == argv[i] || *end || !(o.mc3_heat > 0.0) || o.mc3_heat > 1e300) { fprintf(stderr, "%s: --mc3-heat takes a finite number h > 0\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--mc3-swap-every") && i + 1 < argc) {
      o.mc3_swap_every = atoi(argv[++i]);
      if (o.mc3_swap_every == 0) { fprintf(stderr, "%s: --mc3-swap-every takes a number of iterations k >= 1, or a negative number for no swaps\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--mc3-report") && i + 1 < argc) o.mc3_report_prefix = argv[++i];
    else if (!strcmp(argv[i], "--replicates") && i + 1 < argc) {
      o.replicates = atoi(argv[++i]);
      if (o.replicates < 2 || o.replicates > 16) { fprintf(stderr, "%s: --replicates takes a number of chains R in 2 .. 16\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "--replicates-out") && i + 1 < argc) o.replicates_prefix = argv[++i];
    else if (!strcmp(argv[i], "--replicates-min-freq") && i + 1 < argc) {
      char *end = nullptr;
      const double F = strtod(argv[++i], &end);
      if (end == argv[i] || *end || !(F >= 0.0 && F <= 1.0)) { fprintf(stderr, "%s: --replicates-min-freq takes a number in [0, 1]\n", argv[0]); return usage(argv[0]); }
      o.replicates_min_freq = F == 0.0 ? -1.0 : F;     /* (0 in the options struct means the default) */
    }
    else if (!strcmp(argv[i], "--replicates-every") && i + 1 < argc) {
      o.replicates_every = atoi(argv[++i]);
      if (o.replicates_every < 1) { fprintf(stderr, "%s: --replicates-every takes a number of samples k >= 1\n", argv[0]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[i], "-n") && i + 1 < argc) ++i;   /* thread count of the OpenMP build: accepted, ignored */
    else return usage(argv[0]);
  }
  if (i >= argc || gpus < 1 || gpus > 64) return usage(argv[0]);
  if (o.time_slices && !o.coal_stats_prefix) { fprintf(stderr, "%s: --time-slices needs -s PREFIX\n", argv[0]); return usage(argv[0]); }
  if ((o.gene_trees_loci || o.gene_trees_rows) && !o.gene_trees_prefix) { fprintf(stderr, "%s: --gene-trees-loci and --gene-trees-rows need --gene-trees PREFIX\n", argv[0]); return usage(argv[0]); }
  if ((o.clades_loci || o.clades_slots || o.clades_min_support != 0.0) && !o.clades_prefix) { fprintf(stderr, "%s: --clades-loci, --clades-slots and --clades-min-support need --clades PREFIX\n", argv[0]); return usage(argv[0]); }
  if (o.ess_loci && !o.ess_prefix) { fprintf(stderr, "%s: --ess-loci needs --ess PREFIX\n", argv[0]); return usage(argv[0]); }
  if ((o.predictive_loci || o.predictive_seed || o.predictive_rows) && !o.predictive_prefix) {
    fprintf(stderr, "%s: --predictive-loci, --predictive-seed and --predictive-rows need --predictive PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if ((o.triplets_pops || o.triplets_loci || o.triplets_rows) && !o.triplets_prefix) {
    fprintf(stderr, "%s: --triplets-pops, --triplets-loci and --triplets-rows need --triplets PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if ((o.mutations_loci || o.mutations_rows) && !o.mutations_prefix) {
    fprintf(stderr, "%s: --mutations-loci and --mutations-rows need --mutations PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if ((o.simulate_loci || o.simulate_seed || o.simulate_rows || o.simulate_no_sites) && !o.simulate_prefix) {
    fprintf(stderr, "%s: --simulate-loci, --simulate-seed, --simulate-rows and --simulate-no-sites need --simulate PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if ((o.pair_times_pops || o.pair_times_grid || o.pair_times_loci || o.pair_times_rows) && !o.pair_times_prefix) {
    fprintf(stderr, "%s: --pair-times-pops, --pair-times-grid, --pair-times-loci and --pair-times-rows need --pair-times PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if ((o.sfs_pairs || o.sfs_loci || o.sfs_rows) && !o.sfs_prefix) {
    fprintf(stderr, "%s: --sfs-pairs, --sfs-loci and --sfs-rows need --sfs PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if ((o.marginal_steps || o.marginal_burnin || o.marginal_samples || o.marginal_alpha != 0.0) && !o.marginal_prefix) {
    fprintf(stderr, "%s: --ml-steps, --ml-burnin, --ml-samples and --ml-alpha need --marginal-likelihood PREFIX\n", argv[0]);
    return usage(argv[0]);
  }
  if (o.beta != 0.0 && o.marginal_prefix) { fprintf(stderr, "%s: --beta and --marginal-likelihood exclude each other\n", argv[0]); return usage(argv[0]); }
  if ((o.mc3_heat != 0.0 || o.mc3_swap_every || o.mc3_report_prefix) && !o.mc3_chains) {
    fprintf(stderr, "%s: --mc3-heat, --mc3-swap-every and --mc3-report need --mc3 C\n", argv[0]);
    return usage(argv[0]);
  }
  if (o.mc3_chains && gpus > 1) { fprintf(stderr, "%s: --mc3 runs its chains on one GPU: not with -g N > 1\n", argv[0]); return usage(argv[0]); }
  if (o.mc3_chains && o.beta != 0.0) { fprintf(stderr, "%s: --mc3 and --beta exclude each other\n", argv[0]); return usage(argv[0]); }
  if (o.mc3_chains && o.marginal_prefix) { fprintf(stderr, "%s: --mc3 and --marginal-likelihood exclude each other\n", argv[0]); return usage(argv[0]); }
  if ((o.replicates_prefix || o.replicates_min_freq != 0.0 || o.replicates_every) && !o.replicates) {
    fprintf(stderr, "%s: --replicates-out, --replicates-min-freq and --replicates-every need --replicates R\n", argv[0]);
    return usage(argv[0]);
  }
  if (o.replicates && !o.replicates_prefix) { fprintf(stderr, "%s: --replicates needs --replicates-out PREFIX\n", argv[0]); return usage(argv[0]); }
  if (o.replicates_every && !o.clades_prefix) { fprintf(stderr, "%s: --replicates-every needs --clades PREFIX\n", argv[0]); return usage(argv[0]); }
  if (o.replicates && gpus > 1) { fprintf(stderr, "%s: --replicates runs its chains on one GPU: not with -g N > 1\n", argv[0]); return usage(argv[0]); }
  if (o.replicates && o.mc3_chains) { fprintf(stderr, "%s: --replicates and --mc3 exclude each other\n", argv[0]); return usage(argv[0]); }
  if (o.replicates && o.beta != 0.0) { fprintf(stderr, "%s: --replicates and --beta exclude each other\n", argv[0]); return usage(argv[0]); }
  if (o.replicates && o.marginal_prefix) { fprintf(stderr, "%s: --replicates and --marginal-likelihood exclude each other\n", argv[0]); return usage(argv[0]); }
  o.ctl = argv[i];
  o.ctl2 = i + 1 < argc ? argv[i + 1] : nullptr;
  char self[PATH_MAX];
  ssize_t k = readlink("/proc/self/exe", self, sizeof self - 1);
  if (k <= 0) { perror("readlink"); return 2; }
  self[k] = 0;
  const std::string dir = dirname(self);
  if (gpus == 1) {
    void *h = load_engine(dir, o.ctl, o.ctl2);
    return sym<decltype(&gph_run)>(h, "gph_run")(&o) ? 1 : 0;
  }

  // ---- one chain over `gpus` ranks.  Nothing below this line touches a GPU in the parent.
  const size_t page = 1 << 20;
  char *shared = (char *)mmap(nullptr, page, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  if (shared == MAP_FAILED) { perror("mmap"); return 2; }
  memset(shared, 0, page);
  std::vector<pid_t> kids(gpus, -1);
  for (int r = 0; r < gpus; r++) {
    pid_t p = fork();
    if (p < 0) { perror("fork"); for (int q = 0; q < r; q++) kill(kids[q], SIGTERM); return 2; }
    if (p == 0) {
      prctl(PR_SET_PDEATHSIG, SIGTERM);          /* the launcher died (killed -9, say): do not linger in an exchange */
      if (getppid() == 1) _exit(2);
      void *h = load_engine(dir, o.ctl, o.ctl2);
      Mailbox *mb = (Mailbox *)shared;
      // how many devices are there?  Child 0 asks (the first GPU call of this process tree) and tells the others
      // through the engine library: gph_comm_create_* are the only entry points that need to know
      auto create_rccl = sym<decltype(&gph_comm_create_rccl)>(h, "gph_comm_create_rccl");
      auto attach_shm = sym<decltype(&gph_comm_attach_shm)>(h, "gph_comm_attach_shm");
      auto shm_bytes = sym<decltype(&gph_comm_shm_bytes)>(h, "gph_comm_shm_bytes");
      auto unique_id = sym<decltype(&gph_comm_unique_id)>(h, "gph_comm_unique_id");
      auto destroy = sym<decltype(&gph_comm_destroy)>(h, "gph_comm_destroy");
      auto ndevices = sym<int (*)()>(h, "gph_device_count");
      const int ndev = ndevices();
      if (ndev < 1) { fprintf(stderr, "G-PhoCS-hip: no HIP device\n"); _exit(2); }
      const int mydev = o.device + r < ndev ? o.device + r : (o.device + r) % ndev;
      const bool share = gpus > ndev - o.device || getenv("GPHOCS_HIP_SHM");   /* ranks would share a device */
      gph_comm *comm = nullptr;
      if (share) {
        if (shm_bytes(gpus) + 4096 > page) { fprintf(stderr, "G-PhoCS-hip: shared page too small\n"); _exit(2); }
        comm = attach_shm(shared + 4096, r, gpus);
        if (r == 0 && o.verbose) printf("%d ranks on %d device(s): host shared-memory exchange (RCCL wants one GPU per rank)\n", gpus, ndev);
      } else {
        if (r == 0) {
          if (unique_id(mb->id)) _exit(2);
          mb->id_ready.store(1, std::memory_order_release);
        } else {
          for (int spin = 0; !mb->id_ready.load(std::memory_order_acquire); spin++) { if (spin > 600000) _exit(2); usleep(100); }
        }
        comm = create_rccl(mb->id, r, gpus, mydev);
      }
      if (!comm) { fprintf(stderr, "G-PhoCS-hip: rank %d could not join the communicator\n", r); _exit(2); }
      o.device = mydev;
      o.comm = comm;
      int rc = sym<decltype(&gph_run)>(h, "gph_run")(&o);
      fflush(stdout);
      if (rc == 0) destroy(comm);
      _exit(rc ? 1 : 0);
    }
    kids[r] = p;
    g_kids[r] = p;
    g_nkids = r + 1;
  }
  signal(SIGTERM, forward_signal);
  signal(SIGINT, forward_signal);
  // a rank that fails takes the job down: the others would wait for it in the next exchange
  int status = 0, left = gpus, bad = 0;
  while (left > 0) {
    pid_t p = wait(&status);
    if (p < 0) {
      if (errno == EINTR) continue;
      perror("G-PhoCS-hip: wait");             /* no children left to wait for although some are unaccounted: a failure */
      for (int r = 0; r < gpus; r++) kill(kids[r], SIGTERM);
      return 2;
    }
    left--;
    const bool failed = !WIFEXITED(status) || WEXITSTATUS(status) != 0;
    if (failed && !bad) {
      bad = 1;
      for (int r = 0; r < gpus; r++) if (kids[r] != p) kill(kids[r], SIGTERM);
    }
  }
  if (o.locus_summary_path) {
    /* the ranks' parts of the summary table, in rank order */
    FILE *out = bad ? nullptr : fopen(o.locus_summary_path, "w");
    if (!bad && !out) { perror(o.locus_summary_path); bad = 1; }
    for (int r = 0; r < gpus; r++) {
      const std::string part = std::string(o.locus_summary_path) + ".part" + std::to_string(r);
      if (out) {
        FILE *in = fopen(part.c_str(), "r");
        if (!in) { fprintf(stderr, "G-PhoCS-hip: %s is missing\n", part.c_str()); bad = 1; }
        else {
          char buf[1 << 16];
          size_t nr;
          while ((nr = fread(buf, 1, sizeof buf, in)) > 0)
            if (fwrite(buf, 1, nr, out) != nr) { perror(o.locus_summary_path); bad = 1; break; }
          fclose(in);
        }
      }
      unlink(part.c_str());
    }
    if (out && fclose(out) != 0) { perror(o.locus_summary_path); bad = 1; }
    if (bad && out) unlink(o.locus_summary_path);
  }
  if (o.coal_stats_prefix || o.ancestry_prefix || o.gene_trees_prefix || o.clades_prefix || o.ess_prefix || o.predictive_prefix || o.triplets_prefix || o.mutations_prefix || o.simulate_prefix || o.pair_times_prefix || o.sfs_prefix || o.marginal_prefix || o.mc3_report_prefix || o.replicates_prefix) {
    /* the ranks' parts into the files, by the library that wrote them -- or, after a failure, removed */
    if (sym<decltype(&gph_run_finish)>(load_engine(dir, o.ctl, o.ctl2), "gph_run_finish")(&o, gpus, bad)) bad = 1;
  }
  return bad;
}
