// gph_mc3_run.h -- `--mc3 C [--mc3-heat h] [--mc3-swap-every k] [--mc3-report PREFIX]` (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind Run.  Chain 0 is the run's own engine and driver (Run::E,
// Run::M): the trace, the log, the finetune search and every output go on working on it, and because a swap exchanges states
// it stays the cold chain.  The heated chains 1 .. C - 1 are further engines on the same device, loaded from the same host
// arrays, owned here.
std::string mc3_path(const char *prefix) { return std::string(prefix) + ".mc3.tsv"; }

struct Mc3Run {
  const int C, every;
  const double h;
  std::vector<gph_engine *> E;          /* chains 1 .. C - 1 */
  std::vector<gph_mcmc *> M;
  std::vector<gph_mcmc *> all;          /* chain 0 (the run's) and those */
  gph_mc3 *G = nullptr;
  std::vector<double> betas, sumL;
  int64_t nL = 0, nIter = 0;
  const char *const opt = "--mc3";     /* the option the group runs for */
  /* `--replicates R` (gph_replicates_run.h): the same group with every beta = 1 and no swaps */
  Mc3Run(int chains, const char *option) : C(chains), every(-1), h(0.0), opt(option) {}
  explicit Mc3Run(const gph_run_options &o) : C(o.mc3_chains), every(o.mc3_swap_every == 0 ? 1 : o.mc3_swap_every < 0 ? -1 : o.mc3_swap_every),
                                              h(o.mc3_heat != 0.0 ? o.mc3_heat : 0.1) {}
  ~Mc3Run()
  {
    if (G) gph_mc3_destroy(G);
    for (gph_mcmc *m : M) gph_mcmc_destroy(m);
    for (gph_engine *e : E) gph_engine_destroy(e);
  }
  static int refuse(const char *msg) { fprintf(stderr, "gphocs_hip: %s\n", msg); return GPH_EARG; }
  static int validate(const gph_run_options &o)
  {
    if (!o.mc3_chains) {
      if (o.mc3_heat != 0.0) return refuse("--mc3-heat needs --mc3 C");
      if (o.mc3_swap_every) return refuse("--mc3-swap-every needs --mc3 C");
      if (o.mc3_report_prefix) return refuse("--mc3-report needs --mc3 C");
      return GPH_OK;
    }
    if (o.mc3_chains < 2 || o.mc3_chains > 16) return refuse("--mc3 takes a number of chains C in 2 .. 16");
    if (!(o.mc3_heat >= 0.0) || std::isinf(o.mc3_heat)) return refuse("--mc3-heat takes a finite number h > 0");
    if (o.world > 1 || o.comm || o.allreduce) return refuse("--mc3 runs its chains on one GPU: not with -g N > 1, a communicator or an all-reduce hook");
    if (o.beta != 0.0) return refuse("--mc3 and --beta exclude each other: the ladder sets every chain's beta");
    if (o.marginal_prefix) return refuse("--mc3 and --marginal-likelihood exclude each other");
    return GPH_OK;
  }
  /* the heated chains, behind Run::start_engine and in front of gph_mcmc_initialize of chain 0 */
  int start(Run &R)
  {
    int rc;
    double bytes = 0.0;
    gph_engine_hbm_bytes(R.E, &bytes);
    for (int c = 0; c < C; c++) betas.push_back(1.0 / (1.0 + h * c));
    all.push_back(R.M);
    for (int c = 1; c < C; c++) {
      gph_engine *e = nullptr;
      gph_mcmc *m = nullptr;
      gph_mcmc_config mc = R.mc;
      mc.seed = R.mc.seed + c;
      if ((rc = gph_engine_create(&R.cfg, &e))) return R.fail(rc, "gph_engine_create of a heated chain");
      E.push_back(e);
      if ((rc = gph_engine_load_loci(e, R.le - R.lb, R.offs + R.lb, R.leaf, R.ph, R.cnt, R.info.mutRateMode == 2 ? R.rates + R.lb : nullptr))) {
        snprintf(R.err, sizeof R.err, "%s %d: chain %d could not be allocated; every chain takes %.1f MB of device memory, %.1f MB in all", opt, C, c,
                 bytes / 1e6, C * bytes / 1e6);
        return R.fail(rc, "gph_engine_load_loci of a heated chain");
      }
      if ((rc = gph_mcmc_create(e, &R.cfg, &mc, &m))) return R.fail(rc, "gph_mcmc_create of a heated chain");
      M.push_back(m);
      all.push_back(m);
    }
    return GPH_OK;
  }
  /* behind gph_mcmc_initialize of chain 0: the others', the group, the line that states the ladder */
  int initialize(Run &R)
  {
    int rc;
    for (gph_mcmc *m : M)
      if ((rc = gph_mcmc_initialize(m, nullptr))) return R.fail(rc, "gph_mcmc_initialize of a heated chain");
    if ((rc = gph_mc3_create(all.data(), C, betas.data(), every, (uint32_t)(R.mc.seed + C), &G))) return R.fail(rc, "gph_mc3_create");
    sumL.assign(C, 0.0);
    if (R.lead && h != 0.0) {
      printf("MC3: %d chains on the ladder beta_c = 1 / (1 + %.10g c):", C, h);
      for (double b : betas) printf(" %.10g", b);
      if (every > 0) printf("; a swap of two neighbours is attempted every %d iteration(s).\n", every);
      else printf("; no swaps.\n");
    }
    return GPH_OK;
  }
  int iteration(Run &R, int it)
  {
    int rc;
    if ((rc = gph_mc3_iteration(G, it))) return R.fail(rc, "gph_mc3_iteration");
    nIter++;
    if (it >= 0) {
      for (int c = 0; c < C; c++) { double l = 0.0; gph_mcmc_get_state(all[c], nullptr, &l, nullptr, nullptr, nullptr); sumL[c] += l; }
      nL++;
    }
    return GPH_OK;
  }
  /* every chain runs with the step sizes and the log period chain 0 runs with */
  void push_finetunes(double coal, double mig, double theta, double rate, double mix, const double *taus, double locus)
  {
    for (gph_mcmc *m : M) { gph_mcmc_set_locus_rate_finetune(m, locus); gph_mcmc_set_finetunes(m, coal, mig, theta, rate, mix, taus); }
  }
  void set_log_period(int n) { for (gph_mcmc *m : M) gph_mcmc_set_log_period(m, n); }
  void totals(int64_t &att, int64_t &acc, std::vector<int64_t> &a, std::vector<int64_t> &b) const
  {
    a.assign(C, 0); b.assign(C, 0);
    gph_mc3_swap_counts(G, a.data(), b.data());
    att = acc = 0;
    for (int c = 0; c + 1 < C; c++) { att += a[c]; acc += b[c]; }
  }
  void log_pairs(const Run &R) const
  {
    if (!R.lead) return;
    std::vector<int64_t> a, b;
    int64_t att, acc;
    totals(att, acc, a, b);
    for (int c = 0; c + 1 < C; c++)
      printf("MC3: chains %d and %d (beta %.10g and %.10g): %lld swaps attempted, %lld accepted.\n", c, c + 1, betas[c], betas[c + 1],
             (long long)a[c], (long long)b[c]);
  }
  int write(Run &R, int64_t totalCoals) const
  {
    const std::string path = mc3_path(R.o.mc3_report_prefix);
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { snprintf(R.err, sizeof R.err, "Could not open %s", path.c_str()); return R.fail(GPH_EARG, "writing the MC3 report"); }
    std::vector<int64_t> a, b;
    int64_t att, acc;
    totals(att, acc, a, b);
    const gph_config &cfg = R.cfg;
    int ntau = cfg.K - cfg.Kc;
    for (int p = 0; p < cfg.Kc; p++) ntau += R.mc.updateSampleAge[p] != 0;
    const double n = (double)nIter;
    fprintf(f, "chain\tbeta\tseed\tswapAttempts\tswapAccepted\taccCoal\taccMig\taccSpr\taccTheta\taccMigRate\taccTau\taccMixing\tmeanLnL\n");
    for (int c = 0; c < C; c++) {
      int64_t k[9];
      gph_mcmc_accept_counts(all[c], k);
      const double v[7] = {k[0] / (n * (double)totalCoals), k[7] > 0 ? k[1] / (double)k[7] : 0.0, k[2] / (n * 2 * (double)totalCoals), k[3] / (n * cfg.K),
                           cfg.B > 0 ? k[4] / (n * cfg.B) : 0.0, ntau > 0 ? k[5] / (n * ntau) : 0.0, k[6] / n};
      fprintf(f, "%d\t%.10g\t%d\t%lld\t%lld", c, betas[c], R.mc.seed + c, (long long)a[c], (long long)b[c]);
      for (double x : v) fprintf(f, "\t%.10g", x);
      fprintf(f, "\t%.10g\n", nL > 0 ? sumL[c] / (double)nL : 0.0);
    }
    fprintf(f, "# heat %.10g every %d attempted %lld accepted %lld\n", h, every, (long long)att, (long long)acc);
    const int rcc = ferror(f) | fclose(f);
    if (rcc) { unlink(path.c_str()); return R.fail(GPH_EARG, "writing the MC3 report"); }
    return GPH_OK;
  }
};
