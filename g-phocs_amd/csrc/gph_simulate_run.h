// gph_simulate_run.h -- `--simulate PREFIX [--simulate-loci SPEC] [--simulate-seed N] [--simulate-rows N] [--simulate-no-sites]`
// (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  k_simulate and the site loop keep the
// per-locus accumulators and the per-sample rows on the device (gph_engine_simulate_*); the rows are fetched whenever their buffer
// is full and at the end, the accumulators once, at the end.
// Rank r's text part PREFIX.simulate.part<r> (gph_textparts.h; SiJoin in gph_textjoin.h reads it):
// "H\t<samples>\t<M>\t<C>\t<K>\t<B>\t<seed>" + "\t<name>" per genealogy statistic, then per site statistic; this rank's rows of
// PREFIX.simulate.tsv as "L\t<minP, %a>\t<failed>\t" + row; with sites its observed totals as "O" + "\t<u64>" per site statistic; its
// per-sample rows as "R\t<iteration>" + "\t<u64>" per column.
struct Simulate : RowsOutput {
  const char *seed_text;
  const bool with_sites;
  uint64_t seed = 0;
  int32_t M = 0, C = 0;
  uint64_t *observed = nullptr;      /* where the next fetch of rows leaves the data's site totals, if anywhere */
  explicit Simulate(const gph_run_options &o)
    : RowsOutput(SI_TEXT, o.simulate_prefix, o.simulate_loci, "--simulate-loci", o.simulate_rows), seed_text(o.simulate_seed), with_sites(!o.simulate_no_sites) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.simulate_prefix && (o.simulate_loci || o.simulate_seed || o.simulate_rows || o.simulate_no_sites)) {
      fprintf(stderr, "gphocs_hip: --simulate-loci, --simulate-seed, --simulate-rows and --simulate-no-sites need --simulate PREFIX\n");
      return GPH_EARG;
    }
    if (o.simulate_rows < 0) { fprintf(stderr, "gphocs_hip: --simulate-rows %d is no row count\n", (int)o.simulate_rows); return GPH_EARG; }
    if (o.simulate_seed) {
      char *end = nullptr;
      errno = 0;
      (void)strtoull(o.simulate_seed, &end, 10);
      if (errno || end == o.simulate_seed || *end || o.simulate_seed[0] == '-') { fprintf(stderr, "gphocs_hip: --simulate-seed %s is no unsigned number\n", o.simulate_seed); return GPH_EARG; }
    }
    return GPH_OK;
  }
  int open(Run &R) override
  {
    seed = seed_text ? (uint64_t)strtoull(seed_text, nullptr, 10) : (uint64_t)(int64_t)R.mc.seed;
    M = 3 + R.cfg.K + R.cfg.B;
    C = with_sites ? 1 + R.cfg.Kc * (R.cfg.Kc + 1) / 2 : 0;
    size_rows(2 * (R.cfg.K + R.cfg.B) + 4 + C);
    if (int rc = enabled(R, gph_engine_simulate_enable(R.E, seed, capacity, loci(), (int64_t)sel.size(), with_sites ? 1 : 0, 0), "gph_engine_simulate_enable",
                         "accumulators, records and rows exceed 1 GiB: narrow --simulate-loci or --simulate-rows")) return rc;
    return open_part(R);
  }
  int32_t held(Run &R) override { int32_t h = 0; gph_engine_simulate_shape(R.E, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &h); return h; }
  int fetch(Run &R, int32_t *got) override { return R.check(gph_engine_simulate_fetch_rows(R.E, ibuf.data(), buf.data(), observed, capacity, got), "gph_engine_simulate_fetch_rows"); }
  int take(Run &R, int it) override { return R.check(gph_engine_simulate_sample(R.E, it), "gph_engine_simulate_sample"); }
  std::vector<std::string> stat_names(Run &R) const
  {
    std::vector<std::string> v = {"tmrca", "length", "genLnL"};
    for (const std::string &nm : pop_names(R.C, R.cfg)) v.push_back("coal_" + nm);
    for (const std::string &nm : band_names(R.C, R.cfg)) v.push_back("mig_" + nm);
    return v;
  }
  std::vector<std::string> site_names(Run &R) const
  {
    std::vector<std::string> v;
    if (!with_sites) return v;
    const std::vector<std::string> pops = pop_names(R.C, R.cfg);
    v.push_back("seg");
    for (int p = 0; p < R.cfg.Kc; p++)
      for (int q = p; q < R.cfg.Kc; q++) v.push_back("diff_" + pops[(size_t)p] + "|" + pops[(size_t)q]);
    return v;
  }
  int close(Run &R) override
  {
    int64_t S = 0;
    gph_engine_simulate_shape(R.E, nullptr, nullptr, nullptr, nullptr, nullptr, &S, nullptr);
    std::vector<uint64_t> totals((size_t)C + 1, 0);
    observed = totals.data();
    if (int rc = flush(R)) return rc;
    const size_t W = 5 * (size_t)M + 1;
    std::vector<double> acc(sel.size() * W + 1), sacc(sel.size() * (size_t)C * 5 + 1);
    std::vector<int64_t> sites(sel.size() + 1);
    if (int rc = gph_engine_simulate_fetch_loci(R.E, acc.data(), C ? sacc.data() : nullptr, sites.data(), 0)) return R.fail(rc, "gph_engine_simulate_fetch_loci");
    std::vector<std::string> names = stat_names(R);
    for (const std::string &nm : site_names(R)) names.push_back(nm);
    fprintf(part.f, "H\t%lld\t%d\t%d\t%d\t%d\t%llu", (long long)S, (int)M, (int)C, (int)R.cfg.K, (int)R.cfg.B, (unsigned long long)seed);
    for (const std::string &nm : names) fprintf(part.f, "\t%s", nm.c_str());
    fputc('\n', part.f);
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      const double *a = acc.data() + q * W, failed = a[5 * (size_t)M], n = (double)S - failed;
      std::string row;
      char num[512];
      double minp = 0.0;
      int at = -1;
      for (int c = 0; c < M + C; c++) {
        const double *w = c < M ? a + 5 * (size_t)c : sacc.data() + (q * (size_t)C + (size_t)(c - M)) * 5;
        /* (a genealogy statistic: gt, eq, sx, sy, sy2; a site statistic: obs, gt, eq, s1, s2) */
        const double gt = c < M ? w[0] : w[1], eq = c < M ? w[1] : w[2], s1 = w[3], s2 = w[4];
        const double first = c < M ? (n > 0 ? w[2] / n : 0.0) : w[0];
        const double mean = n > 0 ? s1 / n : 0.0;
        double var = n > 1 ? (s2 - s1 * s1 / n) / (n - 1) : 0.0;
        if (!(var > 0.0)) var = 0.0;
        const double p = n > 0 ? (gt + eq / 2) / n : 0.0, two = 2 * (p < 1 - p ? p : 1 - p);
        if (at < 0 || two < minp) { minp = two; at = c; }
        snprintf(num, sizeof num, "\t%.10g\t%.10g\t%.10g\t%.10g", first, mean, sqrt(var), p);
        row += num;
      }
      part.line("L\t%a\t%lld\t%lld\t%s\t%lld\t%lld\t%lld%s\t%.10g\t%s\n", minp, (long long)failed, (long long)sel[q], nm ? nm : "", (long long)S, (long long)failed,
                (long long)sites[q], row.c_str(), minp, names[(size_t)at].c_str());
    }
    if (C > 0) part.numbers("O", nullptr, totals.data(), (size_t)C);
    write_rows();
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_simulate_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_simulate_discard(prefix, ranks); }
};
