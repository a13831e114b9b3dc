// gph_predictive_run.h -- `--predictive PREFIX [--predictive-loci SPEC] [--predictive-seed N] [--predictive-rows N]`
// (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  k_predictive keeps the per-locus
// accumulators and the per-sample rows on the device (gph_engine_predictive_*); the rows are fetched whenever their buffer is
// full and at the end, the accumulators once, at the end.
// Rank r's text part PREFIX.predictive.part<r> (gph_textparts.h; PdJoin in gph_textjoin.h reads it):
// "H\t<samples>\t<statistics>\t<seed>" + "\t<name>" per statistic, this rank's rows of PREFIX.predictive.tsv as
// "L\t<minP, %a>\t" + row, its observed totals as "O" + "\t<u64>" per statistic, its per-sample rows as "R\t<iteration>" +
// "\t<u64>" per statistic.
struct Predictive : RowsOutput {
  const char *seed_text;
  uint64_t seed = 0;
  int32_t C = 0;
  uint64_t *observed = nullptr;      /* where the next fetch of rows leaves the data's totals, if anywhere */
  explicit Predictive(const gph_run_options &o) : RowsOutput(PD_TEXT, o.predictive_prefix, o.predictive_loci, "--predictive-loci", o.predictive_rows), seed_text(o.predictive_seed) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.predictive_prefix && (o.predictive_loci || o.predictive_seed || o.predictive_rows)) {
      fprintf(stderr, "gphocs_hip: --predictive-loci, --predictive-seed and --predictive-rows need --predictive PREFIX\n");
      return GPH_EARG;
    }
    if (o.predictive_rows < 0) { fprintf(stderr, "gphocs_hip: --predictive-rows %d is no row count\n", (int)o.predictive_rows); return GPH_EARG; }
    if (o.predictive_seed) {
      char *end = nullptr;
      errno = 0;
      (void)strtoull(o.predictive_seed, &end, 10);
      if (errno || end == o.predictive_seed || *end || o.predictive_seed[0] == '-') { fprintf(stderr, "gphocs_hip: --predictive-seed %s is no unsigned number\n", o.predictive_seed); return GPH_EARG; }
    }
    return GPH_OK;
  }
  int open(Run &R) override
  {
    seed = seed_text ? (uint64_t)strtoull(seed_text, nullptr, 10) : (uint64_t)(int64_t)R.mc.seed;
    size_rows(C = 1 + R.cfg.Kc * (R.cfg.Kc + 1) / 2);
    if (int rc = enabled(R, gph_engine_predictive_enable(R.E, seed, capacity, loci(), (int64_t)sel.size(), 0), "gph_engine_predictive_enable",
                         "accumulators and rows exceed 1 GiB: narrow --predictive-loci or --predictive-rows")) return rc;
    return open_part(R);
  }
  int32_t held(Run &R) override { int32_t h = 0; gph_engine_predictive_shape(R.E, nullptr, nullptr, nullptr, &h); return h; }
  /* (the one rows fetch without a leading dimension: its rows are C wide) */
  int fetch(Run &R, int32_t *got) override { return R.check(gph_engine_predictive_fetch_rows(R.E, ibuf.data(), buf.data(), observed, capacity, got), "gph_engine_predictive_fetch_rows"); }
  int take(Run &R, int it) override { return R.check(gph_engine_predictive_sample(R.E, it), "gph_engine_predictive_sample"); }
  std::string stat_name(Run &R, int c) const
  {
    if (c == 0) return "seg";
    const std::vector<std::string> pops = pop_names(R.C, R.cfg);
    for (int p = 0; p < R.cfg.Kc; p++)
      for (int q = p; q < R.cfg.Kc; q++)
        if (1 + p * R.cfg.Kc - p * (p - 1) / 2 + (q - p) == c) return "diff_" + pops[(size_t)p] + "|" + pops[(size_t)q];
    return "?";
  }
  int close(Run &R) override
  {
    int64_t S = 0;
    gph_engine_predictive_shape(R.E, nullptr, nullptr, &S, nullptr);
    std::vector<uint64_t> totals((size_t)C, 0);
    observed = totals.data();
    if (int rc = flush(R)) return rc;
    std::vector<double> acc(sel.size() * (size_t)C * 5 + 1);
    std::vector<int64_t> sites(sel.size() + 1);
    if (int rc = gph_engine_predictive_fetch_loci(R.E, acc.data(), sites.data(), 0)) return R.fail(rc, "gph_engine_predictive_fetch_loci");
    std::vector<std::string> names;
    for (int c = 0; c < C; c++) names.push_back(stat_name(R, c));
    fprintf(part.f, "H\t%lld\t%d\t%llu", (long long)S, (int)C, (unsigned long long)seed);
    for (const std::string &nm : names) fprintf(part.f, "\t%s", nm.c_str());
    fputc('\n', part.f);
    const double n = (double)S;
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      std::string row;
      char num[512];
      double minp = 0.0;
      int at = -1;
      for (int c = 0; c < C; c++) {
        const double *a = acc.data() + (q * (size_t)C + c) * 5;
        const double mean = S > 0 ? a[3] / n : 0.0;
        double var = S > 1 ? (a[4] - a[3] * a[3] / n) / (double)(S - 1) : 0.0;
        if (!(var > 0.0)) var = 0.0;
        const double p = S > 0 ? (a[1] + a[2] / 2) / n : 0.0, two = 2 * (p < 1 - p ? p : 1 - p);
        if (at < 0 || two < minp) { minp = two; at = c; }
        snprintf(num, sizeof num, "\t%.10g\t%.10g\t%.10g\t%.10g", a[0], mean, sqrt(var), p);
        row += num;
      }
      part.line("L\t%a\t%lld\t%s\t%lld\t%lld%s\t%.10g\t%s\n", minp, (long long)sel[q], nm ? nm : "", (long long)S, (long long)sites[q], row.c_str(), minp,
                names[(size_t)at].c_str());
    }
    part.numbers("O", nullptr, totals.data(), (size_t)C);
    write_rows();
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_predictive_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_predictive_discard(prefix, ranks); }
};
