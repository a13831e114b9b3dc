// gph_ess_run.h -- `--ess PREFIX [--ess-loci SPEC]` (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  Per trace column: the values every
// trace line prints are kept on the host before formatting (Run::trace_kept, as the replicate chains' are) and go through
// gph_ess once, at the end, on rank 0.  Per locus: k_ess keeps the levels on the device (gph_engine_ess_*); they are fetched
// once, at the end, and read at the level with batch <= sqrt(samples).
// Rank r's text part PREFIX.ess.part<r> (gph_textparts.h; EsJoin in gph_textjoin.h reads it): "H\t<samples>\t<level>\t
// <series>", rank 0's rows of PREFIX.ess.tsv as "P\t" + row (its summary line included), this rank's rows of
// PREFIX.locus-ess.tsv as "L\t<minEss, %a>\t" + row.
struct Ess : TextOutput {
  std::vector<double> x, vals;       /* [sample][column]: what the trace lines print, before formatting; scratch */
  explicit Ess(const gph_run_options &o) : TextOutput(ES_TEXT, o.ess_prefix, o.ess_loci, "--ess-loci") {}
  static int validate(const gph_run_options &o)
  {
    if (!o.ess_prefix && o.ess_loci) { fprintf(stderr, "gphocs_hip: --ess-loci needs --ess PREFIX\n"); return GPH_EARG; }
    return GPH_OK;
  }
  int open(Run &R) override
  {
    if (int rc = enabled(R, gph_engine_ess_enable(R.E, loci(), (int64_t)sel.size(), 0), "gph_engine_ess_enable",
                         "the accumulators exceed 1 GiB: narrow --ess-loci")) return rc;
    if (int rc = open_part(R)) return rc;
    vals.assign((size_t)R.mc.numParameters + 4, 0.0);
    return GPH_OK;
  }
  int sample(Run &R, int) override
  {
    double logL, dataL;
    if (R.lead) R.trace_kept(R.M, vals.data(), x, logL, dataL);
    return R.check(gph_engine_ess_sample(R.E), "gph_engine_ess_sample");
  }
  int close(Run &R) override
  {
    int32_t M = 0, J = 0;
    int64_t S = 0;
    gph_engine_ess_shape(R.E, nullptr, &M, &J, nullptr, &S);
    const int words = 2 + 2 * J;
    std::vector<double> acc(sel.size() * (size_t)M * words + 1);
    std::vector<uint32_t> changes(sel.size() + 1);
    if (int rc = gph_engine_ess_fetch(R.E, acc.data(), changes.data(), nullptr, 0)) return R.fail(rc, "gph_engine_ess_fetch");
    double r5[5] = {0, 0, 0, 0, 0};
    { const double zero[64] = {0}; gph_ess_read(zero, S, -1, r5); }        /* (the level of S samples) */
    const int level = (int)r5[4];
    fprintf(part.f, "H\t%lld\t%d\t%d\n", (long long)S, level, (int)M);
    if (R.lead) {
      const std::vector<std::string> names = R.trace_columns();
      const int ncol = R.mc.numParameters + 2;
      std::vector<double> col((size_t)(S > 0 ? S : 1));
      double worst = 0.0;
      int worst_at = -1;
      for (int i = 0; i < ncol; i++) {
        for (int64_t s = 0; s < S; s++) col[(size_t)s] = x[(size_t)s * ncol + i];
        double o8[8] = {S > 0 ? col[0] : 0.0, 0, 0, 0, 0, 0, (double)level, 0};
        if (S >= 2)
          if (int rc = gph_ess(col.data(), S, 0, o8)) return R.fail(rc, "gph_ess");
        part.line("P\t%s\t%lld\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\t%d\n", names[(size_t)i].c_str(), (long long)S, o8[0], o8[1], o8[3], o8[5], o8[4], (int)o8[7]);
        if (o8[1] > 0.0 && (worst_at < 0 || o8[5] < worst)) { worst = o8[5]; worst_at = i; }      /* (a constant column has no ESS) */
      }
      part.line("P\t# samples %lld level %d batch %lld minEssAcf %.10g (%s)\n", (long long)S, level, 1ll << level, worst,
                worst_at < 0 ? "-" : names[(size_t)worst_at].c_str());
    }
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      double least = 0.0, e[6];
      bool any = false;
      for (int m = 0; m < M; m++) {
        if (int rc = gph_ess_read(acc.data() + (q * (size_t)M + m) * words, S, -1, r5)) return R.fail(rc, "gph_ess_read");
        e[m] = r5[3];
        if (r5[1] > 0.0 && (!any || r5[3] < least)) { least = r5[3]; any = true; }
      }
      std::string series;
      char num[64];
      for (int m = 0; m < M; m++) { snprintf(num, sizeof num, "\t%.10g", e[m]); series += num; }
      part.line("L\t%a\t%lld\t%s\t%lld%s\t%u\t%.10g\n", least, (long long)sel[q], nm ? nm : "", (long long)S, series.c_str(), (unsigned)changes[q], least);
    }
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_ess_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_ess_discard(prefix, ranks); }
};
