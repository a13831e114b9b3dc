// gph_mutations_run.h -- `--mutations PREFIX [--mutations-loci SPEC] [--mutations-rows N]` (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  k_mutations keeps the per-locus
// accumulators and the per-sample rows on the device (gph_engine_mutations_*); the rows are fetched whenever their buffer is
// full and at the end, the accumulators once, at the end.
// Rank r's text part PREFIX.mutations.part<r> (gph_textparts.h; MuJoin in gph_textjoin.h reads it):
// "H\t<samples>\t<K>\t<n>" + "\t<name>" per population, then per leaf; this rank's rows of PREFIX.mutations.tsv as "L\t" + row;
// its per-sample rows as R lines (RowsOutput) whose numbers are the BIT PATTERNS of the doubles, so that the ranks' doubles add
// without loss.
struct Mutations : RowsOutput {
  int32_t C = 0;
  std::vector<double> dbuf;          /* one fetch as the engine hands it out: [row][1 + C], column 0 the iteration */
  explicit Mutations(const gph_run_options &o) : RowsOutput(MU_TEXT, o.mutations_prefix, o.mutations_loci, "--mutations-loci", o.mutations_rows) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.mutations_prefix && (o.mutations_loci || o.mutations_rows)) {
      fprintf(stderr, "gphocs_hip: --mutations-loci and --mutations-rows need --mutations PREFIX\n");
      return GPH_EARG;
    }
    if (o.mutations_rows < 0) { fprintf(stderr, "gphocs_hip: --mutations-rows %d is no row count\n", (int)o.mutations_rows); return GPH_EARG; }
    return GPH_OK;
  }
  int open(Run &R) override
  {
    size_rows(C = 2 * (R.cfg.K + R.cfg.n));
    if (int rc = enabled(R, gph_engine_mutations_enable(R.E, capacity, loci(), (int64_t)sel.size(), 0), "gph_engine_mutations_enable",
                         "accumulators and rows exceed 1 GiB: narrow --mutations-loci or --mutations-rows")) return rc;
    int32_t c = 0;
    gph_engine_mutations_shape(R.E, &c, nullptr, nullptr, nullptr, nullptr);
    if (c != C) return R.fail(GPH_ESTATE, "gph_engine_mutations_shape");
    dbuf.assign((size_t)capacity * (1 + C), 0.0);
    return open_part(R);
  }
  int32_t held(Run &R) override { int32_t h = 0; gph_engine_mutations_shape(R.E, nullptr, nullptr, nullptr, nullptr, &h); return h; }
  int fetch(Run &R, int32_t *got) override
  {
    if (int rc = R.check(gph_engine_mutations_fetch_rows(R.E, dbuf.data(), capacity, got), "gph_engine_mutations_fetch_rows")) return rc;
    for (int32_t r = 0; r < *got; r++) {
      const double *row = dbuf.data() + (size_t)r * (1 + C);
      ibuf[(size_t)r] = (int32_t)row[0];
      memcpy(buf.data() + (size_t)r * C, row + 1, (size_t)C * 8);      /* (the doubles as they are, in 64-bit words) */
    }
    return GPH_OK;
  }
  int take(Run &R, int it) override { return R.check(gph_engine_mutations_sample(R.E, it), "gph_engine_mutations_sample"); }
  int close(Run &R) override
  {
    int64_t S = 0;
    gph_engine_mutations_shape(R.E, nullptr, nullptr, nullptr, &S, nullptr);
    if (int rc = flush(R)) return rc;
    const int K = R.cfg.K, n = R.cfg.n;
    std::vector<double> acc(sel.size() * (size_t)C + 1);
    if (int rc = gph_engine_mutations_fetch_loci(R.E, acc.data(), (int64_t)C, 0)) return R.fail(rc, "gph_engine_mutations_fetch_loci");
    fprintf(part.f, "H\t%lld\t%d\t%d", (long long)S, K, n);
    for (const std::string &nm : pop_names(R.C, R.cfg)) fprintf(part.f, "\t%s", nm.c_str());
    for (const std::string &nm : leaf_names(R.C, R.cfg)) fprintf(part.f, "\t%s", nm.c_str());
    fputc('\n', part.f);
    const int64_t *poff = nullptr;
    const int32_t *counts = nullptr;
    gph_loci_arrays(R.LC, nullptr, nullptr, &poff, nullptr, nullptr, &counts, nullptr, nullptr);
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      long long sites = 0;                          /* (the rows inside a group of phases carry count 0) */
      for (int64_t r = poff[sel[q]]; r < poff[sel[q] + 1]; r++) sites += counts[r];
      const double *a = acc.data() + q * (size_t)C;
      std::string text;
      char num[64];
      double smut = 0.0, sexp = 0.0;
      for (int p = 0; p < K; p++) {
        smut = smut + a[p];
        sexp = sexp + a[K + p];
        snprintf(num, sizeof num, "\t%.10g\t%.10g", S > 0 ? a[p] / (double)S : 0.0, S > 0 ? a[K + p] / (double)S : 0.0);
        text += num;
      }
      part.line("L\t%lld\t%s\t%lld\t%lld%s\t%.10g\n", (long long)sel[q], nm ? nm : "", (long long)S, sites, text.c_str(), sexp > 0.0 ? smut / sexp : 0.0);
    }
    write_rows();
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_mutations_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_mutations_discard(prefix, ranks); }
};
