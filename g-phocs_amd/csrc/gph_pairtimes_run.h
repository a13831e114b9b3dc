// gph_pairtimes_run.h -- `--pair-times PREFIX [--pair-times-pops "A,B;A,A"] [--pair-times-grid LO,HI,B] [--pair-times-loci SPEC]
// [--pair-times-rows N]` (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  k_pair_times keeps the per-locus
// accumulators and the per-sample rows on the device (gph_engine_pair_times_*); the rows are fetched whenever their buffer is
// full and at the end, the accumulators once, at the end.
// Rank r's text part PREFIX.pair-times.part<r> (gph_textparts.h; PtJoin in gph_textjoin.h reads it):
// "H\t<samples>\t<pairs>\t<bins>" + "\t<P>,<Q>,<m>" (names, leaf pairs) per pair + "\t<u64>" per edge (the double's 64-bit
// pattern), this rank's rows of PREFIX.pair-times.tsv as "L\t" + row, its per-sample rows as "R\t<iteration>" + "\t<u64>" per
// number of a row.
struct PairTimes : RowsOutput {
  const char *pops, *grid;
  std::vector<int32_t> named;        /* --pair-times-pops: [pair][2] population indices as given; empty: all pairs */
  std::vector<int32_t> pr;           /* the pairs taken, members sorted: [NP][2] */
  std::vector<double> edges;
  int32_t NP = 0, B = 0;
  explicit PairTimes(const gph_run_options &o)
    : RowsOutput(PT_TEXT, o.pair_times_prefix, o.pair_times_loci, "--pair-times-loci", o.pair_times_rows), pops(o.pair_times_pops), grid(o.pair_times_grid) {}
  /* "LO,HI,B": B bins, E = B - 1 edges e_k = LO (HI / LO)^(k / (E - 1)), the two ends exact */
  static bool parse_grid(const char *text, std::vector<double> &e, char *err, size_t errlen)
  {
    double lo = 0.0, hi = 0.0;
    int b = 0, used = 0;
    const char *t = text ? text : "1e-6,1e-2,34";
    if (sscanf(t, "%lf,%lf,%d%n", &lo, &hi, &b, &used) != 3 || t[used] != '\0') { snprintf(err, errlen, "'%s' is not LO,HI,B", t); return false; }
    if (!std::isfinite(lo) || !(lo > 0.0)) { snprintf(err, errlen, "LO = %g is not a positive number", lo); return false; }
    if (!std::isfinite(hi) || !(hi > lo)) { snprintf(err, errlen, "HI = %g does not lie above LO = %g", hi, lo); return false; }
    if (b < 3 || b > 128) { snprintf(err, errlen, "B = %d: a grid has 3 .. 128 bins", b); return false; }
    const int E = b - 1;
    e.assign((size_t)E, 0.0);
    for (int k = 0; k < E; k++) e[(size_t)k] = k == 0 ? lo : k == E - 1 ? hi : lo * pow(hi / lo, (double)k / (double)(E - 1));
    for (int k = 1; k < E; k++)
      if (!(e[(size_t)k] > e[(size_t)k - 1])) { snprintf(err, errlen, "LO = %g, HI = %g are too close for %d distinct edges", lo, hi, E); return false; }
    return true;
  }
  static int validate(const gph_run_options &o)
  {
    if (!o.pair_times_prefix && (o.pair_times_pops || o.pair_times_grid || o.pair_times_loci || o.pair_times_rows)) {
      fprintf(stderr, "gphocs_hip: --pair-times-pops, --pair-times-grid, --pair-times-loci and --pair-times-rows need --pair-times PREFIX\n");
      return GPH_EARG;
    }
    if (o.pair_times_rows < 0) { fprintf(stderr, "gphocs_hip: --pair-times-rows %d is no row count\n", (int)o.pair_times_rows); return GPH_EARG; }
    if (o.pair_times_prefix) {
      std::vector<double> e;
      char err[256];
      if (!parse_grid(o.pair_times_grid, e, err, sizeof err)) { fprintf(stderr, "gphocs_hip: --pair-times-grid: %s\n", err); return GPH_EARG; }
    }
    return GPH_OK;
  }
  static int64_t leaf_pairs(const gph_config &cfg, int P, int Q)
  {
    const int64_t a = cfg.samplesPerPop[P], b = cfg.samplesPerPop[Q];
    return P == Q ? a * (a - 1) / 2 : a * b;
  }
  /* the model and the names of --pair-times-pops, once the control file is read and before the sequence file is */
  int check_pops(Run &R)
  {
    const int Kc = R.cfg.Kc;
    char err[256];
    if (!parse_grid(grid, edges, err, sizeof err)) { snprintf(R.err, sizeof R.err, "%s", err); return R.fail(GPH_EARG, "--pair-times-grid"); }
    if (!pops) {
      bool any = false;
      for (int P = 0; P < Kc; P++)
        for (int Q = P; Q < Kc; Q++) any = any || leaf_pairs(R.cfg, P, Q) >= 1;
      if (any) return GPH_OK;
      snprintf(R.err, sizeof R.err, "the model has no pair of populations with a pair of samples");
      return R.fail(GPH_EARG, "--pair-times");
    }
    const std::vector<std::string> names = pop_names(R.C, R.cfg);
    const std::string text(pops);
    std::vector<std::array<int32_t, 2>> seen;
    for (size_t from = 0; from <= text.size();) {
      const size_t semi = std::min(text.find(';', from), text.size());
      const std::string one = text.substr(from, semi - from);
      std::array<int32_t, 2> m = {{-1, -1}};
      int k = 0;
      for (size_t at = 0; at <= one.size(); k++) {
        const size_t comma = std::min(one.find(',', at), one.size());
        const std::string nm = one.substr(at, comma - at);
        int p = -1;
        for (int c = 0; c < Kc; c++) if (names[(size_t)c] == nm) p = c;
        if (p < 0) {
          snprintf(R.err, sizeof R.err, "'%s' in '%s' is no current population of the control file", nm.c_str(), one.c_str());
          return R.fail(GPH_EARG, "--pair-times-pops");
        }
        if (k < 2) m[(size_t)k] = p;
        at = comma + 1;
      }
      if (k != 2) {
        snprintf(R.err, sizeof R.err, "'%s' does not name two populations", one.c_str());
        return R.fail(GPH_EARG, "--pair-times-pops");
      }
      named.insert(named.end(), m.begin(), m.end());
      std::sort(m.begin(), m.end());
      if (leaf_pairs(R.cfg, m[0], m[1]) < 1) {
        if (m[0] == m[1]) snprintf(R.err, sizeof R.err, "the pair '%s' has no pair of samples: population '%s' has fewer than two samples", one.c_str(), names[(size_t)m[0]].c_str());
        else snprintf(R.err, sizeof R.err, "the pair '%s' has no pair of samples: one of its populations has no sample", one.c_str());
        return R.fail(GPH_EARG, "--pair-times-pops");
      }
      if (std::find(seen.begin(), seen.end(), m) != seen.end()) {
        snprintf(R.err, sizeof R.err, "the pair '%s' is named twice", one.c_str());
        return R.fail(GPH_EARG, "--pair-times-pops");
      }
      seen.push_back(m);
      from = semi + 1;
    }
    return GPH_OK;
  }
  int open(Run &R) override
  {
    const int Kc = R.cfg.Kc;
    if (named.empty()) {
      for (int P = 0; P < Kc; P++)
        for (int Q = P; Q < Kc; Q++)
          if (leaf_pairs(R.cfg, P, Q) >= 1) { pr.push_back(P); pr.push_back(Q); }
    } else {
      pr = named;
      for (size_t k = 0; k < pr.size(); k += 2) std::sort(pr.begin() + (long)k, pr.begin() + (long)k + 2);
    }
    NP = (int32_t)(pr.size() / 2);
    B = (int32_t)edges.size() + 1;
    size_rows(NP * (B + 2));
    if (int rc = enabled(R, gph_engine_pair_times_enable(R.E, capacity, loci(), (int64_t)sel.size(), named.empty() ? nullptr : named.data(), (int32_t)(named.size() / 2),
                                                         edges.data(), (int32_t)edges.size(), 0),
                         "gph_engine_pair_times_enable", "accumulators and rows exceed 1 GiB: narrow --pair-times-loci, --pair-times-pops, --pair-times-grid or --pair-times-rows")) return rc;
    int32_t np = 0, b = 0;
    gph_engine_pair_times_shape(R.E, &np, &b, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (np != NP || b != B) return R.fail(GPH_ESTATE, "gph_engine_pair_times_shape");
    return open_part(R);
  }
  int32_t held(Run &R) override { int32_t h = 0; gph_engine_pair_times_shape(R.E, nullptr, nullptr, nullptr, nullptr, nullptr, &h, nullptr); return h; }
  int fetch(Run &R, int32_t *got) override { return R.check(gph_engine_pair_times_fetch_rows(R.E, ibuf.data(), buf.data(), width, capacity, got), "gph_engine_pair_times_fetch_rows"); }
  int take(Run &R, int it) override { return R.check(gph_engine_pair_times_sample(R.E, it), "gph_engine_pair_times_sample"); }
  int close(Run &R) override
  {
    int64_t S = 0;
    gph_engine_pair_times_shape(R.E, nullptr, nullptr, nullptr, nullptr, &S, nullptr, nullptr);
    if (int rc = flush(R)) return rc;
    const size_t w = 4 * (size_t)NP;
    std::vector<double> acc(sel.size() * w + 1);
    if (int rc = gph_engine_pair_times_fetch_loci(R.E, acc.data(), (int64_t)w, 0)) return R.fail(rc, "gph_engine_pair_times_fetch_loci");
    const std::vector<std::string> names = pop_names(R.C, R.cfg);
    fprintf(part.f, "H\t%lld\t%d\t%d", (long long)S, (int)NP, (int)B);
    for (int k = 0; k < NP; k++)
      fprintf(part.f, "\t%s,%s,%lld", names[(size_t)pr[2 * k]].c_str(), names[(size_t)pr[2 * k + 1]].c_str(), (long long)leaf_pairs(R.cfg, pr[2 * k], pr[2 * k + 1]));
    for (double e : edges) { uint64_t bits; memcpy(&bits, &e, 8); fprintf(part.f, "\t%llu", (unsigned long long)bits); }
    fputc('\n', part.f);
    const double Sd = (double)S;
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      const double *A = acc.data() + q * w, *Y = A + NP, *X = Y + NP, *M = X + NP;
      for (int k = 0; k < NP; k++) {
        const long long m = (long long)leaf_pairs(R.cfg, pr[2 * k], pr[2 * k + 1]);
        const double all = Sd * (double)m;
        part.line("L\t%lld\t%s\t%lld\t%s\t%s\t%lld\t%.10g\t%.10g\t%.10g\t%.10g\n", (long long)sel[q], nm ? nm : "", (long long)S, names[(size_t)pr[2 * k]].c_str(),
                  names[(size_t)pr[2 * k + 1]].c_str(), m, all > 0.0 ? A[k] / all : 0.0, S > 0 ? M[k] / Sd : 0.0, S > 0 ? X[k] / Sd : 0.0, all > 0.0 ? Y[k] / all : 0.0);
      }
    }
    write_rows();
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_pair_times_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_pair_times_discard(prefix, ranks); }
};
