// gph_triplets_run.h -- `--triplets PREFIX [--triplets-pops "A,B,C;D,E,F"] [--triplets-loci SPEC] [--triplets-rows N]`
// (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  k_triplets keeps the per-locus
// accumulators and the per-sample rows on the device (gph_engine_triplets_*); the rows are fetched whenever their buffer is
// full and at the end, the accumulators once, at the end.
// Rank r's text part PREFIX.triplets.part<r> (gph_textparts.h; TrJoin in gph_textjoin.h reads it):
// "H\t<samples>\t<triples>" + "\t<P>,<Q>,<R>" (names) per triple, this rank's rows of PREFIX.triplets.tsv as "L\t" + row, its
// per-sample rows as "R\t<iteration>" + "\t<u64>" per slot.
struct Triplets : RowsOutput {
  const char *pops;
  std::vector<int32_t> named;        /* --triplets-pops: [triple][3] population indices as given; empty: all triples */
  std::vector<int32_t> tri;          /* the triples taken, members sorted: [T][3] */
  int32_t T = 0, slots = 0;
  explicit Triplets(const gph_run_options &o) : RowsOutput(TR_TEXT, o.triplets_prefix, o.triplets_loci, "--triplets-loci", o.triplets_rows), pops(o.triplets_pops) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.triplets_prefix && (o.triplets_pops || o.triplets_loci || o.triplets_rows)) {
      fprintf(stderr, "gphocs_hip: --triplets-pops, --triplets-loci and --triplets-rows need --triplets PREFIX\n");
      return GPH_EARG;
    }
    if (o.triplets_rows < 0) { fprintf(stderr, "gphocs_hip: --triplets-rows %d is no row count\n", (int)o.triplets_rows); return GPH_EARG; }
    return GPH_OK;
  }
  /* the model and the names of --triplets-pops, once the control file is read and before the sequence file is */
  int check_pops(Run &R)
  {
    const int Kc = R.cfg.Kc;
    if (Kc < 3) {
      snprintf(R.err, sizeof R.err, "the model has %d current population(s), a triple needs three", Kc);
      return R.fail(GPH_EARG, "--triplets");
    }
    if (!pops) return GPH_OK;
    const std::vector<std::string> names = pop_names(R.C, R.cfg);
    const std::string text(pops);
    std::vector<std::array<int32_t, 3>> seen;
    for (size_t from = 0; from <= text.size();) {
      const size_t semi = std::min(text.find(';', from), text.size());
      const std::string one = text.substr(from, semi - from);
      std::array<int32_t, 3> m = {{-1, -1, -1}};
      int k = 0;
      for (size_t at = 0; at <= one.size(); k++) {
        const size_t comma = std::min(one.find(',', at), one.size());
        const std::string nm = one.substr(at, comma - at);
        int p = -1;
        for (int c = 0; c < Kc; c++) if (names[(size_t)c] == nm) p = c;
        if (p < 0) {
          snprintf(R.err, sizeof R.err, "'%s' in '%s' is no current population of the control file", nm.c_str(), one.c_str());
          return R.fail(GPH_EARG, "--triplets-pops");
        }
        if (k < 3) m[(size_t)k] = p;
        at = comma + 1;
      }
      if (k != 3 || m[0] == m[1] || m[0] == m[2] || m[1] == m[2]) {
        snprintf(R.err, sizeof R.err, "'%s' does not name three different populations", one.c_str());
        return R.fail(GPH_EARG, "--triplets-pops");
      }
      for (int a = 0; a < 3; a++)
        if (R.cfg.samplesPerPop[m[(size_t)a]] < 1) {
          snprintf(R.err, sizeof R.err, "population '%s' in '%s' has no sample", names[(size_t)m[(size_t)a]].c_str(), one.c_str());
          return R.fail(GPH_EARG, "--triplets-pops");
        }
      named.insert(named.end(), m.begin(), m.end());
      std::sort(m.begin(), m.end());
      if (std::find(seen.begin(), seen.end(), m) != seen.end()) {
        snprintf(R.err, sizeof R.err, "the triple '%s' is named twice", one.c_str());
        return R.fail(GPH_EARG, "--triplets-pops");
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
        for (int Q = P + 1; Q < Kc; Q++)
          for (int X = Q + 1; X < Kc; X++)
            if (R.cfg.samplesPerPop[P] >= 1 && R.cfg.samplesPerPop[Q] >= 1 && R.cfg.samplesPerPop[X] >= 1) { tri.push_back(P); tri.push_back(Q); tri.push_back(X); }
    } else {
      tri = named;
      for (size_t k = 0; k < tri.size(); k += 3) std::sort(tri.begin() + (long)k, tri.begin() + (long)k + 3);
    }
    T = (int32_t)(tri.size() / 3);
    size_rows(slots = 3 * T);
    if (int rc = enabled(R, gph_engine_triplets_enable(R.E, capacity, loci(), (int64_t)sel.size(), named.empty() ? nullptr : named.data(), (int32_t)(named.size() / 3), 0),
                         "gph_engine_triplets_enable", "accumulators and rows exceed 1 GiB: narrow --triplets-loci, --triplets-pops or --triplets-rows")) return rc;
    int32_t t = 0;
    gph_engine_triplets_shape(R.E, &t, nullptr, nullptr, nullptr, nullptr);
    if (t != T) return R.fail(GPH_ESTATE, "gph_engine_triplets_shape");
    return open_part(R);
  }
  int32_t held(Run &R) override { int32_t h = 0; gph_engine_triplets_shape(R.E, nullptr, nullptr, nullptr, nullptr, &h); return h; }
  int fetch(Run &R, int32_t *got) override { return R.check(gph_engine_triplets_fetch_rows(R.E, ibuf.data(), buf.data(), slots, capacity, got), "gph_engine_triplets_fetch_rows"); }
  int take(Run &R, int it) override { return R.check(gph_engine_triplets_sample(R.E, it), "gph_engine_triplets_sample"); }
  int close(Run &R) override
  {
    int64_t S = 0;
    gph_engine_triplets_shape(R.E, nullptr, nullptr, nullptr, &S, nullptr);
    if (int rc = flush(R)) return rc;
    const size_t w = 2 * (size_t)slots;
    std::vector<double> acc(sel.size() * w + 1);
    if (int rc = gph_engine_triplets_fetch_loci(R.E, acc.data(), (int64_t)w, 0)) return R.fail(rc, "gph_engine_triplets_fetch_loci");
    const std::vector<std::string> names = pop_names(R.C, R.cfg);
    fprintf(part.f, "H\t%lld\t%d", (long long)S, (int)T);
    for (int k = 0; k < T; k++) fprintf(part.f, "\t%s,%s,%s", names[(size_t)tri[3 * k]].c_str(), names[(size_t)tri[3 * k + 1]].c_str(), names[(size_t)tri[3 * k + 2]].c_str());
    fputc('\n', part.f);
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      for (int k = 0; k < T; k++) {
        const std::string m[3] = {names[(size_t)tri[3 * k]], names[(size_t)tri[3 * k + 1]], names[(size_t)tri[3 * k + 2]]};
        const double all = (double)S * ((double)R.cfg.samplesPerPop[tri[3 * k]] * (double)R.cfg.samplesPerPop[tri[3 * k + 1]] * (double)R.cfg.samplesPerPop[tri[3 * k + 2]]);
        const double *W = acc.data() + q * w + 3 * k, *A = W + slots;
        int top = 0;
        for (int t = 1; t < 3; t++) if (W[t] > W[top]) top = t;
        part.line("L\t%lld\t%s\t%lld\t%s\t%s\t%s\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\t%s\n", (long long)sel[q], nm ? nm : "", (long long)S,
                  m[0].c_str(), m[1].c_str(), m[2].c_str(), all > 0.0 ? W[0] / all : 0.0, all > 0.0 ? W[1] / all : 0.0, all > 0.0 ? W[2] / all : 0.0,
                  W[0] > 0.0 ? A[0] / W[0] : 0.0, W[1] > 0.0 ? A[1] / W[1] : 0.0, W[2] > 0.0 ? A[2] / W[2] : 0.0, tr_label(m, top).c_str());
      }
    }
    write_rows();
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_triplets_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_triplets_discard(prefix, ranks); }
};
