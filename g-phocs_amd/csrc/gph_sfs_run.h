// gph_sfs_run.h -- `--sfs PREFIX [--sfs-pairs "A,B;C,D"|none] [--sfs-loci SPEC] [--sfs-rows N]` (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind the other outputs.  k_sfs_data forms the data side once, at
// enable; k_sfs_tree keeps the per-locus accumulators and the per-sample rows on the device (gph_engine_sfs_*); the rows are
// fetched whenever their buffer is full and at the end, the accumulators and the data side once, at the end.
// Rank r's text part PREFIX.sfs.part<r> (gph_textparts.h; SfsJoin in gph_textjoin.h reads it):
// "H\t<samples>\t<slots>\t<groups>" + "\t<name>" per slot, then per group, + "\t<0|1>" per slot (1: a spectrum slot); this rank's
// rows of PREFIX.sfs.tsv as "L\t" + row; its observed totals as "O" + "\t<u64>" per slot; its per-sample rows as R lines
// (RowsOutput) whose numbers are the BIT PATTERNS of the doubles, so that the ranks' doubles add without loss.
struct Sfs : RowsOutput {
  const char *pairs_text;
  std::vector<int32_t> named;        /* --sfs-pairs: [pair][2] population indices as given */
  bool none = false;                 /* --sfs-pairs none */
  int32_t NS = 0, NG = 0;
  std::vector<double> dbuf;          /* one fetch as the engine hands it out: [row][1 + NS], column 0 the iteration */
  explicit Sfs(const gph_run_options &o) : RowsOutput(SF_TEXT, o.sfs_prefix, o.sfs_loci, "--sfs-loci", o.sfs_rows), pairs_text(o.sfs_pairs) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.sfs_prefix && (o.sfs_pairs || o.sfs_loci || o.sfs_rows)) {
      fprintf(stderr, "gphocs_hip: --sfs-pairs, --sfs-loci and --sfs-rows need --sfs PREFIX\n");
      return GPH_EARG;
    }
    if (o.sfs_rows < 0) { fprintf(stderr, "gphocs_hip: --sfs-rows %d is no row count\n", (int)o.sfs_rows); return GPH_EARG; }
    return GPH_OK;
  }
  /* the model and the names of --sfs-pairs, once the control file is read and before the sequence file is */
  int check_pops(Run &R)
  {
    const int Kc = R.cfg.Kc;
    bool bins = false;
    for (int p = 0; p < Kc; p++) bins = bins || R.cfg.samplesPerPop[p] >= 2;
    none = pairs_text && !strcmp(pairs_text, "none");
    if (!pairs_text || none) {
      bool any = false;
      for (int P = 0; P < Kc && !none; P++)
        for (int Q = P + 1; Q < Kc; Q++) any = any || (R.cfg.samplesPerPop[P] >= 1 && R.cfg.samplesPerPop[Q] >= 1);
      if (bins || any) return GPH_OK;
      snprintf(R.err, sizeof R.err, "no population of the model has two samples and no pair is taken: there is nothing to count");
      return R.fail(GPH_EARG, none ? "--sfs-pairs" : "--sfs");
    }
    const std::vector<std::string> names = pop_names(R.C, R.cfg);
    const std::string text(pairs_text);
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
          return R.fail(GPH_EARG, "--sfs-pairs");
        }
        if (k < 2) m[(size_t)k] = p;
        at = comma + 1;
      }
      if (k != 2 || m[0] == m[1]) {
        snprintf(R.err, sizeof R.err, "'%s' does not name two populations", one.c_str());
        return R.fail(GPH_EARG, "--sfs-pairs");
      }
      named.insert(named.end(), m.begin(), m.end());
      std::sort(m.begin(), m.end());
      if (R.cfg.samplesPerPop[m[0]] < 1 || R.cfg.samplesPerPop[m[1]] < 1) {
        snprintf(R.err, sizeof R.err, "the pair '%s' names a population without a sample", one.c_str());
        return R.fail(GPH_EARG, "--sfs-pairs");
      }
      if (std::find(seen.begin(), seen.end(), m) != seen.end()) {
        snprintf(R.err, sizeof R.err, "the pair '%s' is named twice", one.c_str());
        return R.fail(GPH_EARG, "--sfs-pairs");
      }
      seen.push_back(m);
      from = semi + 1;
    }
    return GPH_OK;
  }
  int open(Run &R) override
  {
    static const int32_t nothing[2] = {0, 0};
    const bool all = named.empty() && !none;
    /* the slots as the engine will count them: the row buffer's default needs their number */
    const int Kc = R.cfg.Kc;
    int32_t ns = 0, ng = 0;
    for (int p = 0; p < Kc; p++)
      if (R.cfg.samplesPerPop[p] >= 2) { ns += R.cfg.samplesPerPop[p] / 2; ng++; }
    for (int P = 0; P < Kc && all; P++)
      for (int Q = P + 1; Q < Kc; Q++)
        if (R.cfg.samplesPerPop[P] >= 1 && R.cfg.samplesPerPop[Q] >= 1) { ns += 4; ng++; }
    ns += 4 * (int32_t)(named.size() / 2); ng += (int32_t)(named.size() / 2);
    size_rows(ns);
    if (int rc = enabled(R, gph_engine_sfs_enable(R.E, capacity, loci(), (int64_t)sel.size(), all ? nullptr : named.empty() ? nothing : named.data(), (int32_t)(named.size() / 2), 0),
                         "gph_engine_sfs_enable", "accumulators and rows exceed 1 GiB: narrow --sfs-loci, --sfs-pairs or --sfs-rows")) return rc;
    gph_engine_sfs_shape(R.E, &NS, &NG, nullptr, nullptr, nullptr, nullptr);
    if (NS != ns || NG != ng) return R.fail(GPH_ESTATE, "gph_engine_sfs_shape");
    dbuf.assign((size_t)capacity * (1 + NS), 0.0);
    return open_part(R);
  }
  int32_t held(Run &R) override { int32_t h = 0; gph_engine_sfs_shape(R.E, nullptr, nullptr, nullptr, nullptr, nullptr, &h); return h; }
  int fetch(Run &R, int32_t *got) override
  {
    if (int rc = R.check(gph_engine_sfs_fetch_rows(R.E, dbuf.data(), capacity, got), "gph_engine_sfs_fetch_rows")) return rc;
    for (int32_t r = 0; r < *got; r++) {
      const double *row = dbuf.data() + (size_t)r * (1 + NS);
      ibuf[(size_t)r] = (int32_t)row[0];
      memcpy(buf.data() + (size_t)r * NS, row + 1, (size_t)NS * 8);      /* (the doubles as they are, in 64-bit words) */
    }
    return GPH_OK;
  }
  int take(Run &R, int it) override { return R.check(gph_engine_sfs_sample(R.E, it), "gph_engine_sfs_sample"); }
  int close(Run &R) override
  {
    int64_t S = 0;
    gph_engine_sfs_shape(R.E, nullptr, nullptr, nullptr, nullptr, &S, nullptr);
    if (int rc = flush(R)) return rc;
    const size_t W = (size_t)NS + NG + 1;
    std::vector<double> acc(sel.size() * (size_t)NS + 1);
    std::vector<uint32_t> obs(sel.size() * W + 1);
    std::vector<uint64_t> tot(W);
    std::vector<int32_t> slots((size_t)NS * 5);
    if (int rc = gph_engine_sfs_fetch_loci(R.E, acc.data(), (int64_t)NS, 0)) return R.fail(rc, "gph_engine_sfs_fetch_loci");
    if (int rc = gph_engine_sfs_fetch_observed(R.E, obs.data(), (int64_t)W, tot.data())) return R.fail(rc, "gph_engine_sfs_fetch_observed");
    if (int rc = gph_engine_sfs_slots(R.E, slots.data())) return R.fail(rc, "gph_engine_sfs_slots");
    const std::vector<std::string> names = pop_names(R.C, R.cfg);
    static const char *const cls[5] = {"sfs_", "privP_", "privQ_", "shared_", "fixed_"};
    std::vector<std::string> gname((size_t)NG);
    fprintf(part.f, "H\t%lld\t%d\t%d", (long long)S, (int)NS, (int)NG);
    for (int s = 0; s < NS; s++) {
      const int32_t *d = slots.data() + 5 * s;
      const std::string g = d[1] == 0 ? names[(size_t)d[2]] : names[(size_t)d[2]] + "|" + names[(size_t)d[3]];
      gname[(size_t)d[0]] = g;
      if (d[1] == 0) fprintf(part.f, "\t%s%s:%d", cls[0], g.c_str(), (int)d[4]);
      else fprintf(part.f, "\t%s%s", cls[d[1]], g.c_str());
    }
    for (const std::string &g : gname) fprintf(part.f, "\t%s", g.c_str());
    for (int s = 0; s < NS; s++) fprintf(part.f, "\t%d", slots[(size_t)(5 * s + 1)] == 0 ? 1 : 0);
    fputc('\n', part.f);
    const double Sd = (double)S;
    for (size_t q = 0; q < sel.size(); q++) {
      const char *nm = gph_loci_name(R.LC, sel[q]);
      const double *E = acc.data() + q * (size_t)NS;
      const uint32_t *o = obs.data() + q * W;
      std::string text;
      char num[96];
      for (int g = 0; g < NG; g++) { snprintf(num, sizeof num, "\t%u", (unsigned)o[NS + g]); text += num; }
      double sobs = 0.0, sexp = 0.0;
      for (int s = 0; s < NS; s++) {
        const double ex = S > 0 ? ((double)o[NS + slots[(size_t)(5 * s)]] * E[s]) / Sd : 0.0;
        if (slots[(size_t)(5 * s + 1)] == 0) { sobs = sobs + (double)o[s]; sexp = sexp + ex; }
        snprintf(num, sizeof num, "\t%u\t%.10g", (unsigned)o[s], ex);
        text += num;
      }
      part.line("L\t%lld\t%s\t%lld\t%u%s\t%.10g\n", (long long)sel[q], nm ? nm : "", (long long)S, (unsigned)o[NS + NG], text.c_str(), sexp > 0.0 ? sobs / sexp : 0.0);
    }
    part.numbers("O", nullptr, tot.data(), (size_t)NS);
    write_rows();
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_sfs_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_sfs_discard(prefix, ranks); }
};
