// gph_replicates_run.h -- `--replicates R --replicates-out PREFIX [--replicates-min-freq F] [--replicates-every k]`
// (gph_run_options says what they do).
//
// Included by gph_program.cpp inside its anonymous namespace, behind Mc3Run and the outputs.  The R chains are an Mc3Run group
// with every beta = 1 and no swaps: chain 0 is the run's own engine and driver, chains 1 .. R - 1 are further engines on the same
// device, given every step size chain 0 is given.  What is added here: the other chains' trace files, their clade tables next
// to chain 0's, the values of every chain's trace lines kept for gph_psrf, and the per-locus comparison of the tables on the
// device (gph_engine_clades_compare).
std::string rep_path(const char *prefix, const char *what) { return std::string(prefix) + what; }

struct Replicates {
  const int C, every;
  const double F;
  Mc3Run &G;
  const Clades *clades = nullptr;       /* `--clades`: chain 0's tables, whose selection and slots the others take */
  std::vector<FILE *> trace;            /* chains 1 .. C - 1 */
  std::vector<std::vector<double>> x;   /* [chain][sample][column]: what the trace lines print, before formatting */
  std::vector<double> vals, rows;       /* scratch of a trace line; the rows of the last compare, [Q][6] */
  int ncol = 0;
  int64_t S = 0, Q = 0, rows_at = -1;   /* samples so far, selected loci, the sample count `rows` belongs to */
  Replicates(const gph_run_options &o, Mc3Run &group) : C(o.replicates), every(o.replicates_every),
    F(o.replicates_min_freq == 0.0 ? 0.1 : o.replicates_min_freq < 0.0 ? 0.0 : o.replicates_min_freq), G(group) {}
  ~Replicates() { for (FILE *f : trace) if (f) fclose(f); }
  static int refuse(const char *msg) { fprintf(stderr, "gphocs_hip: %s\n", msg); return GPH_EARG; }
  static int validate(const gph_run_options &o)
  {
    if (!o.replicates) {
      if (o.replicates_prefix) return refuse("--replicates-out needs --replicates R");
      if (o.replicates_min_freq != 0.0) return refuse("--replicates-min-freq needs --replicates R");
      if (o.replicates_every) return refuse("--replicates-every needs --replicates R");
      return GPH_OK;
    }
    if (o.replicates < 2 || o.replicates > 16) return refuse("--replicates takes a number of chains R in 2 .. 16");
    if (!o.replicates_prefix) return refuse("--replicates needs --replicates-out PREFIX");
    if (!(o.replicates_min_freq <= 1.0)) return refuse("--replicates-min-freq takes a number F in [0, 1]");
    if (o.replicates_every < 0) return refuse("--replicates-every takes a number of samples k >= 1");
    if (o.replicates_every && !o.clades_prefix) return refuse("--replicates-every needs --clades PREFIX");
    if (o.world > 1 || o.comm || o.allreduce) return refuse("--replicates runs its chains on one GPU: not with -g N > 1, a communicator or an all-reduce hook");
    if (o.mc3_chains) return refuse("--replicates and --mc3 exclude each other");
    if (o.beta != 0.0) return refuse("--replicates and --beta exclude each other: every chain samples the posterior");
    if (o.marginal_prefix) return refuse("--replicates and --marginal-likelihood exclude each other");
    return GPH_OK;
  }
  static std::string chain_trace_path(const char *prefix, int c) { return rep_path(prefix, ".chain") + std::to_string(c) + ".trace"; }
  /* behind the outputs' open: the other chains' tables and trace files */
  int open(Run &R, const Clades *cl)
  {
    clades = cl;
    ncol = R.mc.numParameters + 2;
    vals.assign(R.mc.numParameters + 4, 0.0);
    x.assign(C, std::vector<double>());
    if (clades) {
      const int64_t none = 0;
      Q = (int64_t)clades->sel.size();
      for (gph_engine *e : G.E)
        if (int rc = gph_engine_clades_enable(e, clades->slots, clades->sel.empty() ? &none : clades->sel.data(), (int64_t)clades->sel.size(), 0)) {
          if (rc == GPH_EFULL) snprintf(R.err, sizeof R.err, "the tables exceed 1 GiB: narrow --clades-loci or lower --clades-slots");
          return R.fail(rc, "gph_engine_clades_enable of a replicate chain");
        }
      rows.assign((size_t)Q * 6 + 1, 0.0);
    }
    for (int c = 1; c < C; c++) {
      const std::string path = chain_trace_path(R.o.replicates_prefix, c);
      FILE *f = fopen(R.lead ? path.c_str() : "/dev/null", "w");
      if (!f) { snprintf(R.err, sizeof R.err, "Could not open trace file %s", path.c_str()); return R.fail(GPH_EARG, "opening a replicate chain's trace file"); }
      trace.push_back(f);
      R.trace_header(f);
    }
    return GPH_OK;
  }
  /* the tables of the C chains compared: one kernel, one host synchronisation */
  int compare(Run &R)
  {
    if (rows_at == S) return GPH_OK;
    std::vector<gph_engine *> all{R.E};
    all.insert(all.end(), G.E.begin(), G.E.end());
    int64_t got = 0;
    if (int rc = gph_engine_clades_compare(all.data(), C, F, rows.data(), Q, &got)) return R.fail(rc, "gph_engine_clades_compare");
    rows_at = S;
    return GPH_OK;
  }
  void summary(double &mean, double &mx) const
  {
    double sum = 0.0;
    mx = 0.0;
    for (int64_t q = 0; q < Q; q++) { sum = sum + rows[(size_t)q * 6]; mx = rows[(size_t)q * 6] > mx ? rows[(size_t)q * 6] : mx; }
    mean = Q > 0 ? sum / (double)Q : 0.0;
  }
  int say(Run &R)
  {
    if (int rc = compare(R)) return rc;
    double mean, mx;
    summary(mean, mx);
    if (R.lead) { printf("Replicates: sample %lld: ASDSF mean %.10g max %.10g over %lld loci\n", (long long)S, mean, mx, (long long)Q); fflush(stdout); }
    return GPH_OK;
  }
  /* a sample point, behind chain 0's trace line and the outputs' samples */
  int sample(Run &R, int it)
  {
    for (int c = 0; c < C; c++) {
      double logL = 0, dataL = 0;
      R.trace_kept(G.all[(size_t)c], vals.data(), x[(size_t)c], logL, dataL);
      if (c > 0) R.trace_values(trace[(size_t)c - 1], it, vals.data(), logL, dataL);
      if (clades && c > 0)
        if (int rc = gph_engine_clades_sample(G.E[(size_t)c - 1])) return R.fail(rc, "gph_engine_clades_sample of a replicate chain");
    }
    S++;
    return every > 0 && S % every == 0 ? say(R) : GPH_OK;
  }
  /* behind the last iteration, while the chains are still there: the other traces are complete, the last comparison is taken */
  int finish(Run &R)
  {
    int bad = 0;
    for (FILE *&f : trace) { bad |= ferror(f) | fclose(f); f = nullptr; }
    if (bad) return R.fail(GPH_EARG, "writing a replicate chain's trace file");
    if (!clades || S < 1) return GPH_OK;
    if (every > 0 && rows_at != S) return say(R);
    return compare(R);
  }
  /* the two tables, at the end of a run that succeeded */
  int write(Run &R) const
  {
    if (clades && S >= 1) {
      const std::string path = rep_path(R.o.replicates_prefix, ".asdsf.tsv");
      FILE *f = fopen(path.c_str(), "w");
      if (!f) { snprintf(R.err, sizeof R.err, "Could not open %s", path.c_str()); return R.fail(GPH_EARG, "writing the ASDSF table"); }
      fprintf(f, "locus\tname\tsamples\tasdsf\tmaxSd\tcompared\tdistinct\tshared\tdropped\n");
      for (int64_t q = 0; q < Q; q++) {
        const double *r = rows.data() + (size_t)q * 6;
        const char *nm = gph_loci_name(R.LC, clades->sel[(size_t)q]);
        fprintf(f, "%d\t%s\t%d\t%.10g\t%.10g\t%d\t%d\t%d\t%d\n", (int)clades->sel[(size_t)q], nm ? nm : "", (int)S, r[0], r[1], (int)r[2], (int)r[3], (int)r[4],
                (int)r[5]);
      }
      double mean, mx;
      summary(mean, mx);
      fprintf(f, "# chains %d minfreq %.10g loci %lld meanAsdsf %.10g maxAsdsf %.10g\n", C, F, (long long)Q, mean, mx);
      const int rcc = ferror(f) | fclose(f);
      if (rcc) { unlink(path.c_str()); return R.fail(GPH_EARG, "writing the ASDSF table"); }
    }
    const std::string path = rep_path(R.o.replicates_prefix, ".psrf.tsv");
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { snprintf(R.err, sizeof R.err, "Could not open %s", path.c_str()); return R.fail(GPH_EARG, "writing the PSRF table"); }
    fprintf(f, "param\tmean\tsdWithin\tsdBetween\tpsrf\n");
    const std::vector<std::string> names = R.trace_columns();
    std::vector<double> col((size_t)C * (size_t)(S > 0 ? S : 1));
    double worst = 0.0;
    for (int i = 0; i < ncol && S >= 2; i++) {
      for (int c = 0; c < C; c++)
        for (int64_t s = 0; s < S; s++) col[(size_t)c * S + s] = x[(size_t)c][(size_t)s * ncol + i];
      double out[4];
      if (int rc = gph_psrf(col.data(), C, S, out)) { fclose(f); unlink(path.c_str()); return R.fail(rc, "gph_psrf"); }
      fprintf(f, "%s\t%.10g\t%.10g\t%.10g\t%.10g\n", names[(size_t)i].c_str(), out[0], out[1], out[2], out[3]);
      worst = out[3] > worst ? out[3] : worst;
    }
    fprintf(f, "# chains %d samples %lld maxPsrf %.10g\n", C, (long long)S, worst);
    const int rcc = ferror(f) | fclose(f);
    if (rcc) { unlink(path.c_str()); return R.fail(GPH_EARG, "writing the PSRF table"); }
    return GPH_OK;
  }
};
