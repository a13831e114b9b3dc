// gph_textjoin.h -- the eight outputs that travel through text parts (gph_textparts.h): what each format's lines mean
// once the last rank is done (gph_run_finish), and nothing else: its header line, which tag goes to which file, its summary
// and its line on stdout.  The parts' writers are the outputs of a run (gph_program.cpp, gph_*_run.h).
//
// This header DEFINES the sixteen gph_<name>_write / _discard entry points: one translation unit of a program includes it
// (gph_program.cpp in the library; a stand-alone program that wants the joiners without the engine includes it itself).
#ifndef GPH_TEXTJOIN_H
#define GPH_TEXTJOIN_H
#include "gph_textparts.h"
#include <algorithm>
#include <cmath>

namespace {
// clade tables: "C\t" + a row of PREFIX.clades.tsv, "T\t" + a row of PREFIX.consensus.tsv, locus by locus; no H line
struct ClJoin : TextJoin {
  ClJoin() : TextJoin(false) {}
  /* (the headers before any part is read; the formats with an H line print theirs when rank 0's has been read) */
  void start() override
  {
    fprintf(out[0], "locus\tname\tsamples\tdropped\tsize\tsupport\tmeanAge\tmembers\n");
    fprintf(out[1], "locus\tname\tsamples\tdistinct\tdropped\tresolved\ttree\n");
  }
  bool body(char *line, ssize_t, int) override
  {
    if (line[1] != '\t' || (line[0] != 'C' && line[0] != 'T')) return false;
    fputs(line + 2, out[line[0] == 'C' ? 0 : 1]);
    return true;
  }
};

// effective sample sizes: "H\t<samples>\t<level>\t<series>", rank 0's rows of PREFIX.ess.tsv as "P\t" + row (its summary
// line included), a rank's rows of PREFIX.locus-ess.tsv as "L\t<minEss, %a>\t" + row
const char *const ES_SERIES[6] = {"essDataLnL", "essGenLnL", "essTmrca", "essNumMigs", "essTopo", "essRate"};
struct EsJoin : TextJoin {
  long long S = -1, level = -1, M = -1;
  std::vector<std::pair<double, long long>> least;      /* minEss and locus of every row */
  std::string params;                                   /* the summary line of PREFIX.ess.tsv */
  EsJoin() : TextJoin(true) {}
  bool header(char *line, ssize_t, int) override
  {
    long long s = 0, j = 0, m = 0;
    if (!(sscanf(line, "H\t%lld\t%lld\t%lld", &s, &j, &m) == 3 && (S < 0 || (s == S && j == level && m == M)) && m >= 5 && m <= 6)) return false;
    if (S >= 0) return true;
    S = s; level = j; M = m;
    fprintf(out[0], "param\tsamples\tmean\tsd\tessBatch\tessAcf\ttauAcf\ttruncated\n");
    fprintf(out[1], "locus\tname\tsamples");
    for (int k = 0; k < M; k++) fprintf(out[1], "\t%s", ES_SERIES[k]);
    fprintf(out[1], "\ttopoChanges\tminEss\n");
    return true;
  }
  bool body(char *line, ssize_t len, int r) override
  {
    if (line[1] != '\t' || !(line[0] == 'L' || (line[0] == 'P' && r == 0))) return false;
    if (line[0] == 'P') {
      fputs(line + 2, out[0]);
      if (line[2] == '#') params.assign(line + 4, (size_t)len - 5);
      return true;
    }
    char *end = nullptr;
    const double v = strtod(line + 2, &end);
    if (!end || *end != '\t') return false;
    least.emplace_back(v, atoll(end + 1));
    fputs(end + 1, out[1]);
    return true;
  }
  void summary() override
  {
    std::vector<double> v;
    double lo = 0.0;
    long long lo_at = -1;
    for (const auto &p : least) { v.push_back(p.first); if (lo_at < 0 || p.first < lo) { lo = p.first; lo_at = p.second; } }
    std::sort(v.begin(), v.end());
    const size_t Q = v.size();
    const double median = Q == 0 ? 0.0 : Q % 2 ? v[Q / 2] : (v[Q / 2 - 1] + v[Q / 2]) / 2.0;
    char loci[256];
    snprintf(loci, sizeof loci, "loci %lld level %lld batch %lld medianMinEss %.10g minMinEss %.10g (locus %lld)", (long long)Q, level, 1ll << level, median, lo, lo_at);
    fprintf(out[1], "# %s\n", loci);
    printf("ESS: %s; %s\n", params.c_str(), loci);
    fflush(stdout);
  }
};

// the names behind the numbers of an H line: "\t<name>" each, to the end of the line
std::vector<std::string> tab_fields(const char *from, size_t bytes)
{
  std::vector<std::string> v;
  const std::string rest(from, bytes);
  for (size_t at = 0; at < rest.size() && rest[at] == '\t';) {
    const size_t to = std::min(rest.find('\t', at + 1), rest.size());
    v.push_back(rest.substr(at + 1, to - at - 1));
    at = to;
  }
  return v;
}

// predictive checks: "H\t<samples>\t<statistics>\t<seed>" + "\t<name>" per statistic, a rank's rows of PREFIX.predictive.tsv
// as "L\t<minP, %a>\t" + row, its observed totals as "O" + "\t<u64>" per statistic, its per-sample rows as R lines; the L
// rows are concatenated in rank order, the O and R lines added statistic by statistic
struct PdJoin : TextJoin {
  long long S = -1, C = -1, Q = 0, lo_at = -1;
  unsigned long long seed = 0;
  double lo = 0.0;
  std::vector<std::string> names;
  std::vector<unsigned long long> observed;             /* [C] */
  TextRows rows;
  PdJoin() : TextJoin(true) {}
  bool header(char *line, ssize_t len, int) override
  {
    long long s = 0, c = 0;
    unsigned long long sd = 0;
    int used = 0;
    if (!(sscanf(line, "H\t%lld\t%lld\t%llu%n", &s, &c, &sd, &used) == 3 && (S < 0 || (s == S && c == C && sd == seed)) && c >= 1 && line[len - 1] == '\n')) return false;
    if (S >= 0) return true;
    S = s; C = c; seed = sd;
    names = tab_fields(line + used, (size_t)len - used - 1);
    if ((long long)names.size() != C) return false;
    observed.assign((size_t)C, 0);
    rows.shape(S, C);
    fprintf(out[0], "locus\tname\tsamples\tsites");
    for (const std::string &nm : names) fprintf(out[0], "\tobs_%s\tmean_%s\tsd_%s\tp_%s", nm.c_str(), nm.c_str(), nm.c_str(), nm.c_str());
    fprintf(out[0], "\tminP\tstat\n");
    return true;
  }
  bool body(char *line, ssize_t, int r) override
  {
    if (line[0] == 'O') return TextRows::numbers(line + 1, C, observed.data());
    if (line[1] != '\t') return false;
    if (line[0] == 'R') return rows.row(line, r);
    if (line[0] != 'L') return false;
    char *end = nullptr;
    const double v = strtod(line + 2, &end);
    if (!end || *end != '\t') return false;
    if (lo_at < 0 || v < lo) { lo = v; lo_at = atoll(end + 1); }
    Q++;
    fputs(end + 1, out[0]);
    return true;
  }
  bool rank_done() override { return rows.rank_done(); }
  void summary() override
  {
    fprintf(out[0], "# loci %lld samples %lld seed %llu minMinP %.10g (locus %lld)\n", Q, S, seed, lo, lo_at);
    fprintf(out[1], "iter");
    for (const std::string &nm : names) fprintf(out[1], "\t%s", nm.c_str());
    fputc('\n', out[1]);
    rows.print(out[1]);
    std::string obs = "# observed", mean = "# mean", pl = "# p";
    char num[64];
    for (long long c = 0; c < C; c++) {
      unsigned long long sum = 0, gt = 0, eq = 0;
      for (long long s = 0; s < S; s++) {
        const unsigned long long t = rows.totals[(size_t)(s * C + c)];
        sum += t; gt += t > observed[(size_t)c]; eq += t == observed[(size_t)c];
      }
      snprintf(num, sizeof num, "\t%llu", observed[(size_t)c]); obs += num;
      snprintf(num, sizeof num, "\t%.10g", S > 0 ? (double)sum / (double)S : 0.0); mean += num;
      snprintf(num, sizeof num, "\t%.10g", S > 0 ? ((double)gt + (double)eq / 2) / (double)S : 0.0); pl += num;
    }
    fprintf(out[1], "%s\n%s\n%s\n# loci %lld samples %lld seed %llu\n", obs.c_str(), mean.c_str(), pl.c_str(), Q, S, seed);
    printf("Predictive: %s\n", pl.c_str() + 2);
    fflush(stdout);
  }
};

// triplet weights: "H\t<samples>\t<triples>" + "\t<P>,<Q>,<R>" (names) per triple, a rank's rows of PREFIX.triplets.tsv as
// "L\t" + row, its per-sample rows as R lines; the L rows are concatenated in rank order, the R lines added slot by slot
struct TrJoin : TextJoin {
  long long S = -1, T = -1, rowsL = 0;
  std::vector<std::string> names;                       /* [T][3] */
  TextRows rows;                                        /* [sample][3 T] */
  TrJoin() : TextJoin(true) {}
  bool header(char *line, ssize_t len, int) override
  {
    long long s = 0, t = 0;
    int used = 0;
    if (!(sscanf(line, "H\t%lld\t%lld%n", &s, &t, &used) == 2 && (S < 0 || (s == S && t == T)) && t >= 1 && s >= 0 && line[len - 1] == '\n')) return false;
    if (S >= 0) return true;
    S = s; T = t;
    for (const std::string &three : tab_fields(line + used, (size_t)len - used - 1)) {
      const size_t c1 = three.find(','), c2 = c1 == std::string::npos ? c1 : three.find(',', c1 + 1);
      if (c2 == std::string::npos) break;
      names.push_back(three.substr(0, c1)); names.push_back(three.substr(c1 + 1, c2 - c1 - 1)); names.push_back(three.substr(c2 + 1));
    }
    if ((long long)names.size() != 3 * T) return false;
    rows.shape(S, 3 * T);
    fprintf(out[0], "locus\tname\tsamples\tP\tQ\tR\tw_PQ|R\tw_PR|Q\tw_QR|P\tage_PQ|R\tage_PR|Q\tage_QR|P\ttop\n");
    return true;
  }
  bool body(char *line, ssize_t, int r) override
  {
    if (line[1] != '\t') return false;
    if (line[0] == 'R') return rows.row(line, r);
    if (line[0] != 'L') return false;
    fputs(line + 2, out[0]);
    rowsL++;
    return true;
  }
  bool rank_done() override { return rows.rank_done(); }
  void summary() override
  {
    const std::vector<unsigned long long> &totals = rows.totals;
    fprintf(out[1], "iter");
    for (long long k = 0; k < T; k++) {
      const std::string m[3] = {names[(size_t)(3 * k)], names[(size_t)(3 * k + 1)], names[(size_t)(3 * k + 2)]};
      for (int t = 0; t < 3; t++) fprintf(out[1], "\t%s", tr_label(m, t).c_str());
    }
    fputc('\n', out[1]);
    rows.print(out[1]);
    std::string most;
    double most_d = -1.0;
    for (long long k = 0; k < T; k++) {
      const std::string m[3] = {names[(size_t)(3 * k)], names[(size_t)(3 * k + 1)], names[(size_t)(3 * k + 2)]};
      unsigned long long sum[3] = {0, 0, 0};
      for (long long s = 0; s < S; s++)
        for (int t = 0; t < 3; t++) sum[t] += totals[(size_t)(s * 3 * T + 3 * k + t)];
      int major = 0;
      for (int t = 1; t < 3; t++) if (sum[t] > sum[major]) major = t;
      const int ma = major == 0 ? 1 : 0, mb = major == 2 ? 1 : 2;
      const double all = (double)sum[0] + (double)sum[1] + (double)sum[2];
      std::vector<double> D((size_t)S);
      double mean = 0.0, ss = 0.0;
      long long pos = 0;
      for (long long s = 0; s < S; s++) {
        const double a = (double)totals[(size_t)(s * 3 * T + 3 * k + ma)], b = (double)totals[(size_t)(s * 3 * T + 3 * k + mb)];
        D[(size_t)s] = a + b > 0.0 ? (a - b) / (a + b) : 0.0;
        mean = mean + D[(size_t)s];
        pos += D[(size_t)s] > 0.0;
      }
      mean = S > 0 ? mean / (double)S : 0.0;
      for (long long s = 0; s < S; s++) ss = ss + (D[(size_t)s] - mean) * (D[(size_t)s] - mean);
      const double sd = S > 1 ? sqrt(ss / (double)(S - 1)) : 0.0;
      char num[256];
      snprintf(num, sizeof num, " wMajor %.10g D %.10g sd %.10g pPos %.10g", all > 0.0 ? (double)sum[major] / all : 0.0, mean, sd, S > 0 ? (double)pos / (double)S : 0.0);
      const std::string text = m[0] + "," + m[1] + "," + m[2] + " major " + tr_label(m, major) + " minorA " + tr_label(m, ma) + " minorB " + tr_label(m, mb) + num;
      fprintf(out[1], "# asym %s\n", text.c_str());
      if (fabs(mean) > most_d) { most_d = fabs(mean); most = text; }
    }
    fprintf(out[1], "# loci %lld samples %lld triples %lld\n", T > 0 ? rowsL / T : 0, S, T);
    printf("Triplets: %s\n", most.c_str());
    fflush(stdout);
  }
};
// expected substitutions: "H\t<samples>\t<K>\t<n>" + "\t<name>" per population, then per leaf; a rank's rows of
// PREFIX.mutations.tsv as "L\t" + row; its per-sample rows as "R\t<iteration>" + "\t<u64>" per column: the bit pattern of the
// double.  The L rows are concatenated in rank order, the R lines added column by column in rank order (fp64, from 0.0).  The summary lines are formed
// from the values AS PRINTED ("%.10g" read back), so that they can be recomputed from the file's own rows
struct MuJoin : TextJoin {
  long long S = -1, K = -1, n = -1, C = 0, Q = 0, sample = 0;
  std::vector<std::string> names;                       /* [K] populations, then [n] leaves */
  std::vector<double> totals;                           /* [sample][C] */
  std::vector<long long> iters;
  MuJoin() : TextJoin(true) {}
  bool header(char *line, ssize_t len, int) override
  {
    long long s = 0, k = 0, m = 0;
    int used = 0;
    if (!(sscanf(line, "H\t%lld\t%lld\t%lld%n", &s, &k, &m, &used) == 3 && (S < 0 || (s == S && k == K && m == n)) && k >= 1 && m >= 2 && s >= 0 && line[len - 1] == '\n')) return false;
    if (S >= 0) return true;
    S = s; K = k; n = m; C = 2 * (K + n);
    names = tab_fields(line + used, (size_t)len - used - 1);
    if ((long long)names.size() != K + n) return false;
    totals.assign((size_t)(S * C), 0.0);
    iters.assign((size_t)S, 0);
    fprintf(out[0], "locus\tname\tsamples\tsites");
    for (long long p = 0; p < K; p++) fprintf(out[0], "\tmut_%s\texp_%s", names[(size_t)p].c_str(), names[(size_t)p].c_str());
    fprintf(out[0], "\trel\n");
    return true;
  }
  bool body(char *line, ssize_t, int r) override
  {
    if (line[1] != '\t') return false;
    if (line[0] == 'L') { fputs(line + 2, out[0]); Q++; return true; }
    if (line[0] != 'R' || sample >= S) return false;
    char *at = nullptr;
    const long long it = strtoll(line + 2, &at, 10);
    if (at == line + 2 || (r > 0 && iters[(size_t)sample] != it)) return false;
    for (long long c = 0; c < C; c++) {
      if (*at != '\t') return false;
      char *end = nullptr;
      const unsigned long long bits = strtoull(at + 1, &end, 10);
      if (end == at + 1) return false;
      double v;
      memcpy(&v, &bits, 8);
      double &t = totals[(size_t)(sample * C + c)];
      t = t + v;
      at = end;
    }
    if (*at != '\n') return false;
    iters[(size_t)sample++] = it;
    return true;
  }
  bool rank_done() override { const bool all = sample == S; sample = 0; return all; }
  static double printed(double v) { char num[64]; snprintf(num, sizeof num, "%.10g", v); return strtod(num, nullptr); }
  /* mean, sd and the share above 1 of mut / exp over the samples, columns cm and ce */
  std::string ratio_stats(long long cm, long long ce, double &mean) const
  {
    std::vector<double> x((size_t)S);
    double sum = 0.0, ss = 0.0;
    long long high = 0;
    for (long long s = 0; s < S; s++) {
      const double m = printed(totals[(size_t)(s * C + cm)]), e = printed(totals[(size_t)(s * C + ce)]);
      x[(size_t)s] = e != 0.0 ? m / e : 0.0;
      sum = sum + x[(size_t)s];
      high += x[(size_t)s] > 1.0;
    }
    mean = S > 0 ? sum / (double)S : 0.0;
    for (long long s = 0; s < S; s++) ss = ss + (x[(size_t)s] - mean) * (x[(size_t)s] - mean);
    char num[192];
    snprintf(num, sizeof num, "mean %.10g sd %.10g pHigh %.10g", mean, S > 1 ? sqrt(ss / (double)(S - 1)) : 0.0, S > 0 ? (double)high / (double)S : 0.0);
    return num;
  }
  void summary() override
  {
    fprintf(out[1], "iter");
    for (int w = 0; w < 2; w++)
      for (long long p = 0; p < K; p++) fprintf(out[1], "\t%s_%s", w ? "exp" : "mut", names[(size_t)p].c_str());
    for (int w = 0; w < 2; w++)
      for (long long i = 0; i < n; i++) fprintf(out[1], "\t%s_%s.%lld", w ? "expExt" : "mutExt", names[(size_t)(K + i)].c_str(), i);
    fputc('\n', out[1]);
    for (long long s = 0; s < S; s++) {
      fprintf(out[1], "%7d", (int)iters[(size_t)s]);
      for (long long c = 0; c < C; c++) fprintf(out[1], "\t%.10g", totals[(size_t)(s * C + c)]);
      fputc('\n', out[1]);
    }
    std::string most = "none";
    double most_d = -1.0;
    for (long long p = 0; p < K; p++) {
      double mean = 0.0;
      const std::string text = names[(size_t)p] + " " + ratio_stats(p, K + p, mean);
      fprintf(out[1], "# rel %s\n", text.c_str());
      if (mean > 0.0 && fabs(log(mean)) > most_d) { most_d = fabs(log(mean)); most = text; }
    }
    for (long long i = 0; i < n; i++) {
      double mean = 0.0;
      fprintf(out[1], "# ext %s.%lld %s\n", names[(size_t)(K + i)].c_str(), i, ratio_stats(2 * K + i, 2 * K + n + i, mean).c_str());
    }
    fprintf(out[1], "# loci %lld samples %lld\n", Q, S);
    printf("Mutations: %s\n", most.c_str());
    fflush(stdout);
  }
};
// replicate genealogies: "H\t<samples>\t<M>\t<C>\t<K>\t<B>\t<seed>" + "\t<name>" per genealogy statistic, then per site statistic; a
// rank's rows of PREFIX.simulate.tsv as "L\t<minP, %a>\t<failed>\t" + row, its observed site totals as "O" + "\t<u64>", its
// per-sample rows as R lines of 2 (K + B) + 4 + C numbers; the L rows are concatenated in rank order, the O and R lines added
struct SiJoin : TextJoin {
  long long S = -1, M = -1, C = -1, K = -1, B = -1, Q = 0, lo_at = -1, failed = 0;
  unsigned long long seed = 0;
  double lo = 0.0;
  std::vector<std::string> names;                       /* [M + C] */
  std::vector<unsigned long long> observed;             /* [C] */
  TextRows rows;
  SiJoin() : TextJoin(true) {}
  bool header(char *line, ssize_t len, int) override
  {
    long long s = 0, m = 0, c = 0, k = 0, b = 0;
    unsigned long long sd = 0;
    int used = 0;
    if (!(sscanf(line, "H\t%lld\t%lld\t%lld\t%lld\t%lld\t%llu%n", &s, &m, &c, &k, &b, &sd, &used) == 6 &&
          (S < 0 || (s == S && m == M && c == C && k == K && b == B && sd == seed)) && k >= 1 && b >= 0 && c >= 0 && m == 3 + k + b && line[len - 1] == '\n')) return false;
    if (S >= 0) return true;
    S = s; M = m; C = c; K = k; B = b; seed = sd;
    names = tab_fields(line + used, (size_t)len - used - 1);
    if ((long long)names.size() != M + C) return false;
    observed.assign((size_t)C + 1, 0);
    rows.shape(S, 2 * (K + B) + 4 + C);
    fprintf(out[0], "locus\tname\tsamples\tfailed\tsites");
    for (long long i = 0; i < M + C; i++) {
      const char *nm = names[(size_t)i].c_str();
      fprintf(out[0], "\t%s_%s\tmean_%s\tsd_%s\tp_%s", i < M ? "s" : "obs", nm, nm, nm, nm);
    }
    fprintf(out[0], "\tminP\tstat\n");
    return true;
  }
  bool body(char *line, ssize_t, int r) override
  {
    if (line[0] == 'O') return TextRows::numbers(line + 1, C, observed.data());
    if (line[1] != '\t') return false;
    if (line[0] == 'R') return rows.row(line, r);
    if (line[0] != 'L') return false;
    char *end = nullptr, *end2 = nullptr;
    const double v = strtod(line + 2, &end);
    if (!end || *end != '\t') return false;
    const long long f = strtoll(end + 1, &end2, 10);
    if (!end2 || end2 == end + 1 || *end2 != '\t') return false;
    if (f < S && (lo_at < 0 || v < lo)) { lo = v; lo_at = atoll(end2 + 1); }     /* (a locus without a replicate has no p) */
    failed += f;
    Q++;
    fputs(end2 + 1, out[0]);
    return true;
  }
  bool rank_done() override { return rows.rank_done(); }
  void summary() override
  {
    const long long KB = K + B, W = 2 * KB + 4 + C;
    fprintf(out[0], "# loci %lld samples %lld seed %llu failed %lld minMinP %.10g (locus %lld)\n", Q, S, seed, failed, lo, lo_at);
    fprintf(out[1], "iter");
    for (int w = 0; w < 2; w++)
      for (long long c = 0; c < KB; c++) fprintf(out[1], "\t%s.%s", w ? "r" : "s", names[(size_t)(3 + c)].c_str());
    for (int c = 0; c < 3; c++) fprintf(out[1], "\tgt.%s", names[(size_t)c].c_str());
    fprintf(out[1], "\tfailed");
    for (long long c = 0; c < C; c++) fprintf(out[1], "\tr.%s", names[(size_t)(M + c)].c_str());
    fputc('\n', out[1]);
    rows.print(out[1]);
    const std::vector<unsigned long long> &t = rows.totals;
    unsigned long long live = 0;                          /* replicates that did not fail, over the samples */
    for (long long s = 0; s < S; s++) live += (unsigned long long)Q - t[(size_t)(s * W + 2 * KB + 3)];
    std::string obs = "# observed", mean = "# mean", pl = "# p";
    char num[64];
    for (long long c = 0; c < W; c++) {
      unsigned long long sum = 0, gt = 0, eq = 0;
      const bool site = c > 2 * KB + 3, rep = c >= KB && c < 2 * KB;
      for (long long s = 0; s < S; s++) {
        const unsigned long long v = t[(size_t)(s * W + c)], against = site ? observed[(size_t)(c - 2 * KB - 4)] : rep ? t[(size_t)(s * W + c - KB)] : 0;
        sum += v; gt += v > against; eq += v == against;
      }
      if (site) { snprintf(num, sizeof num, "\t%llu", observed[(size_t)(c - 2 * KB - 4)]); obs += num; } else obs += "\t-";
      snprintf(num, sizeof num, "\t%.10g", S > 0 ? (double)sum / (double)S : 0.0); mean += num;
      if (site || rep) snprintf(num, sizeof num, "\t%.10g", S > 0 ? ((double)gt + (double)eq / 2) / (double)S : 0.0);
      else if (c >= 2 * KB && c < 2 * KB + 3) snprintf(num, sizeof num, "\t%.10g", live > 0 ? (double)sum / (double)live : 0.0);
      else snprintf(num, sizeof num, "\t-");
      pl += num;
    }
    fprintf(out[1], "%s\n%s\n%s\n# loci %lld samples %lld seed %llu\n", obs.c_str(), mean.c_str(), pl.c_str(), Q, S, seed);
    printf("Simulate: %s\n", pl.c_str() + 2);
    fflush(stdout);
  }
};
// pair times: "H\t<samples>\t<pairs>\t<bins>" + "\t<P>,<Q>,<m>" (names, leaf pairs) per pair + "\t<u64>" per edge (the double's
// 64-bit pattern); a rank's rows of PREFIX.pair-times.tsv as "L\t" + row, its per-sample rows as R lines of NP (B + 2) numbers;
// the L rows are concatenated in rank order, the R lines added number by number
struct PtJoin : TextJoin {
  long long S = -1, NP = -1, B = -1, rowsL = 0;
  std::vector<std::string> names;                       /* [NP][2] */
  std::vector<long long> m;                             /* [NP] leaf pairs */
  std::vector<double> edges;                            /* [B - 1] */
  TextRows rows;                                        /* [sample][NP (B + 2)] */
  PtJoin() : TextJoin(true) {}
  std::string label(long long k) const { return names[(size_t)(2 * k)] + "|" + names[(size_t)(2 * k + 1)]; }
  bool header(char *line, ssize_t len, int) override
  {
    long long s = 0, np = 0, b = 0;
    int used = 0;
    if (!(sscanf(line, "H\t%lld\t%lld\t%lld%n", &s, &np, &b, &used) == 3 && (S < 0 || (s == S && np == NP && b == B)) && np >= 1 && b >= 2 && b <= 128 && s >= 0 &&
          line[len - 1] == '\n')) return false;
    const std::vector<std::string> f = tab_fields(line + used, (size_t)len - used - 1);
    if ((long long)f.size() != np + b - 1) return false;
    std::vector<std::string> nm;
    std::vector<long long> lp;
    std::vector<double> ed;
    for (long long k = 0; k < np; k++) {
      const std::string &three = f[(size_t)k];
      const size_t c1 = three.find(','), c2 = c1 == std::string::npos ? c1 : three.find(',', c1 + 1);
      if (c2 == std::string::npos) return false;
      nm.push_back(three.substr(0, c1)); nm.push_back(three.substr(c1 + 1, c2 - c1 - 1));
      lp.push_back(atoll(three.c_str() + c2 + 1));
      if (lp.back() < 1) return false;
    }
    for (long long k = 0; k < b - 1; k++) {
      char *end = nullptr;
      const unsigned long long bits = strtoull(f[(size_t)(np + k)].c_str(), &end, 10);
      if (!end || *end != '\0' || end == f[(size_t)(np + k)].c_str()) return false;
      double v;
      memcpy(&v, &bits, 8);
      ed.push_back(v);
    }
    if (S >= 0) return nm == names && lp == m && ed.size() == edges.size() && memcmp(ed.data(), edges.data(), ed.size() * 8) == 0;
    S = s; NP = np; B = b; names = nm; m = lp; edges = ed;
    rows.shape(S, NP * (B + 2));
    fprintf(out[0], "locus\tname\tsamples\tP\tQ\tpairs\tmeanAge\tminAge\tpBelow\tfBelow\n");
    return true;
  }
  bool body(char *line, ssize_t, int r) override
  {
    if (line[1] != '\t') return false;
    if (line[0] == 'R') return rows.row(line, r);
    if (line[0] != 'L') return false;
    fputs(line + 2, out[0]);
    rowsL++;
    return true;
  }
  bool rank_done() override { return rows.rank_done(); }
  /* mean and sample sd (divisor S - 1; 0 for S = 1) of v, sums in sample order from 0.0 */
  static void mean_sd(const std::vector<double> &v, double &mean, double &sd)
  {
    const size_t n = v.size();
    double sum = 0.0, ss = 0.0;
    for (double x : v) sum = sum + x;
    mean = n > 0 ? sum / (double)n : 0.0;
    for (double x : v) ss = ss + (x - mean) * (x - mean);
    sd = n > 1 ? sqrt(ss / (double)(n - 1)) : 0.0;
  }
  void summary() override
  {
    const std::vector<unsigned long long> &t = rows.totals;
    const long long W = NP * (B + 2), Q = NP > 0 ? rowsL / NP : 0;
    fprintf(out[0], "# loci %lld samples %lld pairs %lld bins %lld\n", Q, S, NP, B);
    fprintf(out[1], "iter");
    for (long long k = 0; k < NP; k++)
      for (long long b = 0; b < B; b++) fprintf(out[1], "\t%s:%lld", label(k).c_str(), b);
    for (long long k = 0; k < NP; k++) fprintf(out[1], "\tbelow_%s", label(k).c_str());
    for (long long k = 0; k < NP; k++) fprintf(out[1], "\tloci_%s", label(k).c_str());
    fputc('\n', out[1]);
    rows.print(out[1]);
    fprintf(out[1], "# edges");
    for (double e : edges) fprintf(out[1], " %.17g", e);
    fputc('\n', out[1]);
    std::string most = "none";
    double most_b = -1.0;
    std::vector<double> v((size_t)S);
    char num[256];
    for (long long k = 0; k < NP; k++) {
      const double all = (double)Q * (double)m[(size_t)k];
      std::string cdf = "# cdf " + label(k), sds = "# sd " + label(k);
      for (long long b = 0; b < B; b++) {
        for (long long s = 0; s < S; s++) {
          unsigned long long cum = 0;
          for (long long j = 0; j <= b; j++) cum += t[(size_t)(s * W + k * B + j)];
          v[(size_t)s] = all > 0.0 ? (double)cum / all : 0.0;
        }
        double mean, sd;
        mean_sd(v, mean, sd);
        snprintf(num, sizeof num, " %.10g", mean); cdf += num;
        snprintf(num, sizeof num, " %.10g", sd); sds += num;
      }
      fprintf(out[1], "%s\n%s\n", cdf.c_str(), sds.c_str());
      double bm, bs, lm, ls;
      for (long long s = 0; s < S; s++) v[(size_t)s] = all > 0.0 ? (double)t[(size_t)(s * W + NP * B + k)] / all : 0.0;
      mean_sd(v, bm, bs);
      for (long long s = 0; s < S; s++) v[(size_t)s] = Q > 0 ? (double)t[(size_t)(s * W + NP * B + NP + k)] / (double)Q : 0.0;
      mean_sd(v, lm, ls);
      snprintf(num, sizeof num, " mean %.10g sd %.10g loci %.10g", bm, bs, lm);
      const std::string text = label(k) + num;
      fprintf(out[1], "# below %s\n", text.c_str());
      if (names[(size_t)(2 * k)] != names[(size_t)(2 * k + 1)] && bm > most_b) { most_b = bm; most = text; }
    }
    printf("PairTimes: %s\n", most.c_str());
    fflush(stdout);
  }
};
// site-frequency spectra: "H\t<samples>\t<slots>\t<groups>" + "\t<name>" per slot, then per group, + "\t<0|1>" per slot (1: a
// spectrum slot); a rank's rows of PREFIX.sfs.tsv as "L\t" + row; its observed totals as "O" + "\t<u64>" per slot; its per-sample
// rows as "R\t<iteration>" + "\t<u64>" per slot: the bit pattern of the double.  The L rows are concatenated in rank order, the O
// lines added, the R lines added slot by slot in rank order (fp64, from 0.0)
struct SfsJoin : TextJoin {
  long long S = -1, NS = -1, NG = -1, Q = 0, sample = 0;
  std::vector<std::string> names;                       /* [NS] slots, then [NG] groups, then [NS] flags */
  std::vector<unsigned long long> observed;             /* [NS] */
  std::vector<double> totals;                           /* [sample][NS] */
  std::vector<long long> iters;
  SfsJoin() : TextJoin(true) {}
  bool header(char *line, ssize_t len, int) override
  {
    long long s = 0, ns = 0, ng = 0;
    int used = 0;
    if (!(sscanf(line, "H\t%lld\t%lld\t%lld%n", &s, &ns, &ng, &used) == 3 && (S < 0 || (s == S && ns == NS && ng == NG)) && ns >= 1 && ng >= 1 && s >= 0 &&
          line[len - 1] == '\n')) return false;
    const std::vector<std::string> f = tab_fields(line + used, (size_t)len - used - 1);
    if ((long long)f.size() != 2 * ns + ng) return false;
    if (S >= 0) return f == names;
    S = s; NS = ns; NG = ng; names = f;
    observed.assign((size_t)NS, 0);
    totals.assign((size_t)(S * NS), 0.0);
    iters.assign((size_t)S, 0);
    fprintf(out[0], "locus\tname\tsamples\tsites");
    for (long long g = 0; g < NG; g++) fprintf(out[0], "\tuse_%s", names[(size_t)(NS + g)].c_str());
    for (long long k = 0; k < NS; k++) fprintf(out[0], "\tobs_%s\texp_%s", names[(size_t)k].c_str(), names[(size_t)k].c_str());
    fprintf(out[0], "\trel\n");
    return true;
  }
  bool body(char *line, ssize_t, int r) override
  {
    if (line[0] == 'O') return TextRows::numbers(line + 1, NS, observed.data());
    if (line[1] != '\t') return false;
    if (line[0] == 'L') { fputs(line + 2, out[0]); Q++; return true; }
    if (line[0] != 'R' || sample >= S) return false;
    char *at = nullptr;
    const long long it = strtoll(line + 2, &at, 10);
    if (at == line + 2 || (r > 0 && iters[(size_t)sample] != it)) return false;
    for (long long c = 0; c < NS; c++) {
      if (*at != '\t') return false;
      char *end = nullptr;
      const unsigned long long bits = strtoull(at + 1, &end, 10);
      if (end == at + 1) return false;
      double v;
      memcpy(&v, &bits, 8);
      double &t = totals[(size_t)(sample * NS + c)];
      t = t + v;
      at = end;
    }
    if (*at != '\n') return false;
    iters[(size_t)sample++] = it;
    return true;
  }
  bool rank_done() override { const bool all = sample == S; sample = 0; return all; }
  void summary() override
  {
    fprintf(out[0], "# loci %lld samples %lld slots %lld\n", Q, S, NS);
    fprintf(out[1], "iter");
    for (long long k = 0; k < NS; k++) fprintf(out[1], "\t%s", names[(size_t)k].c_str());
    fputc('\n', out[1]);
    for (long long s = 0; s < S; s++) {
      fprintf(out[1], "%7d", (int)iters[(size_t)s]);
      for (long long c = 0; c < NS; c++) fprintf(out[1], "\t%.10g", totals[(size_t)(s * NS + c)]);
      fputc('\n', out[1]);
    }
    std::string lines[5] = {"# observed", "# mean", "# sd", "# ratio", "# z"}, most = "none";
    double most_z = -1.0;
    char num[256];
    for (long long k = 0; k < NS; k++) {
      double sum = 0.0, ss = 0.0;
      for (long long s = 0; s < S; s++) sum = sum + totals[(size_t)(s * NS + k)];
      const double mean = S > 0 ? sum / (double)S : 0.0;
      for (long long s = 0; s < S; s++) { const double d = totals[(size_t)(s * NS + k)] - mean; ss = ss + d * d; }
      const double sd = S > 1 ? sqrt(ss / (double)(S - 1)) : 0.0, ob = (double)observed[(size_t)k];
      const double ratio = mean != 0.0 ? ob / mean : 0.0, den = sqrt(mean + sd * sd), z = den != 0.0 ? (ob - mean) / den : 0.0;
      snprintf(num, sizeof num, "\t%llu", observed[(size_t)k]); lines[0] += num;
      snprintf(num, sizeof num, "\t%.10g", mean); lines[1] += num;
      snprintf(num, sizeof num, "\t%.10g", sd); lines[2] += num;
      snprintf(num, sizeof num, "\t%.10g", ratio); lines[3] += num;
      snprintf(num, sizeof num, "\t%.10g", z); lines[4] += num;
      if (fabs(z) > most_z) {
        most_z = fabs(z);
        snprintf(num, sizeof num, " observed %llu mean %.10g ratio %.10g z %.10g", observed[(size_t)k], mean, ratio, z);
        most = names[(size_t)k] + num;
      }
    }
    for (const std::string &ln : lines) fprintf(out[1], "%s\n", ln.c_str());
    fprintf(out[1], "# loci %lld samples %lld\n", Q, S);
    printf("SFS: %s\n", most.c_str());
    fflush(stdout);
  }
};
}   // namespace

extern "C" int gph_sfs_write(const char *prefix, int32_t ranks) { SfsJoin J; return text_join(SF_TEXT, J, prefix, ranks); }
extern "C" int gph_sfs_discard(const char *prefix, int32_t ranks) { return text_discard(SF_TEXT, prefix, ranks); }
extern "C" int gph_pair_times_write(const char *prefix, int32_t ranks) { PtJoin J; return text_join(PT_TEXT, J, prefix, ranks); }
extern "C" int gph_pair_times_discard(const char *prefix, int32_t ranks) { return text_discard(PT_TEXT, prefix, ranks); }
extern "C" int gph_simulate_write(const char *prefix, int32_t ranks) { SiJoin J; return text_join(SI_TEXT, J, prefix, ranks); }
extern "C" int gph_simulate_discard(const char *prefix, int32_t ranks) { return text_discard(SI_TEXT, prefix, ranks); }
extern "C" int gph_clades_write(const char *prefix, int32_t ranks) { ClJoin J; return text_join(CL_TEXT, J, prefix, ranks); }
extern "C" int gph_ess_write(const char *prefix, int32_t ranks) { EsJoin J; return text_join(ES_TEXT, J, prefix, ranks); }
extern "C" int gph_predictive_write(const char *prefix, int32_t ranks) { PdJoin J; return text_join(PD_TEXT, J, prefix, ranks); }
extern "C" int gph_triplets_write(const char *prefix, int32_t ranks) { TrJoin J; return text_join(TR_TEXT, J, prefix, ranks); }
extern "C" int gph_mutations_write(const char *prefix, int32_t ranks) { MuJoin J; return text_join(MU_TEXT, J, prefix, ranks); }
extern "C" int gph_clades_discard(const char *prefix, int32_t ranks) { return text_discard(CL_TEXT, prefix, ranks); }
extern "C" int gph_ess_discard(const char *prefix, int32_t ranks) { return text_discard(ES_TEXT, prefix, ranks); }
extern "C" int gph_predictive_discard(const char *prefix, int32_t ranks) { return text_discard(PD_TEXT, prefix, ranks); }
extern "C" int gph_triplets_discard(const char *prefix, int32_t ranks) { return text_discard(TR_TEXT, prefix, ranks); }
extern "C" int gph_mutations_discard(const char *prefix, int32_t ranks) { return text_discard(MU_TEXT, prefix, ranks); }
#endif
