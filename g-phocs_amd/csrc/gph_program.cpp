// gph_program.cpp -- the reference's main() + the trace-file side of performMCMC
// (GPhoCS.c:84-238, 1232-1330, 1763-1769) over the engine: same control file, same sequence
// file, same trace file.  Everything per-locus runs on the MI355X engine; there is no CPU path.
#include "../../include/gphocs_hip.h"
#include "gph_textjoin.h"
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <cstddef>
#include <initializer_list>
#include <limits>
#include <memory>
#include <string>
#include <vector>
#include <unistd.h>

namespace {
// one step of the find-finetunes search for one step size (GPhoCS.c:1896-2180, the same block per proposal
// type): bisection on [min, max] towards 35 % +- 5 % acceptance
struct Finetune {
  double v, lo = 0.0, hi = 10.0;   /* finetuneMins / finetuneMaxes, MAX_FINETUNE = 10 (GPhoCS.h:21-24) */
  void adjust(double pct)
  {
    const double TARGET = 35, RANGE = 5, RES = 0.0000001, MAXF = 10;
    if (pct > TARGET + RANGE) {
      lo = v;
      if (hi - lo < RES) {
        if (hi >= MAXF) hi = lo = MAXF;
        else hi *= 2.0;
      }
    } else if (pct < TARGET - RANGE) {
      hi = v;
      if (hi - lo < RES) lo /= 2.0;
    }
    v = 0.5 * (hi + lo);
  }
};
}   // namespace

// the per-locus summary table (`G-PhoCS-hip -l FILE`) from the raw accumulators of this rank's loci: one row per locus in
// sequence-file order, every derived value as the header comment of include/gphocs_hip.h and README.md define it
static int write_locus_summary(const std::string &path, bool header, const gph_control *C, const gph_config &cfg, const gph_loci *LC,
                               int64_t lb, int64_t nloc, int32_t ncol, int64_t samples, const std::vector<double> &raw, bool var)
{
  FILE *f = fopen(path.c_str(), "w");
  if (!f) { fprintf(stderr, "gphocs_hip: cannot open the locus summary file %s\n", path.c_str()); return GPH_EARG; }
  const int K = cfg.K, B = cfg.B;
  if (header) {
    fprintf(f, "locus\tname\tsamples\tdataLnL\tdataLnL_sd\tgenLnL\tgenLnL_sd\ttmrca\ttmrca_sd");
    for (int b = 0; b < B; b++) {
      const char *src = gph_control_pop_name(C, cfg.bandSrc[b]), *tgt = gph_control_pop_name(C, cfg.bandTgt[b]);
      fprintf(f, "\tmig_%s->%s\tpmig_%s->%s", src, tgt, src, tgt);
    }
    for (int p = 0; p < K; p++) fprintf(f, "\tcoal_%s", gph_control_pop_name(C, p));
    if (var) fprintf(f, "\trate\trate_sd");
    fprintf(f, "\n");
  }
  const double S = (double)samples;
  auto moments = [&](const double *a) {
    const double mean = a[0] + a[1] / S;
    const double v = S > 1 ? (a[2] - a[1] * a[1] / S) / (S - 1) : 0.0;
    fprintf(f, "\t%.10g\t%.10g", mean, std::sqrt(v < 0.0 ? 0.0 : v));
  };
  for (int64_t i = 0; i < nloc; i++) {
    const double *a = raw.data() + (size_t)i * ncol;
    const char *nm = gph_loci_name(LC, lb + i);
    fprintf(f, "%lld\t%s\t%lld", (long long)(lb + i), nm ? nm : "", (long long)samples);
    moments(a + 0);
    moments(a + 3);
    moments(a + 6);
    for (int b = 0; b < B; b++) fprintf(f, "\t%.10g\t%.10g", a[9 + b] / S, a[9 + B + b] / S);
    for (int p = 0; p < K; p++) fprintf(f, "\t%.10g", a[9 + 2 * B + p] / S);
    if (var) moments(a + 9 + 2 * B + K);
    fprintf(f, "\n");
  }
  if (fclose(f) != 0) { fprintf(stderr, "gphocs_hip: writing the locus summary file %s failed\n", path.c_str()); return GPH_EARG; }
  return GPH_OK;
}

// ---- the part files of the statistics samplers.  Rank r's raw rows travel through a binary file PREFIX<suffix><r>: a header
// (magic, a few 32-bit integers, for coal stats the loci of all ranks as int64, the byte count of the names and the names,
// NUL-separated), one record per sample and, written when the rank closes its part, a trailer: the number of records (and,
// for ancestry, the number of bytes of text that sit between the records and the trailer).  A part without that trailer, or
// whose size does not match it, is refused.  (Clade tables, ESS, predictive checks and triplet weights travel as text
// parts instead: gph_textparts.h has their form, gph_textjoin.h what gph_run_finish makes of them.)
//   coal stats  PREFIX.coal.part<r>      n, K, doubles per row | L | n sample names as printed, K population names | row, logPrior
//   time slices PREFIX.slices.part<r>    S, K, B, doubles per row | K population names, B "src->tgt" band names | row
//   ancestry    PREFIX.ancestry.part<r>  n, B, integers per row | n sample names, B band names | iteration, row (32-bit integers)
namespace {
struct PartFormat {
  char magic[8];
  const char *suffix;
  int nh;                               /* header integers */
  bool (*valid)(const int32_t *h);
  bool has_L;                           /* an int64 follows them */
  int (*names)(const int32_t *h);       /* names expected */
  int (*len)(const int32_t *h);         /* elements per record */
  int kept;                             /* trailing elements of a record that are rank 0's (coal stats: logPrior), like element 0 */
  bool text;                            /* trailer: count, text bytes */
};
const PartFormat CS_PART = {{'G', 'P', 'H', 'C', 'S', '1', '\n', 0}, ".coal.part", 3, [](const int32_t *h) { return h[0] >= 2 && h[1] >= 1 && h[2] > 0; }, true,
                            [](const int32_t *h) { return h[0] + h[1]; }, [](const int32_t *h) { return h[2] + 1; }, 1, false};
const PartFormat TS_PART = {{'G', 'P', 'H', 'T', 'S', '1', '\n', 0}, ".slices.part", 4,
                            [](const int32_t *h) { return h[0] >= 1 && h[1] >= 1 && h[2] >= 0 && h[3] == 1 + 2 * h[0] * (h[1] + h[2]); }, false,
                            [](const int32_t *h) { return h[1] + h[2]; }, [](const int32_t *h) { return h[3]; }, 0, false};
const PartFormat AN_PART = {{'G', 'P', 'H', 'A', 'N', '1', '\n', 0}, ".ancestry.part", 3, [](const int32_t *h) { return h[0] >= 1 && h[1] >= 0 && h[2] == h[0] * (h[1] + 1); }, false,
                            [](const int32_t *h) { return h[0] + h[1]; }, [](const int32_t *h) { return h[2] + 1; }, 0, true};
std::string part_path(const PartFormat &F, const char *prefix, int r) { return std::string(prefix) + F.suffix + std::to_string(r); }
void remove_parts(const PartFormat &F, const char *prefix, int ranks) { for (int r = 0; r < ranks; r++) remove(part_path(F, prefix, r).c_str()); }

// rows of the device buffer when the caller names none: 64 samples, fewer when a row is large (the widest variant, 200
// leaves x 39 populations, has rows of 18.6 MB), so that the buffer -- and its host copy -- stay within 256 MB
int32_t cs_default_rows(int32_t row_doubles)
{
  const int64_t fit = ((int64_t)256 << 20) / ((int64_t)row_doubles * 8);
  return (int32_t)(fit < 1 ? 1 : fit > 64 ? 64 : fit);
}

// the parts of `ranks` ranks (records of T), read sample by sample: next() hands out the ranks' records added in rank
// order (counts added, sums added rank 0 first; element 0, the iteration, and the kept tail are rank 0's)
template <typename T> struct PartReader {
  const PartFormat &F;
  std::vector<FILE *> f;
  std::vector<long> text_at;
  std::vector<int64_t> text_bytes;
  int32_t hdr[4] = {0, 0, 0, 0};
  int len = 0;
  int64_t L = 0, samples = 0;
  std::vector<std::string> names;
  std::vector<T> tmp;
  explicit PartReader(const PartFormat &fmt) : F(fmt) {}
  ~PartReader() { for (FILE *x : f) if (x) fclose(x); }
  bool open(const char *prefix, int ranks)
  {
    for (int r = 0; r < ranks; r++) {
      const std::string path = part_path(F, prefix, r);
      FILE *x = fopen(path.c_str(), "rb");
      f.push_back(x);
      char magic[8];
      int32_t h[4] = {0, 0, 0, 0}, nbytes = 0;
      int64_t Lr = 0, tail[2] = {-1, 0};
      bool ok = x && fread(magic, 1, 8, x) == 8 && !memcmp(magic, F.magic, 8) && fread(h, 4, (size_t)F.nh, x) == (size_t)F.nh &&
                (!F.has_L || fread(&Lr, 8, 1, x) == 1) && fread(&nbytes, 4, 1, x) == 1 && nbytes >= 0 && F.valid(h);
      std::vector<std::string> nm;
      if (ok) {
        std::vector<char> buf((size_t)nbytes + 1, 0);
        ok = fread(buf.data(), 1, (size_t)nbytes, x) == (size_t)nbytes;
        for (size_t at = 0; ok && at < (size_t)nbytes; at += strlen(buf.data() + at) + 1) nm.push_back(buf.data() + at);
        ok = ok && (int)nm.size() == F.names(h);
      }
      long body = 0;
      if (ok) {
        /* header | count records | [text |] count [, text bytes] */
        const int tl = F.text ? 2 : 1;
        body = ftell(x);
        ok = body > 0 && fseek(x, -8 * tl, SEEK_END) == 0;
        const long end = ok ? ftell(x) : 0;
        ok = ok && fread(tail, 8, (size_t)tl, x) == (size_t)tl && tail[0] >= 0 && tail[1] >= 0 &&
             end - body == (long)(tail[0] * (int64_t)F.len(h) * (int64_t)sizeof(T) + tail[1]) && fseek(x, body, SEEK_SET) == 0;
      }
      if (!ok) { fprintf(stderr, "gphocs_hip: %s is missing, damaged or incomplete\n", path.c_str()); return false; }
      if (r == 0) { memcpy(hdr, h, sizeof hdr); len = F.len(h); L = Lr; samples = tail[0]; names = nm; }
      else if (memcmp(hdr, h, sizeof hdr) || tail[0] != samples) { fprintf(stderr, "gphocs_hip: %s does not match rank 0's part\n", path.c_str()); return false; }
      text_at.push_back(body + (long)(tail[0] * (int64_t)len * (int64_t)sizeof(T)));
      text_bytes.push_back(tail[1]);
    }
    tmp.resize((size_t)len);
    return true;
  }
  bool next(std::vector<T> &rec)
  {
    rec.resize((size_t)len);
    for (size_t r = 0; r < f.size(); r++) {
      std::vector<T> &into = r == 0 ? rec : tmp;
      if (fread(into.data(), sizeof(T), into.size(), f[r]) != into.size()) return false;
      if (r > 0) for (int c = 1; c < len - F.kept; c++) rec[c] = rec[c] + tmp[c];
    }
    return true;
  }
};

// every sample's combined record of a part set of doubles into out ([max_rows][*row_doubles]); out == nullptr: the shape only
int combined(const PartFormat &F, const char *prefix, int32_t ranks, double *out, int64_t max_rows, int64_t *rows, int32_t *row_doubles)
{
  if (!prefix || ranks < 1 || !rows || !row_doubles) return GPH_EARG;
  PartReader<double> R(F);
  if (!R.open(prefix, ranks)) return GPH_EARG;
  *rows = R.samples;
  *row_doubles = R.len;
  if (!out) return GPH_OK;
  if (max_rows < R.samples) return GPH_EARG;
  std::vector<double> rec;
  for (int64_t i = 0; i < R.samples; i++) {
    if (!R.next(rec)) return GPH_EARG;
    memcpy(out + (size_t)i * rec.size(), rec.data(), sizeof(double) * rec.size());
  }
  return GPH_OK;
}
}   // namespace

// ---- coalescent / sample-pair statistics (`G-PhoCS-hip -s PREFIX`)
extern "C" int gph_coal_stats_discard(const char *prefix, int32_t ranks)
{
  if (!prefix) return GPH_EARG;
  remove_parts(CS_PART, prefix, ranks);
  return GPH_OK;
}

extern "C" int gph_coal_stats_combined(const char *prefix, int32_t ranks, double *out, int64_t max_rows, int64_t *rows, int32_t *row_doubles)
{
  return combined(CS_PART, prefix, ranks, out, max_rows, rows, row_doubles);
}

extern "C" int gph_coal_stats_write(const char *prefix, int32_t ranks)
{
  if (!prefix || ranks < 1) return GPH_EARG;
  static const char *stat[3] = {"probCoal", "probFirstCoal", "meanCoal"};
  std::vector<std::string> paths;
  std::vector<FILE *> out;
  bool ok;
  {
    PartReader<double> R(CS_PART);
    ok = R.open(prefix, ranks);
    const int n = R.hdr[0], K = R.hdr[1], rd = R.hdr[2], npk = n * (n - 1) / 2 * K;
    /* every output file open at once (1 + 3 K of them), so that the parts are read once, sample by sample */
    if (ok) {
      paths.push_back(std::string(prefix) + ".coal.tsv");
      for (int pop = 0; pop < K; pop++)
        for (int st = 0; st < 3; st++) paths.push_back(std::string(prefix) + "." + R.names[n + pop] + "." + stat[st] + ".tsv");
      for (const std::string &p : paths) {
        FILE *x = fopen(p.c_str(), "w");
        if (!x) { fprintf(stderr, "gphocs_hip: cannot open %s\n", p.c_str()); ok = false; break; }
        out.push_back(x);
      }
    }
    if (ok) {
      /* headers: printCoalStats without partitions (GPhoCS.c:924-926) and the node-stats files' (GPhoCS.c:937-981) */
      fprintf(out[0], "iter\tcoalStat\tnumCoal\tmigStat\tnumMig\tlogPrior\tlogGenLikelihood\tlogDataLikelihood\n");
      for (int pop = 0; pop < K; pop++)
        for (int st = 0; st < 3; st++) {
          FILE *x = out[1 + 3 * pop + st];
          fprintf(x, "iter");
          for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) fprintf(x, "\t%s|%s|%s|%s", R.names[i].c_str(), R.names[j].c_str(), R.names[n + pop].c_str(), stat[st]);
          fprintf(x, "\n");
        }
      std::vector<int> pair_of((size_t)n * n, -1);
      for (int i = 0, p = 0; i < n; i++)
        for (int j = i + 1; j < n; j++, p++) pair_of[(size_t)i * n + j] = pair_of[(size_t)j * n + i] = p;
      const double Ld = (double)R.L;
      std::vector<double> rec;
      for (int64_t s = 0; s < R.samples && ok; s++) {
        if (!R.next(rec)) { fprintf(stderr, "gphocs_hip: a part of %s ended early\n", prefix); ok = false; break; }
        const double *a = rec.data();
        /* row formats of GPhoCS.c:990-999; all ordered pairs, the diagonal as 0, normalised as patch.c:2256-2266 (GPhoCS.c:1013-1036) */
        fprintf(out[0], "%7d", (int)a[0]);
        fprintf(out[0], "\t%8f\t%9d\t%8f\t%9d\t%8f\t%8f\t%8f\n", a[1], (int)a[2], a[3], (int)a[4], a[rd], a[5] + a[6], a[6]);
        for (int pop = 0; pop < K; pop++)
          for (int st = 0; st < 3; st++) {
            FILE *x = out[1 + 3 * pop + st];
            fprintf(x, "%7d", (int)a[0]);
            for (int i = 0; i < n; i++)
              for (int j = 0; j < n; j++) {
                const int p = pair_of[(size_t)i * n + j];
                double v = 0.0;
                if (p >= 0) {
                  const double cnt = a[7 + p * K + pop], first = a[7 + npk + p * K + pop], agesum = a[7 + 2 * npk + p * K + pop];
                  v = st == 0 ? cnt / Ld : st == 1 ? first / Ld : cnt > 0 ? agesum / cnt : 0.0;
                }
                fprintf(x, "\t%8f", v);
              }
            fprintf(x, "\n");
          }
      }
    }
    for (size_t i = 0; i < out.size(); i++)
      if ((ferror(out[i]) | fclose(out[i])) != 0) { fprintf(stderr, "gphocs_hip: writing %s failed\n", paths[i].c_str()); ok = false; }
  }
  gph_coal_stats_discard(prefix, ranks);
  if (!ok) for (size_t i = 0; i < out.size(); i++) remove(paths[i].c_str());
  return ok ? GPH_OK : GPH_EARG;
}


// ---- time-sliced statistics (`-s PREFIX --time-slices S`)
// the parts, and PREFIX.slices.tsv should it exist already (the run failed after it was written: a failed run leaves none)
extern "C" int gph_time_slices_discard(const char *prefix, int32_t ranks)
{
  if (!prefix) return GPH_EARG;
  remove_parts(TS_PART, prefix, ranks);
  unlink((std::string(prefix) + ".slices.tsv").c_str());   /* (a file only: whatever else sits under that name is not ours) */
  return GPH_OK;
}

extern "C" int gph_time_slices_combined(const char *prefix, int32_t ranks, double *out, int64_t max_rows, int64_t *rows, int32_t *row_doubles)
{
  return combined(TS_PART, prefix, ranks, out, max_rows, rows, row_doubles);
}

extern "C" int gph_time_slices_write(const char *prefix, int32_t ranks)
{
  if (!prefix || ranks < 1) return GPH_EARG;
  const std::string path = std::string(prefix) + ".slices.tsv";
  FILE *out = nullptr;
  bool ok;
  {
    PartReader<double> R(TS_PART);
    ok = R.open(prefix, ranks);
    const int S = R.hdr[0], K = R.hdr[1], B = R.hdr[2];
    if (ok && !(out = fopen(path.c_str(), "w"))) { fprintf(stderr, "gphocs_hip: cannot open %s\n", path.c_str()); ok = false; }
    if (ok) {
      /* the partition columns of printCoalStats (GPhoCS.c:927-935), then the bands' */
      fprintf(out, "iter");
      for (int q = 0; q < K + B; q++)
        for (int k = 1; k <= S; k++) {
          if (q < K) fprintf(out, "\tnumCoal_%s:%d\tdeltaT_%s:%d", R.names[q].c_str(), k, R.names[q].c_str(), k);
          else fprintf(out, "\tnumMig_%s:%d\tmigT_%s:%d", R.names[q].c_str(), k, R.names[q].c_str(), k);
        }
      fprintf(out, "\n");
      std::vector<double> rec;
      for (int64_t s = 0; s < R.samples && ok; s++) {
        if (!R.next(rec)) { fprintf(stderr, "gphocs_hip: a part of %s ended early\n", path.c_str()); ok = false; break; }
        fprintf(out, "%7d", (int)rec[0]);
        for (int c = 1; c < R.len; c += 2) fprintf(out, "\t%9d\t%8f", (int)rec[c], rec[c + 1]);   /* GPhoCS.c:1005 */
        fprintf(out, "\n");
      }
    }
    if (out && (ferror(out) | fclose(out)) != 0) { fprintf(stderr, "gphocs_hip: writing %s failed\n", path.c_str()); ok = false; }
  }
  remove_parts(TS_PART, prefix, ranks);
  if (!ok && out) remove(path.c_str());
  return ok ? GPH_OK : GPH_EARG;
}

// ---- migration ancestry (`--ancestry PREFIX`): the text behind a part's records is the rank's rows of the per-locus table
// the parts, and the two files should they exist already (the run failed after they were written: a failed run leaves none)
extern "C" int gph_ancestry_discard(const char *prefix, int32_t ranks)
{
  if (!prefix) return GPH_EARG;
  remove_parts(AN_PART, prefix, ranks);
  unlink((std::string(prefix) + ".loci.tsv").c_str());      /* (files only: whatever else sits under these names is not ours) */
  unlink((std::string(prefix) + ".samples.tsv").c_str());
  return GPH_OK;
}

extern "C" int gph_ancestry_write(const char *prefix, int32_t ranks)
{
  if (!prefix || ranks < 1) return GPH_EARG;
  const std::string paths[2] = {std::string(prefix) + ".loci.tsv", std::string(prefix) + ".samples.tsv"};
  FILE *out[2] = {nullptr, nullptr};
  bool ok;
  {
    PartReader<int32_t> R(AN_PART);
    ok = R.open(prefix, ranks);
    for (int k = 0; k < 2 && ok; k++)
      if (!(out[k] = fopen(paths[k].c_str(), "w"))) { fprintf(stderr, "gphocs_hip: cannot open %s\n", paths[k].c_str()); ok = false; }
    if (ok) {
      const int n = R.hdr[0], B = R.hdr[1];
      fprintf(out[1], "iter");
      for (int i = 0; i < n; i++) fprintf(out[1], "\tany_%s#%d", R.names[i].c_str(), i);
      for (int b = 0; b < B; b++)
        for (int i = 0; i < n; i++) fprintf(out[1], "\t%s|%s#%d", R.names[n + b].c_str(), R.names[i].c_str(), i);
      fprintf(out[1], "\n");
      std::vector<int32_t> rec;
      for (int64_t s = 0; s < R.samples && ok; s++) {
        if (!R.next(rec)) { fprintf(stderr, "gphocs_hip: a part of %s ended early\n", paths[1].c_str()); ok = false; break; }
        fprintf(out[1], "%7d", (int)rec[0]);
        for (int c = 1; c < R.len; c++) fprintf(out[1], "\t%9d", (int)rec[c]);
        fprintf(out[1], "\n");
      }
      fprintf(out[0], "locus\tname\tleaf\tsample\tsamples\tpAny");
      for (int b = 0; b < B; b++) fprintf(out[0], "\tp_%s\tage_%s", R.names[n + b].c_str(), R.names[n + b].c_str());
      fprintf(out[0], "\n");
      std::vector<char> buf(1 << 16);
      for (size_t r = 0; r < R.f.size() && ok; r++) {
        ok = fseek(R.f[r], R.text_at[r], SEEK_SET) == 0;
        for (int64_t left = R.text_bytes[r]; left > 0 && ok;) {
          const size_t want = left < (int64_t)buf.size() ? (size_t)left : buf.size();
          ok = fread(buf.data(), 1, want, R.f[r]) == want && fwrite(buf.data(), 1, want, out[0]) == want;
          left -= (int64_t)want;
        }
        if (!ok) fprintf(stderr, "gphocs_hip: copying the rows of %s failed\n", part_path(AN_PART, prefix, (int)r).c_str());
      }
    }
    for (int k = 0; k < 2; k++)
      if (out[k] && (ferror(out[k]) | fclose(out[k])) != 0) { fprintf(stderr, "gphocs_hip: writing %s failed\n", paths[k].c_str()); ok = false; }
  }
  remove_parts(AN_PART, prefix, ranks);
  if (!ok) for (int k = 0; k < 2; k++) if (out[k]) remove(paths[k].c_str());
  return ok ? GPH_OK : GPH_EARG;
}

// ---- sampled genealogies (`--gene-trees PREFIX`): records as plain arrays, one genealogy as a line of extended Newick, and
// the ranks' parts into PREFIX.trees.tsv
namespace {
// a name that may stand in a tree: no white space, none of the characters extended Newick reserves
bool gt_name_ok(const char *s)
{
  if (!s || !*s) return false;
  for (; *s; s++) if (isspace((unsigned char)*s) || strchr("()[],:;'=&", *s)) return false;
  return true;
}
std::string gt_len(double d)
{
  char buf[40];
  snprintf(buf, sizeof buf, "%.10g", d);
  return buf;
}
struct GtTree {
  int n, N;
  const double *age;
  const int32_t *father, *left, *right, *npop;
  int root, nm;
  const int32_t *mbr, *mband;
  const double *mage;
  const char *const *pops; int K;
  const char *const *bands; int B;
  const char *const *labels;
};
// sub(v) of the grammar in include/gphocs_hip.h, appended to out; false: the record is no tree
bool gt_sub(const GtTree &t, int v, int depth, std::string &out)
{
  if (v < 0 || v >= t.N || depth > t.N) return false;
  const int p = t.npop[v];
  if (p < 0 || p >= t.K) return false;
  std::vector<int> ms;                              /* the live migrations on the branch of v, by age; equal ages in `living` order */
  if (v != t.root)
    for (int k = 0; k < t.nm; k++) if (t.mbr[k] == v) ms.push_back(k);
  std::stable_sort(ms.begin(), ms.end(), [&](int a, int b) { return t.mage[a] < t.mage[b]; });
  out.append(ms.size(), '(');
  if (v < t.n) out += t.labels[v];
  else {
    out += '(';
    if (!gt_sub(t, t.left[v], depth + 1, out)) return false;
    out += ',';
    if (!gt_sub(t, t.right[v], depth + 1, out)) return false;
    out += ')';
  }
  out += "[&pop=";
  out += t.pops[p];
  out += ']';
  double a = t.age[v];
  for (int k : ms) {
    const int b = t.mband[k];
    if (b < 0 || b >= t.B) return false;
    out += ':';
    out += gt_len(t.mage[k] - a);
    out += ")[&mig=";
    out += t.bands[b];
    out += ']';
    a = t.mage[k];
  }
  if (v != t.root) {
    const int f = t.father[v];
    if (f < 0 || f >= t.N) return false;
    out += ':';
    out += gt_len(t.age[f] - a);
  }
  return true;
}
int gt_newick(const GtTree &t, std::string &out)
{
  for (int p = 0; p < t.K; p++) if (!gt_name_ok(t.pops[p])) { fprintf(stderr, "gphocs_hip: gene trees: the population name '%s' cannot stand in a tree (white space or one of ()[],:;'=&)\n", t.pops[p] ? t.pops[p] : ""); return GPH_EARG; }
  for (int i = 0; i < t.n; i++) if (!gt_name_ok(t.labels[i])) { fprintf(stderr, "gphocs_hip: gene trees: the leaf label '%s' cannot stand in a tree (white space or one of ()[],:;'=&)\n", t.labels[i] ? t.labels[i] : ""); return GPH_EARG; }
  for (int b = 0; b < t.B; b++) {
    const char *nm = t.bands[b], *arrow = nm ? strstr(nm, "->") : nullptr;
    const bool ok = arrow && gt_name_ok(std::string(nm, arrow).c_str()) && gt_name_ok(arrow + 2);
    if (!ok) { fprintf(stderr, "gphocs_hip: gene trees: the band name '%s' is not <src>-><tgt> of two names that can stand in a tree\n", nm ? nm : ""); return GPH_EARG; }
  }
  out.clear();
  if (t.n < 1 || t.nm < 0 || !gt_sub(t, t.root, 0, out)) return GPH_EARG;
  out += ';';
  return GPH_OK;
}
}   // namespace

extern "C" int gph_gene_tree_newick(int32_t n, const double *age, const int32_t *father, const int32_t *left, const int32_t *right,
                                    const int32_t *npop, int32_t root, int32_t num_migs, const int32_t *mig_branch, const int32_t *mig_band,
                                    const double *mig_age, const char *const *pop_names, int32_t K, const char *const *band_names, int32_t B,
                                    const char *const *leaf_labels, char *out, size_t out_cap, size_t *out_len)
{
  if (n < 1 || !age || !father || !left || !right || !npop || !pop_names || K < 1 || B < 0 || (B > 0 && !band_names) || !leaf_labels ||
      num_migs < 0 || (num_migs > 0 && (!mig_branch || !mig_band || !mig_age)))
    return GPH_EARG;
  const GtTree t = {n, 2 * n - 1, age, father, left, right, npop, root, num_migs, mig_branch, mig_band, mig_age, pop_names, K, band_names, B, leaf_labels};
  std::string text;
  const int rc = gt_newick(t, text);
  if (rc) return rc;
  if (out_len) *out_len = text.size();
  if (!out) return GPH_OK;
  if (out_cap < text.size() + 1) return 2;
  memcpy(out, text.c_str(), text.size() + 1);
  return GPH_OK;
}

// ---- clade tables (gph_engine_clades_*): the majority-rule consensus of one locus's table as text
namespace {
struct ClNode {
  const uint64_t *key;       // nullptr: the unannotated top level of a table that does not hold the root's clade
  uint64_t cnt;
  double age;
  int size, low, parent;     // leaves, smallest leaf, enclosing clade (-1: none)
  std::vector<int> kids;     // >= 0: clade, < 0: leaf -1 - i
};
int cl_popcount(const uint64_t *k, int W) { int c = 0; for (int w = 0; w < W; w++) c += __builtin_popcountll(k[w]); return c; }
int cl_low(const uint64_t *k, int W) { for (int w = 0; w < W; w++) if (k[w]) return 64 * w + __builtin_ctzll(k[w]); return -1; }
void cl_emit(const std::vector<ClNode> &nd, int v, const char *const *labels, int64_t S, std::string &out)
{
  if (v < 0) { out += labels[-1 - v]; return; }
  out += '(';
  for (size_t c = 0; c < nd[v].kids.size(); c++) {
    if (c) out += ',';
    cl_emit(nd, nd[v].kids[c], labels, S, out);
  }
  out += ')';
  if (nd[v].key) out += "[&support=" + gt_len((double)nd[v].cnt / (double)S) + ",age=" + gt_len(nd[v].age / (double)nd[v].cnt) + "]";
}
}   // namespace

extern "C" int gph_clades_consensus(int32_t n, int32_t slots, const uint64_t *entries, int64_t samples, const char *const *leaf_labels,
                                    char *out, size_t out_cap, size_t *out_len, int32_t *resolved)
{
  if (n < 1 || slots < 0 || (slots > 0 && !entries) || samples < 0 || !leaf_labels) return GPH_EARG;
  for (int i = 0; i < n; i++)
    if (!gt_name_ok(leaf_labels[i])) {
      fprintf(stderr, "gphocs_hip: clades: the leaf label '%s' cannot stand in a tree (white space or one of ()[],:;'=&)\n", leaf_labels[i] ? leaf_labels[i] : "");
      return GPH_EARG;
    }
  const int W = (n + 63) / 64, ew = W + 2;
  std::vector<ClNode> nd;
  for (int s = 0; s < slots; s++) {
    const uint64_t *en = entries + (size_t)s * ew;
    if (en[W] == 0 || 2 * en[W] <= (uint64_t)samples) continue;
    ClNode c;
    c.key = en; c.cnt = en[W]; memcpy(&c.age, en + W + 1, 8);
    c.size = cl_popcount(en, W); c.low = cl_low(en, W); c.parent = -1;
    bool inside = c.size >= 2;                                  /* no bit beyond the leaves, two leaves at least */
    for (int w = 0; w < W; w++) {
      const int top = n - 64 * w;
      if (top < 64 && (en[w] >> (top > 0 ? top : 0)) != 0) inside = false;
    }
    if (!inside) { fprintf(stderr, "gphocs_hip: clades: an entry of the table is no clade of %d leaves\n", (int)n); return GPH_EARG; }
    nd.push_back(c);
  }
  const int m = (int)nd.size();
  /* a set of clades is a tree iff every two are nested or disjoint */
  for (int a = 0; a < m; a++)
    for (int b = a + 1; b < m; b++) {
      bool meet = false, a_in_b = true, b_in_a = true;
      for (int w = 0; w < W; w++) {
        const uint64_t x = nd[a].key[w], y = nd[b].key[w];
        meet = meet || (x & y) != 0; a_in_b = a_in_b && (x & ~y) == 0; b_in_a = b_in_a && (y & ~x) == 0;
      }
      if ((meet && !a_in_b && !b_in_a) || (a_in_b && b_in_a)) {
        fprintf(stderr, "gphocs_hip: clades: two clades of the consensus are %s: no tree holds both\n", a_in_b && b_in_a ? "equal" : "neither nested nor disjoint");
        return GPH_EARG;
      }
      if (a_in_b && (nd[a].parent < 0 || nd[b].size < nd[nd[a].parent].size)) nd[a].parent = b;
      if (b_in_a && (nd[b].parent < 0 || nd[a].size < nd[nd[b].parent].size)) nd[b].parent = a;
    }
  int top = -1;
  for (int a = 0; a < m; a++) if (nd[a].size == n) top = a;
  if (top < 0) {
    ClNode c;
    c.key = nullptr; c.cnt = 0; c.age = 0.0; c.size = n; c.low = 0; c.parent = -1;
    nd.push_back(c);
    top = m;
    for (int a = 0; a < m; a++) if (nd[a].parent < 0) nd[a].parent = top;
  }
  for (int a = 0; a < m; a++) if (a != top) nd[nd[a].parent].kids.push_back(a);
  for (int i = 0; i < n; i++) {
    int best = top;
    for (int a = 0; a < m; a++)
      if (((nd[a].key[i / 64] >> (i % 64)) & 1) && nd[a].size < nd[best].size) best = a;
    nd[best].kids.push_back(-1 - i);
  }
  for (auto &c : nd)
    std::sort(c.kids.begin(), c.kids.end(), [&](int a, int b) { return (a < 0 ? -1 - a : nd[a].low) < (b < 0 ? -1 - b : nd[b].low); });
  std::string text;
  if (n == 1) text = leaf_labels[0];
  else cl_emit(nd, top, leaf_labels, samples, text);
  text += ';';
  if (resolved) *resolved = m;
  if (out_len) *out_len = text.size();
  if (!out) return GPH_OK;
  if (out_cap < text.size() + 1) return 2;
  memcpy(out, text.c_str(), text.size() + 1);
  return GPH_OK;
}

extern "C" int gph_gene_trees_decode(const void *records, int64_t count, int32_t record_bytes, const int32_t *off, int32_t N,
                                     double *age, int32_t *father, int32_t *left, int32_t *right, int32_t *npop, int32_t *root, int32_t *num_migs,
                                     double *dataLnL, double *genLnL, int32_t *mig_branch, int32_t *mig_band, int32_t *mig_spop, int32_t *mig_tpop,
                                     double *mig_age)
{
  if (count < 0 || (count > 0 && !records) || !off || N < 1 || record_bytes < 16 * N) return GPH_EARG;
  const int M = GPH_GT_MAX_MIGS;
  for (int64_t r = 0; r < count; r++) {
    const char *rec = (const char *)records + (size_t)r * record_bytes;
    for (int v = 0; v < N; v++) {
      const char *nd = rec + off[GPH_GT_O_NODES] + 16 * v;
      int16_t w[4];
      memcpy(w, nd + 8, 8);
      if (age) memcpy(age + (size_t)r * N + v, nd, 8);
      if (father) father[(size_t)r * N + v] = w[0];
      if (left) left[(size_t)r * N + v] = w[1];
      if (right) right[(size_t)r * N + v] = w[2];
      if (npop) npop[(size_t)r * N + v] = w[3];
    }
    int32_t rt, nm;
    memcpy(&rt, rec + off[GPH_GT_O_ROOT], 4);
    memcpy(&nm, rec + off[GPH_GT_O_NUM_MIGS], 4);
    nm = nm < 0 ? 0 : nm > M ? M : nm;
    if (root) root[r] = rt;
    if (num_migs) num_migs[r] = nm;
    if (dataLnL) memcpy(dataLnL + r, rec + off[GPH_GT_O_DATALNL], 8);
    if (genLnL) memcpy(genLnL + r, rec + off[GPH_GT_O_GENLNL], 8);
    for (int k = 0; k < M; k++) {
      int16_t m = -1, f[6] = {-1, -1, -1, -1, -1, -1};
      double a = 0.0;
      if (k < nm) memcpy(&m, rec + off[GPH_GT_O_LIVING] + 2 * k, 2);
      if (m >= 0 && m < M) {
        memcpy(f, rec + off[GPH_GT_O_MIG_I] + 12 * m, 12);
        memcpy(&a, rec + off[GPH_GT_O_MIG_AGE] + 8 * m, 8);
      }
      const size_t at = (size_t)r * M + k;
      if (mig_branch) mig_branch[at] = f[0];
      if (mig_band) mig_band[at] = f[1];
      if (mig_spop) mig_spop[at] = f[2];
      if (mig_tpop) mig_tpop[at] = f[3];
      if (mig_age) mig_age[at] = a;
    }
  }
  return GPH_OK;
}

// rank r's part PREFIX.trees.part<r>: magic | n, K, B, bytes of a record, the offsets inside one (int32) | selected loci of
// the rank (int64), their global indices (int64 each) | byte count of the names (int32), the names, NUL-separated: K
// populations, B bands, n leaf labels, one sequence-file name per selected locus | per sample: iteration (int32), the row |
// trailer, written when the rank closes its part: the number of samples (int64)
namespace {
const int GT_NH = 4 + GPH_GT_O_COUNT;
/* (written through open_part like the others; read by GtPart below, not by PartReader: its records are no sums) */
const PartFormat GT_PART = {{'G', 'P', 'H', 'G', 'T', '1', '\n', 0}, ".trees.part", GT_NH, nullptr, true, nullptr, nullptr, 0, false};
struct GtPart {
  FILE *f = nullptr;
  int32_t h[GT_NH] = {0};
  std::vector<int64_t> sel;
  std::vector<std::string> names;
  int64_t count = 0;
  ~GtPart() { if (f) fclose(f); }
  bool open(const std::string &path)
  {
    f = fopen(path.c_str(), "rb");
    char magic[8];
    int64_t nsel = -1;
    int32_t nbytes = -1;
    bool ok = f && fread(magic, 1, 8, f) == 8 && !memcmp(magic, GT_PART.magic, 8) && fread(h, 4, (size_t)GT_NH, f) == (size_t)GT_NH &&
              fread(&nsel, 8, 1, f) == 1 && nsel >= 0 && h[0] >= 1 && h[1] >= 1 && h[2] >= 0 && h[3] >= 16 * (2 * h[0] - 1);
    if (ok && nsel > 0) { sel.resize((size_t)nsel); ok = fread(sel.data(), 8, (size_t)nsel, f) == (size_t)nsel; }
    ok = ok && fread(&nbytes, 4, 1, f) == 1 && nbytes >= 0;
    if (ok) {
      std::vector<char> buf((size_t)nbytes + 1, 0);
      ok = fread(buf.data(), 1, (size_t)nbytes, f) == (size_t)nbytes;
      for (size_t at = 0; ok && at < (size_t)nbytes; at += strlen(buf.data() + at) + 1) names.push_back(buf.data() + at);
      ok = ok && (int64_t)names.size() == (int64_t)h[1] + h[2] + h[0] + nsel;
    }
    if (ok) {
      const long body = ftell(f);
      ok = body > 0 && fseek(f, -8, SEEK_END) == 0;
      const long end = ok ? ftell(f) : 0;
      ok = ok && fread(&count, 8, 1, f) == 1 && count >= 0 && end - body == (long)(count * (4 + nsel * (int64_t)h[3])) && fseek(f, body, SEEK_SET) == 0;
    }
    if (!ok) fprintf(stderr, "gphocs_hip: %s is missing, damaged or incomplete\n", path.c_str());
    return ok;
  }
};
}   // namespace

extern "C" int gph_gene_trees_discard(const char *prefix, int32_t ranks)
{
  if (!prefix) return GPH_EARG;
  remove_parts(GT_PART, prefix, ranks);
  unlink((std::string(prefix) + ".trees.tsv").c_str());     /* (a file only: whatever else sits under that name is not ours) */
  return GPH_OK;
}

extern "C" int gph_gene_trees_write(const char *prefix, int32_t ranks)
{
  if (!prefix || ranks < 1) return GPH_EARG;
  const std::string path = std::string(prefix) + ".trees.tsv";
  FILE *out = nullptr;
  bool ok = true;
  {
    std::vector<GtPart> P((size_t)ranks);
    for (int r = 0; r < ranks && ok; r++) {
      ok = P[(size_t)r].open(part_path(GT_PART, prefix, r));
      if (ok && r > 0 && (memcmp(P[0].h, P[(size_t)r].h, sizeof P[0].h) || P[0].count != P[(size_t)r].count)) {
        fprintf(stderr, "gphocs_hip: %s does not match rank 0's part\n", part_path(GT_PART, prefix, r).c_str());
        ok = false;
      }
    }
    if (ok && !(out = fopen(path.c_str(), "w"))) { fprintf(stderr, "gphocs_hip: cannot open %s\n", path.c_str()); ok = false; }
    if (ok) {
      const int n = P[0].h[0], K = P[0].h[1], B = P[0].h[2], rb = P[0].h[3], N = 2 * n - 1, M = GPH_GT_MAX_MIGS;
      const int32_t *off = P[0].h + 4;
      std::vector<const char *> pops, bands, labels;
      for (int p = 0; p < K; p++) pops.push_back(P[0].names[(size_t)p].c_str());
      for (int b = 0; b < B; b++) bands.push_back(P[0].names[(size_t)(K + b)].c_str());
      for (int i = 0; i < n; i++) labels.push_back(P[0].names[(size_t)(K + B + i)].c_str());
      std::vector<double> age((size_t)N), mage((size_t)M);
      std::vector<int32_t> fa((size_t)N), le((size_t)N), ri((size_t)N), np((size_t)N), mbr((size_t)M), mband((size_t)M);
      std::vector<char> row;
      std::string tree;
      fprintf(out, "iter\tlocus\tname\tdataLnL\tgenLnL\ttmrca\tnumMigs\ttree\n");
      for (int64_t s = 0; s < P[0].count && ok; s++) {
        int32_t it0 = 0;
        for (int r = 0; r < ranks && ok; r++) {
          GtPart &p = P[(size_t)r];
          int32_t it = 0;
          row.resize(p.sel.size() * (size_t)rb);
          ok = fread(&it, 4, 1, p.f) == 1 && (row.empty() || fread(row.data(), 1, row.size(), p.f) == row.size());
          if (r == 0) it0 = it;
          if (!ok || it != it0) { fprintf(stderr, "gphocs_hip: %s ended early or holds another sample than rank 0's part\n", part_path(GT_PART, prefix, r).c_str()); ok = false; break; }
          for (size_t q = 0; q < p.sel.size() && ok; q++) {
            int32_t root = 0, nm = 0;
            double dl = 0, gl = 0;
            gph_gene_trees_decode(row.data() + q * (size_t)rb, 1, rb, off, N, age.data(), fa.data(), le.data(), ri.data(), np.data(), &root, &nm,
                                  &dl, &gl, mbr.data(), mband.data(), nullptr, nullptr, mage.data());
            const GtTree t = {n, N, age.data(), fa.data(), le.data(), ri.data(), np.data(), root, nm, mbr.data(), mband.data(), mage.data(),
                              pops.data(), K, bands.data(), B, labels.data()};
            if (gt_newick(t, tree)) { fprintf(stderr, "gphocs_hip: gene trees: the record of locus %lld at iteration %d is no tree\n", (long long)p.sel[q], (int)it); ok = false; break; }
            fprintf(out, "%d\t%lld\t%s\t%.10g\t%.10g\t%.10g\t%d\t%s\n", (int)it, (long long)p.sel[q], p.names[(size_t)(K + B + n) + q].c_str(), dl, gl,
                    age[(size_t)root], (int)nm, tree.c_str());
          }
        }
      }
    }
    if (out && (ferror(out) | fclose(out)) != 0) { fprintf(stderr, "gphocs_hip: writing %s failed\n", path.c_str()); ok = false; }
  }
  remove_parts(GT_PART, prefix, ranks);
  if (!ok && out) remove(path.c_str());
  return ok ? GPH_OK : GPH_EARG;
}

// the selection of `--gene-trees-loci SPEC`: a comma list of i, i-j (both ends included) or i-j:step over 0 .. L - 1, sorted;
// an index named twice or beyond the loci is refused by name
static int gt_parse_spec(const char *spec, int64_t L, std::vector<int64_t> &sel, bool &all, const char *opt = "--gene-trees-loci")
{
  sel.clear();
  all = !spec || !strcmp(spec, "all");
  if (all) return GPH_OK;
  const char *p = spec;
  auto number = [&](int64_t &v) {
    if (!isdigit((unsigned char)*p)) return false;
    char *end;
    const long long x = strtoll(p, &end, 10);
    if (x < 0 || x > std::numeric_limits<int32_t>::max()) return false;
    v = x; p = end;
    return true;
  };
  while (true) {
    int64_t a, b, step = 1;
    if (!number(a)) break;
    b = a;
    if (*p == '-') { p++; if (!number(b) || b < a) break; if (*p == ':') { p++; if (!number(step) || step < 1) break; } }
    if (a >= L) { fprintf(stderr, "gphocs_hip: %s: locus %lld is beyond the %lld loci of the sequence file (indices are 0-based)\n", opt, (long long)a, (long long)L); return GPH_EARG; }
    for (int64_t g = a; g <= b; g += step) {
      if (g >= L) { fprintf(stderr, "gphocs_hip: %s: locus %lld is beyond the %lld loci of the sequence file (indices are 0-based)\n", opt, (long long)g, (long long)L); return GPH_EARG; }
      sel.push_back(g);
    }
    if (*p == ',') { p++; continue; }
    if (*p == 0) {
      std::sort(sel.begin(), sel.end());
      for (size_t k = 1; k < sel.size(); k++)
        if (sel[k] == sel[k - 1]) { fprintf(stderr, "gphocs_hip: %s: locus %lld is named twice\n", opt, (long long)sel[k]); return GPH_EARG; }
      return GPH_OK;
    }
    break;
  }
  fprintf(stderr, "gphocs_hip: %s: '%s' is not a comma list of i, i-j or i-j:step (0-based indices), nor 'all'\n", opt, spec);
  return GPH_EARG;
}

// the names a part's header carries, and writing one
namespace {
// the leaves' names as the statistics files print them: the second haploid of a diploid has no name of its own and takes
// the previous sample's, "NA" without one (GPhoCS.c:942-953)
std::vector<std::string> leaf_names(const gph_control *C, const gph_config &cfg)
{
  std::vector<std::string> v;
  for (int s = 0; s < cfg.n; s++) {
    const char *nm = gph_control_sample_name(C, s);
    if (!nm || !nm[0]) { const char *pv = s > 0 ? gph_control_sample_name(C, s - 1) : nullptr; nm = pv && pv[0] ? pv : "NA"; }
    v.push_back(nm);
  }
  return v;
}
std::vector<std::string> pop_names(const gph_control *C, const gph_config &cfg)
{
  std::vector<std::string> v;
  for (int p = 0; p < cfg.K; p++) v.push_back(gph_control_pop_name(C, p));
  return v;
}
std::vector<std::string> band_names(const gph_control *C, const gph_config &cfg)
{
  std::vector<std::string> v;
  for (int b = 0; b < cfg.B; b++) v.push_back(std::string(gph_control_pop_name(C, cfg.bandSrc[b])) + "->" + gph_control_pop_name(C, cfg.bandTgt[b]));
  return v;
}
// `got` fetched rows of n elements of esz bytes behind a part, row i with its extra value of xsz bytes, if any, in front of it
// (ancestry: the iteration) or behind it (coal stats: logPrior)
int write_rows(FILE *part, const void *rows, size_t esz, int32_t n, int32_t got, const void *extra, size_t xsz, bool in_front)
{
  for (int32_t i = 0; i < got; i++) {
    const char *x = extra ? (const char *)extra + xsz * i : nullptr;
    if (x && in_front && fwrite(x, xsz, 1, part) != 1) return GPH_EARG;
    if (n > 0 && fwrite((const char *)rows + esz * n * i, esz, (size_t)n, part) != (size_t)n) return GPH_EARG;
    if (x && !in_front && fwrite(x, xsz, 1, part) != 1) return GPH_EARG;
  }
  return fflush(part) == 0 ? GPH_OK : GPH_EARG;
}
}   // namespace

// ---- gph_run: the reference's main() over the engine.  A Run holds what the chain needs and frees it, every output of the program
// is an Output with the same few operations, the Log prints the acceptance table and searches the finetunes; run_chain strings them together.
namespace {
// the caller's options as this library knows them: behind the end of a shorter struct (an older caller) everything is 0 / NULL
bool take_options(const gph_run_options *in, gph_run_options &o)
{
  if (!in || in->size < offsetof(gph_run_options, comm) + sizeof in->comm || in->size > sizeof o) return false;
  memset(&o, 0, sizeof o);
  memcpy(&o, in, in->size);
  return true;
}

struct Run {
  const gph_run_options &o;
  const int32_t rank, world;
  const bool lead;               /* rank 0 talks and writes the trace file; every rank runs the same chain */
  gph_control *C = nullptr;
  gph_loci *LC = nullptr;
  gph_engine *E = nullptr;
  gph_mcmc *M = nullptr;         /* freed in this order: mcmc, engine, loci, control */
  gph_config cfg; gph_mcmc_config mc; gph_control_info info;   /* gph_control_get */
  int64_t L = 0, per = 0, lb = 0, le = 0;   /* loci of the sequence file, of a rank's block, this rank's block */
  const int64_t *offs; const uint8_t *leaf; const uint16_t *ph; const int32_t *cnt, *unph; const double *rates;   /* gph_loci_arrays */
  FILE *trace = nullptr;
  std::vector<double> vals;
  char err[512] = "";
  explicit Run(const gph_run_options &opt) : o(opt), rank(opt.rank), world(opt.world), lead(opt.rank == 0) {}
  ~Run()
  {
    if (trace) fclose(trace);
    release_device();
    if (LC) gph_loci_free(LC);
    if (C) gph_control_free(C);
  }
  void release_device()
  {
    if (M) gph_mcmc_destroy(M);
    if (E) gph_engine_destroy(E);
    M = nullptr;
    E = nullptr;
  }
  int fail(int code, const char *what)
  {
    fprintf(stderr, "gphocs_hip: %s failed (status %d)%s%s\n", what, code, err[0] ? ": " : "", err);
    return code;
  }
  int check(int rc, const char *what) { return rc ? fail(rc, what) : GPH_OK; }
  int read_control();
  int read_loci();
  int start_engine();
  int open_trace();
  std::vector<std::string> trace_columns() const;
  void trace_header(FILE *f) const;
  void trace_values(FILE *f, int it, const double *v, double logL, double dataL) const;
  void trace_line(int it);
  void trace_kept(gph_mcmc *m, double *v, std::vector<double> &x, double &logL, double &dataL) const;
};

int Run::read_control()
{
  int rc;
  if (lead) printf("Reading control settings from file %s...\n", o.ctl);
  if (lead && o.ctl2) printf("Reading control settings from secondary file %s...\n", o.ctl2);   /* GPhoCS.c:157-158 */
  if ((rc = gph_control_read(o.ctl, o.ctl2, &C))) return fail(rc, "reading the control file");
  gph_control_get(C, &cfg, &mc, &info);
  if (lead) printf("Done.\n");
  return GPH_OK;
}

// the seed, the sequence file with readSeqFile's progress text, and this rank's block of the loci
int Run::read_loci()
{
  int rc;
  if (mc.seed < 0) {
    if (world > 1) return fail(GPH_EARG, "random-seed must be given in the control file when several ranks run one chain");
    mc.seed = abs(2 * (int)time(NULL) + 1);   /* GPhoCS.c:188-191 */
  }
  if (o.verbose && lead) printf("\nRandom seed set to %d\n", mc.seed);

  auto t0 = std::chrono::steady_clock::now();
  if ((rc = gph_loci_read(C, nullptr, 0, &LC, err, sizeof err))) {
    /* a rejected rate file (locus-mut-rate FIXED): upstream's two lines (readRateFile, GPhoCS.c:491-579, and its caller :1149-1154) */
    if (info.mutRateMode == 2 && (strstr(err, "rate") || strstr(err, "Rate")) && lead) {
      fprintf(stderr, "Error: %s\n", err);
      if (!strstr(err, "Could not find")) fprintf(stderr, "Error: Unable to reading rate file '%s'. Aborting !!\n", info.rateFile);
    }
    return fail(rc, "reading the sequence file");
  }
  int32_t n = 0;
  gph_loci_arrays(LC, &L, &n, &offs, &leaf, &ph, &cnt, &rates, &unph);
  int64_t up = 0;
  for (int64_t g = 0; g < L; g++) up += unph[g];
  double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (lead) {   /* the progress text of readSeqFile (AlignmentProcessor.c:547, 562, 678-687) and main's blank line (GPhoCS.c:233) */
    printf("Reading sequence data...  %lld loci, as specified in sequence file %s.\n", (long long)L, info.seqFile);
    printf("Reading loci (.=100 loci): ");
    for (int64_t g = 1; g <= L; g++)
      if (g % 100 == 0) { printf("."); if (g % 1000 == 0) { printf(" "); if (g % 10000 == 0) printf("\n"); } }
    printf("\n");
    if (o.verbose) printf("Read %lld loci over %d samples: %lld patterns (%.2f per locus) -> %lld phased patterns (%.2f per locus) in %.2f s.\n",
                          (long long)L, n, (long long)up, (double)up / L, (long long)offs[L], (double)offs[L] / L, sec);
    printf("\n");
  }
  // loci shard in contiguous blocks of ceil(L / world) (OpenMP static scheduling of the reference, MultiCoreUtils.h:8)
  per = (L + world - 1) / world;
  lb = std::min<int64_t>(rank * per, L);
  le = std::min<int64_t>((rank + 1) * per, L);
  if ((int64_t)(world - 1) * per >= L) {
    /* the same test on every rank: the whole job stops here, nobody is left waiting in an exchange */
    if (lead) fprintf(stderr, "gphocs_hip: %d ranks over %lld loci in blocks of %lld leave the last rank(s) without loci -- use at most %lld ranks\n",
                      world, (long long)L, (long long)per, (long long)((L + per - 1) / per));
    return fail(GPH_EARG, "sharding the loci over the ranks");
  }
  return GPH_OK;
}

int Run::start_engine()
{
  int rc;
  cfg.L_total = L;
  cfg.locus_begin = lb;
  cfg.device = o.device;
  if ((rc = gph_engine_create(&cfg, &E))) return fail(rc, "gph_engine_create");
  if (world > 1 && o.allreduce && (rc = gph_engine_set_allreduce(E, o.allreduce, o.user))) return fail(rc, "gph_engine_set_allreduce");
  if (o.comm && (rc = gph_engine_set_comm(E, o.comm))) return fail(rc, "gph_engine_set_comm");
  /* pattern offsets are absolute indices into the pattern arrays: the shard is a window of the offset array */
  if ((rc = gph_engine_load_loci(E, le - lb, offs + lb, leaf, ph, cnt, info.mutRateMode == 2 ? rates + lb : nullptr))) return fail(rc, "gph_engine_load_loci");
  return check(gph_mcmc_create(E, &cfg, &mc, &M), "gph_mcmc_create");
}

// trace file header, GPhoCS.c:1273-1311
int Run::open_trace()
{
  trace = fopen(lead ? info.traceFile : "/dev/null", "w");
  if (!trace) { snprintf(err, sizeof err, "Could not open trace file %s", info.traceFile); return fail(GPH_EARG, "opening the trace file"); }
  trace_header(trace);
  vals.assign(mc.numParameters + 4, 0.0);
  return GPH_OK;
}

// the columns behind "Sample", as the header names them
std::vector<std::string> Run::trace_columns() const
{
  std::vector<std::string> c;
  const auto pop = [&](int p) { return std::string(gph_control_pop_name(C, p)); };
  for (int p = 0; p < cfg.K; p++) c.push_back("theta_" + pop(p));
  for (int p = cfg.Kc; p < cfg.K; p++) c.push_back("tau_" + pop(p));
  for (int b = 0; b < cfg.B; b++) c.push_back("m_" + pop(cfg.bandSrc[b]) + "->" + pop(cfg.bandTgt[b]));
  for (int p = 0; p < cfg.Kc; p++)
    if (mc.updateSampleAge[p] || mc.sampleAge[p] > 0.0) c.push_back("tau_" + pop(p));
  if (info.mutRateMode == 1) c.push_back("Variance-Mut");   /* GPhoCS.c:1311-1312 */
  c.push_back("Data-ld-ln");
  c.push_back("Full-ld-ln");
  return c;
}

void Run::trace_header(FILE *f) const
{
  fprintf(f, "Sample");
  for (const std::string &c : trace_columns()) fprintf(f, "\t%s", c.c_str());
  fprintf(f, "\n");
}

void Run::trace_values(FILE *f, int it, const double *v, double logL, double dataL) const   /* GPhoCS.c:1763-1769 */
{
  fprintf(f, "%d\t", it);
  for (int i = 0; i < mc.numParameters; i++) fprintf(f, "%8.5f\t", v[i] * mc.printFactors[i]);
  fprintf(f, "\t%.6f\t%.6f\n", logL, dataL);
  fflush(f);
}

void Run::trace_line(int it)
{
  double logL = 0, dataL = 0;
  gph_mcmc_param_vals(M, vals.data(), mc.numParameters);
  gph_mcmc_get_state(M, &logL, &dataL, nullptr, nullptr, nullptr);
  trace_values(trace, it, vals.data(), logL, dataL);
}

// what a trace line of chain m prints, kept before formatting (behind x: vals[i] * printFactors[i], then logL, then dataL; v:
// scratch of numParameters doubles) -- the replicate chains' PSRF and the ESS table read these
void Run::trace_kept(gph_mcmc *m, double *v, std::vector<double> &x, double &logL, double &dataL) const
{
  logL = dataL = 0;
  gph_mcmc_param_vals(m, v, mc.numParameters);
  gph_mcmc_get_state(m, &logL, &dataL, nullptr, nullptr, nullptr);
  for (int i = 0; i < mc.numParameters; i++) x.push_back(v[i] * mc.printFactors[i]);
  x.push_back(logL);
  x.push_back(dataL);
}

// ---- `--mc3`: the heated chains next to the run's own
#include "gph_mc3_run.h"

// ---- the outputs.  open: enable on the engine, take the shape, size the host buffer, open this rank's part and write its
// header; sample: at a trace line, and a flush when the buffer is full; close: the last flush, the trailer, the part closed;
// write / discard: what becomes of the ranks' parts once the last rank is done (gph_run_finish).
//   Part          this rank's binary part (coal stats, time slices, ancestry, gene trees)
//   Selected      an output over `--<name>-loci SPEC`: this rank's share of the selection, how it is handed to the engine, the
//                 message of an enable call that found the selection too large
//   TextOutput    a Selected whose part is text (gph_textparts.h): clades, ess, mutations and, through RowsOutput, predictive, triplets, simulate, pair times, sfs
//   RowsOutput    a TextOutput that also keeps per-sample rows: fetched when the device buffer is full, printed as R lines
struct Output {
  virtual ~Output() {}
  virtual int open(Run &R) = 0;
  virtual int sample(Run &R, int it) = 0;
  virtual int close(Run &R) = 0;
  virtual int write(int32_t) { return GPH_OK; }
  virtual void discard(int32_t) {}
};

// this rank's part file of one output, as the messages name it
struct Part {
  const std::string name;
  FILE *f = nullptr;
  int64_t written = 0;
  explicit Part(const char *nm) : name(nm) {}
  ~Part() { if (f) fclose(f); }
  /* open, the header written (L: the int64 of the formats that carry one; the gene-trees part: L selected loci and, behind it,
   * their indices) */
  int open(Run &R, const PartFormat &F, const char *prefix, const int32_t *hdr, int64_t L, const int64_t *sel,
           std::initializer_list<std::vector<std::string>> groups)
  {
    if (!(f = fopen(part_path(F, prefix, R.rank).c_str(), "wb"))) {
      snprintf(R.err, sizeof R.err, "Could not open %s", part_path(F, prefix, R.rank).c_str());
      return R.fail(GPH_EARG, ("opening the " + name + " part file").c_str());
    }
    std::string names;
    for (const std::vector<std::string> &v : groups)
      for (const std::string &nm : v) { names += nm; names.push_back('\0'); }
    const int32_t nbytes = (int32_t)names.size();
    fwrite(F.magic, 1, 8, f); fwrite(hdr, 4, (size_t)F.nh, f);
    if (F.has_L) fwrite(&L, 8, 1, f);
    if (sel && L > 0) fwrite(sel, 8, (size_t)L, f);
    fwrite(&nbytes, 4, 1, f);
    fwrite(names.data(), 1, names.size(), f);
    return GPH_OK;
  }
  int written_ok(Run &R, int rc) { return R.check(rc, ("writing the " + name + " part file").c_str()); }
  /* the filled rows of a device buffer behind the part: fetch(&got) brings them to `rows`, write_rows sets each with its
   * extra value; the one host synchronisation of an output */
  template <class Fetch> int flush(Run &R, Fetch fetch, const void *rows, size_t esz, int32_t n, const void *extra, size_t xsz, bool in_front)
  {
    int32_t got = 0;
    int rc = fetch(&got);
    if (!rc) rc = write_rows(f, rows, esz, n, got, extra, xsz, in_front);
    written += got;
    return written_ok(R, rc);
  }
  /* the trailer: records in this part (ancestry: and the bytes of text behind them) */
  int close(Run &R, int64_t text_bytes = -1)
  {
    const int64_t tail[2] = {written, text_bytes};
    const size_t nt = text_bytes < 0 ? 1 : 2;
    if (fwrite(tail, 8, nt, f) != nt) return written_ok(R, GPH_EARG);
    const int rcc = ferror(f) | fclose(f);
    f = nullptr;
    return R.check(rcc ? GPH_EARG : GPH_OK, ("closing the " + name + " part file").c_str());
  }
};

struct LocusSummary : Output {
  int32_t ncol = 0;
  int64_t samples = 0;
  std::vector<double> raw;
  int open(Run &R) override { return R.check(gph_engine_locus_summary_enable(R.E, 1), "gph_engine_locus_summary_enable"); }
  int sample(Run &R, int) override { return R.check(gph_engine_locus_summary_sample(R.E), "gph_engine_locus_summary_sample"); }
  int close(Run &R) override
  {
    gph_engine_locus_summary_columns(R.E, &ncol, &samples);
    raw.resize((size_t)ncol * (R.le - R.lb));
    return R.check(gph_engine_locus_summary_fetch(R.E, raw.data(), ncol, 0), "gph_engine_locus_summary_fetch");
  }
  /* one rank: the file itself; several: this rank's part, concatenated in rank order by the caller (rank 0's has the header) */
  int write_table(Run &R)
  {
    const std::string path = R.world > 1 ? std::string(R.o.locus_summary_path) + ".part" + std::to_string(R.rank) : std::string(R.o.locus_summary_path);
    return write_locus_summary(path, R.lead, R.C, R.cfg, R.LC, R.lb, R.le - R.lb, ncol, samples, raw, R.info.mutRateMode == 1);
  }
};

// coalescent / sample-pair statistics and, with slices > 0, the time-sliced statistics: one prefix, device buffers of as many
// rows that fill and are flushed together, logPrior behind every coal-stats row
struct CoalStats : Output {
  const char *prefix;
  int32_t capacity, slices, rd = 0, ts_rd = 0;
  Part cs{"coal-stats"}, ts{"time-slices"};
  std::vector<double> rows, prior, ts_rows, theta, age, mig;
  explicit CoalStats(const gph_run_options &o) : prefix(o.coal_stats_prefix), capacity(o.coal_stats_rows), slices(o.time_slices) {}
  static int validate(const gph_run_options &o)
  {
    const bool ok = o.time_slices == 0 || (o.time_slices > 0 && o.coal_stats_prefix);
    if (!ok) fprintf(stderr, "gphocs_hip: time slices need a coal-stats prefix\n");
    return ok ? GPH_OK : GPH_EARG;
  }
  int open(Run &R) override
  {
    int rc;
    const gph_config &cfg = R.cfg;
    theta.resize(cfg.K); age.resize(cfg.K); mig.resize(cfg.B > 0 ? cfg.B : 1);
    if (capacity <= 0) capacity = cs_default_rows(7 + 3 * (cfg.n * (cfg.n - 1) / 2) * cfg.K);
    if ((rc = gph_engine_coal_stats_enable(R.E, capacity))) return R.fail(rc, "gph_engine_coal_stats_enable");
    gph_engine_coal_stats_shape(R.E, &rd, nullptr, nullptr, nullptr);
    rows.resize((size_t)rd * capacity);
    const int32_t hdr[3] = {cfg.n, cfg.K, rd};
    if ((rc = cs.open(R, CS_PART, prefix, hdr, R.L, nullptr, {leaf_names(R.C, cfg), pop_names(R.C, cfg)})) || !slices) return rc;
    if ((rc = gph_engine_time_slices_enable(R.E, slices, capacity))) return R.fail(rc, "gph_engine_time_slices_enable");
    gph_engine_time_slices_shape(R.E, &ts_rd, nullptr, nullptr, nullptr, nullptr, nullptr);
    ts_rows.resize((size_t)ts_rd * capacity);
    const int32_t ts_hdr[4] = {slices, cfg.K, cfg.B, ts_rd};
    return ts.open(R, TS_PART, prefix, ts_hdr, 0, nullptr, {pop_names(R.C, cfg), band_names(R.C, cfg)});
  }
  /* logPrior of the parameters a trace line shows: what getLogPrior sums (GPhoCS.c:858-898) -- theta of every population,
   * tau of every ancestral one, the rate of every band, each under its gamma prior of the control file */
  double log_prior(Run &R)
  {
    const gph_config &cfg = R.cfg;
    const gph_mcmc_config &mc = R.mc;
    gph_mcmc_get_state(R.M, nullptr, nullptr, theta.data(), age.data(), mig.data());
    /* log density of a gamma(shape, rate) prior at x: shape ln(rate) - ln Gamma(shape) + (shape - 1) ln x - rate x */
    auto gamma_lpdf = [](double shape, double rate, double x) {
      return shape * std::log(rate) - std::lgamma(shape) + (shape - 1.0) * std::log(x) - rate * x;
    };
    double lp = 0.0;
    for (int p = 0; p < cfg.K; p++) lp += gamma_lpdf(mc.thetaAlpha[p], mc.thetaBeta[p], theta[p]);
    for (int p = cfg.Kc; p < cfg.K; p++) lp += gamma_lpdf(mc.ageAlpha[p], mc.ageBeta[p], age[p]);
    for (int b = 0; b < cfg.B; b++) lp += gamma_lpdf(mc.mrAlpha[b], mc.mrBeta[b], mig[b]);
    return lp;
  }
  /* (both buffers have `capacity` rows and fill together) */
  int flush(Run &R)
  {
    auto fetch = [&](int32_t *got) {
      const int rc = gph_engine_coal_stats_fetch(R.E, rows.data(), capacity, got);
      return rc ? rc : *got != (int32_t)prior.size() ? GPH_ESTATE : GPH_OK;
    };
    const int rc = cs.flush(R, fetch, rows.data(), sizeof(double), rd, prior.data(), sizeof(double), false);
    prior.clear();
    if (rc || !slices) return rc;
    return ts.flush(R, [&](int32_t *got) { return gph_engine_time_slices_fetch(R.E, ts_rows.data(), capacity, got); }, ts_rows.data(),
                    sizeof(double), ts_rd, nullptr, 0, false);
  }
  int sample(Run &R, int it) override
  {
    int rc;
    if ((rc = gph_engine_coal_stats_sample(R.E, it))) return R.fail(rc, "gph_engine_coal_stats_sample");
    if (slices && (rc = gph_engine_time_slices_sample(R.E, it))) return R.fail(rc, "gph_engine_time_slices_sample");
    prior.push_back(log_prior(R));
    return (int32_t)prior.size() < capacity ? GPH_OK : flush(R);
  }
  int close(Run &R) override
  {
    int rc;
    if ((rc = flush(R)) || (rc = cs.close(R)) || !slices) return rc;
    return ts.close(R);
  }
  /* (the slices file first; should the coal-stats files fail after it, one file is removed again, not 1 + 3 K) */
  int write(int32_t ranks) override { const int rc = slices ? gph_time_slices_write(prefix, ranks) : GPH_OK; return rc ? rc : gph_coal_stats_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_coal_stats_discard(prefix, ranks); if (slices) gph_time_slices_discard(prefix, ranks); }
};

// migration ancestry: accumulators and a device buffer of per-sample rows; the part's records each behind their iteration
struct Ancestry : Output {
  const char *prefix;
  int32_t capacity, held = 0, ncol = 0, ri = 0;
  Part part{"ancestry"};
  std::vector<int32_t> rows, iters;
  std::vector<std::string> names;
  explicit Ancestry(const gph_run_options &o) : prefix(o.ancestry_prefix), capacity(o.ancestry_rows) {}
  int open(Run &R) override
  {
    int rc;
    if (capacity <= 0) capacity = 64;
    if ((rc = gph_engine_ancestry_enable(R.E, capacity, 0))) return R.fail(rc, "gph_engine_ancestry_enable");
    gph_engine_ancestry_shape(R.E, &ncol, &ri, nullptr, nullptr);
    rows.resize((size_t)ri * capacity);
    iters.resize((size_t)capacity);
    names = leaf_names(R.C, R.cfg);
    const int32_t hdr[3] = {R.cfg.n, R.cfg.B, ri};
    return part.open(R, AN_PART, prefix, hdr, 0, nullptr, {names, band_names(R.C, R.cfg)});
  }
  int flush(Run &R)
  {
    held = 0;
    return part.flush(R, [&](int32_t *got) { return gph_engine_ancestry_fetch_rows(R.E, iters.data(), rows.data(), ri, capacity, got); },
                      rows.data(), 4, ri, iters.data(), 4, true);
  }
  int sample(Run &R, int it) override
  {
    const int rc = R.check(gph_engine_ancestry_sample(R.E, it), "gph_engine_ancestry_sample");
    return rc || ++held < capacity ? rc : flush(R);
  }
  /* this rank's rows of the per-locus table, as text behind its records */
  int close(Run &R) override
  {
    int rc;
    if ((rc = flush(R))) return rc;
    int64_t S = 0;
    gph_engine_ancestry_shape(R.E, nullptr, nullptr, &S, nullptr);
    std::vector<double> raw((size_t)ncol * (R.le - R.lb));
    if ((rc = gph_engine_ancestry_fetch_loci(R.E, raw.data(), ncol, 0))) return R.fail(rc, "gph_engine_ancestry_fetch_loci");
    const long text0 = ftell(part.f);
    const int n = R.cfg.n, B = R.cfg.B;
    const double Sd = (double)S;
    for (int64_t g = 0; g < R.le - R.lb; g++) {
      const double *a = raw.data() + (size_t)g * ncol;
      const char *nm = gph_loci_name(R.LC, R.lb + g);
      for (int i = 0; i < n; i++) {
        const double any = a[2 * B * n + i];
        if (!(any > 0.0)) continue;
        fprintf(part.f, "%lld\t%s\t%d\t%s\t%lld\t%.10g", (long long)(R.lb + g), nm ? nm : "", i, names[i].c_str(), (long long)S, any / Sd);
        for (int b = 0; b < B; b++) {
          const double c = a[b * n + i], t = a[B * n + b * n + i];
          fprintf(part.f, "\t%.10g\t%.10g", c / Sd, c > 0.0 ? t / c : 0.0);
        }
        fprintf(part.f, "\n");
      }
    }
    const long text1 = ftell(part.f);
    return text0 < 0 || text1 < text0 ? part.written_ok(R, GPH_EARG) : part.close(R, (int64_t)(text1 - text0));
  }
  int write(int32_t ranks) override { return gph_ancestry_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_ancestry_discard(prefix, ranks); }
};

// the names that will stand in trees and member lists, once the control file is read and before anything is computed
static int tree_names_ok(Run &R, const char *opt)
{
  auto refuse = [&](const char *kind, const char *nm) {
    snprintf(R.err, sizeof R.err, "the %s name '%s' cannot stand in a tree (white space or one of ()[],:;'=&)", kind, nm);
    return R.fail(GPH_EARG, opt);
  };
  for (int p = 0; p < R.cfg.K; p++)
    if (!gt_name_ok(gph_control_pop_name(R.C, p))) return refuse("population", gph_control_pop_name(R.C, p));
  for (const std::string &nm : leaf_names(R.C, R.cfg))
    if (!gt_name_ok(nm.c_str())) return refuse("sample", nm.c_str());
  return GPH_OK;
}
// a selection SPEC over the loci just read: this rank's share of it, and the share of the rank that holds most
static int select_loci(Run &R, const char *spec, const char *opt, std::vector<int64_t> &sel, int64_t &widest)
{
  std::vector<int64_t> all_sel, held_by(R.world, 0);
  bool all = true;
  if (int rc = gt_parse_spec(spec, R.L, all_sel, all, opt)) return R.fail(rc, opt);
  if (all) for (int64_t g = 0; g < R.L; g++) all_sel.push_back(g);
  for (int64_t g : all_sel) {
    widest = std::max(widest, ++held_by[g / R.per]);
    if (g >= R.lb && g < R.le) sel.push_back(g);
  }
  return GPH_OK;
}

struct Selected : Output {
  const char *const prefix, *const spec, *const opt;   /* opt: "--<name>-loci", as the messages name the selection */
  std::vector<int64_t> sel;          /* this rank's selected loci (global indices) */
  int64_t widest = 0;                /* selected loci of the rank that holds most: every rank takes the same decisions */
  Selected(const char *prefix_, const char *spec_, const char *opt_) : prefix(prefix_), spec(spec_), opt(opt_) {}
  int select(Run &R) { return select_loci(R, spec, opt, sel, widest); }
  /* (a rank without a selected locus hands over an empty list, not NULL, which would mean all its loci) */
  const int64_t *loci() const { static const int64_t none = 0; return sel.empty() ? &none : sel.data(); }
  /* the return code of `call`, an enable call; advice: what to narrow when the engine's byte limit refused it */
  int enabled(Run &R, int rc, const char *call, const char *advice)
  {
    if (rc == GPH_EFULL) snprintf(R.err, sizeof R.err, "%s", advice);
    return R.check(rc, call);
  }
};

struct TextOutput : Selected {
  const TextPart &F;
  TextWriter part;
  TextOutput(const TextPart &F_, const char *prefix_, const char *spec_, const char *opt_) : Selected(prefix_, spec_, opt_), F(F_) {}
  int open_part(Run &R)
  {
    if (part.open(F, prefix, R.rank)) return GPH_OK;
    snprintf(R.err, sizeof R.err, "Could not open %s", text_part_path(F, prefix, R.rank).c_str());
    return R.fail(GPH_EARG, ("opening the " + std::string(F.name) + " part file").c_str());
  }
  int close_part(Run &R) { return R.check(part.close() ? GPH_OK : GPH_EARG, ("writing the " + std::string(F.name) + " part file").c_str()); }
};

struct RowsOutput : TextOutput {
  int32_t capacity, width = 0;       /* rows of the device buffer, numbers of a row */
  std::vector<uint64_t> rows, buf;   /* every row taken so far [sample][width]; one fetch */
  std::vector<int32_t> iters, ibuf;
  RowsOutput(const TextPart &F_, const char *prefix_, const char *spec_, const char *opt_, int32_t rows_) : TextOutput(F_, prefix_, spec_, opt_), capacity(rows_) {}
  virtual int32_t held(Run &R) = 0;                  /* rows in the device buffer */
  virtual int fetch(Run &R, int32_t *got) = 0;       /* they into ibuf, buf */
  virtual int take(Run &R, int it) = 0;              /* one sample on the engine */
  /* the row width is known and the capacity settled: 0 asked for the default */
  void size_rows(int32_t w)
  {
    width = w;
    if (capacity <= 0) capacity = cs_default_rows(width);
  }
  int open_part(Run &R)
  {
    buf.assign((size_t)capacity * width, 0);
    ibuf.assign((size_t)capacity, 0);
    return TextOutput::open_part(R);
  }
  int flush(Run &R)
  {
    int32_t got = 0;
    if (int rc = fetch(R, &got)) return rc;
    rows.insert(rows.end(), buf.begin(), buf.begin() + (size_t)got * width);
    iters.insert(iters.end(), ibuf.begin(), ibuf.begin() + got);
    return GPH_OK;
  }
  int sample(Run &R, int it) override
  {
    if (held(R) >= capacity)
      if (int rc = flush(R)) return rc;
    return take(R, it);
  }
  void write_rows()
  {
    for (size_t r = 0; r < iters.size(); r++) part.numbers("R", &iters[r], rows.data() + r * (size_t)width, (size_t)width);
  }
};

// sampled genealogies: the row buffer for this rank's selected loci; the part's samples each behind their iteration
struct GeneTrees : Selected {
  int32_t capacity, held = 0, rb = 0;
  Part part{"gene-trees"};
  std::vector<char> rows;
  std::vector<int32_t> iters;
  explicit GeneTrees(const gph_run_options &o) : Selected(o.gene_trees_prefix, o.gene_trees_loci, "--gene-trees-loci"), capacity(o.gene_trees_rows) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.gene_trees_prefix && (o.gene_trees_loci || o.gene_trees_rows != 0)) { fprintf(stderr, "gphocs_hip: a gene-trees selection or row count needs a gene-trees prefix\n"); return GPH_EARG; }
    return o.gene_trees_rows < 0 ? GPH_EARG : GPH_OK;
  }
  int check_names(Run &R) { return tree_names_ok(R, "--gene-trees"); }
  int open(Run &R) override
  {
    /* the bytes of a record (the same on every rank) from an empty selection, then the rows that fit */
    int rc;
    const int64_t none = 0;
    if ((rc = gph_engine_gene_trees_enable(R.E, 1, &none, 0, 0))) return R.fail(rc, "gph_engine_gene_trees_enable");
    gph_engine_gene_trees_shape(R.E, nullptr, nullptr, &rb, nullptr, nullptr);
    const int64_t limit = (int64_t)256 << 20, row_bytes = widest * rb;
    if (row_bytes > limit) {
      snprintf(R.err, sizeof R.err, "one sample of %lld loci x %d bytes a record is %lld bytes, the limit is %lld: narrow --gene-trees-loci",
               (long long)widest, (int)rb, (long long)row_bytes, (long long)limit);
      return R.fail(GPH_EFULL, "--gene-trees");
    }
    const int64_t fit = row_bytes > 0 ? limit / row_bytes : limit;
    capacity = (int32_t)std::min<int64_t>(capacity > 0 ? capacity : 64, fit);
    if ((rc = gph_engine_gene_trees_enable(R.E, capacity, loci(), (int64_t)sel.size(), 0))) return R.fail(rc, "gph_engine_gene_trees_enable");
    int32_t hdr[GT_NH] = {R.cfg.n, R.cfg.K, R.cfg.B, rb};
    gph_engine_gene_trees_shape(R.E, nullptr, nullptr, nullptr, hdr + 4, nullptr);
    rows.resize((size_t)capacity * sel.size() * (size_t)rb);
    iters.resize((size_t)capacity);
    std::vector<std::string> labels = leaf_names(R.C, R.cfg), loci;
    for (int i = 0; i < R.cfg.n; i++) labels[(size_t)i] += "." + std::to_string(i);
    for (int64_t g : sel) { const char *nm = gph_loci_name(R.LC, g); loci.push_back(nm ? nm : ""); }
    return part.open(R, GT_PART, prefix, hdr, (int64_t)sel.size(), sel.data(), {pop_names(R.C, R.cfg), band_names(R.C, R.cfg), labels, loci});
  }
  int flush(Run &R)
  {
    held = 0;
    return part.flush(R, [&](int32_t *got) { return gph_engine_gene_trees_fetch(R.E, iters.data(), rows.data(), capacity, got); },
                      rows.data(), (size_t)rb, (int32_t)sel.size(), iters.data(), 4, true);
  }
  int sample(Run &R, int it) override
  {
    const int rc = R.check(gph_engine_gene_trees_sample(R.E, it), "gph_engine_gene_trees_sample");
    return rc || ++held < capacity ? rc : flush(R);
  }
  int close(Run &R) override { const int rc = flush(R); return rc ? rc : part.close(R); }
  int write(int32_t ranks) override { return gph_gene_trees_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_gene_trees_discard(prefix, ranks); }
};

// clade tables: accumulated on the device over the whole run, fetched once; this rank's rows of the two files as its part
struct Clades : TextOutput {
  int32_t slots;
  double F;
  explicit Clades(const gph_run_options &o) : TextOutput(CL_TEXT, o.clades_prefix, o.clades_loci, "--clades-loci"), slots(o.clades_slots),
                                              F(o.clades_min_support == 0.0 ? 0.5 : o.clades_min_support < 0.0 ? 0.0 : o.clades_min_support) {}
  static int validate(const gph_run_options &o)
  {
    if (!o.clades_prefix && (o.clades_loci || o.clades_slots != 0 || o.clades_min_support != 0.0)) {
      fprintf(stderr, "gphocs_hip: a clades selection, slot count or support threshold needs a clades prefix\n");
      return GPH_EARG;
    }
    if (o.clades_slots != 0 && (o.clades_slots < 2 || (o.clades_slots & (o.clades_slots - 1)) != 0)) {
      fprintf(stderr, "gphocs_hip: clades: %d slots are no power of two >= 2\n", (int)o.clades_slots);
      return GPH_EARG;
    }
    if (!(o.clades_min_support <= 1.0)) { fprintf(stderr, "gphocs_hip: clades: the support threshold lies in [0, 1]\n"); return GPH_EARG; }
    return GPH_OK;
  }
  int check_names(Run &R) { return tree_names_ok(R, "--clades"); }
  int open(Run &R) override
  {
    if (int rc = enabled(R, gph_engine_clades_enable(R.E, slots, loci(), (int64_t)sel.size(), 0), "gph_engine_clades_enable",
                         "the tables exceed 1 GiB: narrow --clades-loci or lower --clades-slots")) return rc;
    return open_part(R);
  }
  int sample(Run &R, int) override { return R.check(gph_engine_clades_sample(R.E), "gph_engine_clades_sample"); }
  int close(Run &R) override
  {
    int32_t P = 0, W = 0;
    int64_t S = 0;
    gph_engine_clades_shape(R.E, nullptr, &P, &W, nullptr, &S);
    const int n = R.cfg.n, ew = W + 2;
    std::vector<uint64_t> ent(sel.size() * (size_t)P * ew + 1);
    std::vector<uint32_t> nkeys(sel.size() + 1), dropped(sel.size() + 1);
    if (int rc = gph_engine_clades_fetch(R.E, ent.data(), nkeys.data(), dropped.data(), 0)) return R.fail(rc, "gph_engine_clades_fetch");
    std::vector<std::string> labels = leaf_names(R.C, R.cfg);
    std::vector<const char *> lab;
    for (int i = 0; i < n; i++) labels[(size_t)i] += "." + std::to_string(i);
    for (int i = 0; i < n; i++) lab.push_back(labels[(size_t)i].c_str());
    std::vector<const uint64_t *> kept;
    std::string tree, members;
    for (size_t q = 0; q < sel.size(); q++) {
      const uint64_t *tab = ent.data() + q * (size_t)P * ew;
      const char *nm = gph_loci_name(R.LC, sel[q]);
      kept.clear();
      for (int s = 0; s < P; s++) {
        const uint64_t *en = tab + (size_t)s * ew;
        if (en[W] != 0 && (double)en[W] / (double)S >= F) kept.push_back(en);
      }
      auto size_of = [&](const uint64_t *en) { int c = 0; for (int w = 0; w < W; w++) c += __builtin_popcountll(en[w]); return c; };
      std::sort(kept.begin(), kept.end(), [&](const uint64_t *a, const uint64_t *b) {
        if (a[W] != b[W]) return a[W] > b[W];
        const int sa = size_of(a), sb = size_of(b);
        if (sa != sb) return sa < sb;
        for (int w = W - 1; w >= 0; w--) if (a[w] != b[w]) return a[w] < b[w];
        return false;
      });
      for (const uint64_t *en : kept) {
        double age;
        memcpy(&age, en + W + 1, 8);
        members.clear();
        for (int i = 0; i < n; i++)
          if ((en[i / 64] >> (i % 64)) & 1) { if (!members.empty()) members += ","; members += lab[(size_t)i]; }
        part.line("C\t%lld\t%s\t%lld\t%u\t%d\t%.10g\t%.10g\t%s\n", (long long)sel[q], nm ? nm : "", (long long)S, (unsigned)dropped[q], size_of(en),
                  (double)en[W] / (double)S, age / (double)en[W], members.c_str());
      }
      size_t len = 0;
      int32_t resolved = 0;
      int rc = gph_clades_consensus(n, P, tab, S, lab.data(), nullptr, 0, &len, &resolved);
      if (!rc) { tree.assign(len + 1, '\0'); rc = gph_clades_consensus(n, P, tab, S, lab.data(), &tree[0], len + 1, &len, &resolved); }
      if (rc) { snprintf(R.err, sizeof R.err, "the table of locus %lld gives no consensus tree", (long long)sel[q]); return R.fail(rc, "gph_clades_consensus"); }
      part.line("T\t%lld\t%s\t%lld\t%u\t%u\t%d\t%s\n", (long long)sel[q], nm ? nm : "", (long long)S, (unsigned)nkeys[q], (unsigned)dropped[q], (int)resolved, tree.c_str());
    }
    return close_part(R);
  }
  int write(int32_t ranks) override { return gph_clades_write(prefix, ranks); }
  void discard(int32_t ranks) override { gph_clades_discard(prefix, ranks); }
};

// ---- `--ess PREFIX [--ess-loci SPEC]`: effective sample sizes per trace column and per locus
#include "gph_ess_run.h"

// ---- `--predictive PREFIX [--predictive-loci SPEC] [--predictive-seed N] [--predictive-rows N]`: posterior predictive checks
#include "gph_predictive_run.h"

// ---- `--triplets PREFIX [--triplets-pops "A,B,C;D,E,F"] [--triplets-loci SPEC] [--triplets-rows N]`: triplet topology weights
#include "gph_triplets_run.h"

// ---- `--mutations PREFIX [--mutations-loci SPEC] [--mutations-rows N]`: expected substitutions per population and per sample
#include "gph_mutations_run.h"

// ---- `--simulate PREFIX [--simulate-loci SPEC] [--simulate-seed N] [--simulate-rows N] [--simulate-no-sites]`: replicate genealogies
#include "gph_simulate_run.h"

// ---- `--pair-times PREFIX [--pair-times-pops "A,B;A,A"] [--pair-times-grid LO,HI,B] [--pair-times-loci SPEC] [--pair-times-rows N]`:
// pairwise coalescence-time distributions
#include "gph_pairtimes_run.h"

// ---- `--sfs PREFIX [--sfs-pairs "A,B;C,D"|none] [--sfs-loci SPEC] [--sfs-rows N]`: site-frequency spectra, data against sampled genealogies
#include "gph_sfs_run.h"

// the enabled outputs in the order of their engine calls at a sample, which is also the order in which gph_run_finish writes
// their files (the groups of fewer files first: should a later one fail, fewer are removed again).  A run closes them in the
// opposite order, as it always did, and opens them in that order too: the summary is now enabled last, not first
struct Outputs {
  std::vector<std::unique_ptr<Output>> list;
  LocusSummary *summary = nullptr;   /* these two have a step of their own in run_chain */
  GeneTrees *trees = nullptr;
  Clades *clades = nullptr;
  Ess *ess = nullptr;
  Predictive *predictive = nullptr;
  Triplets *triplets = nullptr;
  Mutations *mutations = nullptr;
  Simulate *simulate = nullptr;
  PairTimes *pair_times = nullptr;
  Sfs *sfs = nullptr;
  explicit Outputs(const gph_run_options &o)
  {
    if (o.locus_summary_path) list.emplace_back(summary = new LocusSummary);
    if (o.ess_prefix) list.emplace_back(ess = new Ess(o));
    if (o.predictive_prefix) list.emplace_back(predictive = new Predictive(o));
    if (o.triplets_prefix) list.emplace_back(triplets = new Triplets(o));
    if (o.mutations_prefix) list.emplace_back(mutations = new Mutations(o));
    if (o.simulate_prefix) list.emplace_back(simulate = new Simulate(o));
    if (o.pair_times_prefix) list.emplace_back(pair_times = new PairTimes(o));
    if (o.sfs_prefix) list.emplace_back(sfs = new Sfs(o));
    if (o.clades_prefix) list.emplace_back(clades = new Clades(o));
    if (o.gene_trees_prefix) list.emplace_back(trees = new GeneTrees(o));
    if (o.ancestry_prefix) list.emplace_back(new Ancestry(o));
    if (o.coal_stats_prefix) list.emplace_back(new CoalStats(o));
  }
};

// ---- `--replicates`: independent chains next to the run's own, and the diagnostics across them
#include "gph_replicates_run.h"

// ---- the log on stdout and the find-finetunes search (GPhoCS.c:1329, 1356-1447, 1808-2249)
struct Log {
  Run &R;
  const int64_t totalCoals;
  const time_t wall0 = time(NULL);
  int logsPerLine = R.info.logsPerLine, samplesPerLog = R.mc.samplesPerLog, findingFinetunes = 0;
  Finetune fCoal{R.mc.ftCoalTime}, fMig{R.mc.ftMigTime}, fTheta{R.mc.ftTheta}, fRate{R.mc.ftMigRate}, fMix{R.mc.ftMixing}, fLocus{R.mc.ftLocusRate}, fAdmix{-1.0};
  /* fAdmix: upstream also bisects the (unused) admixture step and prints it (GPhoCS.c:2040-2066, 2190) */
  std::vector<Finetune> fTau = std::vector<Finetune>(R.cfg.K);
  int64_t logCount = 1, a0[9] = {0}, aLocus0 = 0;
  std::vector<int64_t> t0v = std::vector<int64_t>(R.cfg.K, 0), tv = t0v;
  /* TAU columns of the log exactly as upstream accumulates them (GPhoCS.c:1620-1650): the whole accept array is
   * added after UpdateTau AND after UpdateSampleAge, so an ancestral population's count goes in twice and an
   * estimated sample age's goes in once stale (the previous iteration's) and once fresh */
  std::vector<int64_t> tauPrevTotal = t0v, tauLastIter = t0v, tauShown = t0v;
  Mc3Run *mc3 = nullptr;         /* `--mc3`: the heated chains are given what chain 0 is given */
  Log(Run &run, int64_t coals, Mc3Run *chains = nullptr) : R(run), totalCoals(coals), mc3(chains) { for (int p = 0; p < R.cfg.K; p++) fTau[p].v = R.mc.ftTaus[p]; }
  const char *printtime(char *buf, size_t len) const   /* printtime(), utils.c:314-326 */
  {
    const long t = (long)(time(NULL) - wall0);
    const long h = t / 3600, mm = (t % 3600) / 60, ss = t - (t / 60) * 60;
    if (h) snprintf(buf, len, "%ld:%02ld:%02ld", h, mm, ss);
    else snprintf(buf, len, "%2ld:%02ld", mm, ss);
    return buf;
  }
  int push_finetunes()
  {
    std::vector<double> taus(R.cfg.K);
    for (int p = 0; p < R.cfg.K; p++) taus[p] = fTau[p].v;
    gph_mcmc_set_locus_rate_finetune(R.M, fLocus.v);
    if (mc3) mc3->push_finetunes(fCoal.v, fMig.v, fTheta.v, fRate.v, fMix.v, taus.data(), fLocus.v);
    return R.check(gph_mcmc_set_finetunes(R.M, fCoal.v, fMig.v, fTheta.v, fRate.v, fMix.v, taus.data()), "gph_mcmc_set_finetunes");
  }
  int start();
  void account();
  int period(int it);
};

// the title and, where the control file asks for it, the start of the search
int Log::start()
{
  if (R.lead) {
    printf("There are %d parameters in the model.\n", R.mc.numParameters);
    printf("Samples   CoalTimes MigTimes  SPRs      Thetas    MigRates ");
    for (int p = 0; p < R.cfg.K; p++) if (p >= R.cfg.Kc || R.mc.updateSampleAge[p]) printf("TAU_%2d    ", p);
    printf("RbberBnd  MutRates  Mixing    | DATA-ln-ld |  TIME\n");
    printf("-------------------------------------------------------------"
           "-------------------------------------------------------------"
           "---------------------------\n");
    fflush(stdout);
  }
  if (!R.info.findFinetunes) return GPH_OK;
  findingFinetunes = 1;
  samplesPerLog = R.info.findFinetunesSamplesPerStep;
  logsPerLine = 1;
  if (R.lead) {
    printf("   ---  Dynamically finding finetune settings for the first %d samples, updating finetunes every %d samples  ---- \n",
           samplesPerLog * R.info.findFinetunesNumSteps, samplesPerLog);
    printf("------------------------------------------------------------"
           "------------------------------------------------------------"
           "-----------------------------\n");
  }
  for (Finetune *f : {&fCoal, &fMig, &fTheta, &fRate, &fMix, &fLocus, &fAdmix}) if (f->v < 0) f->v = 1.0;
  for (int p = 0; p < R.cfg.K; p++) if (fTau[p].v < 0) fTau[p].v = 1.0;
  if (int rc = push_finetunes()) return rc;
  gph_mcmc_set_log_period(R.M, samplesPerLog);
  if (mc3) mc3->set_log_period(samplesPerLog);
  return GPH_OK;
}

// after every iteration: the TAU columns' counts
void Log::account()
{
  gph_mcmc_tau_accept_counts(R.M, tv.data());
  for (int p = 0; p < R.cfg.K; p++) {
    const int64_t now = tv[p] - tauPrevTotal[p];
    tauShown[p] += p >= R.cfg.Kc ? 2 * now : tauLastIter[p] + now;
    tauLastIter[p] = now;
    tauPrevTotal[p] = tv[p];
  }
}

// the end of a log period: acceptance percentages of the period exactly as upstream computes them (GPhoCS.c:1821-1853):
// logCount starts at 1, and the tau counts of a period are added twice (after UpdateTau and again after UpdateSampleAge,
// GPhoCS.c:1620-1623, 1646-1649)
int Log::period(int it)
{
  const gph_config &cfg = R.cfg;
  int64_t a[9], aLocus = 0;
  double logL = 0, dataL = 0;
  gph_mcmc_accept_counts(R.M, a);
  gph_mcmc_tau_accept_counts(R.M, tv.data());
  gph_mcmc_get_state(R.M, &logL, &dataL, nullptr, nullptr, nullptr);
  const double lc = (double)logCount;
  gph_mcmc_locus_rate_state(R.M, &aLocus, nullptr);
  const double pCoal = (a[0] - a0[0]) * 100.0 / (lc * (double)totalCoals);
  const double pMig = (a[1] - a0[1]) * 100.0 / ((double)(a[7] - a0[7]) + 0.000001);
  const double pSpr = (a[2] - a0[2]) * 100.0 / (lc * 2 * (double)totalCoals);
  const double pTheta = (a[3] - a0[3]) * 100.0 / (lc * cfg.K);
  const double pRate = (a[4] - a0[4]) * 100.0 / (lc * cfg.B + 0.000001);
  const double pMix = (a[6] - a0[6]) * 100.0 / lc;
  const double pLocus = (aLocus - aLocus0) * 100.0 / (lc * (double)(R.info.numLoci - 1));   /* GPhoCS.c:1842-1845 */
  if (R.lead) {   /* the log line, GPhoCS.c:1857-1895 */
    char tbuf[64];
    printf("\r%7d   %5.1f%%    %5.1f%%    %5.1f%%    %5.1f%%    %5.1f%%    ", it + 1, pCoal, pMig, pSpr, pTheta, pRate);
    for (int p = 0; p < cfg.K; p++)
      if (p >= cfg.Kc || R.mc.updateSampleAge[p]) printf("%5.1f%%    ", tauShown[p] * 100.0 / lc);
    printf("%6.1f%%    %5.1f%%    %5.1f%%    ", (a[8] - a0[8]) * 100.0 / (lc * (cfg.K - cfg.Kc)), pLocus, pMix);
    printf("|%12.6f|", logL);
    printf(" %s", printtime(tbuf, sizeof tbuf));
    if ((it + 1) % (samplesPerLog * logsPerLine) == 0) printf("\n");
    fflush(stdout);
  }
  if (findingFinetunes) {   /* one step of the search (GPhoCS.c:1896-2251) */
    fCoal.adjust(pCoal); fMig.adjust(pMig); fTheta.adjust(pTheta); fRate.adjust(pRate); fMix.adjust(pMix);
    fLocus.adjust(pLocus);
    fAdmix.adjust(0.0);
    for (int p = cfg.Kc; p < cfg.K; p++) fTau[p].adjust(2 * (tv[p] - t0v[p]) * 100.0 / lc);
    if (int rc = push_finetunes()) return rc;
    if (R.lead) printf("          %-9.7lf %-9.7lf           %-9.7lf %-9.7lf %-9.7lf ", fCoal.v, fMig.v, fTheta.v, fRate.v, fAdmix.v);
    for (int p = cfg.Kc; p < cfg.K; p++) if (R.lead) printf("%-9.7lf ", fTau[p].v);
    if (R.lead) printf("          %-9.7lf %-9.7lf \n", fLocus.v, fMix.v);
  }
  logCount = 1;
  memcpy(a0, a, sizeof a0);
  aLocus0 = aLocus;
  t0v = tv;
  std::fill(tauShown.begin(), tauShown.end(), 0);
  if (findingFinetunes && it + 1 >= R.info.findFinetunesSamplesPerStep * R.info.findFinetunesNumSteps) {
    findingFinetunes = 0;
    samplesPerLog = R.mc.samplesPerLog;
    gph_mcmc_set_log_period(R.M, samplesPerLog);
    if (mc3) mc3->set_log_period(samplesPerLog);
    logsPerLine = R.info.logsPerLine;
    if (R.lead) {   /* GPhoCS.c:2232-2251 */
      printf("\n");
      printf("-------------------------------------  finetunes  ------------------------------------\n");
      printf("          %8lf  %8lf            %8lf  %8lf  ", fCoal.v, fMig.v, fTheta.v, fRate.v);
      for (int p = 0; p < cfg.K; p++) printf("%8lf  ", fTau[p].v);
      printf("          %8lf  %8lf  \n", fLocus.v, fMix.v);
      printf("--------------------------------------------------------------------------------------\n");
    }
  }
  return GPH_OK;
}

// ---- `--beta B` and `--marginal-likelihood PREFIX` (gph_run_options says what they do)
// the beta of the options: 0 = not given = 1, negative = 0
double option_beta(const gph_run_options &o) { return o.beta == 0.0 ? 1.0 : o.beta < 0.0 ? 0.0 : o.beta; }
std::string marginal_path(const char *prefix) { return std::string(prefix) + ".marginal.tsv"; }

struct Marginal {
  struct Rung { int k; double beta, mean, sd, lnRatio, acc[7]; };
  const int K, s;
  const double a;
  int b = 0;
  std::vector<Rung> rungs;
  double lnZss = 0.0, lnZti = 0.0;
  explicit Marginal(const gph_run_options &o) : K(o.marginal_steps ? o.marginal_steps : 32), s(o.marginal_samples ? o.marginal_samples : 2000),
                                                a(o.marginal_alpha != 0.0 ? o.marginal_alpha : 0.3) {}
  static int refuse(const char *msg) { fprintf(stderr, "gphocs_hip: %s\n", msg); return GPH_EARG; }
  static int validate(const gph_run_options &o)
  {
    if (!(o.beta <= 64.0)) return refuse("--beta takes a number in [0, 64]");      /* (a NaN fails the comparison) */
    if (!o.marginal_prefix) {
      if (o.marginal_steps) return refuse("--ml-steps needs --marginal-likelihood PREFIX");
      if (o.marginal_burnin) return refuse("--ml-burnin needs --marginal-likelihood PREFIX");
      if (o.marginal_samples) return refuse("--ml-samples needs --marginal-likelihood PREFIX");
      if (o.marginal_alpha != 0.0) return refuse("--ml-alpha needs --marginal-likelihood PREFIX");
      return GPH_OK;
    }
    if (o.beta != 0.0) return refuse("--beta and --marginal-likelihood exclude each other: the ladder sets beta itself");
    if (o.marginal_steps < 0) return refuse("--ml-steps takes a number of steps K >= 1");
    if (o.marginal_samples < 0) return refuse("--ml-samples takes a number of samples s >= 1");
    if (!(o.marginal_alpha >= 0.0) || std::isinf(o.marginal_alpha)) return refuse("--ml-alpha takes a finite number a > 0");
    return GPH_OK;
  }
  double beta_of(int k) const { return k == K ? 1.0 : k == 0 ? 0.0 : pow((double)k / (double)K, 1.0 / a); }
  /* the ladder, from beta = 1 downward, on the chain as the run left it; `it` goes on counting (the checkAll period with it) but
   * never passes start-mig a second time.  The host synchronisation at the end of every iteration hands out l: no other one */
  int run(Run &R, int64_t totalCoals)
  {
    const gph_control_info &info = R.info;
    const gph_config &cfg = R.cfg;
    b = R.o.marginal_burnin < 0 ? 0 : R.o.marginal_burnin > 0 ? R.o.marginal_burnin : info.burnin > 0 ? info.burnin : 1000;
    int it = std::max(info.numSamples, R.mc.startMig + 1), ntau = cfg.K - cfg.Kc, rc;
    for (int p = 0; p < cfg.Kc; p++) ntau += R.mc.updateSampleAge[p] != 0;
    if (R.lead) printf("Marginal likelihood: %d steps down the ladder beta_k = (k/%d)^(1/%g), %d + %d iterations each.\n", K, K, a, b, s);
    std::vector<std::vector<double>> l(K + 1, std::vector<double>(s));
    const double n = (double)(b + s);
    for (int k = K; k >= 0; k--) {
      Rung r;
      r.k = k; r.beta = beta_of(k); r.lnRatio = 0.0;
      if ((rc = gph_mcmc_set_beta(R.M, r.beta))) return R.fail(rc, "gph_mcmc_set_beta");
      int64_t a0[9], a1[9];
      gph_mcmc_accept_counts(R.M, a0);
      for (int j = -b; j < s; j++, it++) {
        if ((rc = gph_mcmc_iteration(R.M, it))) return R.fail(rc, "gph_mcmc_iteration");
        if (j >= 0) gph_mcmc_get_state(R.M, nullptr, &l[k][j], nullptr, nullptr, nullptr);
      }
      gph_mcmc_accept_counts(R.M, a1);
      double sum = 0.0, ss = 0.0;
      for (int j = 0; j < s; j++) sum += l[k][j];
      r.mean = sum / s;
      for (int j = 0; j < s; j++) ss += (l[k][j] - r.mean) * (l[k][j] - r.mean);
      r.sd = s > 1 ? sqrt(ss / (s - 1)) : 0.0;
      const int64_t d7 = a1[7] - a0[7];
      r.acc[0] = (a1[0] - a0[0]) / (n * (double)totalCoals);
      r.acc[1] = d7 > 0 ? (a1[1] - a0[1]) / (double)d7 : 0.0;
      r.acc[2] = (a1[2] - a0[2]) / (n * 2 * (double)totalCoals);
      r.acc[3] = (a1[3] - a0[3]) / (n * cfg.K);
      r.acc[4] = cfg.B > 0 ? (a1[4] - a0[4]) / (n * cfg.B) : 0.0;
      r.acc[5] = ntau > 0 ? (a1[5] - a0[5]) / (n * ntau) : 0.0;
      r.acc[6] = (a1[6] - a0[6]) / n;
      if (R.lead) {
        printf("rung %3d  beta %-12.10g meanLnL %-16.10g accepted: CoalTimes %5.1f%% MigTimes %5.1f%% SPRs %5.1f%% Thetas %5.1f%% MigRates %5.1f%% Taus %5.1f%% Mixing %5.1f%%\n",
               k, r.beta, r.mean, 100 * r.acc[0], 100 * r.acc[1], 100 * r.acc[2], 100 * r.acc[3], 100 * r.acc[4], 100 * r.acc[5], 100 * r.acc[6]);
        fflush(stdout);
      }
      rungs.push_back(r);
    }
    /* the estimates: rungs[K - k] is rung k */
    for (int k = 0; k < K; k++) {
      const double d = rungs[K - k - 1].beta - rungs[K - k].beta;
      double m = d * l[k][0], e = 0.0;
      for (int j = 1; j < s; j++) m = std::max(m, d * l[k][j]);
      for (int j = 0; j < s; j++) e += exp(d * l[k][j] - m);
      rungs[K - k].lnRatio = m + log(e / s);
      lnZss += rungs[K - k].lnRatio;
      lnZti += d * (rungs[K - k].mean + rungs[K - k - 1].mean) / 2;
    }
    if (R.lead) printf("Marginal likelihood: lnZ_ss %.10g lnZ_ti %.10g (steps %d alpha %.10g)\n", lnZss, lnZti, K, a);
    return gph_mcmc_set_beta(R.M, 1.0);
  }
  int write(Run &R) const
  {
    const std::string path = marginal_path(R.o.marginal_prefix);
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { snprintf(R.err, sizeof R.err, "Could not open %s", path.c_str()); return R.fail(GPH_EARG, "writing the marginal-likelihood table"); }
    fprintf(f, "rung\tbeta\tsamples\tmeanLnL\tsdLnL\tlnRatio\taccCoal\taccMig\taccSpr\taccTheta\taccMigRate\taccTau\taccMixing\n");
    for (const Rung &r : rungs) {
      fprintf(f, "%d\t%.10g\t%d\t%.10g\t%.10g\t%.10g", r.k, r.beta, s, r.mean, r.sd, r.lnRatio);
      for (double v : r.acc) fprintf(f, "\t%.10g", v);
      fprintf(f, "\n");
    }
    fprintf(f, "# lnZ_ss %.10g lnZ_ti %.10g steps %d alpha %.10g\n", lnZss, lnZti, K, a);
    const int rcc = ferror(f) | fclose(f);
    if (rcc) { unlink(path.c_str()); return R.fail(GPH_EARG, "writing the marginal-likelihood table"); }
    return GPH_OK;
  }
};

// one rank's run up to its parts: what becomes of those is gph_run_finish's
int run_chain(const gph_run_options &o)
{
  Run R(o);
  std::unique_ptr<Mc3Run> mc3;   /* (behind R: the heated chains go before the loci they were loaded from) */
  std::unique_ptr<Replicates> rep;
  Outputs outs(o);   /* (behind R: the parts are closed before anything is freed) */
  int rc;
  if ((rc = R.read_control())) return rc;
  if (outs.trees && (rc = outs.trees->check_names(R))) return rc;
  if (outs.clades && (rc = outs.clades->check_names(R))) return rc;
  if (outs.triplets && (rc = outs.triplets->check_pops(R))) return rc;
  if (outs.pair_times && (rc = outs.pair_times->check_pops(R))) return rc;
  if (outs.sfs && (rc = outs.sfs->check_pops(R))) return rc;
  if ((rc = R.read_loci())) return rc;
  if (outs.trees && (rc = outs.trees->select(R))) return rc;
  if (outs.clades && (rc = outs.clades->select(R))) return rc;
  if (outs.ess && (rc = outs.ess->select(R))) return rc;
  if (outs.predictive && (rc = outs.predictive->select(R))) return rc;
  if (outs.triplets && (rc = outs.triplets->select(R))) return rc;
  if (outs.mutations && (rc = outs.mutations->select(R))) return rc;
  if (outs.simulate && (rc = outs.simulate->select(R))) return rc;
  if (outs.pair_times && (rc = outs.pair_times->select(R))) return rc;
  if (outs.sfs && (rc = outs.sfs->select(R))) return rc;
  if ((rc = R.start_engine()) || (rc = R.open_trace())) return rc;
  if (o.beta != 0.0) {
    if ((rc = gph_mcmc_set_beta(R.M, option_beta(o)))) return R.fail(rc, "gph_mcmc_set_beta");
    if (R.lead) printf("Power posterior: beta = %.10g%s -- the trace and every other output describe p(D|G)^beta p(G|Theta) p(Theta); the log-likelihood columns stay those of the plain likelihood.\n",
                       option_beta(o), option_beta(o) == 0.0 ? " (the prior)" : "");
  }
  if (o.mc3_chains) {
    mc3.reset(new Mc3Run(o));
    if ((rc = mc3->start(R))) return rc;
  }
  if (o.replicates) {
    mc3.reset(new Mc3Run(o.replicates, "--replicates"));
    if ((rc = mc3->start(R))) return rc;
    rep.reset(new Replicates(o, *mc3));
  }

  const gph_control_info &info = R.info;
  if (R.lead) printf("Starting MCMC: %d burnin, %d running, sampled every %d iteration(s).\n", info.burnin, info.numSamples, info.sampleSkip);
  if (R.lead && info.mutRateMode == 2) printf("Reading locus rates from file %s... ", info.rateFile);   /* readRateFile's progress text (GPhoCS.c:514), printed from initializeMCMC upstream */
  int64_t totalCoals = 0;
  if ((rc = gph_mcmc_initialize(R.M, &totalCoals))) return R.fail(rc, "gph_mcmc_initialize");
  if (mc3 && (rc = mc3->initialize(R))) return rc;
  for (auto x = outs.list.rbegin(); x != outs.list.rend(); ++x)
    if ((rc = (*x)->open(R))) return rc;
  if (rep && (rc = rep->open(R, outs.clades))) return rc;
  auto t1 = std::chrono::steady_clock::now();
  Log log(R, totalCoals, mc3.get());
  if ((rc = log.start())) return rc;
  for (int it = -info.burnin; it < info.numSamples; it++) {
    if (mc3) { if ((rc = mc3->iteration(R, it))) return rc; }
    else if ((rc = gph_mcmc_iteration(R.M, it))) return R.fail(rc, "gph_mcmc_iteration");
    log.account();
    if (it >= 0 && it % (info.sampleSkip + 1) == 0) {
      R.trace_line(it);
      for (auto &x : outs.list)
        if ((rc = x->sample(R, it))) return rc;
      if (rep && (rc = rep->sample(R, it))) return rc;
    }
    log.logCount++;
    if ((it + 1) % log.samplesPerLog == 0 && (rc = log.period(it))) return rc;
  }
  double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  if (R.lead) {
    char tbuf[64];
    printf("\nMCMC finished. Time used: %s\n", log.printtime(tbuf, sizeof tbuf));   /* GPhoCS.c:2262 */
    if (o.verbose) printf("(%.2f s, %.3f iterations/s)\n", sec, (info.burnin + info.numSamples) / (sec > 0 ? sec : 1));
  }
  if (mc3 && !rep) mc3->log_pairs(R);
  if (rep && (rc = rep->finish(R))) return rc;
  fclose(R.trace);
  R.trace = nullptr;
  for (auto x = outs.list.rbegin(); x != outs.list.rend(); ++x)
    if ((rc = (*x)->close(R))) return rc;
  /* the run is over and what it wrote is closed: the ladder goes on from its last state */
  std::unique_ptr<Marginal> ml;
  if (o.marginal_prefix) {
    ml.reset(new Marginal(o));
    if ((rc = ml->run(R, totalCoals))) return rc;
  }
  /* a CHECKED build of the library (-DGPH_BOUNDS, tests only) says here whether an index left its array during the run */
  int32_t where = 0, checked = 0;
  (void)gph_engine_debug_oob(R.E, &where, &checked);
  /* the report reads the chains' counters: before they go (the group and the heated chains first, then chain 0) */
  int rcr = GPH_OK;
  if (mc3 && o.mc3_report_prefix && R.lead) rcr = mc3->write(R, totalCoals);
  mc3.reset();
  R.release_device();
  if (rcr) return rcr;
  if (checked && where != 0) {
    fprintf(stderr, "gphocs_hip: checked build: an index left its array at %d (source line + 100000 x file: 1 gph_locus.h, 2 gph_kernels.h, "
                    "3 gph_summary.h, 4 gph_coalstats.h, 5 gph_timeslices.h, 6 gph_ancestry.h, 7 gph_sampler.h, 8 gph_genetrees.h, 10 gph_clades.h, 11 gph_cladecmp.h, 12 gph_ess.h, 13 gph_predictive.h, 14 gph_triplets.h, 15 gph_mutations.h, 16 gph_simulate.h, 17 gph_pairtimes.h, 18 gph_sfs.h; 8000xx / 9000xx: typed accessors of the image / the dynamic LDS)\n", (int)where);
    return GPH_EKERNEL;
  }
  if (outs.summary && (rc = outs.summary->write_table(R))) return rc;
  if (rep && R.lead && (rc = rep->write(R))) return rc;
  return ml && R.lead ? ml->write(R) : GPH_OK;
}
}   // namespace

extern "C" int gph_run_finish(const gph_run_options *in, int32_t ranks, int32_t failed)
{
  gph_run_options o;
  if (!take_options(in, o) || ranks < 1) return GPH_EARG;
  Outputs outs(o);
  int rc = GPH_OK;
  for (auto &x : outs.list)
    if (!failed && !rc) rc = x->write(ranks);
  /* a failed run leaves no statistics file and no part behind */
  if (failed || rc) {
    for (auto &x : outs.list) x->discard(ranks);
    if (o.marginal_prefix) unlink(marginal_path(o.marginal_prefix).c_str());
    if (o.mc3_report_prefix) unlink(mc3_path(o.mc3_report_prefix).c_str());
    if (o.replicates_prefix) { unlink(rep_path(o.replicates_prefix, ".psrf.tsv").c_str()); unlink(rep_path(o.replicates_prefix, ".asdsf.tsv").c_str()); }
  }
  return rc;
}

extern "C" int gph_run(const gph_run_options *in)
{
  gph_run_options o;
  if (!take_options(in, o)) return GPH_EARG;
  if (o.comm) { o.rank = gph_comm_rank(o.comm); o.world = gph_comm_world(o.comm); o.allreduce = nullptr; o.user = nullptr; }
  else if (o.world == 0) o.world = 1;
  if (o.world < 1 || o.rank < 0 || o.rank >= o.world || (o.world > 1 && !o.allreduce && !o.comm)) return GPH_EARG;
  /* the checks on the options alone, before anything is read */
  int rc;
  if ((rc = GeneTrees::validate(o)) || (rc = Clades::validate(o)) || (rc = Ess::validate(o)) || (rc = Predictive::validate(o)) || (rc = Triplets::validate(o)) || (rc = Mutations::validate(o)) || (rc = Simulate::validate(o)) || (rc = PairTimes::validate(o)) || (rc = Sfs::validate(o)) || (rc = CoalStats::validate(o)) || (rc = Marginal::validate(o)) || (rc = Mc3Run::validate(o)) ||
      (rc = Replicates::validate(o))) return rc;
  rc = run_chain(o);
  /* one rank: the statistics files now; several: the caller, once every rank's part is complete */
  if (o.world == 1) {
    const int rcf = gph_run_finish(&o, 1, rc);
    if (!rc) rc = rcf;
  }
  return rc;
}

// the simple forms
static gph_run_options plain_options(const char *ctl, const char *ctl2, int32_t device, int32_t verbose)
{
  gph_run_options o;
  memset(&o, 0, sizeof o);
  o.size = sizeof o;
  o.ctl = ctl; o.ctl2 = ctl2; o.device = device; o.verbose = verbose;
  return o;
}

extern "C" int gph_run_control_file(const char *ctl, const char *ctl2, int32_t device, int32_t verbose)
{
  const gph_run_options o = plain_options(ctl, ctl2, device, verbose);
  return gph_run(&o);
}

extern "C" int gph_run_control_file_ranked(const char *ctl, const char *ctl2, int32_t device, int32_t verbose,
                                           int32_t rank, int32_t world, gph_allreduce_fn allreduce, void *user)
{
  gph_run_options o = plain_options(ctl, ctl2, device, verbose);
  o.rank = rank; o.world = world; o.allreduce = allreduce; o.user = user;
  return world < 1 ? GPH_EARG : gph_run(&o);
}

extern "C" int gph_run_control_file_comm(const char *ctl, const char *ctl2, int32_t device, int32_t verbose, gph_comm *comm)
{
  gph_run_options o = plain_options(ctl, ctl2, device, verbose);
  o.comm = comm;
  return gph_run(&o);
}
