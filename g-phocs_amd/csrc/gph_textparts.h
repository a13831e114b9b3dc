// gph_textparts.h -- the text part of a rank, in one place.  Host code that needs nothing of the engine or of a run.
//
// Clade tables, effective sample sizes, predictive checks, triplet weights, expected substitutions, replicate genealogies, pair times and site-frequency spectra each write two files from the ranks' text
// parts.  Rank r's part PREFIX<suffix><r> is written once, when the chain is done: a first line with the format's magic
// word, for most formats a line "H\t..." that every rank writes alike, lines "<tag>\t...", and a last line "E\t<lines>"
// with the number of tagged lines, written when the rank closes its part.  A part without that last line, with anything
// behind it or with another count is refused, like one whose H line differs from rank 0's.
//   TextPart    what names a format: magic word, part suffix, the two output suffixes, the name in messages
//   TextWriter  one rank's part: opened with the magic line, lines counted, closed with the E line
//   TextJoin    the ranks' parts into the two files: text_join reads, a format says what its lines mean
//   TextRows    "R\t<iteration>\t<u64>..." lines added rank by rank (and "O\t<u64>..." lines through numbers())
//   text_discard  parts and files removed
#ifndef GPH_TEXTPARTS_H
#define GPH_TEXTPARTS_H
#include "../../include/gphocs_hip.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/types.h>
#include <unistd.h>

struct TextPart {
  const char *magic;         /* the first line, without its newline */
  const char *suffix;        /* rank r's part is PREFIX<suffix><r> */
  const char *files[2];      /* the outputs are PREFIX<files[k]> */
  const char *name;          /* as the messages of a run name the part */
};
const TextPart CL_TEXT = {"GPHCL1", ".clades.part", {".clades.tsv", ".consensus.tsv"}, "clades"};
const TextPart ES_TEXT = {"GPHES1", ".ess.part", {".ess.tsv", ".locus-ess.tsv"}, "ess"};
const TextPart PD_TEXT = {"GPHPD1", ".predictive.part", {".predictive.tsv", ".predictive-genome.tsv"}, "predictive"};
const TextPart TR_TEXT = {"GPHTR1", ".triplets.part", {".triplets.tsv", ".triplets-genome.tsv"}, "triplets"};
const TextPart MU_TEXT = {"GPHMU1", ".mutations.part", {".mutations.tsv", ".mutations-genome.tsv"}, "mutations"};
const TextPart SI_TEXT = {"GPHSI1", ".simulate.part", {".simulate.tsv", ".simulate-genome.tsv"}, "simulate"};
const TextPart PT_TEXT = {"GPHPT1", ".pair-times.part", {".pair-times.tsv", ".pair-times-genome.tsv"}, "pair-times"};
const TextPart SF_TEXT = {"GPHSF1", ".sfs.part", {".sfs.tsv", ".sfs-genome.tsv"}, "sfs"};

inline std::string text_part_path(const TextPart &F, const char *prefix, int r) { return std::string(prefix) + F.suffix + std::to_string(r); }
inline void text_remove_parts(const TextPart &F, const char *prefix, int ranks) { for (int r = 0; r < ranks; r++) remove(text_part_path(F, prefix, r).c_str()); }

inline int text_discard(const TextPart &F, const char *prefix, int32_t ranks)
{
  if (!prefix) return GPH_EARG;
  text_remove_parts(F, prefix, ranks);
  for (const char *sfx : F.files) unlink((std::string(prefix) + sfx).c_str());     /* (files only: whatever else sits there is not ours) */
  return GPH_OK;
}

struct TextWriter {
  FILE *f = nullptr;
  long long lines = 0;
  ~TextWriter() { if (f) fclose(f); }
  bool open(const TextPart &F, const char *prefix, int rank)
  {
    if (!(f = fopen(text_part_path(F, prefix, rank).c_str(), "w"))) return false;
    fprintf(f, "%s\n", F.magic);
    return true;
  }
  /* one tagged line, its newline included in the format (the H line goes to f directly: it is not counted) */
  __attribute__((format(printf, 2, 3))) void line(const char *fmt, ...)
  {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(f, fmt, ap);
    va_end(ap);
    lines++;
  }
  /* "<tag>[\t<iteration>]" + "\t<u64>" per number, as one line */
  void numbers(const char *tag, const int32_t *iteration, const uint64_t *v, size_t count)
  {
    fputs(tag, f);
    if (iteration) fprintf(f, "\t%d", (int)*iteration);
    for (size_t c = 0; c < count; c++) fprintf(f, "\t%llu", (unsigned long long)v[c]);
    fputc('\n', f);
    lines++;
  }
  bool close()
  {
    fprintf(f, "E\t%lld\n", lines);
    const int rc = ferror(f) | fclose(f);
    f = nullptr;
    return rc == 0;
  }
};

// what a format does with the lines of the ranks' parts (each line with its newline, len > 2).  A false return refuses the part
struct TextJoin {
  FILE *out[2] = {nullptr, nullptr};
  const bool has_header;                                     /* an H line behind the magic line */
  explicit TextJoin(bool h) : has_header(h) {}
  virtual ~TextJoin() {}
  virtual void start() {}                                    /* both files open, no part read yet */
  virtual bool header(char *, ssize_t, int) { return false; }   /* rank r's H line: rank 0's sets the shape, the others' match it */
  virtual bool body(char *line, ssize_t len, int rank) = 0;  /* a tagged line */
  virtual bool rank_done() { return true; }                  /* the part's E line was its last and its count is right */
  virtual void summary() {}                                  /* every part was good */
};

inline int text_join(const TextPart &F, TextJoin &J, const char *prefix, int32_t ranks)
{
  if (!prefix || ranks < 1) return GPH_EARG;
  bool ok = true;
  for (int k = 0; k < 2 && ok; k++)
    if (!(J.out[k] = fopen((std::string(prefix) + F.files[k]).c_str(), "w"))) { fprintf(stderr, "gphocs_hip: cannot open %s%s\n", prefix, F.files[k]); ok = false; }
  if (ok) J.start();
  for (int r = 0; r < ranks && ok; r++) {
    const std::string path = text_part_path(F, prefix, r);
    FILE *in = fopen(path.c_str(), "r");
    char *line = nullptr;
    size_t cap = 0;
    ssize_t len;
    long long lines = 0, told = -1;
    int at = 0;
    while (in && ok && (len = getline(&line, &cap, in)) > 0) {
      at++;
      if (at == 1) { ok = line == std::string(F.magic) + "\n"; continue; }
      if (at == 2 && J.has_header) { ok = J.header(line, len, r); continue; }
      if (told >= 0) { ok = false; break; }                      /* something behind the last line */
      if (line[0] == 'E' && line[1] == '\t') { told = atoll(line + 2); continue; }
      ok = len > 2 && line[len - 1] == '\n' && J.body(line, len, r);
      lines += ok;
    }
    free(line);
    if (in) fclose(in);
    if (!in || !ok || at < (J.has_header ? 2 : 1) || told != lines || !J.rank_done()) {
      fprintf(stderr, "gphocs_hip: %s is missing, damaged or incomplete\n", path.c_str());
      ok = false;
    }
  }
  if (ok) J.summary();
  for (int k = 0; k < 2; k++)
    if (J.out[k] && (ferror(J.out[k]) | fclose(J.out[k])) != 0) { fprintf(stderr, "gphocs_hip: writing %s%s failed\n", prefix, F.files[k]); ok = false; }
  text_remove_parts(F, prefix, ranks);
  if (!ok)
    for (int k = 0; k < 2; k++) if (J.out[k]) remove((std::string(prefix) + F.files[k]).c_str());
  return ok ? GPH_OK : GPH_EARG;
}

// the per-sample rows of the ranks, added: every rank writes one R line per sample, in the same order; the iteration of a
// sample is rank 0's, and the other ranks' must agree with it
struct TextRows {
  long long S = 0, width = 0, sample = 0;
  std::vector<unsigned long long> totals;                    /* [sample][width] */
  std::vector<long long> iters;
  void shape(long long samples, long long w) { S = samples; width = w; totals.assign((size_t)(S * width), 0); iters.assign((size_t)S, 0); }
  /* `count` tab-separated unsigned numbers behind `at`, to the end of the line, added into `into` */
  static bool numbers(char *at, long long count, unsigned long long *into)
  {
    for (long long c = 0; c < count; c++) {
      if (*at != '\t') return false;
      char *end = nullptr;
      const unsigned long long v = strtoull(at + 1, &end, 10);
      if (end == at + 1) return false;
      into[c] += v;
      at = end;
    }
    return *at == '\n';
  }
  /* an R line of rank r */
  bool row(char *line, int r)
  {
    char *end = nullptr;
    const long long it = strtoll(line + 2, &end, 10);
    if (!(sample < S && end != line + 2 && (r == 0 || iters[(size_t)sample] == it) && numbers(end, width, totals.data() + (size_t)(sample * width)))) return false;
    iters[(size_t)sample++] = it;
    return true;
  }
  /* a part is done: it held every sample */
  bool rank_done() { const bool all = sample == S; sample = 0; return all; }
  /* "iter" + the rows, as the genome-wide files print them */
  void print(FILE *f) const
  {
    for (long long s = 0; s < S; s++) {
      fprintf(f, "%7d", (int)iters[(size_t)s]);
      for (long long c = 0; c < width; c++) fprintf(f, "\t%llu", totals[(size_t)(s * width + c)]);
      fputc('\n', f);
    }
  }
};

// the label of slot t of a triple of names: the sisters, then the third (the triplets part's writer and joiner print it)
inline std::string tr_label(const std::string m[3], int t)
{
  return m[t == 2 ? 1 : 0] + "," + m[t == 0 ? 1 : 2] + "|" + m[t == 0 ? 2 : t == 1 ? 1 : 0];
}
#endif
