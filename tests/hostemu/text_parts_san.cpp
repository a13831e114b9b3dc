// text_parts_san.cpp -- a stand-alone program for the sanitizers (tests only): gph_textjoin.h under this main(),
// compiled with -fsanitize=address,undefined (tests/test_text_parts.py builds and runs it).  Nothing of the engine is in it.
//
// Every subdirectory of the directory it is given holds the parts of two ranks under the prefix "out", good or damaged, for
// some of the four text formats.  Each format whose rank-0 part is there is joined, and then discarded once more.
//
//   text_parts_san <directory>
#include <dirent.h>
#include <stdio.h>
#include <string>
#include <unistd.h>
#include "../../g-phocs_amd/csrc/gph_textjoin.h"

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: text_parts_san <directory>\n"); return 2; }
  struct Format { const char *part; int (*write)(const char *, int32_t); int (*discard)(const char *, int32_t); };
  const Format formats[4] = {{".clades.part0", gph_clades_write, gph_clades_discard}, {".ess.part0", gph_ess_write, gph_ess_discard},
                             {".predictive.part0", gph_predictive_write, gph_predictive_discard}, {".triplets.part0", gph_triplets_write, gph_triplets_discard}};
  DIR *top = opendir(argv[1]);
  if (!top) { fprintf(stderr, "text_parts_san: cannot read %s\n", argv[1]); return 1; }
  int dirs = 0, joined = 0, refused = 0;
  while (const dirent *d = readdir(top)) {
    if (d->d_name[0] == '.') continue;
    const std::string prefix = std::string(argv[1]) + "/" + d->d_name + "/out";
    dirs++;
    for (const Format &f : formats) {
      if (access((prefix + f.part).c_str(), F_OK) != 0) continue;
      const int rc = f.write(prefix.c_str(), 2);
      if (rc == GPH_OK) joined++;
      else if (rc == GPH_EARG) refused++;
      else { fprintf(stderr, "text_parts_san: %s%s: status %d\n", prefix.c_str(), f.part, rc); return 1; }
      if (f.discard(prefix.c_str(), 2) != GPH_OK) { fprintf(stderr, "text_parts_san: %s%s: the discard failed\n", prefix.c_str(), f.part); return 1; }
    }
  }
  closedir(top);
  printf("text_parts_san OK: %d directories, %d joined, %d refused\n", dirs, joined, refused);
  return 0;
}
