// tiff_main.cpp — the TIFF reader (csrc/tiff.cpp: container, strip decoder of
// tiff_strip.h, the device kernels' host twin) as a stand-alone program for
// ASan / UBSan (make sanitize_tiff).  Every *.tif of the directory given is
// opened and each of its pages read into a heap buffer of exactly the page's
// size, rows 5 bytes wider than the page: a write past the page trips ASan, a
// write between rows the check below.  Files may be corrupt: a refusal or a
// decode error is counted, not a failure.
#include <dirent.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "runtime.h"
#include "tiff.h"
#include "unpaper_hip.h"

// the library's error reporting, which tiff.cpp and ccitt.cpp call
namespace uph {
static char g_error[512];
bool fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return false;
}
}  // namespace uph

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: tiff_main DIR\n"), 2;
  DIR* d = opendir(argv[1]);
  if (!d) return fprintf(stderr, "tiff_main: cannot open %s\n", argv[1]), 2;
  std::vector<std::string> names;
  while (dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n.size() > 4 && n.compare(n.size() - 4, 4, ".tif") == 0) names.push_back(n);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  int files = 0, decoded = 0, errors = 0, failures = 0;
  for (const std::string& n : names) {
    const std::string path = std::string(argv[1]) + "/" + n;
    files++;
    UphipTiffDocument* doc = uphip_tiff_open(path.c_str());
    if (!doc) {
      errors++;
      continue;
    }
    const int np = std::min(uphip_tiff_page_count(doc), 8);
    for (int p = 0; p < np; p++) {
      UphipPnmInfo info{0, 0, 0};
      float dpi[2];
      if (uphip_tiff_page_probe(doc, p, &info, dpi) != 0) {
        errors++;
        continue;
      }
      if (uphip_tiff_page_on_device(doc, p) < 0) failures++;
      const int64_t rb = uph::row_bytes(info.width, info.format), ls = rb + 5;
      if ((uint64_t)ls * (uint64_t)info.height > (1ull << 28)) {  // hostile sizes are probed only
        errors++;
        continue;
      }
      const size_t bytes = (size_t)(ls * info.height);
      uint8_t* buf = (uint8_t*)malloc(bytes);
      memset(buf, 0xA5, bytes);
      if (uphip_tiff_read_page(doc, p, buf, ls, &info) == 0) decoded++;
      else errors++;
      for (int64_t y = 0; y < info.height; y++)
        for (int64_t x = rb; x < ls; x++)
          if (buf[y * ls + x] != 0xA5) {
            fprintf(stderr, "tiff_main: %s page %d: row %lld written past its bytes\n", n.c_str(), p, (long long)y);
            failures++;
            y = info.height;
            break;
          }
      free(buf);
    }
    uphip_tiff_close(doc);
  }
  if (failures) return fprintf(stderr, "tiff_main: %d failures\n", failures), 1;
  printf("tiff_main: ok (%d files, %d pages decoded, %d refused or corrupt)\n", files, decoded, errors);
  return 0;
}
