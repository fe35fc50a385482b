// The model of k_png_brute's parallel formulation (tools/models/png_brute_model.h) and the driver's launch arithmetic
// (zopfli_amd/csrc/host/png_brute_launch.h) as a plain C++ program, nothing of LodePNG in it.
//   png_brute_print sizes WINDOW LINEBYTES HEIGHT BYTEWIDTH FILE
//       FILE holds HEIGHT rows of LINEBYTES bytes.  For every job = row * 5 + type, in order, one line "bytes bits": the
//       row filtered with `type` (this file's own statement of the five PNG filters) and sized by the model.
//   png_brute_print launch FORCE_SCRATCH MAX_WORKGROUPS N JOBS [N JOBS ...]
//       one line per pair: "in_lds raise_lds_limit row_bytes stride grid lds_bytes" of PngBruteMakeLaunch.
// -DPNG_BRUTE_WRONG=1 .. 6 builds a model that is wrong in one rule (tests/test_cpu_png_brute_sizes.py shows that the suite
// tells each from LodePNG); no other program sets the rules.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_brute_launch.h"
#include "png_brute_model.h"

namespace {

png_brute_model::Rules TheRules() {
  png_brute_model::Rules r;
#if defined(PNG_BRUTE_WRONG)
#if PNG_BRUTE_WRONG == 1
  r.lazy_258_everywhere = true;
#elif PNG_BRUTE_WRONG == 2
  r.zero_cap = 257;
#elif PNG_BRUTE_WRONG == 3
  r.no_far_3_rule = true;
#elif PNG_BRUTE_WRONG == 4
  r.tail_shift = 4;
#elif PNG_BRUTE_WRONG == 5
  r.keep_is_self = true;
#elif PNG_BRUTE_WRONG == 6
  r.no_nicematch = true;
#else
#error "PNG_BRUTE_WRONG is 1 .. 6"
#endif
#endif
  return r;
}

std::vector<unsigned char> ReadFile(const char* path) {
  std::vector<unsigned char> data;
  FILE* fp = fopen(path, "rb");
  if (!fp) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  unsigned char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, fp)) > 0) data.insert(data.end(), buf, buf + got);
  fclose(fp);
  return data;
}

int Paeth(int a, int b, int c) {   // the PNG specification's predictor: left, above, upper left
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  if (pa <= pb && pa <= pc) return a;
  return pb <= pc ? b : c;
}

// PNG filter `type` of a row: `prev` the row above or null (a row of zeros), pixels of `bw` bytes
void FilterRow(unsigned char* out, const unsigned char* row, const unsigned char* prev, size_t n, size_t bw, int type) {
  for (size_t x = 0; x < n; ++x) {
    const int a = x >= bw ? row[x - bw] : 0;
    const int b = prev ? prev[x] : 0;
    const int c = (prev && x >= bw) ? prev[x - bw] : 0;
    int predicted = 0;
    switch (type) {
      case 1: predicted = a; break;
      case 2: predicted = b; break;
      case 3: predicted = (a + b) / 2; break;
      case 4: predicted = Paeth(a, b, c); break;
      default: break;
    }
    out[x] = static_cast<unsigned char>((row[x] - predicted) & 255);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 7 && std::strcmp(argv[1], "sizes") == 0) {
    const unsigned window = static_cast<unsigned>(strtoul(argv[2], nullptr, 10));
    const size_t n = strtoull(argv[3], nullptr, 10), h = strtoull(argv[4], nullptr, 10), bw = strtoull(argv[5], nullptr, 10);
    const std::vector<unsigned char> image = ReadFile(argv[6]);
    if (window == 0 || window > 32768 || (window & (window - 1)) != 0 || n == 0 || bw == 0 || image.size() != n * h) {
      fprintf(stderr, "bad case: window %u, %zu rows of %zu bytes, file of %zu\n", window, h, n, image.size());
      return 2;
    }
    std::vector<unsigned char> f(n);
    const png_brute_model::Rules rules = TheRules();
    for (size_t y = 0; y < h; ++y) {
      for (int type = 0; type < 5; ++type) {
        FilterRow(f.data(), image.data() + y * n, y ? image.data() + (y - 1) * n : nullptr, n, bw, type);
        const png_brute_model::Size s = png_brute_model::ModelSize(f.data(), n, window, rules);
        printf("%zu %zu\n", s.bytes, s.bits);
      }
    }
    return 0;
  }
  if (argc >= 6 && argc % 2 == 0 && std::strcmp(argv[1], "launch") == 0) {
    zamd::PngBruteKnobs knobs;
    knobs.force_scratch = atoi(argv[2]);
    knobs.max_workgroups = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    for (int i = 4; i + 1 < argc; i += 2) {
      const zamd::PngBruteLaunch L = zamd::PngBruteMakeLaunch(static_cast<uint32_t>(strtoul(argv[i], nullptr, 10)),
                                                              static_cast<uint32_t>(strtoul(argv[i + 1], nullptr, 10)), knobs);
      printf("%d %d %llu %llu %u %u\n", L.in_lds ? 1 : 0, L.raise_lds_limit ? 1 : 0, static_cast<unsigned long long>(L.row_bytes),
             static_cast<unsigned long long>(L.stride), L.grid, L.lds_bytes);
    }
    return 0;
  }
  fprintf(stderr, "usage: png_brute_print sizes WINDOW LINEBYTES HEIGHT BYTEWIDTH FILE | launch FORCE_SCRATCH MAX_WORKGROUPS N JOBS [N JOBS ...]\n");
  return 2;
}
