// host/png_container.h's file of a reduced colour mode as a plain C++ program (tests/test_cpu_png_color_cases.py): the
// prefix with PLTE and tRNS (PngPrefixReduced), a zlib stream behind it, the file closed (PngCloseAt).
//   png_prefix_print ZLIB OUT WIDTH HEIGHT COLORTYPE BITDEPTH PALETTE KEY KEY_R KEY_G KEY_B
// PALETTE: the entries r, g, b, a in hex, or - for none.  KEY: 0 or 1.  ZLIB: a stream as
// ZopfliCompress(ZOPFLI_FORMAT_ZLIB) writes it (78 DA ...).  The file is written to OUT; prints "ok BYTES PREFIX", or
// "refused" (exit status 1) when PngReducedFormatOk or PngCloseAt says no.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "png_container.h"

int main(int argc, char** argv) {
  if (argc != 12) {
    std::fprintf(stderr, "usage: png_prefix_print ZLIB OUT WIDTH HEIGHT COLORTYPE BITDEPTH PALETTE KEY KEY_R KEY_G KEY_B\n");
    return 2;
  }
  uint32_t v[9];
  for (int k = 0; k < 4; ++k) v[k] = static_cast<uint32_t>(std::strtoul(argv[3 + k], nullptr, 10));
  for (int k = 0; k < 4; ++k) v[4 + k] = static_cast<uint32_t>(std::strtoul(argv[8 + k], nullptr, 10));
  const std::string hex = std::strcmp(argv[7], "-") == 0 ? "" : argv[7];
  std::vector<unsigned char> palette(hex.size() / 2);
  for (size_t k = 0; k < palette.size(); ++k) palette[k] = static_cast<unsigned char>(std::strtoul(hex.substr(2 * k, 2).c_str(), nullptr, 16));
  if (palette.size() % 4 != 0 || palette.size() > 1024) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<unsigned char> zlib;
  unsigned char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) != 0;) zlib.insert(zlib.end(), buf, buf + n);
  std::fclose(f);
  if (!zamd::PngReducedFormatOk(v[2], v[3])) {
    std::printf("refused\n");
    return 1;
  }
  std::vector<unsigned char> png(zamd::kPngMaxPrefixBytes);
  const size_t prefix = zamd::PngPrefixReduced(v[0], v[1], v[2], v[3], palette.data(), static_cast<uint32_t>(palette.size() / 4), v[4] != 0,
                                               v[5], v[6], v[7], png.data());
  png.resize(prefix);
  png.insert(png.end(), zlib.begin(), zlib.end());
  unsigned char trailer[zamd::kPngTrailerBytes];
  if (!zamd::PngCloseAt(png.data(), png.size(), prefix, trailer)) {
    std::printf("refused\n");
    return 1;
  }
  png.insert(png.end(), trailer, trailer + sizeof(trailer));
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(png.data(), 1, png.size(), o) != png.size()) return 2;
  std::fclose(o);
  std::printf("ok %zu %zu\n", png.size(), prefix);
  return 0;
}
