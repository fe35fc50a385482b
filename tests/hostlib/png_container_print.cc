// host/png_container.h as a plain C++ program (tests/test_cpu_png_container.py): the PNG file around a zlib stream.
//   png_container_print ZLIB OUT WIDTH HEIGHT COLORTYPE BITDEPTH [PIECE]
// PIECE: the least share of a thread in the IDAT's CRC-32 (the library's: 1 MiB), so that a small stream takes the
// threaded path as well.
// ZLIB: a stream as ZopfliCompress(ZOPFLI_FORMAT_ZLIB) writes it (78 DA ...).  The file is written to OUT; prints
// "ok BYTES BYTEWIDTH LINEBYTES", or "refused" (exit status 1) when PngFormatOk or PngAssemble says no.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "png_container.h"

int main(int argc, char** argv) {
  if (argc != 7 && argc != 8) {
    std::fprintf(stderr, "usage: png_container_print ZLIB OUT WIDTH HEIGHT COLORTYPE BITDEPTH [PIECE]\n");
    return 2;
  }
  const uint32_t width = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  const uint32_t height = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
  const uint32_t colortype = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  const uint32_t bitdepth = static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10));
  const size_t piece = argc == 8 ? std::strtoull(argv[7], nullptr, 10) : zamd::kPngCrcPiece;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<unsigned char> zlib;
  unsigned char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) != 0;) zlib.insert(zlib.end(), buf, buf + n);
  std::fclose(f);
  const std::vector<unsigned char> before = zlib;
  std::vector<unsigned char> png;
  if (!zamd::PngFormatOk(colortype, bitdepth) ||
      !zamd::PngAssemble(width, height, colortype, bitdepth, zlib.data(), zlib.size(), &png, piece)) {
    std::printf("refused\n");
    return 1;
  }
  if (zlib != before) {
    std::printf("the stream changed\n");
    return 1;
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(png.data(), 1, png.size(), o) != png.size()) return 2;
  std::fclose(o);
  std::printf("ok %zu %zu %zu\n", png.size(), zamd::PngByteWidth(colortype, bitdepth), zamd::PngLineBytes(width, colortype, bitdepth));
  return 0;
}
