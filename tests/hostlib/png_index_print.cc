// The rules of device/zmx_png_index.h and host/png_index.h on the CPU: the __host__ __device__ functions k_png_index_use and
// k_png_index_convert are made of, run by a plain C++ program, the threads of a launch one after the other
// (tests/test_cpu_png_index_cases.py).
//   png_index_print IN OUT SRC_MOD DST_MOD WIDTH HEIGHT COLORTYPE BITDEPTH PALETTE_HEX LOSSY keep|optimize|retry
// IN: the image's bytes.  It lies at SRC_MOD (0 .. 15) bytes into a heap block of its own that ends with its last byte (a
// read beyond it is the sanitizer's to find).  k_png_index_use's workgroups run in falling order when DST_MOD is odd: the
// table may not depend on who comes first.  Then the host step: the statistics of the expansion (after --lossy_transparent
// where LOSSY is 1), the mode — the input's own (keep), LodePNG's choice (optimize) or zopflipng's second try (retry) — and
// the table into it; and k_png_index_convert at DST_MOD bytes behind a 16-byte boundary, with 64 guard bytes of 0xA5 on
// both sides.  The converted rows are written to OUT.  Prints
//   first F0 .. F255                                   (-1: no pixel has the value)
//   outside N                                          (the first pixel with a value the palette lacks; -1: none)
//   stats COLORED KEY ALPHA NUMCOLORS BITS KEY_R KEY_G KEY_B PALETTE_HEX|-
//   mode COLORTYPE BITDEPTH PALETTESIZE KEY_DEFINED KEY_R KEY_G KEY_B PALETTE_HEX|-
//   table T0 .. T255
//   bad N                                              (what the convert kernel reported; -1: nothing)
//   ok GRID_USE GRID_CONVERT
// or what is wrong (exit status 1).  With a value outside the palette only the first two lines, `bad` (the kernel run with
// the keep mode's table) and ok are printed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "png_color_choose.h"
#include "png_index.h"
#include "zmx_png_index.h"

namespace {
constexpr size_t kGuard = 64;
using namespace zamd;

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}

// k_png_index_use, workgroup by workgroup
void RunUse(const PngIndexImage& I, uint32_t* first, bool falling) {
  const uint32_t groups = PngIndexGrid(I.height * I.linebytes);
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    uint32_t table[kPngIndexValues];
    for (uint32_t local = 0; local < kPngIndexThreads; ++local) PngIndexGroupBegin(table, local);
    for (uint32_t k = 0; k < kPngIndexThreads; ++k) {
      const uint32_t local = falling ? kPngIndexThreads - 1 - k : k;
      PngIndexUseRun(I, table, static_cast<uint64_t>(group) * kPngIndexThreads + local, static_cast<uint64_t>(groups) * kPngIndexThreads);
    }
    for (uint32_t local = 0; local < kPngIndexThreads; ++local) PngIndexGroupFlush(table, first, local);
  }
}

// k_png_index_convert, workgroup by workgroup
void RunConvert(const PngIndexConvParams& P, bool falling) {
  const uint32_t groups = PngIndexGrid(P.in.height * P.rowbytes);
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    uint32_t table[kPngIndexValues];
    std::memcpy(table, P.table, sizeof(table));
    for (uint32_t local = 0; local < kPngIndexThreads; ++local) {
      PngIndexConvRun(P, table, static_cast<uint64_t>(group) * kPngIndexThreads + local, static_cast<uint64_t>(groups) * kPngIndexThreads);
    }
  }
}

void PrintHex(const unsigned char* p, size_t n) {
  if (n == 0) std::printf("-");
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 12) {
    std::fprintf(stderr, "usage: png_index_print IN OUT SRC_MOD DST_MOD WIDTH HEIGHT COLORTYPE BITDEPTH PALETTE_HEX LOSSY keep|optimize|retry\n");
    return 2;
  }
  const uint64_t src_mod = std::strtoull(argv[3], nullptr, 10), dst_mod = std::strtoull(argv[4], nullptr, 10);
  zmx_png_index_image im;
  std::memset(&im, 0, sizeof(im));
  im.width = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  im.height = static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10));
  im.colortype = static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10));
  im.bitdepth = static_cast<uint32_t>(std::strtoul(argv[8], nullptr, 10));
  const std::string hex = std::string(argv[9]) == "-" ? "" : argv[9];
  const bool lossy = std::strtoul(argv[10], nullptr, 10) != 0;
  const std::string what = argv[11];
  if (src_mod > 15 || dst_mod > 15 || im.width == 0 || im.height == 0 || hex.size() % 8 != 0 || hex.size() > 2048) return 2;
  im.palettesize = static_cast<uint32_t>(hex.size() / 8);
  for (size_t i = 0; i < hex.size() / 2; ++i) im.palette[i] = static_cast<unsigned char>(std::strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16));
  if (!PngIndexFormatOk(im.colortype, im.bitdepth) || !PngIndexPaletteSizeOk(im)) return 2;
  if (what != "keep" && what != "optimize" && what != "retry") return 2;

  PngIndexImage I;
  I.linebytes = PngIndexLineBytes(im.width, im.bitdepth);
  I.width = im.width;
  I.height = im.height;
  I.bitdepth = im.bitdepth;
  const uint64_t nbytes = I.linebytes * im.height;
  // (the block ends with the image's last byte)
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, src_mod + nbytes) != 0) return 2;
  unsigned char* block = static_cast<unsigned char*>(mem);
  std::memset(block, 0x5A, src_mod + nbytes);
  unsigned char* image = block + src_mod;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(image, 1, nbytes, f) != nbytes) return 2;
  std::fclose(f);
  const std::vector<unsigned char> image_before(image, image + nbytes);
  I.pixels = image;
  const bool falling = (dst_mod & 1) != 0;

  uint32_t first32[kPngIndexValues];
  std::memset(first32, 0xff, sizeof(first32));
  RunUse(I, first32, falling);
  uint64_t first[256];
  std::printf("first");
  for (uint32_t v = 0; v < 256; ++v) {
    first[v] = first32[v] == kPngIndexNone ? kPngIndexUnused : first32[v];
    std::printf(" %" PRId64, first32[v] == kPngIndexNone ? static_cast<int64_t>(-1) : static_cast<int64_t>(first32[v]));
  }
  std::printf("\n");

  PngIndexPalette seen;
  PngIndexPaletteOf(im, &seen);
  const uint64_t outside = PngIndexFirstOutside(first, seen.size);
  std::printf("outside %" PRId64 "\n", outside == kPngIndexUnused ? static_cast<int64_t>(-1) : static_cast<int64_t>(outside));

  zmx_png_color_mode mode;
  uint32_t table[256];
  if (outside != kPngIndexUnused) {
    // (the host refuses here; the kernel is run all the same, for what it reports)
    std::memset(&mode, 0, sizeof(mode));
    mode.colortype = im.colortype;
    mode.bitdepth = im.bitdepth;
    mode.palettesize = im.palettesize;
    std::memcpy(mode.palette, im.palette, sizeof(mode.palette));
    PngIndexTable(seen, mode, table);
  } else {
    if (lossy) PngIndexLossyTransparent(&seen, first);
    zmx_png_color_stats stats;
    PngIndexColorStats(seen, first, &stats);
    std::printf("stats %u %u %u %u %u %u %u %u ", stats.colored, stats.key, stats.alpha, stats.numcolors, stats.bits, stats.key_r, stats.key_g,
                stats.key_b);
    PrintHex(stats.palette, 4 * static_cast<size_t>(stats.numcolors));
    std::printf("\n");
    const uint64_t numpixels = static_cast<uint64_t>(im.width) * im.height;
    if (what == "keep") {
      PngIndexKeepPlan(im, first, lossy, &mode, table);
    } else {
      if (what == "optimize") PngChooseColor(stats, numpixels, &mode);
      else PngRetryMode(stats, numpixels, &mode);
      PngIndexTable(seen, mode, table);
    }
    if (!PngIndexOutModeOk(mode.colortype, mode.bitdepth)) return Bad("a mode the kernel does not write", mode.colortype);
    std::printf("mode %u %u %u %u %u %u %u ", mode.colortype, mode.bitdepth, mode.palettesize, mode.key_defined, mode.key_r, mode.key_g, mode.key_b);
    PrintHex(mode.palette, mode.colortype == 3 ? 4 * static_cast<size_t>(mode.palettesize) : 0);
    std::printf("\ntable");
    for (uint32_t v = 0; v < 256; ++v) std::printf(" %u", table[v]);
    std::printf("\n");
  }

  PngIndexConvParams P;
  P.in = I;
  P.rowbytes = PngConvRowBytes(im.width, mode.colortype, mode.bitdepth);
  P.colortype = mode.colortype;
  P.bitdepth = mode.bitdepth;
  P.palettesize = seen.size;
  P.table = table;
  uint32_t bad = kPngIndexNone;
  P.bad_pixel = &bad;
  const uint64_t total = P.rowbytes * im.height;
  const uint64_t dst_size = kGuard + dst_mod + total + kGuard;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, dst_size) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::memset(dst_block, 0xA5, dst_size);
  P.out = dst_block + kGuard + dst_mod;
  RunConvert(P, falling);
  std::printf("bad %" PRId64 "\n", bad == kPngIndexNone ? static_cast<int64_t>(-1) : static_cast<int64_t>(bad));

  int rc = 0;
  for (uint64_t j = 0; j < kGuard + dst_mod && !rc; ++j) if (dst_block[j] != 0xA5) rc = Bad("written before the output", j);
  for (uint64_t j = 0; j < kGuard && !rc; ++j) if (dst_block[kGuard + dst_mod + total + j] != 0xA5) rc = Bad("written behind the output", j);
  if (!rc && std::memcmp(image, image_before.data(), nbytes) != 0) rc = Bad("the image changed", 0);
  for (uint64_t j = 0; j < src_mod && !rc; ++j) if (block[j] != 0x5A) rc = Bad("written in front of the image", j);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  if (total && std::fwrite(P.out, 1, total, o) != total) return 2;
  std::fclose(o);
  if (!rc) std::printf("ok %u %u\n", PngIndexGrid(nbytes), PngIndexGrid(total));
  std::free(block);
  std::free(dst_block);
  return rc;
}
