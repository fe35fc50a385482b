// The rules of device/zmx_png_color.h and host/png_color_choose.h on the CPU: the __host__ __device__ functions
// k_png_color_stats, k_png_color_key and k_png_convert are made of, run by a plain C++ program, the threads of a launch
// one after the other (tests/test_cpu_png_color_cases.py).
//   png_color_print IN OUT SRC_MOD DST_MOD WIDTH HEIGHT COLORTYPE BITDEPTH auto|retry
// IN: the image's bytes.  It lies at SRC_MOD (0 .. 15) bytes into a heap block of its own that ends with its last byte (a
// read beyond it is the sanitizer's to find).  The statistics are taken (the workgroups in falling order when DST_MOD is
// odd: the result may not depend on who comes first), the mode chosen — `retry`: the mode of zopflipng's second try — and
// the image converted to it at DST_MOD bytes behind a 16-byte boundary, with 64 guard bytes of 0xA5 on both sides.  The
// converted image is written to OUT.  Prints
//   ok COLORED KEY ALPHA NUMCOLORS BITS KEY_R KEY_G KEY_B | COLORTYPE BITDEPTH PALETTESIZE KEY_DEFINED KEY_R KEY_G KEY_B |
//      ROWBYTES STATS_GRID CONVERT_GRID BAD_PIXEL | PALETTE (hex, 4 * min(NUMCOLORS, 256) bytes, or -)
// or what is wrong (exit status 1).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "png_color_choose.h"
#include "zmx_png_color.h"

namespace {
constexpr size_t kGuard = 64;

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}

// k_png_color_stats, workgroup by workgroup
void RunStats(const zamd::PngColorImage& I, zamd::PngColorState* state, bool falling) {
  const uint32_t groups = zamd::PngColorGrid(I);
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    zamd::PngColorSlot table[zamd::kPngColorSlots];
    uint32_t count = 0, stop = 0;
    const zamd::PngColorGroup grp{table, &count, &stop};
    for (uint32_t local = zamd::kPngColorThreads; local-- > 0;) zamd::PngColorGroupBegin(state, grp, local);
    zamd::PngColorAcc sum = zamd::PngColorAccNone();
    for (uint32_t local = 0; local < zamd::kPngColorThreads; ++local) {
      zamd::PngColorAcc acc = zamd::PngColorAccNone();
      zamd::PngColorStatsThread(I, state, grp, group, groups, falling ? zamd::kPngColorThreads - 1 - local : local, &acc);
      zamd::PngColorAccJoin(&sum, acc);
    }
    zamd::PngColorGroupEnd(state, sum, stop);
    for (uint32_t local = 0; local < zamd::kPngColorThreads; ++local) zamd::PngColorGroupFlush(state, grp, local);
  }
}

void RunConvert(const zamd::PngConvParams& P) {
  const uint32_t groups = zamd::PngConvGrid(P.rowbytes * P.in.height);
  const uint64_t threads = static_cast<uint64_t>(groups) * zamd::kPngColorThreads;
  for (uint32_t group = 0; group < groups; ++group) {
    zamd::PngColorSlot table[zamd::kPngColorSlots];
    for (uint32_t local = 0; local < zamd::kPngColorThreads; ++local) zamd::PngConvTableBegin(table, local);
    for (uint32_t local = 0; local < zamd::kPngColorThreads; ++local) zamd::PngConvTableFill(P, table, local);
    for (uint32_t local = 0; local < zamd::kPngColorThreads; ++local) {
      zamd::PngConvRun(P, table, static_cast<uint64_t>(group) * zamd::kPngColorThreads + local, threads);
    }
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: png_color_print IN OUT SRC_MOD DST_MOD WIDTH HEIGHT COLORTYPE BITDEPTH auto|retry\n");
    return 2;
  }
  const uint64_t src_mod = std::strtoull(argv[3], nullptr, 10), dst_mod = std::strtoull(argv[4], nullptr, 10);
  const uint32_t width = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10)), height = static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10));
  const uint32_t colortype = static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10)), bitdepth = static_cast<uint32_t>(std::strtoul(argv[8], nullptr, 10));
  const bool retry = std::string(argv[9]) == "retry";
  if (src_mod > 15 || dst_mod > 15 || width == 0 || height == 0) return 2;
  if (!(colortype == 0 || colortype == 2 || colortype == 4 || colortype == 6) || !(bitdepth == 8 || bitdepth == 16)) return 2;
  const uint64_t numpixels = static_cast<uint64_t>(width) * height;
  const uint64_t nbytes = numpixels * zamd::PngColorPixelBytes(colortype, bitdepth);

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

  zamd::PngColorImage I;
  I.pixels = image;
  I.numpixels = numpixels;
  I.width = width;
  I.height = height;
  I.colortype = colortype;
  I.bitdepth = bitdepth;

  zamd::PngColorState state;
  std::memset(&state, 0, offsetof(zamd::PngColorState, key_min));
  std::memset(reinterpret_cast<unsigned char*>(&state) + offsetof(zamd::PngColorState, key_min), 0xff,
              sizeof(state) - offsetof(zamd::PngColorState, key_min));
  RunStats(I, &state, (dst_mod & 1) != 0);
  if (zamd::PngColorWantsKeyPass(state)) {
    const uint64_t threads = static_cast<uint64_t>(zamd::PngColorGrid(I)) * zamd::kPngColorThreads;
    for (uint64_t thread = 0; thread < threads; ++thread) {
      if (zamd::PngColorKeyThread(I, state.key_min, thread, threads)) state.key_clash = 1;
    }
  }
  zamd::PngColorSummary sum;
  zamd::PngColorFinish(state, bitdepth, &sum);
  zmx_png_color_stats stats;
  static_assert(sizeof(stats) == sizeof(sum), "PngColorSummary is zmx_png_color_stats");
  std::memcpy(&stats, &sum, sizeof(stats));
  zmx_png_color_mode mode;
  if (retry) zamd::PngRetryMode(stats, numpixels, &mode);
  else zamd::PngChooseColor(stats, numpixels, &mode);
  if (!zamd::PngModeOk(mode, bitdepth)) return Bad("the chosen mode is none", mode.colortype);

  const uint64_t rowbytes = zamd::PngConvRowBytes(width, mode.colortype, mode.bitdepth), total = rowbytes * height;
  const uint64_t dst_size = kGuard + dst_mod + total + kGuard;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, dst_size) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::memset(dst_block, 0xA5, dst_size);
  unsigned char* dst = dst_block + kGuard + dst_mod;
  uint32_t bad_pixel = zamd::kPngColorNoBadPixel;
  zamd::PngConvParams P;
  P.in = I;
  P.out = dst;
  P.rowbytes = rowbytes;
  P.colortype = mode.colortype;
  P.bitdepth = mode.bitdepth;
  P.palettesize = mode.colortype == 3 ? mode.palettesize : 0;
  P.palette = mode.palette;
  P.bad_pixel = &bad_pixel;
  RunConvert(P);

  int rc = 0;
  for (uint64_t j = 0; j < kGuard + dst_mod && !rc; ++j) if (dst_block[j] != 0xA5) rc = Bad("written before the output", j);
  for (uint64_t j = 0; j < kGuard && !rc; ++j) if (dst[total + j] != 0xA5) rc = Bad("written behind the output", j);
  if (!rc && std::memcmp(image, image_before.data(), nbytes) != 0) rc = Bad("the image changed", 0);
  for (uint64_t j = 0; j < src_mod && !rc; ++j) if (block[j] != 0x5A) rc = Bad("written in front of the image", j);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  if (total && std::fwrite(dst, 1, total, o) != total) return 2;
  std::fclose(o);
  if (!rc) {
    std::printf("ok %u %u %u %u %u %u %u %u | %u %u %u %u %u %u %u | %" PRIu64 " %u %u %" PRId64 " | ", stats.colored, stats.key, stats.alpha,
                stats.numcolors, stats.bits, stats.key_r, stats.key_g, stats.key_b, mode.colortype, mode.bitdepth, mode.palettesize,
                mode.key_defined, mode.key_r, mode.key_g, mode.key_b, rowbytes, zamd::PngColorGrid(I), zamd::PngConvGrid(total),
                bad_pixel == zamd::kPngColorNoBadPixel ? static_cast<int64_t>(-1) : static_cast<int64_t>(bad_pixel));
    const uint32_t shown = stats.numcolors > 256 ? 0 : stats.numcolors;
    if (shown == 0) std::printf("-");
    for (uint32_t k = 0; k < 4 * shown; ++k) std::printf("%02x", stats.palette[k]);
    std::printf("\n");
  }
  std::free(block);
  std::free(dst_block);
  return rc;
}
