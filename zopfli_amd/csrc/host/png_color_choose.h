// zmx_png_choose_color: LodePNG's auto_choose_color (lodepng.cpp) on the statistics of zmx_png_color_stats_device, and
// the mode of zopflipng's second try at small palette files (zopflipng_lib.cc TryOptimize).  Host arithmetic only —
// nothing of the library — so a plain C++ program runs it (tests/hostlib/png_color_print.cc).
#ifndef ZOPFLI_AMD_PNG_COLOR_CHOOSE_H_
#define ZOPFLI_AMD_PNG_COLOR_CHOOSE_H_

#include <cstdint>
#include <cstring>

#include "zopfli_amd.h"

namespace zamd {

// The smallest colour mode that holds every colour the statistics speak of.
inline void PngChooseColor(const zmx_png_color_stats& stats, uint64_t numpixels, zmx_png_color_mode* mode) {
  std::memset(mode, 0, sizeof(*mode));
  bool alpha = stats.alpha != 0, key = stats.key != 0;
  uint32_t bits = stats.bits;
  if (key && numpixels <= 16) {   // too few pixels to pay for a tRNS chunk
    alpha = true;
    key = false;
    if (bits < 8) bits = 8;
  }
  const bool gray_ok = stats.colored == 0;
  if (!gray_ok && bits < 8) bits = 8;
  const uint64_t n = stats.numcolors;
  const uint32_t palettebits = n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8;
  bool palette_ok = n <= 256 && bits <= 8 && n != 0;
  if (numpixels < n * 2) palette_ok = false;                          // the palette would cost more than it saves
  if (gray_ok && !alpha && bits <= palettebits) palette_ok = false;   // grey costs less
  if (palette_ok) {
    mode->colortype = 3;
    mode->bitdepth = palettebits;
    mode->palettesize = static_cast<uint32_t>(n);
    std::memcpy(mode->palette, stats.palette, 4 * n);
    return;
  }
  mode->bitdepth = bits;
  mode->colortype = alpha ? (gray_ok ? 4 : 6) : (gray_ok ? 0 : 2);
  if (key) {
    const uint32_t mask = (1u << bits) - 1u;   // (the statistics keep 16-bit values)
    mode->key_defined = 1;
    mode->key_r = static_cast<uint16_t>(stats.key_r & mask);
    mode->key_g = static_cast<uint16_t>(stats.key_g & mask);
    mode->key_b = static_cast<uint16_t>(stats.key_b & mask);
  }
}

// What zopflipng tries as well when the palette file came out below kPngRetryBelow bytes: RGB or RGBA at 8 bits, never
// grey, with the key where there is one on more than 16 pixels.
constexpr size_t kPngRetryBelow = 4096;
inline void PngRetryMode(const zmx_png_color_stats& stats, uint64_t numpixels, zmx_png_color_mode* mode) {
  std::memset(mode, 0, sizeof(*mode));
  const bool alpha = stats.alpha != 0 || (numpixels <= 16 && stats.key != 0);
  mode->colortype = alpha ? 6 : 2;
  mode->bitdepth = 8;
  if (stats.key != 0 && !alpha) {
    mode->key_defined = 1;
    mode->key_r = stats.key_r & 255u;
    mode->key_g = stats.key_g & 255u;
    mode->key_b = stats.key_b & 255u;
  }
}

// What the convert entries take: the pairs of colour type and depth PNG has, a palette of 1 .. 2^depth entries, 16 bits
// only from a 16-bit image.
inline bool PngModeOk(const zmx_png_color_mode& mode, uint32_t in_bitdepth) {
  const uint32_t d = mode.bitdepth;
  if (d == 16 && in_bitdepth != 16) return false;
  switch (mode.colortype) {
    case 0: return d == 1 || d == 2 || d == 4 || d == 8 || d == 16;
    case 2: case 4: case 6: return d == 8 || d == 16;
    case 3: return (d == 1 || d == 2 || d == 4 || d == 8) && mode.palettesize >= 1 && mode.palettesize <= (1u << d);
    default: return false;
  }
}

}  // namespace zamd

#endif  // ZOPFLI_AMD_PNG_COLOR_CHOOSE_H_
