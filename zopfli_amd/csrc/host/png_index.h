// The zmx_png_index_* entries' host part: what zopflipng and LodePNG make of a palette or low-bit grey PNG, derived from
// the image's header, its palette and the first-appearance table of k_png_index_use (device/zmx_png_index.h) — no pixel
// is looked at.  zopflipng decodes such a file to RGBA8 (index i becomes palette[i], a grey value v at depth b becomes
// v * 255 / (2^b - 1) three times with alpha 255), so a grey image is an index image with the ramp as its palette, and
//   - LodePNG's colour statistics of the expansion are the statistics of the entries that are used, a colour's first
//     appearance being the smallest among the indices that carry it;
//   - --lossy_transparent (zopflipng_lib.cc LossyOptimizeTransparent) is always its palette mode — at most 256 colours —:
//     every used entry with alpha 0 gets the RGB of the one whose first pixel comes first;
//   - any output mode is a table of 256 entries for k_png_index_convert;
//   - the file of --keepcolortype keeps the input's mode and palette, in the input's order, unused entries included;
//     only after --lossy_transparent is the palette shrunk to the entries whose own colour still occurs (:137-155).
// Host arithmetic only — nothing of the library — so a plain C++ program runs it (tests/hostlib/png_index_print.cc).
#ifndef ZOPFLI_AMD_PNG_INDEX_H_
#define ZOPFLI_AMD_PNG_INDEX_H_

#include <cstdint>
#include <cstring>

#include "zopfli_amd.h"

namespace zamd {

constexpr uint64_t kPngIndexUnused = ~0ull;   // first[v] of a value no pixel has

// what the index entries take: a palette at 1, 2, 4 or 8 bits, grey at 1, 2 or 4
inline bool PngIndexFormatOk(uint32_t colortype, uint32_t bitdepth) {
  if (colortype == 3) return bitdepth == 1 || bitdepth == 2 || bitdepth == 4 || bitdepth == 8;
  return colortype == 0 && (bitdepth == 1 || bitdepth == 2 || bitdepth == 4);
}
// what they convert to (k_png_index_convert): a palette or grey at 1, 2, 4 or 8 bits; grey + alpha, RGB, RGBA at 8
inline bool PngIndexOutModeOk(uint32_t colortype, uint32_t bitdepth) {
  if (colortype == 0 || colortype == 3) return bitdepth == 1 || bitdepth == 2 || bitdepth == 4 || bitdepth == 8;
  return (colortype == 2 || colortype == 4 || colortype == 6) && bitdepth == 8;
}
inline bool PngIndexPaletteSizeOk(const zmx_png_index_image& im) {
  return im.colortype != 3 || (im.palettesize >= 1 && im.palettesize <= (1u << im.bitdepth));
}

// The entries r, g, b, a the image's values stand for: its palette, or the grey ramp of its depth.
struct PngIndexPalette {
  uint32_t size;
  unsigned char rgba[1024];
};
inline void PngIndexPaletteOf(const zmx_png_index_image& im, PngIndexPalette* p) {
  std::memset(p, 0, sizeof(*p));
  if (im.colortype == 3) {
    p->size = im.palettesize;
    std::memcpy(p->rgba, im.palette, 4 * static_cast<size_t>(im.palettesize));
    return;
  }
  p->size = 1u << im.bitdepth;
  for (uint32_t v = 0; v < p->size; ++v) {
    const unsigned char g = static_cast<unsigned char>(v * 255u / (p->size - 1u));
    p->rgba[4 * v] = p->rgba[4 * v + 1] = p->rgba[4 * v + 2] = g;
    p->rgba[4 * v + 3] = 255;
  }
}

inline uint32_t PngIndexColor(const unsigned char* e) {
  return static_cast<uint32_t>(e[0]) | (static_cast<uint32_t>(e[1]) << 8) | (static_cast<uint32_t>(e[2]) << 16) | (static_cast<uint32_t>(e[3]) << 24);
}
inline bool PngIndexUsed(const PngIndexPalette& p, const uint64_t first[256], uint32_t i) { return i < p.size && first[i] != kPngIndexUnused; }

// The first pixel whose value has no entry, or kPngIndexUnused.
inline uint64_t PngIndexFirstOutside(const uint64_t first[256], uint32_t size) {
  uint64_t at = kPngIndexUnused;
  for (uint32_t v = size; v < 256; ++v) {
    if (first[v] < at) at = first[v];
  }
  return at;
}

// --lossy_transparent on the entries: the used ones with alpha 0 get the RGB of the first transparent pixel.
inline void PngIndexLossyTransparent(PngIndexPalette* p, const uint64_t first[256]) {
  uint32_t from = 256;
  for (uint32_t i = 0; i < p->size; ++i) {
    if (PngIndexUsed(*p, first, i) && p->rgba[4 * i + 3] == 0 && (from == 256 || first[i] < first[from])) from = i;
  }
  if (from == 256) return;
  unsigned char rgb[3];
  std::memcpy(rgb, p->rgba + 4 * from, 3);
  for (uint32_t i = 0; i < p->size; ++i) {
    if (PngIndexUsed(*p, first, i) && p->rgba[4 * i + 3] == 0) std::memcpy(p->rgba + 4 * i, rgb, 3);
  }
}

// lodepng.cpp getValueRequiredBits: what a grey value needs (device/zmx_png_color.h has it for the kernels)
inline uint32_t PngIndexValueBits(uint32_t v) {
  if (v == 0 || v == 255) return 1;
  if (v % 17 != 0) return 8;
  return v % 85 == 0 ? 2u : 4u;
}

// LodePNG's statistics (lodepng_compute_color_stats, its second loop for the key included) of the RGBA8 expansion of an
// image whose values stand for `p`'s entries: what zmx_png_color_stats_device gives for that expansion.
inline void PngIndexColorStats(const PngIndexPalette& p, const uint64_t first[256], zmx_png_color_stats* out) {
  std::memset(out, 0, sizeof(*out));
  uint32_t color[256];
  uint64_t born[256];
  uint32_t n = 0;
  for (uint32_t i = 0; i < p.size; ++i) {
    if (!PngIndexUsed(p, first, i)) continue;
    const uint32_t c = PngIndexColor(p.rgba + 4 * i);
    uint32_t k = 0;
    while (k < n && color[k] != c) ++k;
    if (k == n) {
      color[n] = c;
      born[n++] = first[i];
    } else if (first[i] < born[k]) {
      born[k] = first[i];
    }
  }
  // first-appearance order (insertion sort over at most 256 colours)
  for (uint32_t i = 1; i < n; ++i) {
    const uint32_t c = color[i];
    const uint64_t b = born[i];
    uint32_t at = i;
    for (; at > 0 && born[at - 1] > b; --at) {
      color[at] = color[at - 1];
      born[at] = born[at - 1];
    }
    color[at] = c;
    born[at] = b;
  }
  bool partial = false, transparent = false, two_rgbs = false;
  uint32_t key_rgb = 0, bits = 1;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t r = color[k] & 255u, g = (color[k] >> 8) & 255u, b = (color[k] >> 16) & 255u, a = color[k] >> 24;
    if (r != g || r != b) out->colored = 1;
    if (a != 0 && a != 255) partial = true;
    if (a == 0) {
      if (transparent && (color[k] & 0xffffffu) != key_rgb) two_rgbs = true;
      transparent = true;
      key_rgb = color[k] & 0xffffffu;
    }
    const uint32_t need = PngIndexValueBits(r);
    if (need > bits) bits = need;
  }
  bool clash = false;   // a pixel that is not transparent has the key's RGB
  for (uint32_t k = 0; k < n && transparent; ++k) {
    if ((color[k] >> 24) != 0 && (color[k] & 0xffffffu) == key_rgb) clash = true;
  }
  if (partial || (transparent && (two_rgbs || clash))) out->alpha = 1;
  else if (transparent) out->key = 1;
  if (out->key) {
    out->key_r = static_cast<uint16_t>((key_rgb & 255u) * 257u);
    out->key_g = static_cast<uint16_t>(((key_rgb >> 8) & 255u) * 257u);
    out->key_b = static_cast<uint16_t>(((key_rgb >> 16) & 255u) * 257u);
  }
  out->bits = (out->colored || out->alpha) && bits < 8 ? 8u : bits;
  out->numcolors = n;
  for (uint32_t k = 0; k < n; ++k) {
    for (int j = 0; j < 4; ++j) out->palette[4 * k + j] = static_cast<unsigned char>(color[k] >> (8 * j));
  }
}

// k_png_index_convert's table for `mode` (PngIndexOutModeOk): entry i is what LodePNG's rgba8ToPixel writes for p's
// entry i, the first byte lowest.  A palette pixel becomes the LATER of two equal entries of the mode's palette, as
// LodePNG's colour tree keeps the index added last; an entry whose colour the palette lacks (no pixel has it) gets 0.
inline void PngIndexTable(const PngIndexPalette& p, const zmx_png_color_mode& mode, uint32_t table[256]) {
  std::memset(table, 0, 256 * sizeof(uint32_t));
  for (uint32_t i = 0; i < p.size; ++i) {
    const unsigned char* e = p.rgba + 4 * i;
    uint32_t v = 0;
    if (mode.colortype == 3) {
      for (uint32_t j = 0; j < mode.palettesize && j < 256; ++j) {
        if (std::memcmp(mode.palette + 4 * j, e, 4) == 0) v = j;
      }
    } else if (mode.colortype == 0) {
      v = static_cast<uint32_t>(e[0]) >> (8u - mode.bitdepth);
    } else if (mode.colortype == 4) {
      v = static_cast<uint32_t>(e[0]) | (static_cast<uint32_t>(e[3]) << 8);
    } else if (mode.colortype == 2) {
      v = PngIndexColor(e) & 0xffffffu;
    } else {
      v = PngIndexColor(e);
    }
    table[i] = v;
  }
}

// What the --keepcolortype file is made of: the input's mode — its palette shrunk after --lossy_transparent to the
// entries whose own colour still occurs, where that leaves fewer colours than entries — and the table that maps the
// image's values into it: duplicates to the later index, the renumbering after a shrink.
inline void PngIndexKeepPlan(const zmx_png_index_image& im, const uint64_t first[256], bool lossy_transparent, zmx_png_color_mode* mode,
                             uint32_t table[256]) {
  std::memset(mode, 0, sizeof(*mode));
  mode->colortype = im.colortype;
  mode->bitdepth = im.bitdepth;
  PngIndexPalette p;
  PngIndexPaletteOf(im, &p);
  if (im.colortype != 3) {
    PngIndexTable(p, *mode, table);
    return;
  }
  PngIndexPalette seen = p;
  mode->palettesize = p.size;
  std::memcpy(mode->palette, p.rgba, 4 * static_cast<size_t>(p.size));
  if (lossy_transparent) {
    PngIndexLossyTransparent(&seen, first);
    zmx_png_color_stats stats;
    PngIndexColorStats(seen, first, &stats);
    if (stats.numcolors < p.size) {
      uint32_t kept = 0;
      for (uint32_t i = 0; i < p.size; ++i) {
        bool occurs = false;
        for (uint32_t k = 0; k < stats.numcolors && !occurs; ++k) occurs = std::memcmp(stats.palette + 4 * k, p.rgba + 4 * i, 4) == 0;
        if (occurs) std::memcpy(mode->palette + 4 * kept++, p.rgba + 4 * i, 4);
      }
      std::memset(mode->palette + 4 * kept, 0, 4 * static_cast<size_t>(256 - kept));
      mode->palettesize = kept;
    }
  }
  PngIndexTable(seen, *mode, table);
}

}  // namespace zamd

#endif  // ZOPFLI_AMD_PNG_INDEX_H_
