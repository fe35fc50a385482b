// zmx_png_source (include/zopfli_amd.h): what is refused of one without asking the runtime, its packed image's mode and
// size, its extent — the bytes from the lowest to one past the highest any sample touches, by the signs of the three
// strides.  No HIP, no globals: the device layer (device/drv_png_pack.h), the entries (png_encode.cc) and a plain C++
// program (tests/hostlib/png_source_print.cc) run the same functions.  (The record k_png_pack reads is made of a checked
// source by device/zmx_png_pack.h: PngPackSourceOf.)  A check returns the refusal's text behind `who` (entry_checks.h:
// Refusal), or an empty string.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "entry_checks.h"
#include "zopfli_amd.h"

namespace zamd {

inline bool PngSourceSampleOk(uint32_t sample) { return sample <= ZMX_PNG_SAMPLE_F32; }
inline uint32_t PngSourceSampleBytes(uint32_t sample) { return sample == ZMX_PNG_SAMPLE_U8 ? 1u : sample == ZMX_PNG_SAMPLE_F32 ? 4u : 2u; }
inline uint32_t PngSourceColorType(uint32_t channels) { return channels == 1 ? 0u : channels == 2 ? 4u : channels == 3 ? 2u : 6u; }

// The offsets of the extent from d_data: [*lo, *hi), *lo <= 0 < *hi.  False where they overflow 64 bits.  S: zmx_png_source
// or zmx_png_sink (host/png_sink.h), which has the same fields.
template <class S>
inline bool PngSourceExtent(const S& s, int64_t* lo, int64_t* hi) {
  const int64_t stride[3] = {s.stride_y, s.stride_x, s.stride_c};
  const int64_t last[3] = {static_cast<int64_t>(s.height) - 1, static_cast<int64_t>(s.width) - 1, static_cast<int64_t>(s.channels) - 1};
  int64_t l = 0, h = 0;
  for (int d = 0; d < 3; ++d) {
    int64_t reach = 0;
    if (__builtin_mul_overflow(stride[d], last[d], &reach)) return false;
    if (__builtin_add_overflow(reach < 0 ? l : h, reach, reach < 0 ? &l : &h)) return false;
  }
  if (__builtin_add_overflow(h, static_cast<int64_t>(PngSourceSampleBytes(s.sample)), &h)) return false;
  *lo = l;
  *hi = h;
  return true;
}

struct PngSourcePlan {
  zmx_png_image image;   // the packed image's mode, d_pixels null
  size_t nbytes;         // its size
  uintptr_t lo, hi;      // the extent as addresses
};

// What a source and a sink (host/png_sink.h) are refused for alike, in the order the header lists it, and the extent as
// addresses in [*ext_lo, *ext_hi).  S: zmx_png_source or zmx_png_sink; `sink` chooses the words for the two refused
// type/depth pairs and leaves out the packed row's limit, which a sink has none of.
template <class S>
inline std::string CheckPngStrided(const char* who, const S* s, bool sink, uintptr_t* ext_lo, uintptr_t* ext_hi) {
  if (!s) return Refusal(who, "null argument");
  if (s->width == 0 || s->height == 0) return Refusal(who, "width or height 0");
  if (s->channels < 1 || s->channels > 4) return Refusal(who, std::to_string(s->channels) + " channels (1 .. 4 are taken)");
  if (!PngSourceSampleOk(s->sample)) return Refusal(who, "unknown sample type " + std::to_string(s->sample));
  if (s->bitdepth != 8 && s->bitdepth != 16) return Refusal(who, "a bit depth of " + std::to_string(s->bitdepth) + " (8 or 16)");
  if (s->sample == ZMX_PNG_SAMPLE_U8 && s->bitdepth == 16) {
    return Refusal(who, sink ? "16-bit values are not narrowed to 8-bit samples" : "8-bit samples are not widened to 16 bits");
  }
  if (s->sample == ZMX_PNG_SAMPLE_U16 && s->bitdepth == 8) {
    return Refusal(who, sink ? "8-bit values are not widened to 16-bit samples"
                             : "16-bit samples are not narrowed to 8 bits (ZMX_PNG_LOSSY_8BIT of the optimize entries does that)");
  }
  uint32_t seen = 0;
  for (uint32_t k = 0; k < s->channels; ++k) {
    if (s->order[k] >= s->channels || (seen & (1u << s->order[k]))) return Refusal(who, "order is no permutation of the channels");
    seen |= 1u << s->order[k];
  }
  if (!s->d_data) return Refusal(who, "null pointer");
  const int64_t ssz = PngSourceSampleBytes(s->sample);
  if (reinterpret_cast<uintptr_t>(s->d_data) % static_cast<uintptr_t>(ssz) != 0 || s->stride_y % ssz != 0 || s->stride_x % ssz != 0 ||
      s->stride_c % ssz != 0) {
    return Refusal(who, "d_data or a stride is no multiple of the sample's size, " + std::to_string(ssz));
  }
  const uint64_t rowbytes = static_cast<uint64_t>(s->width) * s->channels * (s->bitdepth / 8);
  if (!sink && rowbytes > 0x7fffffffu) return Refusal(who, "a row of 2^31 bytes or more");
  int64_t lo = 0, hi = 0;
  const uintptr_t base = reinterpret_cast<uintptr_t>(s->d_data);
  if (!PngSourceExtent(*s, &lo, &hi) || 0 - static_cast<uint64_t>(lo) > base || static_cast<uint64_t>(hi) > UINT64_MAX - base) {
    return Refusal(who, "the extent overflows 64 bits");
  }
  *ext_lo = base - (0 - static_cast<uint64_t>(lo));
  *ext_hi = base + static_cast<uint64_t>(hi);
  return std::string();
}

// Everything of section "refused before any launch" that needs no device.
inline std::string CheckPngSource(const char* who, const zmx_png_source* s, PngSourcePlan* plan) {
  uintptr_t ext_lo = 0, ext_hi = 0;
  const std::string msg = CheckPngStrided(who, s, false, &ext_lo, &ext_hi);
  if (!msg.empty()) return msg;
  const uint64_t rowbytes = static_cast<uint64_t>(s->width) * s->channels * (s->bitdepth / 8);
  if (plan) {
    plan->image.d_pixels = nullptr;
    plan->image.width = s->width;
    plan->image.height = s->height;
    plan->image.colortype = PngSourceColorType(s->channels);
    plan->image.bitdepth = s->bitdepth;
    plan->nbytes = static_cast<size_t>(rowbytes * s->height);
    plan->lo = ext_lo;
    plan->hi = ext_hi;
  }
  return std::string();
}

}  // namespace zamd
