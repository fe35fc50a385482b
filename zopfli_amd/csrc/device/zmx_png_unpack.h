// zmx_png_unpack_device: the inverse of zmx_png_pack.h — an image's pixels in the file's own mode, as ZMX_PNG_DECODE_OWN
// lays them out (whole-byte rows, 16-bit samples high byte first), into what a GPU program holds: a strided, planar,
// swizzled, typed sink.  Sample (y, x, c) of a sink goes to data + y * stride_y + x * stride_x + c * stride_c (bytes, any
// sign, never 0 where the extent is above 1); PNG channel k of a pixel goes to sink channel order[k].
//   k_png_unpack  ONE launch for n images, at most kPngUnpackMaxBlocks workgroups.  An image is cut into tiles of
//                 kPngUnpackTilePixels consecutive pixels in row-major order; the tiles of all images are numbered one
//                 after the other, a workgroup strides over that number and finds its tile's image by binary search over
//                 the prefix of tile counts (PngPackSourceOfTile, as k_png_pack and k_bitjoin_many do).  No workgroup
//                 waits for another.  The mode of an image — colour type, depth, the key — comes from its job; the
//                 256-entry RGBA palette of a colour type 3 image is uploaded with the table and staged in LDS by the
//                 workgroup for the tile in hand.  A thread takes runs of kPngUnpackRun consecutive pixels, neighbouring
//                 lanes neighbouring runs.  Three store paths, chosen per sink on the host (PngPackPathOf, the source's
//                 rule):
//                   interleaved  stride_c = the sample's size, stride_x = channels * that, order the identity (or one
//                                channel with stride_x = the sample's size): a run's samples are one run of the sink's
//                                row, stored as 16-byte vectors where its address allows, 8-byte pairs, words or samples
//                                where not.
//                   planar       stride_x = the sample's size, any stride_c, any order: each plane's 8 samples are one
//                                run, stored as wide as its address allows; neighbouring lanes write neighbouring
//                                addresses of a plane.
//                   scalar       everything else, and in the other two every run that crosses a row's end or is not
//                                whole: a store per sample, merely correct.
//                 The input of a whole run at 8 bits a sample or more is loaded as 16-byte vectors or words where its
//                 address allows; below 8 bits a byte load a pixel.
//   the value     include/zopfli_amd.h has the text: lodepng_convert's value v from the file's mode into (the sink's
//                 colour type, its bitdepth) — 16 to 16 the values themselves with the key compared at full depth,
//                 everything else the RGBA8 value of PngRgba8Wide / PngRgba8Narrow, replicated (v * 257) at 16 bits,
//                 grey from colour the R value —; U8 and U16 store v, F32 fl32(v) / maxv by ONE correctly rounded
//                 division, F16 and BF16 that quotient rounded to nearest-even.
// Every byte of every sample is written exactly once, no other byte, the input never.  The rules are __host__ __device__
// functions and templates over `Par`, whose NoteWrite a CPU program (tests/hostlib/png_sink_print.cc) counts the stores
// with while it runs the very code of the kernel, the threads one after the other.  This header compiles without HIP; the
// kernel is there for the device layer only (ZMX_PNG_UNPACK_KERNELS).  Plain loads and stores, nothing else.
#ifndef ZMX_PNG_UNPACK_H_
#define ZMX_PNG_UNPACK_H_

#include <stddef.h>
#include <stdint.h>

#include "zmx_png_decode.h"   // PngRgba8Wide, PngRgba8Narrow, PngWalkRecord, PngLineBytes
#include "zmx_png_pack.h"     // the sample types, PngPackPathOf, PngPackSourceOfTile, the workgroup's size and the grid's cap

// (a run's values and words are arrays with constant indices only while every function that takes them is inlined: then
// they are registers, else scratch memory)
#if defined(__HIP_DEVICE_COMPILE__)
#define ZMX_PNGU_HD __host__ __device__ __attribute__((always_inline))
#else
#define ZMX_PNGU_HD ZMX_PD_HD
#endif

namespace zamd {

constexpr uint32_t kPngUnpackThreads = kPngPackThreads;       // a workgroup: four waves
constexpr uint32_t kPngUnpackMaxBlocks = kPngPackMaxBlocks;
constexpr uint32_t kPngUnpackRun = 8;                         // consecutive pixels a thread takes at a time
constexpr uint32_t kPngUnpackTilePixels = 4096;               // two runs a thread: a 64 x 64 icon is one tile

// One image and its sink, as the kernel reads them (made on the host: PngUnpackJobOf).
struct PngUnpackJob {
  const unsigned char* own;              // height rows of linebytes bytes
  unsigned char* data;                   // sample (0, 0, 0) of the sink
  int64_t stride_y, stride_x, stride_c;  // bytes
  uint64_t npixels, linebytes;
  uint32_t width, height, channels, sample, bitdepth, path;   // the sink's
  uint32_t colortype, depth, bytewidth;                       // the pixels' mode; bytes a pixel, 0 below 8 bits
  uint32_t has_key, key_r, key_g, key_b;
  uint32_t palette;                      // which 256 words of the table's palettes (colour type 3)
  uint8_t order[4];
  uint32_t reserved;
};

struct PngUnpackTable {
  const PngUnpackJob* jobs;     // [n]
  const uint64_t* tile_start;   // [n + 1], ascending: the number of image i's first tile
  const uint32_t* palettes;     // [palettes][256]: r | g << 8 | b << 16 | a << 24, 0xff000000 at and above palettesize
  uint64_t n;
};

// The record of a checked sink (host/png_sink.h) for pixels of `mode` at `own`.  Sink: zmx_png_sink, Mode:
// zmx_png_decode_result (its width and height are the sink's: the host has compared them).
template <class Sink, class Mode>
inline PngUnpackJob PngUnpackJobOf(const Sink& s, const Mode& mode, const void* own, uint32_t palette) {
  PngUnpackJob r;
  r.own = static_cast<const unsigned char*>(own);
  r.data = static_cast<unsigned char*>(s.d_data);
  r.stride_y = s.stride_y;
  r.stride_x = s.stride_x;
  r.stride_c = s.stride_c;
  r.npixels = static_cast<uint64_t>(s.width) * s.height;
  r.linebytes = PngLineBytes(mode.width, PngBpp(mode.colortype, mode.bitdepth));
  r.width = s.width;
  r.height = s.height;
  r.channels = s.channels;
  r.sample = s.sample;
  r.bitdepth = s.bitdepth;
  for (int k = 0; k < 4; ++k) r.order[k] = static_cast<uint32_t>(k) < s.channels ? s.order[k] : 0;
  r.path = PngPackPathOf(s.stride_x, s.stride_c, s.channels, s.sample, r.order);
  r.colortype = mode.colortype;
  r.depth = mode.bitdepth;
  r.bytewidth = mode.bitdepth < 8 ? 0 : PngBpp(mode.colortype, mode.bitdepth) / 8;
  r.has_key = mode.has_key;
  r.key_r = mode.key_r;
  r.key_g = mode.key_g;
  r.key_b = mode.key_b;
  r.palette = palette;
  r.reserved = 0;
  return r;
}

// The 256 words of a mode's palette: its r, g, b, a bytes, and 0, 0, 0, 255 at and above palettesize.
template <class Mode>
inline void PngUnpackPaletteOf(const Mode& mode, uint32_t* out) {
  for (uint32_t i = 0; i < 256; ++i) {
    if (i >= mode.palettesize) { out[i] = 0xff000000u; continue; }
    const unsigned char* p = mode.palette + 4 * i;
    out[i] = p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
  }
}

ZMX_PD_HD inline uint64_t PngUnpackTiles(uint64_t npixels) { return (npixels + kPngUnpackTilePixels - 1) / kPngUnpackTilePixels; }
ZMX_PD_HD inline uint32_t PngUnpackGrid(uint64_t ntiles) {
  return static_cast<uint32_t>(ntiles == 0 ? 1 : ntiles < kPngUnpackMaxBlocks ? ntiles : kPngUnpackMaxBlocks);
}

// ---- values
// 16-bit sample k of a group whose bytes lie first in the low byte
ZMX_PD_HD inline uint32_t PngUnpackBe16(uint64_t g, uint32_t k) {
  return ((static_cast<uint32_t>(g >> (16 * k)) & 255u) << 8) | (static_cast<uint32_t>(g >> (16 * k + 8)) & 255u);
}

// The integer values of one pixel for a sink of `channels` channels at `outdepth` bits, v[k] for PNG channel k.  g: the
// pixel's bytes, the first in the low byte; below 8 bits the pixel's value.
ZMX_PNGU_HD inline void PngUnpackValues(const PngWalkRecord& R, uint32_t channels, uint32_t outdepth, uint64_t g, const uint32_t* palette, uint32_t* v) {
  uint32_t r, gr, b, a;
  if (R.bitdepth == 16 && outdepth == 16) {
    switch (R.colortype) {
      case 0:
        r = gr = b = PngUnpackBe16(g, 0);
        a = R.has_key && r == R.key_r ? 0u : 65535u;
        break;
      case 2:
        r = PngUnpackBe16(g, 0);
        gr = PngUnpackBe16(g, 1);
        b = PngUnpackBe16(g, 2);
        a = R.has_key && r == R.key_r && gr == R.key_g && b == R.key_b ? 0u : 65535u;
        break;
      case 4:
        r = gr = b = PngUnpackBe16(g, 0);
        a = PngUnpackBe16(g, 1);
        break;
      default:
        r = PngUnpackBe16(g, 0);
        gr = PngUnpackBe16(g, 1);
        b = PngUnpackBe16(g, 2);
        a = PngUnpackBe16(g, 3);
        break;
    }
  } else {
    const uint32_t p = R.bitdepth >= 8 ? PngRgba8Wide(R, g, palette) : PngRgba8Narrow(R, static_cast<uint32_t>(g), palette);
    const uint32_t rep = outdepth == 16 ? 257u : 1u;
    r = (p & 255u) * rep;
    gr = ((p >> 8) & 255u) * rep;
    b = ((p >> 16) & 255u) * rep;
    a = (p >> 24) * rep;
  }
  v[0] = r;
  v[1] = channels == 2 ? a : gr;
  v[2] = b;
  v[3] = a;
}

ZMX_PD_HD inline uint32_t PngUnpackBitsOf(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// fl32(v) / maxv: one division, correctly rounded.
ZMX_PD_HD inline uint32_t PngUnpackQuotient(uint32_t v, float maxv) {
#if defined(__HIP_DEVICE_COMPILE__)
  return PngUnpackBitsOf(__fdiv_rn(static_cast<float>(v), maxv));
#else
  return PngUnpackBitsOf(static_cast<float>(v) / maxv);
#endif
}

// The fp32 `f` (bits; in [0, 1]) rounded to nearest-even into an fp16, subnormals included.
ZMX_PD_HD inline uint32_t PngUnpackToF16(uint32_t f) {
  const uint32_t e = f >> 23, m = f & 0x7fffffu;
  if (e == 0) return 0;
  if (e >= 113) {
    uint32_t h = ((e - 112u) << 10) | (m >> 13);
    const uint32_t rem = m & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;   // (a carry out of the mantissa is the next exponent)
    return h;
  }
  const uint32_t shift = 126u - e;   // (14 or more: the value in units of 2^-24)
  if (shift > 25) return 0;
  const uint32_t mant = m | 0x800000u;
  uint32_t h = mant >> shift;
  const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (h & 1u))) ++h;
  return h;
}
ZMX_PD_HD inline uint32_t PngUnpackToBF16(uint32_t f) {
  uint32_t h = f >> 16;
  const uint32_t rem = f & 0xffffu;
  if (rem > 0x8000u || (rem == 0x8000u && (h & 1u))) ++h;
  return h;
}

// The bits of the sample of type ST for the value v.
template <uint32_t ST>
ZMX_PD_HD inline uint32_t PngUnpackSample(uint32_t v, float maxv) {
  if (ST == kPngPackU8 || ST == kPngPackU16) return v;
  const uint32_t f = PngUnpackQuotient(v, maxv);
  return ST == kPngPackF32 ? f : ST == kPngPackF16 ? PngUnpackToF16(f) : PngUnpackToBF16(f);
}
ZMX_PD_HD inline uint32_t PngUnpackSampleOf(uint32_t sample, uint32_t v, float maxv) {
  switch (sample) {
    case kPngPackU8: case kPngPackU16: return v;
    case kPngPackF16: return PngUnpackSample<kPngPackF16>(v, maxv);
    case kPngPackBF16: return PngUnpackSample<kPngPackBF16>(v, maxv);
    default: return PngUnpackSample<kPngPackF32>(v, maxv);
  }
}

// ---- the input
// Pixel (y, x), by byte loads: its bytes, the first in the low byte; below 8 bits its value.
ZMX_PD_HD inline uint64_t PngUnpackGroupAt(const PngUnpackJob& J, uint64_t y, uint32_t x) {
  const unsigned char* const row = J.own + y * J.linebytes;
  if (J.bytewidth == 0) {
    const uint32_t per = 8 / J.depth;
    return (static_cast<uint32_t>(row[x / per]) >> (8 - J.depth * (x % per + 1))) & ((1u << J.depth) - 1u);
  }
  const unsigned char* const p = row + static_cast<uint64_t>(x) * J.bytewidth;
  uint64_t g = 0;
  for (uint32_t k = 0; k < J.bytewidth; ++k) g |= static_cast<uint64_t>(p[k]) << (8 * k);
  return g;
}

// kPngUnpackRun pixels of BW bytes at p, all of them the image's: 16-byte vectors where the run is a whole number of them
// and begins on one, words where it begins on one, else byte by byte.
template <uint32_t BW>
ZMX_PNGU_HD inline void PngUnpackLoadGroups(const unsigned char* p, uint64_t* g) {
  constexpr uint32_t bytes = kPngUnpackRun * BW, words = bytes / 4;
  uint32_t w[words];
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (bytes % 16 == 0 && (a & 15) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < bytes / 16; ++i) {
      PngColorVec x;
      __builtin_memcpy(&x, __builtin_assume_aligned(p + 16 * i, 16), 16);
      ZMX_PNGP_UNROLL
      for (uint32_t k = 0; k < 4; ++k) w[(4 * i + k) % words] = x.w[k];
    }
  } else if ((a & 3) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < words; ++i) w[i] = PngColorLoadWord(p + 4 * i);
  } else {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < words; ++i) {
      w[i] = static_cast<uint32_t>(p[4 * i]) | (static_cast<uint32_t>(p[4 * i + 1]) << 8) | (static_cast<uint32_t>(p[4 * i + 2]) << 16) |
             (static_cast<uint32_t>(p[4 * i + 3]) << 24);
    }
  }
  ZMX_PNGP_UNROLL
  for (uint32_t i = 0; i < kPngUnpackRun; ++i) {
    uint64_t v = 0;
    ZMX_PNGP_UNROLL
    for (uint32_t k = 0; k < BW; ++k) {
      const uint32_t j = i * BW + k;
      v |= static_cast<uint64_t>((w[j >> 2] >> (8 * (j & 3))) & 255u) << (8 * k);
    }
    g[i] = v;
  }
}

// ---- the stores
template <class Par>
ZMX_PNGU_HD inline void PngUnpackStoreSample(unsigned char* p, uint32_t ssz, uint32_t bits, const Par& par) {
  if (ssz == 1) {
    p[0] = static_cast<unsigned char>(bits);
  } else if (ssz == 2) {
    const uint16_t h = static_cast<uint16_t>(bits);
    __builtin_memcpy(__builtin_assume_aligned(p, 2), &h, 2);
  } else {
    __builtin_memcpy(__builtin_assume_aligned(p, 4), &bits, 4);
  }
  par.NoteWrite(p, ssz);
}

// sample i of a run, SSZ bytes, into the run's words
template <uint32_t SSZ>
ZMX_PNGU_HD inline void PngUnpackPut(uint32_t* w, uint32_t i, uint32_t bits) {
  if (SSZ == 4) w[i] = bits;
  else if (SSZ == 2) w[i >> 1] |= (bits & 65535u) << (16 * (i & 1));
  else w[i >> 2] |= (bits & 255u) << (8 * (i & 3));
}

// N samples of SSZ bytes (a multiple of 8 bytes in all), held in words, to p (a multiple of SSZ), all of them the sink's:
// 16-byte vectors and an 8-byte rest where p begins on a vector, 8-byte pairs, words, else sample by sample.
template <uint32_t SSZ, uint32_t N, class Par>
ZMX_PNGU_HD inline void PngUnpackStoreRun(unsigned char* p, const uint32_t* w, const Par& par) {
  constexpr uint32_t bytes = SSZ * N, words = bytes / 4;
  static_assert(bytes % 8 == 0, "a run is whole pairs of words");
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < bytes / 16; ++i) {
      const PngColorVec x = {{w[4 * i], w[(4 * i + 1) % words], w[(4 * i + 2) % words], w[(4 * i + 3) % words]}};
      __builtin_memcpy(__builtin_assume_aligned(p + 16 * i, 16), &x, 16);
      par.NoteWrite(p + 16 * i, 16);
    }
    if (bytes % 16 != 0) {
      const uint64_t x = w[words - 2] | (static_cast<uint64_t>(w[words - 1]) << 32);
      __builtin_memcpy(__builtin_assume_aligned(p + bytes - 8, 8), &x, 8);
      par.NoteWrite(p + bytes - 8, 8);
    }
  } else if ((a & 7) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < bytes / 8; ++i) {
      const uint64_t x = w[2 * i] | (static_cast<uint64_t>(w[2 * i + 1]) << 32);
      __builtin_memcpy(__builtin_assume_aligned(p + 8 * i, 8), &x, 8);
      par.NoteWrite(p + 8 * i, 8);
    }
  } else if ((a & 3) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < words; ++i) {
      __builtin_memcpy(__builtin_assume_aligned(p + 4 * i, 4), &w[i], 4);
      par.NoteWrite(p + 4 * i, 4);
    }
  } else {
    // (SSZ is 1 or 2 here: a multiple of 4 is a multiple of a word)
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < N; ++i) {
      const uint32_t bits = SSZ == 1 ? (w[(i >> 2) % words] >> (8 * (i & 3))) & 255u : (w[(i >> 1) % words] >> (16 * (i & 1))) & 65535u;
      PngUnpackStoreSample(p + SSZ * i, SSZ, bits, par);
    }
  }
}

// A whole run inside row y from column x0 of a sink on the interleaved or the planar path; v[4 * i + k]: pixel i's value
// of PNG channel k.
template <uint32_t ST, uint32_t C, class Par>
ZMX_PNGU_HD inline void PngUnpackFastAs(const PngUnpackJob& J, uint64_t y, uint32_t x0, const uint32_t* v, float maxv, const Par& par) {
  constexpr uint32_t ssz = PngPackSizeOf<ST>::value, R = kPngUnpackRun;
  unsigned char* const row = J.data + static_cast<int64_t>(y) * J.stride_y + static_cast<int64_t>(x0) * J.stride_x;
  if (J.path == kPngPackInterleaved) {
    uint32_t w[R * C * ssz / 4];
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < R * C * ssz / 4; ++i) w[i] = 0;
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < R; ++i) {
      ZMX_PNGP_UNROLL
      for (uint32_t k = 0; k < C; ++k) PngUnpackPut<ssz>(w, i * C + k, PngUnpackSample<ST>(v[4 * i + k], maxv));
    }
    PngUnpackStoreRun<ssz, R * C>(row, w, par);
    return;
  }
  ZMX_PNGP_UNROLL
  for (uint32_t k = 0; k < C; ++k) {
    uint32_t w[R * ssz / 4];
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < R * ssz / 4; ++i) w[i] = 0;
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < R; ++i) PngUnpackPut<ssz>(w, i, PngUnpackSample<ST>(v[4 * i + k], maxv));
    PngUnpackStoreRun<ssz, R>(row + static_cast<int64_t>(J.order[k]) * J.stride_c, w, par);
  }
}

template <uint32_t ST, class Par>
ZMX_PNGU_HD inline void PngUnpackFastOf(const PngUnpackJob& J, uint64_t y, uint32_t x0, const uint32_t* v, float maxv, const Par& par) {
  switch (J.channels) {
    case 1: PngUnpackFastAs<ST, 1>(J, y, x0, v, maxv, par); break;
    case 2: PngUnpackFastAs<ST, 2>(J, y, x0, v, maxv, par); break;
    case 3: PngUnpackFastAs<ST, 3>(J, y, x0, v, maxv, par); break;
    default: PngUnpackFastAs<ST, 4>(J, y, x0, v, maxv, par); break;
  }
}

template <class Par>
ZMX_PNGU_HD inline void PngUnpackFast(const PngUnpackJob& J, uint64_t y, uint32_t x0, const uint32_t* v, float maxv, const Par& par) {
  switch (J.sample) {
    case kPngPackU8: PngUnpackFastOf<kPngPackU8>(J, y, x0, v, maxv, par); break;
    case kPngPackU16: PngUnpackFastOf<kPngPackU16>(J, y, x0, v, maxv, par); break;
    case kPngPackF16: PngUnpackFastOf<kPngPackF16>(J, y, x0, v, maxv, par); break;
    case kPngPackBF16: PngUnpackFastOf<kPngPackBF16>(J, y, x0, v, maxv, par); break;
    default: PngUnpackFastOf<kPngPackF32>(J, y, x0, v, maxv, par); break;
  }
}

// Thread `thread` of a workgroup of `threads` stores its share of tile `tile` of J's image; `palette`: the image's 256
// words where its colour type is 3 (the workgroup's LDS on the device).
template <class Par>
ZMX_PD_HD inline void PngUnpackTile(const PngUnpackJob& J, const uint32_t* palette, uint64_t tile, uint32_t thread, uint32_t threads, const Par& par) {
  PngWalkRecord R = PngWalkRecord{};
  R.colortype = J.colortype;
  R.bitdepth = J.depth;
  R.has_key = J.has_key;
  R.key_r = J.key_r;
  R.key_g = J.key_g;
  R.key_b = J.key_b;
  const float maxv = J.bitdepth == 16 ? 65535.0f : 255.0f;
  const uint32_t ssz = PngPackSampleBytes(J.sample);
  uint32_t order = 0;   // (the four bytes as a word: an index that is no constant would put the whole job into scratch memory)
  __builtin_memcpy(&order, J.order, 4);
  const uint64_t begin = tile * kPngUnpackTilePixels;
  const uint64_t end = J.npixels - begin < kPngUnpackTilePixels ? J.npixels : begin + kPngUnpackTilePixels;
  for (uint64_t p0 = begin + static_cast<uint64_t>(kPngUnpackRun) * thread; p0 < end; p0 += static_cast<uint64_t>(kPngUnpackRun) * threads) {
    uint64_t y = (p0 >> 32) == 0 ? static_cast<uint32_t>(p0) / J.width : p0 / J.width;
    uint32_t x = static_cast<uint32_t>(p0 - y * J.width);
    if (J.path != kPngPackScalar && end - p0 >= kPngUnpackRun && J.width - x >= kPngUnpackRun) {
      uint64_t g[kPngUnpackRun];
      const unsigned char* const in = J.own + y * J.linebytes + static_cast<uint64_t>(x) * J.bytewidth;
      switch (J.bytewidth) {
        case 1: PngUnpackLoadGroups<1>(in, g); break;
        case 2: PngUnpackLoadGroups<2>(in, g); break;
        case 3: PngUnpackLoadGroups<3>(in, g); break;
        case 4: PngUnpackLoadGroups<4>(in, g); break;
        case 6: PngUnpackLoadGroups<6>(in, g); break;
        case 8: PngUnpackLoadGroups<8>(in, g); break;
        default:
          ZMX_PNGP_UNROLL
          for (uint32_t i = 0; i < kPngUnpackRun; ++i) g[i] = PngUnpackGroupAt(J, y, x + i);
          break;
      }
      uint32_t v[4 * kPngUnpackRun];
      ZMX_PNGP_UNROLL
      for (uint32_t i = 0; i < kPngUnpackRun; ++i) PngUnpackValues(R, J.channels, J.bitdepth, g[i], palette, v + 4 * i);
      PngUnpackFast(J, y, x, v, maxv, par);
      continue;
    }
    const uint32_t n = end - p0 < kPngUnpackRun ? static_cast<uint32_t>(end - p0) : kPngUnpackRun;
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t v[4];
      PngUnpackValues(R, J.channels, J.bitdepth, PngUnpackGroupAt(J, y, x), palette, v);
      unsigned char* const px = J.data + static_cast<int64_t>(y) * J.stride_y + static_cast<int64_t>(x) * J.stride_x;
      for (uint32_t k = 0; k < J.channels; ++k) {
        // (v[k] by selects, for the same reason)
        const uint32_t vk = k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
        PngUnpackStoreSample(px + static_cast<int64_t>((order >> (8 * k)) & 255u) * J.stride_c, ssz, PngUnpackSampleOf(J.sample, vk, maxv), par);
      }
      if (++x == J.width) { x = 0; ++y; }
    }
  }
}

// The workgroup's copy of J's palette (colour type 3), each thread its share; a barrier on both sides on the device.
ZMX_PD_HD inline void PngUnpackStage(const PngUnpackTable& T, const PngUnpackJob& J, uint32_t* staged, uint32_t thread, uint32_t threads) {
  for (uint32_t i = thread; i < 256; i += threads) staged[i] = T.palettes[256 * static_cast<uint64_t>(J.palette) + i];
}

// The image that global tile `tile` (< tile_start[n]) belongs to, and the tile's number within it.
ZMX_PD_HD inline uint64_t PngUnpackJobOfTile(const PngUnpackTable& T, uint64_t tile, uint64_t* local) {
  return PngPackSourceOfTile(T.tile_start, T.n, tile, local);
}

}  // namespace zamd

#if defined(ZMX_PNG_UNPACK_KERNELS)

struct PngUnpackDevicePar {
  __device__ void NoteWrite(const void*, uint64_t) const {}
};

__global__ __launch_bounds__(256) void k_png_unpack(zamd::PngUnpackTable T, uint64_t ntiles) {
  __shared__ uint32_t palette[256];
  const PngUnpackDevicePar par;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint64_t local = 0;
    const uint64_t i = zamd::PngUnpackJobOfTile(T, tile, &local);
    const zamd::PngUnpackJob J = T.jobs[i];
    if (J.colortype == 3) {   // (the same for every thread of the workgroup)
      __syncthreads();        // (the tile before this one has read its palette)
      zamd::PngUnpackStage(T, J, palette, threadIdx.x, blockDim.x);
      __syncthreads();
    }
    zamd::PngUnpackTile(J, palette, local, threadIdx.x, blockDim.x, par);
  }
}

#endif  // ZMX_PNG_UNPACK_KERNELS

#endif  // ZMX_PNG_UNPACK_H_
