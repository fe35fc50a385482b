// zmx_png_pack_device: what a GPU program holds — a strided, planar, swizzled, typed image — into PNG byte order: rows back
// to back, channels interleaved, 8-bit samples or 16-bit ones high byte first, as zmx_png_image wants them.  A sample
// (y, x, c) of a source lies at data + y * stride_y + x * stride_x + c * stride_c (bytes, any sign, 0 a broadcast); PNG
// channel k of a pixel is source channel order[k].
//   k_png_pack  ONE launch for n sources, at most kPngPackMaxBlocks workgroups.  A destination is cut into tiles of
//               kPngPackTileVecs aligned 16-byte vectors, counted from the 16-byte boundary at or below its first byte;
//               the tiles of all destinations are numbered one after the other, a workgroup strides over that number and
//               finds its tile's image by binary search over the prefix of tile counts, as k_bitjoin_many does.  No
//               workgroup waits for another.  Threads own the vectors: a vector that lies inside its destination is
//               stored whole, the bytes of one that does not (the head, the tail, a neighbour's bytes) singly — every
//               byte of every destination exactly once, none outside.  Three paths, chosen per source on the host
//               (PngPackPathOf):
//                 interleaved  stride_c = the sample's size, stride_x = channels * that, order the identity (or one
//                              channel with stride_x = the sample's size): a vector's 16 or 8 samples are one run of the
//                              source's row, loaded as 16-byte vectors where the run's address allows, words or samples
//                              where not.
//                 planar       stride_x = the sample's size, any stride_c, any order: a thread takes whole pixels — one
//                              vector, three for three channels, so 48 bytes —, the consecutive samples of each plane
//                              as one run, loaded as wide as its address allows; neighbouring lanes read neighbouring
//                              addresses of one plane.
//                 scalar       everything else, and in the other two every vector that crosses a row's end, does not
//                              begin on a sample's (a pixel's) first byte or is not whole: a load per sample, merely
//                              correct.
//               The value rule (include/zopfli_amd.h has its text): U8 -> 8 the byte, U16 -> 16 the value; F16 and BF16
//               widened to fp32 exactly; F32: q = (uint32) clamp(fl32(fl32(x * maxv) + 0.5f), 0, maxv), the multiply and
//               the add each rounded to fp32 and never contracted, the conversion truncating, a NaN 0.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/png_source_print.cc) runs the very code of
// the kernel, the threads one after the other.  This header compiles without HIP; the kernel is there for the device layer
// only (ZMX_PNG_PACK_KERNELS).  Plain loads and stores, nothing else; the source is never written.
#ifndef ZMX_PNG_PACK_H_
#define ZMX_PNG_PACK_H_

#include <stddef.h>
#include <stdint.h>

#include "zmx_png_color.h"   // ZMX_PNGC_HD, PngColorVec, PngConvAt, the workgroup's size and the grid's cap

#if defined(__HIP_DEVICE_COMPILE__)
#define ZMX_PNGP_UNROLL _Pragma("unroll")
#else
#define ZMX_PNGP_UNROLL
#endif

namespace zamd {

constexpr uint32_t kPngPackThreads = kPngColorThreads;      // a workgroup: four waves
constexpr uint32_t kPngPackMaxBlocks = kPngColorMaxBlocks;
constexpr uint32_t kPngPackTileVecs = 768;                  // 12 KiB of a destination: three vectors a thread, a multiple of 3
// ZMX_PNG_SAMPLE_* (include/zopfli_amd.h)
constexpr uint32_t kPngPackU8 = 0, kPngPackU16 = 1, kPngPackF16 = 2, kPngPackBF16 = 3, kPngPackF32 = 4;
constexpr uint32_t kPngPackScalar = 0, kPngPackInterleaved = 1, kPngPackPlanar = 2;

// One source and its destination, as the kernel reads them (made on the host: PngPackSourceOf).
struct PngPackSource {
  const unsigned char* data;             // sample (0, 0, 0)
  int64_t stride_y, stride_x, stride_c;  // bytes
  unsigned char* out;                    // height * rowbytes bytes, any alignment
  uint64_t rowbytes;                     // width * channels * bitdepth / 8, below 2^31
  uint64_t total;                        // height * rowbytes
  uint32_t width, height, channels, sample, bitdepth, path;
  uint8_t order[4];
  uint32_t reserved;
};

struct PngPackTable {
  const PngPackSource* src;     // [n]
  const uint64_t* tile_start;   // [n + 1], ascending: the number of source i's first tile
  uint64_t n;
};

ZMX_PNGC_HD inline uint32_t PngPackSampleBytes(uint32_t sample) { return sample == kPngPackU8 ? 1u : sample == kPngPackF32 ? 4u : 2u; }

ZMX_PNGC_HD inline uint32_t PngPackPathOf(int64_t stride_x, int64_t stride_c, uint32_t channels, uint32_t sample, const uint8_t* order) {
  const int64_t ssz = PngPackSampleBytes(sample);
  if (channels == 1) return stride_x == ssz ? kPngPackInterleaved : kPngPackScalar;
  bool identity = true;
  for (uint32_t k = 0; k < channels; ++k) identity = identity && order[k] == k;
  if (identity && stride_c == ssz && stride_x == ssz * channels) return kPngPackInterleaved;
  return stride_x == ssz ? kPngPackPlanar : kPngPackScalar;
}

// The record of a source the host has checked (host/png_source.h) whose packed image goes to `out`.  Source: zmx_png_source.
template <class Source>
inline PngPackSource PngPackSourceOf(const Source& s, void* out) {
  PngPackSource r;
  r.data = static_cast<const unsigned char*>(s.d_data);
  r.stride_y = s.stride_y;
  r.stride_x = s.stride_x;
  r.stride_c = s.stride_c;
  r.out = static_cast<unsigned char*>(out);
  r.rowbytes = static_cast<uint64_t>(s.width) * s.channels * (s.bitdepth / 8);
  r.total = r.rowbytes * s.height;
  r.width = s.width;
  r.height = s.height;
  r.channels = s.channels;
  r.sample = s.sample;
  r.bitdepth = s.bitdepth;
  for (int k = 0; k < 4; ++k) r.order[k] = static_cast<uint32_t>(k) < s.channels ? s.order[k] : 0;
  r.path = PngPackPathOf(s.stride_x, s.stride_c, s.channels, s.sample, r.order);
  r.reserved = 0;
  return r;
}

// The vectors and the tiles of a destination.
ZMX_PNGC_HD inline uint64_t PngPackVectors(const unsigned char* out, uint64_t total) {
  return total == 0 ? 0 : ((reinterpret_cast<uintptr_t>(out) & 15) + total + 15) / 16;
}
ZMX_PNGC_HD inline uint64_t PngPackTiles(const unsigned char* out, uint64_t total) {
  return (PngPackVectors(out, total) + kPngPackTileVecs - 1) / kPngPackTileVecs;
}
ZMX_PNGC_HD inline uint32_t PngPackGrid(uint64_t ntiles) {
  return static_cast<uint32_t>(ntiles == 0 ? 1 : ntiles < kPngPackMaxBlocks ? ntiles : kPngPackMaxBlocks);
}

// ---- values
// An fp16 as the fp32 of the same value (denormals, infinities and NaNs included): the bits.
ZMX_PNGC_HD inline uint32_t PngPackWidenF16(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u;
  uint32_t m = h & 0x3ffu;
  if (e == 31) return sign | 0x7f800000u | (m << 13);
  if (e != 0) return sign | ((e + 112u) << 23) | (m << 13);
  if (m == 0) return sign;
  const uint32_t s = static_cast<uint32_t>(__builtin_clz(m)) - 21u;   // the shifts that bring its top bit to bit 10
  m = (m << s) & 0x3ffu;
  return sign | ((113u - s) << 23) | (m << 13);
}

ZMX_PNGC_HD inline float PngPackFloatOf(uint32_t bits) {
  float f;
  __builtin_memcpy(&f, &bits, 4);
  return f;
}

// fl32(fl32(x * maxv) + 0.5f), clamped, truncated; a NaN gives 0.  Two roundings: nothing here may become one fma.
ZMX_PNGC_HD inline uint32_t PngPackQuantF32(float x, float maxv) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float a = __fadd_rn(__fmul_rn(x, maxv), 0.5f);
#else
  volatile float m = x * maxv;
  const float a = m + 0.5f;
#endif
  if (!(a > 0.0f)) return 0u;   // (a NaN, a negative, either zero)
  if (a >= maxv) return static_cast<uint32_t>(maxv);
  return static_cast<uint32_t>(a);
}

// The sample whose bits are `raw` as the PNG's value at 8 or 16 bits (the host has refused U8 -> 16 and U16 -> 8).
ZMX_PNGC_HD inline uint32_t PngPackQuant(uint32_t sample, uint32_t raw, uint32_t bitdepth) {
  if (sample == kPngPackU8 || sample == kPngPackU16) return raw;
  const uint32_t bits = sample == kPngPackF16 ? PngPackWidenF16(raw) : sample == kPngPackBF16 ? raw << 16 : raw;
  return PngPackQuantF32(PngPackFloatOf(bits), bitdepth == 16 ? 65535.0f : 255.0f);
}

// the sample of `ssz` bytes at p, a multiple of its size
ZMX_PNGC_HD inline uint32_t PngPackLoadSample(const unsigned char* p, uint32_t ssz) {
  if (ssz == 1) return p[0];
  if (ssz == 2) {
    uint16_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 2), 2);
    return v;
  }
  return PngColorLoadWord(p);
}

// ---- the scalar path
// the sample a thread quantised last
struct PngPackCache {
  uint64_t row;
  uint32_t index;   // of the sample in its row of the output
  uint32_t q;
  bool have;
};

// byte x of row `row` of the output
ZMX_PNGC_HD inline uint32_t PngPackByte(const PngPackSource& S, uint64_t row, uint64_t x, PngPackCache* c) {
  const uint32_t sb = S.bitdepth / 8;
  const uint32_t xx = static_cast<uint32_t>(x);   // (a row has at most 2^31 - 1 bytes)
  const uint32_t index = xx / sb;
  if (!(c->have && c->row == row && c->index == index)) {
    const uint32_t col = index / S.channels, k = index - col * S.channels;
    const int64_t at = static_cast<int64_t>(row) * S.stride_y + static_cast<int64_t>(col) * S.stride_x + static_cast<int64_t>(S.order[k]) * S.stride_c;
    c->q = PngPackQuant(S.sample, PngPackLoadSample(S.data + at, PngPackSampleBytes(S.sample)), S.bitdepth);
    c->row = row;
    c->index = index;
    c->have = true;
  }
  if (sb == 2) return (xx & 1u) ? c->q & 255u : (c->q >> 8) & 255u;
  return c->q & 255u;
}

// Vector g of the destination, by the scalar rule: whole where all its bytes are the destination's, else its bytes singly.
ZMX_PNGC_HD inline void PngPackEdgeVec(const PngPackSource& S, uint64_t g) {
  const uint64_t lead = reinterpret_cast<uintptr_t>(S.out) & 15;
  const uint64_t b0 = 16 * g > lead ? 16 * g - lead : 0;
  const uint64_t b1 = 16 * g + 16 - lead < S.total ? 16 * g + 16 - lead : S.total;
  if (b0 >= b1) return;
  PngPackCache cache = {0, 0, 0, false};
  uint64_t row, x;
  PngConvAt(b0, S.rowbytes, &row, &x);
  if (b1 - b0 == 16) {
    PngColorVec vec = {{0, 0, 0, 0}};
    for (int j = 0; j < 16; ++j) {
      vec.w[j >> 2] |= PngPackByte(S, row, x, &cache) << (8 * (j & 3));
      if (++x == S.rowbytes) { x = 0; ++row; }
    }
    __builtin_memcpy(__builtin_assume_aligned(S.out + b0, 16), &vec, 16);
    return;
  }
  for (uint64_t b = b0; b < b1; ++b) {
    S.out[b] = static_cast<unsigned char>(PngPackByte(S, row, x, &cache));
    if (++x == S.rowbytes) { x = 0; ++row; }
  }
}

// ---- runs of samples
// N consecutive samples of SSZ bytes at p (a multiple of SSZ), all of them the source's, as their bits: 16-byte vectors
// where the run is a whole number of them and begins on one, words likewise, else sample by sample.  (An index `% N`
// changes nothing where its branch can run — it is below N there —; it keeps the branches that cannot, for this SSZ and N,
// inside the array for the compiler.)
template <uint32_t SSZ, uint32_t N>
ZMX_PNGC_HD inline void PngPackLoadRun(const unsigned char* p, uint32_t* v) {
  constexpr uint32_t bytes = SSZ * N;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (SSZ == 4) {
    if (bytes % 16 == 0 && (a & 15) == 0) {
      ZMX_PNGP_UNROLL
      for (uint32_t i = 0; i < bytes / 16; ++i) {
        PngColorVec x;
        __builtin_memcpy(&x, __builtin_assume_aligned(p + 16 * i, 16), 16);
        ZMX_PNGP_UNROLL
        for (uint32_t k = 0; k < 4; ++k) v[(4 * i + k) % N] = x.w[k];
      }
    } else {
      ZMX_PNGP_UNROLL
      for (uint32_t i = 0; i < N; ++i) v[i] = PngColorLoadWord(p + 4 * i);
    }
    return;
  }
  constexpr uint32_t per_word = 4 / SSZ, mask = SSZ == 1 ? 255u : 65535u;
  if (bytes % 16 == 0 && (a & 15) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < bytes / 16; ++i) {
      PngColorVec x;
      __builtin_memcpy(&x, __builtin_assume_aligned(p + 16 * i, 16), 16);
      ZMX_PNGP_UNROLL
      for (uint32_t k = 0; k < 4 * per_word; ++k) v[(4 * per_word * i + k) % N] = (x.w[k / per_word] >> (8 * SSZ * (k % per_word))) & mask;
    }
  } else if (bytes % 4 == 0 && (a & 3) == 0) {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < bytes / 4; ++i) {
      const uint32_t w = PngColorLoadWord(p + 4 * i);
      ZMX_PNGP_UNROLL
      for (uint32_t k = 0; k < per_word; ++k) v[(per_word * i + k) % N] = (w >> (8 * SSZ * k)) & mask;
    }
  } else {
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < N; ++i) v[i] = PngPackLoadSample(p + SSZ * i, SSZ);
  }
}

// value q as byte `at` of NW words, a sample of SB bytes
template <uint32_t SB, uint32_t NW>
ZMX_PNGC_HD inline void PngPackPut(uint32_t* w, uint32_t at, uint32_t q) {
  if (SB == 1) {
    w[(at >> 2) % NW] |= q << (8 * (at & 3));
  } else {
    // (high byte first; `at` is even)
    w[(at >> 2) % NW] |= (((q >> 8) & 255u) | ((q & 255u) << 8)) << (8 * (at & 3));
  }
}

template <uint32_t ST>
struct PngPackSizeOf { static constexpr uint32_t value = ST == kPngPackU8 ? 1 : ST == kPngPackF32 ? 4 : 2; };

// ---- the interleaved path: the vector at dst is bytes [x, x + 16) of row `row`, x on a sample's first byte
template <uint32_t ST, uint32_t SB>
ZMX_PNGC_HD inline void PngPackInterleavedVec(const PngPackSource& S, uint64_t row, uint64_t x, unsigned char* dst) {
  constexpr uint32_t ssz = PngPackSizeOf<ST>::value, n = 16 / SB;
  const unsigned char* p = S.data + static_cast<int64_t>(row) * S.stride_y + static_cast<int64_t>(x / SB) * ssz;
  uint32_t v[n];
  PngPackLoadRun<ssz, n>(p, v);
  PngColorVec vec = {{0, 0, 0, 0}};
  ZMX_PNGP_UNROLL
  for (uint32_t i = 0; i < n; ++i) PngPackPut<SB, 4>(vec.w, i * SB, PngPackQuant(ST, v[i], 8 * SB));
  __builtin_memcpy(__builtin_assume_aligned(dst, 16), &vec, 16);
}

// ---- the planar path: the G vectors at dst are bytes [x, x + 16 G) of row `row`, x on a pixel's first byte
template <uint32_t ST, uint32_t SB, uint32_t C>
ZMX_PNGC_HD inline void PngPackPlanarUnit(const PngPackSource& S, uint64_t row, uint64_t x, unsigned char* dst) {
  constexpr uint32_t ssz = PngPackSizeOf<ST>::value, G = C == 3 ? 3 : 1, np = 16 * G / (C * SB);
  const unsigned char* p = S.data + static_cast<int64_t>(row) * S.stride_y + static_cast<int64_t>(x / (C * SB)) * ssz;
  uint32_t w[4 * G];
  ZMX_PNGP_UNROLL
  for (uint32_t i = 0; i < 4 * G; ++i) w[i] = 0;
  ZMX_PNGP_UNROLL
  for (uint32_t k = 0; k < C; ++k) {
    uint32_t v[np];
    PngPackLoadRun<ssz, np>(p + static_cast<int64_t>(S.order[k]) * S.stride_c, v);
    ZMX_PNGP_UNROLL
    for (uint32_t i = 0; i < np; ++i) PngPackPut<SB, 4 * G>(w, (i * C + k) * SB, PngPackQuant(ST, v[i], 8 * SB));
  }
  ZMX_PNGP_UNROLL
  for (uint32_t i = 0; i < G; ++i) {
    PngColorVec vec = {{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]}};
    __builtin_memcpy(__builtin_assume_aligned(dst + 16 * i, 16), &vec, 16);
  }
}

template <uint32_t ST, uint32_t SB>
ZMX_PNGC_HD inline void PngPackFastAs(const PngPackSource& S, uint64_t row, uint64_t x, unsigned char* dst) {
  if (S.path == kPngPackInterleaved) PngPackInterleavedVec<ST, SB>(S, row, x, dst);
  else if (S.channels == 2) PngPackPlanarUnit<ST, SB, 2>(S, row, x, dst);
  else if (S.channels == 3) PngPackPlanarUnit<ST, SB, 3>(S, row, x, dst);
  else PngPackPlanarUnit<ST, SB, 4>(S, row, x, dst);
}

ZMX_PNGC_HD inline void PngPackFast(const PngPackSource& S, uint64_t row, uint64_t x, unsigned char* dst) {
  switch (S.sample * 2 + (S.bitdepth == 16 ? 1u : 0u)) {
    case 0: PngPackFastAs<kPngPackU8, 1>(S, row, x, dst); break;
    case 3: PngPackFastAs<kPngPackU16, 2>(S, row, x, dst); break;
    case 4: PngPackFastAs<kPngPackF16, 1>(S, row, x, dst); break;
    case 5: PngPackFastAs<kPngPackF16, 2>(S, row, x, dst); break;
    case 6: PngPackFastAs<kPngPackBF16, 1>(S, row, x, dst); break;
    case 7: PngPackFastAs<kPngPackBF16, 2>(S, row, x, dst); break;
    case 8: PngPackFastAs<kPngPackF32, 1>(S, row, x, dst); break;
    case 9: PngPackFastAs<kPngPackF32, 2>(S, row, x, dst); break;
    default: break;
  }
}

// the vectors a thread takes at a time, and the bytes their first must begin on a multiple of within its row
ZMX_PNGC_HD inline uint32_t PngPackUnitVecs(const PngPackSource& S) { return S.path == kPngPackPlanar && S.channels == 3 ? 3u : 1u; }
ZMX_PNGC_HD inline uint32_t PngPackUnitAlign(const PngPackSource& S) { return (S.path == kPngPackPlanar ? S.channels : 1u) * (S.bitdepth / 8); }

// Thread `thread` of a workgroup of `threads` makes its share of tile `tile` of S's destination.
ZMX_PNGC_HD inline void PngPackTile(const PngPackSource& S, uint64_t tile, uint32_t thread, uint32_t threads) {
  const uint64_t lead = reinterpret_cast<uintptr_t>(S.out) & 15;
  const uint64_t nvec = PngPackVectors(S.out, S.total);
  const uint64_t g0 = tile * kPngPackTileVecs;
  const uint64_t g1 = nvec - g0 < kPngPackTileVecs ? nvec : g0 + kPngPackTileVecs;
  const uint64_t G = PngPackUnitVecs(S), bytes = 16 * G;
  const uint32_t align = PngPackUnitAlign(S);
  for (uint64_t u = g0 + G * thread; u < g1; u += G * threads) {
    // the unit: vectors [u, u + G), those of them below g1
    if (S.path != kPngPackScalar && u + G <= g1 && 16 * u >= lead && 16 * u - lead + bytes <= S.total) {
      uint64_t row, x;
      PngConvAt(16 * u - lead, S.rowbytes, &row, &x);
      if (x + bytes <= S.rowbytes && static_cast<uint32_t>(x) % align == 0) {
        PngPackFast(S, row, x, S.out + (16 * u - lead));
        continue;
      }
    }
    for (uint64_t g = u; g < u + G && g < g1; ++g) PngPackEdgeVec(S, g);
  }
}

// The source that global tile `tile` (< tile_start[n]) belongs to — the last i with tile_start[i] <= tile, which has at
// least one tile — and the tile's number within it.
ZMX_PNGC_HD inline uint64_t PngPackSourceOfTile(const uint64_t* tile_start, uint64_t n, uint64_t tile, uint64_t* local) {
  uint64_t lo = 0, hi = n;   // tile_start[lo] <= tile < tile_start[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (tile_start[mid] <= tile) lo = mid; else hi = mid;
  }
  *local = tile - tile_start[lo];
  return lo;
}

ZMX_PNGC_HD inline void PngPackManyTile(const PngPackTable& T, uint64_t tile, uint32_t thread, uint32_t threads) {
  uint64_t local = 0;
  const uint64_t i = PngPackSourceOfTile(T.tile_start, T.n, tile, &local);
  const PngPackSource S = T.src[i];
  PngPackTile(S, local, thread, threads);
}

}  // namespace zamd

#if defined(ZMX_PNG_PACK_KERNELS)

__global__ __launch_bounds__(256) void k_png_pack(zamd::PngPackTable T, uint64_t ntiles) {
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) zamd::PngPackManyTile(T, tile, threadIdx.x, blockDim.x);
}

#endif  // ZMX_PNG_PACK_KERNELS

#endif  // ZMX_PNG_PACK_H_
