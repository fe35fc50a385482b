// zmx_png_lossy_transparent_device: zopflipng's --lossy_transparent (zopflipng_lib.cc LossyOptimizeTransparent) on an image
// in device memory — grey + alpha or RGBA at 8 bits, or at 16 bits seen through its high bytes.  Every rule is stated on
// the pixel's 8-bit view r, g, b, a (grey gives r = g = b) and on the pixels in raster order, rows back to back.
//   geometry           A thread takes kPngColorChunk (48) bytes a step — 12 RGBA8, 24 GA8, 6 RGBA16, 12 GA16 pixels — a
//                      workgroup of 256 threads the 256 chunks that follow each other: a TILE.  Workgroup g of G (at most
//                      kPngColorMaxBlocks) takes the tiles g, g + G, ...; G tiles are the SWEEP of a full launch.  The
//                      last tile may end inside a chunk; what is left of that chunk is read and written byte by byte.
//   k_png_lossy_stats  one pass.  The flag "some 0 < a < 255" and the smallest index of a pixel with a = 0 stay in
//                      registers, are joined over the wave by shuffles, over the workgroup in LDS, and reach global memory
//                      once a workgroup and only where they say something.  Colours are counted in zmx_png_color.h's
//                      512-slot table, in LDS first, every pixel with a = 0 as the colour 0; a workgroup past 256 colours
//                      stops COUNTING and says so (the others look at every tile's start), never the rest of the pass.
//                      Per tile it leaves the tile's SUMMARY: the RGB of its last pixel with a > 0, or "none".
//   k_png_lossy_carry  one workgroup, carry mode only: summaries -> every tile's CARRY-IN, the summary of the nearest
//                      earlier tile that has one (an exclusive scan under PngLossyPick), 256 tiles a step.
//   k_png_lossy_fill   writes the rewritten image, tile by tile as the statistics read it.  Fixed mode: every a = 0 pixel
//                      gets the 8-bit view of the first transparent pixel, which every thread reads itself.  Carry mode:
//                      a thread's chunk starts from the exclusive scan, over its workgroup, of the chunks' last opaque
//                      RGBs, seeded with the tile's carry-in, and walks its pixels in rising order.  A thread stores the
//                      48 bytes it loaded — 16-byte vectors where the output is aligned, words, else bytes — so every byte
//                      is written exactly once.  At 16 bits only the high bytes of r, g, b change.
// No workgroup waits for another: what a phase needs of the one before passes between launches of one stream.  A tile's
// summary is read by k_png_lossy_carry alone and its carry-in by the one workgroup that fills it, so the work is linear
// in the pixels whatever the image.  In place (the output IS the image) is safe: the bytes read as a source are alphas
// and the RGB of pixels with a > 0, which no thread changes, and the first transparent pixel, rewritten to itself.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/png_lossy_print.cc) runs the very code of
// the kernels, the threads one after the other.  This header compiles without HIP; the kernels are there for the device
// layer only (ZMX_PNG_LOSSY_KERNELS).  Plain loads and stores and the HIP atomics, nothing else.
#ifndef ZMX_PNG_LOSSY_H_
#define ZMX_PNG_LOSSY_H_

#include "zmx_png_color.h"

namespace zamd {

constexpr uint32_t kPngLossyThreads = kPngColorThreads;                 // a workgroup: a tile's chunks
constexpr uint32_t kPngLossyTileBytes = kPngLossyThreads * kPngColorChunk;
constexpr uint32_t kPngLossyScanStep = kPngLossyThreads;                // tiles k_png_lossy_carry takes a step
constexpr uint32_t kPngLossyNone = 0;                                   // a summary, a carry-in: no pixel with a > 0
constexpr uint32_t kPngLossyHas = 0x01000000u;                          // else kPngLossyHas | r | g << 8 | b << 16
constexpr uint32_t kPngLossyNoIndex = 0xffffffffu;                      // no pixel with a = 0
constexpr uint32_t kPngLossyModeNone = 0, kPngLossyModeFixed = 1, kPngLossyModeCarry = 2;

// What k_png_lossy_stats leaves in device memory.  Before the launch: all ones, then zeros from `color` up to its key_min.
// Of `color` the flags (kPngColorPartial alone), overflow, count and table are used.
struct PngLossyState {
  uint32_t first_transparent;   // the smallest index of a pixel with a = 0; kPngLossyNoIndex: none
  uint32_t fill;                // k_png_lossy_fill, fixed mode: kPngLossyHas | the colour it took
  PngColorState color;
};

struct PngLossyParams {
  PngColorImage in;             // colour type 4 or 6
  unsigned char* out;           // the image's size, any alignment; may be in.pixels
  uint32_t mode;                // kPngLossyModeFixed, kPngLossyModeCarry
  uint32_t first_transparent;   // fixed mode
  const uint32_t* carry_in;     // carry mode: [tiles]
  PngLossyState* state;
};

ZMX_PNGC_HD inline uint32_t PngLossyTilePixels(uint32_t colortype, uint32_t bitdepth) {
  return kPngLossyTileBytes / PngColorPixelBytes(colortype, bitdepth);
}
ZMX_PNGC_HD inline uint64_t PngLossyTiles(const PngColorImage& I) {
  const uint64_t per = PngLossyTilePixels(I.colortype, I.bitdepth);
  return (I.numpixels + per - 1) / per;
}
ZMX_PNGC_HD inline uint32_t PngLossyGrid(const PngColorImage& I) {
  const uint64_t tiles = PngLossyTiles(I);
  return static_cast<uint32_t>(tiles == 0 ? 1 : tiles < kPngColorMaxBlocks ? tiles : kPngColorMaxBlocks);
}

// the scan's operator: the right operand if it has a colour, else the left
ZMX_PNGC_HD inline uint32_t PngLossyPick(uint32_t left, uint32_t right) { return right != kPngLossyNone ? right : left; }

// ---- a thread's chunk
// The pixels of thread `local`'s chunk of `tile` that lie in the image: 0 .. 48 / BYTES, and the index of the first.
template <uint32_t BYTES>
ZMX_PNGC_HD inline uint32_t PngLossyChunkPixels(const PngColorImage& I, uint64_t tile, uint32_t local, uint64_t* first) {
  constexpr uint32_t per_chunk = kPngColorChunk / BYTES;
  *first = (tile * kPngLossyThreads + local) * per_chunk;
  if (*first >= I.numpixels) return 0;
  const uint64_t left = I.numpixels - *first;
  return left < per_chunk ? static_cast<uint32_t>(left) : per_chunk;
}

// `npix` pixels at p as little-endian words: a whole chunk by PngColorLoadChunk, less byte by byte (zeros behind them)
template <uint32_t BYTES>
ZMX_PNGC_HD inline void PngLossyLoad(const unsigned char* p, uint32_t npix, uint32_t* w) {
  if (npix == kPngColorChunk / BYTES) {
    PngColorLoadChunk(p, w);
    return;
  }
  for (int k = 0; k < 12; ++k) w[k] = 0;
  for (uint32_t j = 0; j < npix * BYTES; ++j) w[j >> 2] |= static_cast<uint32_t>(p[j]) << (8 * (j & 3));
}

template <uint32_t BYTES>
ZMX_PNGC_HD inline void PngLossyStore(unsigned char* p, uint32_t npix, const uint32_t* w) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (npix != kPngColorChunk / BYTES) {
    for (uint32_t j = 0; j < npix * BYTES; ++j) p[j] = static_cast<unsigned char>(PngColorChunkByte(w, j));
  } else if ((a & 15) == 0) {
    for (int v = 0; v < 3; ++v) {
      PngColorVec x;
      for (int k = 0; k < 4; ++k) x.w[k] = w[4 * v + k];
      __builtin_memcpy(__builtin_assume_aligned(p + 16 * v, 16), &x, 16);
    }
  } else if ((a & 3) == 0) {
    for (int k = 0; k < 12; ++k) __builtin_memcpy(__builtin_assume_aligned(p + 4 * k, 4), &w[k], 4);
  } else {
    for (uint32_t j = 0; j < kPngColorChunk; ++j) p[j] = static_cast<unsigned char>(PngColorChunkByte(w, j));
  }
}

// Pixel j of a chunk in its 8-bit view (CH channels of SB bytes, the high byte first): alpha, and kPngLossyHas | r | g << 8 | b << 16.
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline uint32_t PngLossyAlpha(const uint32_t* w, uint32_t j) { return PngColorChunkByte(w, j * CH * SB + (CH - 1) * SB); }
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline uint32_t PngLossyRgb(const uint32_t* w, uint32_t j) {
  const uint32_t at = j * CH * SB;
  if (CH == 2) return kPngLossyHas | PngColorChunkByte(w, at) * 0x010101u;
  return kPngLossyHas | PngColorChunkByte(w, at) | (PngColorChunkByte(w, at + SB) << 8) | (PngColorChunkByte(w, at + 2 * SB) << 16);
}
ZMX_PNGC_HD inline void PngLossySetByte(uint32_t* w, uint32_t j, uint32_t v) {
  w[j >> 2] = (w[j >> 2] & ~(255u << (8 * (j & 3)))) | (v << (8 * (j & 3)));
}
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline void PngLossySetRgb(uint32_t* w, uint32_t j, uint32_t rgb) {
  const uint32_t at = j * CH * SB;
  PngLossySetByte(w, at, rgb & 255u);
  if (CH == 4) {
    PngLossySetByte(w, at + SB, (rgb >> 8) & 255u);
    PngLossySetByte(w, at + 2 * SB, (rgb >> 16) & 255u);
  }
}

// the RGB of the chunk's last pixel with a > 0, or kPngLossyNone
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline uint32_t PngLossyChunkLast(const uint32_t* w, uint32_t npix) {
  uint32_t last = kPngLossyNone;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < kPngColorChunk / (CH * SB); ++j) {
    if (j < npix && PngLossyAlpha<CH, SB>(w, j) != 0) last = PngLossyRgb<CH, SB>(w, j);
  }
  return last;
}

// ---- the statistics
// what a thread, a wave, a workgroup has seen
struct PngLossyAcc {
  uint32_t partial, first;
};
ZMX_PNGC_HD inline PngLossyAcc PngLossyAccNone() { return PngLossyAcc{0u, kPngLossyNoIndex}; }
ZMX_PNGC_HD inline void PngLossyAccJoin(PngLossyAcc* a, const PngLossyAcc& b) {
  a->partial |= b.partial;
  if (b.first < a->first) a->first = b.first;
}

// a thread's colour counting from tile to tile
struct PngLossyCounter {
  uint32_t last;
  bool have_last;
};

// a tile's first thread, before the tile: has another workgroup given up counting?
ZMX_PNGC_HD inline void PngLossyTileBegin(const PngLossyState* state, const PngColorGroup& grp) {
  if (PngColorPeek32(grp.stop) == 0 && PngColorPeek32(&state->color.overflow) != 0) PngColorOr32(grp.stop, kPngColorStopSeen);
}

// `color` seen at `index` by a thread whose workgroup still counts: into the workgroup's table unless the thread has just
// seen it or its slot holds an index no larger (one LDS read).  *stopped: the workgroup's stop word afterwards.
ZMX_PNGC_HD inline void PngLossyCount(const PngColorGroup& grp, PngLossyCounter* cnt, uint32_t color, uint32_t index, bool* stopped) {
  if (*stopped || (cnt->have_last && color == cnt->last)) return;
  cnt->last = color;
  cnt->have_last = true;
  const PngColorSlot cur = PngColorPeek64(grp.table + PngColorHash(color));
  if (cur != kPngColorEmpty && static_cast<uint32_t>(cur >> 32) == color && static_cast<uint32_t>(cur) <= index) return;
  PngColorInsert(grp.table, grp.count, grp.stop, kPngColorStopOwn, color, index);
  *stopped = PngColorPeek32(grp.stop) != 0;
}

// Thread `local`'s chunk of `tile`: what it saw is added to *acc, its colours go into the workgroup's table; the result
// is position << 32 | RGB of the chunk's last pixel with a > 0 (the largest over a tile is the tile's), or 0.
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline uint64_t PngLossyStatsChunk(const PngColorImage& I, const PngColorGroup& grp, uint64_t tile, uint32_t local,
                                               PngLossyAcc* acc, PngLossyCounter* cnt) {
  constexpr uint32_t bytes = CH * SB, per_chunk = kPngColorChunk / bytes;
  uint64_t first;
  const uint32_t npix = PngLossyChunkPixels<bytes>(I, tile, local, &first);
  if (npix == 0) return 0;
  uint32_t w[12];
  PngLossyLoad<bytes>(I.pixels + first * bytes, npix, w);
  bool stopped = PngColorPeek32(grp.stop) != 0;
  uint64_t key = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < per_chunk; ++j) {
    if (j < npix) {
      const uint32_t a = PngLossyAlpha<CH, SB>(w, j);
      const uint32_t index = static_cast<uint32_t>(first) + j;
      uint32_t color = 0;   // every transparent pixel is the colour 0
      if (a == 0) {
        if (acc->first == kPngLossyNoIndex) acc->first = index;   // (a thread's indices rise)
      } else {
        if (a != 255u) acc->partial = 1;
        const uint32_t rgb = PngLossyRgb<CH, SB>(w, j);
        key = (static_cast<uint64_t>(local * per_chunk + j + 1) << 32) | rgb;
        color = (rgb & 0xffffffu) | (a << 24);
      }
      PngLossyCount(grp, cnt, color, index, &stopped);
    }
  }
  return key;
}

template <typename... A>
ZMX_PNGC_HD inline uint64_t PngLossyStatsChunkOf(const PngColorImage& I, A... a) {
  if (I.colortype == 4) return I.bitdepth == 16 ? PngLossyStatsChunk<2, 2>(I, a...) : PngLossyStatsChunk<2, 1>(I, a...);
  return I.bitdepth == 16 ? PngLossyStatsChunk<4, 2>(I, a...) : PngLossyStatsChunk<4, 1>(I, a...);
}

ZMX_PNGC_HD inline uint32_t PngLossySummaryOf(uint64_t key) { return key == 0 ? kPngLossyNone : static_cast<uint32_t>(key); }

// a workgroup's sum into the state: one thread, and only what says something
ZMX_PNGC_HD inline void PngLossyGroupEnd(PngLossyState* state, const PngLossyAcc& sum, uint32_t stop) {
  if (sum.partial && !(PngColorPeek32(&state->color.flags) & kPngColorPartial)) PngColorOr32(&state->color.flags, kPngColorPartial);
  if (sum.first != kPngLossyNoIndex) PngColorMin32(&state->first_transparent, sum.first);
  if (stop & kPngColorStopOwn) PngColorOr32(&state->color.overflow, 1u);
}

// ---- the rewrite
// the 8-bit view of pixel `index` as a summary
ZMX_PNGC_HD inline uint32_t PngLossyPixelRgb(const PngColorImage& I, uint64_t index) {
  const uint32_t sb = I.bitdepth / 8;
  const unsigned char* p = I.pixels + index * PngColorPixelBytes(I.colortype, I.bitdepth);
  if (I.colortype == 4) return kPngLossyHas | p[0] * 0x010101u;
  return kPngLossyHas | p[0] | (static_cast<uint32_t>(p[sb]) << 8) | (static_cast<uint32_t>(p[2 * sb]) << 16);
}

// The chunk in w rewritten: every pixel with a = 0 gets `carry`'s RGB (none: 0, 0, 0); in carry mode the carry follows
// the pixels with a > 0.
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline void PngLossyRewrite(uint32_t* w, uint32_t npix, uint32_t carry, bool follow) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < kPngColorChunk / (CH * SB); ++j) {
    if (j < npix) {
      if (PngLossyAlpha<CH, SB>(w, j) == 0) PngLossySetRgb<CH, SB>(w, j, carry & 0xffffffu);
      else if (follow) carry = PngLossyRgb<CH, SB>(w, j);
    }
  }
}

// Thread `local`'s chunk of `tile`, first half: loaded into w, *npix its pixels; the result is what the chunk passes on
// in carry mode (PngLossyChunkLast), kPngLossyNone in fixed mode.
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline uint32_t PngLossyFillLoad(const PngLossyParams& P, uint64_t tile, uint32_t local, uint32_t* w, uint32_t* npix) {
  uint64_t first;
  *npix = PngLossyChunkPixels<CH * SB>(P.in, tile, local, &first);
  if (*npix == 0) return kPngLossyNone;
  PngLossyLoad<CH * SB>(P.in.pixels + first * (CH * SB), *npix, w);
  return P.mode == kPngLossyModeCarry ? PngLossyChunkLast<CH, SB>(w, *npix) : kPngLossyNone;
}
// second half: rewritten from `carry` — the fill colour, or what the chunks and tiles before this one pass on — and stored
template <uint32_t CH, uint32_t SB>
ZMX_PNGC_HD inline void PngLossyFillStore(const PngLossyParams& P, uint64_t tile, uint32_t local, uint32_t* w, uint32_t npix, uint32_t carry) {
  if (npix == 0) return;
  PngLossyRewrite<CH, SB>(w, npix, carry, P.mode == kPngLossyModeCarry);
  const uint64_t at = (tile * kPngLossyThreads + local) * kPngColorChunk;
  PngLossyStore<CH * SB>(P.out + at, npix, w);
}

template <typename... A>
ZMX_PNGC_HD inline uint32_t PngLossyFillLoadOf(const PngLossyParams& P, A... a) {
  if (P.in.colortype == 4) return P.in.bitdepth == 16 ? PngLossyFillLoad<2, 2>(P, a...) : PngLossyFillLoad<2, 1>(P, a...);
  return P.in.bitdepth == 16 ? PngLossyFillLoad<4, 2>(P, a...) : PngLossyFillLoad<4, 1>(P, a...);
}
template <typename... A>
ZMX_PNGC_HD inline void PngLossyFillStoreOf(const PngLossyParams& P, A... a) {
  if (P.in.colortype == 4) {
    if (P.in.bitdepth == 16) PngLossyFillStore<2, 2>(P, a...);
    else PngLossyFillStore<2, 1>(P, a...);
  } else {
    if (P.in.bitdepth == 16) PngLossyFillStore<4, 2>(P, a...);
    else PngLossyFillStore<4, 1>(P, a...);
  }
}

// ---- the state read on the host
struct PngLossyDecision {
  uint32_t mode, partial_alpha, numcolors;   // numcolors: 257 = more than 256
};
// zopflipng's choice: the fixed colour where a key or a palette stays possible, else the carry
inline PngLossyDecision PngLossyDecide(const PngLossyState& s) {
  PngLossyDecision d;
  d.partial_alpha = (s.color.flags & kPngColorPartial) ? 1u : 0u;
  d.numcolors = (s.color.overflow != 0 || s.color.count > kPngColorMaxColors) ? kPngColorMaxColors + 1 : s.color.count;
  const bool key = d.partial_alpha == 0, palette = d.numcolors <= kPngColorMaxColors;
  d.mode = s.first_transparent == kPngLossyNoIndex ? kPngLossyModeNone : (key || palette) ? kPngLossyModeFixed : kPngLossyModeCarry;
  return d;
}

}  // namespace zamd

#if defined(ZMX_PNG_LOSSY_KERNELS)

namespace zamd {

// The exclusive scan of `v` over the workgroup under PngLossyPick, seeded with `seed`; *total: the inclusive result of
// the last thread.  `tot`: 8 words of LDS, used alternately (`parity`), so a step costs one barrier.
__device__ inline uint32_t PngLossyGroupScan(uint32_t v, uint32_t seed, uint32_t* tot, uint32_t parity, uint32_t* total) {
  const uint32_t lane = threadIdx.x & (warpSize - 1), wave = threadIdx.x / warpSize, waves = blockDim.x / warpSize;
  uint32_t incl = v;
  for (uint32_t off = 1; off < static_cast<uint32_t>(warpSize); off <<= 1) {
    const uint32_t o = __shfl_up(incl, off);
    if (lane >= off) incl = PngLossyPick(o, incl);
  }
  uint32_t* mine = tot + 4 * (parity & 1u);
  if (lane == static_cast<uint32_t>(warpSize) - 1) mine[wave] = incl;
  const uint32_t before = __shfl_up(incl, 1);
  __syncthreads();
  uint32_t prefix = seed, all = seed;
  for (uint32_t k = 0; k < waves; ++k) {
    if (k < wave) prefix = PngLossyPick(prefix, mine[k]);
    all = PngLossyPick(all, mine[k]);
  }
  *total = all;
  return lane == 0 ? prefix : PngLossyPick(prefix, before);
}

}  // namespace zamd

__global__ __launch_bounds__(256) void k_png_lossy_stats(zamd::PngColorImage I, zamd::PngLossyState* state, uint32_t* summaries) {
  using namespace zamd;
  __shared__ PngColorSlot table[kPngColorSlots];
  __shared__ unsigned long long wave_key[2][4];
  __shared__ uint32_t count, stop, group_partial, group_first;
  const PngColorGroup grp{table, &count, &stop};
  const uint32_t local = threadIdx.x, lane = local & (warpSize - 1), wave = local / warpSize;
  PngColorGroupBegin(&state->color, grp, local);
  if (local == 0) {
    group_partial = 0;
    group_first = kPngLossyNoIndex;
  }
  __syncthreads();
  PngLossyAcc acc = PngLossyAccNone();
  PngLossyCounter cnt{0u, false};
  const uint64_t tiles = PngLossyTiles(I);
  uint32_t parity = 0;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
    if (local == 0) PngLossyTileBegin(state, grp);
    unsigned long long key = PngLossyStatsChunkOf(I, grp, tile, local, &acc, &cnt);
    for (int off = warpSize / 2; off > 0; off >>= 1) {
      const unsigned long long other = __shfl_xor(key, off);
      if (other > key) key = other;
    }
    if (lane == 0) wave_key[parity][wave] = key;
    __syncthreads();
    if (local == 0) {
      unsigned long long best = 0;
      for (uint32_t k = 0; k < kPngLossyThreads / warpSize; ++k) best = wave_key[parity][k] > best ? wave_key[parity][k] : best;
      summaries[tile] = PngLossySummaryOf(best);
    }
  }
  for (int off = warpSize / 2; off > 0; off >>= 1) {
    PngLossyAcc other;
    other.partial = __shfl_xor(acc.partial, off);
    other.first = __shfl_xor(acc.first, off);
    PngLossyAccJoin(&acc, other);
  }
  if (lane == 0) {
    if (acc.partial) atomicOr(&group_partial, 1u);
    if (acc.first != kPngLossyNoIndex) atomicMin(&group_first, acc.first);
  }
  __syncthreads();
  if (local == 0) PngLossyGroupEnd(state, PngLossyAcc{group_partial, group_first}, stop);
  PngColorGroupFlush(&state->color, grp, local);
}

// summaries[tiles] -> carry_in[tiles]; one workgroup
__global__ __launch_bounds__(256) void k_png_lossy_carry(const uint32_t* summaries, uint32_t* carry_in, uint64_t tiles) {
  using namespace zamd;
  __shared__ uint32_t tot[8];
  uint32_t carry = kPngLossyNone, parity = 0;
  for (uint64_t base = 0; base < tiles; base += kPngLossyScanStep, parity ^= 1u) {
    const uint64_t t = base + threadIdx.x;
    const uint32_t v = t < tiles ? summaries[t] : kPngLossyNone;
    uint32_t total;
    const uint32_t before = PngLossyGroupScan(v, carry, tot, parity, &total);
    if (t < tiles) carry_in[t] = before;
    carry = total;
  }
}

__global__ __launch_bounds__(256) void k_png_lossy_fill(zamd::PngLossyParams P) {
  using namespace zamd;
  __shared__ uint32_t tot[8];
  const uint32_t local = threadIdx.x;
  uint32_t fill = kPngLossyNone;
  if (P.mode == kPngLossyModeFixed) {
    fill = PngLossyPixelRgb(P.in, P.first_transparent);
    if (blockIdx.x == 0 && local == 0) P.state->fill = fill;
  }
  const uint64_t tiles = PngLossyTiles(P.in);
  uint32_t parity = 0;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
    uint32_t w[12], npix;
    const uint32_t v = PngLossyFillLoadOf(P, tile, local, w, &npix);
    uint32_t carry = fill;
    if (P.mode == kPngLossyModeCarry) {
      uint32_t total;
      carry = PngLossyGroupScan(v, P.carry_in[tile], tot, parity, &total);
    }
    PngLossyFillStoreOf(P, tile, local, w, npix, carry);
  }
}

#endif  // ZMX_PNG_LOSSY_KERNELS

#endif  // ZMX_PNG_LOSSY_H_
