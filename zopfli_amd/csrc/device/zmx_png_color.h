// zmx_png_color_stats_device, zmx_png_convert_device: LodePNG's colour statistics (lodepng.cpp lodepng_compute_color_stats)
// and its colour conversion (lodepng_convert, rgba8ToPixel, rgba16ToPixel) on an image in device memory — grey, RGB,
// grey + alpha or RGBA at 8 or 16 bits, every rule stated on the pixel's RGBA expansion as zopflipng sees it.
//   k_png_color_stats  one pass, at most kPngColorMaxBlocks workgroups.  A thread takes 48 bytes of the image a step —
//                      a whole number of pixels of every format — as three 16-byte loads where the image is 16-byte
//                      aligned (twelve words where it is 4-byte aligned, bytes otherwise).  The flags (coloured, an
//                      alpha that is neither 0 nor the maximum, a 16-bit sample whose bytes differ), the bits a grey
//                      value needs and the smallest and largest RGB among the transparent pixels stay in registers,
//                      are joined over the wave by shuffles, over the workgroup in LDS, and reach global memory once a
//                      workgroup, and only where they say something.  Colours go into a table of 512 slots in LDS
//                      first: a slot is colour << 32 | the smallest pixel index it was seen at, empty is all ones —
//                      no colour's slot, as an index stays below 2^32 - 1 — and a pixel whose colour the thread has
//                      just seen, or whose slot already holds a smaller index, costs one LDS read.  At its end a
//                      workgroup puts its slots into the global table the same way (compare-and-swap on the empty
//                      slot, a 64-bit minimum on its own colour's), so what the table ends with is a minimum of
//                      indices, not an order of arrival.  A workgroup that has seen more than 256 colours stops
//                      counting and says so in the state; the others look there when they start and every eighth step.
//                      A thread reads its workgroup's stop word before each chunk and after an insertion of its own,
//                      not per pixel: once the workgroup has stopped, a pixel costs registers only.
//   k_png_color_key    LodePNG's second loop: does a pixel that is not transparent have the key's RGB?  Launched only
//                      when one transparent RGB was found and no partial alpha.
//   k_png_convert      the image in another colour mode: rows of (width * bpp + 7) / 8 bytes back to back.  Threads
//                      stride over the aligned 16-byte vectors of the DESTINATION, head and tail bytes singly, every
//                      byte written exactly once and none outside.  For a palette the colour -> rank table (the same
//                      512 slots) is built in LDS by the workgroup first; a colour that is not in the palette is
//                      reported through *bad_pixel (the smallest such pixel) and written as rank 0.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/png_color_print.cc) runs the very code of
// the kernels, the threads one after the other.  This header compiles without HIP; the kernels are there for the device
// layer only (ZMX_PNG_COLOR_KERNELS).  Plain loads and stores and the HIP atomics, nothing else.
#ifndef ZMX_PNG_COLOR_H_
#define ZMX_PNG_COLOR_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMX_PNGC_HD __host__ __device__
#else
#define ZMX_PNGC_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ZMX_PNGC_NOINLINE inline __attribute__((noinline))
#else
#define ZMX_PNGC_NOINLINE inline
#endif

namespace zamd {

constexpr uint32_t kPngColorThreads = 256;      // a workgroup: four waves
constexpr uint32_t kPngColorMaxBlocks = 2048;   // the grid's cap: 8 workgroups for each of 256 CUs
constexpr uint32_t kPngColorSlots = 512;        // of a colour table, in LDS and in the state: twice the colours a palette takes
constexpr uint32_t kPngColorChunk = 48;         // bytes a thread takes a step: whole pixels of 1, 2, 3, 4, 6 and 8 bytes
constexpr uint32_t kPngColorMaxColors = 256;
constexpr uint32_t kPngColorNoBadPixel = 0xffffffffu;

typedef unsigned long long PngColorSlot;        // colour << 32 | pixel index (stats) or rank (convert)
constexpr PngColorSlot kPngColorEmpty = ~0ull;

// PngColorState::flags
constexpr uint32_t kPngColorColored = 1, kPngColorPartial = 2, kPngColorSixteen = 4;
// why a workgroup stopped counting: more than 256 colours of its own, the state said so, a true 16-bit sample
constexpr uint32_t kPngColorStopOwn = 1, kPngColorStopSeen = 2, kPngColorStopSixteen = 4;

// What the statistics kernels leave in device memory.  Before the launch: zeros up to key_min, all ones from there on.
struct PngColorState {
  uint32_t flags;          // kPngColorColored | kPngColorPartial | kPngColorSixteen
  uint32_t bits;           // the largest getValueRequiredBits(r); 0: no pixel said more than 1
  uint32_t overflow;       // more than 256 colours (the table then holds some of them)
  uint32_t count;          // slots taken
  PngColorSlot key_max;    // the largest r << 32 | g << 16 | b among the pixels with alpha 0
  uint32_t key_clash;      // k_png_color_key: a pixel with another alpha has the key's RGB
  uint32_t reserved;
  PngColorSlot key_min;    // the smallest; all ones: no pixel has alpha 0
  PngColorSlot table[kPngColorSlots];
};

struct PngColorImage {
  const unsigned char* pixels;   // PNG byte order, rows back to back
  uint64_t numpixels;            // below 2^32
  uint32_t width, height, colortype /* 0, 2, 4, 6 */, bitdepth /* 8, 16 */;
};

struct PngColorPx { uint32_t r, g, b, a; };   // at the image's own depth

ZMX_PNGC_HD inline uint32_t PngColorChannels(uint32_t colortype) { return colortype == 0 ? 1u : colortype == 2 ? 3u : colortype == 4 ? 2u : 4u; }
ZMX_PNGC_HD inline uint32_t PngColorPixelBytes(uint32_t colortype, uint32_t bitdepth) { return PngColorChannels(colortype) * (bitdepth / 8); }

// ---- atomics: HIP's on the device, plain code where the threads run one after the other
ZMX_PNGC_HD inline PngColorSlot PngColorCas(PngColorSlot* p, PngColorSlot expect, PngColorSlot v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, v);
#else
  const PngColorSlot old = *p;
  if (old == expect) *p = v;
  return old;
#endif
}
ZMX_PNGC_HD inline void PngColorMin64(PngColorSlot* p, PngColorSlot v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}
ZMX_PNGC_HD inline void PngColorMax64(PngColorSlot* p, PngColorSlot v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  if (v > *p) *p = v;
#endif
}
ZMX_PNGC_HD inline uint32_t PngColorAdd32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicAdd(p, v);
#else
  const uint32_t old = *p;
  *p = old + v;
  return old;
#endif
}
ZMX_PNGC_HD inline void PngColorOr32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}
ZMX_PNGC_HD inline void PngColorMax32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  if (v > *p) *p = v;
#endif
}
ZMX_PNGC_HD inline void PngColorMin32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}
ZMX_PNGC_HD inline PngColorSlot PngColorPeek64(const PngColorSlot* p) { return *static_cast<const volatile PngColorSlot*>(p); }
ZMX_PNGC_HD inline uint32_t PngColorPeek32(const uint32_t* p) { return *static_cast<const volatile uint32_t*>(p); }

// ---- the colour table
ZMX_PNGC_HD inline uint32_t PngColorHash(uint32_t color) { return (color * 0x9E3779B1u) >> 23; }   // 9 bits: kPngColorSlots

// `color` seen at `value` (a pixel index): its slot ends with the smallest value.  A slot newly taken counts; past 256 of
// them, or with every slot another colour's, `stopbit` is set in *stop.  (Out of line on the device: the walk over a
// chunk is unrolled up to 48 times, and this is the rare path.)
ZMX_PNGC_HD ZMX_PNGC_NOINLINE void PngColorInsert(PngColorSlot* table, uint32_t* count, uint32_t* stop, uint32_t stopbit, uint32_t color,
                                       uint32_t value) {
  const PngColorSlot mine = (static_cast<PngColorSlot>(color) << 32) | value;
  uint32_t s = PngColorHash(color);
  for (uint32_t probe = 0; probe < kPngColorSlots; ++probe, s = (s + 1) & (kPngColorSlots - 1)) {
    PngColorSlot cur = PngColorPeek64(table + s);
    if (cur == kPngColorEmpty) {
      cur = PngColorCas(table + s, kPngColorEmpty, mine);
      if (cur == kPngColorEmpty) {
        if (PngColorAdd32(count, 1) + 1 > kPngColorMaxColors) PngColorOr32(stop, stopbit);
        return;
      }
    }
    // (cur is a taken slot here: the empty one never reaches this comparison, so FFFFFFFF is a colour like any other)
    if (static_cast<uint32_t>(cur >> 32) == color) {
      if (static_cast<uint32_t>(cur) > value) PngColorMin64(table + s, mine);
      return;
    }
  }
  PngColorOr32(stop, stopbit);
}

// The value `color`'s slot holds, or -1.
ZMX_PNGC_HD inline int PngColorFind(const PngColorSlot* table, uint32_t color) {
  uint32_t s = PngColorHash(color);
  for (uint32_t probe = 0; probe < kPngColorSlots; ++probe, s = (s + 1) & (kPngColorSlots - 1)) {
    const PngColorSlot cur = table[s];
    if (cur == kPngColorEmpty) return -1;
    if (static_cast<uint32_t>(cur >> 32) == color) return static_cast<int>(static_cast<uint32_t>(cur));
  }
  return -1;
}

// ---- pixels
// lodepng.cpp:3684 getValueRequiredBits
ZMX_PNGC_HD inline uint32_t PngColorValueBits(uint32_t v) {
  if (v == 0 || v == 255) return 1;
  if ((v & 15u) != (v >> 4)) return 8;                    // no multiple of 17
  return (v & 3u) == ((v >> 2) & 3u) ? 2u : 4u;            // the nibble 0, 5, 10, 15: a multiple of 85
}

// the pixel whose bytes begin at p
ZMX_PNGC_HD inline PngColorPx PngColorDecode(const unsigned char* p, uint32_t colortype, uint32_t bitdepth) {
  uint32_t s[4] = {0, 0, 0, 0};
  const uint32_t channels = PngColorChannels(colortype);
  for (uint32_t k = 0; k < channels; ++k) s[k] = bitdepth == 16 ? (static_cast<uint32_t>(p[2 * k]) << 8) | p[2 * k + 1] : p[k];
  const uint32_t max = bitdepth == 16 ? 65535u : 255u;
  PngColorPx px;
  if (colortype == 0) px = {s[0], s[0], s[0], max};
  else if (colortype == 2) px = {s[0], s[1], s[2], max};
  else if (colortype == 4) px = {s[0], s[0], s[0], s[1]};
  else px = {s[0], s[1], s[2], s[3]};
  return px;
}

// the pixel's bytes r, g, b, a of LodePNG's 8-bit view (the high bytes of 16-bit samples), as a palette entry lies in memory
ZMX_PNGC_HD inline uint32_t PngColorOf(const PngColorPx& px, uint32_t bitdepth) {
  const uint32_t sh = bitdepth == 16 ? 8u : 0u;
  return (px.r >> sh) | ((px.g >> sh) << 8) | ((px.b >> sh) << 16) | ((px.a >> sh) << 24);
}
ZMX_PNGC_HD inline PngColorSlot PngColorRgbOf(const PngColorPx& px) {
  return (static_cast<PngColorSlot>(px.r) << 32) | (static_cast<PngColorSlot>(px.g) << 16) | px.b;
}

// the aligned word at p
ZMX_PNGC_HD inline uint32_t PngColorLoadWord(const unsigned char* p) {
  uint32_t v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}

struct alignas(16) PngColorVec { uint32_t w[4]; };

// The kPngColorChunk bytes at p, all of them the image's, as twelve little-endian words.
ZMX_PNGC_HD inline void PngColorLoadChunk(const unsigned char* p, uint32_t* w) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) {
    for (int v = 0; v < 3; ++v) {
      PngColorVec x;
      __builtin_memcpy(&x, __builtin_assume_aligned(p + 16 * v, 16), 16);
      for (int k = 0; k < 4; ++k) w[4 * v + k] = x.w[k];
    }
  } else if ((a & 3) == 0) {
    for (int k = 0; k < 12; ++k) w[k] = PngColorLoadWord(p + 4 * k);
  } else {
    for (int k = 0; k < 12; ++k) {
      w[k] = static_cast<uint32_t>(p[4 * k]) | (static_cast<uint32_t>(p[4 * k + 1]) << 8) | (static_cast<uint32_t>(p[4 * k + 2]) << 16) |
             (static_cast<uint32_t>(p[4 * k + 3]) << 24);
    }
  }
}

ZMX_PNGC_HD inline uint32_t PngColorChunkByte(const uint32_t* w, uint32_t j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }

// pixel j of a chunk (CT, D the image's colour type and depth: constants, so the loop over j unrolls into shifts)
template <uint32_t CT, uint32_t D>
ZMX_PNGC_HD inline PngColorPx PngColorChunkPixel(const uint32_t* w, uint32_t j) {
  constexpr uint32_t channels = CT == 0 ? 1 : CT == 2 ? 3 : CT == 4 ? 2 : 4;
  constexpr uint32_t bytes = channels * (D / 8);
  uint32_t s[4] = {0, 0, 0, 0};
  for (uint32_t k = 0; k < channels; ++k) {
    const uint32_t at = j * bytes + k * (D / 8);
    s[k] = D == 16 ? (PngColorChunkByte(w, at) << 8) | PngColorChunkByte(w, at + 1) : PngColorChunkByte(w, at);
  }
  constexpr uint32_t max = D == 16 ? 65535u : 255u;
  PngColorPx px;
  if (CT == 0) px = {s[0], s[0], s[0], max};
  else if (CT == 2) px = {s[0], s[1], s[2], max};
  else if (CT == 4) px = {s[0], s[0], s[0], s[1]};
  else px = {s[0], s[1], s[2], s[3]};
  return px;
}

// Thread `thread` of `threads` (at least kPngColorChunk) visits its share of the pixels in rising order: f(pixel, index).
// `step(k)` runs before the thread's k-th chunk.
template <uint32_t CT, uint32_t D, typename F, typename S>
ZMX_PNGC_HD inline void PngColorWalkAs(const PngColorImage& I, uint64_t thread, uint64_t threads, F& f, S& step) {
  constexpr uint32_t channels = CT == 0 ? 1 : CT == 2 ? 3 : CT == 4 ? 2 : 4;
  constexpr uint32_t bytes = channels * (D / 8);
  constexpr uint32_t per_chunk = kPngColorChunk / bytes;
  const uint64_t chunks = I.numpixels / per_chunk;
  uint32_t k = 0;
  for (uint64_t c = thread; c < chunks; c += threads, ++k) {
    step(k);
    uint32_t w[12];
    PngColorLoadChunk(I.pixels + c * kPngColorChunk, w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < per_chunk; ++j) f(PngColorChunkPixel<CT, D>(w, j), c * per_chunk + j);
  }
  // (the pixels behind the last whole chunk, fewer than 48, on the last threads)
  const uint64_t done = chunks * per_chunk, back = threads - 1 - thread;
  if (back < I.numpixels - done) {
    const uint64_t i = I.numpixels - 1 - back;
    step(k);
    f(PngColorDecode(I.pixels + i * bytes, CT, D), i);
  }
}

template <typename F, typename S>
ZMX_PNGC_HD inline void PngColorWalk(const PngColorImage& I, uint64_t thread, uint64_t threads, F& f, S& step) {
  const uint32_t fmt = I.colortype * 2 + (I.bitdepth == 16 ? 1 : 0);
  switch (fmt) {
    case 0: PngColorWalkAs<0, 8>(I, thread, threads, f, step); break;
    case 1: PngColorWalkAs<0, 16>(I, thread, threads, f, step); break;
    case 4: PngColorWalkAs<2, 8>(I, thread, threads, f, step); break;
    case 5: PngColorWalkAs<2, 16>(I, thread, threads, f, step); break;
    case 8: PngColorWalkAs<4, 8>(I, thread, threads, f, step); break;
    case 9: PngColorWalkAs<4, 16>(I, thread, threads, f, step); break;
    case 12: PngColorWalkAs<6, 8>(I, thread, threads, f, step); break;
    case 13: PngColorWalkAs<6, 16>(I, thread, threads, f, step); break;
    default: break;
  }
}

// the workgroups of a launch over the image
ZMX_PNGC_HD inline uint32_t PngColorGrid(const PngColorImage& I) {
  const uint64_t chunks = I.numpixels * PngColorPixelBytes(I.colortype, I.bitdepth) / kPngColorChunk;
  const uint64_t blocks = (chunks + kPngColorThreads - 1) / kPngColorThreads;
  return static_cast<uint32_t>(blocks == 0 ? 1 : blocks < kPngColorMaxBlocks ? blocks : kPngColorMaxBlocks);
}

// ---- the statistics
// what a thread, a wave, a workgroup has seen
struct PngColorAcc {
  uint32_t flags, bits;
  PngColorSlot key_min, key_max;
};
ZMX_PNGC_HD inline PngColorAcc PngColorAccNone() { return PngColorAcc{0u, 0u, kPngColorEmpty, 0ull}; }

// a workgroup's colour table and its two words (LDS on the device)
struct PngColorGroup {
  PngColorSlot* table;
  uint32_t* count;
  uint32_t* stop;   // kPngColorStop*: not 0 = the workgroup counts no more
};

struct PngColorSeer {
  const uint32_t bitdepth;
  PngColorAcc* acc;
  const PngColorGroup* grp;
  uint32_t last;
  bool have_last;
  bool stopped;   // *grp->stop as this thread saw it last: before each chunk and after each insertion of its own
  ZMX_PNGC_HD void operator()(const PngColorPx& px, uint64_t index) {
    const uint32_t max = bitdepth == 16 ? 65535u : 255u;
    uint32_t flags = 0;
    if (px.r != px.g || px.r != px.b) flags |= kPngColorColored;
    if (px.a != max) {
      if (px.a != 0) {
        flags |= kPngColorPartial;
      } else {
        const PngColorSlot rgb = PngColorRgbOf(px);
        if (rgb < acc->key_min) acc->key_min = rgb;
        if (rgb > acc->key_max) acc->key_max = rgb;
      }
    }
    if (bitdepth == 16) {
      const uint32_t differ = ((px.r ^ (px.r >> 8)) | (px.g ^ (px.g >> 8)) | (px.b ^ (px.b >> 8)) | (px.a ^ (px.a >> 8))) & 255u;
      if (differ) {
        if (!(acc->flags & kPngColorSixteen)) PngColorOr32(grp->stop, kPngColorStopSixteen);
        flags |= kPngColorSixteen;
      }
    }
    acc->flags |= flags;
    const uint32_t bits = PngColorValueBits(bitdepth == 16 ? px.r >> 8 : px.r);
    if (bits > acc->bits) acc->bits = bits;
    const uint32_t color = PngColorOf(px, bitdepth);
    // (a pixel of a photograph ends here, in registers: the workgroup stopped counting within its first chunks)
    if (stopped || (have_last && color == last)) return;   // (the same colour: seen by this thread at a smaller index)
    last = color;
    have_last = true;
    // (one LDS read where the colour sits in its first slot with an index no larger)
    const PngColorSlot cur = PngColorPeek64(grp->table + PngColorHash(color));
    if (cur != kPngColorEmpty && static_cast<uint32_t>(cur >> 32) == color && static_cast<uint32_t>(cur) <= index) return;
    PngColorInsert(grp->table, grp->count, grp->stop, kPngColorStopOwn, color, static_cast<uint32_t>(index));
    stopped = PngColorPeek32(grp->stop) != 0;
  }
};

struct PngColorStepper {
  const PngColorState* state;
  const PngColorGroup* grp;
  PngColorSeer* see;
  bool first_of_group;
  // (the workgroup's first thread looks whether another workgroup has given up counting; every thread, whether its own has)
  ZMX_PNGC_HD void operator()(uint32_t k) {
    if (first_of_group && (k & 7u) == 7u && PngColorPeek32(&state->overflow) != 0) PngColorOr32(grp->stop, kPngColorStopSeen);
    see->stopped = PngColorPeek32(grp->stop) != 0;
  }
};

// a workgroup's table and words before its threads run: slot `local` and the one 256 further
ZMX_PNGC_HD inline void PngColorGroupBegin(const PngColorState* state, const PngColorGroup& grp, uint32_t local) {
  for (uint32_t s = local; s < kPngColorSlots; s += kPngColorThreads) grp.table[s] = kPngColorEmpty;
  if (local == 0) {
    *grp.count = 0;
    *grp.stop = PngColorPeek32(&state->overflow) != 0 ? kPngColorStopSeen : 0u;
  }
}

// thread `local` of workgroup `group` of `groups`: what it saw is added to *acc
ZMX_PNGC_HD inline void PngColorStatsThread(const PngColorImage& I, const PngColorState* state, const PngColorGroup& grp, uint32_t group,
                                            uint32_t groups, uint32_t local, PngColorAcc* acc) {
  PngColorSeer see{I.bitdepth, acc, &grp, 0u, false, false};
  PngColorStepper step{state, &grp, &see, local == 0};
  PngColorWalk(I, static_cast<uint64_t>(group) * kPngColorThreads + local, static_cast<uint64_t>(groups) * kPngColorThreads, see, step);
}

ZMX_PNGC_HD inline void PngColorAccJoin(PngColorAcc* a, const PngColorAcc& b) {
  a->flags |= b.flags;
  if (b.bits > a->bits) a->bits = b.bits;
  if (b.key_min < a->key_min) a->key_min = b.key_min;
  if (b.key_max > a->key_max) a->key_max = b.key_max;
}

// a workgroup's sum into the state: one thread, and only what says something
ZMX_PNGC_HD inline void PngColorGroupEnd(PngColorState* state, const PngColorAcc& sum, uint32_t stop) {
  if (sum.flags & ~PngColorPeek32(&state->flags)) PngColorOr32(&state->flags, sum.flags);
  if (sum.bits > PngColorPeek32(&state->bits)) PngColorMax32(&state->bits, sum.bits);
  if (sum.key_min != kPngColorEmpty) {
    PngColorMin64(&state->key_min, sum.key_min);
    PngColorMax64(&state->key_max, sum.key_max);
  }
  if (stop & kPngColorStopOwn) PngColorOr32(&state->overflow, 1u);
}

// the workgroup's slots `local` and the one 256 further into the state's table, unless the counting has ended
ZMX_PNGC_HD inline void PngColorGroupFlush(PngColorState* state, const PngColorGroup& grp, uint32_t local) {
  if (PngColorPeek32(grp.stop) != 0 || PngColorPeek32(&state->overflow) != 0) return;
  for (uint32_t s = local; s < kPngColorSlots; s += kPngColorThreads) {
    const PngColorSlot cur = grp.table[s];
    if (cur == kPngColorEmpty) continue;
    PngColorInsert(state->table, &state->count, &state->overflow, 1u, static_cast<uint32_t>(cur >> 32), static_cast<uint32_t>(cur));
  }
}

// LodePNG's second loop
struct PngColorKeySeer {
  const PngColorSlot key;
  bool clash;
  ZMX_PNGC_HD void operator()(const PngColorPx& px, uint64_t) {
    if (px.a != 0 && PngColorRgbOf(px) == key) clash = true;
  }
};
struct PngColorNoStep {
  ZMX_PNGC_HD void operator()(uint32_t) {}
};
ZMX_PNGC_HD inline bool PngColorKeyThread(const PngColorImage& I, PngColorSlot key, uint64_t thread, uint64_t threads) {
  PngColorKeySeer see{key, false};
  PngColorNoStep step;
  PngColorWalk(I, thread, threads, see, step);
  return see.clash;
}

// ---- the conversion
struct PngConvParams {
  PngColorImage in;
  unsigned char* out;             // height * rowbytes bytes, any alignment
  uint64_t rowbytes;              // (width * bpp + 7) / 8
  uint32_t colortype, bitdepth;   // the output's: 0 at 1, 2, 4, 8, 16; 2, 4, 6 at 8, 16; 3 at 1, 2, 4, 8; 16 from a 16-bit image only
  uint32_t palettesize;           // colour type 3: 1 .. min(256, 2^bitdepth)
  const unsigned char* palette;   // palettesize entries r, g, b, a
  uint32_t* bad_pixel;            // kPngColorNoBadPixel before the launch; afterwards the first pixel whose colour the palette lacks
};

ZMX_PNGC_HD inline uint32_t PngConvBpp(uint32_t colortype, uint32_t bitdepth) {
  return (colortype == 3 ? 1u : PngColorChannels(colortype)) * bitdepth;
}
ZMX_PNGC_HD inline uint64_t PngConvRowBytes(uint32_t width, uint32_t colortype, uint32_t bitdepth) {
  return (static_cast<uint64_t>(width) * PngConvBpp(colortype, bitdepth) + 7) / 8;
}
ZMX_PNGC_HD inline uint32_t PngConvGrid(uint64_t total) {
  const uint64_t blocks = (total / 16 + kPngColorThreads - 1) / kPngColorThreads;
  return static_cast<uint32_t>(blocks == 0 ? 1 : blocks < kPngColorMaxBlocks ? blocks : kPngColorMaxBlocks);
}

// The palette into a workgroup's table: entry `local`.  Of two equal entries the later one gives the rank, as LodePNG's
// colour tree keeps the index added last.
ZMX_PNGC_HD inline void PngConvTableBegin(PngColorSlot* table, uint32_t local) {
  for (uint32_t s = local; s < kPngColorSlots; s += kPngColorThreads) table[s] = kPngColorEmpty;
}
ZMX_PNGC_HD inline void PngConvTableFill(const PngConvParams& P, PngColorSlot* table, uint32_t local) {
  if (P.colortype != 3) return;
  for (uint32_t i = local; i < P.palettesize; i += kPngColorThreads) {
    const unsigned char* e = P.palette + 4 * i;
    const uint32_t color = static_cast<uint32_t>(e[0]) | (static_cast<uint32_t>(e[1]) << 8) | (static_cast<uint32_t>(e[2]) << 16) |
                           (static_cast<uint32_t>(e[3]) << 24);
    const PngColorSlot mine = (static_cast<PngColorSlot>(color) << 32) | i;
    uint32_t s = PngColorHash(color);
    for (uint32_t probe = 0; probe < kPngColorSlots; ++probe, s = (s + 1) & (kPngColorSlots - 1)) {
      PngColorSlot cur = PngColorPeek64(table + s);
      if (cur == kPngColorEmpty) {
        cur = PngColorCas(table + s, kPngColorEmpty, mine);
        if (cur == kPngColorEmpty) break;
      }
      if (static_cast<uint32_t>(cur >> 32) == color) {
        PngColorMax64(table + s, mine);
        break;
      }
    }
  }
}

// the pixel a thread decoded last
struct PngConvCache {
  uint64_t index;
  PngColorPx px;     // 8-bit values unless the output is 16 bits deep
  uint32_t rank;
  bool have;
};

ZMX_PNGC_HD inline void PngConvFetch(const PngConvParams& P, const PngColorSlot* table, uint64_t index, PngConvCache* c) {
  if (c->have && c->index == index) return;
  const uint32_t bytes = PngColorPixelBytes(P.in.colortype, P.in.bitdepth);
  const unsigned char* p = P.in.pixels + index * bytes;
  unsigned char raw[8];
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (bytes == 4 && (a & 3) == 0) {
    const uint32_t w = PngColorLoadWord(p);
    __builtin_memcpy(raw, &w, 4);
  } else if (bytes == 8 && (a & 3) == 0) {
    const uint32_t w0 = PngColorLoadWord(p), w1 = PngColorLoadWord(p + 4);
    __builtin_memcpy(raw, &w0, 4);
    __builtin_memcpy(raw + 4, &w1, 4);
  } else {
    for (uint32_t k = 0; k < bytes; ++k) raw[k] = p[k];
  }
  PngColorPx px = PngColorDecode(raw, P.in.colortype, P.in.bitdepth);
  c->rank = 0;
  if (P.colortype == 3) {
    const int rank = PngColorFind(table, PngColorOf(px, P.in.bitdepth));
    if (rank < 0) PngColorMin32(P.bad_pixel, static_cast<uint32_t>(index));
    else c->rank = static_cast<uint32_t>(rank);
  }
  if (P.in.bitdepth == 16 && P.bitdepth != 16) px = {px.r >> 8, px.g >> 8, px.b >> 8, px.a >> 8};
  c->px = px;
  c->index = index;
  c->have = true;
}

// byte x of row `row` of the output
ZMX_PNGC_HD inline uint32_t PngConvByte(const PngConvParams& P, const PngColorSlot* table, uint64_t row, uint64_t x, PngConvCache* c) {
  const uint32_t bpp = PngConvBpp(P.colortype, P.bitdepth);
  const uint64_t first = row * P.in.width;
  if (bpp < 8) {
    // most significant bits first; the bits behind the row's last pixel are zero
    const uint32_t per_byte = 8 / bpp;
    uint32_t byte = 0;
    for (uint32_t k = 0; k < per_byte; ++k) {
      const uint64_t col = x * per_byte + k;
      if (col >= P.in.width) break;
      PngConvFetch(P, table, first + col, c);
      const uint32_t v = P.colortype == 3 ? c->rank : c->px.r >> (8 - P.bitdepth);
      byte |= (v & ((1u << bpp) - 1u)) << (8 - bpp * (k + 1));
    }
    return byte;
  }
  const uint32_t width = bpp / 8, sample_bytes = P.bitdepth / 8;
  const uint32_t xx = static_cast<uint32_t>(x);   // (a row has at most 2^31 - 1 bytes)
  const uint32_t col = xx / width, at = xx - col * width, sample = at / sample_bytes;
  PngConvFetch(P, table, first + col, c);
  uint32_t v;
  if (P.colortype == 3) v = c->rank;
  else if (P.colortype == 0) v = c->px.r;
  else if (P.colortype == 4) v = sample == 0 ? c->px.r : c->px.a;
  else v = sample == 0 ? c->px.r : sample == 1 ? c->px.g : sample == 2 ? c->px.b : c->px.a;
  if (sample_bytes == 2) return (at & 1u) ? v & 255u : (v >> 8) & 255u;
  return v & 255u;
}

ZMX_PNGC_HD inline void PngConvAt(uint64_t o, uint64_t rowbytes, uint64_t* row, uint64_t* x) {
  if ((o >> 32) == 0 && (rowbytes >> 32) == 0) *row = static_cast<uint32_t>(o) / static_cast<uint32_t>(rowbytes);
  else *row = o / rowbytes;
  *x = o - *row * rowbytes;
}

// Thread `thread` of `threads` (at least 16) writes its share of the output; `table` is its workgroup's.
ZMX_PNGC_HD inline void PngConvRun(const PngConvParams& P, const PngColorSlot* table, uint64_t thread, uint64_t threads) {
  const uint64_t total = P.in.height * P.rowbytes;
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(P.out) & 15)) & 15;
  if (head > total) head = total;
  const uint64_t nvec = (total - head) / 16;
  PngConvCache cache;
  cache.have = false;
  uint64_t row, x;
  if (thread < head) {
    PngConvAt(thread, P.rowbytes, &row, &x);
    P.out[thread] = static_cast<unsigned char>(PngConvByte(P, table, row, x, &cache));
  }
  for (uint64_t v = thread; v < nvec; v += threads) {
    PngConvAt(head + 16 * v, P.rowbytes, &row, &x);
    PngColorVec vec = {{0, 0, 0, 0}};
    for (int j = 0; j < 16; ++j) {
      vec.w[j >> 2] |= PngConvByte(P, table, row, x, &cache) << (8 * (j & 3));
      if (++x == P.rowbytes) { x = 0; ++row; }
    }
    __builtin_memcpy(__builtin_assume_aligned(P.out + head + 16 * v, 16), &vec, 16);
  }
  const uint64_t done = head + 16 * nvec, back = threads - 1 - thread;
  if (back < total - done) {
    PngConvAt(done + back, P.rowbytes, &row, &x);
    P.out[done + back] = static_cast<unsigned char>(PngConvByte(P, table, row, x, &cache));
  }
}

// ---- the state read on the host: LodePNG's LodePNGColorStats (the layout of zmx_png_color_stats, include/zopfli_amd.h)
struct PngColorSummary {
  uint32_t colored, key, alpha, numcolors, bits;
  uint16_t key_r, key_g, key_b, reserved;
  unsigned char palette[4 * kPngColorMaxColors];
};

// One RGB among the transparent pixels and no partial alpha: k_png_color_key has to say whether a key can be used.
inline bool PngColorWantsKeyPass(const PngColorState& s) {
  return !(s.flags & kPngColorPartial) && s.key_min != kPngColorEmpty && s.key_min == s.key_max;
}

// The statistics of an image of `bitdepth` from its state (after k_png_color_key where PngColorWantsKeyPass).  The key's
// values are zero without a key; the palette holds numcolors entries when that is at most 256, zeros behind them; no
// colours are counted (numcolors 0) for a true 16-bit image.
inline void PngColorFinish(const PngColorState& s, uint32_t bitdepth, PngColorSummary* out) {
  *out = PngColorSummary();
  const bool sixteen = bitdepth == 16 && (s.flags & kPngColorSixteen) != 0;
  out->colored = (s.flags & kPngColorColored) ? 1u : 0u;
  const bool transparent = s.key_min != kPngColorEmpty;
  if (s.flags & kPngColorPartial) out->alpha = 1;
  else if (transparent && (s.key_min != s.key_max || s.key_clash != 0)) out->alpha = 1;
  else if (transparent) out->key = 1;
  if (out->key) {
    const uint32_t scale = bitdepth == 16 ? 1u : 257u;   // (8-bit values with their byte twice, as LodePNG keeps them)
    out->key_r = static_cast<uint16_t>(((s.key_min >> 32) & 0xffffu) * scale);
    out->key_g = static_cast<uint16_t>(((s.key_min >> 16) & 0xffffu) * scale);
    out->key_b = static_cast<uint16_t>((s.key_min & 0xffffu) * scale);
  }
  if (sixteen) {
    out->bits = 16;
    return;
  }
  out->bits = s.bits == 0 ? 1u : s.bits;
  if ((out->colored || out->alpha) && out->bits < 8) out->bits = 8;
  if (s.overflow != 0) {
    out->numcolors = kPngColorMaxColors + 1;
    return;
  }
  // first-appearance order: by the smallest index (insertion sort over at most 256 slots)
  PngColorSlot byindex[kPngColorSlots];
  uint32_t n = 0;
  for (uint32_t i = 0; i < kPngColorSlots; ++i) {
    const PngColorSlot cur = s.table[i];
    if (cur == kPngColorEmpty) continue;
    uint32_t at = n++;
    for (; at > 0 && static_cast<uint32_t>(byindex[at - 1]) > static_cast<uint32_t>(cur); --at) byindex[at] = byindex[at - 1];
    byindex[at] = cur;
  }
  if (n > kPngColorMaxColors) {
    out->numcolors = kPngColorMaxColors + 1;
    return;
  }
  out->numcolors = n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t color = static_cast<uint32_t>(byindex[i] >> 32);
    for (int k = 0; k < 4; ++k) out->palette[4 * i + k] = static_cast<unsigned char>(color >> (8 * k));
  }
}

}  // namespace zamd

#if defined(ZMX_PNG_COLOR_KERNELS)

__global__ __launch_bounds__(256) void k_png_color_stats(zamd::PngColorImage I, zamd::PngColorState* state) {
  using namespace zamd;
  __shared__ PngColorSlot table[kPngColorSlots];
  __shared__ PngColorSlot group_min, group_max;
  __shared__ uint32_t count, stop, group_flags, group_bits;
  const PngColorGroup grp{table, &count, &stop};
  const uint32_t local = threadIdx.x;
  PngColorGroupBegin(state, grp, local);
  if (local == 0) {
    group_flags = 0;
    group_bits = 0;
    group_min = kPngColorEmpty;
    group_max = 0;
  }
  __syncthreads();
  PngColorAcc acc = PngColorAccNone();
  PngColorStatsThread(I, state, grp, blockIdx.x, gridDim.x, local, &acc);
  // over the wave by shuffles, over the workgroup in LDS
  for (int off = warpSize / 2; off > 0; off >>= 1) {
    PngColorAcc other;
    other.flags = __shfl_xor(acc.flags, off);
    other.bits = __shfl_xor(acc.bits, off);
    other.key_min = __shfl_xor(acc.key_min, off);
    other.key_max = __shfl_xor(acc.key_max, off);
    PngColorAccJoin(&acc, other);
  }
  if ((local & (warpSize - 1)) == 0) {
    if (acc.flags) atomicOr(&group_flags, acc.flags);
    if (acc.bits) atomicMax(&group_bits, acc.bits);
    if (acc.key_min != kPngColorEmpty) {
      atomicMin(&group_min, acc.key_min);
      atomicMax(&group_max, acc.key_max);
    }
  }
  __syncthreads();
  if (local == 0) PngColorGroupEnd(state, PngColorAcc{group_flags, group_bits, group_min, group_max}, stop);
  PngColorGroupFlush(state, grp, local);
}

__global__ __launch_bounds__(256) void k_png_color_key(zamd::PngColorImage I, zamd::PngColorSlot key, zamd::PngColorState* state) {
  const bool clash = zamd::PngColorKeyThread(I, key, static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x,
                                             static_cast<uint64_t>(gridDim.x) * blockDim.x);
  // (one store a wave that found one)
  if (__any(clash) && (threadIdx.x & (warpSize - 1)) == 0) atomicOr(&state->key_clash, 1u);
}

__global__ __launch_bounds__(256) void k_png_convert(zamd::PngConvParams P) {
  using namespace zamd;
  __shared__ PngColorSlot table[kPngColorSlots];
  PngConvTableBegin(table, threadIdx.x);
  __syncthreads();
  PngConvTableFill(P, table, threadIdx.x);
  __syncthreads();
  PngConvRun(P, table, static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, static_cast<uint64_t>(gridDim.x) * blockDim.x);
}

#endif  // ZMX_PNG_COLOR_KERNELS

#endif  // ZMX_PNG_COLOR_H_
