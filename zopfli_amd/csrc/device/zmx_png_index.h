// zmx_png_index_use_device, zmx_png_index_convert_device: an index image in device memory — palette indices at 1, 2, 4 or 8
// bits, grey at 1, 2 or 4 — rows of (width * bitdepth + 7) / 8 bytes back to back, the first pixel in a byte's top bits.
// Everything LodePNG does to such an image follows from the host's palette and one fact about the pixels: at which pixel
// each of the 256 values first appears (host/png_index.h).  So there are two kernels and no RGBA expansion.
//   k_png_index_use      one pass, at most kPngColorMaxBlocks workgroups.  Threads stride over the aligned 16-byte
//                        vectors of the IMAGE, head and tail bytes singly — the rows lie back to back, so a row's start
//                        needs no alignment — and a byte's row and column say which of its bits are pixels: the padding
//                        bits behind a row's last pixel are never looked at.  A workgroup keeps 256 words in LDS, the
//                        smallest raster index each value was seen at (all ones: not seen).  A thread walks its pixels
//                        in rising order, so a value it has just seen costs a register compare; otherwise one LDS read,
//                        and an atomic minimum only where the thread's index is below what the slot holds — a flat image
//                        does not serialise on one address.  At its end a workgroup puts the slots it took into the
//                        global table the same way, thread k slot k.  What the table ends with is a minimum of positions,
//                        not an order of arrival: equal from run to run.
//   k_png_index_convert  the image through a table of 256 entries of up to 4 bytes (the first output byte in the entry's
//                        low byte) into any output mode: a palette or grey at 1, 2, 4 or 8 bits — the entry is the new
//                        index or the grey value —, grey + alpha, RGB or RGBA at 8 bits.  Threads stride over the aligned
//                        16-byte vectors of the DESTINATION as k_png_convert's do, every byte written exactly once and
//                        none outside; pixels below 8 bits are packed most significant bits first and rows padded with
//                        zero bits.  The table lies in LDS.  A value at or above `palettesize` is outside the table: the
//                        smallest such pixel is reported through *bad_pixel and written as entry 0.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/png_index_print.cc) runs the very code of
// the kernels, the threads one after the other.  This header compiles without HIP; the kernels are there for the device
// layer only (ZMX_PNG_INDEX_KERNELS).  Plain loads and stores and the HIP atomics, nothing else.
#ifndef ZMX_PNG_INDEX_H_
#define ZMX_PNG_INDEX_H_

#include <stddef.h>
#include <stdint.h>

#include "zmx_png_color.h"   // the atomics, PngColorVec, PngConvBpp, PngConvRowBytes, PngConvAt, PngConvGrid

namespace zamd {

constexpr uint32_t kPngIndexThreads = kPngColorThreads;   // a workgroup: four waves, and a thread for each value
constexpr uint32_t kPngIndexValues = 256;
constexpr uint32_t kPngIndexNone = 0xffffffffu;           // no pixel: an index stays below 2^32 - 1

struct PngIndexImage {
  const unsigned char* pixels;   // height rows of linebytes bytes, any alignment
  uint64_t linebytes;            // (width * bitdepth + 7) / 8
  uint32_t width, height, bitdepth /* 1, 2, 4, 8 */;
};

ZMX_PNGC_HD inline uint64_t PngIndexLineBytes(uint32_t width, uint32_t bitdepth) { return (static_cast<uint64_t>(width) * bitdepth + 7) / 8; }
// the workgroups of a launch over `total` bytes, read or written sixteen at a time
ZMX_PNGC_HD inline uint32_t PngIndexGrid(uint64_t total) { return PngConvGrid(total); }
// pixel k of a byte, the first in its top bits
ZMX_PNGC_HD inline uint32_t PngIndexValueOf(uint32_t byte, uint32_t k, uint32_t bitdepth) {
  return (byte >> (8u - bitdepth * (k + 1u))) & ((1u << bitdepth) - 1u);
}

// ---- first appearances
struct PngIndexSeer {
  uint32_t* table;   // the workgroup's 256 words
  uint32_t last;
  bool have_last;
  ZMX_PNGC_HD void operator()(uint32_t value, uint32_t index) {
    if (have_last && value == last) return;   // (seen by this thread at a smaller index)
    last = value;
    have_last = true;
    if (index < PngColorPeek32(table + value)) PngColorMin32(table + value, index);
  }
};

// the pixels of byte x of row `row`
ZMX_PNGC_HD inline void PngIndexUseByte(const PngIndexImage& I, uint32_t byte, uint64_t row, uint64_t x, PngIndexSeer* see) {
  const uint32_t per_byte = 8u / I.bitdepth;
  const uint64_t col0 = x * per_byte;
  for (uint32_t k = 0; k < per_byte; ++k) {
    if (col0 + k >= I.width) break;   // (padding bits are no pixels)
    (*see)(PngIndexValueOf(byte, k, I.bitdepth), static_cast<uint32_t>(row * I.width + col0 + k));
  }
}

ZMX_PNGC_HD inline void PngIndexGroupBegin(uint32_t* table, uint32_t local) {
  for (uint32_t s = local; s < kPngIndexValues; s += kPngIndexThreads) table[s] = kPngIndexNone;
}

// Thread `thread` of `threads` (at least 16) visits its share of the image's bytes in rising order.
ZMX_PNGC_HD inline void PngIndexUseRun(const PngIndexImage& I, uint32_t* table, uint64_t thread, uint64_t threads) {
  const uint64_t total = I.height * I.linebytes;
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(I.pixels) & 15)) & 15;
  if (head > total) head = total;
  const uint64_t nvec = (total - head) / 16;
  PngIndexSeer see{table, 0u, false};
  uint64_t row, x;
  if (thread < head) {
    PngConvAt(thread, I.linebytes, &row, &x);
    PngIndexUseByte(I, I.pixels[thread], row, x, &see);
  }
  for (uint64_t v = thread; v < nvec; v += threads) {
    PngConvAt(head + 16 * v, I.linebytes, &row, &x);
    PngColorVec vec;
    __builtin_memcpy(&vec, __builtin_assume_aligned(I.pixels + head + 16 * v, 16), 16);
    for (int j = 0; j < 16; ++j) {
      PngIndexUseByte(I, (vec.w[j >> 2] >> (8 * (j & 3))) & 255u, row, x, &see);
      if (++x == I.linebytes) { x = 0; ++row; }
    }
  }
  const uint64_t done = head + 16 * nvec, back = threads - 1 - thread;
  if (back < total - done) {
    PngConvAt(done + back, I.linebytes, &row, &x);
    PngIndexUseByte(I, I.pixels[done + back], row, x, &see);
  }
}

// the workgroup's slot `local` into the global table, where it says something
ZMX_PNGC_HD inline void PngIndexGroupFlush(const uint32_t* table, uint32_t* first, uint32_t local) {
  for (uint32_t s = local; s < kPngIndexValues; s += kPngIndexThreads) {
    const uint32_t cur = table[s];
    if (cur != kPngIndexNone && cur < PngColorPeek32(first + s)) PngColorMin32(first + s, cur);
  }
}

// ---- the conversion
struct PngIndexConvParams {
  PngIndexImage in;
  unsigned char* out;             // height * rowbytes bytes, any alignment
  uint64_t rowbytes;              // (width * bpp + 7) / 8 of the output's mode
  uint32_t colortype, bitdepth;   // the output's: 0 and 3 at 1, 2, 4, 8; 2, 4, 6 at 8 (host/png_index.h: PngIndexOutModeOk)
  uint32_t palettesize;           // the values below it have an entry
  const uint32_t* table;          // 256 entries
  uint32_t* bad_pixel;            // kPngIndexNone before the launch; afterwards the first pixel whose value has no entry
};

// the pixel a thread looked up last
struct PngIndexCache {
  uint64_t index;
  uint32_t entry;
  bool have;
};

// the entry of pixel `col` of row `row`; `table` is the workgroup's copy
ZMX_PNGC_HD inline uint32_t PngIndexFetch(const PngIndexConvParams& P, const uint32_t* table, uint64_t row, uint64_t col, PngIndexCache* c) {
  const uint64_t index = row * P.in.width + col;
  if (c->have && c->index == index) return c->entry;
  const uint64_t bit = col * P.in.bitdepth;
  const uint32_t byte = P.in.pixels[row * P.in.linebytes + (bit >> 3)];
  const uint32_t value = (byte >> (8u - P.in.bitdepth - static_cast<uint32_t>(bit & 7u))) & ((1u << P.in.bitdepth) - 1u);
  uint32_t entry = table[0];
  if (value < P.palettesize) {
    entry = table[value];
  } else if (static_cast<uint32_t>(index) < PngColorPeek32(P.bad_pixel)) {
    PngColorMin32(P.bad_pixel, static_cast<uint32_t>(index));
  }
  c->index = index;
  c->entry = entry;
  c->have = true;
  return entry;
}

// byte x of row `row` of the output
ZMX_PNGC_HD inline uint32_t PngIndexConvByte(const PngIndexConvParams& P, const uint32_t* table, uint64_t row, uint64_t x, PngIndexCache* c) {
  const uint32_t bpp = PngConvBpp(P.colortype, P.bitdepth);
  if (bpp < 8) {
    // most significant bits first; the bits behind the row's last pixel are zero
    const uint32_t per_byte = 8 / bpp;
    uint32_t byte = 0;
    for (uint32_t k = 0; k < per_byte; ++k) {
      const uint64_t col = x * per_byte + k;
      if (col >= P.in.width) break;
      byte |= (PngIndexFetch(P, table, row, col, c) & ((1u << bpp) - 1u)) << (8 - bpp * (k + 1));
    }
    return byte;
  }
  const uint32_t width = bpp / 8;
  const uint32_t xx = static_cast<uint32_t>(x);   // (a row has at most 2^31 - 1 bytes)
  const uint32_t col = xx / width, at = xx - col * width;
  return (PngIndexFetch(P, table, row, col, c) >> (8 * at)) & 255u;
}

// Thread `thread` of `threads` (at least 16) writes its share of the output; `table` is its workgroup's.
ZMX_PNGC_HD inline void PngIndexConvRun(const PngIndexConvParams& P, const uint32_t* table, uint64_t thread, uint64_t threads) {
  const uint64_t total = P.in.height * P.rowbytes;
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(P.out) & 15)) & 15;
  if (head > total) head = total;
  const uint64_t nvec = (total - head) / 16;
  PngIndexCache cache;
  cache.have = false;
  uint64_t row, x;
  if (thread < head) {
    PngConvAt(thread, P.rowbytes, &row, &x);
    P.out[thread] = static_cast<unsigned char>(PngIndexConvByte(P, table, row, x, &cache));
  }
  for (uint64_t v = thread; v < nvec; v += threads) {
    PngConvAt(head + 16 * v, P.rowbytes, &row, &x);
    PngColorVec vec = {{0, 0, 0, 0}};
    for (int j = 0; j < 16; ++j) {
      vec.w[j >> 2] |= PngIndexConvByte(P, table, row, x, &cache) << (8 * (j & 3));
      if (++x == P.rowbytes) { x = 0; ++row; }
    }
    __builtin_memcpy(__builtin_assume_aligned(P.out + head + 16 * v, 16), &vec, 16);
  }
  const uint64_t done = head + 16 * nvec, back = threads - 1 - thread;
  if (back < total - done) {
    PngConvAt(done + back, P.rowbytes, &row, &x);
    P.out[done + back] = static_cast<unsigned char>(PngIndexConvByte(P, table, row, x, &cache));
  }
}

}  // namespace zamd

#if defined(ZMX_PNG_INDEX_KERNELS)

__global__ __launch_bounds__(256) void k_png_index_use(zamd::PngIndexImage I, uint32_t* first) {
  using namespace zamd;
  __shared__ uint32_t table[kPngIndexValues];
  PngIndexGroupBegin(table, threadIdx.x);
  __syncthreads();
  PngIndexUseRun(I, table, static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, static_cast<uint64_t>(gridDim.x) * blockDim.x);
  __syncthreads();
  PngIndexGroupFlush(table, first, threadIdx.x);
}

__global__ __launch_bounds__(256) void k_png_index_convert(zamd::PngIndexConvParams P) {
  using namespace zamd;
  __shared__ uint32_t table[kPngIndexValues];
  for (uint32_t s = threadIdx.x; s < kPngIndexValues; s += blockDim.x) table[s] = P.table[s];
  __syncthreads();
  PngIndexConvRun(P, table, static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, static_cast<uint64_t>(gridDim.x) * blockDim.x);
}

#endif  // ZMX_PNG_INDEX_KERNELS

#endif  // ZMX_PNG_INDEX_H_
