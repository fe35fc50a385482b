// zmx_png_filter_rows_device: the filtered scanlines of a PNG, made on the device from an image in device memory.
// Row r of the output is the filter type types[r] followed by the row's `linebytes` bytes filtered that way
// (lodepng.cpp:5379-5421 filterScanline): what LodePNG hands to its deflate, what zmx_png_encode_device hands to
// zmx_compress_device (host/png_encode.cc).
//   k_png_rows   threads stride over the 16-byte aligned vectors of the DESTINATION, consecutive lanes consecutive vectors;
//                the bytes in front of the first boundary and behind the last one are written singly.  A vector that
//                lies inside one row's bytes — all but two of a long row's — takes its sixteen source bytes, the sixteen
//                to their left and the same two windows of the row above as aligned words (one 16-byte load where the
//                window is aligned, else five words funnel-shifted into four as in zmx_gather.h) and filters four bytes
//                at a time: the differences and Average's floor of the half sum in byte lanes of a word, Paeth byte by
//                byte.  A vector that holds a filter type byte or spans rows (every vector of rows shorter than 16
//                bytes) is made byte by byte.
// The destination rows start at r * (linebytes + 1): they are not co-aligned with the source, whatever its alignment.
// A row of the image comes from HBM once: the threads that read it as "the row above" run beside or behind those that
// filter it (the two are linebytes + 1 bytes of output apart) and find it in the L2.
// Every byte of out[0, height * (linebytes + 1)) is written exactly once, none outside; nothing is read but the aligned
// 4-byte words that hold a byte of the image, and the type bytes.  Plain loads and stores; a type byte above 4 is
// reported through *bad_row (the smallest such row) by the thread that writes that byte, and its row is copied
// unfiltered.  The launch is at most kPngRowsMaxBlocks workgroups whatever the image.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/png_rows_print.cc) runs the very code of
// the kernel, threads one after the other.  This header compiles without HIP; the kernel is there for the device layer
// only (ZMX_PNG_ROWS_KERNELS).
#ifndef ZMX_PNG_ROWS_H_
#define ZMX_PNG_ROWS_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMX_PNGR_HD __host__ __device__
#else
#define ZMX_PNGR_HD
#endif

// A CPU program that wants to see every address of the image the rules read defines ZMX_PNGR_SEE_LOAD(p, n) before it
// includes this header; the device layer's build leaves it empty.
#ifndef ZMX_PNGR_SEE_LOAD
#define ZMX_PNGR_SEE_LOAD(p, n)
#endif

namespace zamd {

constexpr uint32_t kPngRowsThreads = 256;      // a workgroup: four waves
constexpr uint32_t kPngRowsMaxBlocks = 2048;   // the grid's cap: 8 workgroups for each of 256 CUs
constexpr uint32_t kPngRowsNoBadRow = 0xffffffffu;

struct PngRowsParams {
  const unsigned char* image;   // height rows of linebytes bytes
  const unsigned char* types;   // [height]
  unsigned char* out;           // height * (linebytes + 1) bytes, any alignment
  uint64_t linebytes, height;
  uint32_t bytewidth;           // 1 .. 8: the distance to the left neighbour
  uint32_t* bad_row;            // kPngRowsNoBadRow before the launch; afterwards the first row whose type is above 4
};

struct alignas(16) PngRowsVec { uint32_t w[4]; };

// the workgroups of a launch over `total` bytes of output
ZMX_PNGR_HD inline uint32_t PngRowsGrid(uint64_t total) {
  const uint64_t blocks = (total / 16 + kPngRowsThreads - 1) / kPngRowsThreads;
  return static_cast<uint32_t>(blocks == 0 ? 1 : blocks < kPngRowsMaxBlocks ? blocks : kPngRowsMaxBlocks);
}

// lodepng.cpp:3974-3981 paethPredictor: a, then b, then c on ties
ZMX_PNGR_HD inline int PngRowsPaeth(int a, int b, int c) {
  int pa = b - c, pb = a - c, pc = pa + pb;
  pa = pa < 0 ? -pa : pa;
  pb = pb < 0 ? -pb : pb;
  pc = pc < 0 ? -pc : pc;
  if (pb < pa) { a = b; pa = pb; }
  return pc < pa ? c : a;
}

// One filtered byte: s the byte, a its left neighbour, b the one above, c the one above a (0 where there is none).
ZMX_PNGR_HD inline uint32_t PngRowsFilter(uint32_t type, int s, int a, int b, int c) {
  switch (type) {
    case 1: return static_cast<uint32_t>(s - a) & 255u;
    case 2: return static_cast<uint32_t>(s - b) & 255u;
    case 3: return static_cast<uint32_t>(s - ((a + b) >> 1)) & 255u;   // the 9-bit sum halved
    case 4: return static_cast<uint32_t>(s - PngRowsPaeth(a, b, c)) & 255u;
    default: return static_cast<uint32_t>(s);
  }
}

// Byte `o` of the output: *row its scanline, *x its place in it — 0 the filter type byte, x >= 1 byte x - 1 of the row.
ZMX_PNGR_HD inline void PngRowsAt(uint64_t o, uint64_t linebytes, uint64_t* row, uint64_t* x) {
  const uint64_t stride = linebytes + 1;
  // (a 32-bit division where the numbers allow it: the 64-bit one is a long routine on the device)
  if ((o >> 32) == 0 && (stride >> 32) == 0) *row = static_cast<uint32_t>(o) / static_cast<uint32_t>(stride);
  else *row = o / stride;
  *x = o - *row * stride;
}

ZMX_PNGR_HD inline void PngRowsReport(const PngRowsParams& P, uint64_t row) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(P.bad_row, static_cast<uint32_t>(row));
#else
  if (static_cast<uint32_t>(row) < *P.bad_row) *P.bad_row = static_cast<uint32_t>(row);
#endif
}

ZMX_PNGR_HD inline int PngRowsImageByte(const unsigned char* p) {
  ZMX_PNGR_SEE_LOAD(p, 1);
  return *p;
}

// The output byte at (row, x), whatever it is.
ZMX_PNGR_HD inline uint32_t PngRowsByteAt(const PngRowsParams& P, uint64_t row, uint64_t x) {
  uint32_t type = P.types[row];
  if (x == 0) {
    if (type > 4) PngRowsReport(P, row);
    return type;
  }
  if (type > 4) type = 0;
  const uint64_t i = x - 1, L = P.linebytes, bw = P.bytewidth;
  const unsigned char* cur = P.image + row * L + i;
  const int s = PngRowsImageByte(cur);
  const bool left = i >= bw && type != 0 && type != 2, up = row != 0 && type >= 2;
  const int a = left ? PngRowsImageByte(cur - bw) : 0;
  const int b = up ? PngRowsImageByte(cur - L) : 0;
  const int c = left && up && type == 4 ? PngRowsImageByte(cur - L - bw) : 0;
  return PngRowsFilter(type, s, a, b, c);
}

// the aligned word at p (p % 4 == 0)
ZMX_PNGR_HD inline uint32_t PngRowsLoadWord(const unsigned char* p) {
  uint32_t v;
  ZMX_PNGR_SEE_LOAD(p, 4);
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}

// The sixteen bytes at `at` (any alignment; the last of them a byte of the image) as four words.  Words that end at or
// before `lo`, the image's first byte, are not read and count as zero: the window to the left of a row's first bytes
// begins in front of the image in rows 0 and 1.
ZMX_PNGR_HD inline PngRowsVec PngRowsWindow(uintptr_t at, uintptr_t lo) {
  PngRowsVec out;
  const uint32_t off = static_cast<uint32_t>(at & 3);
  if ((at & 15) == 0 && at >= lo) {
    const unsigned char* s = reinterpret_cast<const unsigned char*>(at);
    ZMX_PNGR_SEE_LOAD(s, 16);
    __builtin_memcpy(&out, __builtin_assume_aligned(s, 16), 16);
    return out;
  }
  const uintptr_t w = at - off;
  if (off == 0) {
    for (int k = 0; k < 4; ++k) {
      out.w[k] = w + 4 * k + 4 > lo ? PngRowsLoadWord(reinterpret_cast<const unsigned char*>(w + 4 * k)) : 0u;
    }
    return out;
  }
  // words 0 .. 4 from at - off: the fifth holds bytes 16 - off .. 15 of the sixteen
  const uint32_t sh = 8 * off;   // 8, 16 or 24
  uint32_t lo_word = w + 4 > lo ? PngRowsLoadWord(reinterpret_cast<const unsigned char*>(w)) : 0u;
  for (int k = 0; k < 4; ++k) {
    const uintptr_t next = w + 4 * (k + 1);
    const uint32_t hi_word = next + 4 > lo ? PngRowsLoadWord(reinterpret_cast<const unsigned char*>(next)) : 0u;
    out.w[k] = (lo_word >> sh) | (hi_word << (32 - sh));
    lo_word = hi_word;
  }
  return out;
}

// the first `n` bytes of the sixteen become zero (n >= 16: all)
ZMX_PNGR_HD inline void PngRowsZeroFront(PngRowsVec* v, uint64_t n) {
  for (int k = 0; k < 4; ++k) {
    const uint64_t done = 4u * static_cast<uint32_t>(k);
    const uint64_t nb = n <= done ? 0 : n - done;
    if (nb >= 4) v->w[k] = 0;
    else if (nb != 0) v->w[k] &= 0xffffffffu << (8 * static_cast<uint32_t>(nb));
  }
}

// x - y in each of the four byte lanes
ZMX_PNGR_HD inline uint32_t PngRowsSub4(uint32_t x, uint32_t y) {
  return ((x | 0x80808080u) - (y & 0x7f7f7f7fu)) ^ ((x ^ ~y) & 0x80808080u);
}
// (x + y) >> 1 of the 9-bit sum in each byte lane
ZMX_PNGR_HD inline uint32_t PngRowsHalfSum4(uint32_t x, uint32_t y) {
  return (x & y) + (((x ^ y) & 0xfefefefeu) >> 1);
}

// Sixteen output bytes that all lie in row `row`, from byte i of it on (i + 16 <= linebytes).
ZMX_PNGR_HD inline PngRowsVec PngRowsInRow(const PngRowsParams& P, uint64_t row, uint64_t i) {
  uint32_t type = P.types[row];
  if (type > 4) type = 0;   // (reported by the thread that writes the type byte)
  const uint64_t L = P.linebytes, bw = P.bytewidth;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(P.image);
  const uintptr_t at = lo + row * L + i;
  const PngRowsVec S = PngRowsWindow(at, lo);
  if (type == 0) return S;
  const bool up = row != 0;
  PngRowsVec A = {{0, 0, 0, 0}}, B = {{0, 0, 0, 0}}, C = {{0, 0, 0, 0}}, out;
  if (type != 2) {
    A = PngRowsWindow(at - bw, lo);
    if (i < bw) PngRowsZeroFront(&A, bw - i);
  }
  if (up && type != 1) B = PngRowsWindow(at - L, lo);
  if (up && type == 4) {
    C = PngRowsWindow(at - L - bw, lo);
    if (i < bw) PngRowsZeroFront(&C, bw - i);
  }
  for (int k = 0; k < 4; ++k) {
    if (type == 1) out.w[k] = PngRowsSub4(S.w[k], A.w[k]);
    else if (type == 2) out.w[k] = PngRowsSub4(S.w[k], B.w[k]);
    else if (type == 3) out.w[k] = PngRowsSub4(S.w[k], PngRowsHalfSum4(A.w[k], B.w[k]));
    else {
      uint32_t p = 0;
      for (int j = 0; j < 4; ++j) {
        const int a = static_cast<int>((A.w[k] >> (8 * j)) & 255u), b = static_cast<int>((B.w[k] >> (8 * j)) & 255u);
        const int c = static_cast<int>((C.w[k] >> (8 * j)) & 255u);
        p |= static_cast<uint32_t>(PngRowsPaeth(a, b, c)) << (8 * j);
      }
      out.w[k] = PngRowsSub4(S.w[k], p);
    }
  }
  return out;
}

// The sixteen output bytes from byte `o` on (o + 16 <= the total).
ZMX_PNGR_HD inline PngRowsVec PngRowsVector(const PngRowsParams& P, uint64_t o) {
  uint64_t row, x;
  PngRowsAt(o, P.linebytes, &row, &x);
  if (x >= 1 && x - 1 + 16 <= P.linebytes) return PngRowsInRow(P, row, x - 1);
  PngRowsVec out = {{0, 0, 0, 0}};
  for (int j = 0; j < 16; ++j) {
    out.w[j >> 2] |= PngRowsByteAt(P, row, x) << (8 * (j & 3));
    if (++x > P.linebytes) { x = 0; ++row; }
  }
  return out;
}

// Thread `thread` of `threads` (at least 16) writes its share of the output.
ZMX_PNGR_HD inline void PngRowsRun(const PngRowsParams& P, uint64_t thread, uint64_t threads) {
  const uint64_t total = P.height * (P.linebytes + 1);
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(P.out) & 15)) & 15;   // bytes up to the destination's 16-byte boundary
  if (head > total) head = total;
  const uint64_t nvec = (total - head) / 16;
  uint64_t row, x;
  if (thread < head) {
    PngRowsAt(thread, P.linebytes, &row, &x);
    P.out[thread] = static_cast<unsigned char>(PngRowsByteAt(P, row, x));
  }
  for (uint64_t v = thread; v < nvec; v += threads) {
    const PngRowsVec vec = PngRowsVector(P, head + 16 * v);
    __builtin_memcpy(__builtin_assume_aligned(P.out + head + 16 * v, 16), &vec, 16);
  }
  const uint64_t done = head + 16 * nvec;
  // (the tail on the last threads: the first ones have the head)
  const uint64_t back = threads - 1 - thread;
  if (back < total - done) {
    PngRowsAt(done + back, P.linebytes, &row, &x);
    P.out[done + back] = static_cast<unsigned char>(PngRowsByteAt(P, row, x));
  }
}

}  // namespace zamd

#if defined(ZMX_PNG_ROWS_KERNELS)

__global__ __launch_bounds__(256) void k_png_rows(zamd::PngRowsParams P) {
  zamd::PngRowsRun(P, static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, static_cast<uint64_t>(gridDim.x) * blockDim.x);
}

#endif  // ZMX_PNG_ROWS_KERNELS

#endif  // ZMX_PNG_ROWS_H_
