// zmx_gather_device: n ranges of device memory put end to end in one launch (the inputs of zmx_compress_device_batch,
// host/batch.cc, become the one resident concatenation the batch path works on).
//   k_gather   workgroups stride over fixed 16 KiB tiles of the DESTINATION; a workgroup finds the piece under its
//              tile's first byte by binary search in the prefix offsets and walks the pieces that cross the tile.  A
//              span — one piece within one tile — is copied as bytes up to the destination's 16-byte boundary, 16-byte
//              destination-aligned stores, a byte tail.  The source words of a store are read aligned; where source and
//              destination are not congruent mod 4 two neighbouring words are funnel-shifted into one: the plain
//              expression (lo >> sh) | (hi << (32 - sh)) with sh = 8, 16 or 24, which the compiler turns into
//              v_alignbit_b32.
// Writes touch exactly the span, reads nothing beyond the aligned 4-byte words that hold a byte of it.  Plain loads and
// stores only; the launch is at most kGatherMaxBlocks workgroups whatever n and the total.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/gather_print.cc) runs the very code of
// the kernel, lanes one after the other.  This header compiles without HIP; the kernel is there for the device layer
// only (ZMX_GATHER_KERNELS).
#ifndef ZMX_GATHER_H_
#define ZMX_GATHER_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMX_GATHER_HD __host__ __device__
#else
#define ZMX_GATHER_HD
#endif

// A CPU program that wants to see every address the rules read defines ZMX_GATHER_SEE_LOAD(p, n) before it includes
// this header (tests/hostlib/gather_print.cc holds every read against the words of its piece, on both sides); the
// device layer's build leaves it empty.
#ifndef ZMX_GATHER_SEE_LOAD
#define ZMX_GATHER_SEE_LOAD(p, n)
#endif

namespace zamd {

constexpr uint64_t kGatherTile = 16384;       // bytes of the destination a workgroup takes at a time
constexpr uint32_t kGatherThreads = 256;      // a workgroup: four waves
constexpr uint32_t kGatherWave = 64;
constexpr uint32_t kGatherMaxBlocks = 2048;   // the grid's cap: 8 workgroups for each of 256 CUs
constexpr uint64_t kGatherWaveSpan = 1024;    // a span below this many bytes is one wave's (64 lanes x 16 bytes)

struct alignas(16) GatherVec { uint32_t w[4]; };

// the aligned word at p (p % 4 == 0)
ZMX_GATHER_HD inline uint32_t GatherLoadWord(const unsigned char* p) {
  uint32_t v;
  ZMX_GATHER_SEE_LOAD(p, 4);
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}

// The piece that byte `pos` of the destination comes from: start[0] = 0 <= pos < start[n], the offsets never decrease;
// the piece found holds the byte (empty pieces that start at pos are passed over).
ZMX_GATHER_HD inline uint64_t GatherPieceAt(const uint64_t* start, uint64_t n, uint64_t pos) {
  uint64_t lo = 0, hi = n;   // start[lo] <= pos < start[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (start[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// Lane `lane` of `lanes` (at least 16) copies its share of src[0, len) to dst[0, len).
ZMX_GATHER_HD inline void GatherSpan(unsigned char* dst, const unsigned char* src, uint64_t len, uint32_t lane, uint32_t lanes) {
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;   // bytes up to the destination's 16-byte boundary
  if (head > len) head = len;
  if (lane < head) {
    ZMX_GATHER_SEE_LOAD(src + lane, 1);
    dst[lane] = src[lane];
  }
  const uint64_t nvec = (len - head) / 16;
  const unsigned char* s0 = src + head;
  const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(s0) & 3);   // the source within its word
  const bool vec_src = (reinterpret_cast<uintptr_t>(s0) & 15) == 0;
  for (uint64_t v = lane; v < nvec; v += lanes) {
    const unsigned char* s = s0 + 16 * v;
    GatherVec out;
    if (vec_src) {
      ZMX_GATHER_SEE_LOAD(s, 16);
      __builtin_memcpy(&out, __builtin_assume_aligned(s, 16), 16);
    } else if (off == 0) {
      for (int k = 0; k < 4; ++k) out.w[k] = GatherLoadWord(s + 4 * k);
    } else {
      // words 0 .. 4 from s - off: the fifth holds bytes 16 - off .. 15 of the sixteen
      const unsigned char* w = s - off;
      const uint32_t sh = 8 * off;   // 8, 16 or 24
      uint32_t lo = GatherLoadWord(w);
      for (int k = 0; k < 4; ++k) {
        const uint32_t hi = GatherLoadWord(w + 4 * (k + 1));
        out.w[k] = (lo >> sh) | (hi << (32 - sh));
        lo = hi;
      }
    }
    __builtin_memcpy(__builtin_assume_aligned(dst + head + 16 * v, 16), &out, 16);
  }
  const uint64_t done = head + 16 * nvec;
  // (the tail on the last lanes: the first ones have the head)
  const uint32_t back = lanes - 1 - lane;
  if (back < len - done) {
    ZMX_GATHER_SEE_LOAD(src + done + back, 1);
    dst[done + back] = src[done + back];
  }
}

struct GatherTable {
  const unsigned char* const* src;   // [n]; null: the piece is not this launch's (it lies on another device)
  const uint64_t* start;             // [n + 1]: where piece i begins in the destination; start[n] = the total
  unsigned char* dst;
  uint64_t n;
};

// Thread `thread` of a workgroup of `threads` (a multiple of kGatherWave) copies its share of tile `tile` of the
// destination: the spans of at least kGatherWaveSpan bytes with the whole workgroup, the shorter ones a wave each in turn.
ZMX_GATHER_HD inline void GatherTile(const GatherTable& T, uint64_t tile, uint32_t thread, uint32_t threads) {
  const uint64_t total = T.start[T.n];
  const uint64_t lo = tile * kGatherTile;
  const uint64_t hi = total - lo < kGatherTile ? total : lo + kGatherTile;
  const uint32_t wave = thread / kGatherWave, waves = threads / kGatherWave, lane = thread % kGatherWave;
  uint32_t turn = 0;
  uint64_t pos = lo;
  for (uint64_t i = GatherPieceAt(T.start, T.n, lo); pos < hi; ++i) {
    const uint64_t s = T.start[i], e = T.start[i + 1];
    if (e <= pos) continue;   // an empty piece
    const uint64_t end = e < hi ? e : hi;
    const unsigned char* src = T.src[i];
    if (src != nullptr) {
      if (end - pos >= kGatherWaveSpan) {
        GatherSpan(T.dst + pos, src + (pos - s), end - pos, thread, threads);
      } else {
        if (turn == wave) GatherSpan(T.dst + pos, src + (pos - s), end - pos, lane, kGatherWave);
        turn = turn + 1 == waves ? 0 : turn + 1;
      }
    }
    pos = end;
  }
}

}  // namespace zamd

#if defined(ZMX_GATHER_KERNELS)

__global__ __launch_bounds__(256) void k_gather(zamd::GatherTable T, uint64_t ntiles) {
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) zamd::GatherTile(T, tile, threadIdx.x, blockDim.x);
}

#endif  // ZMX_GATHER_KERNELS

#endif  // ZMX_GATHER_H_
