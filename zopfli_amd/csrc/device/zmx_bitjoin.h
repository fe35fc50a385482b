// zmx_bitjoin_device: n bit strings of device memory joined into one bit string in one launch — the deflate stream of
// zmx_compress_device_to_device (host/device_output.cc) put together where its pieces lie: headers and trees from a small
// uploaded buffer, the symbols' bits from the bit writer's buffers, stored blocks' bytes from the input.
// Bit k of a string at p is (p[k / 8] >> (k % 8)) & 1, deflate's order.  A piece is bits [src_bit, src_bit + nbits) of
// the string at src, and goes to bits [dst_bit, dst_bit + nbits) of the destination; the pieces are sorted by dst_bit
// and none begins before the one in front of it ends.  Bits of the destination that no piece covers are 0.
//   k_bitjoin  workgroups stride over fixed 16 KiB tiles of the DESTINATION (tiles of 16-byte vectors, counted from the
//              16-byte boundary at or below dst); a workgroup finds the piece under its tile's first bit by binary
//              search in dst_bit and walks the pieces that cross the tile.  The vectors that lie wholly inside one
//              piece are made by a lane each from five aligned source words — four where source and destination are
//              congruent mod 32 bits — with the plain funnel shift (lo >> sh) | (hi << (32 - sh)), sh = 1 .. 31, and
//              stored as 16 bytes.  Every other vector — one that holds an edge of a piece, a gap, several tiny pieces,
//              an end of the destination — is made word by word by one general rule, BitjoinWord, which ORs together
//              whatever pieces touch the word; it is stored as 16 bytes where it lies inside the destination and byte
//              by byte where it does not.
// Every byte of dst[0, (total_bits + 7) / 8) is written exactly once, whole, and none beyond; nothing is read but the
// aligned 4-byte words that hold a bit of a piece.  Plain loads and stores only: no atomics, no pre-zeroed destination.
// The launch is at most kBitjoinMaxBlocks workgroups whatever n and the total.
// zmx_bitjoin_many_device / k_bitjoin_many (below): the same join for many destinations in one launch.
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/bitjoin_print.cc, bitjoin_many_print.cc)
// runs the very code of the kernel, lanes one after the other.  This header compiles without HIP; the kernel is there for the device layer
// only (ZMX_BITJOIN_KERNELS).
#ifndef ZMX_BITJOIN_H_
#define ZMX_BITJOIN_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMX_BITJOIN_HD __host__ __device__
#else
#define ZMX_BITJOIN_HD
#endif

// A CPU program that wants to see every address the rules read defines ZMX_BITJOIN_SEE_LOAD(p, n) before it includes
// this header (tests/hostlib/bitjoin_print.cc holds every read against the words of its piece); the device layer's
// build leaves it empty.
#ifndef ZMX_BITJOIN_SEE_LOAD
#define ZMX_BITJOIN_SEE_LOAD(p, n)
#endif

namespace zamd {

constexpr uint64_t kBitjoinTile = 16384;       // bytes of the destination a workgroup takes at a time
constexpr uint64_t kBitjoinTileVecs = kBitjoinTile / 16;
constexpr uint32_t kBitjoinThreads = 256;      // a workgroup: four waves
constexpr uint32_t kBitjoinWave = 64;
constexpr uint32_t kBitjoinMaxBlocks = 2048;   // the grid's cap: 8 workgroups for each of 256 CUs
constexpr uint64_t kBitjoinMaxBits = 1ull << 60;   // of a piece's src_bit, nbits, dst_bit and of total_bits: no sum of two overflows

// (the layout of zmx_bit_piece, include/zopfli_amd.h)
struct BitPiece {
  const void* src;
  uint64_t src_bit, nbits, dst_bit;
};

struct alignas(16) BitjoinVec { uint32_t w[4]; };

struct BitjoinTable {
  const BitPiece* piece;   // [n]
  uint64_t n;
  unsigned char* dst;
  uint64_t total_bits;
};

// the aligned word at address a (a % 4 == 0)
ZMX_BITJOIN_HD inline uint32_t BitjoinLoadWord(uintptr_t a) {
  uint32_t v;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(a);
  ZMX_BITJOIN_SEE_LOAD(p, 4);
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}

// The last piece that begins at or before bit `bit` of the destination (0 when none does): no piece in front of it
// reaches `bit`, so whatever covers bits from `bit` on is this piece or one behind it.
ZMX_BITJOIN_HD inline uint64_t BitjoinPieceAt(const BitPiece* piece, uint64_t n, uint64_t bit) {
  uint64_t lo = 0, hi = n;   // piece[lo].dst_bit <= bit < piece[hi].dst_bit (lo = 0: or none)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (piece[mid].dst_bit <= bit) lo = mid; else hi = mid;
  }
  return lo;
}

// Where bit s of the string at src lies: the aligned word's address and the bit within it.
ZMX_BITJOIN_HD inline uintptr_t BitjoinSourceWord(const void* src, uint64_t s, uint32_t* sh) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(src) + static_cast<uintptr_t>(s >> 3);
  *sh = static_cast<uint32_t>(s & 7) + 8 * static_cast<uint32_t>(at & 3);
  return at & ~static_cast<uintptr_t>(3);
}

// The general rule: bits [wb, wb + 32) of the destination (wb may be negative, and the word may reach beyond total_bits:
// the words over the destination's ends), every piece that touches them ORed in, everything else 0.
ZMX_BITJOIN_HD inline uint32_t BitjoinWord(const BitjoinTable& T, int64_t wb) {
  const int64_t we = wb + 32;
  if (we <= 0 || T.n == 0) return 0;
  uint32_t out = 0;
  for (uint64_t j = BitjoinPieceAt(T.piece, T.n, wb < 0 ? 0 : static_cast<uint64_t>(wb)); j < T.n; ++j) {
    const BitPiece q = T.piece[j];
    if (static_cast<int64_t>(q.dst_bit) >= we) break;
    const int64_t db = static_cast<int64_t>(q.dst_bit), de = db + static_cast<int64_t>(q.nbits);
    const int64_t lo = db > wb ? db : wb, hi = de < we ? de : we;
    if (hi <= lo) continue;     // an empty piece, or one that ends in front of the word
    const uint32_t cnt = static_cast<uint32_t>(hi - lo);   // 1 .. 32
    uint32_t sh;
    const uintptr_t w = BitjoinSourceWord(q.src, q.src_bit + static_cast<uint64_t>(lo - db), &sh);
    uint32_t v = BitjoinLoadWord(w) >> sh;
    if (sh + cnt > 32) v |= BitjoinLoadWord(w + 4) << (32 - sh);   // (sh != 0 here)
    if (cnt < 32) v &= (1u << cnt) - 1u;
    out |= v << static_cast<uint32_t>(lo - wb);
  }
  return out;
}

// Vector g of the destination — the 16 bytes at (dst rounded down to 16) + 16 g — by the general rule: stored whole where
// it lies inside dst[0, nbytes), byte by byte where it hangs over an end.
ZMX_BITJOIN_HD inline void BitjoinEdgeVec(const BitjoinTable& T, uint64_t g) {
  const uint64_t lead = reinterpret_cast<uintptr_t>(T.dst) & 15;
  const uint64_t nbytes = (T.total_bits + 7) / 8;
  const int64_t first = static_cast<int64_t>(16 * g) - static_cast<int64_t>(lead);   // the vector's first byte, in dst
  BitjoinVec out;
  for (int k = 0; k < 4; ++k) out.w[k] = BitjoinWord(T, 8 * (first + 4 * k));
  if (first >= 0 && static_cast<uint64_t>(first) + 16 <= nbytes) {
    __builtin_memcpy(__builtin_assume_aligned(T.dst + first, 16), &out, 16);
    return;
  }
  for (int k = 0; k < 16; ++k) {
    const int64_t at = first + k;
    if (at >= 0 && static_cast<uint64_t>(at) < nbytes) T.dst[at] = static_cast<unsigned char>(out.w[k / 4] >> (8 * (k % 4)));
  }
}

// Vector g, which lies wholly inside piece q: sixteen destination-aligned bytes from five aligned source words.
ZMX_BITJOIN_HD inline void BitjoinInnerVec(const BitjoinTable& T, const BitPiece& q, uint64_t g) {
  const uint64_t lead = reinterpret_cast<uintptr_t>(T.dst) & 15;
  const uint64_t first = 16 * g - lead;            // (g >= 1 where lead != 0: vector 0 hangs over the front)
  uint32_t sh;
  const uintptr_t w = BitjoinSourceWord(q.src, q.src_bit + (8 * first - q.dst_bit), &sh);
  BitjoinVec out;
  if (sh == 0) {
    if ((w & 15) == 0) {
      const unsigned char* p = reinterpret_cast<const unsigned char*>(w);
      ZMX_BITJOIN_SEE_LOAD(p, 16);
      __builtin_memcpy(&out, __builtin_assume_aligned(p, 16), 16);
    } else {
      for (int k = 0; k < 4; ++k) out.w[k] = BitjoinLoadWord(w + 4 * k);
    }
  } else {
    // words 0 .. 4 from w: the fifth holds the last sh bits of the 128
    uint32_t lo = BitjoinLoadWord(w);
    for (int k = 0; k < 4; ++k) {
      const uint32_t hi = BitjoinLoadWord(w + 4 * (k + 1));
      out.w[k] = (lo >> sh) | (hi << (32 - sh));
      lo = hi;
    }
  }
  __builtin_memcpy(__builtin_assume_aligned(T.dst + first, 16), &out, 16);
}

// The vectors of the destination: those that hold a byte of dst[0, (total_bits + 7) / 8).
ZMX_BITJOIN_HD inline uint64_t BitjoinVectors(const unsigned char* dst, uint64_t total_bits) {
  const uint64_t lead = reinterpret_cast<uintptr_t>(dst) & 15;
  return total_bits == 0 ? 0 : (lead + (total_bits + 7) / 8 + 15) / 16;
}

// Thread `thread` of a workgroup of `threads` (a multiple of kBitjoinWave) makes its share of tile `tile` of the
// destination.  The tile's vectors fall into runs — the vectors inside one piece, the vectors between two such runs —
// and a run of at least a wave's 64 vectors is the whole workgroup's, a shorter one a wave's, the waves taking turns.
ZMX_BITJOIN_HD inline void BitjoinTile(const BitjoinTable& T, uint64_t tile, uint32_t thread, uint32_t threads) {
  const uint64_t lead8 = 8 * (reinterpret_cast<uintptr_t>(T.dst) & 15);
  const uint64_t nvec = BitjoinVectors(T.dst, T.total_bits);
  const uint64_t g0 = tile * kBitjoinTileVecs;
  const uint64_t g1 = nvec - g0 < kBitjoinTileVecs ? nvec : g0 + kBitjoinTileVecs;
  const uint32_t wave = thread / kBitjoinWave, waves = threads / kBitjoinWave, lane = thread % kBitjoinWave;
  uint32_t turn = 0;
  // run [a, b) of the tile: `inner` = the vectors of piece q, else by the general rule
  const auto run = [&](uint64_t a, uint64_t b, const BitPiece* q) {
    if (a >= b) return;
    uint64_t first = thread, step = threads;
    if (b - a < kBitjoinWave) {
      const bool mine = turn == wave;
      turn = turn + 1 == waves ? 0 : turn + 1;
      if (!mine) return;
      first = lane;
      step = kBitjoinWave;
    }
    for (uint64_t g = a + first; g < b; g += step) {
      if (q) BitjoinInnerVec(T, *q, g); else BitjoinEdgeVec(T, g);
    }
  };
  uint64_t cur = g0;
  if (T.n != 0) {
    const uint64_t bit0 = 128 * g0 > lead8 ? 128 * g0 - lead8 : 0;   // the tile's first bit of the destination
    for (uint64_t i = BitjoinPieceAt(T.piece, T.n, bit0); i < T.n && cur < g1; ++i) {
      const BitPiece q = T.piece[i];
      if (q.dst_bit + lead8 >= 128 * g1) break;     // it begins behind the tile, and so do the others
      // vector g lies inside the piece: 128 g - lead8 >= dst_bit and 128 (g + 1) - lead8 <= dst_bit + nbits
      uint64_t a = (q.dst_bit + lead8 + 127) / 128, b = (q.dst_bit + q.nbits + lead8) / 128;
      if (a < cur) a = cur;
      if (b > g1) b = g1;
      if (a >= b) continue;
      run(cur, a, nullptr);
      run(a, b, &q);
      cur = b;
    }
  }
  run(cur, g1, nullptr);
}

// ---- zmx_bitjoin_many_device: many destinations in one launch (the streams of zmx_compress_device_batch_to_device).
// Destination d is a join of its own — pieces [first_piece, first_piece + npieces) of one shared table, their dst_bit
// counted from its own dst — and keeps the tiling of a single join: its tiles are counted from the 16-byte boundary at or
// below its own dst, BitjoinVectors of them.  The tiles of all destinations are numbered one after the other;
// tile_start[d] is the number of destination d's first tile (tile_start[ndst]: the number of tiles), made on the host.
// A workgroup strides over that global number, finds the destination by binary search and runs BitjoinTile on the
// local tile, so the launch is at most kBitjoinMaxBlocks workgroups whatever ndst, the piece count and the total.  Two
// destinations may be neighbours inside one 16-byte vector: each join stores only its own bytes of it (BitjoinEdgeVec's
// byte-by-byte path), so every byte of every destination is still written exactly once and none outside them.

// (the layout of zmx_bit_dest, include/zopfli_amd.h)
struct BitDest {
  unsigned char* dst;
  uint64_t total_bits, first_piece, npieces;
};

struct BitjoinManyTable {
  const BitPiece* piece;        // the pieces of all destinations, destination after destination
  const BitDest* dest;          // [ndst]
  const uint64_t* tile_start;   // [ndst + 1], ascending; equal neighbours: a destination of no tile
  uint64_t ndst;
};

// The tiles of a destination.
ZMX_BITJOIN_HD inline uint64_t BitjoinTiles(const unsigned char* dst, uint64_t total_bits) {
  return (BitjoinVectors(dst, total_bits) + kBitjoinTileVecs - 1) / kBitjoinTileVecs;
}

// The destination that global tile `tile` (< tile_start[ndst]) belongs to — the last d with tile_start[d] <= tile, which
// has tile_start[d + 1] > tile and so at least one tile: a destination of no tile is never found — and the tile's
// number within it.
ZMX_BITJOIN_HD inline uint64_t BitjoinDestOfTile(const uint64_t* tile_start, uint64_t ndst, uint64_t tile, uint64_t* local) {
  uint64_t lo = 0, hi = ndst;   // tile_start[lo] <= tile < tile_start[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (tile_start[mid] <= tile) lo = mid; else hi = mid;
  }
  *local = tile - tile_start[lo];
  return lo;
}

// Destination d as a join of its own.
ZMX_BITJOIN_HD inline BitjoinTable BitjoinDestTable(const BitjoinManyTable& M, uint64_t d) {
  const BitDest e = M.dest[d];
  BitjoinTable T;
  T.piece = M.piece + e.first_piece;
  T.n = e.npieces;
  T.dst = e.dst;
  T.total_bits = e.total_bits;
  return T;
}

// Thread `thread` of a workgroup of `threads` makes its share of global tile `tile`.
ZMX_BITJOIN_HD inline void BitjoinManyTile(const BitjoinManyTable& M, uint64_t tile, uint32_t thread, uint32_t threads) {
  uint64_t local = 0;
  const uint64_t d = BitjoinDestOfTile(M.tile_start, M.ndst, tile, &local);
  BitjoinTile(BitjoinDestTable(M, d), local, thread, threads);
}

}  // namespace zamd

#if defined(ZMX_BITJOIN_KERNELS)

__global__ __launch_bounds__(256) void k_bitjoin(zamd::BitjoinTable T, uint64_t ntiles) {
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) zamd::BitjoinTile(T, tile, threadIdx.x, blockDim.x);
}

__global__ __launch_bounds__(256) void k_bitjoin_many(zamd::BitjoinManyTable M, uint64_t ntiles) {
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) zamd::BitjoinManyTile(M, tile, threadIdx.x, blockDim.x);
}

#endif  // ZMX_BITJOIN_KERNELS

#endif  // ZMX_BITJOIN_H_
