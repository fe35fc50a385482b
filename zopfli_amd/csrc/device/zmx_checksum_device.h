// k_checksum_pieces, k_checksum_finish: CRC-32 and Adler-32 of n ranges of ARBITRARY device memory, finished on the device
// (zmx_checksum_device, and the seal of a PNG left in device memory: drv_checksum_device.h).  zmx_checksum.h's two kernels
// read the context's resident, 4-byte-aligned input and leave the pieces to the host; these take a range at any byte
// address, of any length, in any allocation of the context's device, and nothing comes down but the finished values —
// or nothing at all, where a value goes into a stream as four bytes.
//   geometry            k_checksum's: a workgroup per piece of 256 KiB, pieces and lanes counted from the range's END, 256
//                       lanes of 1 KiB; a short leftmost lane or piece counts as full.  Workgroup w takes the piece
//                       piece[w].index of range piece[w].range; a range of 0 bytes has no piece.
//   k_checksum_pieces   runs ck_piece (zmx_checksum.h) itself, on the range seen from the 4-byte-aligned address at or
//                       below its first byte: ck_piece aligns its word loads relative to `in`, so with an aligned `in` they
//                       are aligned absolutely.  A lane reads the up to three bytes in front of its first aligned word
//                       and behind its last byte by byte, so no byte outside the range is read — not even the rest of
//                       the word around a head or tail.  12 B out per piece, as k_checksum.
//   k_checksum_finish   a thread per range: the range's pieces combined from the left, crc = mulmod(crc, x^(8 * piece
//                       bytes)) ^ next and Adler's two sums, then what zamd::FinishCrc32 / FinishAdler32 apply on the host
//                       — the 0xffffffff register through x^(8 len), the final complement, Adler's 1 + ... and len + ...
//                       x^(8 len) comes up in the range's descriptor: the host knows every length before the launch.
//                       The value goes into values[range], or, where the descriptor has `seal`, to the four bytes
//                       there, most significant first — any byte address, plain byte stores.
// No workgroup waits for another: the finish is a second launch on the same stream.  The combine and finish rules are
// __host__ __device__ functions, so a CPU program (tests/hostlib/checksum_device_print.cc) runs the very code of the
// kernel.  This header compiles without HIP; the kernels are there for the device layer only
// (ZMX_CHECKSUM_DEVICE_KERNELS, behind zmx_checksum.h).
#ifndef ZMX_CHECKSUM_DEVICE_H_
#define ZMX_CHECKSUM_DEVICE_H_

#include <stddef.h>
#include <stdint.h>

#include "checksum.h"

#if defined(__HIPCC__)
#define ZMX_CKD_HD __host__ __device__
#else
#define ZMX_CKD_HD
#endif

namespace zamd {

constexpr uint32_t kChecksumDeviceCrc = 0, kChecksumDeviceAdler = 1;   // (ZMX_CRC32, ZMX_ADLER32)
constexpr uint32_t kChecksumFinishThreads = 256;

// A range as the two kernels see it.
struct ChecksumRange {
  const unsigned char* p;   // its first byte (any address; not read where len = 0)
  uint64_t len;
  uint64_t first_piece;     // its pieces in the pieces' array, the RIGHTMOST first (zamd::FinishCrc32's order)
  uint64_t npieces;         // (len + kChecksumPieceBytes - 1) / kChecksumPieceBytes
  unsigned char* seal;      // non-null: the value goes here as four bytes, most significant first, not to values[]
  uint32_t xlen;            // x^(8 len) mod P (CRC-32; unused for Adler-32)
  uint32_t pad;
};
// A workgroup's piece: number `index` of range `range`, counted from the range's end.
struct ChecksumPieceRef {
  uint32_t range, index;
};

ZMX_CKD_HD inline uint64_t ChecksumPieces(uint64_t len) { return (len + kChecksumPieceBytes - 1) / kChecksumPieceBytes; }

// a(x) * b(x) mod P, bit-reflected (zamd::Gf2MulMod, for both sides)
ZMX_CKD_HD inline uint32_t ChecksumMulMod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

// The CRC register, started from 0, after all pieces: pieces[0] is the rightmost; xpiece = x^(8 kChecksumPieceBytes).
ZMX_CKD_HD inline uint32_t ChecksumCombineCrc(const ChecksumPiece* pieces, uint64_t npieces, uint32_t xpiece) {
  uint32_t acc = 0;
  for (uint64_t i = npieces; i-- > 0;) acc = ChecksumMulMod(acc, xpiece) ^ pieces[i].crc0;
  return acc;
}
// ... made the CRC-32 of the `len` bytes: xlen = x^(8 len)
ZMX_CKD_HD inline uint32_t ChecksumFinishCrc(uint32_t crc0, uint32_t xlen) {
  return crc0 ^ ChecksumMulMod(0xffffffffu, xlen) ^ 0xffffffffu;
}
// Adler-32 of `len` bytes from their pieces (zamd::FinishAdler32's arithmetic)
ZMX_CKD_HD inline uint32_t ChecksumFinishAdler(const ChecksumPiece* pieces, uint64_t npieces, uint64_t len) {
  uint64_t sum = 0, wsum = 0;
  for (uint64_t i = npieces; i-- > 0;) {
    // the bytes so far move kChecksumPieceBytes further from the end
    wsum = (wsum + (kChecksumPieceBytes % kAdlerBase) * sum + pieces[i].wsum) % kAdlerBase;
    sum = (sum + pieces[i].sum) % kAdlerBase;
  }
  const uint32_t s1 = static_cast<uint32_t>((1 + sum) % kAdlerBase);
  const uint32_t s2 = static_cast<uint32_t>((len % kAdlerBase + wsum) % kAdlerBase);
  return (s2 << 16) | s1;
}
// the finished checksum of range R
ZMX_CKD_HD inline uint32_t ChecksumFinishRange(uint32_t kind, const ChecksumRange& R, const ChecksumPiece* all_pieces, uint32_t xpiece) {
  const ChecksumPiece* pieces = all_pieces + R.first_piece;
  if (kind == kChecksumDeviceAdler) return ChecksumFinishAdler(pieces, R.npieces, R.len);
  return ChecksumFinishCrc(ChecksumCombineCrc(pieces, R.npieces, xpiece), R.xlen);
}
// a value into a stream: four bytes, most significant first (PNG's chunk CRC, zlib's Adler-32)
ZMX_CKD_HD inline void ChecksumSeal(uint32_t v, unsigned char* dst) {
  for (int k = 0; k < 4; ++k) dst[k] = static_cast<unsigned char>(v >> (24 - 8 * k));
}
// The range seen from the aligned address at or below its first byte: *begin = 0 .. 3, the range is base[*begin, *begin + len).
ZMX_CKD_HD inline const unsigned char* ChecksumAlignedBase(const unsigned char* p, long long* begin) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(p);
  *begin = static_cast<long long>(at & 3u);
  return p - (at & 3u);
}

}  // namespace zamd

#ifdef ZMX_CHECKSUM_DEVICE_KERNELS

struct ChecksumDeviceParams {
  const zamd::ChecksumRange* ranges;
  const zamd::ChecksumPieceRef* piece;   // [pieces]
  u32* out;                              // [pieces][3], as k_checksum; range r's from 3 * ranges[r].first_piece
  u32* values;                           // [nranges]: the finished values of the ranges without `seal`
  unsigned long long nranges;
  u32 kind, xpiece;
  u32 xpow[8];                           // x^(8 * lane bytes * 2^k)
};

__global__ __launch_bounds__(256) void k_checksum_pieces(ChecksumDeviceParams P) {
  const zamd::ChecksumPieceRef ref = P.piece[blockIdx.x];
  const zamd::ChecksumRange R = P.ranges[ref.range];
  long long begin = 0;
  const u8* base = zamd::ChecksumAlignedBase(R.p, &begin);
  const long long end = begin + static_cast<long long>(R.len);
  ck_piece(base, begin, end - static_cast<long long>(ref.index) * static_cast<long long>(zamd::kChecksumPieceBytes), P.xpow,
           P.out + 3 * (R.first_piece + ref.index));
}

__global__ __launch_bounds__(256) void k_checksum_finish(ChecksumDeviceParams P) {
  const unsigned long long r = static_cast<unsigned long long>(blockIdx.x) * zamd::kChecksumFinishThreads + threadIdx.x;
  if (r >= P.nranges) return;
  const zamd::ChecksumRange R = P.ranges[r];
  const u32 v = zamd::ChecksumFinishRange(P.kind, R, reinterpret_cast<const zamd::ChecksumPiece*>(P.out), P.xpiece);
  if (R.seal) zamd::ChecksumSeal(v, R.seal);
  else P.values[r] = v;
}

#endif  // ZMX_CHECKSUM_DEVICE_KERNELS

#endif  // ZMX_CHECKSUM_DEVICE_H_
