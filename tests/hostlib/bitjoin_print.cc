// The rules of device/zmx_bitjoin.h on the CPU: the __host__ __device__ functions k_bitjoin is made of — the tile-to-piece
// search, the walk over a tile's pieces, the vectors inside a piece, the general per-word rule — run by a plain C++
// program, the 256 threads of a workgroup one after the other (tests/test_cpu_bitjoin_rules.py).
//   bitjoin_print TABLE ARENA OUT
// TABLE: the destination's address mod 16 and total_bits, then for every piece "offset in ARENA" (-1: a null pointer),
// src_bit, nbits and dst_bit, all decimal and separated by white space.  ARENA holds the sources' bytes; the offset mod
// 16 is the source pointer's address mod 16.  Every piece is copied into a heap block of its own that begins with the
// 16-byte line of the first aligned word holding one of its bits and ends with the last such word (a read beyond that is
// the sanitizer's to find), and every address the rules read (ZMX_BITJOIN_SEE_LOAD) is held against those words: a read
// in front of a piece's first word or behind its last is reported here, whatever the build.  The destination has 64
// guard bytes of 0xA5 on both sides and is itself filled with 0xA5: a byte the rules leave out shows.  The joined bytes
// are written to OUT and compared here, bit by bit, with the pieces; prints "ok PIECES BYTES TILES", or what differs
// (exit status 1).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace {
// [first, last) of every non-empty piece's aligned words, ascending (the blocks are apart), and the reads outside them
std::vector<std::pair<uintptr_t, uintptr_t>> g_words;
uint64_t g_stray_loads = 0;

void SeeLoad(const void* p, size_t n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = std::upper_bound(g_words.begin(), g_words.end(), std::make_pair(a, UINTPTR_MAX));
  if (it == g_words.begin() || a + n > (it - 1)->second) ++g_stray_loads;
}
}  // namespace
#define ZMX_BITJOIN_SEE_LOAD(p, n) SeeLoad(p, n)

#include "zmx_bitjoin.h"

namespace {
constexpr size_t kGuard = 64;

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}
unsigned Bit(const unsigned char* p, uint64_t k) { return (p[k / 8] >> (k % 8)) & 1u; }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: bitjoin_print TABLE ARENA OUT\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long long dst_mod = 0, total_bits = 0, b = 0, c = 0, d = 0;
  long long a = 0;
  if (std::fscanf(f, "%llu %llu", &dst_mod, &total_bits) != 2 || dst_mod > 15) return 2;
  std::vector<long long> arena_off;
  std::vector<zamd::BitPiece> piece;
  while (std::fscanf(f, "%lld %llu %llu %llu", &a, &b, &c, &d) == 4) {
    arena_off.push_back(a);
    piece.push_back({nullptr, b, c, d});
  }
  std::fclose(f);
  std::vector<unsigned char> arena;
  {
    std::FILE* af = std::fopen(argv[2], "rb");
    if (!af) return 2;
    std::fseek(af, 0, SEEK_END);
    const long size = std::ftell(af);
    std::fseek(af, 0, SEEK_SET);
    arena.resize(static_cast<size_t>(size));
    if (size && std::fread(arena.data(), 1, arena.size(), af) != arena.size()) return 2;
    std::fclose(af);
  }
  const uint64_t n = piece.size();

  std::vector<unsigned char*> block(n, nullptr);
  for (uint64_t i = 0; i < n; ++i) {
    if (arena_off[i] < 0) continue;
    if (piece[i].nbits == 0) {       // any pointer goes: one that must not be read
      piece[i].src = reinterpret_cast<const void*>(static_cast<uintptr_t>(16 + arena_off[i] % 16));
      continue;
    }
    // the piece's aligned words, as offsets in the arena (whose base counts as 16-byte aligned)
    const uint64_t at = static_cast<uint64_t>(arena_off[i]);
    const uint64_t w0 = (at + piece[i].src_bit / 8) & ~3ull, w1 = (at + (piece[i].src_bit + piece[i].nbits + 7) / 8 + 3) & ~3ull;
    if (w1 > ((arena.size() + 3) & ~3ull)) return 2;
    const uint64_t line = w0 & ~15ull;
    void* mem = nullptr;
    if (posix_memalign(&mem, 16, w1 - line) != 0) return 2;
    block[i] = static_cast<unsigned char*>(mem);
    std::memset(block[i], 0x5A, w1 - line);
    for (uint64_t k = w0; k < w1 && k < arena.size(); ++k) block[i][k - line] = arena[k];
    const uintptr_t base = reinterpret_cast<uintptr_t>(block[i]);
    piece[i].src = reinterpret_cast<const void*>(base + at - line);   // (may lie in front of the block: only src + src_bit / 8 onwards is read)
    g_words.emplace_back(base + (w0 - line), base + (w1 - line));
  }
  std::sort(g_words.begin(), g_words.end());
  const uint64_t nbytes = (total_bits + 7) / 8;
  const uint64_t dst_size = kGuard + dst_mod + nbytes + kGuard;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, dst_size) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::memset(dst_block, 0xA5, dst_size);
  unsigned char* dst = dst_block + kGuard + dst_mod;

  zamd::BitjoinTable T;
  T.piece = piece.data();
  T.n = n;
  T.dst = dst;
  T.total_bits = total_bits;
  const uint64_t nvec = zamd::BitjoinVectors(dst, total_bits);
  const uint64_t ntiles = (nvec + zamd::kBitjoinTileVecs - 1) / zamd::kBitjoinTileVecs;
  for (uint64_t tile = 0; tile < ntiles; ++tile) {
    for (uint32_t thread = 0; thread < zamd::kBitjoinThreads; ++thread) zamd::BitjoinTile(T, tile, thread, zamd::kBitjoinThreads);
  }

  int rc = 0;
  if (g_stray_loads) rc = Bad("reads outside the aligned words of the pieces: count", g_stray_loads);
  // the search alone: every piece's first and last bit
  for (uint64_t i = 0; i < n && !rc; ++i) {
    if (piece[i].nbits == 0) continue;
    if (zamd::BitjoinPieceAt(piece.data(), n, piece[i].dst_bit) != i) rc = Bad("BitjoinPieceAt: first bit of piece", i);
    if (zamd::BitjoinPieceAt(piece.data(), n, piece[i].dst_bit + piece[i].nbits - 1) != i) rc = Bad("BitjoinPieceAt: last bit of piece", i);
  }
  std::vector<unsigned char> want(nbytes, 0);
  for (uint64_t i = 0; i < n; ++i) {
    const unsigned char* s = static_cast<const unsigned char*>(piece[i].src);
    for (uint64_t k = 0; k < piece[i].nbits; ++k) {
      const uint64_t to = piece[i].dst_bit + k;
      want[to / 8] = static_cast<unsigned char>(want[to / 8] | (Bit(s, piece[i].src_bit + k) << (to % 8)));
    }
  }
  for (uint64_t j = 0; j < nbytes && !rc; ++j) if (dst[j] != want[j]) rc = Bad("destination differs", j);
  for (uint64_t j = 0; j < kGuard + dst_mod && !rc; ++j) if (dst_block[j] != 0xA5) rc = Bad("written before the destination", j);
  for (uint64_t j = 0; j < kGuard && !rc; ++j) if (dst[nbytes + j] != 0xA5) rc = Bad("written behind the destination", j);
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  if (nbytes && std::fwrite(dst, 1, nbytes, o) != nbytes) return 2;
  std::fclose(o);
  if (!rc) std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n, nbytes, ntiles);
  for (uint64_t i = 0; i < n; ++i) std::free(block[i]);
  std::free(dst_block);
  return rc;
}
