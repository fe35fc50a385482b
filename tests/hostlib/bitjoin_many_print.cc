// The rules of k_bitjoin_many (device/zmx_bitjoin.h) on the CPU: the tile-to-destination search, the table of the
// destination found and BitjoinTile on the local tile, run by a plain C++ program over every global tile — the grid
// emulated workgroup by workgroup, each striding over the tiles as the kernel does, its 256 threads one after the other
// (tests/test_cpu_bitjoin_many_rules.py).
//   bitjoin_many_print TABLE ARENA OUT GRID...
// TABLE: "LEAD TAIL NDST", then for every destination "GAP TOTAL_BITS NPIECES" followed by its pieces, "offset in ARENA"
// (-1: a null pointer), src_bit, nbits and dst_bit each, all decimal and separated by white space.  The destinations lie
// in one heap block of exactly LEAD + (the destinations and their gaps) + TAIL bytes that begins at a 16-byte boundary:
// the first destination GAP bytes behind its first LEAD bytes, every other GAP bytes behind the one before it (0: back to
// back — neighbours then share a 16-byte vector).  The block is filled with 0xA5 before every run, so a byte the rules
// leave out shows as well as one written outside a destination; a write outside the block is the sanitizer's to find.
// ARENA holds the sources' bytes, each piece copied into an exact heap block of its own and every load held against the
// aligned words of a piece, as in bitjoin_print.cc.  The tile counts are the host's (BitjoinTiles, as the driver's).  One
// run for every GRID (the number of workgroups: 1 .. kBitjoinMaxBlocks; 0 = what the driver launches); all must give the
// same block, which is written to OUT and compared here, bit by bit, with the pieces.  Prints "ok NDST NPIECES TILES", or
// what differs (exit status 1).
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
int Bad(const char* what, uint64_t a, uint64_t b) {
  std::printf("%s: %" PRIu64 " at %" PRIu64 "\n", what, a, b);
  return 1;
}
unsigned Bit(const unsigned char* p, uint64_t k) { return (p[k / 8] >> (k % 8)) & 1u; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: bitjoin_many_print TABLE ARENA OUT GRID...\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long long lead = 0, tail = 0, ndst = 0;
  if (std::fscanf(f, "%llu %llu %llu", &lead, &tail, &ndst) != 3) return 2;
  std::vector<uint64_t> gap(ndst);
  std::vector<zamd::BitDest> dest(ndst);
  std::vector<long long> arena_off;
  std::vector<zamd::BitPiece> piece;
  for (uint64_t d = 0; d < ndst; ++d) {
    unsigned long long g = 0, total = 0, np = 0, b = 0, c = 0, e = 0;
    long long a = 0;
    if (std::fscanf(f, "%llu %llu %llu", &g, &total, &np) != 3) return 2;
    gap[d] = g;
    dest[d] = {nullptr, total, piece.size(), np};
    for (uint64_t i = 0; i < np; ++i) {
      if (std::fscanf(f, "%lld %llu %llu %llu", &a, &b, &c, &e) != 4) return 2;
      arena_off.push_back(a);
      piece.push_back({nullptr, b, c, e});
    }
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

  // ---- every source in an exact heap block of its own (bitjoin_print.cc)
  std::vector<unsigned char*> block(n, nullptr);
  for (uint64_t i = 0; i < n; ++i) {
    if (arena_off[i] < 0) continue;
    if (piece[i].nbits == 0) {       // any pointer goes: one that must not be read
      piece[i].src = reinterpret_cast<const void*>(static_cast<uintptr_t>(16 + arena_off[i] % 16));
      continue;
    }
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
    piece[i].src = reinterpret_cast<const void*>(base + at - line);
    g_words.emplace_back(base + (w0 - line), base + (w1 - line));
  }
  std::sort(g_words.begin(), g_words.end());

  // ---- the destinations in one exact block
  uint64_t size = lead;
  std::vector<uint64_t> at(ndst);
  for (uint64_t d = 0; d < ndst; ++d) {
    at[d] = size + gap[d];
    size = at[d] + (dest[d].total_bits + 7) / 8;
  }
  size += tail;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, size ? size : 1) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::vector<uint64_t> tile_start(ndst + 1, 0);
  for (uint64_t d = 0; d < ndst; ++d) {
    dest[d].dst = dst_block + at[d];
    tile_start[d + 1] = tile_start[d] + zamd::BitjoinTiles(dest[d].dst, dest[d].total_bits);
  }
  const uint64_t ntiles = tile_start[ndst];
  zamd::BitjoinManyTable M;
  M.piece = piece.data();
  M.dest = dest.data();
  M.tile_start = tile_start.data();
  M.ndst = ndst;

  // ---- what the block must hold
  std::vector<unsigned char> want(size, 0xA5);
  for (uint64_t d = 0; d < ndst; ++d) {
    const uint64_t nbytes = (dest[d].total_bits + 7) / 8;
    std::fill(want.begin() + static_cast<long>(at[d]), want.begin() + static_cast<long>(at[d] + nbytes), 0);
    for (uint64_t i = 0; i < dest[d].npieces; ++i) {
      const zamd::BitPiece& q = piece[dest[d].first_piece + i];
      const unsigned char* s = static_cast<const unsigned char*>(q.src);
      for (uint64_t k = 0; k < q.nbits; ++k) {
        const uint64_t to = q.dst_bit + k;
        want[at[d] + to / 8] = static_cast<unsigned char>(want[at[d] + to / 8] | (Bit(s, q.src_bit + k) << (to % 8)));
      }
    }
  }

  int rc = 0;
  // the search alone: the first and the last tile of every destination that has one, and no other
  for (uint64_t d = 0; d < ndst && !rc; ++d) {
    uint64_t local = 0;
    if (tile_start[d + 1] == tile_start[d]) continue;
    if (zamd::BitjoinDestOfTile(tile_start.data(), ndst, tile_start[d], &local) != d || local != 0) rc = Bad("BitjoinDestOfTile: first tile of destination", d, tile_start[d]);
    if (zamd::BitjoinDestOfTile(tile_start.data(), ndst, tile_start[d + 1] - 1, &local) != d || local != tile_start[d + 1] - 1 - tile_start[d]) {
      rc = Bad("BitjoinDestOfTile: last tile of destination", d, tile_start[d + 1] - 1);
    }
  }
  for (int a = 4; a < argc && !rc; ++a) {
    uint64_t grid = std::strtoull(argv[a], nullptr, 10);
    if (grid == 0) grid = std::min<uint64_t>(ntiles, zamd::kBitjoinMaxBlocks);
    if (grid > zamd::kBitjoinMaxBlocks) return 2;
    std::memset(dst_block, 0xA5, size);
    for (uint64_t wg = 0; wg < grid; ++wg) {
      for (uint64_t tile = wg; tile < ntiles; tile += grid) {
        for (uint32_t thread = 0; thread < zamd::kBitjoinThreads; ++thread) zamd::BitjoinManyTile(M, tile, thread, zamd::kBitjoinThreads);
      }
    }
    if (g_stray_loads) rc = Bad("reads outside the aligned words of the pieces: count, grid", g_stray_loads, grid);
    for (uint64_t j = 0; j < size && !rc; ++j) {
      if (dst_block[j] != want[j]) rc = Bad("the block differs: grid, byte", grid, j);
    }
  }
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  if (size && std::fwrite(dst_block, 1, size, o) != size) return 2;
  std::fclose(o);
  if (!rc) std::printf("ok %llu %" PRIu64 " %" PRIu64 "\n", ndst, n, ntiles);
  for (uint64_t i = 0; i < n; ++i) std::free(block[i]);
  std::free(dst_block);
  return rc;
}
