// The rules of device/zmx_gather.h on the CPU: the __host__ __device__ functions k_gather is made of — the tile-to-piece
// search, the walk over a tile's pieces, the copy of a span — run by a plain C++ program, the 256 threads of a workgroup
// one after the other (tests/test_cpu_gather_rules.py).
//   gather_print TABLE OUT
// TABLE: the destination's address mod 16, then for every piece "source address mod 16" and "length", all decimal and
// separated by white space.  Byte j of piece i is (131 i + 7 j + 13) mod 256.  Every piece lies in a heap block of its
// own that ends with the last aligned word holding one of its bytes (a read beyond that is the sanitizer's to find),
// and every address the rules read (ZMX_GATHER_SEE_LOAD) is held against the aligned words of the pieces: a read in
// front of a piece's first word — the block starts at a 16-byte boundary, up to three words before it — or behind its
// last is reported here, whatever the build.  The destination has 64 guard bytes of 0xA5 on both sides.  The gathered bytes are written to OUT and compared here
// with a memcpy of every piece; prints "ok PIECES TOTAL TILES", or what differs (exit status 1).
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
#define ZMX_GATHER_SEE_LOAD(p, n) SeeLoad(p, n)

#include "zmx_gather.h"

namespace {
constexpr size_t kGuard = 64;

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: gather_print TABLE OUT\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long long dst_mod = 0, a = 0, b = 0;
  if (std::fscanf(f, "%llu", &dst_mod) != 1 || dst_mod > 15) return 2;
  std::vector<uint64_t> src_mod, len;
  while (std::fscanf(f, "%llu %llu", &a, &b) == 2) {
    if (a > 15) return 2;
    src_mod.push_back(a);
    len.push_back(b);
  }
  std::fclose(f);
  const uint64_t n = src_mod.size();

  std::vector<unsigned char*> block(n);
  std::vector<const unsigned char*> src(n);
  std::vector<uint64_t> start(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    // (the block ends with the last aligned word that holds a byte of the piece)
    const uint64_t size = (src_mod[i] + len[i] + 3) / 4 * 4;
    void* mem = nullptr;
    if (posix_memalign(&mem, 16, size ? size : 1) != 0) return 2;
    block[i] = static_cast<unsigned char*>(mem);
    std::memset(block[i], 0x5A, size);
    unsigned char* p = block[i] + src_mod[i];
    for (uint64_t j = 0; j < len[i]; ++j) p[j] = static_cast<unsigned char>(131 * i + 7 * j + 13);
    src[i] = p;
    start[i + 1] = start[i] + len[i];
    if (len[i]) {
      const uintptr_t at = reinterpret_cast<uintptr_t>(p);
      g_words.emplace_back(at & ~static_cast<uintptr_t>(3), (at + len[i] + 3) & ~static_cast<uintptr_t>(3));
    }
  }
  std::sort(g_words.begin(), g_words.end());
  const uint64_t total = start[n];
  const uint64_t dst_size = kGuard + dst_mod + total + kGuard;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, dst_size) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::memset(dst_block, 0xA5, dst_size);
  unsigned char* dst = dst_block + kGuard + dst_mod;

  zamd::GatherTable T;
  T.src = src.data();
  T.start = start.data();
  T.dst = dst;
  T.n = n;
  const uint64_t ntiles = (total + zamd::kGatherTile - 1) / zamd::kGatherTile;
  for (uint64_t tile = 0; tile < ntiles; ++tile) {
    for (uint32_t thread = 0; thread < zamd::kGatherThreads; ++thread) zamd::GatherTile(T, tile, thread, zamd::kGatherThreads);
  }

  int rc = 0;
  if (g_stray_loads) rc = Bad("reads outside the aligned words of the pieces: count", g_stray_loads);
  // the search alone: every piece's first and last byte, and the byte before a run of empty pieces
  for (uint64_t i = 0; i < n && !rc; ++i) {
    if (len[i] == 0) continue;
    if (zamd::GatherPieceAt(start.data(), n, start[i]) != i) rc = Bad("GatherPieceAt: first byte of piece", i);
    if (zamd::GatherPieceAt(start.data(), n, start[i + 1] - 1) != i) rc = Bad("GatherPieceAt: last byte of piece", i);
  }
  std::vector<unsigned char> want(total);
  for (uint64_t i = 0; i < n; ++i) if (len[i]) std::memcpy(want.data() + start[i], src[i], len[i]);
  for (uint64_t j = 0; j < total && !rc; ++j) if (dst[j] != want[j]) rc = Bad("destination differs", j);
  for (uint64_t j = 0; j < kGuard + dst_mod && !rc; ++j) if (dst_block[j] != 0xA5) rc = Bad("written before the destination", j);
  for (uint64_t j = 0; j < kGuard && !rc; ++j) if (dst[total + j] != 0xA5) rc = Bad("written behind the destination", j);
  for (uint64_t i = 0; i < n && !rc; ++i) {
    for (uint64_t j = 0; j < len[i] && !rc; ++j) {
      if (src[i][j] != static_cast<unsigned char>(131 * i + 7 * j + 13)) rc = Bad("source changed: piece", i);
    }
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  if (total && std::fwrite(dst, 1, total, o) != total) return 2;
  std::fclose(o);
  if (!rc) std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n, total, ntiles);
  for (uint64_t i = 0; i < n; ++i) std::free(block[i]);
  std::free(dst_block);
  return rc;
}
