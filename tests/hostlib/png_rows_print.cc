// The rules of device/zmx_png_rows.h on the CPU: the __host__ __device__ functions k_png_rows is made of — the mapping
// from an output byte to (row, x), the byte-wise filters, the in-row vectors with their windows — run by a plain C++
// program, the threads of the launch one after the other (tests/test_cpu_png_rows_cases.py).
//   png_rows_print IN OUT SRC_MOD DST_MOD LINEBYTES HEIGHT BYTEWIDTH
// IN: the image's HEIGHT * LINEBYTES bytes, then the HEIGHT filter types.  The image lies at SRC_MOD (0 .. 15) bytes into
// a heap block of its own that ends with the last aligned word holding one of its bytes (a read beyond that is the
// sanitizer's to find), and every address of the image the rules read (ZMX_PNGR_SEE_LOAD) is held against the aligned
// words of the image: a read in front of its first word or behind its last is reported here, whatever the build.  The
// output lies at DST_MOD bytes behind a 16-byte boundary, with 64 guard bytes of 0xA5 on both sides.  The scanlines are
// written to OUT; prints "ok TOTAL GRID BADROW" (BADROW -1: every type was at most 4), or what is wrong (exit status 1).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
uintptr_t g_words_lo = 0, g_words_hi = 0;   // the aligned words of the image
uint64_t g_stray_loads = 0;

void SeeLoad(const void* p, size_t n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (a < g_words_lo || a + n > g_words_hi) ++g_stray_loads;
}
}  // namespace
#define ZMX_PNGR_SEE_LOAD(p, n) SeeLoad(p, n)

#include "zmx_png_rows.h"

namespace {
constexpr size_t kGuard = 64;

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 8) {
    std::fprintf(stderr, "usage: png_rows_print IN OUT SRC_MOD DST_MOD LINEBYTES HEIGHT BYTEWIDTH\n");
    return 2;
  }
  const uint64_t src_mod = std::strtoull(argv[3], nullptr, 10), dst_mod = std::strtoull(argv[4], nullptr, 10);
  const uint64_t linebytes = std::strtoull(argv[5], nullptr, 10), height = std::strtoull(argv[6], nullptr, 10);
  const uint64_t bytewidth = std::strtoull(argv[7], nullptr, 10);
  if (src_mod > 15 || dst_mod > 15 || linebytes == 0 || height == 0 || bytewidth == 0 || bytewidth > 8) return 2;
  const uint64_t npix = linebytes * height, total = height * (linebytes + 1);

  // (the block ends with the last aligned word that holds a byte of the image)
  const uint64_t block_size = (src_mod + npix + 3) / 4 * 4;
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, block_size) != 0) return 2;
  unsigned char* block = static_cast<unsigned char*>(mem);
  std::memset(block, 0x5A, block_size);
  unsigned char* image = block + src_mod;
  std::vector<unsigned char> types(height);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(image, 1, npix, f) != npix || std::fread(types.data(), 1, height, f) != height) return 2;
  std::fclose(f);
  const std::vector<unsigned char> image_before(image, image + npix);
  g_words_lo = reinterpret_cast<uintptr_t>(image) & ~static_cast<uintptr_t>(3);
  g_words_hi = (reinterpret_cast<uintptr_t>(image) + npix + 3) & ~static_cast<uintptr_t>(3);

  const uint64_t dst_size = kGuard + dst_mod + total + kGuard;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, dst_size) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::memset(dst_block, 0xA5, dst_size);
  unsigned char* dst = dst_block + kGuard + dst_mod;

  uint32_t bad_row = zamd::kPngRowsNoBadRow;
  zamd::PngRowsParams P;
  P.image = image;
  P.types = types.data();
  P.out = dst;
  P.linebytes = linebytes;
  P.height = height;
  P.bytewidth = static_cast<uint32_t>(bytewidth);
  P.bad_row = &bad_row;
  const uint32_t grid = zamd::PngRowsGrid(total);
  const uint64_t threads = static_cast<uint64_t>(grid) * zamd::kPngRowsThreads;
  for (uint64_t thread = 0; thread < threads; ++thread) zamd::PngRowsRun(P, thread, threads);

  int rc = 0;
  if (g_stray_loads) rc = Bad("reads outside the aligned words of the image: count", g_stray_loads);
  // the mapping alone: the first and the last byte of every scanline
  for (uint64_t r = 0; r < height && !rc; ++r) {
    uint64_t row = 0, x = 0;
    zamd::PngRowsAt(r * (linebytes + 1), linebytes, &row, &x);
    if (row != r || x != 0) rc = Bad("PngRowsAt: first byte of row", r);
    zamd::PngRowsAt(r * (linebytes + 1) + linebytes, linebytes, &row, &x);
    if (row != r || x != linebytes) rc = Bad("PngRowsAt: last byte of row", r);
  }
  for (uint64_t j = 0; j < kGuard + dst_mod && !rc; ++j) if (dst_block[j] != 0xA5) rc = Bad("written before the output", j);
  for (uint64_t j = 0; j < kGuard && !rc; ++j) if (dst[total + j] != 0xA5) rc = Bad("written behind the output", j);
  if (!rc && std::memcmp(image, image_before.data(), npix) != 0) rc = Bad("the image changed", 0);
  for (uint64_t j = 0; j < block_size && !rc; ++j) {
    if ((j < src_mod || j >= src_mod + npix) && block[j] != 0x5A) rc = Bad("written beside the image", j);
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  if (std::fwrite(dst, 1, total, o) != total) return 2;
  std::fclose(o);
  if (!rc) {
    std::printf("ok %" PRIu64 " %u %" PRId64 "\n", total, grid,
                bad_row == zamd::kPngRowsNoBadRow ? static_cast<int64_t>(-1) : static_cast<int64_t>(bad_row));
  }
  std::free(block);
  std::free(dst_block);
  return rc;
}
