// The rules of device/zmx_png_lossy.h on the CPU: the __host__ __device__ functions k_png_lossy_stats, k_png_lossy_carry
// and k_png_lossy_fill are made of, run by a plain C++ program, the threads of a launch one after the other
// (tests/test_cpu_png_lossy_cases.py).
//   png_lossy_print IN OUT SRC_MOD DST_MOD WIDTH HEIGHT COLORTYPE BITDEPTH out|inplace
// IN: the image's bytes.  It lies at SRC_MOD (0 .. 15) bytes into a heap block of its own that ends with its last byte (a
// read beyond it is the sanitizer's to find).  The statistics are taken, the mode decided, the carry-ins made in carry
// mode and the image rewritten — the workgroups in falling order when DST_MOD is odd: the result may not depend on who
// comes first — at DST_MOD bytes behind a 16-byte boundary, with 64 guard bytes of 0xA5 on both sides, or over the image
// itself (`inplace`).  Without a transparent pixel the output is a copy, as the device layer makes it.  The rewritten
// image is written to OUT.  Prints
//   ok MODE PARTIAL NUMCOLORS FILL_R FILL_G FILL_B FIRST(-1: none) | PIXELS_PER_CHUNK TILE_PIXELS SWEEP_PIXELS SCAN_STEP_TILES GRID TILES
// or what is wrong (exit status 1).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zmx_png_lossy.h"

namespace {
constexpr size_t kGuard = 64;
using namespace zamd;

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}

// k_png_lossy_stats, workgroup by workgroup
void RunStats(const PngColorImage& I, PngLossyState* state, std::vector<uint32_t>* summaries, bool falling) {
  const uint32_t groups = PngLossyGrid(I);
  const uint64_t tiles = PngLossyTiles(I);
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    PngColorSlot table[kPngColorSlots];
    uint32_t count = 0, stop = 0;
    const PngColorGroup grp{table, &count, &stop};
    for (uint32_t local = kPngLossyThreads; local-- > 0;) PngColorGroupBegin(&state->color, grp, local);
    std::vector<PngLossyAcc> acc(kPngLossyThreads, PngLossyAccNone());
    std::vector<PngLossyCounter> cnt(kPngLossyThreads, PngLossyCounter{0u, false});
    for (uint64_t tile = group; tile < tiles; tile += groups) {
      PngLossyTileBegin(state, grp);
      uint64_t best = 0;
      for (uint32_t k = 0; k < kPngLossyThreads; ++k) {
        const uint32_t local = falling ? kPngLossyThreads - 1 - k : k;
        const uint64_t key = PngLossyStatsChunkOf(I, grp, tile, local, &acc[local], &cnt[local]);
        if (key > best) best = key;
      }
      (*summaries)[tile] = PngLossySummaryOf(best);
    }
    PngLossyAcc sum = PngLossyAccNone();
    for (uint32_t local = 0; local < kPngLossyThreads; ++local) PngLossyAccJoin(&sum, acc[local]);
    PngLossyGroupEnd(state, sum, stop);
    for (uint32_t local = 0; local < kPngLossyThreads; ++local) PngColorGroupFlush(&state->color, grp, local);
  }
}

// the exclusive scan of a step's values under PngLossyPick, seeded; the inclusive result of the last one is returned
uint32_t Scan(const std::vector<uint32_t>& v, uint32_t seed, std::vector<uint32_t>* before) {
  uint32_t run = seed;
  for (size_t t = 0; t < v.size(); ++t) {
    (*before)[t] = run;
    run = PngLossyPick(run, v[t]);
  }
  return run;
}

// k_png_lossy_carry: kPngLossyScanStep tiles a step
void RunCarry(const std::vector<uint32_t>& summaries, std::vector<uint32_t>* carry_in) {
  const uint64_t tiles = summaries.size();
  uint32_t carry = kPngLossyNone;
  std::vector<uint32_t> v(kPngLossyScanStep), before(kPngLossyScanStep);
  for (uint64_t base = 0; base < tiles; base += kPngLossyScanStep) {
    for (uint32_t t = 0; t < kPngLossyScanStep; ++t) v[t] = base + t < tiles ? summaries[base + t] : kPngLossyNone;
    carry = Scan(v, carry, &before);
    for (uint32_t t = 0; t < kPngLossyScanStep; ++t) if (base + t < tiles) (*carry_in)[base + t] = before[t];
  }
}

// k_png_lossy_fill, workgroup by workgroup
void RunFill(const PngLossyParams& P, bool falling) {
  const uint32_t groups = PngLossyGrid(P.in);
  const uint64_t tiles = PngLossyTiles(P.in);
  std::vector<uint32_t> w(12 * kPngLossyThreads), npix(kPngLossyThreads), v(kPngLossyThreads), before(kPngLossyThreads);
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    uint32_t fill = kPngLossyNone;
    if (P.mode == kPngLossyModeFixed) {
      fill = PngLossyPixelRgb(P.in, P.first_transparent);
      if (group == 0) P.state->fill = fill;
    }
    for (uint64_t tile = group; tile < tiles; tile += groups) {
      for (uint32_t local = 0; local < kPngLossyThreads; ++local) v[local] = PngLossyFillLoadOf(P, tile, local, &w[12 * local], &npix[local]);
      if (P.mode == kPngLossyModeCarry) Scan(v, P.carry_in[tile], &before);
      for (uint32_t k = 0; k < kPngLossyThreads; ++k) {
        const uint32_t local = falling ? kPngLossyThreads - 1 - k : k;
        PngLossyFillStoreOf(P, tile, local, &w[12 * local], npix[local], P.mode == kPngLossyModeCarry ? before[local] : fill);
      }
    }
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: png_lossy_print IN OUT SRC_MOD DST_MOD WIDTH HEIGHT COLORTYPE BITDEPTH out|inplace\n");
    return 2;
  }
  const uint64_t src_mod = std::strtoull(argv[3], nullptr, 10), dst_mod = std::strtoull(argv[4], nullptr, 10);
  const uint32_t width = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10)), height = static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10));
  const uint32_t colortype = static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10)), bitdepth = static_cast<uint32_t>(std::strtoul(argv[8], nullptr, 10));
  const bool inplace = std::string(argv[9]) == "inplace";
  if (src_mod > 15 || dst_mod > 15 || width == 0 || height == 0) return 2;
  if (!(colortype == 4 || colortype == 6) || !(bitdepth == 8 || bitdepth == 16)) return 2;
  const uint64_t numpixels = static_cast<uint64_t>(width) * height;
  const uint64_t nbytes = numpixels * PngColorPixelBytes(colortype, bitdepth);

  // (the block ends with the image's last byte)
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, src_mod + nbytes) != 0) return 2;
  unsigned char* block = static_cast<unsigned char*>(mem);
  std::memset(block, 0x5A, src_mod + nbytes);
  unsigned char* image = block + src_mod;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(image, 1, nbytes, f) != nbytes) return 2;
  std::fclose(f);
  const std::vector<unsigned char> image_before(image, image + nbytes);

  PngColorImage I;
  I.pixels = image;
  I.numpixels = numpixels;
  I.width = width;
  I.height = height;
  I.colortype = colortype;
  I.bitdepth = bitdepth;
  const bool falling = (dst_mod & 1) != 0;
  const uint64_t tiles = PngLossyTiles(I);

  PngLossyState state;
  std::memset(&state, 0xff, sizeof(state));
  std::memset(&state.color, 0, offsetof(PngColorState, key_min));
  std::vector<uint32_t> summaries(tiles, 0xdeadbeefu), carry_in(tiles, 0xdeadbeefu);
  RunStats(I, &state, &summaries, falling);
  const PngLossyDecision d = PngLossyDecide(state);

  const uint64_t dst_size = kGuard + dst_mod + nbytes + kGuard;
  void* dst_mem = nullptr;
  if (posix_memalign(&dst_mem, 16, dst_size) != 0) return 2;
  unsigned char* dst_block = static_cast<unsigned char*>(dst_mem);
  std::memset(dst_block, 0xA5, dst_size);
  unsigned char* dst = inplace ? image : dst_block + kGuard + dst_mod;

  if (d.mode == kPngLossyModeNone) {
    if (!inplace) std::memcpy(dst, image, nbytes);
  } else {
    if (d.mode == kPngLossyModeCarry) RunCarry(summaries, &carry_in);
    PngLossyParams P;
    P.in = I;
    P.out = dst;
    P.mode = d.mode;
    P.first_transparent = state.first_transparent;
    P.carry_in = carry_in.data();
    P.state = &state;
    RunFill(P, falling);
  }

  int rc = 0;
  for (uint64_t j = 0; j < kGuard + dst_mod && !rc; ++j) if (dst_block[j] != 0xA5) rc = Bad("written before the output", j);
  for (uint64_t j = 0; j < kGuard && !rc; ++j) {
    if (dst_block[kGuard + dst_mod + (inplace ? 0 : nbytes) + j] != 0xA5) rc = Bad("written behind the output", j);
  }
  if (!rc && !inplace && std::memcmp(image, image_before.data(), nbytes) != 0) rc = Bad("the image changed", 0);
  for (uint64_t j = 0; j < src_mod && !rc; ++j) if (block[j] != 0x5A) rc = Bad("written in front of the image", j);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  if (nbytes && std::fwrite(dst, 1, nbytes, o) != nbytes) return 2;
  std::fclose(o);
  if (!rc) {
    const uint32_t fill = d.mode == kPngLossyModeFixed ? state.fill : 0u;
    const uint32_t per_chunk = kPngColorChunk / PngColorPixelBytes(colortype, bitdepth);
    const uint64_t tile_pixels = PngLossyTilePixels(colortype, bitdepth);
    std::printf("ok %u %u %u %u %u %u %" PRId64 " | %u %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 "\n", d.mode, d.partial_alpha, d.numcolors,
                fill & 255u, (fill >> 8) & 255u, (fill >> 16) & 255u,
                state.first_transparent == kPngLossyNoIndex ? static_cast<int64_t>(-1) : static_cast<int64_t>(state.first_transparent),
                per_chunk, tile_pixels, tile_pixels * kPngColorMaxBlocks, kPngLossyScanStep, PngLossyGrid(I), tiles);
  }
  std::free(block);
  std::free(dst_block);
  return rc;
}
