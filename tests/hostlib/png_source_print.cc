// The rules of device/zmx_png_pack.h and host/png_source.h on the CPU: the __host__ __device__ functions k_png_pack is made
// of, run by a plain C++ program, the threads of a launch one after the other (tests/test_cpu_png_source_cases.py).
//   png_source_print IN OUT FALLING
// IN: a little-endian u32 count, then per case the record tests/png_source_cases.py: Case.record packs —
//   u64 buflen, u64 fake, i64 offset, stride_y, stride_x, stride_c, u32 width, height, channels, sample, bitdepth,
//   u8 order[4], u32 src_mod, dst_mod — and buflen bytes, the source's allocation.
// A case with fake != 0 is only CHECKED: d_data = fake + offset, no memory behind it.  Every other case is checked and RUN:
// its allocation lies src_mod bytes (a multiple of 4) into a heap block of its own that ends with its last byte — a read
// beyond it is the sanitizer's to find —, d_data = the allocation + offset, and its extent must lie inside the allocation.
// It is packed twice: by a launch of its own, dst_mod bytes behind a 16-byte boundary with 64 guard bytes of 0xA5 on both
// sides, and by ONE launch of all run cases whose destinations lie one behind the other in one arena, each at its dst_mod,
// only the filler bytes that takes between them — neighbours share 16-byte vectors.  The workgroups run in falling order
// when FALLING is 1.  Guards, fillers and every allocation must be as they were.  OUT gets every run case's packed bytes of
// the single launches, then those of the batch.  Prints per case
//   check I REFUSAL...                      (a refused case: the text behind "source I: ")
//   check I ok NBYTES COLORTYPE LO HI       (the extent's offsets from d_data)
//   run I PATH TILES                        (a run case: the path taken and its tiles)
// and at the end `batch TILES GRID` and `ok`, or what is wrong (exit status 1).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "png_source.h"
#include "zmx_png_pack.h"

namespace {
constexpr size_t kGuard = 64;
using namespace zamd;

#pragma pack(push, 1)
struct Record {
  uint64_t buflen, fake;
  int64_t offset, stride_y, stride_x, stride_c;
  uint32_t width, height, channels, sample, bitdepth;
  uint8_t order[4];
  uint32_t src_mod, dst_mod;
};
#pragma pack(pop)

struct Run {
  size_t index;
  zmx_png_source src;
  PngSourcePlan plan;
  unsigned char* block;   // src_mod bytes of 0x5A, then the allocation
  std::vector<unsigned char> before;
  uint32_t src_mod, dst_mod;
};

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}

// k_png_pack over a table, workgroup by workgroup
void Launch(const PngPackTable& T, uint64_t ntiles, bool falling) {
  const uint32_t groups = PngPackGrid(ntiles);
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    for (uint64_t tile = group; tile < ntiles; tile += groups) {
      for (uint32_t k = 0; k < kPngPackThreads; ++k) PngPackManyTile(T, tile, falling ? kPngPackThreads - 1 - k : k, kPngPackThreads);
    }
  }
}

int SourceIntact(const Run& r) {
  const size_t n = r.before.size();
  if (n && std::memcmp(r.block + r.src_mod, r.before.data(), n) != 0) return Bad("a source changed: case", r.index);
  for (uint32_t j = 0; j < r.src_mod; ++j) if (r.block[j] != 0x5A) return Bad("written in front of a source: case", r.index);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: png_source_print IN OUT FALLING\n");
    return 2;
  }
  const bool falling = std::strtoul(argv[3], nullptr, 10) != 0;
  std::FILE* f = std::fopen(argv[1], "rb");
  uint32_t count = 0;
  if (!f || std::fread(&count, 4, 1, f) != 1) return 2;
  std::vector<Run> runs;
  for (uint32_t i = 0; i < count; ++i) {
    Record rec;
    if (std::fread(&rec, sizeof(rec), 1, f) != 1) return 2;
    zmx_png_source s;
    std::memset(&s, 0, sizeof(s));
    s.stride_y = rec.stride_y;
    s.stride_x = rec.stride_x;
    s.stride_c = rec.stride_c;
    s.width = rec.width;
    s.height = rec.height;
    s.channels = rec.channels;
    s.sample = rec.sample;
    s.bitdepth = rec.bitdepth;
    std::memcpy(s.order, rec.order, 4);
    Run r;
    r.index = i;
    r.block = nullptr;
    r.src_mod = rec.src_mod;
    r.dst_mod = rec.dst_mod;
    if (rec.fake != 0) {
      s.d_data = reinterpret_cast<const void*>(static_cast<uintptr_t>(rec.fake + static_cast<uint64_t>(rec.offset)));
      if (rec.fake == 1) s.d_data = nullptr;
    } else {
      if (rec.src_mod > 12 || rec.src_mod % 4 != 0 || rec.dst_mod > 15) return 2;
      void* mem = nullptr;
      if (posix_memalign(&mem, 16, rec.src_mod + rec.buflen + (rec.buflen == 0)) != 0) return 2;
      r.block = static_cast<unsigned char*>(mem);
      std::memset(r.block, 0x5A, rec.src_mod);
      if (rec.buflen && std::fread(r.block + rec.src_mod, 1, rec.buflen, f) != rec.buflen) return 2;
      r.before.assign(r.block + rec.src_mod, r.block + rec.src_mod + rec.buflen);
      s.d_data = r.block + rec.src_mod + rec.offset;
    }
    r.src = s;
    const std::string msg = CheckPngSource("-", &r.src, &r.plan);
    if (!msg.empty()) {
      std::printf("check %u %s\n", i, msg.c_str() + 3);
      if (rec.fake == 0) return Bad("a case that was to run is refused", i);
      continue;
    }
    int64_t lo = 0, hi = 0;
    PngSourceExtent(r.src, &lo, &hi);
    std::printf("check %u ok %zu %u %" PRId64 " %" PRId64 "\n", i, r.plan.nbytes, r.plan.image.colortype, lo, hi);
    if (rec.fake != 0) continue;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(r.block + rec.src_mod);
    if (r.plan.lo < a0 || r.plan.hi > a0 + rec.buflen) return Bad("the extent leaves the allocation: case", i);
    runs.push_back(std::move(r));
  }
  std::fclose(f);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;

  // ---- every case by a launch of its own
  for (const Run& r : runs) {
    const size_t total = r.plan.nbytes, size = kGuard + r.dst_mod + total + kGuard;
    void* mem = nullptr;
    if (posix_memalign(&mem, 16, size) != 0) return 2;
    unsigned char* block = static_cast<unsigned char*>(mem);
    std::memset(block, 0xA5, size);
    unsigned char* out = block + kGuard + r.dst_mod;
    const PngPackSource rec = PngPackSourceOf(r.src, out);
    const uint64_t tile_start[2] = {0, PngPackTiles(rec.out, rec.total)};
    const PngPackTable T{&rec, tile_start, 1};
    Launch(T, tile_start[1], falling);
    std::printf("run %zu %u %" PRIu64 "\n", r.index, rec.path, tile_start[1]);
    for (size_t j = 0; j < kGuard + r.dst_mod; ++j) if (block[j] != 0xA5) return Bad("written before the output: case", r.index);
    for (size_t j = 0; j < kGuard; ++j) if (out[total + j] != 0xA5) return Bad("written behind the output: case", r.index);
    if (SourceIntact(r)) return 1;
    if (std::fwrite(out, 1, total, o) != total) return 2;
    std::free(block);
  }

  // ---- all of them by one launch, the destinations one behind the other
  if (!runs.empty()) {
    std::vector<size_t> at(runs.size());
    size_t cur = kGuard;
    for (size_t k = 0; k < runs.size(); ++k) {
      cur += (runs[k].dst_mod + 16 - cur % 16) % 16;
      at[k] = cur;
      cur += runs[k].plan.nbytes;
    }
    const size_t size = cur + kGuard;
    void* mem = nullptr;
    if (posix_memalign(&mem, 16, size) != 0) return 2;
    unsigned char* arena = static_cast<unsigned char*>(mem);
    std::memset(arena, 0xA5, size);
    std::vector<PngPackSource> recs(runs.size());
    std::vector<uint64_t> tile_start(runs.size() + 1, 0);
    std::vector<unsigned char> mine(size, 0);
    for (size_t k = 0; k < runs.size(); ++k) {
      recs[k] = PngPackSourceOf(runs[k].src, arena + at[k]);
      tile_start[k + 1] = tile_start[k] + PngPackTiles(recs[k].out, recs[k].total);
      std::memset(mine.data() + at[k], 1, runs[k].plan.nbytes);
    }
    const PngPackTable T{recs.data(), tile_start.data(), runs.size()};
    Launch(T, tile_start[runs.size()], falling);
    // (0xA5 may be a packed byte; a guard or a filler is not)
    for (size_t j = 0; j < size; ++j) if (!mine[j] && arena[j] != 0xA5) return Bad("the batch wrote outside its destinations: arena byte", j);
    for (const Run& r : runs) if (SourceIntact(r)) return 1;
    for (size_t k = 0; k < runs.size(); ++k) {
      if (std::fwrite(arena + at[k], 1, runs[k].plan.nbytes, o) != runs[k].plan.nbytes) return 2;
    }
    std::printf("batch %" PRIu64 " %u\n", tile_start[runs.size()], PngPackGrid(tile_start[runs.size()]));
    std::free(arena);
  }
  std::fclose(o);
  for (Run& r : runs) std::free(r.block);
  std::printf("ok\n");
  return 0;
}
