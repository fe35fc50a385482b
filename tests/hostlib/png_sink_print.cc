// The rules of device/zmx_png_unpack.h and host/png_sink.h on the CPU: the __host__ __device__ functions k_png_unpack is
// made of, run by a plain C++ program, the threads of a launch one after the other (tests/test_cpu_png_sink_cases.py).
//   png_sink_print constants
//     prints "TILE_PIXELS RUN THREADS MAX_BLOCKS".
//   png_sink_print IN OUT FALLING
// IN: a little-endian u32 count, then per case
//   the mode: u32 width, height, colortype, bitdepth, palettesize, has_key, key_r, key_g, key_b and the 1024 palette bytes;
//   the sink (tests/png_sink_cases.py: Sink.record): u64 buflen, u64 fake, i64 offset, stride_y, stride_x, stride_c,
//   u32 width, height, channels, sample, bitdepth, u8 order[4], u32 base_mod;
//   u32 own_mod, u64 ownlen and ownlen bytes: the own-mode pixels.
// A case with fake != 0 is only CHECKED (zmx_png_sink_check's rules): d_data = fake + offset (fake 1: null), no memory
// behind it.  Every other case is checked and RUN: its allocation of buflen bytes of 0xA5 lies base_mod bytes behind a
// 16-byte boundary in a heap block of its own that ends with its last byte, its pixels own_mod bytes behind one likewise
// — a byte too many read or written is the sanitizer's to find —, d_data = the allocation + offset, and the extent must
// lie inside the allocation.  It is stored twice: by a launch of its own, and by ONE launch of all run cases into fresh
// allocations.  Every store is counted through Par::NoteWrite, byte by byte: a store outside every allocation ends the
// program.  The workgroups and the threads run in falling order when FALLING is 1.  The pixels must be as they were.
// OUT gets, per run case, the allocation and then the allocation's write counts (a byte each) of the single launches,
// then the same of the batch.  Prints per case
//   check I REFUSAL...                      (a refused case: the text behind "sink I: ")
//   check I ok LO HI                        (the extent's offsets from d_data)
//   run I PATH TILES
// and at the end `batch TILES GRID` and `ok`, or what is wrong (exit status 1).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "png_sink.h"
#include "zmx_png_unpack.h"

namespace {
using namespace zamd;

#pragma pack(push, 1)
struct ModeRecord {
  uint32_t width, height, colortype, bitdepth, palettesize, has_key, key_r, key_g, key_b;
  unsigned char palette[1024];
};
struct SinkRecord {
  uint64_t buflen, fake;
  int64_t offset, stride_y, stride_x, stride_c;
  uint32_t width, height, channels, sample, bitdepth;
  uint8_t order[4];
  uint32_t base_mod;
};
struct OwnRecord {
  uint32_t own_mod;
  uint64_t ownlen;
};
#pragma pack(pop)

// a heap block of mod + n bytes that begins at a 16-byte boundary and ends with its last byte
unsigned char* Block(size_t mod, size_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, mod + n ? mod + n : 1) != 0) std::abort();
  return static_cast<unsigned char*>(p);
}

struct Run {
  size_t index;
  zmx_png_decode_result mode;
  SinkRecord rec;
  unsigned char* own_block;   // own_mod bytes, then the pixels
  uint32_t own_mod;
  std::vector<unsigned char> own_before;
};

struct Target {   // an allocation stores may go to, and how often each byte was written
  uintptr_t lo, hi;
  std::vector<unsigned char>* counts;
};

// The stores of a launch, counted byte by byte.
struct CountPar {
  std::vector<Target> targets;   // sorted by lo
  mutable bool outside = false;
  void Sort() {
    std::sort(targets.begin(), targets.end(), [](const Target& a, const Target& b) { return a.lo < b.lo; });
  }
  void NoteWrite(const void* p, uint64_t n) const {
    const uintptr_t at = reinterpret_cast<uintptr_t>(p);
    auto it = std::upper_bound(targets.begin(), targets.end(), at, [](uintptr_t v, const Target& t) { return v < t.lo; });
    if (it == targets.begin() || at + n > (it - 1)->hi) {
      outside = true;
      return;
    }
    for (uint64_t k = 0; k < n; ++k) {
      unsigned char& c = (*(it - 1)->counts)[at - (it - 1)->lo + k];
      if (c < 255) ++c;
    }
  }
};

zmx_png_sink SinkOf(const SinkRecord& rec, unsigned char* allocation) {
  zmx_png_sink s;
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
  if (allocation) s.d_data = allocation + rec.offset;
  else s.d_data = rec.fake == 1 ? nullptr : reinterpret_cast<void*>(static_cast<uintptr_t>(rec.fake + static_cast<uint64_t>(rec.offset)));
  return s;
}

// k_png_unpack over a table, workgroup by workgroup: the palette staged by all threads, then the tile by all threads
void Launch(const PngUnpackTable& T, uint64_t ntiles, bool falling, const CountPar& par) {
  const uint32_t groups = PngUnpackGrid(ntiles);
  uint32_t staged[256];
  for (uint32_t n = 0; n < groups; ++n) {
    const uint32_t group = falling ? groups - 1 - n : n;
    for (uint64_t tile = group; tile < ntiles; tile += groups) {
      uint64_t local = 0;
      const PngUnpackJob J = T.jobs[PngUnpackJobOfTile(T, tile, &local)];
      for (uint32_t i = 0; i < 256; ++i) staged[i] = 0xdeadbeefu;   // (what the tile before left is not this tile's)
      if (J.colortype == 3) {
        for (uint32_t k = 0; k < kPngUnpackThreads; ++k) PngUnpackStage(T, J, staged, k, kPngUnpackThreads);
      }
      for (uint32_t k = 0; k < kPngUnpackThreads; ++k) {
        PngUnpackTile(J, staged, local, falling ? kPngUnpackThreads - 1 - k : k, kPngUnpackThreads, par);
      }
    }
  }
}

int Bad(const char* what, uint64_t at) {
  std::printf("%s at %" PRIu64 "\n", what, at);
  return 1;
}

// All of `runs` by one launch into fresh allocations; the allocations and their counts to `o`.
int Store(const std::vector<const Run*>& runs, bool falling, std::FILE* o, uint64_t* ntiles_out) {
  const size_t n = runs.size();
  std::vector<unsigned char*> blocks(n);
  std::vector<std::vector<unsigned char>> counts(n);
  std::vector<PngUnpackJob> jobs;
  std::vector<uint32_t> palettes;
  std::vector<uint64_t> tile_start(n + 1, 0);
  CountPar par;
  for (size_t k = 0; k < n; ++k) {
    const Run& r = *runs[k];
    blocks[k] = Block(r.rec.base_mod, r.rec.buflen);
    unsigned char* const allocation = blocks[k] + r.rec.base_mod;
    std::memset(blocks[k], 0xA5, r.rec.base_mod + r.rec.buflen);
    counts[k].assign(r.rec.buflen, 0);
    par.targets.push_back({reinterpret_cast<uintptr_t>(allocation), reinterpret_cast<uintptr_t>(allocation) + r.rec.buflen, &counts[k]});
    const zmx_png_sink s = SinkOf(r.rec, allocation);
    uint32_t at = 0;
    if (r.mode.colortype == 3) {
      at = static_cast<uint32_t>(palettes.size() / 256);
      palettes.resize(palettes.size() + 256);
      PngUnpackPaletteOf(r.mode, palettes.data() + 256 * static_cast<size_t>(at));
    }
    jobs.push_back(PngUnpackJobOf(s, r.mode, r.own_block + r.own_mod, at));
    tile_start[k + 1] = tile_start[k] + PngUnpackTiles(jobs.back().npixels);
  }
  par.Sort();
  const PngUnpackTable T{jobs.data(), tile_start.data(), palettes.data(), n};
  Launch(T, tile_start[n], falling, par);
  *ntiles_out = tile_start[n];
  if (par.outside) return Bad("a store outside every allocation: first case", runs[0]->index);
  for (size_t k = 0; k < n; ++k) {
    const Run& r = *runs[k];
    for (uint32_t j = 0; j < r.rec.base_mod; ++j) if (blocks[k][j] != 0xA5) return Bad("written in front of an allocation: case", r.index);
    if (!r.own_before.empty() && std::memcmp(r.own_block + r.own_mod, r.own_before.data(), r.own_before.size()) != 0) return Bad("the pixels changed: case", r.index);
    if (std::fwrite(blocks[k] + r.rec.base_mod, 1, r.rec.buflen, o) != r.rec.buflen) return 2;
    if (std::fwrite(counts[k].data(), 1, r.rec.buflen, o) != r.rec.buflen) return 2;
    std::free(blocks[k]);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "constants") == 0) {
    std::printf("%u %u %u %u\n", kPngUnpackTilePixels, kPngUnpackRun, kPngUnpackThreads, kPngUnpackMaxBlocks);
    return 0;
  }
  if (argc != 4) {
    std::fprintf(stderr, "usage: png_sink_print constants | IN OUT FALLING\n");
    return 2;
  }
  const bool falling = std::strtoul(argv[3], nullptr, 10) != 0;
  std::FILE* f = std::fopen(argv[1], "rb");
  uint32_t count = 0;
  if (!f || std::fread(&count, 4, 1, f) != 1) return 2;
  std::vector<Run> runs;
  for (uint32_t i = 0; i < count; ++i) {
    ModeRecord mode;
    SinkRecord rec;
    OwnRecord own;
    if (std::fread(&mode, sizeof(mode), 1, f) != 1 || std::fread(&rec, sizeof(rec), 1, f) != 1 || std::fread(&own, sizeof(own), 1, f) != 1) return 2;
    Run r;
    r.index = i;
    r.rec = rec;
    r.own_mod = own.own_mod;
    std::memset(&r.mode, 0, sizeof(r.mode));
    r.mode.width = mode.width;
    r.mode.height = mode.height;
    r.mode.colortype = mode.colortype;
    r.mode.bitdepth = mode.bitdepth;
    r.mode.palettesize = mode.palettesize;
    r.mode.has_key = mode.has_key;
    r.mode.key_r = mode.key_r;
    r.mode.key_g = mode.key_g;
    r.mode.key_b = mode.key_b;
    std::memcpy(r.mode.palette, mode.palette, 1024);
    if (own.own_mod > 15 || rec.base_mod > 15) return 2;
    r.own_block = Block(own.own_mod, own.ownlen);
    if (own.ownlen && std::fread(r.own_block + own.own_mod, 1, own.ownlen, f) != own.ownlen) return 2;
    r.own_before.assign(r.own_block + own.own_mod, r.own_block + own.own_mod + own.ownlen);
    // ---- the checks, on the sink as it will lie (a run case: in an allocation of this very size)
    unsigned char* probe = rec.fake == 0 ? Block(rec.base_mod, rec.buflen) : nullptr;
    const zmx_png_sink s = SinkOf(rec, probe ? probe + rec.base_mod : nullptr);
    PngSinkPlan plan = {0, 0};
    const std::string msg = CheckPngSink("-", &s, &plan);
    if (!msg.empty()) {
      std::printf("check %u %s\n", i, msg.c_str() + 3);
      if (rec.fake == 0) return Bad("a case that was to run is refused", i);
      std::free(r.own_block);
      continue;
    }
    int64_t lo = 0, hi = 0;
    PngSourceExtent(s, &lo, &hi);
    std::printf("check %u ok %" PRId64 " %" PRId64 "\n", i, lo, hi);
    if (rec.fake != 0) {
      std::free(r.own_block);
      continue;
    }
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(probe + rec.base_mod);
    if (plan.lo < a0 || plan.hi > a0 + rec.buflen) return Bad("the extent leaves the allocation: case", i);
    std::free(probe);
    const std::string bad_mode = CheckPngUnpackMode("-", r.mode, s);
    if (!bad_mode.empty()) {
      std::printf("%s\n", bad_mode.c_str());
      return Bad("a case that was to run has a refused mode", i);
    }
    if (own.ownlen != PngOutSize(kPngDecOwn, mode.width, mode.height, mode.colortype, mode.bitdepth)) return Bad("the pixels are not the mode's size: case", i);
    runs.push_back(std::move(r));
  }
  std::fclose(f);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  // ---- every case by a launch of its own
  for (const Run& r : runs) {
    uint64_t ntiles = 0;
    if (const int rc = Store({&r}, falling, o, &ntiles)) return rc;
    const zmx_png_sink s = SinkOf(r.rec, reinterpret_cast<unsigned char*>(uintptr_t{1} << 20));
    uint8_t order[4];
    for (int k = 0; k < 4; ++k) order[k] = static_cast<uint32_t>(k) < s.channels ? s.order[k] : 0;
    std::printf("run %zu %u %" PRIu64 "\n", r.index, PngPackPathOf(s.stride_x, s.stride_c, s.channels, s.sample, order), ntiles);
  }
  // ---- all of them by one launch
  if (!runs.empty()) {
    std::vector<const Run*> all;
    for (const Run& r : runs) all.push_back(&r);
    uint64_t ntiles = 0;
    if (const int rc = Store(all, falling, o, &ntiles)) return rc;
    std::printf("batch %" PRIu64 " %u\n", ntiles, PngUnpackGrid(ntiles));
  }
  std::fclose(o);
  for (Run& r : runs) std::free(r.own_block);
  std::printf("ok\n");
  return 0;
}
