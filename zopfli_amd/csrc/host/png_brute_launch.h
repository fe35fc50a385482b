// How k_png_brute (device/zmx_png_brute.h) is launched for rows of n bytes: where the per-position arrays live, a
// workgroup's slice of the scratch, the grid and the dynamic LDS.  Plain C++ with no HIP in it, so that a CPU program
// (tests/hostlib/png_brute_print.cc `launch`) prints what the driver (device/drv_png.h PngBruteTypes) will do and a test
// holds it to the formulas' own statement.  The constants are the kernel header's; drv_png.h asserts that.
#ifndef ZMX_PNG_BRUTE_LAUNCH_H_
#define ZMX_PNG_BRUTE_LAUNCH_H_

#include <stdint.h>

#include <algorithm>

namespace zamd {

constexpr uint32_t kPngBruteHeadBytes = 65536u * 4u;      // PNGB_HEAD_BYTES
constexpr uint32_t kPngBruteLdsMax = 148u * 1024u;        // PNGB_LDS_MAX
constexpr uint32_t kPngBruteLdsDefault = 64u * 1024u;     // above it the kernel's dynamic LDS limit has to be raised

// bytes of the per-position arrays of a row of n bytes (pngb_row_bytes)
inline uint64_t PngBruteRowBytes(uint32_t n) { return static_cast<uint64_t>((n + 3u) & ~3u) + 8ull * n; }

// What a test may turn (zmx_internal_png_brute_sizes); the default is what every other caller gets.
struct PngBruteKnobs {
  int force_scratch = 0;          // the per-position arrays in the global scratch whatever the row length
  uint32_t max_workgroups = 0;    // a cap on the grid; 0: none
};

struct PngBruteLaunch {
  bool in_lds;            // the per-position arrays live in the dynamic LDS
  bool raise_lds_limit;   // hipFuncAttributeMaxDynamicSharedMemorySize to kPngBruteLdsMax before the launch
  uint64_t row_bytes;
  uint64_t stride;        // bytes of scratch per workgroup
  uint32_t grid;
  uint32_t lds_bytes;     // dynamic LDS of the launch
};

inline PngBruteLaunch PngBruteMakeLaunch(uint32_t n, uint32_t jobs, const PngBruteKnobs& knobs = PngBruteKnobs()) {
  PngBruteLaunch L;
  // the per-position arrays in the dynamic LDS when they fit, else in the scratch beside the head table and the results
  L.row_bytes = PngBruteRowBytes(n);
  L.in_lds = !knobs.force_scratch && L.row_bytes <= kPngBruteLdsMax;
  L.stride = (kPngBruteHeadBytes + 4ull * n + (L.in_lds ? 0 : L.row_bytes) + 255u) & ~255ull;
  // two 1024-lane workgroups fill a CU's 32 waves; the LDS may allow fewer
  const uint64_t per_cu = L.in_lds ? std::max<uint64_t>(1, std::min<uint64_t>(2, (160u * 1024u) / (L.row_bytes + 12u * 1024u))) : 1;
  const uint64_t budget = 1ull << 30;
  uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>({static_cast<uint64_t>(jobs), 256 * per_cu, budget / L.stride}));
  if (knobs.max_workgroups != 0) grid = std::min<uint64_t>(grid, knobs.max_workgroups);
  L.grid = static_cast<uint32_t>(grid);
  L.raise_lds_limit = L.in_lds && L.row_bytes > kPngBruteLdsDefault;
  L.lds_bytes = L.in_lds ? static_cast<uint32_t>(L.row_bytes) : 0u;
  return L;
}

}  // namespace zamd

#endif  // ZMX_PNG_BRUTE_LAUNCH_H_
