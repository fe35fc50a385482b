// TEST-ONLY: the rules of the two pools from the command line — the device memory pool's (zopfli_amd/csrc/device/
// zmx_pool_rules.h) and the context pool's slot choice (zopfli_amd/csrc/host/deal.h).  tests/test_cpu_pools.py calls it.
//   pool_print fit device|pinned WANT CAPS      BestFit over the capacities CAPS ("-" = none): the index, or -1
//   pool_print free DEVICE_CACHED OWN_CACHED CAP KEEP     DecideFree: trim_others cache
//   pool_print pinned                           the pinned rules: least bytes, most cached buffers, largest cached buffer
//   pool_print slots WANT PER_DEVICE SMALL MAY_CREATE_MORE LANES SMALL_LANES DEVICE...     ChooseSlots: a line
//       "device slot create" per pick.  DEVICE = INDEX:SLOTS, or INDEX!:SLOTS for a dead one; SLOTS = a letter per slot,
//       f = free, b = busy, n = busy and its context still being made
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "deal.h"
#include "zmx_pool_rules.h"

namespace {

size_t Number(const char* text) { return static_cast<size_t>(std::strtoull(text, nullptr, 10)); }

std::vector<size_t> Numbers(const char* text) {
  std::vector<size_t> v;
  if (std::strcmp(text, "-") == 0) return v;
  for (const char* p = text; *p;) {
    char* end = nullptr;
    v.push_back(static_cast<size_t>(std::strtoull(p, &end, 10)));
    if (end == p) { v.pop_back(); break; }
    p = *end == ',' ? end + 1 : end;
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "fit" && argc == 5) {
    const std::string list = argv[2];
    if (list != "device" && list != "pinned") return 2;
    zamd::CachedBlocks blocks;
    for (size_t cap : Numbers(argv[4])) blocks.emplace_back(nullptr, cap);
    const size_t best = zamd::BestFit(blocks, Number(argv[3]), list == "device" ? zamd::kDeviceFit : zamd::kPinnedFit);
    std::printf("%ld\n", best == zamd::kNoFit ? -1L : static_cast<long>(best));
    return 0;
  }
  if (what == "free" && argc == 6) {
    const zamd::FreeDecision d = zamd::DecideFree(Number(argv[2]), Number(argv[3]), Number(argv[4]), Number(argv[5]));
    std::printf("%d %d\n", d.trim_others ? 1 : 0, d.cache ? 1 : 0);
    return 0;
  }
  if (what == "pinned" && argc == 2) {
    std::printf("%zu %zu %zu\n", zamd::kPinnedMinBytes, zamd::kPinnedMaxCached, zamd::kPinnedMaxBytes);
    return 0;
  }
  if (what == "slots" && argc >= 8) {
    const zamd::SlotWish wish = {Number(argv[2]), Number(argv[3]), Number(argv[4]) != 0, Number(argv[5]) != 0,
                                 Number(argv[6]), Number(argv[7])};
    std::vector<zamd::DeviceSlots> devices;
    for (int a = 8; a < argc; ++a) {
      const char* colon = std::strchr(argv[a], ':');
      if (!colon) return 2;
      zamd::DeviceSlots dev = {std::atoi(argv[a]), colon > argv[a] && colon[-1] == '!', {}};
      for (const char* p = colon + 1; *p; ++p) {
        if (*p != 'f' && *p != 'b' && *p != 'n') return 2;
        dev.slots.push_back({*p != 'f', *p != 'n'});
      }
      devices.push_back(dev);
    }
    for (const zamd::SlotPick& p : zamd::ChooseSlots(devices, wish)) std::printf("%zu %zu %d\n", p.device, p.slot, p.create ? 1 : 0);
    return 0;
  }
  std::fprintf(stderr, "usage: pool_print fit device|pinned WANT CAPS | free DEVICE_CACHED OWN_CACHED CAP KEEP | pinned | "
                       "slots WANT PER_DEVICE SMALL MAY_CREATE_MORE LANES SMALL_LANES INDEX[!]:SLOTS...\n");
  return 2;
}
