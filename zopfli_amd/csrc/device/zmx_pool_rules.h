// The rules of a context's memory pool (zmx_pool.h), as functions of their arguments alone: which cached block serves a
// request, and what becomes of a block that is given back.  Host only — no HIP here, so that tests/hostlib/pool_print.cc
// compiles it with plain g++.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

namespace zamd {

// Blocks that wait to be handed out again: address and capacity in bytes.
using CachedBlocks = std::vector<std::pair<void*, size_t>>;

// A cached block of `cap` bytes serves a request for `want` when want <= cap <= mul * want + add: a much larger block
// would be kept from the request it fits.
struct FitBound { size_t mul, add; };
constexpr FitBound kDeviceFit = {2, size_t{1} << 20};   // table arrays: up to 2 * want + 1 MiB
constexpr FitBound kPinnedFit = {4, 4096};              // pinned buffers: up to 4 * bytes + 4096

constexpr size_t kNoFit = ~size_t{0};
// The smallest block of `blocks` that serves `want` within `bound` (the first of equals): its index, or kNoFit.
inline size_t BestFit(const CachedBlocks& blocks, size_t want, FitBound bound) {
  size_t best = kNoFit;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const size_t cap = blocks[i].second;
    if (cap >= want && cap <= bound.mul * want + bound.add && (best == kNoFit || cap < blocks[best].second)) best = i;
  }
  return best;
}

// A pinned buffer has at least kPinnedMinBytes; a context keeps at most kPinnedMaxCached of them, none above
// kPinnedMaxBytes.
constexpr size_t kPinnedMinBytes = 4096;
constexpr size_t kPinnedMaxCached = 8;
constexpr size_t kPinnedMaxBytes = size_t{64} << 20;

// What becomes of a device block of `cap` bytes that its context gives back.  `device_cached`: what ALL contexts of the
// device keep cached, `own_cached`: this context's part of it, `keep`: the device's budget.
//   trim_others: the budget is used up and some of it is ANOTHER context's — the idle contexts' caches go first (the
//     context that is working is the one whose arrays will be asked for again), and the question is put once more with
//     the device's new total.  Not when the cache is all this context's own: the owner of the contexts would take its
//     lock and find nothing, on every free of the hot path.
//   cache: the block fits the budget and is kept; otherwise it goes back to the device.
struct FreeDecision { bool trim_others, cache; };
inline FreeDecision DecideFree(size_t device_cached, size_t own_cached, size_t cap, size_t keep) {
  return {device_cached + cap > keep && device_cached > own_cached, device_cached + cap <= keep};
}

}  // namespace zamd
