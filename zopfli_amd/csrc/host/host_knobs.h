// The ZOPFLI_AMD_* switches of the host layer (api.cc, deflate.cc, block_split.cc, lz77_optimal.cc, block_cache.h,
// thread_pool.h), in one place: what each is and how its text is read.  Plain C++, no HIP (the device layer's table is
// device/zmx_knobs.h): tests/hostlib/knob_print.cc prints both.
//
// Two moments of reading.  The PROCESS switches (HostKnobs) are read together at the first use of any of them — never at
// load time: a caller may set them after loading the library and before its first call.  The POOL switches (PoolKnobs:
// which devices, how many contexts each) are read when the context pool is set up, at the first call that needs a
// context — a process may use the resident-input entry points first and name its devices afterwards.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace zamd {

struct HostKnobs {
  // --- what a call is cut into and dealt over (api.cc)
  long split_mb = -1;            // ZOPFLI_AMD_SPLIT_MB: master blocks from which a call takes SPLIT_WAYS contexts of a device; -1 (unset) = by the options, 0 = never; negative text = 0
  size_t split_ways = 3;         // ZOPFLI_AMD_SPLIT_WAYS: contexts of each device such a call is dealt over, at least 1
  bool split_runs = true;        // ZOPFLI_AMD_SPLIT_RUNS: 0 = data with long runs of equal bytes stays on one context
  int stream_prio = 1;           // ZOPFLI_AMD_STREAM_PRIO: 0 = the contexts of a device never at different stream priorities, 2 = always, 1 = where it pays
  bool small_prio = true;        // ZOPFLI_AMD_SMALL_PRIO: 0 = a one-shard call's context stays on the default priority
  bool upload_order = true;      // ZOPFLI_AMD_UPLOAD_ORDER: 0 = the contexts of a device upload all at once
  bool deal_by_cost = true;      // ZOPFLI_AMD_DEAL: "count" = shards of equal counts; anything else = of equal estimated cost
  std::vector<double> shard_weights;   // ZOPFLI_AMD_SHARD_WEIGHTS="28,36,36": the shards' shares (negative = 0; read up to the first text that is no number), for measuring
  size_t deal_after = 8;         // ZOPFLI_AMD_DEAL_AFTER: the polite call of the process from which further contexts are created; negative = 0
  size_t round_parts = 2000;     // ZOPFLI_AMD_ROUND_PARTS: master blocks a round of a call takes; <= 0 = 2000
  size_t parts_per_batch = 256;  // ZOPFLI_AMD_PARTS_PER_BATCH: parts a DeflateParts call takes; <= 0 = 256
  long test_fail_shard = -1;     // ZOPFLI_AMD_TEST_FAIL_SHARD=k: test hook, the k-th shard's first attempt fails
  int keep_heap = 0;             // ZOPFLI_AMD_KEEP_HEAP: 0 = malloc is left alone, 2 = large blocks from the heap too, anything else = no trimming
  // --- the phases of a DeflateParts call (deflate.cc, lz77_optimal.cc)
  int batch_split = -1;          // ZOPFLI_AMD_BATCH_SPLIT: 0 / non-zero force the split searches one by one / round by round together; negative or unset = by the number of parts
  int device_split = 1;          // ZOPFLI_AMD_DEVICE_SPLIT: 0 = the host evaluates every block size of the split search, 2 = the device wherever allowed, 1 = where it pays
  long device_split_from = -1;   // ZOPFLI_AMD_DEVICE_SPLIT_FROM: sequences from which the device may; negative or unset = the caller's default
  size_t device_split_min = 128; // ZOPFLI_AMD_DEVICE_SPLIT_MIN: block sizes a round needs to go to the device
  bool device_encode = true;     // ZOPFLI_AMD_DEVICE_ENCODE: 0 = every block's bits on the host
  bool verify = false;           // ZOPFLI_AMD_VERIFY: ZopfliVerifyLenDist on the device for every parse that is kept
  // --- reports on stderr
  bool trace_call = false;       // ZOPFLI_AMD_TRACE_CALL: where a call's wall time goes, per shard and per phase
  bool prof = false;             // ZOPFLI_AMD_PROF (set at all): phase times per DeflateParts call, split-cost evaluations
  // --- host resources (thread_pool.h, block_cache.h)
  unsigned threads = 0;          // ZOPFLI_AMD_THREADS: threads of the regular pool; 0 (unset or not positive) = by the CPUs
  bool threads_set = false;      // ZOPFLI_AMD_THREADS is set at all: the wide pool is as wide as the regular one
  unsigned wide_threads = 0;     // ZOPFLI_AMD_WIDE_THREADS: threads of the wide pool, for measuring; 0 = by THREADS or the CPUs
  size_t host_cache_mb = 1024;   // ZOPFLI_AMD_HOST_CACHE_MB: budget of the host block cache; <= 0 = no caching
  size_t host_cache_min = 32u << 10;   // ZOPFLI_AMD_HOST_CACHE_MIN: bytes below which a request is malloc's; at least 1024
};

// `get` is getenv or a stand-in for it: const char* get(const char* name), null when the variable is not set.
template <typename GetEnv>
HostKnobs ParseHostKnobs(GetEnv get) {
  auto integer = [&](const char* name, long dflt) { const char* e = get(name); return e ? std::atol(e) : dflt; };
  auto unless_zero = [&](const char* name) { const char* e = get(name); return !e || std::atoi(e) != 0; };   // default on
  auto non_zero = [&](const char* name) { const char* e = get(name); return e && std::atoi(e) != 0; };        // default off
  auto positive = [&](const char* name, size_t dflt) {
    const long v = integer(name, 0);
    return v > 0 ? static_cast<size_t>(v) : dflt;
  };
  HostKnobs k;
  if (const char* e = get("ZOPFLI_AMD_SPLIT_MB")) k.split_mb = std::max(0, std::atoi(e));
  if (const char* e = get("ZOPFLI_AMD_SPLIT_WAYS")) k.split_ways = static_cast<size_t>(std::max(1, std::atoi(e)));
  k.split_runs = unless_zero("ZOPFLI_AMD_SPLIT_RUNS");
  k.stream_prio = static_cast<int>(integer("ZOPFLI_AMD_STREAM_PRIO", 1));
  k.small_prio = unless_zero("ZOPFLI_AMD_SMALL_PRIO");
  k.upload_order = unless_zero("ZOPFLI_AMD_UPLOAD_ORDER");
  if (const char* e = get("ZOPFLI_AMD_DEAL")) k.deal_by_cost = std::strcmp(e, "count") != 0;
  if (const char* e = get("ZOPFLI_AMD_SHARD_WEIGHTS")) {
    for (const char* q = e; *q;) {
      char* end = nullptr;
      const double v = std::strtod(q, &end);
      if (end == q) break;
      k.shard_weights.push_back(v > 0 ? v : 0);
      q = *end == ',' ? end + 1 : end;
    }
  }
  if (const char* e = get("ZOPFLI_AMD_DEAL_AFTER")) k.deal_after = static_cast<size_t>(std::max(0, std::atoi(e)));
  k.round_parts = positive("ZOPFLI_AMD_ROUND_PARTS", 2000);
  k.parts_per_batch = positive("ZOPFLI_AMD_PARTS_PER_BATCH", 256);   // ~40 MB of tables per 1 MB master block
  k.test_fail_shard = integer("ZOPFLI_AMD_TEST_FAIL_SHARD", -1);
  const int keep_heap = static_cast<int>(integer("ZOPFLI_AMD_KEEP_HEAP", 0));
  k.keep_heap = keep_heap == 0 || keep_heap == 2 ? keep_heap : 1;
  k.batch_split = static_cast<int>(integer("ZOPFLI_AMD_BATCH_SPLIT", -1));
  k.device_split = static_cast<int>(integer("ZOPFLI_AMD_DEVICE_SPLIT", 1));
  k.device_split_from = integer("ZOPFLI_AMD_DEVICE_SPLIT_FROM", -1);
  if (const char* e = get("ZOPFLI_AMD_DEVICE_SPLIT_MIN")) k.device_split_min = static_cast<size_t>(std::atoll(e));
  k.device_encode = unless_zero("ZOPFLI_AMD_DEVICE_ENCODE");
  k.verify = non_zero("ZOPFLI_AMD_VERIFY");
  k.trace_call = non_zero("ZOPFLI_AMD_TRACE_CALL");
  k.prof = get("ZOPFLI_AMD_PROF") != nullptr;
  k.threads = static_cast<unsigned>(std::max(0, static_cast<int>(integer("ZOPFLI_AMD_THREADS", 0))));
  k.threads_set = get("ZOPFLI_AMD_THREADS") != nullptr;
  k.wide_threads = static_cast<unsigned>(std::max(0, static_cast<int>(integer("ZOPFLI_AMD_WIDE_THREADS", 0))));
  k.host_cache_mb = static_cast<size_t>(std::max(0l, integer("ZOPFLI_AMD_HOST_CACHE_MB", 1024)));
  k.host_cache_min = static_cast<size_t>(std::max(1l << 10, integer("ZOPFLI_AMD_HOST_CACHE_MIN", 32l << 10)));
  return k;
}

// The process's switches, read from the environment at the first use of any of them.
inline const HostKnobs& HostSwitches() {
  static const HostKnobs k = ParseHostKnobs([](const char* name) -> const char* { return std::getenv(name); });
  return k;
}

// Which devices the entry points' context pool takes, and how many contexts of each.
struct PoolKnobs {
  // ZOPFLI_AMD_DEVICES ("all", a count — "0" or no number: device 0 —, or a comma separated list of HIP device indices, an
  // index may repeat), else ZOPFLI_AMD_DEVICE, else LOCAL_RANK modulo the visible devices, else device 0.  As named: an
  // index that is not there is the pool's to refuse.
  std::vector<int> devices;
  size_t lanes = 3;              // ZOPFLI_AMD_LANES: contexts per device that calls are dealt over, at least 1
  size_t small_lanes = 16;       // ZOPFLI_AMD_SMALL_LANES: contexts per device that small calls may bring into being, at least LANES
};

template <typename GetEnv>
PoolKnobs ParsePoolKnobs(GetEnv get, int visible) {
  PoolKnobs k;
  std::vector<int>& list = k.devices;
  if (const char* e = get("ZOPFLI_AMD_DEVICES")) {
    if (std::strcmp(e, "all") == 0) {
      for (int i = 0; i < visible; ++i) list.push_back(i);
    } else if (std::strchr(e, ',')) {
      for (const char* p = e; *p;) {
        list.push_back(std::atoi(p));
        const char* q = std::strchr(p, ',');
        if (!q) break;
        p = q + 1;
      }
    } else {
      const int n = std::atoi(e);
      for (int i = 0; i < n && i < visible; ++i) list.push_back(i);
      if (list.empty()) list.push_back(0);   // ("0": no count — device 0)
    }
  } else if (const char* e = get("ZOPFLI_AMD_DEVICE")) {
    list.push_back(std::atoi(e));
  } else if (const char* r = get("LOCAL_RANK")) {
    // (one process per GPU under torchrun; with HIP_VISIBLE_DEVICES set per rank every rank sees ONE device and
    //  LOCAL_RANK = k would name a device that is not there: take it modulo what is visible)
    const int n = std::atoi(r);
    list.push_back(visible > 0 && n >= 0 ? n % visible : n);
  } else {
    list.push_back(0);
  }
  if (const char* e = get("ZOPFLI_AMD_LANES")) k.lanes = static_cast<size_t>(std::max(1, std::atoi(e)));
  if (const char* e = get("ZOPFLI_AMD_SMALL_LANES")) k.small_lanes = static_cast<size_t>(std::max(1, std::atoi(e)));
  k.small_lanes = std::max(k.small_lanes, k.lanes);
  return k;
}

// The pool's switches as the environment has them now, for `visible` HIP devices.
inline PoolKnobs PoolSwitches(int visible) {
  return ParsePoolKnobs([](const char* name) -> const char* { return std::getenv(name); }, visible);
}

}  // namespace zamd
