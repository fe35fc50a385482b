// The device memory of one context (zmx_ctx, drv_context.h): every array it holds on the device, the ones it keeps cached
// for the next batch, its pinned host buffers, and the red zones of ZOPFLI_AMD_GUARD.  A part of the driver that zmx_hip.hip
// lists, included after the error helpers (drv_errors.h: HIPCHK, FailFault) and the device switches (Knobs).  The rules — which cached block serves a request,
// what becomes of a block that is given back — are zmx_pool_rules.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

#include "zmx_pool_rules.h"
#include "zopfli_amd.h"

// ---------------------------------------------------------------------------------------------
// ZOPFLI_AMD_GUARD=1 — a debugging mode for the device allocations (round-2 verdict: an unexplained
// "Memory access fault by GPU" must be localisable).  Every pooled or direct allocation gets a red zone of
// kGuardBytes before and after it, filled with 0xA5; its body is filled with 0xCD whenever it is handed out
// (fresh or recycled: stale contents of an earlier batch cannot stand in for data a kernel forgot to write);
// after EVERY kernel launch the stream is drained and k_guard_check reads all red zones of the context: the
// first byte that changed is reported with the kernel that just ran, the allocation's tag and size, and the
// offset.  Slow (a synchronisation per launch); off by default.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr size_t kGuardBytes = 4096;
constexpr u32 kGuardMaxAllocs = 256;
bool GuardOn() { return Knobs().guard; }
}  // namespace

// zones[2 i], zones[2 i + 1] = device addresses of the two red zones of allocation i; res = {flag, alloc, offset, value}
__global__ __launch_bounds__(256) void k_guard_check(const u64* zones, u32 nzones, u32* res) {
  const u32 z = blockIdx.x;
  if (z >= nzones) return;
  const u32* q = reinterpret_cast<const u32*>(zones[z]);
  for (u32 i = threadIdx.x; i < kGuardBytes / 4; i += 256) {
    const u32 v = q[i];
    if (v != 0xa5a5a5a5u && atomicCAS(&res[0], 0u, 1u) == 0u) { res[1] = z; res[2] = i * 4; res[3] = v; }
  }
}

namespace {

// What the pools of ALL contexts of a device keep cached between batches, against ONE budget per device (a third of its
// memory): a lone busy context may cache all of it (100 MB of long runs are 52 GB of DP codes per batch; with a
// per-context third of a third they were hipFree'd and hipMalloc'ed every step: class Z 132 -> 49 MB/s), three busy
// ones share it, and idle ones are trimmed when another runs out (zmx_set_oom_hook).
constexpr int kMaxDevices = 64;
std::atomic<size_t> g_dev_cached[kMaxDevices];
std::atomic<zmx_oom_hook_t> g_oom_hook{nullptr};

// Table arrays are recycled between batches and calls: hipMalloc/hipFree of multi-GB arrays cost more than the kernels
// that fill them.  Not thread-safe: a context serves one call at a time.
class DevicePool {
 public:
  // `keep`: what the contexts of the device may keep cached between batches, together
  void Init(int device, size_t keep) { device_ = device; keep_ = keep; }

  // `bytes` of device memory (at least one), from the cache or from hipMalloc.  `tag` says who asks (guard mode's reports);
  // `stream` is where guard mode fills the red zones and the body.
  hipError_t Alloc(void** p, size_t bytes, const char* tag, hipStream_t stream) {
    if (bytes == 0) bytes = 1;
    const bool guard = GuardOn();
    const size_t want = guard ? ((bytes + 15) & ~static_cast<size_t>(15)) + 2 * kGuardBytes : bytes;
    const size_t best = zamd::BestFit(cached_, want, zamd::kDeviceFit);
    void* base = nullptr;
    size_t cap = want;
    if (best != zamd::kNoFit) {
      base = cached_[best].first;
      cap = cached_[best].second;
      cached_bytes_ -= cap;
      DeviceCached().fetch_sub(cap, std::memory_order_relaxed);
      cached_.erase(cached_.begin() + static_cast<long>(best));
      ++served_cached_;
    } else {
      hipError_t e = hipMalloc(&base, want);
      if (e != hipSuccess && !cached_.empty()) {  // out of memory: drop the cache and retry
        (void)hipGetLastError();
        DropCache();
        e = hipMalloc(&base, want);
      }
      if (e != hipSuccess) {
        // still out of memory: the idle contexts of the same device may sit on gigabytes of cached arrays (the owner
        // of the contexts — context_pool.h's ContextPool — trims them through this hook)
        if (const zmx_oom_hook_t hook = g_oom_hook.load(std::memory_order_acquire)) {
          (void)hipGetLastError();
          hook(device_);
          e = hipMalloc(&base, want);
        }
      }
      if (e != hipSuccess) return e;
      ++served_fresh_;
    }
    *p = base;
    if (guard) {
      const hipError_t e = GuardDress(base, bytes, cap, tag, stream, p);
      if (e != hipSuccess) return e;
    }
    live_[*p] = cap;
    return hipSuccess;
  }

  // Gives a block back: to the cache while the device's budget lasts, else to the device.  (A pointer that is not the
  // pool's goes to hipFree.)
  void Free(void* p) {
    if (!p) return;
    void* base = p;
    auto it = live_.find(p);
    if (it != live_.end()) {
      const size_t cap = it->second;
      live_.erase(it);
      if (guard_live_.erase(p)) base = static_cast<unsigned char*>(p) - kGuardBytes;
      zamd::FreeDecision d = zamd::DecideFree(DeviceCached().load(std::memory_order_relaxed), cached_bytes_, cap, keep_);
      if (d.trim_others) {
        if (const zmx_oom_hook_t hook = g_oom_hook.load(std::memory_order_acquire)) hook(device_);
        d = zamd::DecideFree(DeviceCached().load(std::memory_order_relaxed), cached_bytes_, cap, keep_);
      }
      if (d.cache) {
        cached_.emplace_back(base, cap);
        cached_bytes_ += cap;
        DeviceCached().fetch_add(cap, std::memory_order_relaxed);
        return;
      }
    }
    (void)hipFree(base);
  }

  // The cached blocks go back to the device (the live ones stay).
  void DropCache() {
    for (auto& f : cached_) (void)hipFree(f.first);
    cached_.clear();
    DeviceCached().fetch_sub(cached_bytes_, std::memory_order_relaxed);
    cached_bytes_ = 0;
  }

  // Everything goes back, the live blocks included (the context is being destroyed).
  void ReleaseAll() {
    for (auto& f : pinned_) (void)hipHostFree(f.first);
    pinned_.clear();
    DropCache();
    // (in guard mode the caller's pointer lies behind a red zone)
    for (auto& f : live_) (void)hipFree(guard_live_.count(f.first) ? static_cast<unsigned char*>(f.first) - kGuardBytes : f.first);
    live_.clear();
    guard_live_.clear();
    (void)hipFree(d_guard_tab_);
    d_guard_tab_ = nullptr;
  }

  // Pinned host buffers (a table set's h_runin / h_runout: a few KB per block), kept for the next set: hipHostMalloc +
  // hipHostFree were ~ 0.4 ms of every table set, a tenth of a small call's fixed cost.
  hipError_t PinnedTake(unsigned char** p, size_t bytes, size_t* cap) {
    const size_t best = zamd::BestFit(pinned_, bytes, zamd::kPinnedFit);
    if (best != zamd::kNoFit) {
      *p = static_cast<unsigned char*>(pinned_[best].first);
      *cap = pinned_[best].second;
      pinned_.erase(pinned_.begin() + static_cast<long>(best));
      return hipSuccess;
    }
    *cap = std::max(bytes, zamd::kPinnedMinBytes);
    return hipHostMalloc(reinterpret_cast<void**>(p), *cap, hipHostMallocDefault);
  }
  void PinnedGive(unsigned char* p, size_t cap) {
    if (pinned_.size() < zamd::kPinnedMaxCached && cap <= zamd::kPinnedMaxBytes) pinned_.emplace_back(p, cap);
    else (void)hipHostFree(p);
  }

  // Guard mode: drain `stream` and check every red zone of the context.  `where` = the kernel that just ran.
  int GuardVerify(hipStream_t stream, const char* where) {
    if (hipStreamSynchronize(stream) != hipSuccess) return FailFault(std::string("ZOPFLI_AMD_GUARD: the stream failed after ") + where);
    if (guard_live_.empty()) return 0;
    // (ZOPFLI_AMD_GUARD_SELFTEST=N: the N-th check finds a byte that this function itself just broke — the test that the
    //  mode reports what it is there to report)
    const u64 selftest = Knobs().guard_selftest;
    std::vector<std::pair<void*, GuardInfo>> live(guard_live_.begin(), guard_live_.end());
    if (!d_guard_tab_) HIPCHK(hipMalloc(reinterpret_cast<void**>(&d_guard_tab_), (2 * static_cast<size_t>(kGuardMaxAllocs) + 2) * sizeof(u64)));
    ++guard_checks_;
    // every live allocation, kGuardMaxAllocs at a time (a context that holds parent, optimal and fixed-tree tables plus
    // temporaries has more than one table's worth)
    for (size_t first = 0; first < live.size(); first += kGuardMaxAllocs) {
      const u32 n = static_cast<u32>(std::min<size_t>(live.size() - first, kGuardMaxAllocs));
      std::vector<u64> tab(2 * static_cast<size_t>(kGuardMaxAllocs) + 2, 0);
      for (u32 i = 0; i < n; ++i) {
        const unsigned char* user = static_cast<const unsigned char*>(live[first + i].first);
        tab[2 * i] = reinterpret_cast<u64>(user - kGuardBytes);
        tab[2 * i + 1] = reinterpret_cast<u64>(user + live[first + i].second.bytes);
      }
      if (first == 0 && selftest && guard_checks_ == selftest) HIPCHK(hipMemset(reinterpret_cast<void*>(tab[1] + 100), 0x5a, 1));
      HIPCHK(hipMemcpy(d_guard_tab_, tab.data(), tab.size() * sizeof(u64), hipMemcpyHostToDevice));   // (the result words zeroed with it)
      u32* res = reinterpret_cast<u32*>(d_guard_tab_ + 2 * static_cast<size_t>(kGuardMaxAllocs));
      hipLaunchKernelGGL(k_guard_check, dim3(2 * n), dim3(256), 0, stream, d_guard_tab_, 2 * n, res);
      HIPCHK(hipGetLastError());
      u32 h[4] = {0, 0, 0, 0};
      HIPCHK(hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost));
      if (h[0] == 0) continue;
      const auto& g = live[first + (h[1] >> 1)].second;
      char buf[400];
      std::snprintf(buf, sizeof(buf), "ZOPFLI_AMD_GUARD: after %s the red zone %s allocation '%s' (%zu bytes) changed: byte offset %u of the zone holds 0x%08x",
                    where, (h[1] & 1u) ? "behind" : "in front of", g.tag ? g.tag : "?", g.bytes, h[2], h[3]);
      std::fprintf(stderr, "%s\n", buf);
      return FailFault(buf);
    }
    return 0;
  }

  // zmx_internal_pool_stats: live allocations and their bytes, cached blocks and their bytes, what all contexts of the
  // device keep cached, cached pinned buffers, allocations served by hipMalloc and from the cache since Init
  void Stats(uint64_t out[8]) const {
    uint64_t live_bytes = 0;
    for (auto& f : live_) live_bytes += f.second;
    out[0] = live_.size();
    out[1] = live_bytes;
    out[2] = cached_.size();
    out[3] = cached_bytes_;
    out[4] = DeviceCached().load(std::memory_order_relaxed);
    out[5] = pinned_.size();
    out[6] = served_fresh_;
    out[7] = served_cached_;
  }

  static void SetOomHook(zmx_oom_hook_t hook) { g_oom_hook.store(hook, std::memory_order_release); }

 private:
  struct GuardInfo { size_t bytes; const char* tag; };   // the bytes the caller asked for and who asked
  std::atomic<size_t>& DeviceCached() const { return g_dev_cached[device_ >= 0 && device_ < kMaxDevices ? device_ : 0]; }

  // The red zones and the poison of an allocation that is being handed out (guard mode): base = what hipMalloc
  // returned, the caller gets base + kGuardBytes.
  hipError_t GuardDress(void* base, size_t bytes, size_t cap, const char* tag, hipStream_t stream, void** user) {
    unsigned char* b = static_cast<unsigned char*>(base);
    const size_t body = (bytes + 15) & ~static_cast<size_t>(15);
    hipError_t e = hipMemsetAsync(b, 0xa5, kGuardBytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(b + kGuardBytes, 0xcd, cap - 2 * kGuardBytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(b + kGuardBytes + body, 0xa5, kGuardBytes, stream);
    *user = b + kGuardBytes;
    guard_live_[*user] = GuardInfo{body, tag};
    return e;
  }

  int device_ = 0;
  size_t keep_ = 0;
  std::unordered_map<void*, size_t> live_;             // what the caller holds -> capacity
  zamd::CachedBlocks cached_;                          // base addresses (guard mode: of the front red zone)
  size_t cached_bytes_ = 0;
  zamd::CachedBlocks pinned_;
  std::unordered_map<void*, GuardInfo> guard_live_;    // guard mode, keyed like live_
  u64* d_guard_tab_ = nullptr;   // [kGuardMaxAllocs][2] zone pairs for k_guard_check, then 4 result words
  u64 guard_checks_ = 0;
  uint64_t served_fresh_ = 0, served_cached_ = 0;
};

}  // namespace
