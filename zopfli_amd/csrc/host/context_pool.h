// The device contexts of the Zopfli* entry points (api.cc).
//
// Which devices: ONE by default — ZOPFLI_AMD_DEVICE, else LOCAL_RANK (one process per GPU under torchrun), else
// device 0: a program that links libzopfli.so.1 must not find itself holding every GPU of the node.  Several only
// when asked: ZOPFLI_AMD_DEVICES = "all", a count, or a comma separated list of HIP device indices (an index may
// repeat: two contexts on one device, which is how the multi-device path is exercised on a one-GPU box); master
// blocks are independent (deflate.c:916-923), so a request with several of them is dealt across those devices.
//
// Re-entrancy (the reference has no globals: callers may run concurrent calls on distinct buffers): a
// device has up to ZOPFLI_AMD_LANES contexts (default 3), created when first needed; a request takes one free
// context on each device it uses and gives them back when it is done, so callers overlap — one's host phases
// (cost models, block splitting, merging) with the others' kernels — and a fourth waits.  A device whose context
// cannot be created (not gfx950, out of memory) is dropped from the list; only when none is left does the call die.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "deal.h"
#include "host_knobs.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"

namespace zamd {

// (api.cc)
[[noreturn]] void Die(const char* what);
void MaybeKeepHeap();

class ContextPool {
 public:
  // one free context on each of up to `want` devices (at least one), in device order; with `per_device` > 1 up to
  // that many free contexts of every device it uses (a large request on one device is dealt over two of its
  // contexts: one half's host phases run beside the other half's kernels)
  // `polite`: a call that is not large takes several contexts of a device only while it is the only caller — with other
  // calls in flight (holding contexts or waiting for one) it takes one, as every call below the dealing threshold does.
  // `small`: a call below the 32 master blocks from which calls are dealt whatever else runs (small files — what zopfli is
  // mostly used on — and the medium calls that, alone, politely take all three dealing contexts: a second such caller
  // no longer waits for the first to finish).  When every context of its
  // device is busy such a call gets a context of its own beyond the ZOPFLI_AMD_LANES of the dealing — up to
  // ZOPFLI_AMD_SMALL_LANES (16) per device — instead of waiting: sixteen callers with 64 KiB files keep eight streams of
  // small kernels and eight host threads' split searches going, where three contexts left thirteen of them waiting.
  // Which slots that makes is ChooseSlots (deal.h).
  // `only_device` >= 0: contexts of that HIP device alone (a call whose output stays in that device's memory); empty when
  // it is not one of the pool's live devices.
  std::vector<zmx_ctx*> Acquire(size_t want, size_t per_device = 1, std::vector<int>* device_of = nullptr,
                                bool polite = false, bool small = false, int only_device = -1) {
    std::unique_lock<std::mutex> lock(mu_);
    Init();
    ++in_flight_;
    // ... and it does not CREATE the further contexts before the eighth such call of the process (ZOPFLI_AMD_DEAL_AFTER):
    // a context costs ~ 50 ms to set up and saves such a call 5 - 15 ms, which a program that compresses a few files
    // and exits never earns back (zopflipng on one 1024 x 1024 image: 0.62 -> 0.70 s when its calls set up two more
    // contexts); a long-lived caller pays once.  (The first context a call takes is created whenever none is free.)
    const bool may_create_more = !polite || per_device <= 1 || ++polite_wishes_ >= HostSwitches().deal_after;
    for (;;) {
      if (polite && in_flight_ > 1) per_device = 1;
      std::vector<DeviceSlots> snap = Snapshot();
      if (only_device >= 0) {
        bool found = false;
        for (DeviceSlots& d : snap) {
          if (d.index != only_device) d.dead = true;
          found |= !d.dead;
        }
        if (!found) return {};   // (the call counts as in flight until its Release, like any other)
      }
      std::vector<Slot*> slots = Take(ChooseSlots(snap, {want, per_device, small, may_create_more, lanes_, small_lanes_}));
      CreateMissing(&lock, &slots);
      bool any_alive = false;
      for (auto& dev : devices_) any_alive |= !dev.dead;
      if (!any_alive) Die("no usable gfx950 device (there is no CPU fallback)");
      if (!slots.empty()) {
        std::vector<zmx_ctx*> got;
        for (Slot* s : slots) got.push_back(s->ctx);
        if (device_of) {
          device_of->clear();
          for (Slot* s : slots) device_of->push_back(s->dev->index);
        }
        return got;
      }
      cv_.wait(lock);   // every context of every device is busy
    }
  }
  // zmx_set_oom_hook: a context of `device` is out of memory even after dropping its own cache — the idle contexts of
  // that device give their cached arrays back
  void TrimIdle(int device) {
    // hipFree synchronises the device: not under the pool's lock (every Acquire / Release would wait behind it).  The
    // idle contexts are taken out of circulation, trimmed, and put back.
    std::vector<Slot*> mine;
    {
      std::lock_guard<std::mutex> lock(mu_);
      for (auto& dev : devices_) {
        if (dev.index != device) continue;
        for (auto& sl : dev.slots) if (!sl->busy && sl->ctx) { sl->busy = true; mine.push_back(sl.get()); }
      }
    }
    if (mine.empty()) return;
    for (Slot* sl : mine) zmx_ctx_trim_cache(sl->ctx);
    {
      std::lock_guard<std::mutex> lock(mu_);
      for (Slot* sl : mine) sl->busy = false;
    }
    cv_.notify_all();
  }
  size_t InFlight() {
    std::lock_guard<std::mutex> lock(mu_);
    return in_flight_;
  }
  void Release(const std::vector<zmx_ctx*>& ctxs) {
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (in_flight_) --in_flight_;
      for (auto& dev : devices_)
        for (auto& sl : dev.slots)
          if (std::find(ctxs.begin(), ctxs.end(), sl->ctx) != ctxs.end()) sl->busy = false;
    }
    cv_.notify_all();
  }

 private:
  struct Device;
  struct Slot { zmx_ctx* ctx; bool busy; Device* dev; };
  struct Device { int index; bool dead = false; std::vector<std::unique_ptr<Slot>> slots; };
  void Init() {
    if (!devices_.empty()) return;
    MaybeKeepHeap();
    const int visible = zmx_device_count();
    const PoolKnobs knobs = PoolSwitches(visible);
    for (int d : knobs.devices) {
      if (d < 0 || d >= visible) {
        std::fprintf(stderr, "zopfli_amd: no HIP device %d (%d visible): ignored\n", d, visible);
        continue;
      }
      Device dev;
      dev.index = d;
      devices_.push_back(std::move(dev));
    }
    if (devices_.empty()) {
      zmx_internal_set_error("no HIP device to run on", ZMX_ERR_DEVICE);
      Die("no usable gfx950 device (there is no CPU fallback)");
    }
    lanes_ = knobs.lanes;
    small_lanes_ = knobs.small_lanes;
    zmx_set_oom_hook(&ContextPool::OomHook);
  }
  // what ChooseSlots sees of the pool (under the lock)
  std::vector<DeviceSlots> Snapshot() const {
    std::vector<DeviceSlots> snap;
    for (auto& dev : devices_) {
      snap.push_back({dev.index, dev.dead, {}});
      for (auto& sl : dev.slots) snap.back().slots.push_back({sl->busy, sl->ctx != nullptr});
    }
    return snap;
  }
  // The picked slots, now busy (under the lock).  A new context's slot is taken here; the context itself is made by
  // CreateMissing.
  std::vector<Slot*> Take(const std::vector<SlotPick>& picks) {
    std::vector<Slot*> slots;
    for (const SlotPick& p : picks) {
      Device& dev = devices_[p.device];
      if (p.slot == dev.slots.size()) dev.slots.emplace_back(new Slot{nullptr, false, &dev});
      dev.slots[p.slot]->busy = true;
      slots.push_back(dev.slots[p.slot].get());
    }
    return slots;
  }
  // Makes the contexts that `slots` lack, without the pool's lock (HIP start-up, streams, events: up to seconds on first
  // use, and every Release would wait behind it).  A slot whose context cannot be made leaves `slots` and its device; a
  // device that is left without slots is dead.
  void CreateMissing(std::unique_lock<std::mutex>* lock, std::vector<Slot*>* slots) {
    bool missing = false;
    for (Slot* s : *slots) missing |= s->ctx == nullptr;
    if (!missing) return;
    lock->unlock();
    std::vector<std::pair<Slot*, zmx_ctx*>> made;
    std::vector<std::pair<Slot*, std::string>> failed;
    for (Slot* s : *slots) {
      if (s->ctx) continue;
      zmx_ctx* c = nullptr;
      if (zmx_ctx_create(s->dev->index, &c) != 0) failed.emplace_back(s, zmx_last_error());
      else made.emplace_back(s, c);
    }
    lock->lock();
    for (auto& m : made) m.first->ctx = m.second;
    for (auto& f : failed) {
      Device* dev = f.first->dev;
      for (size_t i = 0; i < dev->slots.size(); ++i) {
        if (dev->slots[i].get() == f.first) { dev->slots.erase(dev->slots.begin() + static_cast<long>(i)); break; }
      }
      slots->erase(std::find(slots->begin(), slots->end(), f.first));
      if (dev->slots.empty()) {
        std::fprintf(stderr, "zopfli_amd: device %d is not usable: %s\n", dev->index, f.second.c_str());
        dev->dead = true;
      }
    }
    if (!failed.empty()) cv_.notify_all();
  }
  static void OomHook(int device);
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Device> devices_;
  size_t lanes_ = 3;
  size_t small_lanes_ = 16;  // contexts per device that calls of one or two master blocks may bring into being (1000 x 64 KiB through 16 callers: 8.9 MB/s with 3, 20.4 with 8, 27.7 with 16; profiles/r06_small_files.txt)
  size_t in_flight_ = 0;     // calls between Acquire and Release
  size_t polite_wishes_ = 0; // polite calls so far that asked for more than one context of a device
};

inline ContextPool& Pool() {
  static ContextPool* pool = new ContextPool();   // (never destroyed: HIP may be gone by the time statics are)
  return *pool;
}
inline void ContextPool::OomHook(int device) { Pool().TrimIdle(device); }

struct Lease {
  std::vector<int> device_of;      // HIP device index of ctxs[i]
  std::vector<zmx_ctx*> ctxs;
  explicit Lease(size_t want, size_t per_device = 1, bool polite = false, bool small = false, int only_device = -1)
      : ctxs(Pool().Acquire(want, per_device, &device_of, polite, small, only_device)) {}
  ~Lease() { Pool().Release(ctxs); }
};

}  // namespace zamd
