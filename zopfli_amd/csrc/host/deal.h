// Cost-aware dealing of master blocks (deflate.c:916-923 is the unit: master blocks are independent).
//
// A master block of long runs of equal bytes costs several times a master block of text ("Per
// class"): contiguous equal-COUNT shards put a mixed corpus's expensive stretches on one or two ranks.  The shards
// are therefore balanced by an estimate of each master block's cost that is a function of the BYTES alone — every
// rank, and the in-process dealer, compute the same ranges from the same input; nothing is measured, nothing is
// exchanged.
#pragma once
#include <cstddef>
#include <vector>

namespace zamd {

// Cost of compressing in[begin, end) relative to the same number of bytes of text (1.0 per 1 000 000 bytes), from
// probes of 64 bytes every 1024.
double MasterBlockCost(const unsigned char* in, size_t begin, size_t end);
// ... from its counts: `probes` probes over `bytes` bytes, of which `runs` found 64 equal bytes and `few` at most 4
// distinct values.  MasterBlockCost ends here, and so do counts taken on the device (device/zmx_probe.h).
double CostFromCounts(size_t bytes, size_t probes, size_t runs, size_t few);

// first[s] .. first[s + 1]: the blocks of shard s — contiguous, in order, none empty while blocks >= shards, the
// largest shard's cost as small as a prefix walk makes it.  `first` gets shards + 1 entries.
void DealByCost(const std::vector<double>& cost, size_t shards, std::vector<size_t>* first);

// The plan of a call that is dealt over several contexts (api.cc: RunPartsShardedOnce).  Functions of their arguments
// alone: no context, no environment.

// Data with long runs of equal bytes?  Sampled: one probe every 4096 bytes of in[lo, hi), "the next 64 bytes are equal";
// 1 % of the probes make a call "data with runs".
bool LooksLikeRuns(const unsigned char* in, size_t lo, size_t hi);
// ... from its counts: `hits` of `probes` probes found 64 equal bytes
bool RunsFromCounts(size_t probes, size_t hits);

// first[s] .. first[s + 1]: the parts of shard s of `ndev` (at most `nparts`), contiguous and none empty: equal counts;
// of equal cost (DealByCost) where `cost` — nparts entries — is given; `weights` (ZOPFLI_AMD_SHARD_WEIGHTS), when there is
// one for every shard and their sum is positive, override both with their shares.
std::vector<size_t> ShardRanges(size_t nparts, size_t ndev, const double* cost, const std::vector<double>& weights);

// The stream priorities of shards whose contexts lie on the devices `device_of`: the contexts of ONE device run at three
// levels — its first shard 1, its last -1, those between 0; a device with a single shard stays at 0.
std::vector<int> ShardPriorities(const std::vector<int>& device_of);

// The shard whose upload each shard waits for: the one before it on the same device, -1 = none.
std::vector<long> UploadAfter(const std::vector<int>& device_of);

// Which contexts a call takes (context_pool.h: ContextPool::Acquire), as a function of a snapshot of the pool.  A device
// has slots, each with one context or waiting for its own to be made.
struct SlotState { bool busy, created; };
struct DeviceSlots { int index; bool dead; std::vector<SlotState> slots; };
struct SlotWish {
  size_t want;            // devices (each with at least one slot)
  size_t per_device;      // free slots of every device the call uses, at most
  bool small;             // the call may bring a slot beyond `lanes` into being rather than wait
  bool may_create_more;   // false: only a device's first slot of this call may be a new one
  size_t lanes;           // slots per device
  size_t small_lanes;     // ... with those that `small` calls add
};
// `slot` of the device at position `device` of the snapshot; slot >= its slots.size(): a new slot, to be appended.
// `create`: the slot has no context yet.
struct SlotPick { size_t device, slot; bool create; };
// In device order, a device's existing free slots before its new ones; empty when everything is busy and nothing may be
// made.  Dead devices are skipped.  A `small` call with per_device 1 fills the FIRST live device up to small_lanes before
// it looks at the next one (ADVICE.md item 1 argues against that; the policy is kept as it is here).
std::vector<SlotPick> ChooseSlots(const std::vector<DeviceSlots>& devices, const SlotWish& wish);

}  // namespace zamd
