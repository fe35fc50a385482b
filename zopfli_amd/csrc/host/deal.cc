#include "deal.h"

#include <algorithm>
#include <cstdint>

#include "zopfli_amd.h"

namespace zamd {

// What a kind of data costs relative to text, per byte (profiles/r05_classes.json: ms per 100 MB through ZopfliCompress,
// numiterations 15 — text 123, long runs of equal bytes ~ 4.6 x, two-symbol data 2.3 x; markup, PNG-like and random data
// within 30 % of text).  Long runs: the chain walks them as a few lone waves; few distinct bytes:
// hash chains at the 8192-hit cap.
static constexpr double kRunWeight = 3.6;      // added per byte that lies in a run of 64+ equal bytes
static constexpr double kFewWeight = 1.3;      // added per byte in a stretch of at most 4 distinct byte values (not a run)

double CostFromCounts(size_t bytes, size_t probes, size_t runs, size_t few) {
  if (bytes == 0) return 0.0;
  const double n = static_cast<double>(bytes) / 1e6;
  if (probes == 0) return n;
  return n * (1.0 + kRunWeight * static_cast<double>(runs) / static_cast<double>(probes) +
              kFewWeight * static_cast<double>(few) / static_cast<double>(probes));
}

bool RunsFromCounts(size_t probes, size_t hits) { return probes > 0 && hits * 100 >= probes; }

double MasterBlockCost(const unsigned char* in, size_t begin, size_t end) {
  if (end <= begin) return 0.0;
  size_t probes = 0, runs = 0, few = 0;
  for (size_t i = begin; i + 64 <= end; i += 1024, ++probes) {
    const unsigned char c0 = in[i];
    size_t k = 1;
    while (k < 64 && in[i + k] == c0) ++k;
    if (k == 64) { ++runs; continue; }
    uint64_t seen[4] = {0, 0, 0, 0};
    unsigned distinct = 0;
    for (size_t j = 0; j < 64 && distinct <= 4; ++j) {
      const unsigned char c = in[i + j];
      const uint64_t bit = 1ull << (c & 63);
      if (!(seen[c >> 6] & bit)) { seen[c >> 6] |= bit; ++distinct; }
    }
    if (distinct <= 4) ++few;
  }
  return CostFromCounts(end - begin, probes, runs, few);
}

void DealByCost(const std::vector<double>& cost, size_t shards, std::vector<size_t>* first) {
  const size_t n = cost.size();
  if (shards == 0) shards = 1;
  first->assign(shards + 1, n);
  (*first)[0] = 0;
  double total = 0;
  for (double c : cost) total += c;
  // shard s ends where the running cost comes closest to its share of the total, but leaves a block for every shard
  // still to come (and takes at least one itself) while there are blocks to go round
  if (n <= shards) {      // a block each while they last; the shards at the end are empty
    for (size_t s = 0; s <= shards; ++s) (*first)[s] = s < n ? s : n;
    return;
  }
  size_t at = 0;
  double acc = 0;
  for (size_t s = 0; s + 1 < shards; ++s) {
    const double want = total * static_cast<double>(s + 1) / static_cast<double>(shards);
    const size_t left = shards - 1 - s;                                   // shards after this one
    const size_t hi = std::max(at, n > left ? n - left : static_cast<size_t>(0));   // ... each of which gets a block if there is one
    const size_t lo = at < hi ? at + 1 : at;                              // and so does this one
    size_t to = at;
    while (to < hi && (to < lo || acc + cost[to] * 0.5 <= want)) {        // a block goes to the side its midpoint lies on
      acc += cost[to];
      ++to;
    }
    (*first)[s + 1] = to;
    at = to;
  }
  (*first)[shards] = n;
}

bool LooksLikeRuns(const unsigned char* in, size_t lo, size_t hi) {
  size_t probes = 0, hits = 0;
  for (size_t i = lo; i + 64 <= hi; i += 4096, ++probes) {
    const unsigned char c0 = in[i];
    size_t k = 1;
    while (k < 64 && in[i + k] == c0) ++k;
    hits += k == 64;
  }
  return RunsFromCounts(probes, hits);
}

std::vector<size_t> ShardRanges(size_t nparts, size_t ndev, const double* cost, const std::vector<double>& weights) {
  std::vector<size_t> first(ndev + 1);
  for (size_t d = 0; d <= ndev; ++d) first[d] = nparts * d / ndev;
  if (cost) DealByCost(std::vector<double>(cost, cost + nparts), ndev, &first);
  double total = 0;
  for (size_t d = 0; d < ndev && d < weights.size(); ++d) total += weights[d];
  if (weights.size() >= ndev && total > 0) {
    double acc = 0;
    size_t at = 0;
    for (size_t d = 0; d < ndev; ++d) {
      acc += weights[d];
      size_t to = d + 1 == ndev ? nparts : static_cast<size_t>(nparts * acc / total + 0.5);
      to = std::max(to, at + 1);                       // no empty shard
      to = std::min(to, nparts - (ndev - 1 - d));
      first[d] = at;
      first[d + 1] = to;
      at = to;
    }
  }
  return first;
}

std::vector<int> ShardPriorities(const std::vector<int>& device_of) {
  const size_t ndev = device_of.size();
  std::vector<int> priority(ndev, 0);
  for (size_t d = 0; d < ndev; ++d) {
    size_t before = 0, same = 0;
    for (size_t e = 0; e < ndev; ++e) {
      if (device_of[e] != device_of[d]) continue;
      ++same;
      if (e < d) ++before;
    }
    if (same > 1) priority[d] = before == 0 ? 1 : before + 1 == same ? -1 : 0;
  }
  return priority;
}

std::vector<long> UploadAfter(const std::vector<int>& device_of) {
  std::vector<long> after(device_of.size(), -1);
  for (size_t d = 1; d < device_of.size(); ++d) {
    for (size_t e = d; e-- > 0;) {
      if (device_of[e] == device_of[d]) { after[d] = static_cast<long>(e); break; }
    }
  }
  return after;
}

std::vector<SlotPick> ChooseSlots(const std::vector<DeviceSlots>& devices, const SlotWish& wish) {
  std::vector<SlotPick> picks;
  size_t used_devices = 0;
  for (size_t d = 0; d < devices.size() && used_devices != wish.want; ++d) {
    const DeviceSlots& dev = devices[d];
    if (dev.dead) continue;
    size_t next = 0;                    // the existing slots before it are busy or picked
    size_t total = dev.slots.size();    // ... with the new ones of this answer
    size_t here = 0;
    for (size_t lane = 0; lane < wish.per_device; ++lane, ++here) {
      while (next < dev.slots.size() && dev.slots[next].busy) ++next;
      if (next < dev.slots.size()) {
        picks.push_back({d, next, !dev.slots[next].created});
        ++next;
        continue;
      }
      const bool room = total < wish.lanes || (wish.small && wish.per_device == 1 && total < wish.small_lanes);
      if (!room || !(wish.may_create_more || lane == 0)) break;
      picks.push_back({d, total++, true});
    }
    if (here) ++used_devices;
  }
  return picks;
}

}  // namespace zamd

extern "C" {

// include/zopfli_amd.h
int zmx_master_block_costs(const unsigned char* in, size_t insize, double* cost, size_t ncost) {
  const size_t kMb = 1000000;   // ZOPFLI_MASTER_BLOCK_SIZE, util.h:60
  const size_t n = insize == 0 ? 1 : (insize + kMb - 1) / kMb;
  if (ncost < n) return -1;
  for (size_t b = 0; b < n; ++b) cost[b] = zamd::MasterBlockCost(in, b * kMb, std::min(insize, (b + 1) * kMb));
  return static_cast<int>(n > 0x7fffffff ? 0x7fffffff : n);
}

int zmx_deal_master_blocks(const double* cost, size_t nblocks, size_t shards, size_t* first) {
  if (shards == 0) return -1;
  std::vector<size_t> f;
  zamd::DealByCost(std::vector<double>(cost, cost + nblocks), shards, &f);
  for (size_t s = 0; s <= shards; ++s) first[s] = f[s];
  return 0;
}

}  // extern "C"
