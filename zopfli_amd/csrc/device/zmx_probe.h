// What the host used to read of the input's bytes itself, for an input that lives in device memory only
// (zmx_set_input_device, zmx_compress_device):
//   k_probe_counts  the integer counts behind zamd::MasterBlockCost and zamd::LooksLikeRuns (host/deal.cc) of a list of
//                   ranges; the doubles come from the counts on the host (zamd::CostFromCounts, zamd::RunsFromCounts)
//   k_tail_runs     per block, where the run of bytes equal to its last byte begins (PlanReuse, drv_build.h)
// and, beside them, the parity probe of whole match tables:
//   k_rec_digest    two 64-bit sums over the logical content of every match record (zmx_match_digest, drv_probes.h)
// The rules are __host__ __device__ functions, so a CPU program (tests/hostlib/probe_print.cc) runs the very code of
// the kernels against the host's own loops in deal.cc; PlanReuse walks a host input with TailRunStart.  This header compiles without HIP; the kernels are there for the device layer only (ZMX_PROBE_KERNELS).
#ifndef ZMX_PROBE_H_
#define ZMX_PROBE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define ZMX_HD __host__ __device__
#else
#define ZMX_HD
#endif

namespace zamd {

constexpr uint64_t kProbeBytes = 64;       // a probe: "the next 64 bytes"
constexpr uint64_t kProbeStride = 1024;    // MasterBlockCost's probes; every fourth is one of LooksLikeRuns (4096)
constexpr uint64_t kTailRunMax = 65600;    // PlanReuse looks no further back than this from a block's end

// The counts of one range.  probes / runs / few: MasterBlockCost (a probe every 1024 bytes: 64 equal bytes; at most 4
// distinct values and not a run).  probes4k / hits: LooksLikeRuns (a probe every 4096 bytes: 64 equal bytes).
enum { kProbes = 0, kRuns = 1, kFew = 2, kProbes4k = 3, kHits = 4, kProbeCounts = 5 };

// 0 = neither, 1 = the 64 bytes at p are equal, 2 = they hold at most 4 distinct values (and are not a run)
ZMX_HD inline int ProbeClass(const unsigned char* p) {
  uint32_t seen = p[0];   // the distinct values so far, a byte each
  uint32_t n = 1;
  for (uint32_t j = 1; j < kProbeBytes; ++j) {
    const uint32_t c = p[j];
    bool known = false;
    for (uint32_t k = 0; k < 4; ++k) known |= k < n && ((seen >> (8 * k)) & 255u) == c;
    if (known) continue;
    if (n == 4) return 0;
    seen |= c << (8 * n);
    ++n;
  }
  return n == 1 ? 1 : 2;
}

// Probes of [begin, end): probe k lies at begin + 1024 k, while its 64 bytes end at or before `end`.
ZMX_HD inline uint64_t ProbeCount(uint64_t begin, uint64_t end) {
  return end >= begin + kProbeBytes ? (end - begin - kProbeBytes) / kProbeStride + 1 : 0;
}

// Adds probe k of the range that begins at `begin` to its counts.
ZMX_HD inline void ProbeAdd(const unsigned char* in, uint64_t begin, uint64_t k, uint32_t counts[kProbeCounts]) {
  const int cls = ProbeClass(in + begin + k * kProbeStride);
  counts[kProbes] += 1;
  counts[kRuns] += cls == 1;
  counts[kFew] += cls == 2;
  if (k % 4 == 0) {
    counts[kProbes4k] += 1;
    counts[kHits] += cls == 1;
  }
}

// The counts of in[begin, end), one probe after the other (the host's path; k_probe_counts gives the same numbers).
inline void ProbeRange(const unsigned char* in, uint64_t begin, uint64_t end, uint32_t counts[kProbeCounts]) {
  for (int i = 0; i < kProbeCounts; ++i) counts[i] = 0;
  const uint64_t n = ProbeCount(begin, end);
  for (uint64_t k = 0; k < n; ++k) ProbeAdd(in, begin, k, counts);
}

// The lowest position PlanReuse's walk back from inend - 1 may reach.
ZMX_HD inline uint64_t TailRunFloor(uint64_t instart, uint64_t inend) {
  // the walk stops once inend - r reaches 65600
  return inend >= instart + kTailRunMax ? inend - kTailRunMax : instart;
}

// First position r of the block in[instart, inend), inend > instart, from which every byte up to inend - 1 equals the
// last one — as far back as TailRunFloor.
inline uint64_t TailRunStart(const unsigned char* in, uint64_t instart, uint64_t inend) {
  const uint64_t lo = TailRunFloor(instart, inend);
  const unsigned char last = in[inend - 1];
  uint64_t r = inend - 1;
  while (r > lo && in[r - 1] == last) --r;
  return r;
}

}  // namespace zamd

#if defined(ZMX_PROBE_KERNELS)

#include "zmx_kernels.h"   // BlockDesc and the record layout (k_rec_digest)

// Workgroups (x, range): a lane per probe, striding over the range's probes; a wave sums its lanes' counts and adds them
// to the range's five words (zeroed by the host).  Byte loads: the input may start at any address.
struct ProbeParams {
  const unsigned char* in;
  const uint64_t* ranges;   // [n][2]: begin, end
  uint32_t* counts;         // [n][kProbeCounts]
};

__global__ __launch_bounds__(256) void k_probe_counts(ProbeParams P) {
  const uint64_t begin = P.ranges[2 * blockIdx.y], end = P.ranges[2 * blockIdx.y + 1];
  const uint64_t n = zamd::ProbeCount(begin, end);
  uint32_t c[zamd::kProbeCounts] = {0, 0, 0, 0, 0};
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n;
       k += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
    zamd::ProbeAdd(P.in, begin, k, c);
  }
  for (int i = 0; i < zamd::kProbeCounts; ++i) {
    uint32_t v = c[i];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&P.counts[blockIdx.y * zamd::kProbeCounts + i], v);
  }
}

// A wave per block: 64 bytes a step back from the block's last byte, until one differs from it or the floor is reached.
struct TailRunParams {
  const unsigned char* in;
  const uint64_t* blocks;   // [n][2]: instart, inend
  uint64_t* r;              // [n]: zamd::TailRunStart (inend for an empty block)
};

__global__ __launch_bounds__(64) void k_tail_runs(TailRunParams P) {
  const uint64_t instart = P.blocks[2 * blockIdx.x], inend = P.blocks[2 * blockIdx.x + 1];
  uint64_t r = inend;
  if (inend > instart) {
    const uint64_t lo = zamd::TailRunFloor(instart, inend);
    const unsigned char last = P.in[inend - 1];
    r = lo;
    // lanes look at the 64 positions below `top`; the first lane that sees another byte ends the run above itself
    for (uint64_t top = inend - 1; top > lo; top = top - lo > 64 ? top - 64 : lo) {
      const bool valid = top - lo > threadIdx.x;
      const bool differs = valid && P.in[top - 1 - threadIdx.x] != last;
      const unsigned long long m = __ballot(differs);
      if (m) {
        r = top - static_cast<uint64_t>(__ffsll(static_cast<long long>(m)) - 1);
        break;
      }
    }
  }
  if (threadIdx.x == 0) P.r[blockIdx.x] = r;
}

// Parity probe over WHOLE tables: two 64-bit sums over all positions of a hash of (block, position in the block,
// length, distance, same, literal, every change point of sublen) — the logical content of the records, whatever
// the order the pool handed out its entries in.  Two table sets over the same blocks with equal digests hold the
// same ZopfliFindLongestMatch results (test_match_kernels_agree compares the kernels at sizes no per-position
// loop reaches).
__device__ __forceinline__ u64 dg_mix(u64 h, u64 v) {
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 31;
  return h;
}
// (C linkage: the kernel keeps the plain name it has in the resource tables and the profiles)
extern "C" __global__ __launch_bounds__(256) void k_rec_digest(const BlockDesc* __restrict__ blocks, const u32* __restrict__ recs,
                                                               const u32* __restrict__ pool, unsigned long long* out) {
  const BlockDesc bd = blocks[blockIdx.y];
  const u64 B = bd.inend - bd.instart;
  u64 s0 = 0, s1 = 0;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < B; i += (u64)gridDim.x * 256) {
    const u32* r = recs + (bd.pos_off + i) * 8;
    u64 h = dg_mix((u64)blockIdx.y * 0x100000001B3ull, i);
    h = dg_mix(h, r[0]);
    h = dg_mix(h, zamd::RecWord1(zamd::RecSame(r[1]), zamd::RecLiteral(r[1]), 0));
    // (the number of change points in front of them: the walk's two halves)
    auto mix = [&](u32 len, u32 dist) { h = dg_mix(h, zamd::RecPoolEntry(len, dist)); };
    const u32 ncpf = zamd::RecCount(r[1]);
    if (ncpf != zamd::kRecOverflow) {
      h = dg_mix(h, ncpf);
      zamd::RecWalkInlineCps(r, ncpf, mix);
    } else {
      const u32 off = zamd::RecPoolOffset(r[2]), n = zamd::RecPoolCount(r[3]);
      h = dg_mix(h, n);
      zamd::RecWalkPoolCps(pool, off, n, mix);
    }
    s0 += h;
    s1 += (h >> 17 | h << 47) * 0x94D049BB133111EBull;
  }
  atomicAdd(out, s0);
  atomicAdd(out + 1, s1);
}

#endif  // ZMX_PROBE_KERNELS

#endif  // ZMX_PROBE_H_
