// What the inflate entries (inflate.cc, device/drv_inflate.h) decide without a device, as plain functions that tests share:
// the order of the jobs, the rounds, what the entries refuse of their ranges, the verdict over a call's results.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "entry_checks.h"
#include "zmx_inflate.h"
#include "zopfli_amd.h"

namespace zamd {

constexpr size_t kInflateRoundJobs = 65536;   // what one launch's job and result arrays take

inline const char* InflateStatusName(uint32_t status) {
  static const char* const kNames[kInflateStatuses] = {
      "ZMX_INFLATE_OK", "ZMX_INFLATE_HEADER", "ZMX_INFLATE_DICT", "ZMX_INFLATE_BLOCK_TYPE", "ZMX_INFLATE_STORED_LEN",
      "ZMX_INFLATE_TOO_MANY_SYMBOLS", "ZMX_INFLATE_REPEAT", "ZMX_INFLATE_OVERSUBSCRIBED", "ZMX_INFLATE_INCOMPLETE",
      "ZMX_INFLATE_NO_END_CODE", "ZMX_INFLATE_BAD_CODE", "ZMX_INFLATE_BAD_SYMBOL", "ZMX_INFLATE_DISTANCE", "ZMX_INFLATE_TRUNCATED",
      "ZMX_INFLATE_CAPACITY", "ZMX_INFLATE_CHECKSUM", "ZMX_INFLATE_SIZE"};
  return status < kInflateStatuses ? kNames[status] : "an unknown status";
}

inline bool InflateFormatOk(int format) {
  return format == ZOPFLI_FORMAT_GZIP || format == ZOPFLI_FORMAT_ZLIB || format == ZOPFLI_FORMAT_DEFLATE;
}

// The jobs longest input first, as the chain's run tasks are listed: the waves that take longest start first.  Equal
// sizes keep the caller's order.
inline std::vector<InflateJob> InflateJobs(size_t n, const void* const* d_in, const size_t* insize, void* const* d_out, const size_t* capacity) {
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), size_t{0});
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return insize[a] > insize[b]; });
  std::vector<InflateJob> jobs(n);
  for (size_t k = 0; k < n; ++k) {
    const size_t i = order[k];
    unsigned char* const out = d_out ? static_cast<unsigned char*>(d_out[i]) : nullptr;
    jobs[k] = {static_cast<const unsigned char*>(d_in[i]), insize[i], out, out && capacity ? capacity[i] : 0, i};
  }
  return jobs;
}
// round r of the sorted jobs: [begin, end)
inline size_t InflateRounds(size_t n) { return (n + kInflateRoundJobs - 1) / kInflateRoundJobs; }
inline void InflateRound(size_t n, size_t r, size_t* begin, size_t* end) {
  *begin = r * kInflateRoundJobs;
  *end = std::min(n, *begin + kInflateRoundJobs);
}

// No destination may share a byte with another destination or with any input of the call (a null destination has none).
inline std::string CheckInflateApart(const char* who, size_t n, const void* const* d_in, const size_t* insize, void* const* d_out,
                                     const size_t* capacity) {
  if (!d_out) return std::string();
  ApartRanges apart;
  for (size_t i = 0; i < n; ++i) {
    if (!d_out[i]) continue;
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_out[i]);
    apart.Add(at, at + capacity[i], i);
  }
  apart.Sort();
  size_t a = 0, b = 0;
  if (apart.Overlap(&a, &b)) {
    return Refusal(who, "destination " + std::to_string(std::max(a, b)) + " overlaps destination " + std::to_string(std::min(a, b)));
  }
  for (size_t i = 0; i < n; ++i) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_in[i]);
    if (apart.Hit(at, at + insize[i], &a)) return Refusal(who, "destination " + std::to_string(a) + " overlaps input " + std::to_string(i));
  }
  return std::string();
}

// The verdict over a call's results: empty when every stream is ZMX_INFLATE_OK; else the first failing stream's index and
// status by name — for ZMX_INFLATE_CAPACITY also what it takes — and the class of the failure.
inline std::string InflateVerdict(const char* who, size_t n, const zmx_inflate_result* results, const size_t* capacity, int* error_class) {
  for (size_t i = 0; i < n; ++i) {
    const zmx_inflate_result& r = results[i];
    if (r.status == ZMX_INFLATE_OK) continue;
    std::string text = "stream " + std::to_string(i) + ": " + InflateStatusName(r.status) + " (" + std::to_string(r.status) + ") in block " +
                       std::to_string(r.block);
    if (r.status == ZMX_INFLATE_CAPACITY) {
      text += ": the output takes " + std::to_string(r.outsize) + " bytes, d_out has " + std::to_string(capacity ? capacity[i] : 0);
    }
    *error_class = r.status == ZMX_INFLATE_CAPACITY ? ZMX_ERR_REFUSED : ZMX_ERR_DATA;
    return Refusal(who, text);
  }
  return std::string();
}

// The trailer's verdict on a stream that ended ZMX_INFLATE_OK with its output stored, whose checksum the device computed
// (CRC-32 for gzip, Adler-32 for zlib).
inline uint32_t InflateTrailerVerdict(int format, const zmx_inflate_result& r, uint32_t computed) {
  if (computed != r.stored_check) return ZMX_INFLATE_CHECKSUM;
  if (format == ZOPFLI_FORMAT_GZIP && r.stored_isize != static_cast<uint32_t>(r.outsize & 0xffffffffu)) return ZMX_INFLATE_SIZE;
  return ZMX_INFLATE_OK;
}

}  // namespace zamd
