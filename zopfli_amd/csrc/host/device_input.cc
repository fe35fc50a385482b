// zmx_compress_device: ZopfliCompress of bytes that already lie in device memory.
//
// The host reads an input's bytes in four places — the probes that deal master blocks over the contexts, the tail of a
// block when match tables are reused, the bytes of stored blocks, the shards' uploads — and each has a device form
// (device/zmx_probe.h, zmx_set_input_device, zmx_internal_input_fetch).  Here: the pointer is checked, the probes' counts
// are taken once, on a pooled context, and the call then runs as a host call's does (dealing.h), its shards copying
// their bytes device to device.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "deal.h"
#include "dealing.h"
#include "host_knobs.h"
#include "symbols.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"
#include "../device/zmx_probe.h"

namespace {

int Refuse(const char* msg) {
  zmx_internal_set_error(msg, ZMX_ERR_REFUSED);
  return -1;
}

// MasterBlockCost of every master block and LooksLikeRuns of every round of d_in[0, insize), from one launch of
// k_probe_counts on a pooled context.  On the pointer's own device the kernel reads the caller's buffer; a context of
// another device takes a copy first (zmx_set_input_device: the runtime's peer copy).
}  // namespace

int zamd::ProbeDeviceInput(const void* d_in, size_t insize, int device, zamd::DeviceInput* dev) {
  const size_t nblocks = (insize + zamd::kMasterBlock - 1) / zamd::kMasterBlock;
  const size_t nrounds = (nblocks + dev->round_parts - 1) / dev->round_parts;
  std::vector<uint64_t> ranges;
  for (size_t b = 0; b < nblocks; ++b) {
    ranges.push_back(b * zamd::kMasterBlock);
    ranges.push_back(std::min(insize, (b + 1) * zamd::kMasterBlock));
  }
  for (size_t r = 0; r < nrounds; ++r) {
    ranges.push_back(r * dev->round_parts * zamd::kMasterBlock);
    ranges.push_back(std::min(insize, (r + 1) * dev->round_parts * zamd::kMasterBlock));
  }
  std::vector<uint32_t> counts((nblocks + nrounds) * zamd::kProbeCounts);
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    const void* bytes = d_in;
    if (zmx_internal_device(ctx) != device) {
      if (zmx_set_input_device(ctx, d_in, insize) != 0) return -1;
      bytes = nullptr;
    }
    return zmx_internal_probe_counts(ctx, bytes, nblocks + nrounds, ranges.data(), counts.data());
  });
  if (rc) return rc;
  dev->cost.resize(nblocks);
  for (size_t b = 0; b < nblocks; ++b) {
    const uint32_t* k = &counts[b * zamd::kProbeCounts];
    dev->cost[b] = zamd::CostFromCounts(ranges[2 * b + 1] - ranges[2 * b], k[zamd::kProbes], k[zamd::kRuns], k[zamd::kFew]);
  }
  dev->runs.resize(nrounds);
  for (size_t r = 0; r < nrounds; ++r) {
    const uint32_t* k = &counts[(nblocks + r) * zamd::kProbeCounts];
    dev->runs[r] = zamd::RunsFromCounts(k[zamd::kProbes4k], k[zamd::kHits]);
  }
  return 0;
}

extern "C" int zmx_compress_device(const ZopfliOptions* options, ZopfliFormat output_type, const void* d_in, size_t insize,
                                   unsigned char** out, size_t* outsize) {
  if (!options || !out || !outsize) return Refuse("zmx_compress_device: null argument");
  if (output_type != ZOPFLI_FORMAT_GZIP && output_type != ZOPFLI_FORMAT_ZLIB && output_type != ZOPFLI_FORMAT_DEFLATE) {
    char msg[96];
    std::snprintf(msg, sizeof(msg), "zmx_compress_device: invalid ZopfliFormat %d", static_cast<int>(output_type));
    return Refuse(msg);
  }
  int device = -1;
  if (zmx_internal_device_pointer("zmx_compress_device", d_in, insize, &device) != 0) return -1;
  zamd::DeviceInput dev;
  dev.round_parts = std::max<size_t>(zamd::HostSwitches().round_parts, 1);
  dev.upload = [&](zmx_ctx* ctx, size_t base, size_t n) {
    return zmx_set_input_device(ctx, static_cast<const unsigned char*>(d_in) + base, n);
  };
  // (one master block: one shard on one context, whatever its bytes — nothing reads the counts)
  if (insize > zamd::kMasterBlock && zamd::ProbeDeviceInput(d_in, insize, device, &dev) != 0) return -1;
  if (zamd::CompressFromDevice(options, output_type, &dev, insize, out, outsize) != 0) {
    zmx_internal_set_error(dev.error.c_str(), dev.error_class);
    return -1;
  }
  return 0;
}
