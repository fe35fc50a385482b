// What the batch entry point (batch.cc, zmx_compress_batch) and png.cc share with the single-call path of api.cc: the master
// blocks of an input and the dealing of parts over the context pool — contexts, cost dealing, ordered uploads, stream
// priorities, the retry of a failed shard on another context.  api.cc itself calls no device function that the batch
// added: the hooks below are where batch.cc tells a context about its segments and takes its checksums.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "deflate.h"
#include "symbols.h"
#include "zopfli_amd.h"

namespace zamd {

// A request whose input is the concatenation of independent inputs (zmx_set_input_segments).
struct ShardHooks {
  // the first byte of the input that position `pos` lies in: a shard's upload starts at max(this, start - 32 KiB)
  std::function<size_t(size_t pos)> floor;
  // called on the shard's thread once its bytes in[base, ...) are resident on `ctx`, the shard holding parts
  // [first, last) of the request: tells the context its segments (and takes what else the caller needs of the
  // resident bytes); non-zero = failure, with zmx_last_error / zmx_last_error_class set
  std::function<int(size_t shard, zmx_ctx* ctx, size_t base, size_t first, size_t last)> uploaded;
  // a DeflateParts call takes parts up to this many bytes (halved when the device layer asks for fewer)
  size_t group_bytes = 0;
  // the block-split search's rounds on the device (g_split_on_device, deflate.h)
  bool split_on_device = false;
  // the failure of the request, when it fails
  std::string error;
  int error_class = ZMX_ERR_NONE;
};

// The container's checksum over in[0, limit) of a dealt call, taken on the devices from the bytes they hold anyway —
// each device its own parts' bytes, put together in stream order.
struct ChecksumRequest {
  int kind;         // ZMX_CRC32 / ZMX_ADLER32
  size_t limit;     // bytes covered (the parts must start at 0 and cover them)
  uint32_t value;
};

// A request whose input lies in device memory (zmx_compress_device, device_input.cc; zmx_compress_device_batch,
// batch.cc): the host holds no byte of it.  What the dealing reads of the bytes comes from counts taken on the device
// before it (k_probe_counts), so the dealing is that of the same bytes on the host.
struct DeviceInput {
  // bytes [base, base + n) of the input become the resident input of `ctx` (zmx_set_input_device)
  std::function<int(zmx_ctx* ctx, size_t base, size_t n)> upload;
  // By PART of the request, wherever its bytes start (the parts of a batch start where their inputs do):
  std::vector<double> cost;   // MasterBlockCost of every part (empty: nothing to deal)
  std::vector<char> runs;     // LooksLikeRuns of every round of `round_parts` parts (ZOPFLI_AMD_ROUND_PARTS)
  size_t round_parts = 1;
  size_t first_part = 0;      // the part of the request that the round being dealt begins with (set by who runs the rounds)
  // Output that stays in device memory (zmx_compress_device_to_device, device_output.cc; zmx_compress_device_batch_to_device,
  // batch.cc, which takes the chunk counts of RunPartsDealt's `part_chunks` with the chunks; one round only):
  // the shards run with g_device_output set and leave the bytes of stored blocks where they are; the call is dealt over the
  // contexts of `only_device` alone; `finish` runs once the shards are collected, on one of the call's contexts and while
  // the call still holds them all — the chunks' device bits are theirs — with the container's checksum (0 without one);
  // non-zero = failure, with zmx_last_error / zmx_last_error_class set.  The chunks let go of their device bits before the
  // contexts go back to the pool, whatever `finish` did with them.
  bool device_output = false;
  int only_device = -1;
  std::function<int(zmx_ctx* ctx, std::vector<Chunk>* chunks, uint32_t sum)> finish;
  // the failure of the request, when it fails
  std::string error;
  int error_class = ZMX_ERR_NONE;
  // of part i of the round being dealt
  double Cost(size_t i) const { return cost[first_part + i]; }
  // of the round being dealt
  bool Runs() const {
    const size_t round = first_part / round_parts;
    return round < runs.size() && runs[round] != 0;
  }
};
// ZopfliCompress of `insize` bytes of device memory: dealt, retried and done in rounds as a host call's; non-zero on
// failure, with dev->error / error_class set and *out, *outsize as they were
int CompressFromDevice(const ZopfliOptions* options, ZopfliFormat output_type, DeviceInput* dev, size_t insize,
                       unsigned char** out, size_t* outsize);

// dev->cost and dev->runs (dev->round_parts set) of d_in[0, insize), memory of HIP device `device`: MasterBlockCost of every
// master block and LooksLikeRuns of every round, from one launch of k_probe_counts on a pooled context (device_input.cc)
int ProbeDeviceInput(const void* d_in, size_t insize, int device, DeviceInput* dev);

// ZopfliDeflate's master blocks of an input of `insize` bytes (deflate.c:916-923): at least one, even when empty
std::vector<Part> InputMasterBlocks(size_t insize, bool final);
// the parts of a request dealt over the pool's contexts (one round: the request's bytes plus a window stay below 2^32);
// `part_chunks` gets the number of chunks of every part, in part order.  `dev` (with `in` null): the bytes lie in device
// memory, positions as for `in`; stored chunks then carry their bytes.
int RunPartsDealt(const ZopfliOptions& options, int btype, const unsigned char* in, const std::vector<Part>& parts,
                  std::vector<Chunk>* chunks, std::vector<size_t>* part_chunks, ShardHooks* hooks, DeviceInput* dev = nullptr);
// the per-call timing and statistics of the calling thread start again (zmx_last_timing ...)
void ResetCallStats();
// input bytes the calling thread's call moved device to device outside its shards (zmx_last_input_traffic [1])
void AddDeviceTraffic(double bytes);
// what zmx_last_output_traffic reports of the calling thread's call (four numbers)
void SetOutputTraffic(const double* t4);
// ZopfliDeflate (btype 2) of the one round of master blocks `parts` of a device input whose output stays in device memory:
// dealt as RunPartsDealt deals, `sum` taken as a whole-stream call takes it, then dev->finish; on failure dev->error /
// error_class are set
int RunPartsToDevice(const ZopfliOptions& options, const std::vector<Part>& parts, ChecksumRequest* sum, DeviceInput* dev);
// ZOPFLI_AMD_TRACE_CALL=1, and the clock of its lines
bool TraceCallOn();
double CallWallMs();
// `fn` on one of the pool's contexts, held for the call (what the *_pooled entry points outside api.cc use);
// `only_device` >= 0: a context of that HIP device — -1 with the error set when it is none of the library's
int OnPooledContext(const std::function<int(zmx_ctx*)>& fn, int only_device = -1);

}  // namespace zamd
