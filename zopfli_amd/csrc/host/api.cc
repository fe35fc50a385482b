// C ABI of libzopfli_amd.so, part 1: the reference's public surface
// (zopfli.h:67,86; deflate.h:58,67; gzip_container.h:42; zlib_container.h:42),
// plus the resident-input stream entry points used by bench.py and by the
// multi-GPU gather.
#include <chrono>
#include <malloc.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "block_cache.h"
#include "block_cost.h"
#include "context_pool.h"
#include "deflate.h"
#include "lz77_optimal.h"
#include "symbols.h"
#include "deal.h"
#include "dealing.h"
#include "thread_pool.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"

namespace zamd {

[[noreturn]] void Die(const char* what) {
  std::fprintf(stderr, "zopfli_amd: %s: %s\n", what, zmx_last_error());
  std::exit(EXIT_FAILURE);
}

// OPT-IN ONLY (ZOPFLI_AMD_KEEP_HEAP=1 / 2; unset or 0: malloc is left alone): mallopt so that glibc neither trims its
// arenas nor shrinks the worker threads' heaps.  Round 5 made this the default (+12 % with block splitting) and the review
// was right to object: it reconfigures the allocator of the whole host process, for good — a drop-in libzopfli.so.1 must
// not (the reference has no side effects outside its arguments).  Round 6: the host arrays that caused the
// churn — the blocks' symbol stores, positions, sampled histograms, bit buffers — take their memory from the library's
// own block cache (block_cache.h, ZOPFLI_AMD_HOST_CACHE_MB), which touches nothing process-wide.  The switch stays for
// measuring one against the other.
void MaybeKeepHeap() {
  static const bool once = [] {
    const int mode = zamd::HostSwitches().keep_heap;
    if (mode == 0) return true;
    if (mode == 2) {          // (for measuring: large blocks from the heap too — 32 MB is the most glibc takes; no better, nor is 1 MB)
      mallopt(M_MMAP_THRESHOLD, 32 << 20);
      mallopt(M_TRIM_THRESHOLD, 1 << 30);
      mallopt(M_TOP_PAD, 64 << 20);
    } else {
      mallopt(M_TRIM_THRESHOLD, 1 << 30);
      mallopt(M_TOP_PAD, 256 << 20);
    }
    return true;
  }();
  (void)once;
}

zmx_stats& ThreadStats() {
  static thread_local zmx_stats stats = {};
  return stats;
}

unsigned long long& CallPositions() {
  static thread_local unsigned long long positions = 0;
  return positions;
}

}  // namespace zamd

namespace {

// a shard thread's sums since it started, zeroed — and added to the calling thread's (at the join of a call's shards)
zmx_stats TakeStats() {
  const zmx_stats s = zamd::ThreadStats();
  zamd::ThreadStats() = zmx_stats{};
  return s;
}
void AddStats(const zmx_stats& s) {
  zmx_stats& t = zamd::ThreadStats();
  for (int i = 0; i < 3; ++i) t.kernel_seconds[i] += s.kernel_seconds[i];
  t.squeeze_launches += s.squeeze_launches;
  for (int i = 0; i < 3; ++i) t.match5[i] += s.match5[i];
  for (int i = 0; i < 4; ++i) t.match[i] += s.match[i];
  for (int i = 0; i < ZMX_SEG_N; ++i) t.seg[i] += s.seg[i];
}

using zamd::Die;
using zamd::kMasterBlock;
using zamd::Lease;
using zamd::MaybeKeepHeap;
using zamd::Pool;

// ZOPFLI_AMD_TRACE_CALL=1: where a Zopfli* call's wall time goes, per shard and for the call (stderr)
bool TraceCall() { return zamd::HostSwitches().trace_call; }
double WallMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// zmx_last_input_traffic: the input bytes of the calling thread's last call that went host to device, device to device,
// device to host (a call's shard threads hand theirs to the caller's at the join)
thread_local double g_traffic[3] = {0, 0, 0};
// zmx_last_output_traffic: the stream's bytes device to host and host to device, the blocks whose symbols' bits stayed on
// the device and those the host wrote and uploaded
thread_local double g_out_traffic[4] = {0, 0, 0, 0};

// The stored chunks of an input the host holds no copy of (zmx_set_input_device) take their bytes from the context
// they were computed on, each its own range only; positions relative to the context's input.
// (The reference from THIS file is weak, the declaration and the device layer's definition are not: these host sources
//  also load with the device-layer stand-in of the commit before this function's stub, so that that commit's host tests
//  run against them unchanged.  Only a stand-in can lack it, and no stand-in holds an input in device memory.)
#pragma weak zmx_internal_input_fetch
int FetchStoredBytes(zmx_ctx* ctx, std::vector<zamd::Chunk>* chunks, double* fetched) {
  for (zamd::Chunk& c : *chunks) {
    if (c.kind != zamd::Chunk::kStored || c.end == c.start) continue;
    if (!zmx_internal_input_fetch) {
      zmx_internal_set_error("stored block of a device input: this build cannot fetch its bytes", ZMX_ERR_DEVICE);
      return -1;
    }
    c.raw.resize(c.end - c.start);
    if (zmx_internal_input_fetch(ctx, c.start, c.end, c.raw.data()) != 0) return -1;
    *fetched += static_cast<double>(c.end - c.start);
  }
  return 0;
}

std::vector<zamd::Part> MasterBlocks(size_t insize, bool final) {
  // deflate.c:916-923: do { ... } while (i < insize), so an empty input still
  // yields one (empty) part.
  std::vector<zamd::Part> parts;
  size_t i = 0;
  do {
    const bool masterfinal = i + kMasterBlock >= insize;
    const size_t size = masterfinal ? insize - i : kMasterBlock;
    parts.push_back({i, i + size, final && masterfinal});
    i += size;
  } while (i < insize);
  return parts;
}

// `group_bytes` (batches of many small inputs, zamd::ShardHooks): a DeflateParts call takes parts up to that many bytes
// instead of ZOPFLI_AMD_PARTS_PER_BATCH parts — 256 parts of 64 KiB would leave the device idle — and at most 2048 of them (a part
// may become 15 blocks or more, and the blocks of a table build are one launch dimension).
// `part_chunks` (optional): the number of chunks of every part, in part order.
int RunParts(zmx_ctx* ctx, const ZopfliOptions& options, int btype, const std::vector<zamd::Part>& parts,
             std::vector<zamd::Chunk>* chunks, std::vector<size_t>* part_chunks = nullptr, size_t group_bytes = 0) {
  size_t step = zamd::HostSwitches().parts_per_batch;
  size_t step_bytes = group_bytes;
  for (size_t a = 0; a < parts.size();) {
    size_t b = a + step < parts.size() ? a + step : parts.size();
    if (group_bytes) {
      b = a + 1;
      size_t bytes = parts[a].inend - parts[a].instart;
      while (b < parts.size() && b - a < 2048 && bytes + (parts[b].inend - parts[b].instart) <= step_bytes) {
        bytes += parts[b].inend - parts[b].instart;
        ++b;
      }
    }
    std::vector<zamd::Part> group(parts.begin() + static_cast<long>(a), parts.begin() + static_cast<long>(b));
    std::vector<zamd::Chunk> got;
    const int rc = zamd::DeflateParts(ctx, options, btype, group, &got, part_chunks);
    if (rc == -2 && b - a > 1) {   // the DP edges of the batch do not fit the device layer's budget: smaller batches
      step = (b - a + 1) / 2;
      step_bytes = std::max<size_t>(step_bytes / 2, 1);
      continue;
    }
    if (rc) return rc;
    for (auto& c : got) chunks->push_back(std::move(c));
    a = b;
  }
  return 0;
}

// The parts of one request (positions relative to `in`) dealt over the shared contexts in contiguous
// runs, one host thread per device; each device gets its parts' bytes plus the 32 KiB before them
// (all a part reads: lz77.c:551-552).  Chunks come back in stream order, stored chunks carrying
// positions relative to `in`.
//
// `sum` (optional): the container's checksum over in[0, sum->limit), taken on the devices from the bytes
// they hold anyway — each device its own parts' bytes, put together in stream order.
using zamd::ChecksumRequest;   // (dealing.h)

struct Shard {
  size_t first = 0, last = 0, base = 0;
  std::vector<zamd::Chunk> chunks;
  std::vector<size_t> part_chunks;
  int rc = 0;
  std::string err;
  int err_class = ZMX_ERR_NONE;   // zmx_last_error_class() of the failure
  zamd::Timing timing;
  uint32_t sum = 0;
  size_t sum_bytes = 0;
  bool redone = false;
  zmx_stats stats = {};          // the shard thread's kernel / match / task statistics (TakeStats)
  double traffic[3] = {0, 0, 0}; // its input bytes, as g_traffic (all attempts)
};

// The contexts of ONE device take their bytes over the same link: asked for at once, three uploads end together and
// the device has nothing to do until then (12 ms of a 122 ms call on 100 MB; the kernel timeline of
// tools/r04_timeline.sh).  One after the other, in stream order, the first context computes while the second's bytes
// travel — and the contexts stay out of step from there on: their host phases (block split, cost models) fall
// beside the others' kernels instead of beside each other.
struct UploadOrder {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<char> done;
  std::vector<long> after;     // the shard whose upload this one waits for, -1 = none (zamd::UploadAfter)
};
struct UploadTurn {     // marks a shard's upload as over, however its attempt ends
  UploadOrder& o; size_t d; bool released = false;
  void Wait() {
    if (o.after[d] < 0) return;
    std::unique_lock<std::mutex> lock(o.mu);
    o.cv.wait(lock, [&] { return o.done[static_cast<size_t>(o.after[d])] != 0; });
  }
  void Release() {
    if (released) return;
    released = true;
    { std::lock_guard<std::mutex> lock(o.mu); o.done[d] = 1; }
    o.cv.notify_all();
  }
  ~UploadTurn() { Release(); }
};

// A call that is dealt: what its shards share.
struct ShardedCall {
  const ZopfliOptions& options;
  int btype;
  const unsigned char* in;
  zamd::DeviceInput* dev;         // the input lies in device memory (`in` is null then)
  const std::vector<zamd::Part>& parts;
  ChecksumRequest* sum;
  bool want_part_chunks;
  zamd::ShardHooks* hooks;
  double t_begin;                 // WallMs() when the call asked for its contexts
  std::vector<Shard> shards;
  std::vector<int> priority;      // stream priority of every shard's context
  std::vector<unsigned long long> device_positions;   // per shard: the bytes of all the call's shards on its device
  UploadOrder order;
};

// How many contexts of each device the call takes; *runs: its data has long runs of equal bytes.
//
// (ZOPFLI_AMD_SPLIT_MB: from this many master blocks on, a request is dealt over ZOPFLI_AMD_SPLIT_WAYS = 3 contexts of
//  each device — measured on 100 MB of text: 2 ways 123.2 ms, 3 ways 121.1, 4 ways 140; with block splitting 225 / 197 / 231;
//  0 = never.  The GPU idles while the host computes a hundred cost models between two squeeze runs — 6 % of a
//  100 MB call — and through the whole block-split search; two halves fill each other's gaps.)
// Round 5, from how many master blocks on (profiles/r05_split_from.txt): with block splitting from 4 — the contexts'
// split searches fall beside each other's kernels: 4 MB of text 33.7 -> 29.2 ms, 8 MB 46.5 -> 37.4, 12 MB 59.8 -> 43.6,
// 24 MB 97.4 -> 62.8 (it was 32 until then); without block splitting it is worth 3 - 6 % from 12 MB on and nothing
// below: from 16.
// Data with long runs of equal bytes: there the squeeze runs wait for a few very long single-wave tasks (zmx_dp5.h)
// and most of the device idles — but a second context's tasks on the same SIMDs slow exactly those tasks (round 3,
// class Z: 61 -> 35 MB/s on two contexts, so such data stayed on one).  Round 5: dealt all the same, with the contexts
// at three stream PRIORITIES (as calls with block splitting are, PlanShards): the first context's long tasks win their
// SIMDs, the others fill what it leaves — class Z 131 -> 190 MB/s, class M 165 -> 245 (189 / 245 on four, 187 / 250 on
// six contexts; without the priorities 112 / 170; profiles/r05_runs_ctx.txt).  Which data: zamd::LooksLikeRuns.
// (ZOPFLI_AMD_SPLIT_RUNS=0 or ZOPFLI_AMD_STREAM_PRIO=0: such data on one context, as before — for measuring)
size_t ContextsPerDevice(const ZopfliOptions& options, int btype, const unsigned char* in, const zamd::DeviceInput* dev,
                         const std::vector<zamd::Part>& parts, bool* runs) {
  const zamd::HostKnobs& k = zamd::HostSwitches();
  const size_t split_from = k.split_mb >= 0 ? static_cast<size_t>(k.split_mb) : (options.blocksplitting && btype == 2 ? 4 : 16);
  *runs = false;
  if (!split_from || parts.size() < split_from) return 1;
  *runs = dev ? dev->Runs()
              : in != nullptr && zamd::LooksLikeRuns(in, parts.front().instart, parts.back().inend);
  const bool one_context = *runs && !(k.stream_prio && k.split_runs);
  return one_context ? 1 : k.split_ways;
}

// The shards' part ranges, stream priorities and upload order, for contexts on the devices `device_of` (one per shard).
void PlanShards(ShardedCall* call, const std::vector<int>& device_of, bool runs) {
  const zamd::HostKnobs& k = zamd::HostSwitches();
  const std::vector<zamd::Part>& parts = call->parts;
  const size_t ndev = device_of.size();
  // Shards of equal COST, not of equal count (deal.h): on a mixed corpus the master blocks of long runs of equal bytes
  // cost several times the others, and contiguous equal-count shards leave them to one or two contexts.  From the
  // bytes alone — the one-process-per-GPU launchers compute the same ranges (zmx_master_block_costs).
  // (ZOPFLI_AMD_DEAL=count: equal counts, as before — for measuring)
  std::vector<double> cost;
  const bool have_costs = call->dev ? !call->dev->cost.empty() : call->in != nullptr;
  if (k.deal_by_cost && ndev > 1 && have_costs && parts.size() > ndev) {
    cost.resize(parts.size());
    if (call->dev) {
      for (size_t i = 0; i < parts.size(); ++i) cost[i] = call->dev->Cost(i);
    } else {
      zamd::ParallelFor(parts.size(), [&](size_t i) { cost[i] = zamd::MasterBlockCost(call->in, parts[i].instart, parts[i].inend); });
    }
  }
  const std::vector<size_t> first = zamd::ShardRanges(parts.size(), ndev, cost.empty() ? nullptr : cost.data(), k.shard_weights);
  call->shards = std::vector<Shard>(ndev);
  for (size_t d = 0; d < ndev; ++d) { call->shards[d].first = first[d]; call->shards[d].last = first[d + 1]; }
  // what the call puts on each shard's device in all: the chain's task length goes by that, not by the shard (RunShard)
  // (not for data with long runs of equal bytes: a pass of the chain waits for its longest task there, and tasks twice as
  //  long took class Z from 482 to 673 ms a step)
  call->device_positions.assign(ndev, 0);
  for (size_t d = 0; d < ndev && !runs; ++d) {
    for (size_t e = 0; e < ndev; ++e) {
      if (device_of[e] == device_of[d] && first[e + 1] > first[e]) call->device_positions[d] += parts[first[e + 1] - 1].inend - parts[first[e]].instart;
    }
  }
  // With block splitting the contexts of one device run at three stream priorities — one after the other instead of
  // side by side: their split searches and joins then fall beside the others' kernels (zmx_ctx_set_priority; 100 MB of
  // text 152 -> 145 ms, without block splitting 123 -> 130: there every context stays on its default streams).
  // Data with runs: with or without block splitting (ContextsPerDevice).
  // (ZOPFLI_AMD_STREAM_PRIO=0: never; 2: always — for measuring)
  const bool priorities = k.stream_prio && ((call->options.blocksplitting && call->btype == 2) || runs || k.stream_prio == 2);
  call->priority = priorities ? zamd::ShardPriorities(device_of) : std::vector<int>(ndev, 0);
  // (ZOPFLI_AMD_UPLOAD_ORDER=0: all at once, as before — for measuring)
  call->order.done.assign(ndev, 0);
  call->order.after = k.upload_order ? zamd::UploadAfter(device_of) : std::vector<long>(ndev, -1);
}

// (a call that is one shard — a small file — keeps the level its context was given when first seen: the contexts of
//  concurrent small callers then lie on streams of all three priorities, i.e. on three sets of hardware queues instead of
//  one — the runtime gives a priority four queues, and sixteen streams on four queues run their short kernels one after
//  the other: 1 000 files of 64 KiB through 16 callers 26.8 -> 29.9 MB/s, 160 of 1 MB 220 -> 283, profiles/r06_small_hwq.txt;
//  ZOPFLI_AMD_SMALL_PRIO=0: every such call on the default priority, as before)
int SmallCallLevel(zmx_ctx* ctx) {
  static std::mutex mu;
  static std::unordered_map<zmx_ctx*, int> levels;
  std::lock_guard<std::mutex> g(mu);
  auto it = levels.find(ctx);
  if (it == levels.end()) it = levels.emplace(ctx, static_cast<int>(levels.size() % 3) - 1).first;
  return it->second;
}

// Shard `d` of the call on `ctx`: upload, checksum, its parts.  `retry`: again, on another shard's context.
void RunShard(ShardedCall* call, size_t d, zmx_ctx* ctx, bool retry) {
  const std::vector<zamd::Part>& parts = call->parts;
  zamd::ShardHooks* hooks = call->hooks;
  ChecksumRequest* sum = call->sum;
  Shard& sh = call->shards[d];
  UploadTurn turn{call->order, d};
  int level = retry ? 0 : call->priority[d];
  if (zamd::HostSwitches().small_prio && call->shards.size() == 1 && !retry) level = SmallCallLevel(ctx);
  if (zmx_ctx_set_priority(ctx, level) != 0) {
    // (not fatal: the context stays on the streams it has, the shards then run side by side instead of in turn)
    std::fprintf(stderr, "zopfli_amd: stream priorities unavailable (%s)\n", zmx_last_error());
  }
  sh.rc = 0;
  sh.err.clear();
  sh.err_class = ZMX_ERR_NONE;
  sh.chunks.clear();
  sh.part_chunks.clear();
  sh.sum = 0;
  sh.sum_bytes = 0;
  auto fail = [&] { sh.rc = -1; sh.err = zmx_last_error(); sh.err_class = zmx_last_error_class(); };
  // (ZOPFLI_AMD_TEST_FAIL_SHARD=k: the k-th shard's first attempt fails before it does anything — the test of the
  //  re-queue, RetryFailedShards)
  if (!retry && zamd::HostSwitches().test_fail_shard == static_cast<long>(d)) {
    sh.rc = -1;
    sh.err = "injected failure (ZOPFLI_AMD_TEST_FAIL_SHARD): PoolAlloc(pool) too large — the text must not matter";
    sh.err_class = ZMX_ERR_OUT_OF_MEMORY;
    return;
  }
  const size_t start = parts[sh.first].instart, end = parts[sh.last - 1].inend;
  sh.base = start > zamd::kWindow ? start - zamd::kWindow : 0;
  if (hooks) sh.base = std::max(sh.base, hooks->floor(parts[sh.first].instart));
  const double tr0 = WallMs();
  if (!retry) turn.Wait();
  const double tr1 = WallMs();
  const int up = call->dev ? call->dev->upload(ctx, sh.base, end - sh.base) : zmx_set_input(ctx, call->in + sh.base, end - sh.base);
  sh.traffic[call->dev ? 1 : 0] += static_cast<double>(end - sh.base);
  turn.Release();
  const double tr2 = WallMs();
  if (up != 0 || (hooks && hooks->uploaded(d, ctx, sh.base, sh.first, sh.last) != 0)) return fail();
  if (sum && start < sum->limit) {
    sh.sum_bytes = std::min(end, sum->limit) - start;
    if (zmx_checksum(ctx, sum->kind, start - sh.base, start - sh.base + sh.sum_bytes, &sh.sum) != 0) return fail();
  }
  std::vector<zamd::Part> mine(parts.begin() + static_cast<long>(sh.first), parts.begin() + static_cast<long>(sh.last));
  for (auto& p : mine) { p.instart -= sh.base; p.inend -= sh.base; }
  const double tr3 = WallMs();
  // A dealt call's table sets take the task length of the whole call on this device (zamd::CallPositions): the contexts
  // share the device, and a context's third of 100 MB got 1024-position tasks where 2048 are faster (112.2 -> 107.0 ms a
  // step, profiles/chain_stretch.txt).  A call that is one shard says nothing: the thresholds of small calls stay.
  struct CallPositionsScope {
    explicit CallPositionsScope(unsigned long long n) { zamd::CallPositions() = n; }
    ~CallPositionsScope() { zamd::CallPositions() = 0; }
  } call_positions(call->shards.size() > 1 ? call->device_positions[d] : 0);
  struct SplitOnDevice {
    bool was;
    explicit SplitOnDevice(bool on) : was(zamd::g_split_on_device) { zamd::g_split_on_device = on || was; }
    ~SplitOnDevice() { zamd::g_split_on_device = was; }
  } split_on_device(hooks && hooks->split_on_device);
  const bool device_output = call->dev && call->dev->device_output;
  struct DeviceOutput {
    bool was;
    explicit DeviceOutput(bool on) : was(zamd::g_device_output) { zamd::g_device_output = on; }
    ~DeviceOutput() { zamd::g_device_output = was; }
  } device_output_mode(device_output);
  sh.rc = RunParts(ctx, call->options, call->btype, mine, &sh.chunks, call->want_part_chunks ? &sh.part_chunks : nullptr,
                   hooks ? hooks->group_bytes : 0);
  // (output in device memory: the join reads the stored blocks' bytes where the input lies)
  if (!sh.rc && call->dev && !device_output && FetchStoredBytes(ctx,&sh.chunks, &sh.traffic[2]) != 0) sh.rc = -1;
  if (sh.rc) { sh.err = zmx_last_error(); sh.err_class = zmx_last_error_class(); }
  if (TraceCall()) {
    std::fprintf(stderr, "  shard %zu (%zu parts): start +%.2f ms, wait for turn %.2f, upload %.2f, checksum %.2f, parts %.2f, end +%.2f\n",
                 d, sh.last - sh.first, tr0 - call->t_begin, tr1 - tr0, tr2 - tr1, tr3 - tr2, WallMs() - tr3, WallMs() - call->t_begin);
  }
  for (auto& c : sh.chunks) {
    if (c.kind == zamd::Chunk::kStored) { c.start += sh.base; c.end += sh.base; }
  }
  sh.timing = zamd::ThreadTiming();
  if (d != 0 && !retry) sh.stats = TakeStats();   // (a thread of its own: its sums go to the caller's below)
}

// Every shard on its context: the first on the calling thread, the others on a thread each.
void RunShards(ShardedCall* call, const std::vector<zmx_ctx*>& ctxs) {
  const size_t ndev = call->shards.size();
  std::vector<std::thread> threads;
  for (size_t d = 1; d < ndev; ++d) threads.emplace_back(RunShard, call, d, ctxs[d], false);
  RunShard(call, 0, ctxs[0], false);
  for (auto& t : threads) t.join();
  for (size_t d = 1; d < ndev; ++d) AddStats(call->shards[d].stats);
  // the slowest device's breakdown stands for the request (zmx_last_timing)
  for (size_t d = 1; d < ndev; ++d) {
    const zamd::Timing& a = call->shards[d].timing;
    zamd::Timing& t = zamd::ThreadTiming();
    if (a.tables + a.greedy + a.squeeze + a.cost_model + a.split + a.encode >
        t.tables + t.greedy + t.squeeze + t.cost_model + t.split + t.encode) t = a;
  }
}

// A shard that failed (its device ran out of memory, its context is broken) is done again on a context that just
// finished its own shard without error — another device's where there is one — before the request gives up: the
// parts are independent (deflate.c:916-923), whoever computes them computes the same bits.
void RetryFailedShards(ShardedCall* call, const std::vector<zmx_ctx*>& ctxs) {
  std::vector<Shard>& shards = call->shards;
  for (size_t d = 0; d < shards.size(); ++d) {
    if (!shards[d].rc) continue;
    // (not a failure that would repeat itself on any context — a request the device layer refuses, a table set that
    //  overflows its pools after the retries the device layer makes itself: ZMX_ERR_REFUSED.  By the error's CLASS, not its
    //  text: an out-of-memory inside PoolAlloc reads "PoolAlloc(...): out of memory" and is exactly what a retry is for)
    if (shards[d].err_class == ZMX_ERR_REFUSED) continue;
    zmx_ctx* other = nullptr;
    for (size_t e = 0; e < shards.size() && !other; ++e) if (e != d && !shards[e].rc && !shards[e].redone) other = ctxs[e];
    if (!other) break;
    std::fprintf(stderr, "zopfli_amd: a shard failed (%s): done again on another context\n", shards[d].err.c_str());
    RunShard(call, d, other, true);
    shards[d].redone = true;
  }
}

// The shards' chunks (and chunk counts) in stream order; the first failed shard's code, with its text on stderr.
int CollectShards(ShardedCall* call, std::vector<zamd::Chunk>* chunks, std::vector<size_t>* part_chunks) {
  for (auto& sh : call->shards) {
    if (sh.rc) {
      std::fprintf(stderr, "zopfli_amd: device error: %s\n", sh.err.c_str());
      if (call->hooks) { call->hooks->error = sh.err; call->hooks->error_class = sh.err_class; }
      if (call->dev) { call->dev->error = sh.err; call->dev->error_class = sh.err_class; }
      return sh.rc;
    }
    for (auto& c : sh.chunks) chunks->push_back(std::move(c));
    if (part_chunks) part_chunks->insert(part_chunks->end(), sh.part_chunks.begin(), sh.part_chunks.end());
  }
  return 0;
}

// A small call among other calls in flight (many small files, a caller thread each): its host phases — the split
// searches' rounds of nine probes, the cost models of a block or two — run on the calling thread.  The worker pool takes
// one fork-join at a time: sixteen callers queueing for it, each job a few microseconds of work per woken thread, were
// slower than three (profiles/r06_small_files.txt); the callers are the parallelism.
struct InlineHostWork {
  bool on, was;
  explicit InlineHostWork(bool o) : on(o), was(zamd::g_host_inline) { if (on) zamd::g_host_inline = true; }
  ~InlineHostWork() { if (on) zamd::g_host_inline = was; }
};

// `hooks` (zmx_compress_batch): `in` is the concatenation of independent inputs — a shard's upload starts no lower than
// the first byte of its first part's input, the hooks tell the context its segments after the upload, the parts are
// grouped by bytes; `part_chunks` (optional) gets the number of chunks of every part, in part order.
int RunPartsShardedOnce(const ZopfliOptions& options, int btype, const unsigned char* in,
                        const std::vector<zamd::Part>& parts, std::vector<zamd::Chunk>* chunks,
                        ChecksumRequest* sum = nullptr, std::vector<size_t>* part_chunks = nullptr,
                        zamd::ShardHooks* hooks = nullptr, zamd::DeviceInput* dev = nullptr) {
  bool runs = false;
  const size_t per_device = ContextsPerDevice(options, btype, in, dev, parts, &runs);
  const double tr_begin = WallMs();
  const Lease lease(parts.size(), per_device, /*polite=*/parts.size() < 32, /*small=*/parts.size() < 32, dev ? dev->only_device : -1);
  if (lease.ctxs.empty()) {   // (only_device alone: every other call waits or dies in the pool)
    dev->error = "device " + std::to_string(dev->only_device) + " is not one of the library's devices (ZOPFLI_AMD_DEVICE, ZOPFLI_AMD_DEVICES)";
    dev->error_class = ZMX_ERR_REFUSED;
    return -1;
  }
  const double tr_lease = WallMs();
  const InlineHostWork inline_host(parts.size() <= 2 && Pool().InFlight() > 1);
  const size_t ndev = std::min(lease.ctxs.size(), parts.size());
  ShardedCall call{options, btype, in, dev, parts, sum, part_chunks != nullptr, hooks, tr_begin, {}, {}, {}, {}};
  PlanShards(&call, std::vector<int>(lease.device_of.begin(), lease.device_of.begin() + static_cast<long>(ndev)), runs);
  RunShards(&call, lease.ctxs);
  RetryFailedShards(&call, lease.ctxs);
  for (const Shard& sh : call.shards) for (int i = 0; i < 3; ++i) g_traffic[i] += sh.traffic[i];
  const double tr_joined = WallMs();
  const int rc = CollectShards(&call, chunks, part_chunks);
  if (rc) {
    for (zamd::Chunk& c : *chunks) c.dev_owner.reset();   // (those of the shards before the failed one: while the contexts are still the call's)
    return rc;
  }
  if (TraceCall()) {
    std::fprintf(stderr, "RunPartsSharded: lease %.2f ms, shards done +%.2f, chunks moved +%.2f\n", tr_lease - tr_begin,
                 tr_joined - tr_begin, WallMs() - tr_begin);
  }
  if (sum) {
    sum->value = sum->kind == ZMX_ADLER32 ? 1u : 0u;   // of no bytes
    for (auto& sh : call.shards) {
      if (sh.sum_bytes) sum->value = zmx_checksum_combine(sum->kind, sum->value, sh.sum, sh.sum_bytes);
    }
  }
  if (dev && dev->finish) {
    const int frc = dev->finish(lease.ctxs[0], chunks, sum ? sum->value : 0);
    if (frc) { dev->error = zmx_last_error(); dev->error_class = zmx_last_error_class(); }
    for (zamd::Chunk& c : *chunks) c.dev_owner.reset();   // (while the contexts are still the call's)
    return frc;
  }
  return 0;
}

// The device layer indexes the positions of a resident input with 32 bits; the reference takes a size_t.  A request
// of more master blocks than ZOPFLI_AMD_ROUND_PARTS (2000: 2 GB, so that a round's shard plus its window stays below
// 2^32 bytes whatever the dealing) is done in ROUNDS, one after the other, each dealt over the contexts like a call of
// its own; master blocks are independent (deflate.c:916-923), their bit chunks are joined in stream order as always,
// and the container checksum of the rounds is put together like that of the shards (zmx_checksum_combine).
int RunPartsSharded(const ZopfliOptions& options, int btype, const unsigned char* in,
                    const std::vector<zamd::Part>& parts, std::vector<zamd::Chunk>* chunks,
                    ChecksumRequest* sum = nullptr, zamd::DeviceInput* dev = nullptr) {
  const size_t round_parts = zamd::HostSwitches().round_parts;
  if (dev) dev->first_part = 0;
  if (parts.size() <= round_parts) return RunPartsShardedOnce(options, btype, in, parts, chunks, sum, nullptr, nullptr, dev);
  uint32_t acc = sum ? (sum->kind == ZMX_ADLER32 ? 1u : 0u) : 0u;   // of no bytes
  for (size_t a = 0; a < parts.size(); a += round_parts) {
    const size_t b = std::min(parts.size(), a + round_parts);
    if (dev) dev->first_part = a;
    const std::vector<zamd::Part> round(parts.begin() + static_cast<long>(a), parts.begin() + static_cast<long>(b));
    ChecksumRequest rs{sum ? sum->kind : 0, sum ? sum->limit : 0, 0};
    const int rc = RunPartsShardedOnce(options, btype, in, round, chunks, sum ? &rs : nullptr, nullptr, nullptr, dev);
    if (rc) return rc;
    if (sum && round.front().instart < sum->limit) {
      const size_t covered = std::min(round.back().inend, sum->limit) - round.front().instart;
      acc = zmx_checksum_combine(sum->kind, acc, rs.value, covered);
    }
  }
  if (sum) sum->value = acc;
  return 0;
}

// Appends merged chunks at (*out, *outsize, *bp), reference conventions.
void EmitChunks(const std::vector<zamd::Chunk>& chunks, const unsigned char* in, unsigned char* bp,
                unsigned char** out, size_t* outsize, bool verbose = false) {
  const size_t before = *outsize;
  zamd::MergeChunks(chunks, in, bp, out, outsize, verbose);
  g_out_traffic[0] += static_cast<double>(*outsize - before);
}

void ResetTiming() {
  zamd::ThreadTiming() = zamd::Timing();
  (void)TakeStats();
  g_traffic[0] = g_traffic[1] = g_traffic[2] = 0;
  for (double& t : g_out_traffic) t = 0;
}

void PushByte(unsigned v, unsigned char** out, size_t* outsize) {
  const uint8_t b = static_cast<uint8_t>(v);
  zamd::AppendToOutput(&b, 1, out, outsize);
}

}  // namespace

// dealing.h: what zmx_compress_batch (batch.cc) shares with the calls above
namespace zamd {
std::vector<Part> InputMasterBlocks(size_t insize, bool final) { return MasterBlocks(insize, final); }
int RunPartsDealt(const ZopfliOptions& options, int btype, const unsigned char* in, const std::vector<Part>& parts,
                  std::vector<Chunk>* chunks, std::vector<size_t>* part_chunks, ShardHooks* hooks, DeviceInput* dev) {
  return RunPartsShardedOnce(options, btype, in, parts, chunks, nullptr, part_chunks, hooks, dev);
}
void ResetCallStats() { ResetTiming(); }
void AddDeviceTraffic(double bytes) { g_traffic[1] += bytes; }
void SetOutputTraffic(const double* t4) { for (int i = 0; i < 4; ++i) g_out_traffic[i] = t4[i]; }
int RunPartsToDevice(const ZopfliOptions& options, const std::vector<Part>& parts, ChecksumRequest* sum, DeviceInput* dev) {
  std::vector<Chunk> chunks;
  return RunPartsShardedOnce(options, 2, nullptr, parts, &chunks, sum, nullptr, nullptr, dev);
}
bool TraceCallOn() { return TraceCall(); }
double CallWallMs() { return WallMs(); }
int OnPooledContext(const std::function<int(zmx_ctx*)>& fn, int only_device) {
  Lease lease(1, 1, false, false, only_device);
  if (lease.ctxs.empty()) {   // (only_device alone: every other call waits or dies in the pool)
    const std::string msg = "device " + std::to_string(only_device) + " is not one of the library's devices (ZOPFLI_AMD_DEVICE, ZOPFLI_AMD_DEVICES)";
    zmx_internal_set_error(msg.c_str(), ZMX_ERR_REFUSED);
    return -1;
  }
  return fn(lease.ctxs[0]);
}
}  // namespace zamd

extern "C" {

size_t zmx_host_cache_trim(void) { return zamd::BlockCache::Trim(); }

void ZopfliInitOptions(ZopfliOptions* options) {
  options->verbose = 0;
  options->verbose_more = 0;
  options->numiterations = 15;
  options->blocksplitting = 1;
  options->blocksplittinglast = 0;
  options->blocksplittingmax = 15;
}

void ZopfliDeflatePart(const ZopfliOptions* options, int btype, int final, const unsigned char* in,
                       size_t instart, size_t inend, unsigned char* bp, unsigned char** out,
                       size_t* outsize) {
  ResetTiming();
  // only in[windowstart, inend) is read (lz77.c:551-552): that becomes the resident input
  std::vector<zamd::Part> parts{{instart, inend, final != 0}};
  std::vector<zamd::Chunk> chunks;
  if (RunPartsSharded(*options, btype, in, parts, &chunks) != 0) Die("device error");
  EmitChunks(chunks, in, bp, out, outsize, options->verbose != 0);
}

}  // extern "C"

namespace {
// The input of a whole-stream call: host bytes, or device memory (`in` is null then).
struct Input {
  const unsigned char* in;
  zamd::DeviceInput* dev;
};

// ZopfliDeflate (deflate.c:908-931); `sum`: see RunPartsSharded; `prefix`: the container's header, appended once the
// parts are done — a call that fails (non-zero, zmx_last_error) leaves *out and *outsize as they were
int DeflateWhole(const ZopfliOptions* options, int btype, int final, const Input& input, size_t insize,
                 const unsigned char* prefix, size_t nprefix, unsigned char* bp, unsigned char** out, size_t* outsize,
                 ChecksumRequest* sum) {
  const unsigned char* in = input.in;
  const size_t offset = *outsize + nprefix;
  {
    const double tr0 = WallMs();
    ResetTiming();
    const std::vector<zamd::Part> parts = MasterBlocks(insize, final != 0);
    std::vector<zamd::Chunk> chunks;
    const double tr1 = WallMs();
    if (const int rc = RunPartsSharded(*options, btype, in, parts, &chunks, sum, input.dev)) return rc;
    const double tr2 = WallMs();
    if (nprefix) zamd::AppendToOutput(prefix, nprefix, out, outsize);
    g_out_traffic[0] += static_cast<double>(nprefix);
    EmitChunks(chunks, in, bp, out, outsize, options->verbose != 0);
    const double tr3 = WallMs();
    chunks.clear();
    chunks.shrink_to_fit();
    if (TraceCall()) {
      std::fprintf(stderr, "DeflateWhole: set-up %.2f ms, parts %.2f, merge %.2f, chunks freed %.2f\n", tr1 - tr0, tr2 - tr1,
                   tr3 - tr2, WallMs() - tr3);
    }
  }
  if (options->verbose) {
    std::fprintf(stderr, "Original Size: %lu, Deflate: %lu, Compression: %f%% Removed\n",
                 static_cast<unsigned long>(insize), static_cast<unsigned long>(*outsize - offset),
                 100.0 * static_cast<double>(insize - (*outsize - offset)) / static_cast<double>(insize));
  }
  return 0;
}

int GzipFrom(const ZopfliOptions* options, const Input& input, size_t insize, unsigned char** out, size_t* outsize) {
  // the CRC is taken on the device(s) from the resident input (zmx_checksum)
  ChecksumRequest sum{ZMX_CRC32, insize, 0};
  unsigned char bp = 0;
  static const unsigned char header[10] = {31, 139, 8, 0, 0, 0, 0, 0, 2, 3};  // gzip_container.c:90-101
  if (const int rc = DeflateWhole(options, 2, 1, input, insize, header, 10, &bp, out, outsize, &sum)) return rc;
  const uint32_t crc = sum.value;
  for (int i = 0; i < 4; ++i) PushByte((crc >> (8 * i)) & 255, out, outsize);
  for (int i = 0; i < 4; ++i) PushByte((insize >> (8 * i)) & 255, out, outsize);
  g_out_traffic[0] += 8;
  if (options->verbose) {
    std::fprintf(stderr, "Original Size: %d, Gzip: %d, Compression: %f%% Removed\n", static_cast<int>(insize),
                 static_cast<int>(*outsize), 100.0 * static_cast<double>(insize - *outsize) / static_cast<double>(insize));
  }
  return 0;
}

int ZlibFrom(const ZopfliOptions* options, const Input& input, size_t insize, unsigned char** out, size_t* outsize) {
  // the reference truncates the size to unsigned here (zlib_container.c:54)
  ChecksumRequest sum{ZMX_ADLER32, static_cast<unsigned>(insize), 0};
  unsigned char bp = 0;
  const unsigned cmf = 120, flevel = 3, fdict = 0;  // CM 8, CINFO 7
  unsigned cmfflg = 256 * cmf + fdict * 32 + flevel * 64;
  cmfflg += 31 - cmfflg % 31;
  const unsigned char header[2] = {static_cast<unsigned char>(cmfflg / 256), static_cast<unsigned char>(cmfflg % 256)};
  if (const int rc = DeflateWhole(options, 2, 1, input, insize, header, 2, &bp, out, outsize, &sum)) return rc;
  const uint32_t checksum = sum.value;
  for (int i = 3; i >= 0; --i) PushByte((checksum >> (8 * i)) & 255, out, outsize);
  g_out_traffic[0] += 4;
  if (options->verbose) {
    std::fprintf(stderr, "Original Size: %d, Zlib: %d, Compression: %f%% Removed\n", static_cast<int>(insize),
                 static_cast<int>(*outsize), 100.0 * static_cast<double>(insize - *outsize) / static_cast<double>(insize));
  }
  return 0;
}
}  // namespace

namespace zamd {
int CompressFromDevice(const ZopfliOptions* options, ZopfliFormat output_type, DeviceInput* dev, size_t insize,
                       unsigned char** out, size_t* outsize) {
  const Input input{nullptr, dev};
  if (output_type == ZOPFLI_FORMAT_GZIP) return GzipFrom(options, input, insize, out, outsize);
  if (output_type == ZOPFLI_FORMAT_ZLIB) return ZlibFrom(options, input, insize, out, outsize);
  unsigned char bp = 0;
  return DeflateWhole(options, 2, 1, input, insize, nullptr, 0, &bp, out, outsize, nullptr);
}
}  // namespace zamd

extern "C" {

void ZopfliDeflate(const ZopfliOptions* options, int btype, int final, const unsigned char* in,
                   size_t insize, unsigned char* bp, unsigned char** out, size_t* outsize) {
  if (DeflateWhole(options, btype, final, Input{in, nullptr}, insize, nullptr, 0, bp, out, outsize, nullptr) != 0) Die("device error");
}

void ZopfliGzipCompress(const ZopfliOptions* options, const unsigned char* in, size_t insize,
                        unsigned char** out, size_t* outsize) {
  if (GzipFrom(options, Input{in, nullptr}, insize, out, outsize) != 0) Die("device error");
}

void ZopfliZlibCompress(const ZopfliOptions* options, const unsigned char* in, size_t insize,
                        unsigned char** out, size_t* outsize) {
  if (ZlibFrom(options, Input{in, nullptr}, insize, out, outsize) != 0) Die("device error");
}

void ZopfliCompress(const ZopfliOptions* options, ZopfliFormat output_type, const unsigned char* in,
                    size_t insize, unsigned char** out, size_t* outsize) {
  if (output_type == ZOPFLI_FORMAT_GZIP) {
    ZopfliGzipCompress(options, in, insize, out, outsize);
  } else if (output_type == ZOPFLI_FORMAT_ZLIB) {
    ZopfliZlibCompress(options, in, insize, out, outsize);
  } else if (output_type == ZOPFLI_FORMAT_DEFLATE) {
    unsigned char bp = 0;
    ZopfliDeflate(options, 2, 1, in, insize, &bp, out, outsize);
  } else {
    std::fprintf(stderr, "zopfli_amd: invalid ZopfliFormat %d\n", static_cast<int>(output_type));
    std::abort();  // the reference asserts (zopfli_lib.c:40)
  }
}

int zmx_deflate_range(zmx_ctx* ctx, const ZopfliOptions* options, size_t instart, size_t inend, int final,
                      unsigned char** blob, size_t* blobsize) {
  MaybeKeepHeap();
  ResetTiming();
  if (inend < instart || inend > zmx_internal_input_size(ctx)) return -1;
  // deflate.c:916-923 on [instart, inend)
  std::vector<zamd::Part> parts;
  size_t i = instart;
  do {
    const bool masterfinal = i + kMasterBlock >= inend;
    const size_t size = masterfinal ? inend - i : kMasterBlock;
    parts.push_back({i, i + size, final != 0 && masterfinal});
    i += size;
  } while (i < inend);
  std::vector<zamd::Chunk> chunks;
  const auto tr0 = std::chrono::steady_clock::now();
  const int rc = RunParts(ctx, *options, 2, parts, &chunks);
  if (rc) return rc;
  const auto ts0 = std::chrono::steady_clock::now();
  if (zamd::HostSwitches().prof)
    std::fprintf(stderr, "zmx_deflate_range: RunParts %.1f ms\n", std::chrono::duration<double>(ts0 - tr0).count() * 1e3);
  const unsigned char* host = zmx_internal_input_host(ctx);
  // (an input set from device memory: the host has no copy, the stored blocks bring their bytes)
  if (!host && FetchStoredBytes(ctx, &chunks, &g_traffic[2]) != 0) return -1;
  *blob = zamd::SerializeChunks(chunks, host, blobsize);
  if (!*blob) return -1;
  zamd::ThreadTiming().serialize += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts0).count();
  return 0;
}

int zmx_chunks_merge(const unsigned char* const* blobs, const size_t* blobsizes, size_t nblobs,
                     unsigned char* bp, unsigned char** out, size_t* outsize) {
  std::vector<zamd::Chunk> chunks;
  for (size_t i = 0; i < nblobs; ++i) {
    if (!zamd::DeserializeChunks(blobs[i], blobsizes[i], &chunks)) return -1;
  }
  EmitChunks(chunks, nullptr, bp, out, outsize);
  return 0;
}

int zmx_last_timing(double* out8) {
  const zamd::Timing& t = zamd::ThreadTiming();
  out8[0] = t.tables;
  out8[1] = t.greedy;
  out8[2] = t.squeeze;
  out8[3] = t.cost_model;
  out8[4] = t.split;
  out8[5] = t.encode;
  const zmx_stats& s = zamd::ThreadStats();
  out8[6] = s.kernel_seconds[1];
  out8[7] = s.squeeze_launches;
  return 0;
}

int zmx_last_kernel_timing(double* out4) {
  const zmx_stats& s = zamd::ThreadStats();
  for (int i = 0; i < 3; ++i) out4[i] = s.kernel_seconds[i];
  out4[3] = s.squeeze_launches;
  return 0;
}

int zmx_last_match_timing(double* out4) {
  const zmx_stats& s = zamd::ThreadStats();
  for (int i = 0; i < 4; ++i) out4[i] = s.match[i];
  return 0;
}

int zmx_last_match_walk(double* out3) {
  const zmx_stats& s = zamd::ThreadStats();
  for (int i = 0; i < 3; ++i) out3[i] = s.match5[i];
  return 0;
}

int zmx_last_seg_stats(double* out8) {
  const zmx_stats& s = zamd::ThreadStats();
  for (int i = 0; i < ZMX_SEG_N; ++i) out8[i] = s.seg[i];   // (ZMX_SEG_N = the 8 of the public header)
  return 0;
}

int zmx_last_input_traffic(double* out3) {
  for (int i = 0; i < 3; ++i) out3[i] = g_traffic[i];
  return 0;
}

int zmx_last_output_traffic(double* out4) {
  for (int i = 0; i < 4; ++i) out4[i] = g_out_traffic[i];
  return 0;
}

int zmx_last_host_timing(double* out2) {
  out2[0] = zamd::ThreadTiming().download;
  out2[1] = zamd::ThreadTiming().serialize;
  return 0;
}

// deflate.h:79,85 on the reference's own store type (lz77.h:44-62): the histogram of the range from litlens / dists,
// its byte length from pos (lz77.c:160-166), then the block-cost code of the library (host/block_cost.cc)
namespace {
zamd::Histogram RangeHistogram(const ZopfliLZ77Store* lz77, size_t lstart, size_t lend) {
  zamd::Histogram h;
  h.Clear();
  for (size_t i = lstart; i < lend; ++i) {
    if (lz77->dists[i] == 0) {
      h.ll[lz77->litlens[i]]++;
    } else {
      h.ll[zamd::LengthSymbol(lz77->litlens[i])]++;
      h.d[zamd::DistSymbol(lz77->dists[i])]++;
    }
  }
  return h;
}
double StoredSize(const ZopfliLZ77Store* lz77, size_t lstart, size_t lend) {
  size_t length = 0;
  if (lstart != lend) {
    const size_t l = lend - 1;
    length = lz77->pos[l] + (lz77->dists[l] == 0 ? 1 : lz77->litlens[l]) - lz77->pos[lstart];
  }
  const size_t rem = length % 65535;
  const size_t blocks = length / 65535 + (rem ? 1 : 0);
  return static_cast<double>(blocks * 5 * 8 + length * 8);      // deflate.c:591-597
}
}  // namespace

double ZopfliCalculateBlockSize(const ZopfliLZ77Store* lz77, size_t lstart, size_t lend, int btype) {
  if (btype == 0) return StoredSize(lz77, lstart, lend);
  return zamd::BlockSizeFromHistogram(RangeHistogram(lz77, lstart, lend), btype);
}

double ZopfliCalculateBlockSizeAutoType(const ZopfliLZ77Store* lz77, size_t lstart, size_t lend) {
  const double stored = StoredSize(lz77, lstart, lend);
  const zamd::Histogram h = RangeHistogram(lz77, lstart, lend);
  const double fixed = lz77->size > 1000 ? stored : zamd::BlockSizeFromHistogram(h, 1);   // deflate.c:614-616
  const double dynamic = zamd::BlockSizeFromHistogram(h, 2);
  return (stored < fixed && stored < dynamic) ? stored : (fixed < dynamic ? fixed : dynamic);
}

// zopflipng's per-row filter search on one of the entry points' contexts (include/zopfli_amd.h)
int zmx_png_filter_types_pooled(const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                                unsigned char* minsum_types, unsigned char* entropy_types) {
  Lease lease(1);
  return zmx_png_filter_types(lease.ctxs[0], image, linebytes, height, bytewidth, minsum_types, entropy_types);
}

}  // extern "C"
