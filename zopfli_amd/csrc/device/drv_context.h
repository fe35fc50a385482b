// Driver part: zmx_ctx (device, streams, events, pool, staging), PoolAllocT, PoolScope, PoolFree, PinnedGive, StageReserve,
// create / destroy / priority / share / trim, the match-kernel, match-order and kernel-timing setters.  Needs drv_errors.h, zmx_pool.h.
#pragma once

struct zmx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  u8* d_in = nullptr;
  size_t insize = 0, in_cap = 0;
  const unsigned char* h_in = nullptr;  // caller's buffer (borrowed until the next zmx_set_input); null: the input came from device memory (zmx_set_input_device)
  std::vector<u64> seg_starts;          // zmx_set_input_segments: first byte of each independent input (empty: one input)
  u32* d_scratch = nullptr;  // k_match2 per-lane overflow change points
  u32* d_scratch5 = nullptr; // k_match5's (it may run beside k_match2)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream2 = nullptr;   // the run tasks' k_dp5_spec beside the others' (zmx_squeeze_run)
  bool stream2_outstanding = false;   // a kernel on stream2 reads pooled scratch arrays and `stream` has not been made to wait for it yet
  hipStream_t alt_stream[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};   // zmx_ctx_set_priority: [0] the created pair, [1] high, [2] low
  hipEvent_t ev2[2] = {nullptr, nullptr};
  u32* h_stage = nullptr;    // pinned staging for store downloads (grow-only)
  size_t stage_cap = 0;      // in u32
  size_t code_budget = 0;    // what one batch's DP edges may take (BuildDpRows): a third of the device's memory (hipMemGetInfo at creation), at most 96 GiB
  DevicePool pool;           // every device array and pinned buffer of the context (zmx_pool.h)
};

namespace {

constexpr size_t kPoolKeepMax = 96ull << 30;

template <typename T>
hipError_t PoolAllocT(zmx_ctx* c, T** p, size_t n, const char* tag) {
  return c->pool.Alloc(reinterpret_cast<void**>(p), (n ? n : 1) * sizeof(T), tag, c->stream);
}
#define PoolAlloc(c, p, n) PoolAllocT(c, p, n, #p)

// Which match-table kernel (ZOPFLI_AMD_MATCH / zmx_set_match_kernel):
//   0 (default) per block: k_hits estimates the hits per position of the reference's walk; blocks above
//       ZOPFLI_AMD_MATCH_HITS (300) take the exact skip-walk k_match5 (level links + counted hits, zmx_match5.h: 5 - 9 x
//       faster on PNG-like and two-symbol data, profiles/r04_match.txt), the others k_match2, side by side on two streams
//   2 = k_chain + k_match2 everywhere (prev links, a lane per position)
//   5 = k_match5 everywhere
// All produce the same records (test_match_kernels_agree).  Tables built from a parent recompute their few tiles with
// k_match2 either way.
std::atomic<int> g_match_kernel{-1};
int MatchKernel() {
  const int v = g_match_kernel.load(std::memory_order_relaxed);
  return v < 0 ? Knobs().match : v;      // (the setter's choice, else the environment's)
}
// k_match2 hands out a tile's positions longest walk first, by k_hits' estimates (ZOPFLI_AMD_MATCH_ORDER /
// zmx_set_match_order; 0 = in ascending order).  Whole builds only: a table built from a parent recomputes a few
// tiles, for which nobody runs k_hits.
std::atomic<int> g_match_order{-1};
bool MatchOrder() {
  const int v = g_match_order.load(std::memory_order_relaxed);
  return v < 0 ? Knobs().match_order : v != 0;
}

// Temporary arrays of one call: back to the pool when the call returns, whichever way (HIPCHK returns early).
struct PoolScope {
  zmx_ctx* c;
  std::vector<void*> held;
  explicit PoolScope(zmx_ctx* ctx) : c(ctx) {}
  ~PoolScope();
  template <typename T>
  hipError_t AllocT(T** p, size_t n, const char* tag) {
    const hipError_t e = PoolAllocT(c, p, n, tag);
    if (e == hipSuccess) held.push_back(*p);
    return e;
  }
  // AllocT, and the n elements at `host` on their way into it, on the context's stream (n = 0: nothing to copy)
  template <typename T>
  hipError_t Upload(T** p, const T* host, size_t n, const char* tag) {
    const hipError_t e = AllocT(p, n, tag);
    return e != hipSuccess || n == 0 ? e : hipMemcpyAsync(*p, host, n * sizeof(T), hipMemcpyHostToDevice, c->stream);
  }
};

// (zmx_tables_free without a context: straight back to the device)
void PoolFree(zmx_ctx* c, void* p) {
  if (c) c->pool.Free(p);
  else if (p) (void)hipFree(p);
}

PoolScope::~PoolScope() {
  // (an error return between a launch on stream2 and the join: the kernel may still be reading these arrays)
  if (c->stream2_outstanding) {
    (void)hipStreamSynchronize(c->stream2);
    c->stream2_outstanding = false;
  }
  for (void* p : held) PoolFree(c, p);
}

}  // namespace

extern "C" {
int zmx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// The phase times of a squeeze run (k_wtab / the chain / the trace: zmx_last_kernel_timing, zmx_last_timing's dp_kernel)
// are four event records and three readings a run — seven of a run's ~22 runtime calls, which is what sixteen concurrent
// callers of small files queue for.  Off unless somebody asks: ZOPFLI_AMD_KERNEL_TIMING=1, ZOPFLI_AMD_PROF, or this call
// (bench.py, tools/latency.py and the tests' harness do).
static std::atomic<int> g_kernel_timing{-1};
static bool KernelTiming() {
  const int v = g_kernel_timing.load(std::memory_order_relaxed);
  return v < 0 ? Knobs().kernel_timing : v != 0;
}
void zmx_set_kernel_timing(int on) { g_kernel_timing.store(on ? 1 : 0, std::memory_order_relaxed); }

int zmx_has_experiments(void) { return 0; }   // (always 0; kept for ABI)

void zmx_set_oom_hook(zmx_oom_hook_t hook) { DevicePool::SetOomHook(hook); }

// Keeps nothing: the budgets are per DEVICE, whoever uses them (zmx_pool.h), and no context needs to know how many share
// its device.  Kept for the ABI.
int zmx_ctx_set_share(zmx_ctx* c, unsigned /*contexts_on_device*/) {
  if (!c) return FailMsg("zmx_ctx_set_share: no context");
  return 0;
}

int zmx_ctx_trim_cache(zmx_ctx* c) {
  if (!c) return 0;
  DEVICE_ENTRY(c->device);
  c->pool.DropCache();
  return 0;
}

int zmx_set_match_kernel(int kernel) {
  if (kernel == 3 || kernel == 4) return FailMsg("zmx_set_match_kernel: kernels 3 and 4 were removed");
  if (kernel != 0 && kernel != 2 && kernel != 5) return FailMsg("zmx_set_match_kernel: 0, 2 or 5");
  g_match_kernel.store(kernel, std::memory_order_relaxed);
  return 0;
}

int zmx_set_match_order(int on) {
  g_match_order.store(on != 0 ? 1 : 0, std::memory_order_relaxed);
  return 0;
}

// (no context: as PoolFree)
static void PinnedGive(zmx_ctx* c, unsigned char** p, size_t cap) {
  if (!*p) return;
  if (c) c->pool.PinnedGive(*p, cap);
  else (void)hipHostFree(*p);
  *p = nullptr;
}

// The streams, events and budgets of a new context, on its device.
static int InitContext(zmx_ctx* c) {
  HIPCHK(hipStreamCreate(&c->stream));
  for (int i = 0; i < 4; ++i) HIPCHK(hipEventCreate(&c->ev[i]));
  HIPCHK(hipStreamCreate(&c->stream2));
  for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev2[i], hipEventDisableTiming));
  {
    // Budgets from what the device has, not from what an MI355X has on paper: several contexts may share one
    // device (ZOPFLI_AMD_DEVICES=0,0), other processes may hold memory already.
    size_t mem_free = 0, mem_total = 0;
    HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
    c->code_budget = std::min<size_t>(kPoolKeepMax, mem_free / 3);
    c->pool.Init(c->device, c->code_budget);
  }

  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain), hipFuncAttributeMaxDynamicSharedMemorySize,
                             CH_LDS_BYTES));
  return 0;
}

int zmx_ctx_create(int device, zmx_ctx** out) {
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return FailMsg("zmx_ctx_create: no such HIP device");
  DEVICE_ENTRY(device);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    return FailMsg(std::string("zmx_ctx_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  }
  zmx_ctx* c = new zmx_ctx();
  c->device = device;
  const int rc = InitContext(c);
  if (rc != 0) {
    zmx_ctx_destroy(c);   // (what InitContext made so far; the error it reported stays)
    return rc;
  }
  *out = c;
  return 0;
}

// Which streams the context's next calls run on: level 0 = the pair it was created with, +1 / -1 = a pair of the highest /
// lowest priority the device has (made when first asked for).  A call with block splitting that is dealt over the three
// contexts of a device gives them three priorities (api.cc): the contexts then run one AFTER the other where they would
// share the device evenly, so their host phases — the split searches, the joins — come at different times and fall beside
// the others' kernels instead of beside each other (100 MB of text: 152 -> 145 ms); without block splitting there is
// little host work to hide and running in turn only costs the overlap of the kernels' tails (123 -> 130 ms), so such
// calls stay on level 0.  Only between calls: the context must be idle.
int zmx_ctx_set_priority(zmx_ctx* c, int level) {
  DEVICE_ENTRY(c->device);
  const int k = level > 0 ? 1 : level < 0 ? 2 : 0;
  // (first: from here on zmx_ctx_destroy frees by alt_stream[][], a pair created half-way below included)
  if (!c->alt_stream[0][0]) { c->alt_stream[0][0] = c->stream; c->alt_stream[0][1] = c->stream2; }   // the pair of zmx_ctx_create
  if (k && !c->alt_stream[k][1]) {
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (int i = 0; i < 2; ++i) {
      if (c->alt_stream[k][i]) continue;      // (an earlier call got this far)
      HIPCHK(hipStreamCreateWithPriority(&c->alt_stream[k][i], hipStreamDefault, k == 1 ? greatest : least));
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream2));
  c->stream = c->alt_stream[k][0];
  c->stream2 = c->alt_stream[k][1];
  return 0;
}

void zmx_ctx_destroy(zmx_ctx* c) {
  if (!c) return;
  DeviceGuard dev_guard(c->device);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  c->pool.ReleaseAll();   // (the input and k_match2's scratch are pooled allocations too)
  for (int i = 0; i < 4; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  for (int i = 0; i < 2; ++i) if (c->ev2[i]) (void)hipEventDestroy(c->ev2[i]);
  if (c->alt_stream[0][0]) {       // (stream / stream2 are one of these pairs)
    for (int k = 0; k < 3; ++k) for (int i = 0; i < 2; ++i) if (c->alt_stream[k][i]) (void)hipStreamDestroy(c->alt_stream[k][i]);
  } else {
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  delete c;
}

// The pinned staging buffer of a context holds at least `words` u32 (grow-only, with a quarter to spare).
static int StageReserve(zmx_ctx* c, size_t words) {
  if (words <= c->stage_cap) return 0;
  if (c->h_stage) HIPCHK(hipHostFree(c->h_stage));
  c->h_stage = nullptr;
  c->stage_cap = 0;
  const size_t cap = words + words / 4 + 16;
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->h_stage), cap * sizeof(u32), hipHostMallocDefault));
  c->stage_cap = cap;
  return 0;
}
}  // extern "C"
