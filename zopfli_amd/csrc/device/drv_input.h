// Driver part: the resident input (CopyInput, zmx_set_input*, segments), CheckDevicePointer, DeviceRangeChecker, the zmx_internal_*
// seam, the probe counts, zmx_gather_device, zmx_master_block_costs_device.  Needs drv_context.h (zmx_ctx, PoolScope, KernelTiming).
#pragma once

constexpr size_t kInputPad = 4096;

extern "C" {
// ---- the seam to the host layer (host/zmx_internal.h says what each does)
size_t zmx_internal_input_size(zmx_ctx* ctx) { return ctx->insize; }
int zmx_internal_device(zmx_ctx* ctx) { return ctx->device; }
void zmx_internal_set_error(const char* msg, int cls) { g_err = msg; g_err_class = cls; }
const unsigned char* zmx_internal_input_host(zmx_ctx* ctx) { return ctx->h_in; }
void zmx_internal_pool_stats(zmx_ctx* ctx, uint64_t out[8]) { ctx->pool.Stats(out); }

// `insize` bytes at `src` become the context's resident input: its own copy, kInputPad zero bytes behind it.
static int CopyInput(zmx_ctx* c, const void* src, size_t insize, hipMemcpyKind kind) {
  DEVICE_ENTRY(c->device);
  if (insize + kInputPad > c->in_cap) {
    PoolFree(c, c->d_in);
    c->d_in = nullptr;
    c->in_cap = insize + kInputPad;
    HIPCHK(PoolAllocT(c, &c->d_in, c->in_cap, "d_in"));
  }
  if (insize) HIPCHK(hipMemcpyAsync(c->d_in, src, insize, kind, c->stream));
  HIPCHK(hipMemsetAsync(c->d_in + insize, 0, kInputPad, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->insize = insize;
  c->h_in = nullptr;
  c->seg_starts.clear();
  return 0;
}

int zmx_set_input(zmx_ctx* c, const unsigned char* in, size_t insize) {
  if (const int rc = CopyInput(c, in, insize, hipMemcpyHostToDevice)) return rc;
  c->h_in = in;
  return 0;
}

// [p, p + n) must be plain device memory: what the copy engines and a kernel of the pointer's device read without the
// host's help.  Refused before any copy or launch: a null pointer, host memory (registered or not), managed memory
// (its pages may live on the host: reading them depends on XNACK), a range that leaves its allocation.
// *device: the HIP device the memory lies on (-1 for n = 0, where any pointer goes).
// (alloc_lo, alloc_size: optional, the allocation the range lies in)
static int CheckDevicePointer(const char* who, const void* p, size_t n, int* device, uintptr_t* alloc_lo = nullptr,
                              size_t* alloc_size = nullptr) {
  *device = -1;
  if (n == 0) return 0;
  const std::string w(who);
  if (p == nullptr) return FailMsg(w + ": null pointer with a non-zero size");
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();   // (a pointer the runtime has never seen: not an error of the device)
    return FailMsg(w + ": the pointer is not device memory");
  }
  if (a.isManaged || a.type == hipMemoryTypeManaged) return FailMsg(w + ": managed memory is not taken (copy it to device memory)");
  if (a.type != hipMemoryTypeDevice) return FailMsg(w + ": the pointer is not device memory");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return FailMsg(w + ": the pointer's allocation is unknown");
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), at = reinterpret_cast<uintptr_t>(p);
  if (at < lo || at - lo > size || n > size - (at - lo)) return FailMsg(w + ": the range leaves its allocation");
  *device = a.device;
  if (alloc_lo) *alloc_lo = lo;
  if (alloc_size) *alloc_size = size;
  return 0;
}

// CheckDevicePointer for the ranges of a list: the runtime is asked once for consecutive ranges of one allocation
// (slices of a tensor, the tensors of one arena).
struct DeviceRangeChecker {
  uintptr_t lo = 0;
  size_t size = 0;
  int device = -1;
  int Check(const char* who, const void* p, size_t n, int* device_out) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(p);
    if (n != 0 && size != 0 && at >= lo && at - lo <= size && n <= size - (at - lo)) {
      *device_out = device;
      return 0;
    }
    uintptr_t l = 0;
    size_t s = 0;
    if (const int rc = CheckDevicePointer(who, p, n, device_out, &l, &s)) return rc;
    if (n != 0) { lo = l; size = s; device = *device_out; }
    return 0;
  }
};

int zmx_internal_device_pointer(const char* who, const void* p, size_t n, int* device) {
  return CheckDevicePointer(who, p, n, device);
}

int zmx_internal_device_pointers(const char* who, size_t n, const void* const* p, const size_t* nbytes) {
  DeviceRangeChecker checker;
  int device = -1;
  for (size_t i = 0; i < n; ++i) {
    if (const int rc = checker.Check(who, p[i], nbytes[i], &device)) return rc;
  }
  return 0;
}

int zmx_internal_device_pointers_one_device(const char* who, size_t n, const void* const* p, const size_t* nbytes, int* device) {
  DeviceRangeChecker checker;
  *device = -1;
  for (size_t i = 0; i < n; ++i) {
    const std::string w = std::string(who) + ": range " + std::to_string(i);
    if (nbytes[i] != 0 && p[i] == nullptr) return FailMsg(w + ": null pointer with a non-zero size");
    int at = -1;
    if (const int rc = checker.Check(w.c_str(), p[i], nbytes[i], &at)) return rc;
    if (at < 0) continue;
    if (*device >= 0 && at != *device) return FailMsg(w + " lies on another device than the ranges before it");
    *device = at;
  }
  return 0;
}

int zmx_internal_device_alloc(int device, size_t n, void** p) {
  *p = nullptr;
  DEVICE_ENTRY(device);
  HIPCHK(hipMalloc(p, n ? n : 1));
  return 0;
}

void zmx_internal_device_free(int device, void* p) {
  if (!p) return;
  DeviceGuard dev_guard(device);
  (void)hipFree(p);
}

int zmx_internal_device_copy(int device, void* d_dst, const void* d_src, size_t n) {
  if (n == 0) return 0;
  DEVICE_ENTRY(device);
  HIPCHK(hipMemcpy(d_dst, d_src, n, hipMemcpyDeviceToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));   // (a copy within one device may return before it is done; the source is freed next)
  return 0;
}

int zmx_set_input_device(zmx_ctx* c, const void* d_in, size_t insize) {
  int device = -1;
  if (const int rc = CheckDevicePointer("zmx_set_input_device", d_in, insize, &device)) return rc;
  // (hipMemcpyDefault: the runtime finds the source's device itself — a peer copy where it is another one)
  return CopyInput(c, d_in, insize, hipMemcpyDefault);
}

int zmx_internal_input_fetch(zmx_ctx* c, size_t begin, size_t end, unsigned char* dst) {
  if (begin > end || end > c->insize) return FailMsg("zmx_internal_input_fetch: range outside the resident input");
  if (begin == end) return 0;
  DEVICE_ENTRY(c->device);
  HIPCHK(hipMemcpyAsync(dst, c->d_in + begin, end - begin, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int zmx_internal_probe_counts(zmx_ctx* c, const void* bytes, size_t n, const uint64_t* ranges, uint32_t* counts) {
  if (n == 0) return 0;
  if (n > 65535) return FailMsg("zmx_internal_probe_counts: too many ranges for one launch");
  u64 longest = 0;
  for (size_t r = 0; r < n; ++r) {
    if (bytes == nullptr && (ranges[2 * r] > ranges[2 * r + 1] || ranges[2 * r + 1] > c->insize)) {
      return FailMsg("zmx_internal_probe_counts: range outside the resident input");
    }
    longest = std::max<u64>(longest, zamd::ProbeCount(ranges[2 * r], ranges[2 * r + 1]));
  }
  std::memset(counts, 0, n * zamd::kProbeCounts * sizeof(uint32_t));
  if (longest == 0) return 0;
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  uint64_t* d_ranges = nullptr;
  uint32_t* d_counts = nullptr;
  HIPCHK(tmp.Upload(&d_ranges, ranges, 2 * n, "d_ranges"));
  HIPCHK(tmp.AllocT(&d_counts, n * zamd::kProbeCounts, "d_counts"));
  HIPCHK(hipMemsetAsync(d_counts, 0, n * zamd::kProbeCounts * sizeof(uint32_t), c->stream));
  ProbeParams P;
  P.in = bytes ? static_cast<const unsigned char*>(bytes) : c->d_in;
  P.ranges = d_ranges;
  P.counts = d_counts;
  const unsigned gx = static_cast<unsigned>(std::min<u64>((longest + 255) / 256, 64));
  hipLaunchKernelGGL(k_probe_counts, dim3(gx, static_cast<unsigned>(n)), dim3(256), 0, c->stream, P);
  KCHK(c, "k_probe_counts");
  HIPCHK(hipMemcpyAsync(counts, d_counts, n * zamd::kProbeCounts * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

static thread_local double g_gather_ms = 0;   // (zmx_internal_gather_ms)
double zmx_internal_gather_ms(void) { return g_gather_ms; }

int zmx_gather_device(zmx_ctx* c, size_t n, const void* const* d_src, const size_t* nbytes, void* d_dst) {
  g_gather_ms = 0;
  if (n == 0) return 0;
  if (!d_src || !nbytes) return FailMsg("zmx_gather_device: null array");
  std::vector<uint64_t> start(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if (nbytes[i] > SIZE_MAX - start[i]) return FailMsg("zmx_gather_device: the sizes overflow");
    start[i + 1] = start[i] + nbytes[i];
  }
  const uint64_t total = start[n];
  // ---- every range checked before anything is copied
  int dst_device = -1;
  if (const int rc = CheckDevicePointer("zmx_gather_device", d_dst, total, &dst_device)) return rc;
  DeviceRangeChecker checker;
  std::vector<const unsigned char*> src(n, nullptr);   // the kernel's pieces: those on the context's device
  std::vector<size_t> foreign;                         // the others: a copy each
  size_t local = 0;
  const uintptr_t dlo = reinterpret_cast<uintptr_t>(d_dst);
  for (size_t i = 0; i < n; ++i) {
    int device = -1;
    if (const int rc = checker.Check("zmx_gather_device", d_src[i], nbytes[i], &device)) return rc;
    if (nbytes[i] == 0) continue;
    const uintptr_t slo = reinterpret_cast<uintptr_t>(d_src[i]);
    if (slo < dlo + total && dlo < slo + nbytes[i]) return FailMsg("zmx_gather_device: the destination overlaps a source");
    if (device == c->device) { src[i] = static_cast<const unsigned char*>(d_src[i]); ++local; }
    else foreign.push_back(i);
  }
  if (total == 0) return 0;
  if (dst_device != c->device) return FailMsg("zmx_gather_device: the destination is not memory of the context's device");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (the table: held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  const auto enqueue = [&]() -> int {
    if (timed && local == 0) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    if (local != 0) {
      const unsigned char** d_ptrs = nullptr;
      uint64_t* d_start = nullptr;
      HIPCHK(tmp.Upload(&d_ptrs, src.data(), n, "gather_src"));
      HIPCHK(tmp.Upload(&d_start, start.data(), n + 1, "gather_start"));
      zamd::GatherTable T;
      T.src = d_ptrs;
      T.start = d_start;
      T.dst = static_cast<unsigned char*>(d_dst);
      T.n = n;
      // (the grid: tiles of the destination up to the cap, whatever n and the total)
      const uint64_t ntiles = (total + zamd::kGatherTile - 1) / zamd::kGatherTile;
      const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(ntiles, zamd::kGatherMaxBlocks));
      if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
      hipLaunchKernelGGL(k_gather, dim3(grid), dim3(zamd::kGatherThreads), 0, c->stream, T, ntiles);
      KCHK(c, "k_gather");
    }
    for (const size_t i : foreign) {
      HIPCHK(hipMemcpyAsync(static_cast<unsigned char*>(d_dst) + start[i], d_src[i], nbytes[i], hipMemcpyDefault, c->stream));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    return 0;
  };
  if (const int rc = enqueue()) {
    // what was queued before the failure may still read the table: drained before `tmp` gives it back (the failure's
    // message and class stay as they are)
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_gather_ms = ms;
  }
  return 0;
}

int zmx_master_block_costs_device(zmx_ctx* c, double* cost, size_t ncost) {
  const size_t kMb = 1000000;   // ZOPFLI_MASTER_BLOCK_SIZE, util.h:60
  const size_t n = c->insize == 0 ? 1 : (c->insize + kMb - 1) / kMb;
  if (ncost < n) return -1;
  if (n > 65535) return FailMsg("zmx_master_block_costs_device: more than 65535 master blocks");
  std::vector<uint64_t> ranges(2 * n);
  for (size_t b = 0; b < n; ++b) {
    ranges[2 * b] = b * kMb;
    ranges[2 * b + 1] = std::min(c->insize, (b + 1) * kMb);
  }
  std::vector<uint32_t> counts(n * zamd::kProbeCounts);
  if (const int rc = zmx_internal_probe_counts(c, nullptr, n, ranges.data(), counts.data())) return rc;
  for (size_t b = 0; b < n; ++b) {
    const uint32_t* k = &counts[b * zamd::kProbeCounts];
    cost[b] = zamd::CostFromCounts(ranges[2 * b + 1] - ranges[2 * b], k[zamd::kProbes], k[zamd::kRuns], k[zamd::kFew]);
  }
  return static_cast<int>(n);
}

// The resident input is the concatenation of independent inputs: a block's window stops at the first byte of its own
// input instead of reaching 32 KiB into the one before it (BuildTables).  Every kernel works on [ws, inend) with link
// indices relative to ws, so a floor on ws is all the rest needs.
int zmx_set_input_segments(zmx_ctx* c, const uint64_t* starts, size_t nseg) {
  if (nseg == 0 || starts == nullptr) return FailMsg("zmx_set_input_segments: no segments");
  if (starts[0] != 0) return FailMsg("zmx_set_input_segments: the first segment must start at 0");
  for (size_t i = 0; i < nseg; ++i) {
    if (starts[i] > c->insize) return FailMsg("zmx_set_input_segments: a segment starts past the end of the input");
    if (i && starts[i] < starts[i - 1]) return FailMsg("zmx_set_input_segments: segment starts must not decrease");
  }
  c->seg_starts.assign(starts, starts + nseg);
  if (nseg == 1) c->seg_starts.clear();
  return 0;
}
}  // extern "C"
