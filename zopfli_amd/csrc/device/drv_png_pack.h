// zmx_hip.hip, part: zmx_png_pack_device — strided, planar, typed sources into PNG byte order, n of them in one launch
// (zmx_png_pack.h; the checks that need no runtime, the extents and the kernel's records are host/png_source.h's).
// Needs drv_errors.h (FailMsg, HIPCHK, KCHK, DEVICE_ENTRY), drv_context.h (zmx_ctx, PoolScope, KernelTiming) and
// drv_input.h (DeviceRangeChecker).
static thread_local double g_png_pack_ms = 0;   // k_png_pack of the calling thread's last call (zmx_internal_png_pack_ms)

extern "C" {
double zmx_internal_png_pack_ms(void) { return g_png_pack_ms; }

int zmx_internal_png_pack(zmx_ctx* c, const char* who, size_t n, const zmx_png_source* sources, void* const* d_out, const size_t* capacity) {
  g_png_pack_ms = 0;
  const std::string w(who);
  if (!c) return FailMsg(w + ": no context");
  if (n == 0) return 0;
  if (!sources || !d_out || !capacity) return FailMsg(w + ": null argument");
  std::vector<zamd::PngSourcePlan> plan(n);
  for (size_t i = 0; i < n; ++i) {
    const std::string wi = w + ": source " + std::to_string(i);
    const std::string msg = zamd::CheckPngSource(wi.c_str(), &sources[i], &plan[i]);
    if (!msg.empty()) return FailMsg(msg);
    if (capacity[i] < plan[i].nbytes) {
      return FailMsg(wi + ": the packed image takes " + std::to_string(plan[i].nbytes) + " bytes, the capacity is " + std::to_string(capacity[i]));
    }
    if (!d_out[i]) return FailMsg(wi + ": null destination");
  }
  DeviceRangeChecker src_checker, dst_checker;
  zamd::ApartRanges dests;
  for (size_t i = 0; i < n; ++i) {
    const std::string wi = w + ": source " + std::to_string(i);
    int device = -1;
    if (const int rc = src_checker.Check((wi + ": the extent").c_str(), reinterpret_cast<const void*>(plan[i].lo), plan[i].hi - plan[i].lo, &device)) return rc;
    if (device != c->device) return FailMsg(wi + ": memory of another device than the context's");
    if (const int rc = dst_checker.Check((wi + ": the destination").c_str(), d_out[i], plan[i].nbytes, &device)) return rc;
    if (device != c->device) return FailMsg(wi + ": the destination is memory of another device than the context's");
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_out[i]);
    dests.Add(at, at + plan[i].nbytes, i);
  }
  dests.Sort();
  size_t a = 0, b = 0;
  if (dests.Overlap(&a, &b)) {
    return FailMsg(w + ": source " + std::to_string(std::max(a, b)) + ": its destination overlaps that of source " + std::to_string(std::min(a, b)));
  }
  for (size_t i = 0; i < n; ++i) {
    if (dests.Hit(plan[i].lo, plan[i].hi, &a)) {
      return FailMsg(w + ": source " + std::to_string(i) + ": the destination of source " + std::to_string(a) + " overlaps its extent");
    }
  }
  std::vector<zamd::PngPackSource> records(n);
  std::vector<uint64_t> tile_start(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    records[i] = zamd::PngPackSourceOf(sources[i], d_out[i]);
    tile_start[i + 1] = tile_start[i] + zamd::PngPackTiles(records[i].out, records[i].total);
  }
  const uint64_t ntiles = tile_start[n];
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (the tables: held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  const auto enqueue = [&]() -> int {
    zamd::PngPackSource* d_records = nullptr;
    uint64_t* d_tile_start = nullptr;
    HIPCHK(tmp.Upload(&d_records, records.data(), n, "png_pack_sources"));
    HIPCHK(tmp.Upload(&d_tile_start, tile_start.data(), n + 1, "png_pack_tile_start"));
    zamd::PngPackTable T;
    T.src = d_records;
    T.tile_start = d_tile_start;
    T.n = n;
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_png_pack, dim3(zamd::PngPackGrid(ntiles)), dim3(zamd::kPngPackThreads), 0, c->stream, T, ntiles);
    KCHK(c, "k_png_pack");
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    return 0;
  };
  if (const int rc = enqueue()) {
    (void)hipStreamSynchronize(c->stream);   // (what was queued may still read the tables: drained before `tmp` gives them back)
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_png_pack_ms = ms;
  }
  return 0;
}

int zmx_png_pack_device(zmx_ctx* c, size_t n, const zmx_png_source* sources, void* const* d_out, const size_t* capacity) {
  return zmx_internal_png_pack(c, "zmx_png_pack_device", n, sources, d_out, capacity);
}
}  // extern "C"
