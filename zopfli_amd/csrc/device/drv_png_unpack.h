// zmx_hip.hip, part: zmx_png_unpack_device — own-mode pixels into strided, planar, typed sinks, n of them in one launch
// (zmx_png_unpack.h; the checks that need no runtime and the extents are host/png_sink.h's).  Also what the decode's sink
// entries (drv_png_decode.h) take from here: the sinks' checks and the launch.
// Needs drv_errors.h (FailMsg, HIPCHK, KCHK, DEVICE_ENTRY), drv_context.h (zmx_ctx, PoolScope, KernelTiming) and
// drv_input.h (DeviceRangeChecker).
#pragma once

static thread_local double g_png_unpack_ms = 0;   // k_png_unpack of the calling thread's last call (zmx_internal_png_unpack_ms)

namespace {

// Every sink checked (host/png_sink.h), its extent plain memory of the context's device inside one allocation, no two
// extents sharing a byte.  `extents` holds them sorted, for the caller's own ranges (ApartRanges::Hit).
int PngSinksCheck(zmx_ctx* c, const std::string& w, size_t n, const zmx_png_sink* sinks, zamd::ApartRanges* extents) {
  DeviceRangeChecker checker;
  for (size_t i = 0; i < n; ++i) {
    const std::string wi = w + ": sink " + std::to_string(i);
    zamd::PngSinkPlan plan;
    const std::string msg = zamd::CheckPngSink(wi.c_str(), &sinks[i], &plan);
    if (!msg.empty()) return FailMsg(msg);
    int device = -1;
    if (const int rc = checker.Check((wi + ": the extent").c_str(), reinterpret_cast<const void*>(plan.lo), plan.hi - plan.lo, &device)) return rc;
    if (device != c->device) return FailMsg(wi + ": memory of another device than the context's");
    extents->Add(plan.lo, plan.hi, i);
  }
  extents->Sort();
  size_t a = 0, b = 0;
  if (extents->Overlap(&a, &b)) {
    return FailMsg(w + ": sink " + std::to_string(std::max(a, b)) + ": its extent overlaps that of sink " + std::to_string(std::min(a, b)));
  }
  return 0;
}

// k_png_unpack over `jobs` on the context's stream, the tables from `tmp`; nothing is waited for.  `palettes`: 256 words
// for each palette a job names.
int PngUnpackEnqueue(zmx_ctx* c, PoolScope* tmp, const std::vector<zamd::PngUnpackJob>& jobs, const std::vector<uint32_t>& palettes, bool timed) {
  if (jobs.empty()) return 0;
  const size_t n = jobs.size();
  std::vector<uint64_t> tile_start(n + 1, 0);
  for (size_t i = 0; i < n; ++i) tile_start[i + 1] = tile_start[i] + zamd::PngUnpackTiles(jobs[i].npixels);
  const uint64_t ntiles = tile_start[n];
  zamd::PngUnpackJob* d_jobs = nullptr;
  uint64_t* d_tile_start = nullptr;
  uint32_t* d_palettes = nullptr;
  HIPCHK(tmp->Upload(&d_jobs, jobs.data(), n, "png_unpack_jobs"));
  HIPCHK(tmp->Upload(&d_tile_start, tile_start.data(), n + 1, "png_unpack_tile_start"));
  if (!palettes.empty()) HIPCHK(tmp->Upload(&d_palettes, palettes.data(), palettes.size(), "png_unpack_palettes"));
  zamd::PngUnpackTable T;
  T.jobs = d_jobs;
  T.tile_start = d_tile_start;
  T.palettes = d_palettes;
  T.n = n;
  if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
  hipLaunchKernelGGL(k_png_unpack, dim3(zamd::PngUnpackGrid(ntiles)), dim3(zamd::kPngUnpackThreads), 0, c->stream, T, ntiles);
  KCHK(c, "k_png_unpack");
  if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
  return 0;
}

// The job of image i and, for colour type 3, its palette behind those of the images before it.
void PngUnpackAddJob(const zmx_png_sink& sink, const zmx_png_decode_result& mode, const void* own, std::vector<zamd::PngUnpackJob>* jobs,
                     std::vector<uint32_t>* palettes) {
  uint32_t at = 0;
  if (mode.colortype == 3) {
    at = static_cast<uint32_t>(palettes->size() / 256);
    palettes->resize(palettes->size() + 256);
    zamd::PngUnpackPaletteOf(mode, palettes->data() + 256 * static_cast<size_t>(at));
  }
  jobs->push_back(zamd::PngUnpackJobOf(sink, mode, own, at));
}

}  // namespace

extern "C" {
double zmx_internal_png_unpack_ms(void) { return g_png_unpack_ms; }

int zmx_png_unpack_device(zmx_ctx* c, size_t n, const zmx_png_decode_result* modes, const void* const* d_own, const zmx_png_sink* sinks) {
  g_png_unpack_ms = 0;
  const std::string w = "zmx_png_unpack_device";
  if (!c) return FailMsg(w + ": no context");
  if (n == 0) return 0;
  if (!modes || !d_own || !sinks) return FailMsg(w + ": null argument");
  zamd::ApartRanges extents;
  if (const int rc = PngSinksCheck(c, w, n, sinks, &extents)) return rc;
  DeviceRangeChecker own_checker;
  for (size_t i = 0; i < n; ++i) {
    const std::string wi = w + ": image " + std::to_string(i);
    const std::string msg = zamd::CheckPngUnpackMode(wi.c_str(), modes[i], sinks[i]);
    if (!msg.empty()) return FailMsg(msg);
    const size_t nbytes = static_cast<size_t>(zamd::PngOutSize(zamd::kPngDecOwn, modes[i].width, modes[i].height, modes[i].colortype, modes[i].bitdepth));
    if (!d_own[i]) return FailMsg(wi + ": null pixels");
    int device = -1;
    if (const int rc = own_checker.Check((wi + ": the pixels").c_str(), d_own[i], nbytes, &device)) return rc;
    if (device != c->device) return FailMsg(wi + ": the pixels are memory of another device than the context's");
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_own[i]);
    size_t hit = 0;
    if (extents.Hit(at, at + nbytes, &hit)) return FailMsg(wi + ": the extent of sink " + std::to_string(hit) + " overlaps its pixels");
  }
  std::vector<zamd::PngUnpackJob> jobs;
  std::vector<uint32_t> palettes;
  jobs.reserve(n);
  for (size_t i = 0; i < n; ++i) PngUnpackAddJob(sinks[i], modes[i], d_own[i], &jobs, &palettes);
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (the tables: held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  if (const int rc = PngUnpackEnqueue(c, &tmp, jobs, palettes, timed)) {
    (void)hipStreamSynchronize(c->stream);   // (what was queued may still read the tables: drained before `tmp` gives them back)
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_png_unpack_ms = ms;
  }
  return 0;
}
}  // extern "C"
