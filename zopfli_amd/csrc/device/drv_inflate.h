// Driver part: inflate on the device (zmx_inflate.h).  Holds k_inflate's launch (zmx_internal_inflate_run: what the pooled
// entries of host/inflate.cc run round by round) and zmx_inflate_device_ctx, the step on a context the caller holds.
// Needs drv_context.h (zmx_ctx, PoolScope, KernelTiming), drv_input.h (DeviceRangeChecker), host/inflate_plan.h.
#pragma once

static_assert(zamd::kInflateOk == ZMX_INFLATE_OK && zamd::kInflateHeader == ZMX_INFLATE_HEADER && zamd::kInflateDict == ZMX_INFLATE_DICT &&
                  zamd::kInflateBlockType == ZMX_INFLATE_BLOCK_TYPE && zamd::kInflateStoredLen == ZMX_INFLATE_STORED_LEN &&
                  zamd::kInflateTooManySymbols == ZMX_INFLATE_TOO_MANY_SYMBOLS && zamd::kInflateRepeat == ZMX_INFLATE_REPEAT &&
                  zamd::kInflateOversubscribed == ZMX_INFLATE_OVERSUBSCRIBED && zamd::kInflateIncomplete == ZMX_INFLATE_INCOMPLETE &&
                  zamd::kInflateNoEndCode == ZMX_INFLATE_NO_END_CODE && zamd::kInflateBadCode == ZMX_INFLATE_BAD_CODE &&
                  zamd::kInflateBadSymbol == ZMX_INFLATE_BAD_SYMBOL && zamd::kInflateDistance == ZMX_INFLATE_DISTANCE &&
                  zamd::kInflateTruncated == ZMX_INFLATE_TRUNCATED && zamd::kInflateCapacity == ZMX_INFLATE_CAPACITY &&
                  zamd::kInflateChecksum == ZMX_INFLATE_CHECKSUM && zamd::kInflateSize == ZMX_INFLATE_SIZE,
              "the kernel's statuses are the ABI's");
static_assert(zamd::kInflateGzip == ZOPFLI_FORMAT_GZIP && zamd::kInflateZlib == ZOPFLI_FORMAT_ZLIB && zamd::kInflateDeflate == ZOPFLI_FORMAT_DEFLATE,
              "the kernel's formats are the ABI's");
static_assert(sizeof(zmx_inflate_result) == sizeof(zamd::InflateResult) && offsetof(zmx_inflate_result, status) == offsetof(zamd::InflateResult, status) &&
                  offsetof(zmx_inflate_result, stored_isize) == offsetof(zamd::InflateResult, stored_isize),
              "the kernel's result is the ABI's");
static_assert(sizeof(zamd::InflateScratch) <= 65536, "a wave's LDS: at least two waves a CU");

extern "C" {
static thread_local double g_inflate_ms = 0;   // (zmx_internal_inflate_ms)
double zmx_internal_inflate_ms(void) { return g_inflate_ms; }

int zmx_internal_inflate_run(zmx_ctx* c, int format, size_t n, const zamd::InflateJob* jobs, zmx_inflate_result* results) {
  g_inflate_ms = 0;
  if (n == 0) return 0;
  if (n > zamd::kInflateRoundJobs) return FailMsg("zmx_internal_inflate_run: too many jobs for one launch");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  std::vector<zamd::InflateResult> got(n);
  const auto enqueue = [&]() -> int {
    zamd::InflateJob* d_jobs = nullptr;
    zamd::InflateResult* d_results = nullptr;
    HIPCHK(tmp.Upload(&d_jobs, jobs, n, "inflate_jobs"));
    HIPCHK(tmp.AllocT(&d_results, n, "inflate_results"));
    InflateParams P;
    P.jobs = d_jobs;
    P.results = d_results;
    P.njobs = static_cast<u32>(n);
    P.format = static_cast<u32>(format);
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_inflate, dim3(static_cast<unsigned>(n)), dim3(zamd::kInflateLanes), 0, c->stream, P);
    KCHK(c, "k_inflate");
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipMemcpyAsync(got.data(), d_results, n * sizeof(zamd::InflateResult), hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  if (const int rc = enqueue()) {
    (void)hipStreamSynchronize(c->stream);   // (what was queued may still read the jobs: drained before `tmp` gives them back)
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_inflate_ms = ms;
  }
  for (size_t k = 0; k < n; ++k) {
    const zamd::InflateResult& r = got[k];
    results[jobs[k].index] = {r.outsize, r.consumed, r.status, r.block, r.stored_check, r.stored_isize};
  }
  return 0;
}

int zmx_inflate_device_ctx(zmx_ctx* c, ZopfliFormat format, size_t n, const void* const* d_in, const size_t* insize, void* const* d_out,
                           const size_t* capacity, zmx_inflate_result* results) {
  static const char* const kWho = "zmx_inflate_device_ctx";
  if (!c) return FailMsg("zmx_inflate_device_ctx: no context");
  if (!zamd::InflateFormatOk(format)) return FailMsg(std::string(kWho) + ": invalid ZopfliFormat " + std::to_string(static_cast<int>(format)));
  if (n == 0) return 0;
  if (!d_in || !insize || !results || (d_out && !capacity)) return FailMsg("zmx_inflate_device_ctx: null array");
  // ---- every range checked before anything is launched
  DeviceRangeChecker in_checker, out_checker;
  for (size_t i = 0; i < n; ++i) {
    int device = -1;
    const std::string w = std::string(kWho) + ": input " + std::to_string(i);
    if (const int rc = in_checker.Check(w.c_str(), d_in[i], insize[i], &device)) return rc;
    if (device >= 0 && device != c->device) return FailMsg(w + " is not memory of the context's device");
    if (!d_out || !d_out[i]) continue;
    const std::string wo = std::string(kWho) + ": destination " + std::to_string(i);
    if (const int rc = out_checker.Check(wo.c_str(), d_out[i], capacity[i], &device)) return rc;
    if (device >= 0 && device != c->device) return FailMsg(wo + " is not memory of the context's device");
  }
  const std::string apart = zamd::CheckInflateApart(kWho, n, d_in, insize, d_out, capacity);
  if (!apart.empty()) return FailMsg(apart);
  const std::vector<zamd::InflateJob> jobs = zamd::InflateJobs(n, d_in, insize, d_out, capacity);
  std::vector<zmx_inflate_result> got(n);
  for (size_t r = 0; r < zamd::InflateRounds(n); ++r) {
    size_t begin = 0, end = 0;
    zamd::InflateRound(n, r, &begin, &end);
    if (const int rc = zmx_internal_inflate_run(c, format, end - begin, jobs.data() + begin, got.data())) return rc;
  }
  std::copy(got.begin(), got.end(), results);
  int error_class = ZMX_ERR_NONE;
  const std::string verdict = zamd::InflateVerdict(kWho, n, results, d_out ? capacity : nullptr, &error_class);
  if (verdict.empty()) return 0;
  g_err = verdict;
  g_err_class = error_class;
  return -1;
}
}  // extern "C"
