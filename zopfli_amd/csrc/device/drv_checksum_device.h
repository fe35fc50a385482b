// Driver part: checksums of arbitrary device memory, finished on the device (zmx_checksum_device.h).  Holds
// zmx_checksum_device and zmx_internal_checksum_seal (the CRC-32 of a PNG's IDAT, written where the file lies).
// Needs drv_context.h (zmx_ctx, PoolScope, KernelTiming), drv_input.h (DeviceRangeChecker), drv_checksum.h (IsChecksumKind).
#pragma once

static_assert(zamd::kChecksumDeviceCrc == ZMX_CRC32 && zamd::kChecksumDeviceAdler == ZMX_ADLER32, "the kernels' kinds are the ABI's");

extern "C" {
static thread_local double g_checksum_device_ms[2] = {0, 0};   // (zmx_internal_checksum_device_ms)
void zmx_internal_checksum_device_ms(double out[2]) {
  out[0] = g_checksum_device_ms[0];
  out[1] = g_checksum_device_ms[1];
}

// The two launches over n ranges the caller has checked: d_ptr[i][0, nbytes[i]) on the context's device.  seal null: the
// values come down into values[0, n); else value i goes to the four bytes at seal[i], and nothing comes down.
static int RunChecksumDevice(zmx_ctx* c, int kind, size_t n, const void* const* d_ptr, const size_t* nbytes, unsigned char* const* seal,
                             uint32_t* values) {
  g_checksum_device_ms[0] = g_checksum_device_ms[1] = 0;
  std::vector<zamd::ChecksumRange> ranges(n);
  uint64_t npieces = 0;
  for (size_t r = 0; r < n; ++r) {
    zamd::ChecksumRange& R = ranges[r];
    R.p = static_cast<const unsigned char*>(d_ptr[r]);
    R.len = nbytes[r];
    R.first_piece = npieces;
    R.npieces = zamd::ChecksumPieces(R.len);
    R.seal = seal ? seal[r] : nullptr;
    R.xlen = kind == ZMX_CRC32 ? zamd::Gf2XPow8(R.len) : 0;
    R.pad = 0;
    npieces += R.npieces;
  }
  if (npieces > 0x7fffffffull || n > 0xffffffffull) return FailMsg("zmx_checksum_device: too many pieces for one launch");
  std::vector<zamd::ChecksumPieceRef> refs(static_cast<size_t>(npieces));
  for (size_t r = 0; r < n; ++r) {
    for (uint64_t j = 0; j < ranges[r].npieces; ++j) refs[ranges[r].first_piece + j] = {static_cast<uint32_t>(r), static_cast<uint32_t>(j)};
  }
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  const auto enqueue = [&]() -> int {
    zamd::ChecksumRange* d_ranges = nullptr;
    zamd::ChecksumPieceRef* d_refs = nullptr;
    u32 *d_out = nullptr, *d_values = nullptr;
    HIPCHK(tmp.Upload(&d_ranges, ranges.data(), n, "checksum_ranges"));
    HIPCHK(tmp.Upload(&d_refs, refs.data(), refs.size(), "checksum_refs"));
    HIPCHK(tmp.AllocT(&d_out, 3 * refs.size(), "checksum_pieces"));
    HIPCHK(tmp.AllocT(&d_values, n, "checksum_values"));
    ChecksumDeviceParams P;
    P.ranges = d_ranges;
    P.piece = d_refs;
    P.out = d_out;
    P.values = d_values;
    P.nranges = n;
    P.kind = static_cast<u32>(kind);
    P.xpiece = zamd::Gf2XPow8(zamd::kChecksumPieceBytes);
    zamd::ChecksumTreePowers(P.xpow);
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    if (!refs.empty()) {
      hipLaunchKernelGGL(k_checksum_pieces, dim3(static_cast<unsigned>(refs.size())), dim3(256), 0, c->stream, P);
      KCHK(c, "k_checksum_pieces");
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    const size_t grid = (n + zamd::kChecksumFinishThreads - 1) / zamd::kChecksumFinishThreads;
    hipLaunchKernelGGL(k_checksum_finish, dim3(static_cast<unsigned>(grid)), dim3(zamd::kChecksumFinishThreads), 0, c->stream, P);
    KCHK(c, "k_checksum_finish");
    if (timed) HIPCHK(hipEventRecord(c->ev[2], c->stream));
    if (!seal) HIPCHK(hipMemcpyAsync(values, d_values, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
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
    g_checksum_device_ms[0] = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[1], c->ev[2]));
    g_checksum_device_ms[1] = ms;
  }
  return 0;
}

int zmx_checksum_device(zmx_ctx* c, int kind, size_t n, const void* const* d_ptr, const size_t* nbytes, uint32_t* values) {
  static const char* const kWho = "zmx_checksum_device";
  if (!c) return FailMsg("zmx_checksum_device: no context");
  if (!IsChecksumKind(kind)) return FailMsg("zmx_checksum_device: unknown kind");
  if (n == 0) return 0;
  if (!d_ptr || !nbytes || !values) return FailMsg("zmx_checksum_device: null array");
  // ---- every range checked before anything is launched (the results go to an array of the call's own first)
  DeviceRangeChecker checker;
  for (size_t i = 0; i < n; ++i) {
    const std::string w = std::string(kWho) + ": range " + std::to_string(i);
    int device = -1;
    if (const int rc = checker.Check(w.c_str(), d_ptr[i], nbytes[i], &device)) return rc;
    if (device >= 0 && device != c->device) return FailMsg(w + " is not memory of the context's device");
  }
  std::vector<uint32_t> got(n);
  if (const int rc = RunChecksumDevice(c, kind, n, d_ptr, nbytes, nullptr, got.data())) return rc;
  std::copy(got.begin(), got.end(), values);
  return 0;
}

int zmx_internal_checksum_seal(zmx_ctx* c, int kind, size_t n, const void* const* d_ptr, const size_t* nbytes, unsigned char* const* d_seal) {
  if (n == 0) return 0;
  return RunChecksumDevice(c, kind, n, d_ptr, nbytes, d_seal, nullptr);
}
}  // extern "C"
