// zmx_inflate_device, zmx_inflate_device_batch: deflate, zlib and gzip streams in device memory decoded into device memory
// on a context from the pool, checksums verified.
//
// The call checks its ranges (entry_checks.h, inflate_plan.h), lists the jobs longest input first, holds one context of the
// ranges' device and runs k_inflate round by round (zmx_internal_inflate_run: 32 bytes a stream come down).  Then the
// outputs of the gzip and zlib streams that ended OK with their output stored go through zmx_checksum_device — its two
// kernels, launched once for the batch, 4 bytes a stream come down — and the host compares the values with the trailers
// the kernel returned, and gzip's ISIZE with the size.  No byte of a stream or of its output visits the host.  Size-only
// calls, over-capacity streams and raw deflate have nothing to compare.
#include <string>
#include <vector>

#include "dealing.h"
#include "inflate_plan.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"

namespace {

int Refuse(const std::string& msg) {
  zmx_internal_set_error(msg.c_str(), ZMX_ERR_REFUSED);
  return -1;
}

int InflateBatch(const char* who, ZopfliFormat format, size_t n, const void* const* d_in, const size_t* insize, void* const* d_out,
                 const size_t* capacity, zmx_inflate_result* results) {
  if (!zamd::InflateFormatOk(format)) return Refuse(std::string(who) + ": invalid ZopfliFormat " + std::to_string(static_cast<int>(format)));
  if (n == 0) return 0;
  if (!d_in || !insize || !results || (d_out && !capacity)) return Refuse(std::string(who) + ": null array");
  // ---- every range checked before a context is taken
  int in_device = -1, out_device = -1;
  if (zmx_internal_device_pointers_one_device((std::string(who) + ": d_in").c_str(), n, d_in, insize, &in_device) != 0) return -1;
  if (d_out) {
    // (a null destination is the size-only mode: no range)
    std::vector<size_t> bytes(n);
    for (size_t i = 0; i < n; ++i) bytes[i] = d_out[i] ? capacity[i] : 0;
    if (zmx_internal_device_pointers_one_device((std::string(who) + ": d_out").c_str(), n, d_out, bytes.data(), &out_device) != 0) return -1;
    if (in_device >= 0 && out_device >= 0 && in_device != out_device) return Refuse(std::string(who) + ": d_in and d_out lie on different devices");
  }
  const std::string apart = zamd::CheckInflateApart(who, n, d_in, insize, d_out, capacity);
  if (!apart.empty()) return Refuse(apart);
  const std::vector<zamd::InflateJob> jobs = zamd::InflateJobs(n, d_in, insize, d_out, capacity);
  std::vector<zmx_inflate_result> got(n);
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    for (size_t r = 0; r < zamd::InflateRounds(n); ++r) {
      size_t begin = 0, end = 0;
      zamd::InflateRound(n, r, &begin, &end);
      if (zmx_internal_inflate_run(ctx, format, end - begin, jobs.data() + begin, got.data()) != 0) return -1;
    }
    if (format == ZOPFLI_FORMAT_DEFLATE || !d_out) return 0;
    // ---- the checksums of what was stored, one launch pair for the batch
    std::vector<size_t> which;
    std::vector<const void*> ptrs;
    std::vector<size_t> sizes;
    for (size_t i = 0; i < n; ++i) {
      if (got[i].status != ZMX_INFLATE_OK || !d_out[i]) continue;
      which.push_back(i);
      ptrs.push_back(d_out[i]);
      sizes.push_back(static_cast<size_t>(got[i].outsize));
    }
    if (which.empty()) return 0;
    std::vector<uint32_t> values(which.size());
    const int kind = format == ZOPFLI_FORMAT_GZIP ? ZMX_CRC32 : ZMX_ADLER32;
    if (zmx_checksum_device(ctx, kind, which.size(), ptrs.data(), sizes.data(), values.data()) != 0) return -1;
    for (size_t k = 0; k < which.size(); ++k) got[which[k]].status = zamd::InflateTrailerVerdict(format, got[which[k]], values[k]);
    return 0;
  }, in_device >= 0 ? in_device : out_device);
  if (rc != 0) return rc;
  for (size_t i = 0; i < n; ++i) results[i] = got[i];
  int error_class = ZMX_ERR_NONE;
  const std::string verdict = zamd::InflateVerdict(who, n, results, d_out ? capacity : nullptr, &error_class);
  if (verdict.empty()) return 0;
  zmx_internal_set_error(verdict.c_str(), error_class);
  return -1;
}

}  // namespace

extern "C" int zmx_inflate_device_batch(ZopfliFormat format, size_t n, const void* const* d_in, const size_t* insize, void* const* d_out,
                                        const size_t* capacity, zmx_inflate_result* results) {
  return InflateBatch("zmx_inflate_device_batch", format, n, d_in, insize, d_out, capacity, results);
}

extern "C" int zmx_inflate_device(ZopfliFormat format, const void* d_in, size_t insize, void* d_out, size_t capacity, size_t* outsize) {
  if (!outsize) return Refuse("zmx_inflate_device: null argument");
  *outsize = 0;
  zmx_inflate_result result = {0, 0, 0, 0, 0, 0};
  const int rc = InflateBatch("zmx_inflate_device", format, 1, &d_in, &insize, &d_out, &capacity, &result);
  *outsize = static_cast<size_t>(result.outsize);
  return rc;
}
