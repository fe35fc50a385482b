// zmx_png_info_device, zmx_png_decode_device, zmx_png_decode_device_batch: PNG files in device memory decoded into device
// memory on a context from the pool.
//
// The call checks its ranges (entry_checks.h, png_decode_plan.h), holds one context of the ranges' device and runs
// zmx_internal_png_decode_run on it (device/drv_png_decode.h): k_png_chunks over all files, the chunks' CRC-32s, split IDATs
// put end to end, k_inflate into the call's scanline buffer, the Adler-32s, k_png_unfilter into the destinations.  No byte
// of a file, of its stream or of its pixels visits the host: zmx_last_input_traffic and zmx_last_output_traffic stay 0.
// The zmx_png_decode_sink_* entries and zmx_png_sink_check: the same run with zmx_png_sinks in the destinations' place
// (png_sink.h has what is refused of one without a device).
#include <string>
#include <vector>

#include "dealing.h"
#include "png_decode_plan.h"
#include "png_sink.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"

namespace {

int Refuse(const std::string& msg) {
  zmx_internal_set_error(msg.c_str(), ZMX_ERR_REFUSED);
  return -1;
}

int DecodeBatch(const char* who, int mode, bool info_only, size_t n, const void* const* d_file, const size_t* filesize, void* const* d_out,
                const size_t* capacity, zmx_png_decode_result* results) {
  if (!zamd::PngDecodeModeOk(mode)) return Refuse(std::string(who) + ": unknown mode " + std::to_string(mode));
  if (n == 0) return 0;
  if (!d_file || !filesize || !results || (d_out && !capacity)) return Refuse(std::string(who) + ": null array");
  zamd::ResetCallStats();
  // ---- every range checked before a context is taken
  int in_device = -1, out_device = -1;
  if (zmx_internal_device_pointers_one_device((std::string(who) + ": d_file").c_str(), n, d_file, filesize, &in_device) != 0) return -1;
  if (d_out) {
    // (a null destination is the size-only mode: no range)
    std::vector<size_t> bytes(n);
    for (size_t i = 0; i < n; ++i) bytes[i] = d_out[i] ? capacity[i] : 0;
    if (zmx_internal_device_pointers_one_device((std::string(who) + ": d_out").c_str(), n, d_out, bytes.data(), &out_device) != 0) return -1;
    if (in_device >= 0 && out_device >= 0 && in_device != out_device) return Refuse(std::string(who) + ": d_file and d_out lie on different devices");
  }
  const std::string apart = zamd::CheckPngDecodeApart(who, n, d_file, filesize, d_out, capacity);
  if (!apart.empty()) return Refuse(apart);
  std::vector<zmx_png_decode_result> got(n);
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    return zmx_internal_png_decode_run(ctx, who, mode, info_only ? 1 : 0, n, d_file, filesize, d_out, capacity, got.data(), nullptr);
  }, in_device >= 0 ? in_device : out_device);
  if (rc != 0) return rc;
  for (size_t i = 0; i < n; ++i) results[i] = got[i];
  int error_class = ZMX_ERR_NONE;
  const std::string verdict = zamd::PngDecodeVerdict(who, n, results, d_out ? capacity : nullptr, &error_class);
  if (verdict.empty()) return 0;
  zmx_internal_set_error(verdict.c_str(), error_class);
  return -1;
}

// The decode into sinks: the files' ranges are checked here, the sinks on the context that runs (their extents must be its
// device's).
int DecodeSinkBatch(const char* who, size_t n, const void* const* d_file, const size_t* filesize, const zmx_png_sink* sinks,
                    zmx_png_decode_result* results) {
  if (n == 0) return 0;
  if (!d_file || !filesize || !sinks || !results) return Refuse(std::string(who) + ": null array");
  zamd::ResetCallStats();
  int in_device = -1;
  if (zmx_internal_device_pointers_one_device((std::string(who) + ": d_file").c_str(), n, d_file, filesize, &in_device) != 0) return -1;
  for (size_t i = 0; i < n; ++i) {
    // (before a context is taken: what needs no runtime)
    const std::string msg = zamd::CheckPngSink((std::string(who) + ": sink " + std::to_string(i)).c_str(), &sinks[i], nullptr);
    if (!msg.empty()) return Refuse(msg);
  }
  std::vector<zmx_png_decode_result> got(n);
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    return zmx_internal_png_decode_sink_run(ctx, who, n, d_file, filesize, sinks, got.data(), nullptr);
  }, in_device);
  if (rc != 0) return rc;
  for (size_t i = 0; i < n; ++i) results[i] = got[i];
  int error_class = ZMX_ERR_NONE;
  const std::string verdict = zamd::PngDecodeVerdict(who, n, results, nullptr, &error_class);
  if (verdict.empty()) return 0;
  zmx_internal_set_error(verdict.c_str(), error_class);
  return -1;
}

}  // namespace

extern "C" int zmx_png_sink_check(const zmx_png_sink* sink) {
  const std::string msg = zamd::CheckPngSink("zmx_png_sink_check", sink, nullptr);
  return msg.empty() ? 0 : Refuse(msg);
}

extern "C" int zmx_png_decode_sink_device_batch(size_t n, const void* const* d_file, const size_t* filesize, const zmx_png_sink* sinks,
                                                zmx_png_decode_result* results) {
  return DecodeSinkBatch("zmx_png_decode_sink_device_batch", n, d_file, filesize, sinks, results);
}

extern "C" int zmx_png_decode_sink_device(const void* d_file, size_t filesize, const zmx_png_sink* sink, zmx_png_decode_result* result) {
  if (!sink || !result) return Refuse("zmx_png_decode_sink_device: null argument");
  return DecodeSinkBatch("zmx_png_decode_sink_device", 1, &d_file, &filesize, sink, result);
}

extern "C" int zmx_png_info_device(size_t n, const void* const* d_file, const size_t* filesize, zmx_png_decode_result* results) {
  return DecodeBatch("zmx_png_info_device", ZMX_PNG_DECODE_OWN, true, n, d_file, filesize, nullptr, nullptr, results);
}

extern "C" int zmx_png_decode_device_batch(int mode, size_t n, const void* const* d_file, const size_t* filesize, void* const* d_out,
                                           const size_t* capacity, zmx_png_decode_result* results) {
  return DecodeBatch("zmx_png_decode_device_batch", mode, false, n, d_file, filesize, d_out, capacity, results);
}

extern "C" int zmx_png_decode_device(int mode, const void* d_file, size_t filesize, void* d_out, size_t capacity, zmx_png_decode_result* result) {
  if (!result) return Refuse("zmx_png_decode_device: null argument");
  return DecodeBatch("zmx_png_decode_device", mode, false, 1, &d_file, &filesize, &d_out, &capacity, result);
}
