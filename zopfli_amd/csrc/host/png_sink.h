// zmx_png_sink (include/zopfli_amd.h): what is refused of one without asking the runtime, and its extent.  A sink is a
// source turned round — the same fields, written where a source is read —, so the checks and the extent are
// host/png_source.h's (CheckPngStrided, PngSourceExtent); what a sink adds is that no two of its samples may share a byte.
// No HIP, no globals: the device layer (device/drv_png_unpack.h), the entries (png_decode.cc) and a plain C++ program
// (tests/hostlib/png_sink_print.cc) run the same functions.  A check returns the refusal's text behind `who`, or an empty
// string.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "png_source.h"
#include "zmx_png_decode.h"
#include "zopfli_amd.h"

namespace zamd {

struct PngSinkPlan {
  uintptr_t lo, hi;   // the extent as addresses
};

// Whether samples of a sink whose strides' reaches do not overflow (its extent has been computed) lie apart: the
// dimensions with an extent above 1, by |stride| ascending — each |stride| at least the sample's size plus what the
// smaller ones reach.
inline bool PngSinkSamplesApart(const zmx_png_sink& s) {
  struct Dim { uint64_t stride, last; };
  const int64_t stride[3] = {s.stride_y, s.stride_x, s.stride_c};
  const uint32_t extent[3] = {s.height, s.width, s.channels};
  Dim dims[3];
  int n = 0;
  for (int d = 0; d < 3; ++d) {
    if (extent[d] <= 1) continue;
    dims[n++] = {stride[d] < 0 ? 0 - static_cast<uint64_t>(stride[d]) : static_cast<uint64_t>(stride[d]), static_cast<uint64_t>(extent[d]) - 1};
  }
  std::sort(dims, dims + n, [](const Dim& a, const Dim& b) { return a.stride < b.stride; });
  uint64_t reach = PngSourceSampleBytes(s.sample);   // (the sums are below the extent's size, which did not overflow)
  for (int d = 0; d < n; ++d) {
    if (dims[d].stride < reach) return false;
    reach += dims[d].stride * dims[d].last;
  }
  return true;
}

// Everything of the sink's "refused before anything runs" that needs no device.
inline std::string CheckPngSink(const char* who, const zmx_png_sink* s, PngSinkPlan* plan) {
  uintptr_t lo = 0, hi = 0;
  const std::string msg = CheckPngStrided(who, s, true, &lo, &hi);
  if (!msg.empty()) return msg;
  if (!PngSinkSamplesApart(*s)) return Refusal(who, "samples of the sink share a byte (a stride of 0, or one below what the smaller ones reach)");
  if (plan) {
    plan->lo = lo;
    plan->hi = hi;
  }
  return std::string();
}

// What zmx_png_unpack_device refuses of a mode and its sink: `mode` says what the own-mode pixels are.
inline std::string CheckPngUnpackMode(const char* who, const zmx_png_decode_result& mode, const zmx_png_sink& sink) {
  if (mode.status != ZMX_PNG_DECODE_OK) return Refusal(who, "its mode has status " + std::to_string(mode.status) + ", not ZMX_PNG_DECODE_OK");
  if (!PngColorOk(mode.colortype, mode.bitdepth)) {
    return Refusal(who, "colour type " + std::to_string(mode.colortype) + " at " + std::to_string(mode.bitdepth) + " bits is no PNG mode");
  }
  if (mode.colortype == 3 && (mode.palettesize == 0 || mode.palettesize > 256)) return Refusal(who, "a palette of " + std::to_string(mode.palettesize) + " entries");
  if (mode.width != sink.width || mode.height != sink.height) {
    return Refusal(who, "the pixels are " + std::to_string(mode.width) + " x " + std::to_string(mode.height) + ", the sink is " +
                            std::to_string(sink.width) + " x " + std::to_string(sink.height));
  }
  return std::string();
}

}  // namespace zamd
