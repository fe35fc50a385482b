// What the PNG decode entries (png_decode.cc, device/drv_png_decode.h) decide without a device, as plain functions that
// tests share: a result from a walk record, which chunk ranges are summed, the verdicts of the CRCs, of the stream and of
// the sizes, where a file's stream lies, what the entries refuse of their ranges, the verdict over a call's results.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "inflate_plan.h"
#include "zmx_png_decode.h"
#include "zopfli_amd.h"

namespace zamd {

constexpr uint64_t kPngScanlineLimit = 1ull << 40;   // a file's scanlines: refused at or above

inline const char* PngDecodeStatusName(uint32_t status) {
  static const char* const kNames[kPngDecStatuses] = {
      "ZMX_PNG_DECODE_OK", "ZMX_PNG_DECODE_SIGNATURE", "ZMX_PNG_DECODE_IHDR", "ZMX_PNG_DECODE_INTERLACE", "ZMX_PNG_DECODE_CHUNK",
      "ZMX_PNG_DECODE_CRITICAL", "ZMX_PNG_DECODE_CRC", "ZMX_PNG_DECODE_PLTE", "ZMX_PNG_DECODE_TRNS", "ZMX_PNG_DECODE_STREAM",
      "ZMX_PNG_DECODE_SIZE", "ZMX_PNG_DECODE_FILTER", "ZMX_PNG_DECODE_CAPACITY", "ZMX_PNG_DECODE_SHAPE"};
  return status < kPngDecStatuses ? kNames[status] : "an unknown status";
}

inline bool PngDecodeModeOk(int mode) { return mode == ZMX_PNG_DECODE_OWN || mode == ZMX_PNG_DECODE_RGBA8; }

// Whether the walk read the header (the fields of the record hold).
inline bool PngHeaderKnown(const PngWalkRecord& R) { return R.status != kPngDecSignature && R.status != kPngDecIhdr; }

// The scanlines of a file whose header is known: height * (1 + linebytes); false when that is kPngScanlineLimit or more.
inline bool PngScanBytes(const PngWalkRecord& R, uint64_t* bytes) {
  const uint64_t line = 1 + PngLineBytes(R.width, PngBpp(R.colortype, R.bitdepth));   // (below 2^36)
  if (line > kPngScanlineLimit / R.height) return false;
  *bytes = line * R.height;
  return true;
}

// The result of a file after its walk: the header's fields, the sizes, the palette (`palette`: the 256 words k_png_chunks
// wrote for the file, null where there is none).
inline void PngResultFromWalk(const PngWalkRecord& R, int mode, const uint32_t* palette, zmx_png_decode_result* out) {
  std::memset(out, 0, sizeof(*out));
  out->status = R.status;
  out->detail = R.status == kPngDecChunk || R.status == kPngDecCritical || R.status == kPngDecPlte || R.status == kPngDecTrns ? R.stop : 0;
  if (!PngHeaderKnown(R)) return;
  out->width = R.width;
  out->height = R.height;
  out->colortype = R.colortype;
  out->bitdepth = R.bitdepth;
  out->interlace = R.interlace;
  out->palettesize = R.palettesize;
  out->has_key = R.has_key;
  out->key_r = R.key_r;
  out->key_g = R.key_g;
  out->key_b = R.key_b;
  uint64_t scan = 0;
  if (PngScanBytes(R, &scan)) {
    out->outsize_own = PngOutSize(kPngDecOwn, R.width, R.height, R.colortype, R.bitdepth);
    out->outsize_rgba8 = PngOutSize(kPngDecRgba8, R.width, R.height, R.colortype, R.bitdepth);
    out->outsize = mode == ZMX_PNG_DECODE_RGBA8 ? out->outsize_rgba8 : out->outsize_own;
  }
  if (palette && R.has_plte && (R.status == kPngDecOk || R.status == kPngDecInterlace)) {
    for (uint32_t i = 0; i < R.palettesize; ++i) {
      for (int k = 0; k < 4; ++k) out->palette[4 * i + k] = static_cast<unsigned char>(palette[i] >> (8 * k));
    }
  }
}

// The CRCs' verdict on a file whose walk ended OK: the first entry (in file order) whose computed CRC-32 is not the stored
// one gives ZMX_PNG_DECODE_CRC with its chunk's number.  computed[k] belongs to entries[k].
inline void PngCrcVerdict(const PngChunkEntry* entries, const uint32_t* computed, uint32_t n, zmx_png_decode_result* out) {
  for (uint32_t k = 0; k < n; ++k) {
    if (computed[k] == entries[k].crc) continue;
    out->status = kPngDecCrc;
    out->detail = entries[k].index;
    return;
  }
}

// The stream's verdict from k_inflate's result of a run into exactly `scan` bytes (or of a size-only run).
inline void PngStreamVerdict(const zmx_inflate_result& r, uint64_t scan, zmx_png_decode_result* out) {
  if (r.status == ZMX_INFLATE_CAPACITY || (r.status == ZMX_INFLATE_OK && r.outsize != scan)) {
    out->status = kPngDecSize;
    out->detail = 0;
  } else if (r.status != ZMX_INFLATE_OK) {
    out->status = kPngDecStream;
    out->detail = r.status;
  }
}

// No destination may share a byte with another destination or with any file of the call: the inflate entries' rule.
inline std::string CheckPngDecodeApart(const char* who, size_t n, const void* const* d_file, const size_t* filesize, void* const* d_out,
                                       const size_t* capacity) {
  return CheckInflateApart(who, n, d_file, filesize, d_out, capacity);
}

// The verdict over a call's results: empty when every file is OK; else the first failing file's index and status by name
// and the class of the failure.
inline std::string PngDecodeVerdict(const char* who, size_t n, const zmx_png_decode_result* results, const size_t* capacity, int* error_class) {
  for (size_t i = 0; i < n; ++i) {
    const zmx_png_decode_result& r = results[i];
    if (r.status == kPngDecOk) continue;
    std::string text = "file " + std::to_string(i) + ": " + PngDecodeStatusName(r.status) + " (" + std::to_string(r.status) + "), detail " +
                       std::to_string(r.detail);
    if (r.status == kPngDecStream) text += std::string(" (") + InflateStatusName(r.detail) + ")";
    if (r.status == kPngDecCapacity) {
      text += ": the pixels take " + std::to_string(r.outsize) + " bytes, d_out has " + std::to_string(capacity ? capacity[i] : 0);
    }
    *error_class = r.status == kPngDecCapacity ? ZMX_ERR_REFUSED : ZMX_ERR_DATA;
    return Refusal(who, text);
  }
  return std::string();
}

}  // namespace zamd
