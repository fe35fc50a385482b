// zmx_png_encode_device, zmx_png_encode_device_batch: an image in device memory as the PNG file zopflipng writes for it
// (include/zopfli_amd.h says which).  The filter types and the filtered scanlines are made on a pooled context of the
// image's device, into a buffer of the call's own that outlives the context's hold: the context goes back to the pool
// BEFORE zmx_compress_device(ZLIB) of the buffer runs, which takes contexts itself.  The stream's second byte and the
// chunks around it are png_container.h's.  (Outside api.cc, as png.cc is: the host-only test library links api.cc
// against a stand-in for the device layer.)
#include <cstdlib>
#include <string>
#include <vector>

#include "dealing.h"
#include "deflate.h"
#include "png_container.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"

namespace {

constexpr unsigned kBruteWindow = 32768;   // zopflipng's final encode (zopflipng_lib.cc:360)

int Refuse(const std::string& msg) {
  zmx_internal_set_error(msg.c_str(), ZMX_ERR_REFUSED);
  return -1;
}

// a device allocation of the call's own
struct DeviceBuffer {
  int device = -1;
  void* p = nullptr;
  ~DeviceBuffer() { zmx_internal_device_free(device, p); }
};

struct Geometry {
  size_t linebytes, bytewidth, height, scanlines;   // scanlines = height * (linebytes + 1)
};

// What is refused of an image on the host, before its pointer is looked at.
int CheckImage(const std::string& w, const zmx_png_image& im, Geometry* g) {
  if (im.width == 0 || im.height == 0) return Refuse(w + ": width or height 0");
  if (!zamd::PngFormatOk(im.colortype, im.bitdepth)) {
    return Refuse(w + ": colour type " + std::to_string(im.colortype) + " at " + std::to_string(im.bitdepth) +
                  " bits is not taken (0, 2, 4, 6 at 8 or 16)");
  }
  g->bytewidth = zamd::PngByteWidth(im.colortype, im.bitdepth);
  g->linebytes = zamd::PngLineBytes(im.width, im.colortype, im.bitdepth);
  g->height = im.height;
  if (g->linebytes > 0x7fffffffu || g->height > 0x7fffffffu) return Refuse(w + ": bad geometry");
  g->scanlines = g->height * (g->linebytes + 1);
  return 0;
}

bool StrategyOk(int strategy, bool predefined_allowed) {
  return (strategy >= ZMX_PNG_FILTER_ZERO && strategy <= ZMX_PNG_FILTER_BRUTE) ||
         (predefined_allowed && strategy == ZMX_PNG_FILTER_PREDEFINED);
}

// A file in the making: a malloc'ed array under the reference's convention that begins with PngPrefix's bytes, for
// ZopfliCompress to append the stream to.
struct File {
  unsigned char* bytes = nullptr;
  size_t size = 0;
  File() = default;
  File(const File&) = delete;
  File& operator=(const File&) = delete;
  ~File() { std::free(bytes); }
  void Begin(const zmx_png_image& im) {
    unsigned char prefix[zamd::kPngPrefixBytes];
    zamd::PngPrefix(im.width, im.height, im.colortype, im.bitdepth, prefix);
    zamd::AppendToOutput(prefix, sizeof(prefix), &bytes, &size);
  }
  // the stream is in: what depends on it, and the file's end
  bool Close() {
    unsigned char trailer[zamd::kPngTrailerBytes];
    if (!zamd::PngClose(bytes, size, trailer)) return false;
    zamd::AppendToOutput(trailer, sizeof(trailer), &bytes, &size);
    return true;
  }
  // appended to (*out, *outsize): handed over as it is where they hold nothing (*out is not looked at while the size is 0)
  void GiveTo(unsigned char** out, size_t* outsize) {
    if (*outsize == 0) {
      *out = bytes;
      *outsize = size;
      bytes = nullptr;
    } else {
      zamd::AppendToOutput(bytes, size, out, outsize);
    }
  }
};

int BadStream(const std::string& w) {
  zmx_internal_set_error((w + ": the zlib stream does not fit an IDAT chunk").c_str(), ZMX_ERR_DEVICE);
  return -1;
}

}  // namespace

extern "C" int zmx_png_encode_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                     const unsigned char* predefined, unsigned char** out, size_t* outsize) {
  const std::string w = "zmx_png_encode_device";
  if (!options || !image || !out || !outsize) return Refuse(w + ": null argument");
  Geometry g;
  if (CheckImage(w, *image, &g) != 0) return -1;
  if (!StrategyOk(strategy, true)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  if (strategy == ZMX_PNG_FILTER_PREDEFINED) {
    if (!predefined) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED without types");
    for (size_t r = 0; r < g.height; ++r) {
      if (predefined[r] > 4) return Refuse(w + ": predefined type " + std::to_string(predefined[r]) + " of row " + std::to_string(r));
    }
  }
  DeviceBuffer scan;
  if (zmx_internal_device_pointer(w.c_str(), image->d_pixels, g.linebytes * g.height, &scan.device) != 0) return -1;
  if (zmx_internal_device_alloc(scan.device, g.scanlines, &scan.p) != 0) return -1;
  // (the context is held for the types and the rows only)
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    return zmx_internal_png_scanlines(ctx, image->d_pixels, g.linebytes, g.height, g.bytewidth, strategy, kBruteWindow,
                                      predefined, scan.p);
  }, scan.device);
  if (rc != 0) return -1;
  File file;
  file.Begin(*image);
  if (zmx_compress_device(options, ZOPFLI_FORMAT_ZLIB, scan.p, g.scanlines, &file.bytes, &file.size) != 0) return -1;
  if (!file.Close()) return BadStream(w);
  file.GiveTo(out, outsize);
  return 0;
}

extern "C" int zmx_png_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                           unsigned char** out, size_t* outsize) {
  const std::string w = "zmx_png_encode_device_batch";
  if (n == 0) return 0;
  if (!options || !images || !out || !outsize) return Refuse(w + ": null argument");
  if (strategy == ZMX_PNG_FILTER_PREDEFINED) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED is the single call's");
  if (!StrategyOk(strategy, false)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  std::vector<Geometry> g(n);
  std::vector<size_t> start(n + 1, 0);   // where image i's scanlines begin in the one buffer
  std::vector<const void*> pixels(n);
  std::vector<size_t> nbytes(n);
  for (size_t i = 0; i < n; ++i) {
    const std::string wi = w + ": image " + std::to_string(i);
    if (CheckImage(wi, images[i], &g[i]) != 0) return -1;
    if (g[i].scanlines > SIZE_MAX - start[i]) return Refuse(w + ": the sizes overflow");
    start[i + 1] = start[i] + g[i].scanlines;
    pixels[i] = images[i].d_pixels;
    nbytes[i] = g[i].linebytes * g[i].height;
  }
  DeviceBuffer scan;
  if (zmx_internal_device_pointers_one_device(w.c_str(), n, pixels.data(), nbytes.data(), &scan.device) != 0) return -1;
  if (zmx_internal_device_alloc(scan.device, start[n], &scan.p) != 0) return -1;
  unsigned char* const base = static_cast<unsigned char*>(scan.p);
  // (one hold of a context for all images; a launch set per image: tools/png_device.py measures what that costs)
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    for (size_t i = 0; i < n; ++i) {
      if (zmx_internal_png_scanlines(ctx, pixels[i], g[i].linebytes, g[i].height, g[i].bytewidth, strategy, kBruteWindow, nullptr,
                                     base + start[i]) != 0) {
        return -1;
      }
    }
    return 0;
  }, scan.device);
  if (rc != 0) return -1;
  std::vector<const void*> slices(n);
  std::vector<size_t> sizes(n);
  std::vector<File> files(n);
  std::vector<unsigned char*> bytes(n);
  std::vector<size_t> filled(n);
  for (size_t i = 0; i < n; ++i) {
    slices[i] = base + start[i];
    sizes[i] = g[i].scanlines;
    files[i].Begin(images[i]);
    bytes[i] = files[i].bytes;
    filled[i] = files[i].size;
  }
  // (a failed call changes none of them: the files still own their arrays)
  if (zmx_compress_device_batch(options, ZOPFLI_FORMAT_ZLIB, n, slices.data(), sizes.data(), bytes.data(), filled.data()) != 0) return -1;
  for (size_t i = 0; i < n; ++i) {
    files[i].bytes = bytes[i];
    files[i].size = filled[i];
  }
  // every file made before any out[i] is touched
  for (size_t i = 0; i < n; ++i) {
    if (!files[i].Close()) return BadStream(w);
  }
  for (size_t i = 0; i < n; ++i) files[i].GiveTo(&out[i], &outsize[i]);
  return 0;
}
