// zmx_png_encode_device, zmx_png_encode_device_batch: an image in device memory as the PNG file zopflipng writes for it
// (include/zopfli_amd.h says which).  The filter types and the filtered scanlines are made on a pooled context of the
// image's device, into a buffer of the call's own that outlives the context's hold: the context goes back to the pool
// BEFORE zmx_compress_device(ZLIB) of the buffer runs, which takes contexts itself.  The stream's second byte and the
// chunks around it are png_container.h's.  (Outside api.cc, as png.cc is: the host-only test library links api.cc
// against a stand-in for the device layer.)
// zmx_png_optimize_device and its batch, further down, reduce the colour mode first: the statistics
// (zmx_png_color_stats_device), LodePNG's choice (png_color_choose.h) and the conversion run on the same hold of the
// context as the types and the rows; a palette file below 4096 bytes is made a second time as RGB or RGBA, on a second
// hold, and the smaller file is kept.
// The _lossy entries put zopflipng's --lossy_8bit and --lossy_transparent in front (zmx_internal_png_lossy_image, on the
// first hold of the context): the 8-bit and the rewritten image go to a buffer of the call's own, and everything after
// runs on that instead of the caller's pixels.  The entries without the suffix are these with lossy = 0.
// ZMX_PNG_FILTER_AUTO is zopflipng's own choice of the strategy (zmx_png_choose_strategy_device, further down): made on the
// first hold of the context, after the rewrite and the 8-bit conversion, image by image in the batches; everything after
// is the entry's path with the strategy chosen.
// The zmx_png_index_* entries, at the end, take a palette or low-bit grey image: k_png_index_use's table of first
// appearances, png_index.h's statistics, mode and conversion table, k_png_index_convert, and from there the other entries'
// path — the trials, the row search, the compression and the tails are shared through RowSource and FinishOptimize*.
// The _to_device entries and zmx_png_encode_device_batch_packed leave the file in device memory: the same first hold (the
// *FrontHalf functions, shared with the host-output entries), then the to-device compress path with the file's frame
// around the stream (device_output_plan.h: PngFrame) and the IDAT's CRC-32 sealed on the device.
// The zmx_png_*_source_* entries, last, take strided, planar, float and 16-bit sources (png_source.h): every source
// checked, one buffer for all packed images, one hold of a context for one k_png_pack launch, then the entry of the same
// name without _source on zmx_png_images that point into the buffer.
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "dealing.h"
#include "deflate.h"
#include "device_output_plan.h"
#include "png_color_choose.h"
#include "png_container.h"
#include "png_index.h"
#include "png_source.h"
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
  return (strategy >= ZMX_PNG_FILTER_ZERO && strategy <= ZMX_PNG_FILTER_BRUTE) || strategy == ZMX_PNG_FILTER_AUTO ||
         (predefined_allowed && strategy == ZMX_PNG_FILTER_PREDEFINED);
}

// _PREDEFINED's types, and the ones _AUTO may be given for its eighth trial
int CheckPredefined(const std::string& w, int strategy, const unsigned char* predefined, size_t height) {
  if (strategy == ZMX_PNG_FILTER_PREDEFINED && !predefined) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED without types");
  if (strategy != ZMX_PNG_FILTER_PREDEFINED && strategy != ZMX_PNG_FILTER_AUTO) return 0;
  for (size_t r = 0; predefined && r < height; ++r) {
    if (predefined[r] > 4) return Refuse(w + ": predefined type " + std::to_string(predefined[r]) + " of row " + std::to_string(r));
  }
  return 0;
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
  size_t prefix_bytes = zamd::kPngPrefixBytes;
  void Begin(const zmx_png_image& im) {
    unsigned char prefix[zamd::kPngPrefixBytes];
    zamd::PngPrefix(im.width, im.height, im.colortype, im.bitdepth, prefix);
    zamd::AppendToOutput(prefix, sizeof(prefix), &bytes, &size);
  }
  // the file of the image in `mode`: PLTE and tRNS where the mode has them
  void BeginReduced(const zmx_png_image& im, const zmx_png_color_mode& mode) { BeginIn(im.width, im.height, mode); }
  // (a mode without a palette and a key gives Begin's bytes)
  void BeginIn(uint32_t width, uint32_t height, const zmx_png_color_mode& mode) {
    unsigned char prefix[zamd::kPngMaxPrefixBytes];
    prefix_bytes = zamd::PngPrefixReduced(width, height, mode.colortype, mode.bitdepth, mode.palette, mode.palettesize,
                                          mode.key_defined != 0, mode.key_r, mode.key_g, mode.key_b, prefix);
    zamd::AppendToOutput(prefix, prefix_bytes, &bytes, &size);
  }
  // the stream is in: what depends on it, and the file's end
  bool Close() {
    unsigned char trailer[zamd::kPngTrailerBytes];
    if (!zamd::PngCloseAt(bytes, size, prefix_bytes, trailer)) return false;
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

// What a _lossy entry makes of an image before anything else (zopflipng_lib.cc:415-428): its 8-bit image where the
// optimize entry has _8BIT and the image is 16 bits deep, the rewrite of the transparent pixels where it has _TRANSPARENT
// and the image is 8-bit by then and has an alpha channel.  bytes: the buffer either takes, 0 where nothing is made.
struct LossyPlan {
  bool to8 = false, transparent = false;
  size_t bytes = 0;
};

LossyPlan PlanLossy(const zmx_png_image& im, const Geometry& g, unsigned lossy, bool optimize) {
  LossyPlan p;
  p.to8 = optimize && (lossy & ZMX_PNG_LOSSY_8BIT) != 0 && im.bitdepth == 16;
  p.transparent = (lossy & ZMX_PNG_LOSSY_TRANSPARENT) != 0 && (im.bitdepth == 8 || p.to8) && (im.colortype == 4 || im.colortype == 6);
  if (p.to8 || p.transparent) p.bytes = g.linebytes / (p.to8 ? 2 : 1) * g.height;
  return p;
}

// The rewrite's kernels index pixels with 32 bits, as the colour statistics do.
int CheckRewritable(const std::string& w, const zmx_png_image& im, const LossyPlan& plan) {
  if (plan.transparent && static_cast<uint64_t>(im.width) * im.height > 0xffffffffull) {
    return Refuse(w + ": an image of 2^32 pixels or more with ZMX_PNG_LOSSY_TRANSPARENT");
  }
  return 0;
}

bool LossyOk(unsigned lossy) { return (lossy & ~(ZMX_PNG_LOSSY_TRANSPARENT | ZMX_PNG_LOSSY_8BIT)) == 0; }

int BadStream(const std::string& w) {
  zmx_internal_set_error((w + ": the zlib stream does not fit an IDAT chunk").c_str(), ZMX_ERR_DEVICE);
  return -1;
}

// Where a to-device entry leaves its file (or, for the packed batch, all files): null for the host-output entries.
struct DeviceDest {
  void* d_out;
  size_t capacity;
};

// What a to-device entry refuses of its destination before anything runs: not plain device memory, another device than
// the images', a byte shared with any of the n images (pixels[i][0, nbytes[i])).
int CheckDest(const std::string& w, const DeviceDest& dest, int img_device, size_t n, const void* const* pixels, const size_t* nbytes) {
  if (dest.capacity != 0 && dest.d_out == nullptr) return Refuse(w + ": d_out: null pointer with a non-zero size");
  int device = -1;
  if (zmx_internal_device_pointer((w + ": d_out").c_str(), dest.d_out, dest.capacity, &device) != 0) return -1;
  if (dest.capacity == 0) return 0;
  if (device != img_device) return Refuse(w + ": the image and d_out lie on different devices");
  const uintptr_t b = reinterpret_cast<uintptr_t>(dest.d_out);
  for (size_t i = 0; i < n; ++i) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(pixels[i]);
    if (a < b + dest.capacity && b < a + nbytes[i]) return Refuse(w + ": d_out overlaps image " + std::to_string(i));
  }
  return 0;
}

// The frame of the file of a width x height image in `mode` (device_output_plan.h)
zamd::PngFrame FrameIn(uint32_t width, uint32_t height, const zmx_png_color_mode& mode) {
  zamd::PngFrame frame;
  frame.file_prefix.resize(zamd::kPngMaxPrefixBytes);
  frame.file_prefix.resize(zamd::PngPrefixReduced(width, height, mode.colortype, mode.bitdepth, mode.palette, mode.palettesize,
                                                  mode.key_defined != 0, mode.key_r, mode.key_g, mode.key_b, frame.file_prefix.data()));
  return frame;
}
// ... of `im`: in `mode`, or as it is (null)
zamd::PngFrame FrameOf(const zmx_png_image& im, const zmx_png_color_mode* mode) {
  if (mode) return FrameIn(im.width, im.height, *mode);
  zamd::PngFrame frame;
  frame.file_prefix.resize(zamd::kPngPrefixBytes);
  zamd::PngPrefix(im.width, im.height, im.colortype, im.bitdepth, frame.file_prefix.data());
  return frame;
}

// room that does for the file around `scanlines` filtered bytes, whatever its prefix
size_t FileBound(size_t scanlines) {
  return zamd::kPngMaxPrefixBytes + zamd::CompressBound(ZOPFLI_FORMAT_ZLIB, scanlines) + zamd::kPngTrailerBytes;
}

}  // namespace

namespace {

// What is made of one image: its statistics, the mode of the first file, the scanlines' size in that mode.
struct Reduced {
  zmx_png_color_stats stats;
  zmx_png_color_mode mode;
  bool as_is = false;      // the mode is the image's own: nothing is converted
  size_t scanlines = 0;    // height * (row bytes + 1)
};

bool SameMode(const zmx_png_image& im, const zmx_png_color_mode& mode) {
  return mode.colortype == im.colortype && mode.bitdepth == im.bitdepth && mode.key_defined == 0;
}

size_t BitsPerPixel(const zmx_png_color_mode& mode) { return (mode.colortype == 3 ? 1 : zamd::PngChannels(mode.colortype)) * mode.bitdepth; }
size_t RowBytesIn(uint32_t width, const zmx_png_color_mode& mode) { return (static_cast<size_t>(width) * BitsPerPixel(mode) + 7) / 8; }
size_t ByteWidthIn(const zmx_png_color_mode& mode) { return BitsPerPixel(mode) < 8 ? 1 : BitsPerPixel(mode) / 8; }
size_t ScanlinesIn(uint32_t width, uint32_t height, const zmx_png_color_mode& mode) {
  return static_cast<size_t>(height) * (RowBytesIn(width, mode) + 1);
}
size_t ScanlinesIn(const zmx_png_image& im, const zmx_png_color_mode& mode) { return ScanlinesIn(im.width, im.height, mode); }

zmx_png_color_mode OwnMode(const zmx_png_image& im) {
  zmx_png_color_mode own = zmx_png_color_mode();
  own.colortype = im.colortype;
  own.bitdepth = im.bitdepth;
  return own;
}

// An image as rows in a colour mode, whatever it is made of (a zmx_png_image: k_png_convert; an index image: its table and
// k_png_index_convert): on a held context the `height` rows of RowBytesIn(width, mode) bytes go to d_room, memory of the
// context's device that the caller owns, and *d_rows = d_room — or *d_rows = where the image lies in that mode already.
struct RowSource {
  uint32_t width, height;
  std::function<int(zmx_ctx* ctx, const zmx_png_color_mode& mode, void* d_room, const void** d_rows)> in_mode;
};

RowSource RowsOf(const zmx_png_image& im) {
  return RowSource{im.width, im.height, [&im](zmx_ctx* ctx, const zmx_png_color_mode& mode, void* d_room, const void** d_rows) {
    if (SameMode(im, mode)) {
      *d_rows = im.d_pixels;
      return 0;
    }
    *d_rows = d_room;
    return zmx_png_convert_device(ctx, &im, &mode, d_room, RowBytesIn(im.width, mode) * im.height);
  }};
}

int CheckReducible(const std::string& w, const zmx_png_image& im, Geometry* g) {
  if (CheckImage(w, im, g) != 0) return -1;
  if (static_cast<uint64_t>(im.width) * im.height > 0xffffffffull) return Refuse(w + ": an image of 2^32 pixels or more");
  return 0;
}

// on a held context: the statistics and the mode of the first file
int StatsAndMode(zmx_ctx* ctx, const zmx_png_image& im, Reduced* r) {
  if (zmx_png_color_stats_device(ctx, &im, &r->stats) != 0) return -1;
  zamd::PngChooseColor(r->stats, static_cast<uint64_t>(im.width) * im.height, &r->mode);
  r->as_is = SameMode(im, r->mode);
  r->scanlines = ScanlinesIn(im, r->mode);
  return 0;
}

// ---- zopflipng's choice of the filter strategy (zopflipng_lib.cc AutoChooseFilterStrategy)
constexpr unsigned kTrialWindow = 8192;
constexpr int kTrialStrategies[8] = {ZMX_PNG_FILTER_ZERO, ZMX_PNG_FILTER_ONE,    ZMX_PNG_FILTER_TWO,     ZMX_PNG_FILTER_THREE,
                                     ZMX_PNG_FILTER_FOUR, ZMX_PNG_FILTER_MINSUM, ZMX_PNG_FILTER_ENTROPY, ZMX_PNG_FILTER_PREDEFINED};

// The file sizes of the trials of an image in `mode` on a held context: the converted rows and the rows of all trials in
// one buffer, one zmx_png_deflate_sizes_device, the container's bytes around each stream.
int TrialFileSizes(zmx_ctx* ctx, const std::string& w, int device, const RowSource& src, const zmx_png_color_mode& mode,
                   const unsigned char* predefined, int ntrials, uint64_t* file_bytes) {
  const size_t scanlines = ScanlinesIn(src.width, src.height, mode), rowbytes = RowBytesIn(src.width, mode);
  if (scanlines > SIZE_MAX / 9) return Refuse(w + ": the sizes overflow");
  const size_t room = (rowbytes * src.height + 15) & ~static_cast<size_t>(15);
  DeviceBuffer buf;
  buf.device = device;
  if (zmx_internal_device_alloc(device, room + scanlines * ntrials, &buf.p) != 0) return -1;
  unsigned char* const trials = static_cast<unsigned char*>(buf.p) + room;
  const void* d_rows = nullptr;
  if (src.in_mode(ctx, mode, buf.p, &d_rows) != 0) return -1;
  if (zmx_internal_png_trial_scanlines(ctx, w.c_str(), d_rows, rowbytes, src.height, ByteWidthIn(mode), predefined, ntrials, trials) != 0) return -1;
  const void* ptrs[8];
  size_t sizes[8];
  uint64_t zlib_bytes[8];
  for (int k = 0; k < ntrials; ++k) {
    ptrs[k] = trials + static_cast<size_t>(k) * scanlines;
    sizes[k] = scanlines;
  }
  if (zmx_png_deflate_sizes_device(ctx, static_cast<size_t>(ntrials), ptrs, sizes, kTrialWindow, zlib_bytes) != 0) return -1;
  unsigned char prefix[zamd::kPngMaxPrefixBytes];
  const size_t prefix_bytes = zamd::PngPrefixReduced(src.width, src.height, mode.colortype, mode.bitdepth, mode.palette, mode.palettesize,
                                                     mode.key_defined != 0, mode.key_r, mode.key_g, mode.key_b, prefix);
  for (int k = 0; k < ntrials; ++k) file_bytes[k] = prefix_bytes + zlib_bytes[k] + zamd::kPngTrailerBytes;
  return 0;
}

// The choice for an image the caller has checked, on a held context: its trials in `mode`.  `stats` non-null: the colour
// mode was reduced (`mode` is the choice of these statistics), so a small palette file competes with its second try.
int ChooseStrategy(zmx_ctx* ctx, const std::string& w, int device, const RowSource& src, const zmx_png_color_mode& mode,
                   const zmx_png_color_stats* stats, const unsigned char* predefined, int* strategy, uint64_t* file_bytes) {
  const int ntrials = predefined ? 8 : 7;
  uint64_t bytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (TrialFileSizes(ctx, w, device, src, mode, predefined, ntrials, bytes) != 0) return -1;
  bool small = false;
  for (int k = 0; k < ntrials; ++k) small = small || bytes[k] < zamd::kPngRetryBelow;
  if (stats && mode.colortype == 3 && small) {
    // TryOptimize's second try sits inside every trial: a small palette file competes with its RGB / RGBA file
    zmx_png_color_mode retry;
    zamd::PngRetryMode(*stats, static_cast<uint64_t>(src.width) * src.height, &retry);
    uint64_t second[8];
    if (TrialFileSizes(ctx, w, device, src, retry, predefined, ntrials, second) != 0) return -1;
    for (int k = 0; k < ntrials; ++k) {
      if (bytes[k] < zamd::kPngRetryBelow && second[k] < bytes[k]) bytes[k] = second[k];
    }
  }
  int best = 0;
  for (int k = 1; k < ntrials; ++k) {
    if (bytes[k] < bytes[best]) best = k;
  }
  *strategy = kTrialStrategies[best];
  if (file_bytes) {
    for (int k = 0; k < 8; ++k) file_bytes[k] = bytes[k];
  }
  return 0;
}

// ... for a zmx_png_image: as it is, or reduced — `known`: its statistics and mode where the caller has them
int ChooseStrategy(zmx_ctx* ctx, const std::string& w, int device, const zmx_png_image& im, bool reduce_color, const Reduced* known,
                   const unsigned char* predefined, int* strategy, uint64_t* file_bytes) {
  if (!reduce_color) return ChooseStrategy(ctx, w, device, RowsOf(im), OwnMode(im), nullptr, predefined, strategy, file_bytes);
  Reduced mine;
  if (!known) {
    if (StatsAndMode(ctx, im, &mine) != 0) return -1;
    known = &mine;
  }
  return ChooseStrategy(ctx, w, device, RowsOf(im), known->mode, &known->stats, predefined, strategy, file_bytes);
}

}  // namespace

extern "C" int zmx_png_choose_strategy_device(zmx_ctx* ctx, const zmx_png_image* image, int reduce_color, const unsigned char* predefined,
                                              int* strategy, uint64_t file_bytes[8]) {
  const std::string w = "zmx_png_choose_strategy_device";
  if (!ctx || !image || !strategy || !file_bytes) return Refuse(w + ": null argument");
  Geometry g;
  if ((reduce_color ? CheckReducible(w, *image, &g) : CheckImage(w, *image, &g)) != 0) return -1;
  if (CheckPredefined(w, ZMX_PNG_FILTER_AUTO, predefined, g.height) != 0) return -1;
  int device = -1;
  if (zmx_internal_device_pointer(w.c_str(), image->d_pixels, g.linebytes * g.height, &device) != 0) return -1;
  int chosen = 0;
  uint64_t bytes[8];
  if (ChooseStrategy(ctx, w, device, *image, reduce_color != 0, nullptr, predefined, &chosen, bytes) != 0) return -1;
  *strategy = chosen;
  for (int k = 0; k < 8; ++k) file_bytes[k] = bytes[k];
  return 0;
}

namespace {

// What zmx_png_encode_device[_lossy] and zmx_png_encode_device_to_device share: the checks (`dest`: the to-device entry's
// destination, checked with them) and the first hold of a context, which leaves the filtered scanlines in `scan`.
struct EncodeFront {
  Geometry g;
  DeviceBuffer scan, rewritten;
};

int EncodeFrontHalf(const std::string& w, const ZopfliOptions* options, const zmx_png_image* image, int strategy, const unsigned char* predefined,
                    unsigned lossy, const DeviceDest* dest, EncodeFront* f) {
  if (!options || !image) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  Geometry& g = f->g;
  if (CheckImage(w, *image, &g) != 0) return -1;
  if (!StrategyOk(strategy, true)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  if (CheckPredefined(w, strategy, predefined, g.height) != 0) return -1;
  const LossyPlan plan = PlanLossy(*image, g, lossy, false);
  if (CheckRewritable(w, *image, plan) != 0) return -1;
  DeviceBuffer& scan = f->scan;
  DeviceBuffer& rewritten = f->rewritten;
  const size_t nbytes = g.linebytes * g.height;
  if (zmx_internal_device_pointer(w.c_str(), image->d_pixels, nbytes, &scan.device) != 0) return -1;
  if (dest && CheckDest(w, *dest, scan.device, 1, &image->d_pixels, &nbytes) != 0) return -1;
  if (zmx_internal_device_alloc(scan.device, g.scanlines, &scan.p) != 0) return -1;
  rewritten.device = scan.device;
  if (plan.bytes != 0 && zmx_internal_device_alloc(scan.device, plan.bytes, &rewritten.p) != 0) return -1;
  zmx_png_image work = *image;
  // (the context is held for the rewrite, the types and the rows only)
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    if (plan.bytes != 0 && zmx_internal_png_lossy_image(ctx, w.c_str(), image, 0, 1, rewritten.p, &work) != 0) return -1;
    if (strategy == ZMX_PNG_FILTER_AUTO && ChooseStrategy(ctx, w, scan.device, work, false, nullptr, predefined, &strategy, nullptr) != 0) return -1;
    return zmx_internal_png_scanlines(ctx, work.d_pixels, g.linebytes, g.height, g.bytewidth, strategy, kBruteWindow, predefined, scan.p);
  }, scan.device);
}

int EncodeOne(const std::string& w, const ZopfliOptions* options, const zmx_png_image* image, int strategy, const unsigned char* predefined,
              unsigned lossy, unsigned char** out, size_t* outsize) {
  if (!options || !image || !out || !outsize) return Refuse(w + ": null argument");
  EncodeFront f;
  if (EncodeFrontHalf(w, options, image, strategy, predefined, lossy, nullptr, &f) != 0) return -1;
  File file;
  file.Begin(*image);
  if (zmx_compress_device(options, ZOPFLI_FORMAT_ZLIB, f.scan.p, f.g.scanlines, &file.bytes, &file.size) != 0) return -1;
  if (!file.Close()) return BadStream(w);
  file.GiveTo(out, outsize);
  return 0;
}

// The file left in device memory: the stream goes zmx_compress_device_to_device's way with the file's frame around it.
int EncodeOneToDevice(const std::string& w, const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                      const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize) {
  if (!options || !image || !outsize) return Refuse(w + ": null argument");
  *outsize = 0;
  const DeviceDest dest{d_out, capacity};
  EncodeFront f;
  if (EncodeFrontHalf(w, options, image, strategy, predefined, lossy, &dest, &f) != 0) return -1;
  const zamd::PngFrame frame = FrameOf(*image, nullptr);
  return zamd::CompressDeviceToDevice(w.c_str(), options, ZOPFLI_FORMAT_ZLIB, f.scan.p, f.g.scanlines, d_out, capacity, outsize, &frame);
}

// What zmx_png_encode_device_batch[_lossy] and zmx_png_encode_device_batch_packed share (n > 0): the checks (`dest`: the
// arena, checked with them) and the one hold of a context, which leaves image i's filtered scanlines at scan + start[i].
struct BatchFront {
  std::vector<Geometry> g;
  std::vector<size_t> start;
  DeviceBuffer scan, rewritten;
};

int EncodeBatchFrontHalf(const std::string& w, const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy, unsigned lossy,
                         const DeviceDest* dest, BatchFront* f) {
  if (!options || !images) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  if (strategy == ZMX_PNG_FILTER_PREDEFINED) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED is the single call's");
  if (!StrategyOk(strategy, false)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  std::vector<Geometry>& g = f->g;
  std::vector<size_t>& start = f->start;   // where image i's scanlines begin in the one buffer
  g.resize(n);
  start.assign(n + 1, 0);
  std::vector<size_t> rstart(n + 1, 0);  // and its rewritten pixels in theirs
  std::vector<LossyPlan> plan(n);
  std::vector<const void*> pixels(n);
  std::vector<size_t> nbytes(n);
  for (size_t i = 0; i < n; ++i) {
    const std::string wi = w + ": image " + std::to_string(i);
    if (CheckImage(wi, images[i], &g[i]) != 0) return -1;
    if (g[i].scanlines > SIZE_MAX - start[i]) return Refuse(w + ": the sizes overflow");
    start[i + 1] = start[i] + g[i].scanlines;
    plan[i] = PlanLossy(images[i], g[i], lossy, false);
    if (CheckRewritable(wi, images[i], plan[i]) != 0) return -1;
    rstart[i + 1] = rstart[i] + ((plan[i].bytes + 15) & ~static_cast<size_t>(15));
    pixels[i] = images[i].d_pixels;
    nbytes[i] = g[i].linebytes * g[i].height;
  }
  DeviceBuffer& scan = f->scan;
  DeviceBuffer& rewritten = f->rewritten;
  if (zmx_internal_device_pointers_one_device(w.c_str(), n, pixels.data(), nbytes.data(), &scan.device) != 0) return -1;
  if (dest && CheckDest(w, *dest, scan.device, n, pixels.data(), nbytes.data()) != 0) return -1;
  if (zmx_internal_device_alloc(scan.device, start[n], &scan.p) != 0) return -1;
  rewritten.device = scan.device;
  if (rstart[n] != 0 && zmx_internal_device_alloc(scan.device, rstart[n], &rewritten.p) != 0) return -1;
  unsigned char* const base = static_cast<unsigned char*>(scan.p);
  // (one hold of a context for all images; a launch set per image: tools/png_device.py measures what that costs)
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    for (size_t i = 0; i < n; ++i) {
      zmx_png_image work = images[i];
      if (plan[i].bytes != 0 &&
          zmx_internal_png_lossy_image(ctx, w.c_str(), &images[i], 0, 1, static_cast<unsigned char*>(rewritten.p) + rstart[i], &work) != 0) {
        return -1;
      }
      int chosen = strategy;
      if (strategy == ZMX_PNG_FILTER_AUTO && ChooseStrategy(ctx, w, scan.device, work, false, nullptr, nullptr, &chosen, nullptr) != 0) return -1;
      if (zmx_internal_png_scanlines(ctx, work.d_pixels, g[i].linebytes, g[i].height, g[i].bytewidth, chosen, kBruteWindow, nullptr,
                                     base + start[i]) != 0) {
        return -1;
      }
    }
    return 0;
  }, scan.device);
}

int EncodeBatch(const std::string& w, const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy, unsigned lossy,
                unsigned char** out, size_t* outsize) {
  if (n == 0) return 0;
  if (!options || !images || !out || !outsize) return Refuse(w + ": null argument");
  BatchFront f;
  if (EncodeBatchFrontHalf(w, options, n, images, strategy, lossy, nullptr, &f) != 0) return -1;
  const std::vector<Geometry>& g = f.g;
  const std::vector<size_t>& start = f.start;
  unsigned char* const base = static_cast<unsigned char*>(f.scan.p);
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

// The files left in one arena: zmx_compress_device_batch_packed's plan with a frame per stream.
int EncodeBatchPacked(const std::string& w, const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy, unsigned lossy,
                      void* d_arena, size_t capacity, size_t align, size_t* outoffset, size_t* outsize) {
  if (n == 0) return 0;
  if (!options || !images || !outoffset || !outsize) return Refuse(w + ": null argument");
  if (!zamd::PackedAlignOk(align)) return Refuse(w + ": align " + std::to_string(align) + " is not a power of two from 1 to 4096");
  const DeviceDest dest{d_arena, capacity};
  BatchFront f;
  if (EncodeBatchFrontHalf(w, options, n, images, strategy, lossy, &dest, &f) != 0) return -1;
  std::vector<const void*> slices(n);
  std::vector<size_t> sizes(n);
  std::vector<zamd::PngFrame> frames(n);
  for (size_t i = 0; i < n; ++i) {
    slices[i] = static_cast<unsigned char*>(f.scan.p) + f.start[i];
    sizes[i] = f.g[i].scanlines;
    frames[i] = FrameOf(images[i], nullptr);
  }
  return zamd::CompressDeviceBatchPackedFramed(w.c_str(), options, n, slices.data(), sizes.data(), frames.data(), d_arena, capacity, align,
                                               outoffset, outsize);
}

}  // namespace

extern "C" size_t zmx_png_bound(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth) {
  if (width == 0 || height == 0 || !zamd::PngFormatOk(colortype, bitdepth)) return 0;
  return zamd::PngBound(width, height, colortype, bitdepth);
}
extern "C" size_t zmx_png_batch_bound(size_t n, const zmx_png_image* images, size_t align) {
  if (n == 0 || !images || !zamd::PackedAlignOk(align)) return 0;
  for (size_t i = 0; i < n; ++i) {
    if (images[i].width == 0 || images[i].height == 0 || !zamd::PngFormatOk(images[i].colortype, images[i].bitdepth)) return 0;
  }
  return zamd::PngBatchBound(n, images, align);
}
extern "C" int zmx_png_encode_device_to_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                               const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize) {
  return EncodeOneToDevice("zmx_png_encode_device_to_device", options, image, strategy, predefined, lossy, d_out, capacity, outsize);
}
extern "C" int zmx_png_encode_device_batch_packed(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                                  unsigned lossy, void* d_arena, size_t capacity, size_t align, size_t* outoffset,
                                                  size_t* outsize) {
  return EncodeBatchPacked("zmx_png_encode_device_batch_packed", options, n, images, strategy, lossy, d_arena, capacity, align, outoffset,
                           outsize);
}

extern "C" int zmx_png_encode_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                     const unsigned char* predefined, unsigned char** out, size_t* outsize) {
  return EncodeOne("zmx_png_encode_device", options, image, strategy, predefined, 0, out, outsize);
}
extern "C" int zmx_png_encode_device_lossy(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                           const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return EncodeOne("zmx_png_encode_device_lossy", options, image, strategy, predefined, lossy, out, outsize);
}
extern "C" int zmx_png_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                           unsigned char** out, size_t* outsize) {
  return EncodeBatch("zmx_png_encode_device_batch", options, n, images, strategy, 0, out, outsize);
}
extern "C" int zmx_png_encode_device_batch_lossy(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                                 unsigned lossy, unsigned char** out, size_t* outsize) {
  return EncodeBatch("zmx_png_encode_device_batch_lossy", options, n, images, strategy, lossy, out, outsize);
}

// ---- zmx_png_optimize_device, zmx_png_optimize_device_batch: the colour mode reduced first (png_color_choose.h)
extern "C" int zmx_png_choose_color(const zmx_png_color_stats* stats, uint64_t numpixels, zmx_png_color_mode* out) {
  if (!stats || !out) return Refuse("zmx_png_choose_color: null argument");
  zamd::PngChooseColor(*stats, numpixels, out);
  return 0;
}

namespace {

// Of two closed files of one image the one zopflipng keeps: the second only when it is strictly smaller.
File& Smaller(File& first, File& second) { return second.size < first.size ? second : first; }

}  // namespace

namespace {

// What zmx_png_optimize_device[_lossy] and zmx_png_optimize_device_to_device share: the checks (`dest`: the to-device
// entry's destination, checked with them) and the first hold of a context, which leaves the first file's scanlines in
// `scan`; and the second try's scanlines, on a second hold.
struct OptimizeFront {
  int device = -1;
  int strategy = 0;         // the one the rows were made with (_AUTO: the chosen one)
  Reduced r;
  DeviceBuffer scan, rewritten;
  zmx_png_image work;       // what is encoded: the caller's image, or its 8-bit or rewritten image in `rewritten`
};

int OptimizeFrontHalf(const std::string& w, const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                      const unsigned char* predefined, unsigned lossy, const DeviceDest* dest, OptimizeFront* f) {
  if (!options || !image) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  Geometry g;
  if (CheckReducible(w, *image, &g) != 0) return -1;
  if (!StrategyOk(strategy, true)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  if (CheckPredefined(w, strategy, predefined, g.height) != 0) return -1;
  int& device = f->device;
  const size_t nbytes = g.linebytes * g.height;
  if (zmx_internal_device_pointer(w.c_str(), image->d_pixels, nbytes, &device) != 0) return -1;
  if (dest && CheckDest(w, *dest, device, 1, &image->d_pixels, &nbytes) != 0) return -1;
  const LossyPlan plan = PlanLossy(*image, g, lossy, true);
  Reduced& r = f->r;
  DeviceBuffer& scan = f->scan;
  DeviceBuffer& rewritten = f->rewritten;
  scan.device = rewritten.device = device;
  if (plan.bytes != 0 && zmx_internal_device_alloc(device, plan.bytes, &rewritten.p) != 0) return -1;
  zmx_png_image& work = f->work;
  work = *image;
  // (the context is held for the rewrite, the statistics, the conversion, the types and the rows only)
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    if (plan.bytes != 0 && zmx_internal_png_lossy_image(ctx, w.c_str(), image, plan.to8, plan.transparent, rewritten.p, &work) != 0) return -1;
    if (StatsAndMode(ctx, work, &r) != 0) return -1;
    if (strategy == ZMX_PNG_FILTER_AUTO && ChooseStrategy(ctx, w, device, work, true, &r, predefined, &strategy, nullptr) != 0) return -1;
    if (zmx_internal_device_alloc(device, r.scanlines, &scan.p) != 0) return -1;
    return zmx_internal_png_reduced_scanlines(ctx, &work, r.as_is ? nullptr : &r.mode, strategy, kBruteWindow, predefined, scan.p);
  }, device);
  f->strategy = strategy;
  return rc;
}

// its mode and its scanlines, into scan2
int SecondTryScanlines(const OptimizeFront& f, const unsigned char* predefined, zmx_png_color_mode* retry, bool* as_is, size_t* scanlines,
                       DeviceBuffer* scan2) {
  zamd::PngRetryMode(f.r.stats, static_cast<uint64_t>(f.work.width) * f.work.height, retry);
  *as_is = SameMode(f.work, *retry);
  *scanlines = ScanlinesIn(f.work, *retry);
  scan2->device = f.device;
  if (zmx_internal_device_alloc(f.device, *scanlines, &scan2->p) != 0) return -1;
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    return zmx_internal_png_reduced_scanlines(ctx, &f.work, *as_is ? nullptr : retry, f.strategy, kBruteWindow, predefined, scan2->p);
  }, f.device);
}

// zopflipng's second try at a small palette file, made by whoever holds the image: its mode, its scanlines' size and the
// scanlines, into a buffer allocated here.  0, or -1 with the error set.
using SecondTry = std::function<int(zmx_png_color_mode* retry, size_t* scanlines, DeviceBuffer* scan2)>;

// What the optimize entries with host output share once the first file's scanlines lie in `scan`: the file in `mode`, the
// second try where it is a palette file below 4096 bytes, the smaller of the two handed over.
int FinishOptimize(const std::string& w, const ZopfliOptions* options, uint32_t width, uint32_t height, const zmx_png_color_mode& mode,
                   const void* d_scan, size_t scanlines, const SecondTry& second_try, unsigned char** out, size_t* outsize) {
  File file;
  file.BeginIn(width, height, mode);
  if (zmx_compress_device(options, ZOPFLI_FORMAT_ZLIB, d_scan, scanlines, &file.bytes, &file.size) != 0) return -1;
  if (!file.Close()) return BadStream(w);
  File second;
  if (mode.colortype == 3 && file.size < zamd::kPngRetryBelow) {
    zmx_png_color_mode retry;
    size_t scanlines2 = 0;
    DeviceBuffer scan2;
    if (second_try(&retry, &scanlines2, &scan2) != 0) return -1;
    second.BeginIn(width, height, retry);
    if (zmx_compress_device(options, ZOPFLI_FORMAT_ZLIB, scan2.p, scanlines2, &second.bytes, &second.size) != 0) return -1;
    if (!second.Close()) return BadStream(w);
    Smaller(file, second).GiveTo(out, outsize);
    return 0;
  }
  file.GiveTo(out, outsize);
  return 0;
}

// The same with the file left in device memory.  A mode other than a palette: the one file goes straight into d_out, as the
// encode entry's.  A palette: which file is kept, and so its size, is known only when the first is made — so the first goes
// into a buffer of the call's own, the second (where one is due) into another, and ONE device-to-device copy puts the kept
// file into d_out: every byte of the file is written and none outside it, and a capacity of exactly the kept file's size does.
int FinishOptimizeToDevice(const std::string& w, const ZopfliOptions* options, int device, uint32_t width, uint32_t height,
                           const zmx_png_color_mode& mode, const void* d_scan, size_t scanlines, const SecondTry& second_try, void* d_out,
                           size_t capacity, size_t* outsize) {
  const zamd::PngFrame frame = FrameIn(width, height, mode);
  if (mode.colortype != 3) {
    return zamd::CompressDeviceToDevice(w.c_str(), options, ZOPFLI_FORMAT_ZLIB, d_scan, scanlines, d_out, capacity, outsize, &frame);
  }
  DeviceBuffer first, second;
  first.device = second.device = device;
  const size_t room = FileBound(scanlines);
  size_t first_bytes = 0, second_bytes = 0;
  if (zmx_internal_device_alloc(device, room, &first.p) != 0) return -1;
  if (zamd::CompressDeviceToDevice(w.c_str(), options, ZOPFLI_FORMAT_ZLIB, d_scan, scanlines, first.p, room, &first_bytes, &frame) != 0) {
    *outsize = first_bytes;   // (a stream that fits no IDAT: the size it would have taken)
    return -1;
  }
  const void* kept = first.p;
  size_t kept_bytes = first_bytes;
  if (first_bytes < zamd::kPngRetryBelow) {
    zmx_png_color_mode retry;
    size_t scanlines2 = 0;
    DeviceBuffer scan2;
    if (second_try(&retry, &scanlines2, &scan2) != 0) return -1;
    const zamd::PngFrame frame2 = FrameIn(width, height, retry);
    const size_t room2 = FileBound(scanlines2);
    if (zmx_internal_device_alloc(device, room2, &second.p) != 0) return -1;
    if (zamd::CompressDeviceToDevice(w.c_str(), options, ZOPFLI_FORMAT_ZLIB, scan2.p, scanlines2, second.p, room2, &second_bytes, &frame2) != 0) return -1;
    if (second_bytes < first_bytes) {
      kept = second.p;
      kept_bytes = second_bytes;
    }
  }
  *outsize = kept_bytes;
  if (kept_bytes > capacity) {
    return Refuse(w + ": the file takes " + std::to_string(kept_bytes) + " bytes, d_out has " + std::to_string(capacity));
  }
  return zmx_internal_device_copy(device, d_out, kept, kept_bytes);
}

SecondTry SecondTryOf(const OptimizeFront& f, const unsigned char* predefined) {
  return [&f, predefined](zmx_png_color_mode* retry, size_t* scanlines, DeviceBuffer* scan2) {
    bool as_is = false;
    return SecondTryScanlines(f, predefined, retry, &as_is, scanlines, scan2);
  };
}

int OptimizeOne(const std::string& w, const ZopfliOptions* options, const zmx_png_image* image, int strategy, const unsigned char* predefined,
                unsigned lossy, unsigned char** out, size_t* outsize) {
  if (!options || !image || !out || !outsize) return Refuse(w + ": null argument");
  OptimizeFront f;
  if (OptimizeFrontHalf(w, options, image, strategy, predefined, lossy, nullptr, &f) != 0) return -1;
  return FinishOptimize(w, options, f.work.width, f.work.height, f.r.mode, f.scan.p, f.r.scanlines, SecondTryOf(f, predefined), out, outsize);
}

int OptimizeOneToDevice(const std::string& w, const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                        const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize) {
  if (!options || !image || !outsize) return Refuse(w + ": null argument");
  *outsize = 0;
  const DeviceDest dest{d_out, capacity};
  OptimizeFront f;
  if (OptimizeFrontHalf(w, options, image, strategy, predefined, lossy, &dest, &f) != 0) return -1;
  return FinishOptimizeToDevice(w, options, f.device, f.work.width, f.work.height, f.r.mode, f.scan.p, f.r.scanlines,
                                SecondTryOf(f, predefined), d_out, capacity, outsize);
}

}  // namespace

extern "C" int zmx_png_optimize_device_to_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                                 const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                 size_t* outsize) {
  return OptimizeOneToDevice("zmx_png_optimize_device_to_device", options, image, strategy, predefined, lossy, d_out, capacity, outsize);
}

extern "C" int zmx_png_optimize_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                       const unsigned char* predefined, unsigned char** out, size_t* outsize) {
  return OptimizeOne("zmx_png_optimize_device", options, image, strategy, predefined, 0, out, outsize);
}
extern "C" int zmx_png_optimize_device_lossy(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                             const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return OptimizeOne("zmx_png_optimize_device_lossy", options, image, strategy, predefined, lossy, out, outsize);
}

namespace {

// One zmx_compress_device_batch over the scanlines of the images `which` — image which[k]'s at base + start[k], in
// modes[k] (as_is[k]: the image's own) — into files[k], closed.
int CompressInto(const ZopfliOptions* options, const std::string& w, const zmx_png_image* images, const std::vector<size_t>& which,
                 const std::vector<zmx_png_color_mode>& modes, const std::vector<char>& as_is, const unsigned char* base,
                 const std::vector<size_t>& start, std::vector<File>* files) {
  const size_t m = which.size();
  std::vector<const void*> slices(m);
  std::vector<size_t> sizes(m), filled(m);
  std::vector<unsigned char*> bytes(m);
  for (size_t k = 0; k < m; ++k) {
    slices[k] = base + start[k];
    sizes[k] = start[k + 1] - start[k];
    if (as_is[k]) (*files)[k].Begin(images[which[k]]);
    else (*files)[k].BeginReduced(images[which[k]], modes[k]);
    bytes[k] = (*files)[k].bytes;
    filled[k] = (*files)[k].size;
  }
  // (a failed call changes none of them: the files still own their arrays)
  if (zmx_compress_device_batch(options, ZOPFLI_FORMAT_ZLIB, m, slices.data(), sizes.data(), bytes.data(), filled.data()) != 0) return -1;
  for (size_t k = 0; k < m; ++k) {
    (*files)[k].bytes = bytes[k];
    (*files)[k].size = filled[k];
  }
  for (size_t k = 0; k < m; ++k) {
    if (!(*files)[k].Close()) return BadStream(w);
  }
  return 0;
}

}  // namespace

namespace {

int OptimizeBatch(const std::string& w, const ZopfliOptions* options, size_t n, const zmx_png_image* callers, int strategy, unsigned lossy,
                  unsigned char** out, size_t* outsize) {
  if (n == 0) return 0;
  if (!options || !callers || !out || !outsize) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  if (strategy == ZMX_PNG_FILTER_PREDEFINED) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED is the single call's");
  if (!StrategyOk(strategy, false)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  std::vector<const void*> pixels(n);
  std::vector<size_t> nbytes(n);
  std::vector<LossyPlan> plan(n);
  std::vector<size_t> rstart(n + 1, 0);   // where image i's 8-bit or rewritten pixels begin in their buffer
  for (size_t i = 0; i < n; ++i) {
    Geometry g;
    if (CheckReducible(w + ": image " + std::to_string(i), callers[i], &g) != 0) return -1;
    pixels[i] = callers[i].d_pixels;
    nbytes[i] = g.linebytes * g.height;
    plan[i] = PlanLossy(callers[i], g, lossy, true);
    rstart[i + 1] = rstart[i] + ((plan[i].bytes + 15) & ~static_cast<size_t>(15));
  }
  int device = -1;
  if (zmx_internal_device_pointers_one_device(w.c_str(), n, pixels.data(), nbytes.data(), &device) != 0) return -1;
  DeviceBuffer rewritten;
  rewritten.device = device;
  if (rstart[n] != 0 && zmx_internal_device_alloc(device, rstart[n], &rewritten.p) != 0) return -1;
  // what is encoded: the callers' images, or their 8-bit or rewritten images in `rewritten`
  std::vector<zmx_png_image> work(callers, callers + n);
  const zmx_png_image* const images = work.data();
  // the first files: statistics for all, one buffer, conversion and rows image by image, on one hold of a context
  std::vector<Reduced> r(n);
  std::vector<int> chosen(n, strategy);   // (_AUTO: the strategy of each image's own trials)
  std::vector<size_t> all(n), start(n + 1, 0);
  std::vector<zmx_png_color_mode> modes(n);
  std::vector<char> as_is(n);
  DeviceBuffer scan;
  scan.device = device;
  int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    for (size_t i = 0; i < n; ++i) {
      if (plan[i].bytes != 0 && zmx_internal_png_lossy_image(ctx, w.c_str(), &callers[i], plan[i].to8, plan[i].transparent,
                                                             static_cast<unsigned char*>(rewritten.p) + rstart[i], &work[i]) != 0) {
        return -1;
      }
      if (StatsAndMode(ctx, images[i], &r[i]) != 0) return -1;
      if (strategy == ZMX_PNG_FILTER_AUTO && ChooseStrategy(ctx, w, device, images[i], true, &r[i], nullptr, &chosen[i], nullptr) != 0) return -1;
      if (r[i].scanlines > SIZE_MAX - start[i]) return Refuse(w + ": the sizes overflow");
      start[i + 1] = start[i] + r[i].scanlines;
    }
    if (zmx_internal_device_alloc(device, start[n], &scan.p) != 0) return -1;
    for (size_t i = 0; i < n; ++i) {
      if (zmx_internal_png_reduced_scanlines(ctx, &images[i], r[i].as_is ? nullptr : &r[i].mode, chosen[i], kBruteWindow, nullptr,
                                             static_cast<unsigned char*>(scan.p) + start[i]) != 0) {
        return -1;
      }
    }
    return 0;
  }, device);
  if (rc != 0) return -1;
  for (size_t i = 0; i < n; ++i) {
    all[i] = i;
    modes[i] = r[i].mode;
    as_is[i] = r[i].as_is ? 1 : 0;
  }
  std::vector<File> files(n);
  if (CompressInto(options, w, images, all, modes, as_is, static_cast<const unsigned char*>(scan.p), start, &files) != 0) return -1;
  // zopflipng's second try at the small palette files, all of them in one more batch
  std::vector<size_t> again;
  for (size_t i = 0; i < n; ++i) {
    if (r[i].mode.colortype == 3 && files[i].size < zamd::kPngRetryBelow) again.push_back(i);
  }
  std::vector<File> seconds(again.size());
  if (!again.empty()) {
    const size_t m = again.size();
    std::vector<zmx_png_color_mode> modes2(m);
    std::vector<char> as_is2(m);
    std::vector<size_t> start2(m + 1, 0);
    for (size_t k = 0; k < m; ++k) {
      const zmx_png_image& im = images[again[k]];
      zamd::PngRetryMode(r[again[k]].stats, static_cast<uint64_t>(im.width) * im.height, &modes2[k]);
      as_is2[k] = SameMode(im, modes2[k]) ? 1 : 0;
      start2[k + 1] = start2[k] + ScanlinesIn(im, modes2[k]);
    }
    DeviceBuffer scan2;
    scan2.device = device;
    if (zmx_internal_device_alloc(device, start2[m], &scan2.p) != 0) return -1;
    rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
      for (size_t k = 0; k < m; ++k) {
        if (zmx_internal_png_reduced_scanlines(ctx, &images[again[k]], as_is2[k] ? nullptr : &modes2[k], chosen[again[k]], kBruteWindow, nullptr,
                                               static_cast<unsigned char*>(scan2.p) + start2[k]) != 0) {
          return -1;
        }
      }
      return 0;
    }, device);
    if (rc != 0) return -1;
    if (CompressInto(options, w, images, again, modes2, as_is2, static_cast<const unsigned char*>(scan2.p), start2, &seconds) != 0) return -1;
  }
  // every file made before any out[i] is touched
  std::vector<File*> kept(n);
  for (size_t i = 0; i < n; ++i) kept[i] = &files[i];
  for (size_t k = 0; k < again.size(); ++k) kept[again[k]] = &Smaller(files[again[k]], seconds[k]);
  for (size_t i = 0; i < n; ++i) kept[i]->GiveTo(&out[i], &outsize[i]);
  return 0;
}

}  // namespace

extern "C" int zmx_png_optimize_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                             unsigned char** out, size_t* outsize) {
  return OptimizeBatch("zmx_png_optimize_device_batch", options, n, images, strategy, 0, out, outsize);
}
extern "C" int zmx_png_optimize_device_batch_lossy(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                                   unsigned lossy, unsigned char** out, size_t* outsize) {
  return OptimizeBatch("zmx_png_optimize_device_batch_lossy", options, n, images, strategy, lossy, out, outsize);
}

// ---- palette, 1/2/4-bit grey and index images (png_index.h; device/zmx_png_index.h)
namespace {

// What is refused of an index image on the host, before its pointer is looked at; *nbytes its size.
int CheckIndexImage(const std::string& w, const zmx_png_index_image& im, size_t* nbytes) {
  if (im.width == 0 || im.height == 0) return Refuse(w + ": width or height 0");
  if (!zamd::PngIndexFormatOk(im.colortype, im.bitdepth)) {
    return Refuse(w + ": colour type " + std::to_string(im.colortype) + " at " + std::to_string(im.bitdepth) +
                  " bits is no index image (3 at 1, 2, 4, 8; 0 at 1, 2, 4)");
  }
  if (!zamd::PngIndexPaletteSizeOk(im)) {
    return Refuse(w + ": a palette of " + std::to_string(im.palettesize) + " entries at " + std::to_string(im.bitdepth) + " bits");
  }
  if (static_cast<uint64_t>(im.width) * im.height > 0xffffffffull) return Refuse(w + ": an image of 2^32 pixels or more");
  const uint64_t linebytes = (static_cast<uint64_t>(im.width) * im.bitdepth + 7) / 8;
  if (linebytes > 0x7fffffffu || im.height > 0x7fffffffu) return Refuse(w + ": bad geometry");
  *nbytes = static_cast<size_t>(linebytes) * im.height;
  return 0;
}

// What the host makes of an image's first appearances: the entries as zopflipng sees them (after --lossy_transparent where
// asked), the statistics of the expansion, and the mode of the first file — LodePNG's choice, or the input's own.
struct IndexPlan {
  uint64_t first[256];
  zamd::PngIndexPalette seen;
  zmx_png_color_stats stats;
  zmx_png_color_mode mode;
};

int CheckInsidePalette(const std::string& w, const zmx_png_index_image& im, const uint64_t first[256]) {
  zamd::PngIndexPalette p;
  zamd::PngIndexPaletteOf(im, &p);
  const uint64_t outside = zamd::PngIndexFirstOutside(first, p.size);
  if (outside == zamd::kPngIndexUnused) return 0;
  return Refuse(w + ": pixel " + std::to_string(outside) + " has a value outside the palette of " + std::to_string(p.size) + " entries");
}

int PlanIndex(const std::string& w, const zmx_png_index_image& im, unsigned lossy, bool optimize, IndexPlan* plan) {
  if (CheckInsidePalette(w, im, plan->first) != 0) return -1;
  zamd::PngIndexPaletteOf(im, &plan->seen);
  if (lossy & ZMX_PNG_LOSSY_TRANSPARENT) zamd::PngIndexLossyTransparent(&plan->seen, plan->first);
  zamd::PngIndexColorStats(plan->seen, plan->first, &plan->stats);
  if (optimize) {
    zamd::PngChooseColor(plan->stats, static_cast<uint64_t>(im.width) * im.height, &plan->mode);
  } else {
    uint32_t table[256];
    zamd::PngIndexKeepPlan(im, plan->first, (lossy & ZMX_PNG_LOSSY_TRANSPARENT) != 0, &plan->mode, table);
  }
  return 0;
}

RowSource RowsOf(const zmx_png_index_image& im, const zamd::PngIndexPalette& seen) {
  return RowSource{im.width, im.height, [&im, &seen](zmx_ctx* ctx, const zmx_png_color_mode& mode, void* d_room, const void** d_rows) {
    uint32_t table[256];
    zamd::PngIndexTable(seen, mode, table);
    *d_rows = d_room;
    return zmx_png_index_convert_device(ctx, &im, &mode, table, d_room, RowBytesIn(im.width, mode) * im.height);
  }};
}

// On a held context: the image in `mode` (into d_room, RowBytesIn * height bytes) and the filtered scanlines of that under
// `strategy` into d_scan, ScanlinesIn bytes; both the caller's.
int ScanlinesOf(zmx_ctx* ctx, const RowSource& src, const zmx_png_color_mode& mode, int strategy, const unsigned char* predefined, void* d_room,
                void* d_scan) {
  const void* d_rows = nullptr;
  if (src.in_mode(ctx, mode, d_room, &d_rows) != 0) return -1;
  return zmx_internal_png_scanlines(ctx, d_rows, RowBytesIn(src.width, mode), src.height, ByteWidthIn(mode), strategy, kBruteWindow, predefined,
                                    d_scan);
}

// ... with both buffers allocated here; the scanlines stay in *scan
int ScanlinesOf(zmx_ctx* ctx, int device, const RowSource& src, const zmx_png_color_mode& mode, int strategy, const unsigned char* predefined,
                DeviceBuffer* scan) {
  DeviceBuffer room;
  room.device = scan->device = device;
  if (zmx_internal_device_alloc(device, RowBytesIn(src.width, mode) * src.height, &room.p) != 0) return -1;
  if (zmx_internal_device_alloc(device, ScanlinesIn(src.width, src.height, mode), &scan->p) != 0) return -1;
  return ScanlinesOf(ctx, src, mode, strategy, predefined, room.p, scan->p);
}

// What the single index entries share: the checks (`dest`: a to-device entry's destination, checked with them) and the
// first hold of a context, which leaves the first file's scanlines in `scan`.
struct IndexFront {
  int device = -1;
  int strategy = 0;   // the one the rows were made with (_AUTO: the chosen one)
  IndexPlan plan;
  size_t scanlines = 0;
  DeviceBuffer scan;
};

int IndexFrontHalf(const std::string& w, const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                   const unsigned char* predefined, unsigned lossy, bool optimize, const DeviceDest* dest, IndexFront* f) {
  if (!options || !image) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  size_t nbytes = 0;
  if (CheckIndexImage(w, *image, &nbytes) != 0) return -1;
  if (!StrategyOk(strategy, true)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  if (CheckPredefined(w, strategy, predefined, image->height) != 0) return -1;
  if (zmx_internal_device_pointer(w.c_str(), image->d_pixels, nbytes, &f->device) != 0) return -1;
  if (dest && CheckDest(w, *dest, f->device, 1, &image->d_pixels, &nbytes) != 0) return -1;
  IndexPlan& plan = f->plan;
  // (the context is held for the first appearances, the trials, the conversion, the types and the rows only)
  const int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    if (zmx_png_index_use_device(ctx, image, plan.first) != 0) return -1;
    if (PlanIndex(w, *image, lossy, optimize, &plan) != 0) return -1;
    const RowSource src = RowsOf(*image, plan.seen);
    if (strategy == ZMX_PNG_FILTER_AUTO &&
        ChooseStrategy(ctx, w, f->device, src, plan.mode, optimize ? &plan.stats : nullptr, predefined, &strategy, nullptr) != 0) {
      return -1;
    }
    f->scanlines = ScanlinesIn(image->width, image->height, plan.mode);
    return ScanlinesOf(ctx, f->device, src, plan.mode, strategy, predefined, &f->scan);
  }, f->device);
  f->strategy = strategy;
  return rc;
}

// the second try's mode and scanlines, on a second hold
SecondTry SecondTryOf(const IndexFront& f, const zmx_png_index_image& image, const unsigned char* predefined) {
  return [&f, &image, predefined](zmx_png_color_mode* retry, size_t* scanlines, DeviceBuffer* scan2) {
    zamd::PngRetryMode(f.plan.stats, static_cast<uint64_t>(image.width) * image.height, retry);
    *scanlines = ScanlinesIn(image.width, image.height, *retry);
    return zamd::OnPooledContext([&](zmx_ctx* ctx) {
      return ScanlinesOf(ctx, f.device, RowsOf(image, f.plan.seen), *retry, f.strategy, predefined, scan2);
    }, f.device);
  };
}

int IndexOne(const std::string& w, const ZopfliOptions* options, const zmx_png_index_image* image, int strategy, const unsigned char* predefined,
             unsigned lossy, bool optimize, unsigned char** out, size_t* outsize) {
  if (!options || !image || !out || !outsize) return Refuse(w + ": null argument");
  IndexFront f;
  if (IndexFrontHalf(w, options, image, strategy, predefined, lossy, optimize, nullptr, &f) != 0) return -1;
  if (optimize) {
    return FinishOptimize(w, options, image->width, image->height, f.plan.mode, f.scan.p, f.scanlines, SecondTryOf(f, *image, predefined), out,
                          outsize);
  }
  File file;
  file.BeginIn(image->width, image->height, f.plan.mode);
  if (zmx_compress_device(options, ZOPFLI_FORMAT_ZLIB, f.scan.p, f.scanlines, &file.bytes, &file.size) != 0) return -1;
  if (!file.Close()) return BadStream(w);
  file.GiveTo(out, outsize);
  return 0;
}

int IndexOneToDevice(const std::string& w, const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                     const unsigned char* predefined, unsigned lossy, bool optimize, void* d_out, size_t capacity, size_t* outsize) {
  if (!options || !image || !outsize) return Refuse(w + ": null argument");
  *outsize = 0;
  const DeviceDest dest{d_out, capacity};
  IndexFront f;
  if (IndexFrontHalf(w, options, image, strategy, predefined, lossy, optimize, &dest, &f) != 0) return -1;
  if (optimize) {
    return FinishOptimizeToDevice(w, options, f.device, image->width, image->height, f.plan.mode, f.scan.p, f.scanlines,
                                  SecondTryOf(f, *image, predefined), d_out, capacity, outsize);
  }
  const zamd::PngFrame frame = FrameIn(image->width, image->height, f.plan.mode);
  return zamd::CompressDeviceToDevice(w.c_str(), options, ZOPFLI_FORMAT_ZLIB, f.scan.p, f.scanlines, d_out, capacity, outsize, &frame);
}

// Both batches: image by image one k_png_index_use, the host step and one k_png_index_convert on one hold of a context,
// ONE zmx_compress_device_batch over all scanlines, and for `optimize` one more hold and one more batch for the second tries.
int IndexBatch(const std::string& w, const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy, unsigned lossy,
               bool optimize, unsigned char** out, size_t* outsize) {
  if (n == 0) return 0;
  if (!options || !images || !out || !outsize) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  if (strategy == ZMX_PNG_FILTER_PREDEFINED) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED is the single call's");
  if (!StrategyOk(strategy, false)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  std::vector<const void*> pixels(n);
  std::vector<size_t> nbytes(n);
  for (size_t i = 0; i < n; ++i) {
    if (CheckIndexImage(w + ": image " + std::to_string(i), images[i], &nbytes[i]) != 0) return -1;
    pixels[i] = images[i].d_pixels;
  }
  int device = -1;
  if (zmx_internal_device_pointers_one_device(w.c_str(), n, pixels.data(), nbytes.data(), &device) != 0) return -1;
  // (CompressInto's view of the images: their width and height)
  std::vector<zmx_png_image> dims(n);
  for (size_t i = 0; i < n; ++i) dims[i] = zmx_png_image{nullptr, images[i].width, images[i].height, 0, 0};
  std::vector<IndexPlan> plan(n);
  std::vector<int> chosen(n, strategy);   // (_AUTO: the strategy of each image's own trials)
  std::vector<size_t> all(n), start(n + 1, 0);
  std::vector<zmx_png_color_mode> modes(n);
  const std::vector<char> converted(n, 0);   // (no file is "the image as it is")
  DeviceBuffer scan, room;
  scan.device = room.device = device;
  int rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
    size_t most = 0;
    for (size_t i = 0; i < n; ++i) {
      const std::string wi = w + ": image " + std::to_string(i);
      if (zmx_png_index_use_device(ctx, &images[i], plan[i].first) != 0) return -1;
      if (PlanIndex(wi, images[i], lossy, optimize, &plan[i]) != 0) return -1;
      if (strategy == ZMX_PNG_FILTER_AUTO && ChooseStrategy(ctx, w, device, RowsOf(images[i], plan[i].seen), plan[i].mode,
                                                            optimize ? &plan[i].stats : nullptr, nullptr, &chosen[i], nullptr) != 0) {
        return -1;
      }
      const size_t scanlines = ScanlinesIn(images[i].width, images[i].height, plan[i].mode);
      if (scanlines > SIZE_MAX - start[i]) return Refuse(w + ": the sizes overflow");
      start[i + 1] = start[i] + scanlines;
      most = std::max(most, scanlines);
    }
    if (zmx_internal_device_alloc(device, start[n], &scan.p) != 0) return -1;
    if (zmx_internal_device_alloc(device, most, &room.p) != 0) return -1;
    for (size_t i = 0; i < n; ++i) {
      if (ScanlinesOf(ctx, RowsOf(images[i], plan[i].seen), plan[i].mode, chosen[i], nullptr, room.p,
                      static_cast<unsigned char*>(scan.p) + start[i]) != 0) {
        return -1;
      }
    }
    return 0;
  }, device);
  if (rc != 0) return -1;
  for (size_t i = 0; i < n; ++i) {
    all[i] = i;
    modes[i] = plan[i].mode;
  }
  std::vector<File> files(n);
  if (CompressInto(options, w, dims.data(), all, modes, converted, static_cast<const unsigned char*>(scan.p), start, &files) != 0) return -1;
  // zopflipng's second try at the small palette files, all of them in one more batch
  std::vector<size_t> again;
  for (size_t i = 0; optimize && i < n; ++i) {
    if (plan[i].mode.colortype == 3 && files[i].size < zamd::kPngRetryBelow) again.push_back(i);
  }
  std::vector<File> seconds(again.size());
  if (!again.empty()) {
    const size_t m = again.size();
    std::vector<zmx_png_color_mode> modes2(m);
    std::vector<size_t> start2(m + 1, 0);
    size_t most = 0;
    for (size_t k = 0; k < m; ++k) {
      const zmx_png_index_image& im = images[again[k]];
      zamd::PngRetryMode(plan[again[k]].stats, static_cast<uint64_t>(im.width) * im.height, &modes2[k]);
      start2[k + 1] = start2[k] + ScanlinesIn(im.width, im.height, modes2[k]);
      most = std::max(most, start2[k + 1] - start2[k]);
    }
    DeviceBuffer scan2, room2;
    scan2.device = room2.device = device;
    if (zmx_internal_device_alloc(device, start2[m], &scan2.p) != 0) return -1;
    if (zmx_internal_device_alloc(device, most, &room2.p) != 0) return -1;
    rc = zamd::OnPooledContext([&](zmx_ctx* ctx) {
      for (size_t k = 0; k < m; ++k) {
        if (ScanlinesOf(ctx, RowsOf(images[again[k]], plan[again[k]].seen), modes2[k], chosen[again[k]], nullptr, room2.p,
                        static_cast<unsigned char*>(scan2.p) + start2[k]) != 0) {
          return -1;
        }
      }
      return 0;
    }, device);
    if (rc != 0) return -1;
    const std::vector<char> converted2(m, 0);
    if (CompressInto(options, w, dims.data(), again, modes2, converted2, static_cast<const unsigned char*>(scan2.p), start2, &seconds) != 0) return -1;
  }
  // every file made before any out[i] is touched
  std::vector<File*> kept(n);
  for (size_t i = 0; i < n; ++i) kept[i] = &files[i];
  for (size_t k = 0; k < again.size(); ++k) kept[again[k]] = &Smaller(files[again[k]], seconds[k]);
  for (size_t i = 0; i < n; ++i) kept[i]->GiveTo(&out[i], &outsize[i]);
  return 0;
}

}  // namespace

extern "C" int zmx_png_index_color_stats(const zmx_png_index_image* image, const uint64_t first[256], unsigned lossy, zmx_png_color_stats* out) {
  const std::string w = "zmx_png_index_color_stats";
  if (!image || !first || !out) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  size_t nbytes = 0;
  if (CheckIndexImage(w, *image, &nbytes) != 0) return -1;
  IndexPlan plan;
  std::copy(first, first + 256, plan.first);
  if (PlanIndex(w, *image, lossy, true, &plan) != 0) return -1;
  *out = plan.stats;
  return 0;
}

extern "C" int zmx_png_index_table(const zmx_png_index_image* image, const uint64_t first[256], unsigned lossy, const zmx_png_color_mode* mode,
                                   uint32_t table[256]) {
  const std::string w = "zmx_png_index_table";
  if (!image || !first || !mode || !table) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  size_t nbytes = 0;
  if (CheckIndexImage(w, *image, &nbytes) != 0) return -1;
  if (!zamd::PngIndexOutModeOk(mode->colortype, mode->bitdepth) || (mode->colortype == 3 && (mode->palettesize == 0 || mode->palettesize > 256))) {
    return Refuse(w + ": colour type " + std::to_string(mode->colortype) + " at " + std::to_string(mode->bitdepth) +
                  " bits is no mode an index image converts to");
  }
  IndexPlan plan;
  std::copy(first, first + 256, plan.first);
  if (PlanIndex(w, *image, lossy, true, &plan) != 0) return -1;
  zamd::PngIndexTable(plan.seen, *mode, table);
  return 0;
}

extern "C" int zmx_png_index_keep_plan(const zmx_png_index_image* image, const uint64_t first[256], unsigned lossy, zmx_png_color_mode* mode,
                                       uint32_t table[256]) {
  const std::string w = "zmx_png_index_keep_plan";
  if (!image || !first || !mode || !table) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  size_t nbytes = 0;
  if (CheckIndexImage(w, *image, &nbytes) != 0) return -1;
  if (CheckInsidePalette(w, *image, first) != 0) return -1;
  zamd::PngIndexKeepPlan(*image, first, (lossy & ZMX_PNG_LOSSY_TRANSPARENT) != 0, mode, table);
  return 0;
}

extern "C" int zmx_png_index_choose_strategy_device(zmx_ctx* ctx, const zmx_png_index_image* image, int reduce_color, unsigned lossy,
                                                    const unsigned char* predefined, int* strategy, uint64_t file_bytes[8]) {
  const std::string w = "zmx_png_index_choose_strategy_device";
  if (!ctx || !image || !strategy || !file_bytes) return Refuse(w + ": null argument");
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  size_t nbytes = 0;
  if (CheckIndexImage(w, *image, &nbytes) != 0) return -1;
  if (CheckPredefined(w, ZMX_PNG_FILTER_AUTO, predefined, image->height) != 0) return -1;
  int device = -1;
  if (zmx_internal_device_pointer(w.c_str(), image->d_pixels, nbytes, &device) != 0) return -1;
  IndexPlan plan;
  if (zmx_png_index_use_device(ctx, image, plan.first) != 0) return -1;
  if (PlanIndex(w, *image, lossy, reduce_color != 0, &plan) != 0) return -1;
  int chosen = 0;
  uint64_t bytes[8];
  if (ChooseStrategy(ctx, w, device, RowsOf(*image, plan.seen), plan.mode, reduce_color ? &plan.stats : nullptr, predefined, &chosen, bytes) != 0) {
    return -1;
  }
  *strategy = chosen;
  for (int k = 0; k < 8; ++k) file_bytes[k] = bytes[k];
  return 0;
}

extern "C" size_t zmx_png_index_bound(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth) {
  if (width == 0 || height == 0 || !zamd::PngIndexFormatOk(colortype, bitdepth)) return 0;
  if (static_cast<uint64_t>(width) * height > 0xffffffffull) return 0;
  return zamd::PngIndexBound(width, height);
}

extern "C" int zmx_png_index_encode_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                           const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return IndexOne("zmx_png_index_encode_device", options, image, strategy, predefined, lossy, false, out, outsize);
}
extern "C" int zmx_png_index_optimize_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                             const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return IndexOne("zmx_png_index_optimize_device", options, image, strategy, predefined, lossy, true, out, outsize);
}
extern "C" int zmx_png_index_encode_device_to_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                                     const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                     size_t* outsize) {
  return IndexOneToDevice("zmx_png_index_encode_device_to_device", options, image, strategy, predefined, lossy, false, d_out, capacity, outsize);
}
extern "C" int zmx_png_index_optimize_device_to_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                                       const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                       size_t* outsize) {
  return IndexOneToDevice("zmx_png_index_optimize_device_to_device", options, image, strategy, predefined, lossy, true, d_out, capacity, outsize);
}
extern "C" int zmx_png_index_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy,
                                                 unsigned lossy, unsigned char** out, size_t* outsize) {
  return IndexBatch("zmx_png_index_encode_device_batch", options, n, images, strategy, lossy, false, out, outsize);
}
extern "C" int zmx_png_index_optimize_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy,
                                                   unsigned lossy, unsigned char** out, size_t* outsize) {
  return IndexBatch("zmx_png_index_optimize_device_batch", options, n, images, strategy, lossy, true, out, outsize);
}

// ---- strided, planar, float and 16-bit sources (png_source.h; device/zmx_png_pack.h)
namespace {

// The packed images of n sources in ONE buffer of the call's own, slices rounded up to 16 bytes, made by one k_png_pack
// launch on one hold of a context: images[i] is source i as the other entries take it.
struct Packed {
  DeviceBuffer buf;
  std::vector<zmx_png_image> images;
};

// Every source checked — with `dest`, the to-device entry's destination, held against the sources' extents — before
// anything runs; then the buffer and the launch.
int PackSources(const std::string& w, size_t n, const zmx_png_source* sources, const DeviceDest* dest, Packed* p) {
  std::vector<size_t> start(n + 1, 0), sizes(n), extent_bytes(n);
  std::vector<const void*> extent(n);
  p->images.resize(n);
  for (size_t i = 0; i < n; ++i) {
    zamd::PngSourcePlan plan;
    const std::string msg = zamd::CheckPngSource((w + ": source " + std::to_string(i)).c_str(), &sources[i], &plan);
    if (!msg.empty()) return Refuse(msg);
    p->images[i] = plan.image;
    sizes[i] = plan.nbytes;
    const size_t slice = (plan.nbytes + 15) & ~static_cast<size_t>(15);
    if (slice > SIZE_MAX - start[i]) return Refuse(w + ": the sizes overflow");
    start[i + 1] = start[i] + slice;
    extent[i] = reinterpret_cast<const void*>(plan.lo);
    extent_bytes[i] = plan.hi - plan.lo;
  }
  // (the device of the first extent; the pack holds every extent against its context's device)
  if (zmx_internal_device_pointer((w + ": source 0: the extent").c_str(), extent[0], extent_bytes[0], &p->buf.device) != 0) return -1;
  if (dest && CheckDest(w, *dest, p->buf.device, n, extent.data(), extent_bytes.data()) != 0) return -1;
  if (zmx_internal_device_alloc(p->buf.device, start[n], &p->buf.p) != 0) return -1;
  std::vector<void*> outs(n);
  for (size_t i = 0; i < n; ++i) {
    outs[i] = static_cast<unsigned char*>(p->buf.p) + start[i];
    p->images[i].d_pixels = outs[i];
  }
  return zamd::OnPooledContext([&](zmx_ctx* ctx) { return zmx_internal_png_pack(ctx, w.c_str(), n, sources, outs.data(), sizes.data()); },
                               p->buf.device);
}

// What the entries behind the pack refuse of their other arguments, held in front of it: nothing runs for a call that is
// refused anyway.
int CheckBehindPack(const std::string& w, int strategy, unsigned lossy, bool single, const unsigned char* predefined, const zmx_png_source* source) {
  if (!LossyOk(lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(lossy));
  if (!single && strategy == ZMX_PNG_FILTER_PREDEFINED) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED is the single call's");
  if (!StrategyOk(strategy, single)) return Refuse(w + ": unknown strategy " + std::to_string(strategy));
  if (single && source && CheckPredefined(w, strategy, predefined, source->height) != 0) return -1;
  return 0;
}

}  // namespace

extern "C" int zmx_png_source_image(const zmx_png_source* src, zmx_png_image* image, size_t* nbytes) {
  zamd::PngSourcePlan plan;
  const std::string msg = zamd::CheckPngSource("zmx_png_source_image", src, &plan);
  if (!msg.empty()) return Refuse(msg);
  if (image) *image = plan.image;
  if (nbytes) *nbytes = plan.nbytes;
  return 0;
}

extern "C" size_t zmx_png_source_bound(const zmx_png_source* source) {
  zamd::PngSourcePlan plan;
  if (!zamd::CheckPngSource("zmx_png_source_bound", source, &plan).empty()) return 0;
  return zmx_png_bound(plan.image.width, plan.image.height, plan.image.colortype, plan.image.bitdepth);
}
extern "C" size_t zmx_png_source_batch_bound(size_t n, const zmx_png_source* sources, size_t align) {
  if (n == 0 || !sources) return 0;
  std::vector<zmx_png_image> images(n);
  for (size_t i = 0; i < n; ++i) {
    zamd::PngSourcePlan plan;
    if (!zamd::CheckPngSource("zmx_png_source_batch_bound", &sources[i], &plan).empty()) return 0;
    images[i] = plan.image;
  }
  return zmx_png_batch_bound(n, images.data(), align);
}

extern "C" int zmx_png_encode_source_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                            const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  const std::string w = "zmx_png_encode_source_device";
  if (!options || !source || !out || !outsize) return Refuse(w + ": null argument");
  if (CheckBehindPack(w, strategy, lossy, true, predefined, source) != 0) return -1;
  Packed p;
  if (PackSources(w, 1, source, nullptr, &p) != 0) return -1;
  return EncodeOne(w, options, &p.images[0], strategy, predefined, lossy, out, outsize);
}
extern "C" int zmx_png_optimize_source_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                              const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  const std::string w = "zmx_png_optimize_source_device";
  if (!options || !source || !out || !outsize) return Refuse(w + ": null argument");
  if (CheckBehindPack(w, strategy, lossy, true, predefined, source) != 0) return -1;
  Packed p;
  if (PackSources(w, 1, source, nullptr, &p) != 0) return -1;
  return OptimizeOne(w, options, &p.images[0], strategy, predefined, lossy, out, outsize);
}
extern "C" int zmx_png_encode_source_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                                  unsigned lossy, unsigned char** out, size_t* outsize) {
  const std::string w = "zmx_png_encode_source_device_batch";
  if (n == 0) return 0;
  if (!options || !sources || !out || !outsize) return Refuse(w + ": null argument");
  if (CheckBehindPack(w, strategy, lossy, false, nullptr, nullptr) != 0) return -1;
  Packed p;
  if (PackSources(w, n, sources, nullptr, &p) != 0) return -1;
  return EncodeBatch(w, options, n, p.images.data(), strategy, lossy, out, outsize);
}
extern "C" int zmx_png_optimize_source_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                                    unsigned lossy, unsigned char** out, size_t* outsize) {
  const std::string w = "zmx_png_optimize_source_device_batch";
  if (n == 0) return 0;
  if (!options || !sources || !out || !outsize) return Refuse(w + ": null argument");
  if (CheckBehindPack(w, strategy, lossy, false, nullptr, nullptr) != 0) return -1;
  Packed p;
  if (PackSources(w, n, sources, nullptr, &p) != 0) return -1;
  return OptimizeBatch(w, options, n, p.images.data(), strategy, lossy, out, outsize);
}
extern "C" int zmx_png_encode_source_device_to_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                                      const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                      size_t* outsize) {
  const std::string w = "zmx_png_encode_source_device_to_device";
  if (!options || !source || !outsize) return Refuse(w + ": null argument");
  *outsize = 0;
  if (CheckBehindPack(w, strategy, lossy, true, predefined, source) != 0) return -1;
  const DeviceDest dest{d_out, capacity};
  Packed p;
  if (PackSources(w, 1, source, &dest, &p) != 0) return -1;
  return EncodeOneToDevice(w, options, &p.images[0], strategy, predefined, lossy, d_out, capacity, outsize);
}
extern "C" int zmx_png_optimize_source_device_to_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                                        const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                        size_t* outsize) {
  const std::string w = "zmx_png_optimize_source_device_to_device";
  if (!options || !source || !outsize) return Refuse(w + ": null argument");
  *outsize = 0;
  if (CheckBehindPack(w, strategy, lossy, true, predefined, source) != 0) return -1;
  const DeviceDest dest{d_out, capacity};
  Packed p;
  if (PackSources(w, 1, source, &dest, &p) != 0) return -1;
  return OptimizeOneToDevice(w, options, &p.images[0], strategy, predefined, lossy, d_out, capacity, outsize);
}
extern "C" int zmx_png_encode_source_device_batch_packed(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                                         unsigned lossy, void* d_arena, size_t capacity, size_t align, size_t* outoffset,
                                                         size_t* outsize) {
  const std::string w = "zmx_png_encode_source_device_batch_packed";
  if (n == 0) return 0;
  if (!options || !sources || !outoffset || !outsize) return Refuse(w + ": null argument");
  if (!zamd::PackedAlignOk(align)) return Refuse(w + ": align " + std::to_string(align) + " is not a power of two from 1 to 4096");
  if (CheckBehindPack(w, strategy, lossy, false, nullptr, nullptr) != 0) return -1;
  const DeviceDest dest{d_arena, capacity};
  Packed p;
  if (PackSources(w, n, sources, &dest, &p) != 0) return -1;
  return EncodeBatchPacked(w, options, n, p.images.data(), strategy, lossy, d_arena, capacity, align, outoffset, outsize);
}
