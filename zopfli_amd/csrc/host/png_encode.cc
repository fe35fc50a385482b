// The zmx_png_* entries that make a PNG file of an image in device memory (include/zopfli_amd.h says which file): encode
// and optimize, plain and _lossy, index, _to_device, _batch, _batch_packed and _source_*.  They are ONE pipeline:
//
//   Kind      what the images are made of — ColourKind: zmx_png_images, as they are (encode) or with the colour mode
//             reduced (optimize), the _lossy rewrite in front; IndexKind: zmx_png_index_images, palette or low-bit grey.
//             A kind checks image i on the host, and on a held context prepares it and makes its filtered scanlines.
//   Subject   one prepared image: its rows in any colour mode (RowSource), the first file's mode, the statistics where a
//             second try competes (null: the encode entries and index-encode), the strategy its rows are made with.
//   MakeFront the checks of a call of n images, the buffers, and one hold of a pooled context on which every image is
//             prepared, given its strategy (_AUTO: zopflipng's choice, image by image) and filtered into one scan buffer.
//             A single call is a front of one image, with _PREDEFINED allowed and no ": image i" in its messages.
//   Finish*   the files around the streams.  FinishBatch: one zmx_compress_device_batch over the first files, zopflipng's
//             second try at the palette files below 4096 bytes on one more hold and in one more batch, the smaller kept,
//             and no out[i] touched before every file is made.  FinishOne / FinishOneToDevice: the same for one file,
//             through zmx_compress_device or into device memory.  BatchPacked: the first files in one arena.
//
// The scanlines go to a buffer of the call's own that outlives the context's hold: the context is back in the pool BEFORE
// any zmx_compress_device* / CompressDeviceToDevice* call runs — those take contexts themselves, so a hold around them can
// deadlock the pool.  The stream's second byte and the chunks around it are png_container.h's; the to-device paths put
// the file's frame around the stream (device_output_plan.h: PngFrame) and seal the IDAT's CRC-32 on the device.
// ZMX_PNG_FILTER_AUTO is zopflipng's own choice of the strategy (ChooseStrategy; zmx_png_choose_strategy_device).
// The zmx_png_*_source_* entries, last, take strided, planar, float and 16-bit sources (png_source.h): every source
// checked, one buffer for all packed images, one hold of a context for one k_png_pack launch, then the pipeline on
// zmx_png_images that point into the buffer.
// (Outside api.cc, as png.cc is: the host-only test library links api.cc against a stand-in for the device layer.)
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <memory>
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

size_t RoundUp16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

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

int CheckReducible(const std::string& w, const zmx_png_image& im, Geometry* g) {
  if (CheckImage(w, im, g) != 0) return -1;
  if (static_cast<uint64_t>(im.width) * im.height > 0xffffffffull) return Refuse(w + ": an image of 2^32 pixels or more");
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

// A file in the making: a malloc'ed array under the reference's convention that begins with the file's bytes up to the
// IDAT's type, for ZopfliCompress to append the stream to.
struct File {
  unsigned char* bytes = nullptr;
  size_t size = 0;
  File() = default;
  File(const File&) = delete;
  File& operator=(const File&) = delete;
  ~File() { std::free(bytes); }
  size_t prefix_bytes = zamd::kPngPrefixBytes;
  // the file of a width x height image in `mode`: PLTE and tRNS where the mode has them
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

// Of two closed files of one image the one zopflipng keeps: the second only when it is strictly smaller.
File& Smaller(File& first, File& second) { return second.size < first.size ? second : first; }

// What a _lossy entry makes of an image before anything else (zopflipng_lib.cc:415-428): its 8-bit image where the
// optimize entry has _8BIT and the image is 16 bits deep, the rewrite of the transparent pixels where it has _TRANSPARENT
// and the image is 8-bit by then and has an alpha channel.  bytes: the buffer either takes, 0 where nothing is made.
// (of an image that CheckImage has passed)
struct LossyPlan {
  bool to8 = false, transparent = false;
  size_t bytes = 0;
};

LossyPlan PlanLossy(const zmx_png_image& im, unsigned lossy, bool optimize) {
  LossyPlan p;
  p.to8 = optimize && (lossy & ZMX_PNG_LOSSY_8BIT) != 0 && im.bitdepth == 16;
  p.transparent = (lossy & ZMX_PNG_LOSSY_TRANSPARENT) != 0 && (im.bitdepth == 8 || p.to8) && (im.colortype == 4 || im.colortype == 6);
  if (p.to8 || p.transparent) p.bytes = zamd::PngLineBytes(im.width, im.colortype, im.bitdepth) / (p.to8 ? 2 : 1) * im.height;
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

// room that does for the file around `scanlines` filtered bytes, whatever its prefix
size_t FileBound(size_t scanlines) {
  return zamd::kPngMaxPrefixBytes + zamd::CompressBound(ZOPFLI_FORMAT_ZLIB, scanlines) + zamd::kPngTrailerBytes;
}

// ---- colour modes, and an image as rows in one
bool SameMode(const zmx_png_image& im, const zmx_png_color_mode& mode) {
  return mode.colortype == im.colortype && mode.bitdepth == im.bitdepth && mode.key_defined == 0;
}

size_t BitsPerPixel(const zmx_png_color_mode& mode) { return (mode.colortype == 3 ? 1 : zamd::PngChannels(mode.colortype)) * mode.bitdepth; }
size_t RowBytesIn(uint32_t width, const zmx_png_color_mode& mode) { return (static_cast<size_t>(width) * BitsPerPixel(mode) + 7) / 8; }
size_t ByteWidthIn(const zmx_png_color_mode& mode) { return BitsPerPixel(mode) < 8 ? 1 : BitsPerPixel(mode) / 8; }
size_t ScanlinesIn(uint32_t width, uint32_t height, const zmx_png_color_mode& mode) {
  return static_cast<size_t>(height) * (RowBytesIn(width, mode) + 1);
}

// the mode an image lies in: the first (and only) file's of the encode entries
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

// on a held context: the statistics of an image and LodePNG's choice of its mode
int StatsAndMode(zmx_ctx* ctx, const zmx_png_image& im, zmx_png_color_stats* stats, zmx_png_color_mode* mode) {
  if (zmx_png_color_stats_device(ctx, &im, stats) != 0) return -1;
  zamd::PngChooseColor(*stats, static_cast<uint64_t>(im.width) * im.height, mode);
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
  const size_t room = RoundUp16(rowbytes * src.height);
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
  zmx_png_color_stats stats;
  zmx_png_color_mode mode = OwnMode(*image);
  if (reduce_color && StatsAndMode(ctx, *image, &stats, &mode) != 0) return -1;
  int chosen = 0;
  uint64_t bytes[8];
  if (ChooseStrategy(ctx, w, device, RowsOf(*image), mode, reduce_color ? &stats : nullptr, predefined, &chosen, bytes) != 0) return -1;
  *strategy = chosen;
  for (int k = 0; k < 8; ++k) file_bytes[k] = bytes[k];
  return 0;
}

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
extern "C" int zmx_png_choose_color(const zmx_png_color_stats* stats, uint64_t numpixels, zmx_png_color_mode* out) {
  if (!stats || !out) return Refuse("zmx_png_choose_color: null argument");
  zamd::PngChooseColor(*stats, numpixels, out);
  return 0;
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

// ---- the pipeline: Subject, Kind, MakeFront, the finishes

// One prepared image.  It is made in place and stays there: `rows` and `stats` point into it.
struct Subject {
  uint32_t width = 0, height = 0;
  RowSource rows;
  zmx_png_color_mode mode;                       // the first file's
  const zmx_png_color_stats* stats = nullptr;    // what a second try is made from; null: none competes
  int strategy = 0;                              // the one the rows are made with (_AUTO: the chosen one)
  // what the kind keeps alive
  zmx_png_image work;                            // ColourKind: what is encoded — the caller's image, or its 8-bit or rewritten image
  zmx_png_color_stats work_stats;                // ... and its statistics, where the mode is reduced
  std::unique_ptr<IndexPlan> plan;               // IndexKind
  Subject() = default;
  Subject(const Subject&) = delete;
  Subject& operator=(const Subject&) = delete;
};

// whether zopflipng tries the image a second time, as RGB or RGBA, once its first file has `file_bytes`
bool SecondTryDue(const Subject& s, size_t file_bytes) { return s.stats && s.mode.colortype == 3 && file_bytes < zamd::kPngRetryBelow; }

// What an entry was asked for, beyond its images.
struct Call {
  std::string w;                      // the entry's name
  const ZopfliOptions* options;
  int strategy;
  const unsigned char* predefined;    // the single call's; null in a batch
  unsigned lossy;
};

// What a kind's host checks give of image i
struct Checked {
  const void* pixels;
  size_t nbytes;       // the pixels'
  size_t rewritten;    // of a buffer of the call's own that Prepare fills; 0: none
  uint32_t height;
};

// What the images of a call are made of.  `w` is the entry's name, `wi` the same with ": image i" in a batch.
struct Kind {
  const void* const given;   // the caller's array of images (null: refused)
  explicit Kind(const void* images) : given(images) {}
  virtual ~Kind() = default;
  // the host checks of image i, before its pointer is looked at
  virtual int Check(const std::string& wi, unsigned lossy, size_t i, Checked* c) const = 0;
  // on a held context: image i as a Subject, all but its strategy
  virtual int Prepare(zmx_ctx* ctx, const std::string& w, const std::string& wi, unsigned lossy, size_t i, void* d_rewritten, Subject* s) const = 0;
  // whether Scanlines wants d_room: RowBytesIn * height bytes for the image in `mode`
  virtual bool NeedsRoom() const = 0;
  // on a held context: the filtered scanlines of `s` in `mode` under s.strategy into d_scan, ScanlinesIn bytes
  virtual int Scanlines(zmx_ctx* ctx, const Subject& s, const zmx_png_color_mode& mode, const unsigned char* predefined, void* d_room,
                        void* d_scan) const = 0;
};

// zmx_png_images: as they are (the encode entries), or with the colour mode reduced (`reduce`: the optimize entries); the
// _lossy rewrite in front of either.  A conversion goes to the context's pool: no room of the call's own.
struct ColourKind : Kind {
  const zmx_png_image* const images;
  const bool reduce;
  ColourKind(const zmx_png_image* images_, bool reduce_) : Kind(images_), images(images_), reduce(reduce_) {}
  int Check(const std::string& wi, unsigned lossy, size_t i, Checked* c) const override {
    const zmx_png_image& im = images[i];
    Geometry g;
    if ((reduce ? CheckReducible(wi, im, &g) : CheckImage(wi, im, &g)) != 0) return -1;
    const LossyPlan plan = PlanLossy(im, lossy, reduce);
    if (CheckRewritable(wi, im, plan) != 0) return -1;
    *c = Checked{im.d_pixels, g.linebytes * g.height, plan.bytes, im.height};
    return 0;
  }
  int Prepare(zmx_ctx* ctx, const std::string& w, const std::string&, unsigned lossy, size_t i, void* d_rewritten, Subject* s) const override {
    const LossyPlan plan = PlanLossy(images[i], lossy, reduce);
    s->work = images[i];
    if (plan.bytes != 0 && zmx_internal_png_lossy_image(ctx, w.c_str(), &images[i], plan.to8, plan.transparent, d_rewritten, &s->work) != 0) return -1;
    s->width = s->work.width;
    s->height = s->work.height;
    s->rows = RowsOf(s->work);
    s->mode = OwnMode(s->work);
    if (!reduce) return 0;
    s->stats = &s->work_stats;
    return StatsAndMode(ctx, s->work, &s->work_stats, &s->mode);
  }
  bool NeedsRoom() const override { return false; }
  int Scanlines(zmx_ctx* ctx, const Subject& s, const zmx_png_color_mode& mode, const unsigned char* predefined, void*, void* d_scan) const override {
    if (SameMode(s.work, mode)) {
      return zmx_internal_png_scanlines(ctx, s.work.d_pixels, RowBytesIn(s.width, mode), s.height, ByteWidthIn(mode), s.strategy, kBruteWindow,
                                        predefined, d_scan);
    }
    return zmx_internal_png_reduced_scanlines(ctx, &s.work, &mode, s.strategy, kBruteWindow, predefined, d_scan);
  }
};

// zmx_png_index_images: one k_png_index_use and the host's plan in place of the statistics — the input's own mode (the
// index-encode entries) or LodePNG's choice (`optimize`) —, k_png_index_convert into a room of the call's own.
struct IndexKind : Kind {
  const zmx_png_index_image* const images;
  const bool optimize;
  IndexKind(const zmx_png_index_image* images_, bool optimize_) : Kind(images_), images(images_), optimize(optimize_) {}
  int Check(const std::string& wi, unsigned, size_t i, Checked* c) const override {
    size_t nbytes = 0;
    if (CheckIndexImage(wi, images[i], &nbytes) != 0) return -1;
    *c = Checked{images[i].d_pixels, nbytes, 0, images[i].height};
    return 0;
  }
  int Prepare(zmx_ctx* ctx, const std::string&, const std::string& wi, unsigned lossy, size_t i, void*, Subject* s) const override {
    const zmx_png_index_image& im = images[i];
    s->plan.reset(new IndexPlan);
    if (zmx_png_index_use_device(ctx, &im, s->plan->first) != 0) return -1;
    if (PlanIndex(wi, im, lossy, optimize, s->plan.get()) != 0) return -1;
    s->width = im.width;
    s->height = im.height;
    s->rows = RowsOf(im, s->plan->seen);
    s->mode = s->plan->mode;
    s->stats = optimize ? &s->plan->stats : nullptr;
    return 0;
  }
  bool NeedsRoom() const override { return true; }
  int Scanlines(zmx_ctx* ctx, const Subject& s, const zmx_png_color_mode& mode, const unsigned char* predefined, void* d_room,
                void* d_scan) const override {
    return ScanlinesOf(ctx, s.rows, mode, s.strategy, predefined, d_room, d_scan);
  }
};

// What the front of a call leaves: every image prepared, image i's filtered scanlines in its first file's mode at
// scan + start[i] (start[n]: their end).
struct Front {
  int device = -1;
  std::vector<Subject> subjects;
  std::vector<size_t> start;
  DeviceBuffer scan, rewritten;
  const void* Scan(size_t i) const { return static_cast<const unsigned char*>(scan.p) + start[i]; }
  size_t ScanBytes(size_t i) const { return start[i + 1] - start[i]; }
};

// The front of a call of n > 0 images, single or batch: the checks (`dest`: a to-device entry's destination, checked with
// them), the buffers, and the first hold of a context — prepare, the _AUTO choice and the layout image by image, then the
// rows of all.
int MakeFront(const Call& c, const Kind& kind, size_t n, bool single, const DeviceDest* dest, Front* f) {
  const std::string& w = c.w;
  const auto name = [&](size_t i) { return single ? w : w + ": image " + std::to_string(i); };
  if (!LossyOk(c.lossy)) return Refuse(w + ": unknown lossy flags " + std::to_string(c.lossy));
  if (!single) {
    if (c.strategy == ZMX_PNG_FILTER_PREDEFINED) return Refuse(w + ": ZMX_PNG_FILTER_PREDEFINED is the single call's");
    if (!StrategyOk(c.strategy, false)) return Refuse(w + ": unknown strategy " + std::to_string(c.strategy));
  }
  std::vector<const void*> pixels(n);
  std::vector<size_t> nbytes(n);
  std::vector<size_t> rstart(n + 1, 0);   // where image i's 8-bit or rewritten pixels begin in their buffer
  uint32_t height = 0;
  for (size_t i = 0; i < n; ++i) {
    Checked checked;
    if (kind.Check(name(i), c.lossy, i, &checked) != 0) return -1;
    pixels[i] = checked.pixels;
    nbytes[i] = checked.nbytes;
    rstart[i + 1] = rstart[i] + RoundUp16(checked.rewritten);
    height = checked.height;
  }
  if (single) {
    if (!StrategyOk(c.strategy, true)) return Refuse(w + ": unknown strategy " + std::to_string(c.strategy));
    if (CheckPredefined(w, c.strategy, c.predefined, height) != 0) return -1;
    if (zmx_internal_device_pointer(w.c_str(), pixels[0], nbytes[0], &f->device) != 0) return -1;
  } else if (zmx_internal_device_pointers_one_device(w.c_str(), n, pixels.data(), nbytes.data(), &f->device) != 0) {
    return -1;
  }
  const int device = f->device;
  if (dest && CheckDest(w, *dest, device, n, pixels.data(), nbytes.data()) != 0) return -1;
  DeviceBuffer room;
  f->scan.device = f->rewritten.device = room.device = device;
  if (rstart[n] != 0 && zmx_internal_device_alloc(device, rstart[n], &f->rewritten.p) != 0) return -1;
  f->subjects = std::vector<Subject>(n);
  f->start.assign(n + 1, 0);
  // (one hold of a context for all images, for the device work only; a launch set per image: tools/png_device.py measures
  // what that costs)
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    size_t room_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
      Subject& s = f->subjects[i];
      if (kind.Prepare(ctx, w, name(i), c.lossy, i, static_cast<unsigned char*>(f->rewritten.p) + rstart[i], &s) != 0) return -1;
      s.strategy = c.strategy;
      if (c.strategy == ZMX_PNG_FILTER_AUTO && ChooseStrategy(ctx, w, device, s.rows, s.mode, s.stats, c.predefined, &s.strategy, nullptr) != 0) {
        return -1;
      }
      const size_t scanlines = ScanlinesIn(s.width, s.height, s.mode);
      if (scanlines > SIZE_MAX - f->start[i]) return Refuse(w + ": the sizes overflow");
      f->start[i + 1] = f->start[i] + scanlines;
      room_bytes = std::max(room_bytes, RowBytesIn(s.width, s.mode) * s.height);
    }
    if (zmx_internal_device_alloc(device, f->start[n], &f->scan.p) != 0) return -1;
    if (kind.NeedsRoom() && zmx_internal_device_alloc(device, room_bytes, &room.p) != 0) return -1;
    for (size_t i = 0; i < n; ++i) {
      const Subject& s = f->subjects[i];
      if (kind.Scanlines(ctx, s, s.mode, c.predefined, room.p, static_cast<unsigned char*>(f->scan.p) + f->start[i]) != 0) return -1;
    }
    return 0;
  }, device);
}

// zopflipng's second try at the small palette files of the subjects `again`: their modes, and on one more hold of a context
// their scanlines side by side, `again[k]`'s at scan + start[k].
struct SecondTries {
  std::vector<zmx_png_color_mode> modes;
  std::vector<size_t> start;
  DeviceBuffer scan;
};

int MakeSecondTries(const Kind& kind, int device, const std::vector<const Subject*>& again, const unsigned char* predefined, SecondTries* t) {
  const size_t m = again.size();
  t->modes.resize(m);
  t->start.assign(m + 1, 0);
  size_t room_bytes = 0;
  for (size_t k = 0; k < m; ++k) {
    const Subject& s = *again[k];
    zamd::PngRetryMode(*s.stats, static_cast<uint64_t>(s.width) * s.height, &t->modes[k]);
    t->start[k + 1] = t->start[k] + ScanlinesIn(s.width, s.height, t->modes[k]);
    room_bytes = std::max(room_bytes, RowBytesIn(s.width, t->modes[k]) * s.height);
  }
  DeviceBuffer room;
  t->scan.device = room.device = device;
  if (zmx_internal_device_alloc(device, t->start[m], &t->scan.p) != 0) return -1;
  if (kind.NeedsRoom() && zmx_internal_device_alloc(device, room_bytes, &room.p) != 0) return -1;
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    for (size_t k = 0; k < m; ++k) {
      if (kind.Scanlines(ctx, *again[k], t->modes[k], predefined, room.p, static_cast<unsigned char*>(t->scan.p) + t->start[k]) != 0) return -1;
    }
    return 0;
  }, device);
}

// One zmx_compress_device_batch over the scanlines of the subjects `which` — which[k]'s at base + start[k], in *modes[k] —
// into files[k], closed.
int CompressInto(const Call& c, const std::vector<const Subject*>& which, const std::vector<const zmx_png_color_mode*>& modes,
                 const void* base, const std::vector<size_t>& start, std::vector<File>* files) {
  const size_t m = which.size();
  std::vector<const void*> slices(m);
  std::vector<size_t> sizes(m), filled(m);
  std::vector<unsigned char*> bytes(m);
  for (size_t k = 0; k < m; ++k) {
    slices[k] = static_cast<const unsigned char*>(base) + start[k];
    sizes[k] = start[k + 1] - start[k];
    (*files)[k].BeginIn(which[k]->width, which[k]->height, *modes[k]);
    bytes[k] = (*files)[k].bytes;
    filled[k] = (*files)[k].size;
  }
  // (a failed call changes none of them: the files still own their arrays)
  if (zmx_compress_device_batch(c.options, ZOPFLI_FORMAT_ZLIB, m, slices.data(), sizes.data(), bytes.data(), filled.data()) != 0) return -1;
  for (size_t k = 0; k < m; ++k) {
    (*files)[k].bytes = bytes[k];
    (*files)[k].size = filled[k];
  }
  for (size_t k = 0; k < m; ++k) {
    if (!(*files)[k].Close()) return BadStream(c.w);
  }
  return 0;
}

// The batch with host output, once the front is made: ONE zmx_compress_device_batch over the first files, one more hold and
// one more batch for all second tries together (none for a kind without statistics), the smaller of the two handed over.
int FinishBatch(const Call& c, const Kind& kind, const Front& f, unsigned char** out, size_t* outsize) {
  const size_t n = f.subjects.size();
  std::vector<const Subject*> all(n);
  std::vector<const zmx_png_color_mode*> modes(n);
  for (size_t i = 0; i < n; ++i) {
    all[i] = &f.subjects[i];
    modes[i] = &f.subjects[i].mode;
  }
  std::vector<File> files(n);
  if (CompressInto(c, all, modes, f.scan.p, f.start, &files) != 0) return -1;
  // zopflipng's second try at the small palette files, all of them in one more batch
  std::vector<size_t> again;
  for (size_t i = 0; i < n; ++i) {
    if (SecondTryDue(f.subjects[i], files[i].size)) again.push_back(i);
  }
  std::vector<File> seconds(again.size());
  if (!again.empty()) {
    std::vector<const Subject*> retried(again.size());
    std::vector<const zmx_png_color_mode*> modes2(again.size());
    for (size_t k = 0; k < again.size(); ++k) retried[k] = &f.subjects[again[k]];
    SecondTries t;
    if (MakeSecondTries(kind, f.device, retried, c.predefined, &t) != 0) return -1;
    for (size_t k = 0; k < again.size(); ++k) modes2[k] = &t.modes[k];
    if (CompressInto(c, retried, modes2, t.scan.p, t.start, &seconds) != 0) return -1;
  }
  // every file made before any out[i] is touched
  std::vector<File*> kept(n);
  for (size_t i = 0; i < n; ++i) kept[i] = &files[i];
  for (size_t k = 0; k < again.size(); ++k) kept[again[k]] = &Smaller(files[again[k]], seconds[k]);
  for (size_t i = 0; i < n; ++i) kept[i]->GiveTo(&out[i], &outsize[i]);
  return 0;
}

// One file with host output, once the front is made: the file in the subject's mode through zmx_compress_device, the second
// try where one is due, the smaller of the two handed over.
int FinishOne(const Call& c, const Kind& kind, const Front& f, unsigned char** out, size_t* outsize) {
  const Subject& s = f.subjects[0];
  File file;
  file.BeginIn(s.width, s.height, s.mode);
  if (zmx_compress_device(c.options, ZOPFLI_FORMAT_ZLIB, f.Scan(0), f.ScanBytes(0), &file.bytes, &file.size) != 0) return -1;
  if (!file.Close()) return BadStream(c.w);
  File second;
  if (SecondTryDue(s, file.size)) {
    SecondTries t;
    if (MakeSecondTries(kind, f.device, {&s}, c.predefined, &t) != 0) return -1;
    second.BeginIn(s.width, s.height, t.modes[0]);
    if (zmx_compress_device(c.options, ZOPFLI_FORMAT_ZLIB, t.scan.p, t.start[1], &second.bytes, &second.size) != 0) return -1;
    if (!second.Close()) return BadStream(c.w);
    Smaller(file, second).GiveTo(out, outsize);
    return 0;
  }
  file.GiveTo(out, outsize);
  return 0;
}

// The same with the file left in device memory: the stream goes zmx_compress_device_to_device's way with the file's frame
// around it.  Where no second try can be due — no statistics, or a mode other than a palette — the one file goes straight
// into d_out.  Else which file is kept, and so its size, is known only when the first is made — so the first goes into a
// buffer of the call's own, the second (where one is due) into another, and ONE device-to-device copy puts the kept file
// into d_out: every byte of the file is written and none outside it, and a capacity of exactly the kept file's size does.
int FinishOneToDevice(const Call& c, const Kind& kind, const Front& f, const DeviceDest& dest, size_t* outsize) {
  const Subject& s = f.subjects[0];
  const char* const w = c.w.c_str();
  const int device = f.device;
  const zamd::PngFrame frame = FrameIn(s.width, s.height, s.mode);
  if (!SecondTryDue(s, 0)) {
    return zamd::CompressDeviceToDevice(w, c.options, ZOPFLI_FORMAT_ZLIB, f.Scan(0), f.ScanBytes(0), dest.d_out, dest.capacity, outsize, &frame);
  }
  DeviceBuffer first, second;
  first.device = second.device = device;
  const size_t room = FileBound(f.ScanBytes(0));
  size_t first_bytes = 0, second_bytes = 0;
  if (zmx_internal_device_alloc(device, room, &first.p) != 0) return -1;
  if (zamd::CompressDeviceToDevice(w, c.options, ZOPFLI_FORMAT_ZLIB, f.Scan(0), f.ScanBytes(0), first.p, room, &first_bytes, &frame) != 0) {
    *outsize = first_bytes;   // (a stream that fits no IDAT: the size it would have taken)
    return -1;
  }
  const void* kept = first.p;
  size_t kept_bytes = first_bytes;
  if (SecondTryDue(s, first_bytes)) {
    SecondTries t;
    if (MakeSecondTries(kind, device, {&s}, c.predefined, &t) != 0) return -1;
    const zamd::PngFrame frame2 = FrameIn(s.width, s.height, t.modes[0]);
    const size_t room2 = FileBound(t.start[1]);
    if (zmx_internal_device_alloc(device, room2, &second.p) != 0) return -1;
    if (zamd::CompressDeviceToDevice(w, c.options, ZOPFLI_FORMAT_ZLIB, t.scan.p, t.start[1], second.p, room2, &second_bytes, &frame2) != 0) return -1;
    if (second_bytes < first_bytes) {
      kept = second.p;
      kept_bytes = second_bytes;
    }
  }
  *outsize = kept_bytes;
  if (kept_bytes > dest.capacity) {
    return Refuse(c.w + ": the file takes " + std::to_string(kept_bytes) + " bytes, d_out has " + std::to_string(dest.capacity));
  }
  return zmx_internal_device_copy(device, dest.d_out, kept, kept_bytes);
}

// ---- the four shapes of an entry
int One(const Call& c, const Kind& kind, unsigned char** out, size_t* outsize) {
  if (!c.options || !kind.given || !out || !outsize) return Refuse(c.w + ": null argument");
  Front f;
  if (MakeFront(c, kind, 1, true, nullptr, &f) != 0) return -1;
  return FinishOne(c, kind, f, out, outsize);
}

int OneToDevice(const Call& c, const Kind& kind, void* d_out, size_t capacity, size_t* outsize) {
  if (!c.options || !kind.given || !outsize) return Refuse(c.w + ": null argument");
  *outsize = 0;
  const DeviceDest dest{d_out, capacity};
  Front f;
  if (MakeFront(c, kind, 1, true, &dest, &f) != 0) return -1;
  return FinishOneToDevice(c, kind, f, dest, outsize);
}

int Batch(const Call& c, const Kind& kind, size_t n, unsigned char** out, size_t* outsize) {
  if (n == 0) return 0;
  if (!c.options || !kind.given || !out || !outsize) return Refuse(c.w + ": null argument");
  Front f;
  if (MakeFront(c, kind, n, false, nullptr, &f) != 0) return -1;
  return FinishBatch(c, kind, f, out, outsize);
}

// The first files left in one arena: zmx_compress_device_batch_packed's plan with a frame per stream.  (For a kind without
// a second try: the encode entries.)
int BatchPacked(const Call& c, const Kind& kind, size_t n, void* d_arena, size_t capacity, size_t align, size_t* outoffset, size_t* outsize) {
  if (n == 0) return 0;
  if (!c.options || !kind.given || !outoffset || !outsize) return Refuse(c.w + ": null argument");
  if (!zamd::PackedAlignOk(align)) return Refuse(c.w + ": align " + std::to_string(align) + " is not a power of two from 1 to 4096");
  const DeviceDest dest{d_arena, capacity};
  Front f;
  if (MakeFront(c, kind, n, false, &dest, &f) != 0) return -1;
  std::vector<const void*> slices(n);
  std::vector<size_t> sizes(n);
  std::vector<zamd::PngFrame> frames(n);
  for (size_t i = 0; i < n; ++i) {
    slices[i] = f.Scan(i);
    sizes[i] = f.ScanBytes(i);
    frames[i] = FrameIn(f.subjects[i].width, f.subjects[i].height, f.subjects[i].mode);
  }
  return zamd::CompressDeviceBatchPackedFramed(c.w.c_str(), c.options, n, slices.data(), sizes.data(), frames.data(), d_arena, capacity, align,
                                               outoffset, outsize);
}

}  // namespace

// ---- zmx_png_encode_device and its kin: the image's own colour mode
extern "C" int zmx_png_encode_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                     const unsigned char* predefined, unsigned char** out, size_t* outsize) {
  return One(Call{"zmx_png_encode_device", options, strategy, predefined, 0}, ColourKind(image, false), out, outsize);
}
extern "C" int zmx_png_encode_device_lossy(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                           const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return One(Call{"zmx_png_encode_device_lossy", options, strategy, predefined, lossy}, ColourKind(image, false), out, outsize);
}
extern "C" int zmx_png_encode_device_to_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                               const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize) {
  return OneToDevice(Call{"zmx_png_encode_device_to_device", options, strategy, predefined, lossy}, ColourKind(image, false), d_out, capacity,
                     outsize);
}
extern "C" int zmx_png_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                           unsigned char** out, size_t* outsize) {
  return Batch(Call{"zmx_png_encode_device_batch", options, strategy, nullptr, 0}, ColourKind(images, false), n, out, outsize);
}
extern "C" int zmx_png_encode_device_batch_lossy(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                                 unsigned lossy, unsigned char** out, size_t* outsize) {
  return Batch(Call{"zmx_png_encode_device_batch_lossy", options, strategy, nullptr, lossy}, ColourKind(images, false), n, out, outsize);
}
extern "C" int zmx_png_encode_device_batch_packed(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                                  unsigned lossy, void* d_arena, size_t capacity, size_t align, size_t* outoffset,
                                                  size_t* outsize) {
  return BatchPacked(Call{"zmx_png_encode_device_batch_packed", options, strategy, nullptr, lossy}, ColourKind(images, false), n, d_arena,
                     capacity, align, outoffset, outsize);
}

// ---- zmx_png_optimize_device and its kin: the colour mode reduced first (png_color_choose.h)
extern "C" int zmx_png_optimize_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                       const unsigned char* predefined, unsigned char** out, size_t* outsize) {
  return One(Call{"zmx_png_optimize_device", options, strategy, predefined, 0}, ColourKind(image, true), out, outsize);
}
extern "C" int zmx_png_optimize_device_lossy(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                             const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return One(Call{"zmx_png_optimize_device_lossy", options, strategy, predefined, lossy}, ColourKind(image, true), out, outsize);
}
extern "C" int zmx_png_optimize_device_to_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                                 const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                 size_t* outsize) {
  return OneToDevice(Call{"zmx_png_optimize_device_to_device", options, strategy, predefined, lossy}, ColourKind(image, true), d_out, capacity,
                     outsize);
}
extern "C" int zmx_png_optimize_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                             unsigned char** out, size_t* outsize) {
  return Batch(Call{"zmx_png_optimize_device_batch", options, strategy, nullptr, 0}, ColourKind(images, true), n, out, outsize);
}
extern "C" int zmx_png_optimize_device_batch_lossy(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                                   unsigned lossy, unsigned char** out, size_t* outsize) {
  return Batch(Call{"zmx_png_optimize_device_batch_lossy", options, strategy, nullptr, lossy}, ColourKind(images, true), n, out, outsize);
}

// ---- the index entries, and the host arithmetic they share with tests and tools
extern "C" int zmx_png_index_encode_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                           const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return One(Call{"zmx_png_index_encode_device", options, strategy, predefined, lossy}, IndexKind(image, false), out, outsize);
}
extern "C" int zmx_png_index_optimize_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                             const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return One(Call{"zmx_png_index_optimize_device", options, strategy, predefined, lossy}, IndexKind(image, true), out, outsize);
}
extern "C" int zmx_png_index_encode_device_to_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                                     const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                     size_t* outsize) {
  return OneToDevice(Call{"zmx_png_index_encode_device_to_device", options, strategy, predefined, lossy}, IndexKind(image, false), d_out,
                     capacity, outsize);
}
extern "C" int zmx_png_index_optimize_device_to_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                                       const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                       size_t* outsize) {
  return OneToDevice(Call{"zmx_png_index_optimize_device_to_device", options, strategy, predefined, lossy}, IndexKind(image, true), d_out,
                     capacity, outsize);
}
extern "C" int zmx_png_index_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy,
                                                 unsigned lossy, unsigned char** out, size_t* outsize) {
  return Batch(Call{"zmx_png_index_encode_device_batch", options, strategy, nullptr, lossy}, IndexKind(images, false), n, out, outsize);
}
extern "C" int zmx_png_index_optimize_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy,
                                                   unsigned lossy, unsigned char** out, size_t* outsize) {
  return Batch(Call{"zmx_png_index_optimize_device_batch", options, strategy, nullptr, lossy}, IndexKind(images, true), n, out, outsize);
}

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
    const size_t slice = RoundUp16(plan.nbytes);
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

// The source entries with host output: `reduce` the optimize ones; `single`: one source, with `predefined`.
int SourcesToHost(const std::string& w, bool reduce, bool single, const ZopfliOptions* options, size_t n, const zmx_png_source* sources,
                  int strategy, const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  if (n == 0) return 0;
  if (!options || !sources || !out || !outsize) return Refuse(w + ": null argument");
  if (CheckBehindPack(w, strategy, lossy, single, predefined, sources) != 0) return -1;
  Packed p;
  if (PackSources(w, n, sources, nullptr, &p) != 0) return -1;
  const Call c{w, options, strategy, predefined, lossy};
  const ColourKind kind(p.images.data(), reduce);
  return single ? One(c, kind, out, outsize) : Batch(c, kind, n, out, outsize);
}

// ... with the file left in device memory
int SourceToDevice(const std::string& w, bool reduce, const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                   const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize) {
  if (!options || !source || !outsize) return Refuse(w + ": null argument");
  *outsize = 0;
  if (CheckBehindPack(w, strategy, lossy, true, predefined, source) != 0) return -1;
  const DeviceDest dest{d_out, capacity};
  Packed p;
  if (PackSources(w, 1, source, &dest, &p) != 0) return -1;
  return OneToDevice(Call{w, options, strategy, predefined, lossy}, ColourKind(p.images.data(), reduce), d_out, capacity, outsize);
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
  return SourcesToHost("zmx_png_encode_source_device", false, true, options, 1, source, strategy, predefined, lossy, out, outsize);
}
extern "C" int zmx_png_optimize_source_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                              const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize) {
  return SourcesToHost("zmx_png_optimize_source_device", true, true, options, 1, source, strategy, predefined, lossy, out, outsize);
}
extern "C" int zmx_png_encode_source_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                                  unsigned lossy, unsigned char** out, size_t* outsize) {
  return SourcesToHost("zmx_png_encode_source_device_batch", false, false, options, n, sources, strategy, nullptr, lossy, out, outsize);
}
extern "C" int zmx_png_optimize_source_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                                    unsigned lossy, unsigned char** out, size_t* outsize) {
  return SourcesToHost("zmx_png_optimize_source_device_batch", true, false, options, n, sources, strategy, nullptr, lossy, out, outsize);
}
extern "C" int zmx_png_encode_source_device_to_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                                      const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                      size_t* outsize) {
  return SourceToDevice("zmx_png_encode_source_device_to_device", false, options, source, strategy, predefined, lossy, d_out, capacity, outsize);
}
extern "C" int zmx_png_optimize_source_device_to_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                                        const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                                        size_t* outsize) {
  return SourceToDevice("zmx_png_optimize_source_device_to_device", true, options, source, strategy, predefined, lossy, d_out, capacity, outsize);
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
  return BatchPacked(Call{w, options, strategy, nullptr, lossy}, ColourKind(p.images.data(), false), n, d_arena, capacity, align, outoffset,
                     outsize);
}
