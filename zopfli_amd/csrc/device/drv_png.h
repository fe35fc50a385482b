// Driver part: LodePNG's filter choices on the device (zmx_png.h, zmx_png_brute.h) and the filtered scanlines
// (zmx_png_rows.h).  Holds zmx_png_filter_types, zmx_png_filter_types_brute, their device-image form
// zmx_png_filter_types_device, zmx_png_filter_rows_device and the encoder's zmx_internal_png_scanlines; the colour
// statistics and conversion (zmx_png_color.h); zopflipng's --lossy_transparent (zmx_png_lossy.h); index images
// (zmx_png_index.h: zmx_png_index_use_device, zmx_png_index_convert_device); LodePNG's zlib size of
// device buffers and the rows of zopflipng's strategy trials (zmx_png_lodeflate.h).  Needs drv_context.h (zmx_ctx,
// PoolScope) and drv_input.h (CheckDevicePointer).
#pragma once

// an image the kernels can index with 32 bits: rows of `linebytes`, at most `max_height` of them, pixels of 1 .. 8 bytes
static bool PngGeometryOk(size_t linebytes, size_t height, size_t max_height, size_t bytewidth) {
  return linebytes != 0 && bytewidth != 0 && linebytes <= 0x7fffffffu && height <= max_height && bytewidth <= 8;
}

// k_png_filter_types on an image in memory of the context's device: the types into d_minsum / d_entropy ([height] each,
// either may be null), queued on the context's stream.
static int PngHeuristicTypes(zmx_ctx* c, const u8* d_img, size_t linebytes, size_t height, size_t bytewidth, u8* d_minsum,
                             u8* d_entropy) {
  PngFilterParams pp;
  pp.image = d_img;
  pp.linebytes = static_cast<u32>(linebytes);
  pp.height = static_cast<u32>(height);
  pp.bytewidth = static_cast<u32>(bytewidth);
  pp.minsum = d_minsum;
  pp.entropy = d_entropy;
  hipLaunchKernelGGL(k_png_filter_types, dim3(static_cast<unsigned>(height)), dim3(PNGF_THREADS), 0, c->stream, pp);
  KCHK(c, "k_png_filter_types");
  return 0;
}

static bool PngWindowOk(unsigned windowsize) {   // LodePNG's errors 60 / 90
  return windowsize != 0 && windowsize <= 32768u && (windowsize & (windowsize - 1u)) == 0;
}

static_assert(zamd::kPngBruteHeadBytes == PNGB_HEAD_BYTES && zamd::kPngBruteLdsMax == PNGB_LDS_MAX, "host/png_brute_launch.h restates zmx_png_brute.h");

// What a test may take of a search besides the types (zmx_internal_png_brute_sizes): device arrays of `tmp`, [5 * height]
// each, that live as long as `tmp` does.
struct PngBruteArrays {
  u64* d_sizes = nullptr;
  u64* d_bits = nullptr;
};

// k_png_brute + k_png_brute_pick on an image in memory of the context's device: the types into d_types[height], queued on
// the context's stream; the scratch arrays are `tmp`'s.  The launch is host/png_brute_launch.h's; `knobs` are a test's
// (the default everywhere else), and so is `arrays`, which makes the kernel keep its bit counts.
static int PngBruteTypes(zmx_ctx* c, PoolScope* tmp, const u8* d_img, size_t linebytes, size_t height, size_t bytewidth,
                         unsigned windowsize, u8* d_types, const zamd::PngBruteKnobs& knobs, PngBruteArrays* arrays = nullptr) {
  const u32 n = static_cast<u32>(linebytes), jobs = static_cast<u32>(5 * height);
  const zamd::PngBruteLaunch L = zamd::PngBruteMakeLaunch(n, jobs, knobs);
  const u64 stride = L.stride;
  const u32 grid = L.grid;
  if (L.raise_lds_limit) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_png_brute), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(PNGB_LDS_MAX)));
  }
  u8* d_scratch = nullptr;
  u64* d_sizes = nullptr;
  HIPCHK(tmp->AllocT(&d_scratch, static_cast<size_t>(stride) * grid, "d_png_brute_scratch"));
  HIPCHK(tmp->AllocT(&d_sizes, static_cast<size_t>(jobs), "d_png_brute_sizes"));
  PngBruteParams pp;
  pp.image = d_img;
  pp.linebytes = n;
  pp.height = static_cast<u32>(height);
  pp.bytewidth = static_cast<u32>(bytewidth);
  pp.window = windowsize;
  pp.jobs = jobs;
  pp.scratch = d_scratch;
  pp.scratch_stride = stride;
  pp.in_lds = L.in_lds ? 1u : 0u;
  pp.sizes = d_sizes;
  if (arrays) {
    HIPCHK(tmp->AllocT(&pp.bits, static_cast<size_t>(jobs), "d_png_brute_bits"));
    arrays->d_sizes = d_sizes;
    arrays->d_bits = pp.bits;
  }
  hipLaunchKernelGGL(k_png_brute, dim3(grid), dim3(PNGB_THREADS), L.lds_bytes, c->stream, pp);
  KCHK(c, "k_png_brute");
  hipLaunchKernelGGL(k_png_brute_pick, dim3(static_cast<unsigned>((height + 255) / 256)), dim3(256), 0, c->stream,
                     static_cast<const u64*>(d_sizes), static_cast<u32>(height), d_types);
  KCHK(c, "k_png_brute_pick");
  return 0;
}

// The types of `strategy` (ZMX_PNG_FILTER_ZERO .. _BRUTE) for an image in memory of the context's device, into
// d_types[height] (the same device), queued on the context's stream; everything checked by the caller but the strategy
// and the limits that depend on it.
static int PngTypesOnDevice(zmx_ctx* c, PoolScope* tmp, const char* who, const u8* d_img, size_t linebytes, size_t height,
                            size_t bytewidth, int strategy, unsigned windowsize, u8* d_types) {
  const std::string w(who);
  if (strategy >= ZMX_PNG_FILTER_ZERO && strategy <= ZMX_PNG_FILTER_FOUR) {
    HIPCHK(hipMemsetAsync(d_types, strategy, height, c->stream));
    return 0;
  }
  if (strategy == ZMX_PNG_FILTER_MINSUM) return PngHeuristicTypes(c, d_img, linebytes, height, bytewidth, d_types, nullptr);
  if (strategy == ZMX_PNG_FILTER_ENTROPY) return PngHeuristicTypes(c, d_img, linebytes, height, bytewidth, nullptr, d_types);
  if (strategy != ZMX_PNG_FILTER_BRUTE) return FailMsg(w + ": unknown strategy " + std::to_string(strategy));
  if (!PngWindowOk(windowsize)) return FailMsg(w + ": the window must be a power of two of at most 32768");
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu / 5u, bytewidth)) return FailMsg(w + ": bad geometry");
  return PngBruteTypes(c, tmp, d_img, linebytes, height, bytewidth, windowsize, d_types, zamd::PngBruteKnobs());
}

static bool PngStrategyKnown(int strategy) { return strategy >= ZMX_PNG_FILTER_ZERO && strategy <= ZMX_PNG_FILTER_BRUTE; }

static bool RangesOverlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t alo = reinterpret_cast<uintptr_t>(a), blo = reinterpret_cast<uintptr_t>(b);
  return na != 0 && nb != 0 && alo < blo + nb && blo < alo + na;
}

static thread_local double g_png_rows_ms = 0;   // (zmx_internal_png_rows_ms)

// k_png_rows, the caller having checked everything: queued on the context's stream, then drained; the flag read.
static int PngRowsOnDevice(zmx_ctx* c, PoolScope* tmp, const char* who, const u8* d_img, size_t linebytes, size_t height,
                           size_t bytewidth, const u8* d_types, u8* d_out) {
  u32* d_bad = nullptr;
  HIPCHK(tmp->AllocT(&d_bad, 1, "d_png_bad_row"));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, sizeof(u32), c->stream));
  zamd::PngRowsParams P;
  P.image = d_img;
  P.types = d_types;
  P.out = d_out;
  P.linebytes = linebytes;
  P.height = height;
  P.bytewidth = static_cast<u32>(bytewidth);
  P.bad_row = d_bad;
  const bool timed = KernelTiming();
  if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
  hipLaunchKernelGGL(k_png_rows, dim3(zamd::PngRowsGrid(static_cast<u64>(height) * (linebytes + 1))),
                     dim3(zamd::kPngRowsThreads), 0, c->stream, P);
  KCHK(c, "k_png_rows");
  if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
  u32 bad = zamd::kPngRowsNoBadRow;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_png_rows_ms = ms;
  }
  if (bad != zamd::kPngRowsNoBadRow) {
    return FailMsg(std::string(who) + ": row " + std::to_string(bad) + " has a filter type above 4");
  }
  return 0;
}

// ---- colour statistics and conversion (zmx_png_color.h)
static_assert(sizeof(zamd::PngColorSummary) == sizeof(zmx_png_color_stats), "PngColorSummary is zmx_png_color_stats");

static thread_local double g_png_color_ms[3] = {0, 0, 0};   // k_png_color_stats, k_png_color_key, k_png_convert (zmx_internal_png_color_ms)

// What every colour entry refuses of an image before its pointer is looked at; *nbytes its size.
static int PngColorImageOf(const char* who, const zmx_png_image* image, zamd::PngColorImage* I, size_t* nbytes) {
  const std::string w(who);
  if (!image) return FailMsg(w + ": no image");
  if (image->width == 0 || image->height == 0) return FailMsg(w + ": width or height 0");
  const u32 ct = image->colortype, depth = image->bitdepth;
  if (!(ct == 0 || ct == 2 || ct == 4 || ct == 6) || !(depth == 8 || depth == 16)) {
    return FailMsg(w + ": colour type " + std::to_string(ct) + " at " + std::to_string(depth) + " bits is not taken (0, 2, 4, 6 at 8 or 16)");
  }
  const u64 linebytes = static_cast<u64>(image->width) * zamd::PngColorPixelBytes(ct, depth);
  if (!PngGeometryOk(linebytes, image->height, 0x7fffffffu, zamd::PngColorPixelBytes(ct, depth))) return FailMsg(w + ": bad geometry");
  const u64 numpixels = static_cast<u64>(image->width) * image->height;
  if (numpixels > 0xffffffffull) return FailMsg(w + ": an image of 2^32 pixels or more");
  I->pixels = static_cast<const u8*>(image->d_pixels);
  I->numpixels = numpixels;
  I->width = image->width;
  I->height = image->height;
  I->colortype = ct;
  I->bitdepth = depth;
  *nbytes = static_cast<size_t>(linebytes * image->height);
  return 0;
}

// The statistics of an image the caller has checked: one launch, the state read, k_png_color_key and a second read where
// a key is possible.  Drains the context's stream.
static int PngColorStatsOnDevice(zmx_ctx* c, PoolScope* tmp, const zamd::PngColorImage& I, zmx_png_color_stats* out) {
  zamd::PngColorState* d_state = nullptr;
  HIPCHK(tmp->AllocT(&d_state, 1, "d_png_color_state"));
  u8* const raw = reinterpret_cast<u8*>(d_state);
  const size_t zeros = offsetof(zamd::PngColorState, key_min);
  HIPCHK(hipMemsetAsync(raw, 0, zeros, c->stream));
  HIPCHK(hipMemsetAsync(raw + zeros, 0xff, sizeof(zamd::PngColorState) - zeros, c->stream));
  const bool timed = KernelTiming();
  const u32 grid = zamd::PngColorGrid(I);
  if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
  hipLaunchKernelGGL(k_png_color_stats, dim3(grid), dim3(zamd::kPngColorThreads), 0, c->stream, I, d_state);
  KCHK(c, "k_png_color_stats");
  if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
  zamd::PngColorState state;
  HIPCHK(hipMemcpyAsync(&state, d_state, sizeof(state), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_png_color_ms[0] = ms;
  }
  if (zamd::PngColorWantsKeyPass(state)) {
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_png_color_key, dim3(grid), dim3(zamd::kPngColorThreads), 0, c->stream, I, state.key_min, d_state);
    KCHK(c, "k_png_color_key");
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipMemcpyAsync(&state.key_clash, &d_state->key_clash, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (timed) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
      g_png_color_ms[1] = ms;
    }
  }
  zamd::PngColorSummary sum;
  zamd::PngColorFinish(state, I.bitdepth, &sum);
  std::memcpy(out, &sum, sizeof(sum));
  return 0;
}

// k_png_convert, the caller having checked everything: the image in `mode` into d_out.  Drains the context's stream.
static int PngConvertOnDevice(zmx_ctx* c, PoolScope* tmp, const char* who, const zamd::PngColorImage& I, const zmx_png_color_mode& mode,
                              u8* d_out) {
  u32* d_bad = nullptr;
  u8* d_palette = nullptr;
  HIPCHK(tmp->AllocT(&d_bad, 1, "d_png_bad_pixel"));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, sizeof(u32), c->stream));
  if (mode.colortype == 3) HIPCHK(tmp->Upload(&d_palette, mode.palette, 4 * static_cast<size_t>(mode.palettesize), "d_png_palette"));
  zamd::PngConvParams P;
  P.in = I;
  P.out = d_out;
  P.rowbytes = zamd::PngConvRowBytes(I.width, mode.colortype, mode.bitdepth);
  P.colortype = mode.colortype;
  P.bitdepth = mode.bitdepth;
  P.palettesize = mode.colortype == 3 ? mode.palettesize : 0;
  P.palette = d_palette;
  P.bad_pixel = d_bad;
  const bool timed = KernelTiming();
  if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
  hipLaunchKernelGGL(k_png_convert, dim3(zamd::PngConvGrid(P.rowbytes * I.height)), dim3(zamd::kPngColorThreads), 0, c->stream, P);
  KCHK(c, "k_png_convert");
  if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
  u32 bad = zamd::kPngColorNoBadPixel;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_png_color_ms[2] = ms;
  }
  if (bad != zamd::kPngColorNoBadPixel) {
    return FailMsg(std::string(who) + ": pixel " + std::to_string(bad) + " has a colour that is not in the palette");
  }
  return 0;
}

// ---- zopflipng's --lossy_transparent (zmx_png_lossy.h)
static thread_local double g_png_lossy_ms[3] = {0, 0, 0};   // k_png_lossy_stats, k_png_lossy_carry, k_png_lossy_fill (zmx_internal_png_lossy_ms)

// One kernel's time where kernel timing is on: between Begin and End on the context's stream; End drains it.
struct PngLossyTimer {
  zmx_ctx* c;
  bool timed;
  hipError_t Begin() { return timed ? hipEventRecord(c->ev[0], c->stream) : hipSuccess; }
  hipError_t End(double* ms) {
    if (!timed) return hipSuccess;
    hipError_t e = hipEventRecord(c->ev[1], c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    float f = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&f, c->ev[0], c->ev[1]);
    *ms = f;
    return e;
  }
};

// The rewrite of an image the caller has checked (colour type 4 or 6), into d_out — the image's own pixels: in place.
// Statistics, the state read, then the carry scan (mode 2) and the fill, or with `copy_when_none` a copy where no pixel is
// transparent.  *info is filled.  Drains the context's stream.
static int PngLossyOnDevice(zmx_ctx* c, PoolScope* tmp, const zamd::PngColorImage& I, size_t nbytes, u8* d_out, bool copy_when_none,
                            zmx_png_lossy_info* info) {
  const u64 tiles = zamd::PngLossyTiles(I);
  const u32 grid = zamd::PngLossyGrid(I);
  zamd::PngLossyState* d_state = nullptr;
  u32* d_summaries = nullptr;
  HIPCHK(tmp->AllocT(&d_state, 1, "d_png_lossy_state"));
  HIPCHK(tmp->AllocT(&d_summaries, static_cast<size_t>(tiles), "d_png_lossy_summaries"));
  u8* const raw = reinterpret_cast<u8*>(d_state);
  HIPCHK(hipMemsetAsync(raw, 0xff, sizeof(zamd::PngLossyState), c->stream));
  HIPCHK(hipMemsetAsync(raw + offsetof(zamd::PngLossyState, color), 0, offsetof(zamd::PngColorState, key_min), c->stream));
  PngLossyTimer timer{c, KernelTiming()};
  HIPCHK(timer.Begin());
  hipLaunchKernelGGL(k_png_lossy_stats, dim3(grid), dim3(zamd::kPngLossyThreads), 0, c->stream, I, d_state, d_summaries);
  KCHK(c, "k_png_lossy_stats");
  HIPCHK(timer.End(&g_png_lossy_ms[0]));
  zamd::PngLossyState state;   // (all of it but the table)
  HIPCHK(hipMemcpyAsync(&state, d_state, offsetof(zamd::PngLossyState, color) + offsetof(zamd::PngColorState, table), hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const zamd::PngLossyDecision d = zamd::PngLossyDecide(state);
  *info = zmx_png_lossy_info();
  info->mode = d.mode;
  info->partial_alpha = d.partial_alpha;
  info->numcolors = d.numcolors;
  info->first_transparent = state.first_transparent == zamd::kPngLossyNoIndex ? UINT64_MAX : state.first_transparent;
  if (d.mode == zamd::kPngLossyModeNone) {
    if (copy_when_none && d_out != I.pixels) {
      HIPCHK(hipMemcpyAsync(d_out, I.pixels, nbytes, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
  }
  zamd::PngLossyParams P;
  P.in = I;
  P.out = d_out;
  P.mode = d.mode;
  P.first_transparent = state.first_transparent;
  P.carry_in = nullptr;
  P.state = d_state;
  if (d.mode == zamd::kPngLossyModeCarry) {
    u32* d_carry = nullptr;
    HIPCHK(tmp->AllocT(&d_carry, static_cast<size_t>(tiles), "d_png_lossy_carry"));
    HIPCHK(timer.Begin());
    hipLaunchKernelGGL(k_png_lossy_carry, dim3(1), dim3(zamd::kPngLossyThreads), 0, c->stream, static_cast<const u32*>(d_summaries), d_carry,
                       tiles);
    KCHK(c, "k_png_lossy_carry");
    HIPCHK(timer.End(&g_png_lossy_ms[1]));
    P.carry_in = d_carry;
  }
  HIPCHK(timer.Begin());
  hipLaunchKernelGGL(k_png_lossy_fill, dim3(grid), dim3(zamd::kPngLossyThreads), 0, c->stream, P);
  KCHK(c, "k_png_lossy_fill");
  HIPCHK(timer.End(&g_png_lossy_ms[2]));
  u32 fill = 0;
  if (d.mode == zamd::kPngLossyModeFixed) HIPCHK(hipMemcpyAsync(&fill, &d_state->fill, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  info->fill_r = fill & 255u;
  info->fill_g = (fill >> 8) & 255u;
  info->fill_b = (fill >> 16) & 255u;
  return 0;
}

extern "C" {
double zmx_internal_png_rows_ms(void) { return g_png_rows_ms; }
void zmx_internal_png_color_ms(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_png_color_ms[k];
}
void zmx_internal_png_lossy_ms(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_png_lossy_ms[k];
}

int zmx_png_color_stats_device(zmx_ctx* c, const zmx_png_image* image, zmx_png_color_stats* out) {
  const char* who = "zmx_png_color_stats_device";
  g_png_color_ms[0] = g_png_color_ms[1] = 0;
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (!out) return FailMsg(std::string(who) + ": no output");
  zamd::PngColorImage I;
  size_t nbytes = 0;
  if (const int rc = PngColorImageOf(who, image, &I, &nbytes)) return rc;
  int img_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (img_device != c->device) return FailMsg(std::string(who) + ": memory of another device than the context's");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  const int rc = PngColorStatsOnDevice(c, &tmp, I, out);
  if (rc != 0) (void)hipStreamSynchronize(c->stream);   // what was queued may still use `tmp`'s arrays
  return rc;
}

int zmx_png_convert_device(zmx_ctx* c, const zmx_png_image* image, const zmx_png_color_mode* mode, void* d_out, size_t capacity) {
  const char* who = "zmx_png_convert_device";
  g_png_color_ms[2] = 0;
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (!mode) return FailMsg(std::string(who) + ": no mode");
  zamd::PngColorImage I;
  size_t nbytes = 0;
  if (const int rc = PngColorImageOf(who, image, &I, &nbytes)) return rc;
  if (!zamd::PngModeOk(*mode, I.bitdepth)) {
    return FailMsg(std::string(who) + ": colour type " + std::to_string(mode->colortype) + " at " + std::to_string(mode->bitdepth) +
                   " bits with a palette of " + std::to_string(mode->palettesize) + " is no mode this image converts to");
  }
  const u64 rowbytes = zamd::PngConvRowBytes(I.width, mode->colortype, mode->bitdepth);
  if (rowbytes > 0x7fffffffu) return FailMsg(std::string(who) + ": bad geometry");
  const size_t total = static_cast<size_t>(rowbytes * I.height);
  if (capacity < total) {
    return FailMsg(std::string(who) + ": the output takes " + std::to_string(total) + " bytes, the capacity is " + std::to_string(capacity));
  }
  int img_device = -1, out_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (const int rc = CheckDevicePointer(who, d_out, total, &out_device)) return rc;
  if (img_device != c->device || out_device != c->device) return FailMsg(std::string(who) + ": memory of another device than the context's");
  if (RangesOverlap(d_out, total, image->d_pixels, nbytes)) return FailMsg(std::string(who) + ": the output overlaps the image");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  const int rc = PngConvertOnDevice(c, &tmp, who, I, *mode, static_cast<u8*>(d_out));
  if (rc != 0) (void)hipStreamSynchronize(c->stream);
  return rc;
}

int zmx_png_lossy_transparent_device(zmx_ctx* c, const zmx_png_image* image, void* d_out, size_t capacity, zmx_png_lossy_info* info) {
  const char* who = "zmx_png_lossy_transparent_device";
  g_png_lossy_ms[0] = g_png_lossy_ms[1] = g_png_lossy_ms[2] = 0;
  if (!c) return FailMsg(std::string(who) + ": no context");
  zamd::PngColorImage I;
  size_t nbytes = 0;
  if (const int rc = PngColorImageOf(who, image, &I, &nbytes)) return rc;
  if (capacity < nbytes) {
    return FailMsg(std::string(who) + ": the output takes " + std::to_string(nbytes) + " bytes, the capacity is " + std::to_string(capacity));
  }
  int img_device = -1, out_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (const int rc = CheckDevicePointer(who, d_out, nbytes, &out_device)) return rc;
  if (img_device != c->device || out_device != c->device) return FailMsg(std::string(who) + ": memory of another device than the context's");
  if (d_out != image->d_pixels && RangesOverlap(d_out, nbytes, image->d_pixels, nbytes)) {
    return FailMsg(std::string(who) + ": the output overlaps the image without being the image");
  }
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  zmx_png_lossy_info got = zmx_png_lossy_info();
  got.first_transparent = UINT64_MAX;
  int rc = 0;
  if (I.colortype == 4 || I.colortype == 6) {
    rc = PngLossyOnDevice(c, &tmp, I, nbytes, static_cast<u8*>(d_out), true, &got);
  } else if (d_out != image->d_pixels) {
    // (no alpha channel: nothing is transparent)
    const hipError_t e = hipMemcpyAsync(d_out, image->d_pixels, nbytes, hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) rc = Fail("hipMemcpyAsync(image)", e, __FILE__, __LINE__);
  }
  const hipError_t e = hipStreamSynchronize(c->stream);   // what was queued may still use `tmp`'s arrays
  if (rc != 0) return rc;
  HIPCHK(e);
  if (info) *info = got;
  return 0;
}

// The _lossy entries' device part (host/png_encode.cc; zmx_internal.h says what it makes).
int zmx_internal_png_lossy_image(zmx_ctx* c, const char* who, const zmx_png_image* image, int to8, int transparent, void* d_buf,
                                 zmx_png_image* work) {
  zamd::PngColorImage I;
  size_t nbytes = 0;
  if (const int rc = PngColorImageOf(who, image, &I, &nbytes)) return rc;
  int img_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (img_device != c->device) return FailMsg(std::string(who) + ": the image is memory of another device than the context's");
  *work = *image;
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  int rc = 0;
  if (to8 && I.bitdepth == 16) {
    zmx_png_color_mode mode = zmx_png_color_mode();
    mode.colortype = I.colortype;
    mode.bitdepth = 8;
    rc = PngConvertOnDevice(c, &tmp, who, I, mode, static_cast<u8*>(d_buf));
    I.pixels = static_cast<const u8*>(d_buf);
    I.bitdepth = 8;
    nbytes /= 2;
    work->d_pixels = d_buf;
    work->bitdepth = 8;
  }
  if (rc == 0 && transparent && I.bitdepth == 8 && (I.colortype == 4 || I.colortype == 6)) {
    zmx_png_lossy_info info;
    rc = PngLossyOnDevice(c, &tmp, I, nbytes, static_cast<u8*>(d_buf), false, &info);
    if (rc == 0 && info.mode != zamd::kPngLossyModeNone) work->d_pixels = d_buf;
  }
  if (rc != 0) (void)hipStreamSynchronize(c->stream);
  return rc;
}

// zmx_png_optimize_device's device part (host/png_optimize.cc): the image in `mode` (null: as it is) in memory of the
// context's pool, then the types of `strategy` and the filtered scanlines of that into d_out, a buffer of the caller's
// own of height * (rowbytes + 1) bytes on the context's device.  The caller has checked the image and the mode.
int zmx_internal_png_reduced_scanlines(zmx_ctx* c, const zmx_png_image* image, const zmx_png_color_mode* mode, int strategy,
                                       unsigned windowsize, const unsigned char* predefined, void* d_out) {
  const char* who = "zmx_png_optimize_device";
  zamd::PngColorImage I;
  size_t nbytes = 0;
  if (const int rc = PngColorImageOf(who, image, &I, &nbytes)) return rc;
  if (!mode) {
    return zmx_internal_png_scanlines(c, image->d_pixels, nbytes / I.height, I.height, zamd::PngColorPixelBytes(I.colortype, I.bitdepth),
                                      strategy, windowsize, predefined, d_out);
  }
  if (!zamd::PngModeOk(*mode, I.bitdepth)) return FailMsg(std::string(who) + ": no mode this image converts to");
  const u64 rowbytes = zamd::PngConvRowBytes(I.width, mode->colortype, mode->bitdepth);
  const u32 bpp = zamd::PngConvBpp(mode->colortype, mode->bitdepth);
  int img_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (img_device != c->device) return FailMsg(std::string(who) + ": the image is memory of another device than the context's");
  u8* d_conv = nullptr;
  {
    DEVICE_ENTRY(c->device);
    PoolScope tmp(c);
    HIPCHK(tmp.AllocT(&d_conv, static_cast<size_t>(rowbytes * I.height), "d_png_converted"));
    int rc = PngConvertOnDevice(c, &tmp, who, I, *mode, d_conv);
    if (rc == 0) {
      rc = zmx_internal_png_scanlines(c, d_conv, static_cast<size_t>(rowbytes), I.height, bpp < 8 ? 1 : bpp / 8, strategy, windowsize,
                                      predefined, d_out);
    }
    if (rc != 0) (void)hipStreamSynchronize(c->stream);
    return rc;
  }
}


// PNG filter heuristics (zmx_png.h): the filter type LodePNG's MINSUM / ENTROPY strategy picks for every scanline.
int zmx_png_filter_types(zmx_ctx* c, const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                         unsigned char* minsum_types, unsigned char* entropy_types) {
  if (!c) return FailMsg("zmx_png_filter_types: no context");
  if (height == 0 || (!minsum_types && !entropy_types)) return 0;
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu, bytewidth)) return FailMsg("zmx_png_filter_types: bad geometry");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  u8* d_img = nullptr;
  u8* d_types = nullptr;
  HIPCHK(tmp.Upload(&d_img, image, linebytes * height, "d_png_image"));
  HIPCHK(tmp.AllocT(&d_types, 2 * height, "d_png_types"));
  if (const int rc = PngHeuristicTypes(c, d_img, linebytes, height, bytewidth, minsum_types ? d_types : nullptr,
                                       entropy_types ? d_types + height : nullptr)) {
    return rc;
  }
  if (minsum_types) HIPCHK(hipMemcpyAsync(minsum_types, d_types, height, hipMemcpyDeviceToHost, c->stream));
  if (entropy_types) HIPCHK(hipMemcpyAsync(entropy_types, d_types + height, height, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// LodePNG's brute-force row search (zmx_png_brute.h): the filter type LFS_BRUTE_FORCE picks for every scanline when the
// rows are deflated with a window of `windowsize`.
int zmx_png_filter_types_brute(zmx_ctx* c, const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                               unsigned windowsize, unsigned char* types) {
  if (!c) return FailMsg("zmx_png_filter_types_brute: no context");
  if (!PngWindowOk(windowsize)) return FailMsg("zmx_png_filter_types_brute: the window must be a power of two of at most 32768");
  if (height == 0) return 0;
  if (!types) return FailMsg("zmx_png_filter_types_brute: no output");
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu / 5u, bytewidth)) return FailMsg("zmx_png_filter_types_brute: bad geometry");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  u8* d_img = nullptr;
  u8* d_types = nullptr;
  HIPCHK(tmp.Upload(&d_img, image, linebytes * height, "d_png_image"));
  HIPCHK(tmp.AllocT(&d_types, height, "d_png_types"));
  if (const int rc = PngBruteTypes(c, &tmp, d_img, linebytes, height, bytewidth, windowsize, d_types, zamd::PngBruteKnobs())) return rc;
  HIPCHK(hipMemcpyAsync(types, d_types, height, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// Test hook (tests/test_gpu_png_brute_sizes.py): zmx_png_filter_types_brute with the same checks that also hands over the
// five sizes and bit counts of every row as k_png_brute wrote them, and runs the launch a test asks for.
int zmx_internal_png_brute_sizes(zmx_ctx* c, const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                                 unsigned windowsize, int force_scratch, unsigned max_workgroups, uint64_t* sizes, uint64_t* bits,
                                 unsigned char* types) {
  const char* who = "zmx_internal_png_brute_sizes";
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (!PngWindowOk(windowsize)) return FailMsg(std::string(who) + ": the window must be a power of two of at most 32768");
  if (force_scratch != 0 && force_scratch != 1) return FailMsg(std::string(who) + ": force_scratch is 0 or 1");
  if (height == 0) return 0;
  if (!image || !sizes || !bits || !types) return FailMsg(std::string(who) + ": a null argument");
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu / 5u, bytewidth)) return FailMsg(std::string(who) + ": bad geometry");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  u8* d_img = nullptr;
  u8* d_types = nullptr;
  HIPCHK(tmp.Upload(&d_img, image, linebytes * height, "d_png_image"));
  HIPCHK(tmp.AllocT(&d_types, height, "d_png_types"));
  zamd::PngBruteKnobs knobs;
  knobs.force_scratch = force_scratch;
  knobs.max_workgroups = max_workgroups;
  PngBruteArrays arrays;
  const int rc = PngBruteTypes(c, &tmp, d_img, linebytes, height, bytewidth, windowsize, d_types, knobs, &arrays);
  // (what was queued uses the scratch arrays: drained before `tmp` gives them back, on the failing paths too)
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  HIPCHK(e);
  HIPCHK(hipMemcpy(sizes, arrays.d_sizes, 5 * height * sizeof(u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(bits, arrays.d_bits, 5 * height * sizeof(u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(types, d_types, height, hipMemcpyDeviceToHost));
  return 0;
}

// The row searches on an image that lies in device memory; the types stay there.
int zmx_png_filter_types_device(zmx_ctx* c, const void* d_image, size_t linebytes, size_t height, size_t bytewidth,
                                int strategy, unsigned windowsize, void* d_types) {
  const char* who = "zmx_png_filter_types_device";
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (!PngStrategyKnown(strategy)) return FailMsg(std::string(who) + ": unknown strategy " + std::to_string(strategy));
  if (height == 0) return 0;
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu, bytewidth)) return FailMsg(std::string(who) + ": bad geometry");
  int img_device = -1, types_device = -1;
  if (const int rc = CheckDevicePointer(who, d_image, linebytes * height, &img_device)) return rc;
  if (const int rc = CheckDevicePointer(who, d_types, height, &types_device)) return rc;
  if (img_device != c->device || types_device != c->device) return FailMsg(std::string(who) + ": memory of another device than the context's");
  if (RangesOverlap(d_image, linebytes * height, d_types, height)) return FailMsg(std::string(who) + ": the types overlap the image");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  const int rc = PngTypesOnDevice(c, &tmp, who, static_cast<const u8*>(d_image), linebytes, height, bytewidth, strategy,
                                  windowsize, static_cast<u8*>(d_types));
  // (what was queued reads the scratch arrays: drained before `tmp` gives them back, on the failing paths too)
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  HIPCHK(e);
  return 0;
}

// The filtered scanlines (zmx_png_rows.h).
int zmx_png_filter_rows_device(zmx_ctx* c, const void* d_image, size_t linebytes, size_t height, size_t bytewidth,
                               const void* d_types, void* d_out, size_t capacity) {
  const char* who = "zmx_png_filter_rows_device";
  g_png_rows_ms = 0;
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (height == 0) return 0;
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu, bytewidth)) return FailMsg(std::string(who) + ": bad geometry");
  const size_t total = height * (linebytes + 1);
  if (capacity < total) {
    return FailMsg(std::string(who) + ": the output takes " + std::to_string(total) + " bytes, the capacity is " + std::to_string(capacity));
  }
  int img_device = -1, types_device = -1, out_device = -1;
  if (const int rc = CheckDevicePointer(who, d_image, linebytes * height, &img_device)) return rc;
  if (const int rc = CheckDevicePointer(who, d_types, height, &types_device)) return rc;
  if (const int rc = CheckDevicePointer(who, d_out, total, &out_device)) return rc;
  if (img_device != c->device || types_device != c->device || out_device != c->device) {
    return FailMsg(std::string(who) + ": memory of another device than the context's");
  }
  if (RangesOverlap(d_out, total, d_image, linebytes * height)) return FailMsg(std::string(who) + ": the output overlaps the image");
  if (RangesOverlap(d_out, total, d_types, height)) return FailMsg(std::string(who) + ": the output overlaps the types");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  return PngRowsOnDevice(c, &tmp, who, static_cast<const u8*>(d_image), linebytes, height, bytewidth,
                         static_cast<const u8*>(d_types), static_cast<u8*>(d_out));
}

// zmx_png_encode_device's device part (host/png_encode.cc): the types of `strategy` — ZMX_PNG_FILTER_PREDEFINED: the
// `height` host bytes at `predefined`, checked by the caller — and the scanlines of d_image into d_out, a buffer of the
// caller's own of height * (linebytes + 1) bytes on the context's device.  The image is checked as the device entries
// check theirs.
int zmx_internal_png_scanlines(zmx_ctx* c, const void* d_image, size_t linebytes, size_t height, size_t bytewidth, int strategy,
                               unsigned windowsize, const unsigned char* predefined, void* d_out) {
  const char* who = "zmx_png_encode_device";
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu, bytewidth) || height == 0) return FailMsg(std::string(who) + ": bad geometry");
  int img_device = -1;
  if (const int rc = CheckDevicePointer(who, d_image, linebytes * height, &img_device)) return rc;
  if (img_device != c->device) return FailMsg(std::string(who) + ": the image is memory of another device than the context's");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  u8* d_types = nullptr;
  int rc = 0;
  if (strategy == ZMX_PNG_FILTER_PREDEFINED) {
    const hipError_t e = tmp.Upload(&d_types, predefined, height, "d_png_types");
    if (e != hipSuccess) rc = Fail("Upload(d_png_types)", e, __FILE__, __LINE__);
  } else {
    const hipError_t e = tmp.AllocT(&d_types, height, "d_png_types");
    if (e != hipSuccess) rc = Fail("AllocT(d_png_types)", e, __FILE__, __LINE__);
    else rc = PngTypesOnDevice(c, &tmp, who, static_cast<const u8*>(d_image), linebytes, height, bytewidth, strategy, windowsize, d_types);
  }
  if (rc == 0) {
    // (drains the stream whichever way it returns once the kernel is queued)
    rc = PngRowsOnDevice(c, &tmp, who, static_cast<const u8*>(d_image), linebytes, height, bytewidth, d_types, static_cast<u8*>(d_out));
  }
  if (rc != 0) (void)hipStreamSynchronize(c->stream);   // what was queued may still read `tmp`'s arrays
  return rc;
}
}  // extern "C"

// ---- index images: first appearances and the table-driven conversion (zmx_png_index.h)
static thread_local double g_png_index_ms[2] = {0, 0};   // k_png_index_use, k_png_index_convert (zmx_internal_png_index_ms)

// What every index entry refuses of an image before its pointer is looked at; *nbytes its size.
static int PngIndexImageOf(const char* who, const zmx_png_index_image* image, zamd::PngIndexImage* I, size_t* nbytes) {
  const std::string w(who);
  if (!image) return FailMsg(w + ": no image");
  if (image->width == 0 || image->height == 0) return FailMsg(w + ": width or height 0");
  const u32 ct = image->colortype, depth = image->bitdepth;
  const bool depth_ok = depth == 1 || depth == 2 || depth == 4 || (depth == 8 && ct == 3);
  if (!(ct == 0 || ct == 3) || !depth_ok) {
    return FailMsg(w + ": colour type " + std::to_string(ct) + " at " + std::to_string(depth) + " bits is no index image (3 at 1, 2, 4, 8; 0 at 1, 2, 4)");
  }
  if (ct == 3 && (image->palettesize == 0 || image->palettesize > (1u << depth))) {
    return FailMsg(w + ": a palette of " + std::to_string(image->palettesize) + " entries at " + std::to_string(depth) + " bits");
  }
  if (static_cast<u64>(image->width) * image->height > 0xffffffffull) return FailMsg(w + ": an image of 2^32 pixels or more");
  I->pixels = static_cast<const u8*>(image->d_pixels);
  I->linebytes = zamd::PngIndexLineBytes(image->width, depth);
  I->width = image->width;
  I->height = image->height;
  I->bitdepth = depth;
  if (!PngGeometryOk(I->linebytes, image->height, 0x7fffffffu, 1)) return FailMsg(w + ": bad geometry");
  *nbytes = static_cast<size_t>(I->linebytes * image->height);
  return 0;
}

// k_png_index_use on an image the caller has checked: the table read.  Drains the context's stream.
static int PngIndexUseOnDevice(zmx_ctx* c, PoolScope* tmp, const zamd::PngIndexImage& I, size_t nbytes, uint64_t* first) {
  u32* d_first = nullptr;
  HIPCHK(tmp->AllocT(&d_first, zamd::kPngIndexValues, "d_png_index_first"));
  HIPCHK(hipMemsetAsync(d_first, 0xff, zamd::kPngIndexValues * sizeof(u32), c->stream));
  PngLossyTimer timer{c, KernelTiming()};
  HIPCHK(timer.Begin());
  hipLaunchKernelGGL(k_png_index_use, dim3(zamd::PngIndexGrid(nbytes)), dim3(zamd::kPngIndexThreads), 0, c->stream, I, d_first);
  KCHK(c, "k_png_index_use");
  HIPCHK(timer.End(&g_png_index_ms[0]));
  u32 got[zamd::kPngIndexValues];
  HIPCHK(hipMemcpyAsync(got, d_first, sizeof(got), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (u32 v = 0; v < zamd::kPngIndexValues; ++v) first[v] = got[v] == zamd::kPngIndexNone ? UINT64_MAX : got[v];
  return 0;
}

// k_png_index_convert, the caller having checked everything: the image through `table` into d_out in the output mode.
// Drains the context's stream.
static int PngIndexConvertOnDevice(zmx_ctx* c, PoolScope* tmp, const char* who, const zamd::PngIndexImage& I, u32 palettesize,
                                   const zmx_png_color_mode& mode, const uint32_t* table, u8* d_out) {
  u32* d_bad = nullptr;
  u32* d_table = nullptr;
  HIPCHK(tmp->AllocT(&d_bad, 1, "d_png_bad_pixel"));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, sizeof(u32), c->stream));
  HIPCHK(tmp->Upload(&d_table, table, zamd::kPngIndexValues, "d_png_index_table"));
  zamd::PngIndexConvParams P;
  P.in = I;
  P.out = d_out;
  P.rowbytes = zamd::PngConvRowBytes(I.width, mode.colortype, mode.bitdepth);
  P.colortype = mode.colortype;
  P.bitdepth = mode.bitdepth;
  P.palettesize = palettesize;
  P.table = d_table;
  P.bad_pixel = d_bad;
  PngLossyTimer timer{c, KernelTiming()};
  HIPCHK(timer.Begin());
  hipLaunchKernelGGL(k_png_index_convert, dim3(zamd::PngIndexGrid(P.rowbytes * I.height)), dim3(zamd::kPngIndexThreads), 0, c->stream, P);
  KCHK(c, "k_png_index_convert");
  HIPCHK(timer.End(&g_png_index_ms[1]));
  u32 bad = zamd::kPngIndexNone;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (bad != zamd::kPngIndexNone) return FailMsg(std::string(who) + ": pixel " + std::to_string(bad) + " has a value outside the palette");
  return 0;
}

extern "C" {
void zmx_internal_png_index_ms(double out[2]) {
  for (int k = 0; k < 2; ++k) out[k] = g_png_index_ms[k];
}

int zmx_png_index_use_device(zmx_ctx* c, const zmx_png_index_image* image, uint64_t first[256]) {
  const char* who = "zmx_png_index_use_device";
  g_png_index_ms[0] = 0;
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (!first) return FailMsg(std::string(who) + ": no output");
  zamd::PngIndexImage I;
  size_t nbytes = 0;
  if (const int rc = PngIndexImageOf(who, image, &I, &nbytes)) return rc;
  int img_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (img_device != c->device) return FailMsg(std::string(who) + ": memory of another device than the context's");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  uint64_t got[zamd::kPngIndexValues];
  const int rc = PngIndexUseOnDevice(c, &tmp, I, nbytes, got);
  if (rc != 0) {
    (void)hipStreamSynchronize(c->stream);   // what was queued may still use `tmp`'s arrays
    return rc;
  }
  std::copy(got, got + zamd::kPngIndexValues, first);
  return 0;
}

int zmx_png_index_convert_device(zmx_ctx* c, const zmx_png_index_image* image, const zmx_png_color_mode* mode, const uint32_t table[256],
                                 void* d_out, size_t capacity) {
  const char* who = "zmx_png_index_convert_device";
  g_png_index_ms[1] = 0;
  if (!c) return FailMsg(std::string(who) + ": no context");
  if (!mode || !table) return FailMsg(std::string(who) + ": no mode or no table");
  zamd::PngIndexImage I;
  size_t nbytes = 0;
  if (const int rc = PngIndexImageOf(who, image, &I, &nbytes)) return rc;
  if (!zamd::PngIndexOutModeOk(mode->colortype, mode->bitdepth)) {
    return FailMsg(std::string(who) + ": colour type " + std::to_string(mode->colortype) + " at " + std::to_string(mode->bitdepth) +
                   " bits is no mode an index image converts to");
  }
  const u64 rowbytes = zamd::PngConvRowBytes(I.width, mode->colortype, mode->bitdepth);
  if (rowbytes > 0x7fffffffu) return FailMsg(std::string(who) + ": bad geometry");
  const size_t total = static_cast<size_t>(rowbytes * I.height);
  if (capacity < total) {
    return FailMsg(std::string(who) + ": the output takes " + std::to_string(total) + " bytes, the capacity is " + std::to_string(capacity));
  }
  int img_device = -1, out_device = -1;
  if (const int rc = CheckDevicePointer(who, image->d_pixels, nbytes, &img_device)) return rc;
  if (const int rc = CheckDevicePointer(who, d_out, total, &out_device)) return rc;
  if (img_device != c->device || out_device != c->device) return FailMsg(std::string(who) + ": memory of another device than the context's");
  if (RangesOverlap(d_out, total, image->d_pixels, nbytes)) return FailMsg(std::string(who) + ": the output overlaps the image");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  const u32 palettesize = image->colortype == 3 ? image->palettesize : 1u << image->bitdepth;
  const int rc = PngIndexConvertOnDevice(c, &tmp, who, I, palettesize, *mode, table, static_cast<u8*>(d_out));
  if (rc != 0) (void)hipStreamSynchronize(c->stream);
  return rc;
}
}  // extern "C"

// ---- LodePNG's zlib size of device buffers (zmx_png_lodeflate.h, host/png_lodeflate_size.h)
static thread_local double g_png_lo_ms[6] = {0, 0, 0, 0, 0, 0};   // k_png_lo_hash, _links, _ask, _keep, _search, _parse (zmx_internal_png_lodeflate_ms)

// What a test may take of a call besides the sizes (zmx_internal_png_lodeflate_arrays): host arrays, each null or of
// [positions] words — `counts` of [blocks][kLoCountWords] —, that receive the device's arrays as the kernels left them.
struct PngLoArrays {
  uint32_t* hc = nullptr;
  uint32_t* zc = nullptr;
  uint32_t* ld = nullptr;
  uint32_t* counts = nullptr;
};

// The six kernels over buffers the caller has checked, in tiles of `tile_len` positions (at most kLoTileLen); the counts
// read, the sizes made.  Drains the context's stream.
static int PngLoSizesOnDevice(zmx_ctx* c, PoolScope* tmp, size_t n, const void* const* d_in, const size_t* insize, unsigned windowsize,
                              uint32_t tile_len, uint64_t* zlib_bytes, const PngLoArrays& arrays = PngLoArrays()) {
  const zamd::LoPlan plan = zamd::LoMakePlan(n, d_in, insize, tile_len);
  const size_t ntiles = plan.tiles.size(), nblocks = plan.blocks.size();
  if (ntiles > 0x7fffffffu || nblocks > 0x7fffffffu) return FailMsg("zmx_png_deflate_sizes_device: too many tiles in one call");
  zamd::LoBuf* d_bufs = nullptr;
  zamd::LoTile* d_tiles = nullptr;
  zamd::LoTile* d_blocks = nullptr;
  zamd::LoParams P;
  HIPCHK(tmp->Upload(&d_bufs, plan.bufs.data(), n, "d_png_lo_bufs"));
  HIPCHK(tmp->Upload(&d_tiles, plan.tiles.data(), ntiles, "d_png_lo_tiles"));
  HIPCHK(tmp->Upload(&d_blocks, plan.blocks.data(), nblocks, "d_png_lo_blocks"));
  HIPCHK(tmp->AllocT(&P.HC, static_cast<size_t>(plan.positions), "d_png_lo_hc"));
  HIPCHK(tmp->AllocT(&P.ZC, static_cast<size_t>(plan.positions), "d_png_lo_zc"));
  HIPCHK(tmp->AllocT(&P.LD, static_cast<size_t>(plan.positions), "d_png_lo_ld"));
  HIPCHK(tmp->AllocT(&P.tables, ntiles * static_cast<size_t>(zamd::kLoTableLen), "d_png_lo_tables"));
  HIPCHK(tmp->AllocT(&P.counts, nblocks * static_cast<size_t>(zamd::kLoCountWords), "d_png_lo_counts"));
  P.bufs = d_bufs;
  P.tiles = d_tiles;
  P.blocks = d_blocks;
  P.window = windowsize;
  P.ntiles = static_cast<u32>(ntiles);
  P.nblocks = static_cast<u32>(nblocks);
  P.tile_len = tile_len;
  HIPCHK(hipMemsetAsync(P.tables, 0, ntiles * static_cast<size_t>(zamd::kLoTableLen) * sizeof(u32), c->stream));
  PngLossyTimer timer{c, KernelTiming()};
  const u32 gx = (plan.longest_tile + zamd::kLoThreads - 1) / zamd::kLoThreads;
  // a per-position kernel over all tiles, at most 65535 rows of workgroups a launch
#define PNG_LO_PER_POSITION(kernel, slot)                                                                                       \
  do {                                                                                                                           \
    HIPCHK(timer.Begin());                                                                                                       \
    for (size_t t0 = 0; t0 < ntiles; t0 += 65535) {                                                                              \
      const u32 rows = static_cast<u32>(std::min<size_t>(65535, ntiles - t0));                                                   \
      hipLaunchKernelGGL(kernel, dim3(gx, rows), dim3(zamd::kLoThreads), 0, c->stream, P, static_cast<u32>(t0));                 \
      KCHK(c, #kernel);                                                                                                          \
    }                                                                                                                            \
    HIPCHK(timer.End(&g_png_lo_ms[slot]));                                                                                       \
  } while (0)
  PNG_LO_PER_POSITION(k_png_lo_hash, 0);
  HIPCHK(timer.Begin());
  hipLaunchKernelGGL(k_png_lo_links, dim3(static_cast<u32>(ntiles)), dim3(zamd::kLoThreads), 0, c->stream, P);
  KCHK(c, "k_png_lo_links");
  HIPCHK(timer.End(&g_png_lo_ms[1]));
  PNG_LO_PER_POSITION(k_png_lo_ask, 2);
  PNG_LO_PER_POSITION(k_png_lo_keep, 3);
  PNG_LO_PER_POSITION(k_png_lo_search, 4);
#undef PNG_LO_PER_POSITION
  HIPCHK(timer.Begin());
  hipLaunchKernelGGL(k_png_lo_parse, dim3(static_cast<u32>(nblocks)), dim3(64), 0, c->stream, P);
  KCHK(c, "k_png_lo_parse");
  HIPCHK(timer.End(&g_png_lo_ms[5]));
  std::vector<u32> counts(nblocks * static_cast<size_t>(zamd::kLoCountWords));
  HIPCHK(hipMemcpyAsync(counts.data(), P.counts, counts.size() * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t words = static_cast<size_t>(plan.positions);
  if (arrays.hc) HIPCHK(hipMemcpy(arrays.hc, P.HC, words * sizeof(u32), hipMemcpyDeviceToHost));
  if (arrays.zc) HIPCHK(hipMemcpy(arrays.zc, P.ZC, words * sizeof(u32), hipMemcpyDeviceToHost));
  if (arrays.ld) HIPCHK(hipMemcpy(arrays.ld, P.LD, words * sizeof(u32), hipMemcpyDeviceToHost));
  if (arrays.counts) std::copy(counts.begin(), counts.end(), arrays.counts);
  std::vector<zamd::LoBlockCounts> blocks(nblocks);
  for (size_t b = 0; b < nblocks; ++b) {
    const u32* w = counts.data() + b * zamd::kLoCountWords;
    std::memcpy(blocks[b].ll, w, sizeof(blocks[b].ll));
    std::memcpy(blocks[b].d, w + zamd::kLoNumLl, sizeof(blocks[b].d));
    blocks[b].extra_bits = static_cast<uint64_t>(w[316]) | (static_cast<uint64_t>(w[317]) << 32);
  }
  for (size_t i = 0; i < n; ++i) {
    zlib_bytes[i] = zamd::LoZlibBytes(blocks.data() + plan.first_block[i], plan.first_block[i + 1] - plan.first_block[i]);
  }
  return 0;
}

extern "C" {
void zmx_internal_png_lodeflate_ms(double out[6]) {
  for (int k = 0; k < 6; ++k) out[k] = g_png_lo_ms[k];
}

// The checks of a call's arguments, before anything runs; 0, or the refusal.
static int PngLoCheckCall(const char* who, zmx_ctx* c, size_t n, const void* const* d_in, const size_t* insize, unsigned windowsize,
                          const uint64_t* zlib_bytes) {
  const std::string w(who);
  if (!c) return FailMsg(w + ": no context");
  if (n == 0 || !d_in || !insize || !zlib_bytes) return FailMsg(w + ": a null argument or no buffer");
  if (!PngWindowOk(windowsize)) return FailMsg(w + ": the window must be a power of two of at most 32768");
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (insize[i] == 0) return FailMsg(w + ": buffer " + std::to_string(i) + " has no bytes");
    if (!d_in[i]) return FailMsg(w + ": buffer " + std::to_string(i) + " is a null pointer");
    total += insize[i];
    if (total > (1ull << 40)) return FailMsg(w + ": more than 2^40 bytes in one call");
  }
  for (size_t i = 0; i < n; ++i) {
    int device = -1;
    if (const int rc = CheckDevicePointer(who, d_in[i], insize[i], &device)) return rc;
    if (device != c->device) return FailMsg(w + ": memory of another device than the context's");
  }
  return 0;
}

// A checked call: the kernels, the stream drained, the sizes handed over when all went well.
static int PngLoCheckedCall(zmx_ctx* c, size_t n, const void* const* d_in, const size_t* insize, unsigned windowsize, uint32_t tile_len,
                            uint64_t* zlib_bytes, const PngLoArrays& arrays) {
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  std::vector<uint64_t> sizes(n);
  const int rc = PngLoSizesOnDevice(c, &tmp, n, d_in, insize, windowsize, tile_len, sizes.data(), arrays);
  // (what was queued uses the scratch arrays: drained before `tmp` gives them back, on the failing paths too)
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  HIPCHK(e);
  std::copy(sizes.begin(), sizes.end(), zlib_bytes);
  return 0;
}

int zmx_png_deflate_sizes_device(zmx_ctx* c, size_t n, const void* const* d_in, const size_t* insize, unsigned windowsize,
                                 uint64_t* zlib_bytes) {
  for (double& ms : g_png_lo_ms) ms = 0;
  if (const int rc = PngLoCheckCall("zmx_png_deflate_sizes_device", c, n, d_in, insize, windowsize, zlib_bytes)) return rc;
  return PngLoCheckedCall(c, n, d_in, insize, windowsize, zamd::kLoTileLen, zlib_bytes, PngLoArrays());
}

int zmx_internal_png_lodeflate_arrays(zmx_ctx* c, size_t n, const void* const* d_in, const size_t* insize, unsigned windowsize,
                                      unsigned tile_len, uint32_t* hc, uint32_t* zc, uint32_t* ld, uint32_t* counts, uint64_t* zlib_bytes) {
  const char* who = "zmx_internal_png_lodeflate_arrays";
  const std::string w(who);
  for (double& ms : g_png_lo_ms) ms = 0;
  if (const int rc = PngLoCheckCall(who, c, n, d_in, insize, windowsize, zlib_bytes)) return rc;
  if (tile_len == 0) tile_len = zamd::kLoTileLen;
  if (tile_len > zamd::kLoTileLen) return FailMsg(w + ": a tile of more than " + std::to_string(zamd::kLoTileLen) + " positions");
  uint64_t ntiles = 0;
  for (size_t i = 0; i < n; ++i) ntiles += (insize[i] + tile_len - 1) / tile_len;
  if (ntiles > 1024) return FailMsg(w + ": " + std::to_string(ntiles) + " tiles, more than 1024 (a tile's head table is 263 KB)");
  PngLoArrays arrays;
  arrays.hc = hc;
  arrays.zc = zc;
  arrays.ld = ld;
  arrays.counts = counts;
  return PngLoCheckedCall(c, n, d_in, insize, windowsize, tile_len, zlib_bytes, arrays);
}

// zmx_png_choose_strategy_device's device part (host/png_encode.cc): the rows of trial k = 0 .. ntrials - 1 of an image
// that lies converted at d_rows — `height` rows of `rowbytes` bytes — at d_out + k * height * (rowbytes + 1), in zopflipng's
// order: the types 0 .. 4, MINSUM, ENTROPY, and for ntrials = 8 the `height` host bytes at `predefined` (checked by the
// caller).  d_out is a buffer of the caller's own on the context's device.  The rows are checked as the device entries
// check an image.
int zmx_internal_png_trial_scanlines(zmx_ctx* c, const char* who, const void* d_rows, size_t rowbytes, size_t height, size_t bytewidth,
                                     const unsigned char* predefined, int ntrials, void* d_out) {
  if (!PngGeometryOk(rowbytes, height, 0x7fffffffu, bytewidth) || height == 0) return FailMsg(std::string(who) + ": bad geometry");
  int img_device = -1;
  if (const int rc = CheckDevicePointer(who, d_rows, rowbytes * height, &img_device)) return rc;
  if (img_device != c->device) return FailMsg(std::string(who) + ": the image is memory of another device than the context's");
  const size_t scanlines = height * (rowbytes + 1);
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  const u8* d_img = static_cast<const u8*>(d_rows);
  int rc = 0;
  u8* d_types = nullptr;
  {
    const hipError_t e = tmp.AllocT(&d_types, height, "d_png_types");
    if (e != hipSuccess) rc = Fail("AllocT(d_png_types)", e, __FILE__, __LINE__);
  }
  for (int k = 0; rc == 0 && k < ntrials; ++k) {
    if (k == 7) {
      const hipError_t e = hipMemcpyAsync(d_types, predefined, height, hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) rc = Fail("hipMemcpyAsync(d_png_types)", e, __FILE__, __LINE__);
    } else {
      rc = PngTypesOnDevice(c, &tmp, who, d_img, rowbytes, height, bytewidth, k, 0, d_types);
    }
    // (drains the stream whichever way it returns once the kernel is queued: d_types is free for the next trial)
    if (rc == 0) rc = PngRowsOnDevice(c, &tmp, who, d_img, rowbytes, height, bytewidth, d_types,
                                      static_cast<u8*>(d_out) + static_cast<size_t>(k) * scanlines);
  }
  if (rc != 0) (void)hipStreamSynchronize(c->stream);
  return rc;
}
}  // extern "C"
