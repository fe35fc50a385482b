// Driver part: LodePNG's filter choices on the device (zmx_png.h, zmx_png_brute.h).  Holds
// zmx_png_filter_types and zmx_png_filter_types_brute.  Needs drv_context.h (zmx_ctx, PoolScope).
#pragma once

extern "C" {
// an image the kernels can index with 32 bits: rows of `linebytes`, at most `max_height` of them, pixels of 1 .. 8 bytes
static bool PngGeometryOk(size_t linebytes, size_t height, size_t max_height, size_t bytewidth) {
  return linebytes != 0 && bytewidth != 0 && linebytes <= 0x7fffffffu && height <= max_height && bytewidth <= 8;
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
  PngFilterParams pp;
  pp.image = d_img;
  pp.linebytes = static_cast<u32>(linebytes);
  pp.height = static_cast<u32>(height);
  pp.bytewidth = static_cast<u32>(bytewidth);
  pp.minsum = minsum_types ? d_types : nullptr;
  pp.entropy = entropy_types ? d_types + height : nullptr;
  hipLaunchKernelGGL(k_png_filter_types, dim3(static_cast<unsigned>(height)), dim3(PNGF_THREADS), 0, c->stream, pp);
  KCHK(c, "k_png_filter_types");
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
  if (windowsize == 0 || windowsize > 32768u || (windowsize & (windowsize - 1u)) != 0) {   // LodePNG's errors 60 / 90
    return FailMsg("zmx_png_filter_types_brute: the window must be a power of two of at most 32768");
  }
  if (height == 0) return 0;
  if (!types) return FailMsg("zmx_png_filter_types_brute: no output");
  if (!PngGeometryOk(linebytes, height, 0x7fffffffu / 5u, bytewidth)) return FailMsg("zmx_png_filter_types_brute: bad geometry");
  DEVICE_ENTRY(c->device);
  const u32 n = static_cast<u32>(linebytes), jobs = static_cast<u32>(5 * height);
  // the per-position arrays in the dynamic LDS when they fit, else in the scratch beside the head table and the results
  const u64 row_bytes = pngb_row_bytes(n);
  const bool in_lds = row_bytes <= PNGB_LDS_MAX;
  const u64 stride = (PNGB_HEAD_BYTES + 4ull * n + (in_lds ? 0 : row_bytes) + 255u) & ~255ull;
  // two 1024-lane workgroups fill a CU's 32 waves; the LDS may allow fewer
  const u64 per_cu = in_lds ? std::max<u64>(1, std::min<u64>(2, (160u * 1024u) / (row_bytes + 12u * 1024u))) : 1;
  const u64 budget = 1ull << 30;
  const u32 grid = static_cast<u32>(std::max<u64>(1, std::min<u64>({static_cast<u64>(jobs), 256 * per_cu, budget / stride})));
  if (in_lds && row_bytes > 64u * 1024u) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_png_brute), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(PNGB_LDS_MAX)));
  }
  PoolScope tmp(c);
  u8* d_img = nullptr;
  u8* d_scratch = nullptr;
  u8* d_types = nullptr;
  u64* d_sizes = nullptr;
  HIPCHK(tmp.Upload(&d_img, image, linebytes * height, "d_png_image"));
  HIPCHK(tmp.AllocT(&d_scratch, static_cast<size_t>(stride) * grid, "d_png_brute_scratch"));
  HIPCHK(tmp.AllocT(&d_sizes, static_cast<size_t>(jobs), "d_png_brute_sizes"));
  HIPCHK(tmp.AllocT(&d_types, height, "d_png_types"));
  PngBruteParams pp;
  pp.image = d_img;
  pp.linebytes = n;
  pp.height = static_cast<u32>(height);
  pp.bytewidth = static_cast<u32>(bytewidth);
  pp.window = windowsize;
  pp.jobs = jobs;
  pp.scratch = d_scratch;
  pp.scratch_stride = stride;
  pp.in_lds = in_lds ? 1u : 0u;
  pp.sizes = d_sizes;
  hipLaunchKernelGGL(k_png_brute, dim3(grid), dim3(PNGB_THREADS), in_lds ? static_cast<unsigned>(row_bytes) : 0u, c->stream, pp);
  KCHK(c, "k_png_brute");
  hipLaunchKernelGGL(k_png_brute_pick, dim3(static_cast<unsigned>((height + 255) / 256)), dim3(256), 0, c->stream,
                     static_cast<const u64*>(d_sizes), static_cast<u32>(height), d_types);
  KCHK(c, "k_png_brute_pick");
  HIPCHK(hipMemcpyAsync(types, d_types, height, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
}  // extern "C"
