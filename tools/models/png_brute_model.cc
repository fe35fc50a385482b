// The model of k_png_brute's parallel formulation (png_brute_model.h beside this file, which states it) against LodePNG's
// own lodepng_zlib_compress (btype 1) on the same bytes, and against filter() with LFS_BRUTE_FORCE.
// lodepng.cpp is compiled in from wherever it lies (nothing copied):
//   g++ -O2 -std=c++17 -I $LODEPNG_DIR tools/models/png_brute_model.cc -o /tmp/png_brute_model && /tmp/png_brute_model
#include "lodepng.cpp"

#include <cstdio>
#include <random>
#include <vector>

#include "png_brute_model.h"

namespace {

size_t ModelSize(const unsigned char* f, size_t n, unsigned W) { return png_brute_model::ModelSize(f, n, W).bytes; }

size_t LodeSize(const unsigned char* f, size_t n, unsigned W) {
  LodePNGCompressSettings s;
  lodepng_compress_settings_init(&s);
  s.btype = 1;
  s.windowsize = W;
  unsigned char* out = nullptr;
  size_t size = 0;
  if (lodepng_zlib_compress(&out, &size, f, n, &s) != 0) size = 0;
  free(out);
  return size;
}

std::vector<unsigned char> Row(std::mt19937& g, int kind, size_t n) {
  std::vector<unsigned char> r(n);
  auto u = [&](unsigned m) { return static_cast<unsigned>(g() % m); };
  switch (kind) {
    case 0: for (auto& b : r) b = u(256); break;                                   // random
    case 1: for (auto& b : r) b = u(8) ? 0 : u(256); break;                        // zero-heavy
    case 2: {                                                                      // long zero runs
      size_t i = 0;
      while (i < n) { const size_t run = u(600); for (size_t k = 0; k < run && i < n; ++k) r[i++] = 0; if (i < n) r[i++] = u(256); }
      break;
    }
    case 3: { const size_t per = 1 + u(40); for (size_t i = 0; i < n; ++i) r[i] = (i % per) * 37 & 255; if (n) r[u(n)] ^= 1; break; }   // periodic
    case 4: for (size_t i = 0; i < n; ++i) r[i] = (i % 3 == 0) ? 0x10 : (i % 3 == 1) ? 0x01 : 0x00; break;   // non-zero, hash 0
    case 5: { for (auto& b : r) b = u(256); for (size_t i = 0; i + 5000 < n; i += 997) { r[i + 5000] = r[i]; r[i + 5001] = r[i + 1]; r[i + 5002] = r[i + 2]; } break; }  // far 3-byte matches
    case 6: for (auto& b : r) b = u(50) ? 17 : u(256); break;                      // flat
    default: for (size_t i = 0; i < n; ++i) r[i] = static_cast<unsigned char>((i / 4) * 3 + u(7) - 3); break;  // gradient with noise
  }
  return r;
}

}  // namespace

int main() {
  std::mt19937 g(12345);
  const unsigned windows[] = {1, 2, 16, 64, 256, 2048, 32768};
  const size_t lens[] = {1, 2, 3, 4, 5, 17, 255, 256, 257, 300, 1000, 2049, 4096, 9000, 16384, 40000, 70000};
  size_t rows = 0, bad = 0;
  for (unsigned W : windows)
    for (size_t n : lens)
      for (int kind = 0; kind < 8; ++kind) {
        if (n > 20000 && W < 256 && kind != 2) continue;   // (long rows on tiny windows: a few kinds are enough)
        const std::vector<unsigned char> r = Row(g, kind, n);
        const size_t a = ModelSize(r.data(), n, W), b = LodeSize(r.data(), n, W);
        ++rows;
        if (a != b) { ++bad; printf("MISMATCH W=%u n=%zu kind=%d model=%zu lodepng=%zu\n", W, n, kind, a, b); }
      }
  // whole images: the chosen type per row against filter() with LFS_BRUTE_FORCE (window 2048, LodePNG's default)
  size_t img_rows = 0, img_bad = 0;
  for (int kind = 0; kind < 8; ++kind) {
    const unsigned w = 300 + 97 * kind, h = 24, bytewidth = 4, linebytes = w * 4;
    std::vector<unsigned char> raw;
    for (unsigned y = 0; y < h; ++y) { auto r = Row(g, kind, linebytes); raw.insert(raw.end(), r.begin(), r.end()); }
    LodePNGColorMode mode;
    lodepng_color_mode_init(&mode);
    mode.colortype = LCT_RGBA;
    mode.bitdepth = 8;
    LodePNGEncoderSettings es;
    lodepng_encoder_settings_init(&es);
    es.filter_palette_zero = 0;
    es.filter_strategy = LFS_BRUTE_FORCE;
    std::vector<unsigned char> out(h * (linebytes + 1));
    if (filter(out.data(), raw.data(), w, h, &mode, &es) != 0) { printf("filter() failed\n"); return 2; }
    std::vector<unsigned char> att(linebytes);
    for (unsigned y = 0; y < h; ++y) {
      unsigned best = 0;
      size_t smallest = 0;
      for (unsigned t = 0; t < 5; ++t) {
        filterScanline(att.data(), &raw[y * linebytes], y ? &raw[(y - 1) * linebytes] : nullptr, linebytes, bytewidth, t);
        const size_t s = ModelSize(att.data(), linebytes, 2048);
        if (t == 0 || s < smallest) { best = t; smallest = s; }
      }
      ++img_rows;
      if (best != out[y * (linebytes + 1)]) { ++img_bad; printf("TYPE MISMATCH kind=%d y=%u model=%u lodepng=%u\n", kind, y, best, out[y * (linebytes + 1)]); }
    }
  }
  printf("%zu rows against lodepng_zlib_compress: %zu differ; %zu image rows against filter(LFS_BRUTE_FORCE): %zu differ\n",
         rows, bad, img_rows, img_bad);
  return bad || img_bad ? 1 : 0;
}
