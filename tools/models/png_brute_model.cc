// Model (CPU) of the parallel formulation k_png_brute (zmx_png_brute.h) uses for LodePNG's LFS_BRUTE_FORCE row search
// (lodepng.cpp:5585-5632): the zlib size of one filtered scanline under LodePNG's fixed-tree deflate (encodeLZ77,
// :1593-1740), computed as
//   1. per position p: the hash H[p] (getHash, :1544-1561) and the zero count Z[p] (countZeros where H[p] == 0, else 0);
//   2. per position p: the value C[p] that inserting p writes into chain[p & M] — the slot of the last q < p with the
//      same hash, or, when there is none, what the slot already held (C[p - W], or the slot itself when p < W); the same
//      CZ[p] for chainz under the key Z;
//   3. per position, independently: LodePNG's match search with the state "positions 0..pos inserted", where slot s
//      holds what its latest position pos - ((pos - s) & M) wrote (the initial state when that is below 0);
//   4. one serial lazy-matching scan over the (length, offset) results, summing fixed-code bits (:2029-2072).
// against LodePNG's own lodepng_zlib_compress (btype 1) on the same bytes, and against filter() with LFS_BRUTE_FORCE.
// lodepng.cpp is compiled in from wherever it lies (nothing copied):
//   g++ -O2 -std=c++17 -I $LODEPNG_DIR tools/models/png_brute_model.cc -o /tmp/png_brute_model && /tmp/png_brute_model
#include "lodepng.cpp"

#include <cstdio>
#include <random>
#include <vector>

namespace {

const unsigned kKeep = 0xffffu;

unsigned HashAt(const unsigned char* f, size_t n, size_t p) {
  if (p + 2 < n) return (f[p] ^ (f[p + 1] << 4u) ^ (f[p + 2] << 8u)) & 65535u;
  unsigned r = 0;
  for (size_t i = 0; p + i < n; ++i) r ^= static_cast<unsigned>(f[p + i]) << (8u * i);
  return r & 65535u;
}

unsigned LengthExtra(unsigned l) { return (l <= 10 || l == 258) ? 0 : (31 - __builtin_clz(l - 3)) - 2; }
unsigned DistExtra(unsigned d) { return d <= 4 ? 0 : (31 - __builtin_clz(d - 1)) - 1; }
unsigned LitBits(unsigned c) { return c < 144 ? 8 : 9; }

size_t ModelSize(const unsigned char* f, size_t n, unsigned W) {
  const unsigned M = W - 1, maxchain = W >= 8192 ? W : W / 8, maxlazy = W >= 8192 ? 258 : 64, nice = 128;
  std::vector<unsigned> H(n), Z(n), C(n), CZ(n), L(n), D(n);
  // 1. hash and zero count (the zero runs from their starts, then masked by H == 0)
  for (size_t p = 0; p < n; ++p) H[p] = HashAt(f, n, p);
  for (size_t p = 0; p < n; ++p) {
    size_t e = p;
    while (e < n && e - p < 258 && f[e] == 0) ++e;
    Z[p] = H[p] == 0 ? static_cast<unsigned>(e - p) : 0;
  }
  // 2. the chain links: last earlier position with the same key, else KEEP, resolved per residue class
  std::vector<long> head(65536, -1), headz(259, -1);
  for (size_t p = 0; p < n; ++p) {
    C[p] = head[H[p]] >= 0 ? static_cast<unsigned>(head[H[p]]) & M : kKeep;
    CZ[p] = headz[Z[p]] >= 0 ? static_cast<unsigned>(headz[Z[p]]) & M : kKeep;
    head[H[p]] = static_cast<long>(p);
    headz[Z[p]] = static_cast<long>(p);
  }
  for (size_t r = 0; r < n && r < W; ++r) {
    unsigned pc = static_cast<unsigned>(r), pz = static_cast<unsigned>(r);
    for (size_t p = r; p < n; p += W) {
      if (C[p] == kKeep) C[p] = pc;
      if (CZ[p] == kKeep) CZ[p] = pz;
      pc = C[p];
      pz = CZ[p];
    }
  }
  // 3. the search at every position on its own
  for (size_t pos = 0; pos < n; ++pos) {
    const unsigned wpos = static_cast<unsigned>(pos) & M, hv = H[pos], nz = Z[pos];
    const size_t last = n < pos + 258 ? n : pos + 258;
    auto at = [&](unsigned s) { return static_cast<long>(pos) - static_cast<long>((wpos - s) & M); };  // slot's owner
    unsigned length = 0, offset = 0, hashpos = C[pos], prev_offset = 0, chainlength = 0;
    for (;;) {
      if (chainlength++ >= maxchain) break;
      const unsigned cur = hashpos <= wpos ? wpos - hashpos : wpos - hashpos + W;
      if (cur < prev_offset) break;
      prev_offset = cur;
      const long q = at(hashpos);
      if (cur > 0) {
        size_t fo = pos, ba = pos - cur;
        if (nz >= 3) {
          unsigned skip = Z[q];
          if (skip > nz) skip = nz;
          fo += skip;
          ba += skip;
        }
        while (fo != last && f[ba] == f[fo]) { ++fo; ++ba; }
        const unsigned cl = static_cast<unsigned>(fo - pos);
        if (cl > length) {
          length = cl;
          offset = cur;
          if (cl >= nice) break;
        }
      }
      const unsigned chainv = q >= 0 ? C[q] : hashpos;
      if (hashpos == chainv) break;
      if (nz >= 3 && length > nz) {
        hashpos = q >= 0 ? CZ[q] : hashpos;
        const long q2 = at(hashpos);
        if (q2 < 0 || Z[q2] != nz) break;
      } else {
        hashpos = chainv;
        const long q2 = at(hashpos);
        if (q2 < 0 || H[q2] != hv) break;
      }
    }
    L[pos] = length;
    D[pos] = offset;
  }
  // 4. the lazy scan
  size_t bits = 3 + 7;
  unsigned lazy = 0, ll = 0, lo = 0;
  for (size_t pos = 0; pos < n; ++pos) {
    unsigned length = L[pos], offset = D[pos];
    if (!lazy && length >= 3 && length <= maxlazy && length < 258) { lazy = 1; ll = length; lo = offset; continue; }
    if (lazy) {
      lazy = 0;
      if (length > ll + 1) bits += LitBits(f[pos - 1]);
      else { length = ll; offset = lo; --pos; }
    }
    if (length < 3 || (length == 3 && offset > 4096)) bits += LitBits(f[pos]);
    else {
      bits += (length <= 114 ? 7 : 8) + LengthExtra(length) + 5 + DistExtra(offset);
      pos += length - 1;
    }
  }
  return 6 + (bits + 7) / 8;
}

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
