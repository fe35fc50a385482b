// Model (CPU) of zmx_png_deflate_sizes_device: the length lodepng_zlib_compress returns for a buffer under LodePNG's
// default settings (btype 2, lazy matching, minmatch 3, nicematch 128) at a given window, computed the way the kernels of
// zopfli_amd/csrc/device/zmx_png_lodeflate.h compute it and then sized by zopfli_amd/csrc/host/png_lodeflate_size.h:
//   1. the deflate blocks of lodepng_deflatev (blocksize = insize / 8 + 8 within [65536, 262144]); every position knows
//      the end of its block;
//   2. per position p: H[p] (getHash with the block's end as `size`: the short form in a block's last two positions) and
//      Z[p] (the zero run from p, capped at 258 and at the block's end, where H[p] == 0; else 0);
//   3. per position p: C[p], the slot of the last q < p of the WHOLE buffer with H[q] == H[p] (the Hash is initialised
//      once per buffer), else what the slot held — C[p - W], or the slot itself; the same CZ[p] under the key Z;
//   4. per position, independently: LodePNG's search on the state "0..pos inserted", a match ending at the block's end;
//   5. per block, serially: the lazy parse (lazy state 0 at every block's start) into 286 + 30 counts and the extra bits;
//   6. LoDynamicBlockBits per block, the blocks' bits end to end.
// It is held against LodePNG's own lodepng_zlib_compress.  lodepng.cpp is compiled in from wherever it lies:
//   g++ -O2 -std=c++17 -I $LODEPNG_DIR -I zopfli_amd/csrc/host tools/models/png_lodeflate_model.cc -o png_lodeflate_model
//   png_lodeflate_model                      the fuzz; prints its counts, exit status 1 on any difference
//   png_lodeflate_model size FILE WINDOW     prints "<lodepng bytes> <model bytes>" for the bytes of FILE
//   png_lodeflate_model huff FILE            the same with use_lz77 0: a block's counts are then its bytes' counts, which
//                                            puts a chosen histogram of literals before deflateDynamic's trees
#include "lodepng.cpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "png_lodeflate_size.h"

namespace {

const unsigned kKeep = 0xffffu;

unsigned Log2(unsigned v) { return 31u - static_cast<unsigned>(__builtin_clz(v)); }
unsigned LengthExtra(unsigned l) { return (l <= 10 || l == 258) ? 0 : Log2(l - 3) - 2; }
unsigned LengthSymbol(unsigned l) { return l == 258 ? 285 : 257 + 4 * LengthExtra(l) + ((l - 3) >> LengthExtra(l)); }
unsigned DistExtra(unsigned d) { return d <= 4 ? 0 : Log2(d - 1) - 1; }
unsigned DistSymbol(unsigned d) { return 2 * DistExtra(d) + ((d - 1) >> DistExtra(d)); }

void ModelCounts(const unsigned char* f, size_t n, unsigned W, std::vector<zamd::LoBlockCounts>* blocks) {
  const unsigned M = W - 1, maxchain = W >= 8192 ? W : W / 8, maxlazy = W >= 8192 ? 258 : 64, nice = 128;
  const size_t bs = zamd::LoBlockSize(n), nb = zamd::LoNumBlocks(n);
  auto end_of = [&](size_t p) { const size_t e = (p / bs + 1) * bs; return e < n ? e : n; };
  std::vector<unsigned> H(n), Z(n), C(n), CZ(n), L(n), D(n);
  for (size_t p = 0; p < n; ++p) {
    const size_t e = end_of(p);
    unsigned h = 0;
    if (p + 2 < e) h = f[p] ^ (f[p + 1] << 4u) ^ (f[p + 2] << 8u);
    else for (size_t i = 0; p + i < e; ++i) h ^= static_cast<unsigned>(f[p + i]) << (8u * i);
    H[p] = h & 65535u;
    size_t z = p;
    while (z < e && z - p < 258 && f[z] == 0) ++z;
    Z[p] = H[p] == 0 ? static_cast<unsigned>(z - p) : 0;
  }
  std::vector<long> head(65536, -1), headz(259, -1);
  for (size_t p = 0; p < n; ++p) {
    C[p] = head[H[p]] >= 0 ? static_cast<unsigned>(head[H[p]]) & M : kKeep;
    CZ[p] = headz[Z[p]] >= 0 ? static_cast<unsigned>(headz[Z[p]]) & M : kKeep;
    head[H[p]] = static_cast<long>(p);
    headz[Z[p]] = static_cast<long>(p);
  }
  for (size_t p = 0; p < n; ++p) {
    if (C[p] == kKeep) C[p] = p >= W ? C[p - W] : static_cast<unsigned>(p);
    if (CZ[p] == kKeep) CZ[p] = p >= W ? CZ[p - W] : static_cast<unsigned>(p);
  }
  for (size_t pos = 0; pos < n; ++pos) {
    const unsigned wpos = static_cast<unsigned>(pos) & M, hv = H[pos], nz = Z[pos];
    const size_t e = end_of(pos), last = e < pos + 258 ? e : pos + 258;
    auto at = [&](unsigned s) { return static_cast<long>(pos) - static_cast<long>((wpos - s) & M); };
    unsigned length = 0, offset = 0, hashpos = C[pos], prev_offset = 0, chainlength = 0;
    for (;;) {
      if (chainlength++ >= maxchain) break;
      const unsigned cur = hashpos <= wpos ? wpos - hashpos : wpos - hashpos + W;
      if (cur < prev_offset) break;
      prev_offset = cur;
      const long q = at(hashpos);
      if (cur > 0) {
        if (q < 0) break;   // (a slot nothing has written: LodePNG reaches those only as chain[i] == i)
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
  blocks->assign(nb, zamd::LoBlockCounts());
  for (size_t b = 0; b < nb; ++b) {
    zamd::LoBlockCounts& out = (*blocks)[b];
    const size_t s = b * bs, e = end_of(s);
    unsigned lazy = 0, ll = 0, lo = 0;
    for (size_t pos = s; pos < e; ++pos) {
      unsigned length = L[pos], offset = D[pos];
      if (!lazy && length >= 3 && length <= maxlazy && length < 258) { lazy = 1; ll = length; lo = offset; continue; }
      if (lazy) {
        lazy = 0;
        if (length > ll + 1) ++out.ll[f[pos - 1]];
        else { length = ll; offset = lo; --pos; }
      }
      if (length < 3 || (length == 3 && offset > 4096)) ++out.ll[f[pos]];
      else {
        ++out.ll[LengthSymbol(length)];
        ++out.d[DistSymbol(offset)];
        out.extra_bits += LengthExtra(length) + DistExtra(offset);
        pos += length - 1;
      }
    }
  }
}

size_t ModelSize(const unsigned char* f, size_t n, unsigned W) {
  std::vector<zamd::LoBlockCounts> blocks;
  ModelCounts(f, n, W, &blocks);
  return static_cast<size_t>(zamd::LoZlibBytes(blocks.data(), blocks.size()));
}

size_t LodeSize(const unsigned char* f, size_t n, unsigned W) {
  LodePNGCompressSettings s;
  lodepng_compress_settings_init(&s);
  s.windowsize = W;
  unsigned char* out = nullptr;
  size_t size = 0;
  if (lodepng_zlib_compress(&out, &size, f, n, &s) != 0) size = 0;
  free(out);
  return size;
}

// LodePNG's length when it only Huffman-codes the bytes (use_lz77 0): every block's counts are its bytes' counts, so
// a histogram of literals can be put before deflateDynamic's trees as it stands
size_t LodeHuffSize(const unsigned char* f, size_t n) {
  LodePNGCompressSettings s;
  lodepng_compress_settings_init(&s);
  s.use_lz77 = 0;
  unsigned char* out = nullptr;
  size_t size = 0;
  if (lodepng_zlib_compress(&out, &size, f, n, &s) != 0) size = 0;
  free(out);
  return size;
}

size_t ModelHuffSize(const unsigned char* f, size_t n) {
  const size_t bs = zamd::LoBlockSize(n), nb = zamd::LoNumBlocks(n);
  std::vector<zamd::LoBlockCounts> blocks(nb, zamd::LoBlockCounts());
  for (size_t p = 0; p < n; ++p) ++blocks[p / bs].ll[f[p]];
  return static_cast<size_t>(zamd::LoZlibBytes(blocks.data(), nb));
}

std::vector<unsigned char> Data(std::mt19937& g, int kind, size_t n, unsigned W) {
  std::vector<unsigned char> r(n);
  auto u = [&](unsigned m) { return static_cast<unsigned>(g() % m); };
  switch (kind) {
    case 0: for (auto& b : r) b = u(256); break;                                   // random
    case 1: for (auto& b : r) b = u(8) ? 0 : u(256); break;                        // zero-heavy
    case 2: {                                                                      // long zero runs (across block ends too)
      size_t i = 0;
      while (i < n) { const size_t run = u(600); for (size_t k = 0; k < run && i < n; ++k) r[i++] = 0; if (i < n) r[i++] = u(256); }
      break;
    }
    case 3: { const size_t per = 1 + u(40); for (size_t i = 0; i < n; ++i) r[i] = (i % per) * 37 & 255; if (n) r[u(n)] ^= 1; break; }   // short period
    case 4: for (size_t i = 0; i < n; ++i) r[i] = (i % 3 == 0) ? 0x10 : (i % 3 == 1) ? 0x01 : 0x00; break;   // non-zero, hash 0
    case 5: {                                                                      // far 3-byte matches on both sides of 4096
      for (auto& b : r) b = u(256);
      const size_t far = 4090 + u(12);
      for (size_t i = 0; i + far + 3 < n; i += 997) { r[i + far] = r[i]; r[i + far + 1] = r[i + 1]; r[i + far + 2] = r[i + 2]; }
      break;
    }
    case 6: for (auto& b : r) b = u(50) ? 17 : u(256); break;                      // flat
    case 7: for (size_t i = 0; i < n; ++i) r[i] = static_cast<unsigned char>((i / 4) * 3 + u(7) - 3); break;  // gradient with noise
    case 8: {                                                                      // a period just below or above the window
      const size_t per = W - 3 + u(7);
      std::vector<unsigned char> base(per);
      for (auto& b : base) b = u(4) ? u(256) : 0;
      for (size_t i = 0; i < n; ++i) r[i] = base[i % per];
      for (size_t i = 0; i < n; i += 1 + u(3000)) r[i] = u(256);
      break;
    }
    case 9: {                                                                      // zero runs laid over every block end
      for (auto& b : r) b = u(3) ? u(256) : 0;
      const size_t bs = zamd::LoBlockSize(n);
      for (size_t e = bs; e < n; e += bs) {
        const size_t a = e - std::min<size_t>(e, u(700)), z = std::min(n, e + u(700));
        for (size_t i = a; i < z; ++i) r[i] = 0;
      }
      break;
    }
    default: {                                                                     // filtered image rows: Sub of a smooth RGBA image, a type byte per row
      const size_t line = 1 + 4 * (16 + u(300));
      unsigned v[4] = {u(256), u(256), u(256), 255};
      for (size_t i = 0; i < n; ++i) {
        if (i % line == 0) { r[i] = 1; continue; }
        const unsigned ch = (i % line - 1) % 4;
        const int dlt = ch == 3 ? 0 : static_cast<int>(u(5)) - 2;
        v[ch] = (v[ch] + dlt) & 255;
        r[i] = static_cast<unsigned char>(dlt);
      }
      break;
    }
  }
  return r;
}

int Fuzz() {
  std::mt19937 g(20250607);
  const unsigned windows[] = {256, 1024, 2048, 8192, 32768};
  const size_t lens[] = {1, 2, 3, 4, 5, 17, 257, 258, 259, 1000, 8191, 8192, 8193, 40000, 65535, 65536, 65537, 70000, 131077, 200000, 600000};
  size_t cases = 0, bad = 0;
  for (unsigned W : windows)
    for (size_t n : lens)
      for (int kind = 0; kind < 11; ++kind) {
        if (n >= 200000 && W != 8192 && kind % 3 != 0) continue;   // (the long ones at every window: a few kinds are enough)
        if (n >= 100000 && (kind == 3 || kind == 6) && W >= 8192 && W != 8192) continue;
        const std::vector<unsigned char> r = Data(g, kind, n, W);
        const size_t a = ModelSize(r.data(), n, W), b = LodeSize(r.data(), n, W);
        ++cases;
        if (a != b) { ++bad; printf("MISMATCH W=%u n=%zu kind=%d model=%zu lodepng=%zu\n", W, n, kind, a, b); }
      }
  // the 262144 cap: 2.2 MB at the window the trials use
  for (int kind : {0, 1, 9, 10}) {
    const size_t n = 2200000;
    const std::vector<unsigned char> r = Data(g, kind, n, 8192);
    const size_t a = ModelSize(r.data(), n, 8192), b = LodeSize(r.data(), n, 8192);
    ++cases;
    if (a != b) { ++bad; printf("MISMATCH W=8192 n=%zu kind=%d model=%zu lodepng=%zu\n", n, kind, a, b); }
  }
  // the code lengths alone, against lodepng_huffman_code_lengths: random, sparse, powers of two, plateaus, Fibonacci
  size_t trees = 0, tbad = 0;
  for (int it = 0; it < 6000; ++it) {
    const int shape = it % 6, which = (it / 6) % 3;
    const size_t numcodes = which == 0 ? 257 + g() % 30 : which == 1 ? 2 + g() % 29 : 19;
    const unsigned maxbits = which == 2 ? 7 : 15;
    std::vector<uint32_t> c(numcodes);
    for (size_t i = 0; i < numcodes; ++i) {
      unsigned v = 0;
      if (shape == 0) v = g() % 1000;
      else if (shape == 1) v = (g() % 4) ? 0 : g() % 50;
      else if (shape == 2) v = 1u << (g() % 18);
      else if (shape == 3) v = 7 + (g() % 9 == 0);
      else if (shape == 4) v = (g() % 16) ? 0 : 1 + g() % 3;
      else v = i < 40 ? (i < 2 ? 1 : c[i - 1] + c[i - 2]) : 0;
      c[i] = v;
    }
    std::vector<unsigned> mine(numcodes), theirs(numcodes), freq(c.begin(), c.end());
    zamd::LoCodeLengths(c.data(), numcodes, maxbits, mine.data());
    lodepng_huffman_code_lengths(theirs.data(), freq.data(), numcodes, maxbits);
    ++trees;
    if (mine != theirs) { ++tbad; printf("LENGTHS MISMATCH it=%d\n", it); }
  }
  // whole blocks of literals (use_lz77 0): the trees' encoding, the trims, the run-length coding
  for (int it = 0; it < 400; ++it) {
    const size_t n = 1 + g() % (it % 8 == 0 ? 300000 : 4000);
    const unsigned lo = g() % 256, span = 1 + g() % (256 - lo), skew = g() % 4;
    std::vector<unsigned char> r(n);
    for (auto& b : r) { unsigned v = g() % span; if (skew) v = v * (g() % span) / span; if (skew > 1) v = v * (g() % span) / span; b = static_cast<unsigned char>(lo + v); }
    ++trees;
    const size_t a = ModelHuffSize(r.data(), n), b = LodeHuffSize(r.data(), n);
    if (a != b) { ++tbad; printf("HUFF MISMATCH it=%d n=%zu model=%zu lodepng=%zu\n", it, n, a, b); }
  }
  printf("%zu buffers against lodepng_zlib_compress: %zu differ; %zu histograms against LodePNG's code lengths and literal-only blocks: %zu differ\n", cases, bad, trees, tbad);
  return bad || tbad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 4 && std::strcmp(argv[1], "size") == 0) {
    std::vector<unsigned char> data;
    FILE* fp = fopen(argv[2], "rb");
    if (!fp) return 2;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) data.insert(data.end(), buf, buf + got);
    fclose(fp);
    const unsigned W = static_cast<unsigned>(atoi(argv[3]));
    printf("%zu %zu\n", LodeSize(data.data(), data.size(), W), ModelSize(data.data(), data.size(), W));
    return 0;
  }
  if (argc >= 3 && std::strcmp(argv[1], "huff") == 0) {
    std::vector<unsigned char> data;
    FILE* fp = fopen(argv[2], "rb");
    if (!fp) return 2;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) data.insert(data.end(), buf, buf + got);
    fclose(fp);
    printf("%zu %zu\n", LodeHuffSize(data.data(), data.size()), ModelHuffSize(data.data(), data.size()));
    return 0;
  }
  return Fuzz();
}
