// The container of zmx_png_encode_device (png_encode.cc): the PNG file around one zlib stream, as LodePNG's encoder
// writes it for zopflipng (lodepng.cpp lodepng_encode: the signature, IHDR, one IDAT, IEND; no other chunk).  Host
// arithmetic only — no device call, nothing of the library but checksum.h's CRC algebra — so a plain C++ program
// runs it (tests/hostlib/png_container_print.cc, linked with checksum.cc).
// The file is made in place around the stream: PngPrefix's 41 bytes go in front of where ZopfliCompress appends it, and
// PngClose fills in what depends on the stream and gives the 16 bytes that follow it, so a stream of tens of megabytes
// is neither copied nor read more than once (its CRC-32: eight bytes a step, in pieces on a few threads when long).
#ifndef ZOPFLI_AMD_PNG_CONTAINER_H_
#define ZOPFLI_AMD_PNG_CONTAINER_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "checksum.h"

namespace zamd {

// what zmx_png_encode_device takes: grey, RGB, grey + alpha, RGBA at 8 or 16 bits
inline bool PngFormatOk(uint32_t colortype, uint32_t bitdepth) {
  return (colortype == 0 || colortype == 2 || colortype == 4 || colortype == 6) && (bitdepth == 8 || bitdepth == 16);
}
inline uint32_t PngChannels(uint32_t colortype) { return colortype == 0 ? 1 : colortype == 2 ? 3 : colortype == 4 ? 2 : 4; }
// bytes per pixel: the distance to a byte's left neighbour (bit depths of 8 and 16 only)
inline size_t PngByteWidth(uint32_t colortype, uint32_t bitdepth) { return PngChannels(colortype) * (bitdepth / 8); }
inline size_t PngLineBytes(uint32_t width, uint32_t colortype, uint32_t bitdepth) {
  return static_cast<size_t>(width) * PngByteWidth(colortype, bitdepth);
}

constexpr size_t kPngPrefixBytes = 41;        // signature 8, IHDR chunk 25, the IDAT's length and type 8
constexpr size_t kPngTrailerBytes = 16;       // the IDAT's CRC 4, IEND chunk 12
constexpr size_t kPngCrcPiece = 1u << 20;     // a thread's share of a long stream's CRC is at least this
constexpr size_t kPngCrcThreads = 8;

// CRC-32 of data[0, n) on its own, over kCrcPoly, eight bytes a step (Intel's slicing-by-8: table k advances a byte by
// k more zero bytes).
inline uint32_t PngCrc32(const unsigned char* data, size_t n) {
  static const struct Tables {
    uint32_t t[8][256];
    Tables() {
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        t[0][i] = c;
      }
      for (uint32_t i = 0; i < 256; ++i) {
        for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255u];
      }
    }
  } T;
  uint32_t crc = 0xffffffffu;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint32_t lo, hi;
    std::memcpy(&lo, data + i, 4);
    std::memcpy(&hi, data + i + 4, 4);
    lo ^= crc;   // (little-endian hosts: the library's only ones)
    crc = T.t[7][lo & 255u] ^ T.t[6][(lo >> 8) & 255u] ^ T.t[5][(lo >> 16) & 255u] ^ T.t[4][lo >> 24] ^
          T.t[3][hi & 255u] ^ T.t[2][(hi >> 8) & 255u] ^ T.t[1][(hi >> 16) & 255u] ^ T.t[0][hi >> 24];
  }
  for (; i < n; ++i) crc = T.t[0][(crc ^ data[i]) & 255u] ^ (crc >> 8);
  return ~crc;
}

// CRC-32 of A followed by B from theirs (what zmx_checksum_combine does for ZMX_CRC32)
inline uint32_t PngCrcJoin(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return Gf2MulMod(crc_a, Gf2XPow8(len_b)) ^ crc_b; }

// The same CRC-32 in pieces of at least `piece` bytes, on up to kPngCrcThreads threads, joined in order.
inline uint32_t PngCrc32Pieces(const unsigned char* data, size_t n, size_t piece) {
  const size_t pieces = std::min(kPngCrcThreads, n / std::max<size_t>(piece, 1));
  if (pieces < 2) return PngCrc32(data, n);
  const size_t share = n / pieces;
  std::vector<uint32_t> crc(pieces);
  std::vector<std::thread> threads;
  const auto at = [&](size_t p) { return p == pieces ? n : p * share; };
  for (size_t p = 1; p < pieces; ++p) threads.emplace_back([&, p] { crc[p] = PngCrc32(data + at(p), at(p + 1) - at(p)); });
  crc[0] = PngCrc32(data, at(1));
  for (std::thread& t : threads) t.join();
  uint32_t all = crc[0];
  for (size_t p = 1; p < pieces; ++p) all = PngCrcJoin(all, crc[p], at(p + 1) - at(p));
  return all;
}

inline void PngStore32(unsigned char* p, uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = static_cast<unsigned char>(v >> (24 - 8 * k));
}

// The file's first kPngPrefixBytes bytes; the IDAT's length is PngClose's to fill in.
inline void PngPrefix(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth, unsigned char* prefix) {
  static const unsigned char kSignature[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  std::memcpy(prefix, kSignature, 8);
  PngStore32(prefix + 8, 13);
  std::memcpy(prefix + 12, "IHDR", 4);
  PngStore32(prefix + 16, width);
  PngStore32(prefix + 20, height);
  prefix[24] = static_cast<unsigned char>(bitdepth);
  prefix[25] = static_cast<unsigned char>(colortype);
  prefix[26] = prefix[27] = prefix[28] = 0;   // compression, filter method, no interlace
  PngStore32(prefix + 29, PngCrc32(prefix + 12, 17));
  PngStore32(prefix + 33, 0);
  std::memcpy(prefix + 37, "IDAT", 4);
}

// file[0, size): PngPrefix's bytes and behind them the stream ZopfliCompress(ZOPFLI_FORMAT_ZLIB) makes of the filtered
// scanlines.  Its second byte — zopfli writes 78 DA, "maximum compression" — becomes LodePNG's 01 (lodepng.cpp
// lodepng_zlib_compress: FLEVEL 0, and the FCHECK that makes 0x7801 a multiple of 31), the IDAT's length is filled in, and
// `trailer` gets the kPngTrailerBytes bytes that end the file.  False, with nothing changed, when the stream cannot be
// one (shorter than a header and an Adler-32, or not 78 DA) or does not fit a chunk's 31-bit length.
// (PngCloseAt: the same behind a prefix of `prefix_bytes` bytes, PngPrefixReduced's)
inline bool PngCloseAt(unsigned char* file, size_t size, size_t prefix_bytes, unsigned char* trailer, size_t crc_piece = kPngCrcPiece) {
  if (prefix_bytes < kPngPrefixBytes || size < prefix_bytes + 6) return false;
  const size_t n = size - prefix_bytes;
  unsigned char* zlib = file + prefix_bytes;
  if (n > 0x7fffffffu || zlib[0] != 0x78 || zlib[1] != 0xda) return false;
  zlib[1] = 0x01;
  PngStore32(file + prefix_bytes - 8, static_cast<uint32_t>(n));
  PngStore32(trailer, PngCrcJoin(PngCrc32(file + prefix_bytes - 4, 4), PngCrc32Pieces(zlib, n, crc_piece), n));
  PngStore32(trailer + 4, 0);
  std::memcpy(trailer + 8, "IEND", 4);
  PngStore32(trailer + 12, PngCrc32(trailer + 8, 4));
  return true;
}
inline bool PngClose(unsigned char* file, size_t size, unsigned char* trailer, size_t crc_piece = kPngCrcPiece) {
  return PngCloseAt(file, size, kPngPrefixBytes, trailer, crc_piece);
}

// ---- the prefix of a file whose colour mode was reduced (zmx_png_optimize_device, png_optimize.cc): LodePNG's chunk
// order IHDR, PLTE, tRNS, IDAT (lodepng.cpp lodepng_encode, addChunk_PLTE, addChunk_tRNS)
// what such a file may be: the modes PNG has
inline bool PngReducedFormatOk(uint32_t colortype, uint32_t bitdepth) {
  switch (colortype) {
    case 0: return bitdepth == 1 || bitdepth == 2 || bitdepth == 4 || bitdepth == 8 || bitdepth == 16;
    case 3: return bitdepth == 1 || bitdepth == 2 || bitdepth == 4 || bitdepth == 8;
    case 2: case 4: case 6: return bitdepth == 8 || bitdepth == 16;
    default: return false;
  }
}
// signature 8, IHDR 25, PLTE up to 12 + 768, tRNS up to 12 + 256, the IDAT's length and type 8
constexpr size_t kPngMaxPrefixBytes = 8 + 25 + (12 + 768) + (12 + 256) + 8;

// one whole chunk at p; returns its size
inline size_t PngChunk(unsigned char* p, const char* tag, const unsigned char* data, size_t n) {
  PngStore32(p, static_cast<uint32_t>(n));
  std::memcpy(p + 4, tag, 4);
  if (n) std::memcpy(p + 8, data, n);
  PngStore32(p + 8 + n, PngCrc32(p + 4, 4 + n));
  return 12 + n;
}

// The file up to the IDAT's type, into prefix[kPngMaxPrefixBytes]; returns its size.  Colour type 3: PLTE with the RGB of
// each of the `palettesize` (1 .. 256) entries r, g, b, a at `palette`, and tRNS with their alphas up to the last that
// is not 255 (none: no chunk).  Colour types 0 and 2 with `key`: tRNS with the grey value, or the three, as 16-bit numbers.
inline size_t PngPrefixReduced(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth, const unsigned char* palette,
                               uint32_t palettesize, bool key, uint32_t key_r, uint32_t key_g, uint32_t key_b, unsigned char* prefix) {
  unsigned char plain[kPngPrefixBytes];
  PngPrefix(width, height, colortype, bitdepth, plain);
  std::memcpy(prefix, plain, 33);
  size_t at = 33;
  if (colortype == 3) {
    unsigned char rgb[768], alphas[256];
    size_t amount = 0;
    for (uint32_t i = 0; i < palettesize; ++i) {
      std::memcpy(rgb + 3 * i, palette + 4 * i, 3);
      alphas[i] = palette[4 * i + 3];
      if (alphas[i] != 255) amount = i + 1;
    }
    at += PngChunk(prefix + at, "PLTE", rgb, 3 * static_cast<size_t>(palettesize));
    if (amount) at += PngChunk(prefix + at, "tRNS", alphas, amount);
  } else if (key && (colortype == 0 || colortype == 2)) {
    const uint32_t v[3] = {key_r, key_g, key_b};
    unsigned char data[6];
    for (int k = 0; k < 3; ++k) {
      data[2 * k] = static_cast<unsigned char>(v[k] >> 8);
      data[2 * k + 1] = static_cast<unsigned char>(v[k] & 255u);
    }
    at += PngChunk(prefix + at, "tRNS", data, colortype == 0 ? 2 : 6);
  }
  PngStore32(prefix + at, 0);
  std::memcpy(prefix + at + 4, "IDAT", 4);
  return at + 8;
}

// The whole file around a stream that lies elsewhere (`zlib` is not changed).
inline bool PngAssemble(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth, const unsigned char* zlib, size_t n,
                        std::vector<unsigned char>* png, size_t crc_piece = kPngCrcPiece) {
  png->assign(kPngPrefixBytes + n + kPngTrailerBytes, 0);
  PngPrefix(width, height, colortype, bitdepth, png->data());
  if (n) std::memcpy(png->data() + kPngPrefixBytes, zlib, n);
  return PngClose(png->data(), kPngPrefixBytes + n, png->data() + kPngPrefixBytes + n, crc_piece);
}

}  // namespace zamd

#endif  // ZOPFLI_AMD_PNG_CONTAINER_H_
