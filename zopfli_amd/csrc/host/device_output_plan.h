// zmx_compress_device_to_device and zmx_compress_device_batch_to_device, the part that needs no device: zmx_compress_bound's
// arithmetic, the packed form's offsets, the containers' bytes and the planner that turns a stream's chunk list into the
// piece table of a bit join.  Host code only (tests build it without HIP).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "deflate.h"
#include "png_container.h"
#include "symbols.h"
#include "zopfli_amd.h"

namespace zamd {

// An upper bound of what ZopfliCompress makes of `insize` bytes, from the reference's rules:
//  - The input is cut into master blocks of 1 000 000 bytes (deflate.c:916-923; an empty input is one empty master
//    block), each compressed on its own.
//  - A master block becomes at most `blocksplittingmax` blocks (blocksplitter.c:310 stops the search there; the second
//    attempt of deflate.c:872-893 searches under the same limit and replaces the first).  ZopfliInitOptions sets 15;
//    kBoundBlocks = 64 leaves room for callers that raise it.  (blocksplittingmax = 0, no limit, or above 64 is outside
//    the bound: such a call still reports the size it needs when the capacity does not do.)
//  - No block costs more than its stored form: AddLZ77BlockAutoType (deflate.c:747-800) writes the block stored unless
//    fixed or dynamic is strictly smaller than 8 * (5 * pieces + length) bits, pieces = ceil(length / 65535)
//    (deflate.c:591-597) — and those two sizes are exact.
//  - A stored piece is 3 header bits, padding to the next byte, LEN, NLEN and the bytes (deflate.c:625-665): up to 10 bits
//    in front of LEN where the estimate counts 8, so 6 bytes a piece cover it; an empty block is 10 bits (fixed).
//  - The pieces of a master block of M bytes in B blocks are at most M / 65535 + B (a rounding up per block).
// So a master block of M bytes takes at most M + 6 * (M / 65535 + kBoundBlocks + 1) bytes, the stream one byte more for
// its last, partial byte; gzip adds 10 + 8 bytes, zlib 2 + 4.
constexpr size_t kBoundBlocks = 64;
inline size_t ContainerBytes(ZopfliFormat format) {
  return format == ZOPFLI_FORMAT_GZIP ? 18 : format == ZOPFLI_FORMAT_ZLIB ? 6 : 0;
}
inline size_t CompressBound(ZopfliFormat format, size_t insize) {
  const size_t master_blocks = insize == 0 ? 1 : (insize + kMasterBlock - 1) / kMasterBlock;
  const size_t pieces = insize / 65535 + master_blocks * (kBoundBlocks + 1);   // (the floors of M / 65535 add up to at most insize / 65535)
  return insize + 6 * pieces + 1 + ContainerBytes(format);
}

// An arena that does for the streams of n inputs packed as zmx_compress_device_batch_packed packs them: every stream's
// own bound, rounded up to `align` — stream i then begins at or below the sum of the rounded bounds before it.
inline size_t AlignUp(size_t v, size_t align) { return (v + align - 1) / align * align; }
inline size_t CompressBatchBound(ZopfliFormat format, size_t n, const size_t* insize, size_t align) {
  size_t sum = 0;
  for (size_t i = 0; i < n; ++i) sum += AlignUp(CompressBound(format, insize[i]), align);
  return sum;
}
// `align` as the packed form takes it: a power of two, 1 .. 4096.
inline bool PackedAlignOk(size_t align) { return align >= 1 && align <= 4096 && (align & (align - 1)) == 0; }
// Where the packed form puts n streams of size[i] bytes: offset[i] is the end of stream i - 1 rounded up to `align`
// (offset[0] = 0; an empty stream takes no room but is aligned like the others).  Returns the end of the last stream.
inline size_t PackedOffsets(size_t n, const size_t* size, size_t align, size_t* offset) {
  size_t end = 0;
  for (size_t i = 0; i < n; ++i) {
    offset[i] = AlignUp(end, align);
    end = offset[i] + size[i];
  }
  return end;
}

// The container's bytes around the deflate stream, as the reference writes them.
inline std::vector<uint8_t> ContainerHeader(ZopfliFormat format) {
  if (format == ZOPFLI_FORMAT_GZIP) return {31, 139, 8, 0, 0, 0, 0, 0, 2, 3};   // gzip_container.c:90-101
  if (format == ZOPFLI_FORMAT_ZLIB) {                                           // zlib_container.c:56-64
    unsigned cmfflg = 256 * 120 + 3 * 64;   // CM 8, CINFO 7, FLEVEL 3, no dictionary
    cmfflg += 31 - cmfflg % 31;
    return {static_cast<uint8_t>(cmfflg / 256), static_cast<uint8_t>(cmfflg % 256)};
  }
  return {};
}
inline std::vector<uint8_t> ContainerTrailer(ZopfliFormat format, uint32_t sum, size_t insize) {
  std::vector<uint8_t> t;
  if (format == ZOPFLI_FORMAT_GZIP) {          // CRC-32, then ISIZE, both little-endian (gzip_container.c:107-116)
    for (int i = 0; i < 4; ++i) t.push_back(static_cast<uint8_t>(sum >> (8 * i)));
    for (int i = 0; i < 4; ++i) t.push_back(static_cast<uint8_t>(insize >> (8 * i)));
  } else if (format == ZOPFLI_FORMAT_ZLIB) {   // Adler-32, big-endian (zlib_container.c:71-74)
    for (int i = 3; i >= 0; --i) t.push_back(static_cast<uint8_t>(sum >> (8 * i)));
  }
  return t;
}

// A piece of the plan: `nbits` bits from bit `src_bit` of the literals buffer at byte `lit` (literal) or of the device
// string at `dev`, to bit `dst_bit` of the output.
struct PlanPiece {
  bool literal;
  size_t lit;
  const void* dev;
  uint64_t src_bit, nbits, dst_bit;
};
struct OutputPlan {
  std::vector<uint8_t> literals;   // uploaded once: headers, trees, LEN / NLEN, the trailer, blocks the host wrote
  std::vector<PlanPiece> pieces;   // sorted by dst_bit
  uint64_t total_bits = 0;         // a whole number of bytes
  size_t device_blocks = 0;        // blocks whose symbols' bits never left the device
  size_t host_blocks = 0;          // blocks the host wrote
};

// The stream of `prefix` (the container's header), the chunks [first, last) and `trailer`, from bit 0: MergeChunks'
// placement arithmetic (deflate.cc) with no running bit pointer, the output always beginning byte-aligned.  `d_in`: the
// device memory the stored chunks' positions refer to.
inline OutputPlan PlanOutput(const std::vector<uint8_t>& prefix, const Chunk* first, const Chunk* last, const unsigned char* d_in,
                             const std::vector<uint8_t>& trailer) {
  OutputPlan plan;
  std::vector<uint8_t>& lit = plan.literals;
  const auto literal = [&](const uint8_t* bytes, size_t nbytes, uint64_t nbits, uint64_t dst_bit) {
    if (nbits == 0) return;
    plan.pieces.push_back({true, lit.size(), nullptr, 0, nbits, dst_bit});
    lit.insert(lit.end(), bytes, bytes + nbytes);
  };
  literal(prefix.data(), prefix.size(), 8 * prefix.size(), 0);
  uint64_t cur = 8 * prefix.size();
  for (const Chunk* it = first; it != last; ++it) {
    const Chunk& c = *it;
    if (c.kind == Chunk::kBits) {
      literal(c.BitData(), (c.nbits + 7) / 8, c.nbits, cur);
      cur += c.nbits;
      ++plan.host_blocks;
    } else if (c.kind == Chunk::kDeviceBits) {
      literal(c.bits.data(), (c.header_bits + 7) / 8, c.header_bits, cur);
      if (c.nbits > c.header_bits) plan.pieces.push_back({false, 0, c.dev_bits, c.header_bits, c.nbits - c.header_bits, cur + c.header_bits});
      cur += c.nbits;
      ++plan.device_blocks;
    } else {
      // AddNonCompressedBlock (deflate.c:625-665): pieces of at most 65535 bytes, each byte-aligned behind its 3 header bits
      size_t pos = c.start;
      for (;;) {
        size_t piece = 65535;
        if (pos + piece > c.end) piece = c.end - pos;
        const bool last = pos + piece >= c.end;
        const uint8_t header = c.final_block && last ? 1 : 0;   // BFINAL, BTYPE 00
        literal(&header, 1, 3, cur);
        cur = (cur + 3 + 7) / 8 * 8;
        const unsigned len = static_cast<unsigned>(piece), nlen = ~len & 0xffffu;
        const uint8_t lens[4] = {static_cast<uint8_t>(len & 255), static_cast<uint8_t>(len >> 8), static_cast<uint8_t>(nlen & 255),
                                 static_cast<uint8_t>(nlen >> 8)};
        literal(lens, 4, 32, cur);
        cur += 32;
        if (piece) plan.pieces.push_back({false, 0, d_in + pos, 0, 8 * static_cast<uint64_t>(piece), cur});
        cur += 8 * static_cast<uint64_t>(piece);
        if (last) break;
        pos += piece;
      }
    }
  }
  cur = (cur + 7) / 8 * 8;
  literal(trailer.data(), trailer.size(), 8 * trailer.size(), cur);
  plan.total_bits = cur + 8 * trailer.size();
  return plan;
}
inline OutputPlan PlanOutput(const std::vector<uint8_t>& prefix, const std::vector<Chunk>& chunks, const unsigned char* d_in,
                             const std::vector<uint8_t>& trailer) {
  return PlanOutput(prefix, chunks.data(), chunks.data() + chunks.size(), d_in, trailer);
}

// ---- a FRAME around the zlib stream: the PNG file left in device memory (zmx_png_encode_device_to_device and its kin)
// The stream goes the way of zmx_compress_device_to_device(ZOPFLI_FORMAT_ZLIB); the frame replaces the container's header
// by bytes in front of the stream's first bit and puts bytes behind its Adler-32, all of them literals of the same plan:
//   in front   `file_prefix` — png_container.h's PngPrefix / PngPrefixReduced, up to and including "IDAT" — and 78 01,
//              LodePNG's zlib header written straight away (PngCloseAt patches zopfli's 78 DA on the host);
//   behind     four placeholder bytes where the IDAT's CRC-32 goes, and the 12 bytes of IEND.
// The plan gives the file's size, and so the IDAT's length (PngFrameSetLength), before anything is written.  What the plan
// cannot hold is the CRC-32: it covers "IDAT" and the joined stream — [file_prefix.size() - 4, file size - 16) of the file
// — and is sealed into the placeholder by the device after the join (zmx_internal_checksum_seal).
struct PngFrame {
  std::vector<uint8_t> file_prefix;
};
inline std::vector<uint8_t> PngFrameHeader(const PngFrame& frame) {
  std::vector<uint8_t> h = frame.file_prefix;
  h.push_back(0x78);
  h.push_back(0x01);
  return h;
}
// `zlib_trailer`: ContainerTrailer(ZOPFLI_FORMAT_ZLIB, ...)
inline std::vector<uint8_t> PngFrameTrailer(std::vector<uint8_t> zlib_trailer) {
  unsigned char tail[kPngTrailerBytes];
  PngStore32(tail, 0);   // the placeholder
  PngStore32(tail + 4, 0);
  std::memcpy(tail + 8, "IEND", 4);
  PngStore32(tail + 12, PngCrc32(tail + 8, 4));
  zlib_trailer.insert(zlib_trailer.end(), tail, tail + kPngTrailerBytes);
  return zlib_trailer;
}
// The IDAT's length of a file of `file_bytes` bytes behind a prefix of `prefix_bytes`.
inline uint64_t PngFrameIdatBytes(uint64_t file_bytes, size_t prefix_bytes) { return file_bytes - prefix_bytes - kPngTrailerBytes; }
constexpr uint64_t kPngMaxChunkBytes = 0x7fffffffu;   // a chunk's length has 31 bits
// Fills the IDAT's length into a plan made with PngFrameHeader / PngFrameTrailer (the prefix is its first literal);
// false, with nothing changed, when the stream does not fit a chunk.
inline bool PngFrameSetLength(const PngFrame& frame, OutputPlan* plan) {
  const uint64_t n = PngFrameIdatBytes(plan->total_bits / 8, frame.file_prefix.size());
  if (n > kPngMaxChunkBytes) return false;
  PngStore32(plan->literals.data() + frame.file_prefix.size() - 8, static_cast<uint32_t>(n));
  return true;
}

// An upper bound of the PNG file that zmx_png_encode_device / zmx_png_optimize_device (and their to-device forms) make of
// an image of height rows in the mode (colortype, bitdepth):
//   kPngMaxPrefixBytes + CompressBound(ZLIB, height * (linebytes + 1)) + kPngTrailerBytes.
//  - The IDAT's payload is ZopfliCompress(ZLIB) of the filtered scanlines — the header's second byte differs, its size
//    does not —, so CompressBound above bounds it, given the scanlines' size S.
//  - S of the input's mode bounds S of the mode of the FIRST file.  S = height * (ceil(width * bpp / 8) + 1) rises with
//    bpp, the bits per pixel, and colour reduction (png_color_choose.h, LodePNG's auto_choose_color) only ever picks a
//    mode whose bpp is at most the input's: it drops channels that say nothing (alpha, colour), halves 16 bits to 8 when
//    every sample's two bytes are equal, goes below 8 bits for grey, or to a palette of at most 8 bits per pixel where the
//    input has at least 8 (colour types 0, 2, 4, 6 at 8 or 16 bits) — and otherwise keeps the input's mode.
//  - The second try of a small palette file (PngRetryMode: RGB or RGBA at 8 bits) may have MORE bits per pixel than the
//    input (grey + alpha at 8 bits retried as RGBA).  It needs no room of the caller's: it is made into a buffer of the
//    call's own and replaces the first file only when it is strictly smaller, so the file that is kept is never larger
//    than the first.
//  - --lossy_8bit halves the sample width before anything else (16 -> 8 bits, same colour type): bpp halves, S falls.
//    --lossy_transparent rewrites pixels in place: S is unchanged.
//  - CompressBound rises with its input size, so the bound of the largest S holds for the S actually used.
//  - The prefix is at most kPngMaxPrefixBytes (signature, IHDR, a full PLTE and tRNS, the IDAT's length and type).
inline size_t PngBound(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth) {
  const size_t scanlines = static_cast<size_t>(height) * (PngLineBytes(width, colortype, bitdepth) + 1);
  return kPngMaxPrefixBytes + CompressBound(ZOPFLI_FORMAT_ZLIB, scanlines) + kPngTrailerBytes;
}
// The same for the index entries (zmx_png_index_bound): a palette or grey image of 1 .. 8 bits per pixel.
//  - The --keepcolortype file has the input's own bits per pixel.  LodePNG's choice for the expansion is not bounded by
//    them: a 1-bit palette of two colours on few pixels comes out as RGB or RGBA at 8 bits (fewer than two pixels a
//    colour), and the to-device optimize entry writes such a first file straight into d_out.
//  - No mode that can come out has more than 32 bits per pixel — the expansion has 8-bit samples only, so 16-bit modes
//    are never chosen, and the second try is RGB or RGBA at 8 bits — and S rises with the bits per pixel.  So S of RGBA at 8
//    bits bounds S of every file either entry makes, the kept one included.
inline size_t PngIndexBound(uint32_t width, uint32_t height) { return PngBound(width, height, 6, 8); }
inline size_t PngBatchBound(size_t n, const zmx_png_image* images, size_t align) {
  size_t sum = 0;
  for (size_t i = 0; i < n; ++i) sum += AlignUp(PngBound(images[i].width, images[i].height, images[i].colortype, images[i].bitdepth), align);
  return sum;
}

// ---- the two to-device compress entries with a frame (device_output.cc, batch.cc; for png_encode.cc)
// zmx_compress_device_to_device under the name `who`; `frame` non-null: ZOPFLI_FORMAT_ZLIB with the frame around it, the
// CRC-32 sealed after the join, while the call still holds its contexts.  A stream that does not fit an IDAT is refused
// like a capacity that is too small: *outsize = the file's size, d_out untouched.
int CompressDeviceToDevice(const char* who, const ZopfliOptions* options, ZopfliFormat output_type, const void* d_in, size_t insize,
                           void* d_out, size_t capacity, size_t* outsize, const PngFrame* frame);
// zmx_compress_device_batch_packed(ZOPFLI_FORMAT_ZLIB) under the name `who` with frames[i] around stream i: one join for
// all files, then one seal (two launches) for all of them.
int CompressDeviceBatchPackedFramed(const char* who, const ZopfliOptions* options, size_t n, const void* const* d_in, const size_t* insize,
                                    const PngFrame* frames, void* d_arena, size_t capacity, size_t align, size_t* outoffset, size_t* outsize);

}  // namespace zamd
