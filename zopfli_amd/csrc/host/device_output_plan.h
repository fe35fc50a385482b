// zmx_compress_device_to_device and zmx_compress_device_batch_to_device, the part that needs no device: zmx_compress_bound's
// arithmetic, the packed form's offsets, the containers' bytes and the planner that turns a stream's chunk list into the
// piece table of a bit join.  Host code only (tests build it without HIP).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "deflate.h"
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

}  // namespace zamd
