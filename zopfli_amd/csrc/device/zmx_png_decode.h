// k_png_chunks, k_png_unfilter: n PNG files in device memory decoded into device memory (zmx_png_decode_device*,
// drv_png_decode.h).  Between the two kernels the IDAT stream goes through k_inflate (zmx_inflate.h) and the chunks'
// CRC-32s and the stream's Adler-32 through the checksum kernels (zmx_checksum_device.h), all unchanged.
//   k_png_chunks   one launch for n files, a LANE a file: the walk over a file's chunks is a chain of dependent loads (a
//                  chunk's length says where the next one begins), so there is nothing to widen.  Per file a fixed record
//                  (PngWalkRecord) and up to `cap` entries of the chunks whose CRC is checked — IHDR, PLTE, tRNS, every
//                  IDAT, IEND — in file order.  A file with more of them than `cap` is still counted to its end
//                  (nentries); the host walks it again with room, so no number is a limit.  Every load lies inside
//                  [file, file + size): PngWalk compares before it reads.
//   k_png_unfilter one launch for n images, a WAVE an image.  A band is 64 rows, lane l on row band * 64 + l, skewed by
//                  one group (bytewidth bytes: LodePNG's unit): at step t lane l makes group t - l of its row.  What it
//                  needs of the row above — groups t - l and t - l - 1 — lane l - 1 made at steps t - 1 and t - 2: the
//                  first comes by one wave shift a step, the second is the first of the step before, kept in a register,
//                  as the row's own last group ("left") is.  No LDS, no barrier in the steady state.  All five filter
//                  types take the same walk; a lane reads its own row's type.
//   the band carry lane 0's row above is lane 63's row of the band before.  Lane 63 writes its groups into a carry row,
//                  lane 0 reads them a band later: in LDS (kPngCarryBytes), never from what the wave stored to d_out.
//                  Within a band lane 0 reads group g at step g and lane 63 overwrites it at step g + 63, so one row
//                  serves; a barrier between bands (one wave: its waits alone) orders band against band.
//   the wide path  rows longer than kPngCarryBytes (or PngDecodeHooks::force_wide) carry through two rows of global
//                  memory of the call's own, written by band b and read by band b + 1, with a KERNEL boundary between
//                  the bands: the driver launches band after band (band_first, band_count = 1), all wide images of the
//                  call in each launch.
//   loads          a lane's bytes are sequential in its row and apart from the other lanes': it loads the aligned
//                  32-bit word around a byte once and steps through it in a register.  The scanlines lie in a buffer of
//                  the call's own whose slices begin at 16-byte boundaries and end on whole words, so the word around
//                  any byte of a slice may be read.
//   stores         fused, no second pass: _OWN the unfiltered bytes (the padding bits of a row's last byte cleared for
//                  depths below 8), _RGBA8 the converted pixels (lodepng_decode32's), the palette with its tRNS alpha
//                  from a 1 KiB LDS table read from the file's PLTE and tRNS where they lie.  A lane gathers its bytes
//                  by destination word: a whole aligned word that is all its own is one 32-bit store, the bytes at a
//                  row's ends go singly.  Nothing at or beyond `limit` = min(capacity, outsize) is stored (PngFlush
//                  compares every store), at any alignment of the destination.
//   a bad filter   a row whose type byte is above 4 ends its image with kPngDecFilter and the lowest such row; the bands
//                  below it are written, nothing of its own band.
// Every rule is a __host__ __device__ function and the walks are templates over `Par`, which says how the 64 lanes run:
// side by side on the device (PngDevicePar below), one after the other in a CPU program
// (tests/hostlib/png_decode_print.cc), which so runs the very code of the kernels.  The header compiles without HIP; the
// kernels are there for the device layer only (ZMX_PNG_DECODE_KERNELS).
#ifndef ZMX_PNG_DECODE_H_
#define ZMX_PNG_DECODE_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMX_PD_HD __host__ __device__
#else
#define ZMX_PD_HD
#endif

namespace zamd {

// (ZMX_PNG_DECODE_* of include/zopfli_amd.h: drv_png_decode.h holds the two against each other)
enum PngDecodeStatus : uint32_t {
  kPngDecOk = 0,
  kPngDecSignature,   // bad signature, or shorter than 33 bytes
  kPngDecIhdr,
  kPngDecInterlace,   // Adam7: recognised, not decoded
  kPngDecChunk,       // no room for a chunk, a length above 2^31 - 1, a chunk past the file's end
  kPngDecCritical,    // an unknown critical chunk
  kPngDecCrc,         // (set by the host from the checksum kernels' values)
  kPngDecPlte,
  kPngDecTrns,
  kPngDecStream,      // (host: k_inflate's verdict, or the Adler-32)
  kPngDecSize,        // (host)
  kPngDecFilter,
  kPngDecCapacity,    // (host)
  kPngDecShape,       // (host, the sink entries: the file's size is not its sink's)
  kPngDecStatuses
};
constexpr uint32_t kPngDecOwn = 0, kPngDecRgba8 = 1;   // (ZMX_PNG_DECODE_OWN, _RGBA8)
constexpr uint32_t kPngDecLanes = 64;
constexpr uint32_t kPngCarryBytes = 16384;     // the LDS carry row: longer rows take the wide path
constexpr uint32_t kPngDecEntries = 8;         // entries a file in the first walk (IHDR, PLTE, tRNS, IDAT, IEND: 5)
enum PngChunkKind : uint32_t { kPngChunkIhdr = 0, kPngChunkPlte, kPngChunkTrns, kPngChunkIdat, kPngChunkIend };

struct PngChunkEntry {      // a chunk whose CRC-32 is checked
  uint64_t offset;          // of its length field in the file; the CRC covers [offset + 4, offset + 8 + length)
  uint32_t length, crc;     // the data's bytes, the stored CRC-32
  uint32_t kind, index;     // a PngChunkKind; the chunk's number in the file (IHDR 0)
};
static_assert(sizeof(PngChunkEntry) == 24, "24 bytes an entry");

struct PngWalkRecord {
  uint32_t status, stop;    // a PngDecodeStatus of the walk; the number of the chunk it stopped at
  uint32_t width, height, colortype, bitdepth, interlace, palettesize;
  uint32_t has_key, key_r, key_g, key_b;
  uint32_t nentries, nidat;         // all there are, whatever the capacity
  uint64_t idat_bytes;
  uint64_t plte_offset, trns_offset;   // of the DATA of the last PLTE, and of the tRNS that holds for it
  uint32_t trns_length, has_plte;
};
static_assert(sizeof(PngWalkRecord) == 88, "88 bytes a file");

struct PngFileRef {
  const unsigned char* file;
  uint64_t size;
  uint64_t entry_first;     // where the file's entries begin in the launch's entry array
  uint32_t entry_cap, slot; // how many it may write; the file's record and palette slot
};

// ---- the header's rules
ZMX_PD_HD inline uint32_t PngBe32(const unsigned char* p) {
  return (static_cast<uint32_t>(p[0]) << 24) | (static_cast<uint32_t>(p[1]) << 16) | (static_cast<uint32_t>(p[2]) << 8) | p[3];
}
ZMX_PD_HD inline bool PngTypeIs(const unsigned char* p, char a, char b, char c, char d) {
  return p[0] == static_cast<unsigned char>(a) && p[1] == static_cast<unsigned char>(b) && p[2] == static_cast<unsigned char>(c) &&
         p[3] == static_cast<unsigned char>(d);
}
// LodePNG's checkColorValidity: the 15 legal pairs
ZMX_PD_HD inline bool PngColorOk(uint32_t colortype, uint32_t depth) {
  switch (colortype) {
    case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    case 2: case 4: case 6: return depth == 8 || depth == 16;
    default: return false;
  }
}
ZMX_PD_HD inline uint32_t PngChannels(uint32_t colortype) { return colortype == 2 ? 3 : colortype == 4 ? 2 : colortype == 6 ? 4 : 1; }
ZMX_PD_HD inline uint32_t PngBpp(uint32_t colortype, uint32_t depth) { return PngChannels(colortype) * depth; }
ZMX_PD_HD inline uint64_t PngLineBytes(uint32_t width, uint32_t bpp) { return (static_cast<uint64_t>(width) * bpp + 7) / 8; }
ZMX_PD_HD inline uint32_t PngByteWidth(uint32_t bpp) { return bpp < 8 ? 1 : bpp / 8; }

// ---- the chunk walk (LodePNG's lodepng_inspect and decodeGeneric's loop, readChunk_PLTE, readChunk_tRNS)
ZMX_PD_HD inline void PngAddEntry(PngWalkRecord* R, PngChunkEntry* entries, uint32_t cap, uint64_t offset, uint32_t length, uint32_t crc,
                                  uint32_t kind, uint32_t index) {
  if (R->nentries < cap) entries[R->nentries] = {offset, length, crc, kind, index};
  ++R->nentries;
}

ZMX_PD_HD inline void PngWalk(const unsigned char* f, uint64_t size, uint32_t cap, PngChunkEntry* entries, PngWalkRecord* R) {
  *R = PngWalkRecord{};
  if (size < 33) { R->status = kPngDecSignature; return; }
  if (f[0] != 137 || f[1] != 80 || f[2] != 78 || f[3] != 71 || f[4] != 13 || f[5] != 10 || f[6] != 26 || f[7] != 10) {
    R->status = kPngDecSignature;
    return;
  }
  if (PngBe32(f + 8) != 13 || !PngTypeIs(f + 12, 'I', 'H', 'D', 'R')) { R->status = kPngDecIhdr; return; }
  R->width = PngBe32(f + 16);
  R->height = PngBe32(f + 20);
  R->bitdepth = f[24];
  R->colortype = f[25];
  R->interlace = f[28];
  if (R->width == 0 || R->height == 0 || !PngColorOk(R->colortype, R->bitdepth) || f[26] != 0 || f[27] != 0 || R->interlace > 1) {
    R->status = kPngDecIhdr;
    return;
  }
  PngAddEntry(R, entries, cap, 8, 13, PngBe32(f + 29), kPngChunkIhdr, 0);
  uint64_t pos = 33;
  uint32_t index = 1;
  for (;; ++index) {
    R->stop = index;
    if (size - pos < 12) { R->status = kPngDecChunk; return; }      // (pos <= size always)
    const uint32_t length = PngBe32(f + pos);
    if (length > 0x7fffffffu || size - pos - 12 < length) { R->status = kPngDecChunk; return; }
    const unsigned char* const type = f + pos + 4;
    const uint32_t crc = PngBe32(f + pos + 8 + length);
    if (PngTypeIs(type, 'I', 'D', 'A', 'T')) {
      ++R->nidat;
      R->idat_bytes += length;
      PngAddEntry(R, entries, cap, pos, length, crc, kPngChunkIdat, index);
    } else if (PngTypeIs(type, 'I', 'E', 'N', 'D')) {
      PngAddEntry(R, entries, cap, pos, length, crc, kPngChunkIend, index);
      break;
    } else if (PngTypeIs(type, 'P', 'L', 'T', 'E')) {
      R->palettesize = length / 3;
      if (R->palettesize == 0 || R->palettesize > 256) { R->status = kPngDecPlte; return; }
      R->has_plte = 1;
      R->plte_offset = pos + 8;
      if (R->colortype == 3) R->trns_length = 0;    // (a new palette is opaque again)
      PngAddEntry(R, entries, cap, pos, length, crc, kPngChunkPlte, index);
    } else if (PngTypeIs(type, 't', 'R', 'N', 'S')) {
      if (R->colortype == 3) {
        if (length > R->palettesize) { R->status = kPngDecTrns; return; }
        R->trns_offset = pos + 8;
        R->trns_length = length;
      } else if (R->colortype == 0) {
        if (length != 2) { R->status = kPngDecTrns; return; }
        R->has_key = 1;
        R->key_r = R->key_g = R->key_b = 256u * f[pos + 8] + f[pos + 9];
      } else if (R->colortype == 2) {
        if (length != 6) { R->status = kPngDecTrns; return; }
        R->has_key = 1;
        R->key_r = 256u * f[pos + 8] + f[pos + 9];
        R->key_g = 256u * f[pos + 10] + f[pos + 11];
        R->key_b = 256u * f[pos + 12] + f[pos + 13];
      } else {
        R->status = kPngDecTrns;
        return;
      }
      PngAddEntry(R, entries, cap, pos, length, crc, kPngChunkTrns, index);
    } else if (!(type[0] & 32)) {
      R->status = kPngDecCritical;
      return;
    }
    pos += 12 + static_cast<uint64_t>(length);
  }
  if (R->colortype == 3 && !R->has_plte) { R->status = kPngDecPlte; return; }
  if (R->interlace == 1) R->status = kPngDecInterlace;
}

// Entry i of the palette as the decoder sees it: r | g << 8 | b << 16 | a << 24 (the bytes in memory order); an index at or
// above palettesize is 0, 0, 0, 255 (LodePNG's lodepng_color_mode_alloc_palette).
ZMX_PD_HD inline uint32_t PngPaletteRgba(const unsigned char* f, const PngWalkRecord& R, uint32_t i) {
  if (!R.has_plte || i >= R.palettesize) return 0xff000000u;
  const unsigned char* const p = f + R.plte_offset + 3 * static_cast<uint64_t>(i);
  const uint32_t a = i < R.trns_length ? f[R.trns_offset + i] : 255u;
  return p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (a << 24);
}

// ---- the sizes
// What the pixels take: _OWN rows of linebytes back to back, _RGBA8 four bytes a pixel.
ZMX_PD_HD inline uint64_t PngOutSize(uint32_t mode, uint32_t width, uint32_t height, uint32_t colortype, uint32_t depth) {
  if (mode == kPngDecRgba8) return 4ull * width * height;
  return PngLineBytes(width, PngBpp(colortype, depth)) * height;
}

// ---- the unfilter
ZMX_PD_HD inline uint32_t PngPaeth(uint32_t a, uint32_t b, uint32_t c) {   // LodePNG's paethPredictor
  const int32_t ia = static_cast<int32_t>(a), ib = static_cast<int32_t>(b), ic = static_cast<int32_t>(c);
  int32_t pa = ib - ic, pb = ia - ic, pc = ia + ib - ic - ic;
  pa = pa < 0 ? -pa : pa;
  pb = pb < 0 ? -pb : pb;
  pc = pc < 0 ? -pc : pc;
  uint32_t best = a;
  if (pb < pa) { best = b; pa = pb; }
  return pc < pa ? c : best;
}
ZMX_PD_HD inline uint32_t PngRecon(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  switch (type) {
    case 1: return (x + a) & 255;
    case 2: return (x + b) & 255;
    case 3: return (x + ((a + b) >> 1)) & 255;
    case 4: return (x + PngPaeth(a, b, c)) & 255;
    default: return x;
  }
}

struct PngUnfilterJob {
  PngWalkRecord rec;          // the header, the key, where PLTE and tRNS lie
  const unsigned char* file;  // (for the palette)
  const unsigned char* scan;  // height * (1 + linebytes) bytes; the aligned word around any of them may be read
  unsigned char* out;
  uint64_t limit;             // no byte at or beyond out + limit is stored
  unsigned char* carry[2];    // the wide path's rows, linebytes each; null: the LDS row
  uint32_t mode, index;       // kPngDecOwn / kPngDecRgba8; the caller's number of the file (the host's)
};
struct PngUnfilterResult { uint32_t status, row; };
struct PngUnfilterScratch {   // a wave's LDS
  unsigned char carry[kPngCarryBytes];
  uint32_t palette[256];
};

struct PngLane {
  uint64_t cur, shifted, up;  // the group just made (the next one's "left"); lane - 1's `cur`; the group above
  uint64_t opos;              // where in `out` the next byte goes
  uint32_t word, type;        // the aligned input word last loaded; the row's filter type
  uint32_t acc, nacc;         // the bytes gathered for the destination word in hand, by their place in it
};

// The byte at p through the lane's word: loaded when p enters a new aligned word (or `fresh`).
template <class Par>
ZMX_PD_HD inline uint32_t PngScanByte(PngLane* L, const unsigned char* p, bool fresh, const Par& par) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(p);
  if (fresh || (at & 3) == 0) {
    L->word = *reinterpret_cast<const uint32_t*>(at & ~static_cast<uintptr_t>(3));
    par.NoteRead(p, 1);
  }
  return (L->word >> (8 * (at & 3))) & 255;
}

// The gathered bytes — the last of them at out + opos - 1 — go out: one 32-bit store where the word is whole, else singly.
template <class Par>
ZMX_PD_HD inline void PngFlush(PngLane* L, const PngUnfilterJob& job, const Par& par) {
  if (L->nacc == 0) return;
  const uint64_t first = L->opos - L->nacc;
  unsigned char* const p = job.out + first;
  if (L->nacc == 4 && L->opos <= job.limit) {
    *reinterpret_cast<uint32_t*>(p) = L->acc;    // (nacc = 4 only when p is word-aligned: PngEmit flushes at a word's last byte)
    par.NoteWrite(p, 4);
  } else {
    for (uint32_t k = 0; k < L->nacc; ++k) {
      if (first + k >= job.limit) break;
      p[k] = static_cast<unsigned char>(L->acc >> (8 * (reinterpret_cast<uintptr_t>(p + k) & 3)));
      par.NoteWrite(p + k, 1);
    }
  }
  L->acc = 0;
  L->nacc = 0;
}
template <class Par>
ZMX_PD_HD inline void PngEmit(PngLane* L, const PngUnfilterJob& job, uint32_t byte, const Par& par) {
  const uint32_t place = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(job.out + L->opos) & 3);
  L->acc |= byte << (8 * place);
  ++L->nacc;
  ++L->opos;
  if (place == 3) PngFlush(L, job, par);
}
template <class Par>
ZMX_PD_HD inline void PngEmit4(PngLane* L, const PngUnfilterJob& job, uint32_t rgba, const Par& par) {
  for (uint32_t k = 0; k < 4; ++k) PngEmit(L, job, (rgba >> (8 * k)) & 255, par);
}

// One pixel of depth >= 8 as lodepng_decode32 gives it; `g` holds the group's bytes, the first in its low byte.
ZMX_PD_HD inline uint32_t PngRgba8Wide(const PngWalkRecord& R, uint64_t g, const uint32_t* palette) {
  const uint32_t b0 = static_cast<uint32_t>(g) & 255, b1 = static_cast<uint32_t>(g >> 8) & 255, b2 = static_cast<uint32_t>(g >> 16) & 255,
                 b3 = static_cast<uint32_t>(g >> 24) & 255, b4 = static_cast<uint32_t>(g >> 32) & 255, b5 = static_cast<uint32_t>(g >> 40) & 255,
                 b6 = static_cast<uint32_t>(g >> 48) & 255;
  const bool deep = R.bitdepth == 16;
  uint32_t r, gr, b, a = 255;
  switch (R.colortype) {
    case 0: {
      r = gr = b = b0;
      const uint32_t v = deep ? 256u * b0 + b1 : b0;
      if (R.has_key && v == R.key_r) a = 0;
      break;
    }
    case 2: {
      r = b0;
      gr = deep ? b2 : b1;
      b = deep ? b4 : b2;
      const uint32_t vr = deep ? 256u * b0 + b1 : b0, vg = deep ? 256u * b2 + b3 : b1, vb = deep ? 256u * b4 + b5 : b2;
      if (R.has_key && vr == R.key_r && vg == R.key_g && vb == R.key_b) a = 0;
      break;
    }
    case 3: return palette[b0];
    case 4:
      r = gr = b = b0;
      a = deep ? b2 : b1;
      break;
    default:
      r = b0;
      gr = deep ? b2 : b1;
      b = deep ? b4 : b2;
      a = deep ? b6 : b3;
      break;
  }
  return r | (gr << 8) | (b << 16) | (a << 24);
}
// One pixel of depth 1, 2 or 4 (grey or palette) of value v.
ZMX_PD_HD inline uint32_t PngRgba8Narrow(const PngWalkRecord& R, uint32_t v, const uint32_t* palette) {
  if (R.colortype == 3) return palette[v];
  const uint32_t grey = v * 255 / ((1u << R.bitdepth) - 1);
  const uint32_t a = R.has_key && v == R.key_r ? 0u : 255u;
  return grey | (grey << 8) | (grey << 16) | (a << 24);
}

// The unfilter of bands [band_first, band_first + band_count) of one image by one wave.  Par: Each(f) runs f(lane, PngLane*)
// for the 64 lanes; Shift() gives every lane its lower neighbour's `cur` in `shifted`; FirstLane(pred) the lowest lane
// whose pred(lane, PngLane*) holds, 64 for none; Sync() orders band against band.
template <class Par>
ZMX_PD_HD inline void PngUnfilterBands(const PngUnfilterJob& job, PngUnfilterScratch* S, uint32_t band_first, uint32_t band_count, Par& par,
                                       PngUnfilterResult* result) {
  const PngWalkRecord& R = job.rec;
  const uint32_t bpp = PngBpp(R.colortype, R.bitdepth);
  const uint64_t linebytes = PngLineBytes(R.width, bpp);
  const uint32_t bw = PngByteWidth(bpp);
  const uint64_t groups = linebytes / bw;       // (a row is whole groups: below 8 bits a group is a byte)
  const uint32_t bands = (R.height + kPngDecLanes - 1) / kPngDecLanes;
  const bool rgba = job.mode == kPngDecRgba8;
  const bool wide = job.carry[0] != nullptr;
  if (rgba && R.colortype == 3) {
    par.Each([&](uint32_t lane, PngLane*) {
      for (uint32_t i = lane; i < 256; i += kPngDecLanes) S->palette[i] = PngPaletteRgba(job.file, R, i);
    });
    par.Sync();
  }
  // (what is valid of a row's last byte below 8 bits)
  const uint32_t last_bits = bpp < 8 ? static_cast<uint32_t>(static_cast<uint64_t>(R.width) * bpp - 8 * (linebytes - 1)) : 8;
  const uint32_t last_mask = (0xffu << (8 - last_bits)) & 0xffu;
  const uint32_t per_byte = bpp < 8 ? 8 / bpp : 1;
  for (uint32_t band = band_first; band < bands && band - band_first < band_count; ++band) {
    const uint32_t row0 = band * kPngDecLanes;
    const uint32_t rows = R.height - row0 < kPngDecLanes ? R.height - row0 : kPngDecLanes;
    const unsigned char* const carry_in = wide ? job.carry[(band + 1) & 1] : S->carry;
    unsigned char* const carry_out = wide ? job.carry[band & 1] : S->carry;
    par.Each([&](uint32_t lane, PngLane* L) {
      *L = PngLane{};
      if (lane >= rows) return;
      const uint64_t row = row0 + lane;
      L->type = PngScanByte(L, job.scan + row * (1 + linebytes), true, par);
      L->opos = rgba ? 4ull * R.width * row : linebytes * row;
    });
    const uint32_t bad = par.FirstLane([&](uint32_t lane, PngLane* L) { return lane < rows && L->type > 4; });
    if (bad < kPngDecLanes) {
      result->status = kPngDecFilter;
      result->row = row0 + bad;
      return;
    }
    const uint64_t steps = groups + rows - 1;
    for (uint64_t t = 0; t < steps; ++t) {
      par.Shift();
      par.Each([&](uint32_t lane, PngLane* L) {
        if (lane >= rows || t < lane || t - lane >= groups) return;
        const uint64_t g = t - lane;
        const uint64_t row = row0 + lane;
        // ---- the neighbours: left is the group just made, above-left the group that was above it
        const uint64_t left = g == 0 ? 0 : L->cur;
        const uint64_t upleft = g == 0 ? 0 : L->up;
        uint64_t up = 0;
        if (lane != 0) {
          up = L->shifted;
        } else if (band != 0) {
          for (uint32_t k = 0; k < bw; ++k) up |= static_cast<uint64_t>(carry_in[g * bw + k]) << (8 * k);
        }
        L->up = up;
        // ---- the group
        const unsigned char* const in = job.scan + row * (1 + linebytes) + 1 + g * bw;
        uint64_t cur = 0;
        for (uint32_t k = 0; k < bw; ++k) {
          const uint32_t x = PngScanByte(L, in + k, false, par);
          const uint32_t v = PngRecon(L->type, x, static_cast<uint32_t>(left >> (8 * k)) & 255, static_cast<uint32_t>(up >> (8 * k)) & 255,
                                      static_cast<uint32_t>(upleft >> (8 * k)) & 255);
          cur |= static_cast<uint64_t>(v) << (8 * k);
        }
        L->cur = cur;
        if (lane == kPngDecLanes - 1) {
          for (uint32_t k = 0; k < bw; ++k) carry_out[g * bw + k] = static_cast<unsigned char>(cur >> (8 * k));
        }
        // ---- the store
        const bool last = g + 1 == groups;
        if (!rgba) {
          for (uint32_t k = 0; k < bw; ++k) {
            uint32_t v = static_cast<uint32_t>(cur >> (8 * k)) & 255;
            if (last && bpp < 8) v &= last_mask;
            PngEmit(L, job, v, par);
          }
        } else if (bpp >= 8) {
          PngEmit4(L, job, PngRgba8Wide(R, cur, S->palette), par);
        } else {
          const uint32_t byte = static_cast<uint32_t>(cur) & 255;
          for (uint32_t j = 0; j < per_byte; ++j) {
            if (g * per_byte + j >= R.width) break;
            const uint32_t v = (byte >> (8 - bpp * (j + 1))) & ((1u << bpp) - 1);
            PngEmit4(L, job, PngRgba8Narrow(R, v, S->palette), par);
          }
        }
        if (last) PngFlush(L, job, par);
      });
    }
    par.Sync();
  }
}

}  // namespace zamd

#ifdef ZMX_PNG_DECODE_KERNELS

struct PngChunksParams {
  const zamd::PngFileRef* files;
  zamd::PngWalkRecord* records;   // [slot]
  zamd::PngChunkEntry* entries;
  u32* palettes;                  // [slot][256]: written for a file that has a PLTE and walked to its end
  u32 nfiles;
};

__global__ __launch_bounds__(64) void k_png_chunks(PngChunksParams P) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.nfiles) return;
  const zamd::PngFileRef F = P.files[i];
  zamd::PngWalkRecord R;
  zamd::PngWalk(F.file, F.size, F.entry_cap, P.entries + F.entry_first, &R);
  P.records[F.slot] = R;
  if (R.has_plte && (R.status == zamd::kPngDecOk || R.status == zamd::kPngDecInterlace)) {
    for (u32 e = 0; e < R.palettesize; ++e) P.palettes[256 * static_cast<u64>(F.slot) + e] = zamd::PngPaletteRgba(F.file, R, e);
  }
}

struct PngUnfilterParams {
  const zamd::PngUnfilterJob* jobs;
  zamd::PngUnfilterResult* results;   // zeroed before the first launch
  u32 njobs, band_first, band_count;
};

// The 64 lanes of the wave side by side, each with its state in registers.
struct PngDevicePar {
  zamd::PngLane lane_state;
  template <class F>
  __device__ void Each(F f) { f(threadIdx.x, &lane_state); }
  __device__ void Shift() {
    lane_state.shifted = __shfl_up(static_cast<unsigned long long>(lane_state.cur), 1);
  }
  template <class F>
  __device__ u32 FirstLane(F pred) {
    const unsigned long long mask = __ballot(pred(threadIdx.x, &lane_state) ? 1 : 0);
    return mask ? static_cast<u32>(__ffsll(mask) - 1) : zamd::kPngDecLanes;
  }
  __device__ void Sync() const { __syncthreads(); }
  __device__ void NoteRead(const void*, u64) const {}
  __device__ void NoteWrite(const void*, u64) const {}
};

__global__ __launch_bounds__(64) void k_png_unfilter(PngUnfilterParams P) {
  __shared__ zamd::PngUnfilterScratch S;
  if (blockIdx.x >= P.njobs) return;
  if (P.results[blockIdx.x].status != zamd::kPngDecOk) return;   // (the wide path: a band before this one found a bad filter byte)
  const zamd::PngUnfilterJob job = P.jobs[blockIdx.x];
  zamd::PngUnfilterResult r = {zamd::kPngDecOk, 0};
  PngDevicePar par;
  zamd::PngUnfilterBands(job, &S, P.band_first, P.band_count, par, &r);
  if (threadIdx.x == 0 && r.status != zamd::kPngDecOk) P.results[blockIdx.x] = r;
}

#endif  // ZMX_PNG_DECODE_KERNELS

#endif  // ZMX_PNG_DECODE_H_
