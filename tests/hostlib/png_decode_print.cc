// The rules of device/zmx_png_decode.h and host/png_decode_plan.h as a plain C++ program (tests/test_cpu_png_decode_cases.py):
// the kernels' own walks — PngWalk, PngUnfilterBands with its shift, band carry and fused stores, and k_inflate's InflateWalk
// between them — with the 64 lanes run one after the other, in the order the driver (device/drv_png_decode.h) runs them.
// No device.
//   png_decode_print
//     stdin: lines "MODE CAPACITY IN_SHIFT OUT_SHIFT FORCE_WIDE ENTRY_CAP HEX" — MODE 0 own, 1 rgba8; CAPACITY the
//     destination's bytes, or "null" for the size-only mode; the file's first byte IN_SHIFT bytes and the destination's
//     OUT_SHIFT bytes behind a 16-byte boundary; FORCE_WIDE 0 / 1; ENTRY_CAP the chunk entries of the first walk (0: the
//     header's own); HEX the file ("-": empty).  File and destination are heap blocks that end with the range, so that a
//     sanitizer sees a byte too many.  Per line it prints
//       "STATUS DETAIL WIDTH HEIGHT COLORTYPE BITDEPTH INTERLACE PALETTESIZE HAS_KEY KEY_R KEY_G KEY_B OUTSIZE OUTSIZE_OWN
//        OUTSIZE_RGBA8 PALETTE_CRC OUT_CRC WRITE_LO WRITE_HI WALKS WIDE"
//     the result's fields; the CRC-32 of the result's palette and of the outsize bytes stored (0 where nothing was); the
//     lowest and one past the highest byte written, relative to the destination's first ("- -": none); how often the file
//     was walked; whether the wide path ran.
//   png_decode_print constants
//     prints "CARRY_BYTES ENTRIES SCRATCH_BYTES RESULT_BYTES".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "png_decode_plan.h"
#include "zmx_inflate.h"
#include "zmx_png_decode.h"

namespace {

struct InflatePar {
  template <class F>
  void Each(F f) const {
    for (uint32_t lane = 0; lane < zamd::kInflateLanes; ++lane) f(lane);
  }
  uint32_t U32(uint32_t v) const { return v; }
  void NoteRead(const void*, uint64_t) const {}
  void NoteWrite(const void*, uint64_t) const {}
};

// The 64 lanes one after the other, each with its own state; the shift takes every lane's value before any lane moves on.
struct UnfilterPar {
  zamd::PngLane lanes[zamd::kPngDecLanes];
  mutable const unsigned char *write_lo = nullptr, *write_hi = nullptr;
  template <class F>
  void Each(F f) {
    for (uint32_t lane = 0; lane < zamd::kPngDecLanes; ++lane) f(lane, &lanes[lane]);
  }
  void Shift() {
    for (uint32_t lane = zamd::kPngDecLanes - 1; lane > 0; --lane) lanes[lane].shifted = lanes[lane - 1].cur;
  }
  template <class F>
  uint32_t FirstLane(F pred) {
    for (uint32_t lane = 0; lane < zamd::kPngDecLanes; ++lane) {
      if (pred(lane, &lanes[lane])) return lane;
    }
    return zamd::kPngDecLanes;
  }
  void Sync() const {}
  void NoteRead(const void*, uint64_t) const {}
  void NoteWrite(const void* p, uint64_t n) const {
    const unsigned char* const q = static_cast<const unsigned char*>(p);
    if (!write_lo || q < write_lo) write_lo = q;
    if (!write_hi || q + n > write_hi) write_hi = q + n;
  }
};

uint32_t Crc32(const unsigned char* p, size_t n) {
  uint32_t crc = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc & 1) ? (crc >> 1) ^ 0xedb88320u : crc >> 1;
  }
  return ~crc;
}
uint32_t Adler32(const unsigned char* p, size_t n) {
  uint32_t a = 1, b = 0;
  for (size_t i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521;
    b = (b + a) % 65521;
  }
  return (b << 16) | a;
}

// a heap block of shift + n bytes that begins at a 16-byte boundary
unsigned char* Block(size_t shift, size_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, shift + n ? shift + n : 1) != 0) std::abort();
  return static_cast<unsigned char*>(p);
}
size_t Align16(size_t v) { return (v + 15) & ~size_t{15}; }

int Nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "constants") == 0) {
    std::printf("%u %u %zu %zu\n", zamd::kPngCarryBytes, zamd::kPngDecEntries, sizeof(zamd::PngUnfilterScratch), sizeof(zmx_png_decode_result));
    return 0;
  }
  if (argc != 1) {
    std::fprintf(stderr, "usage: png_decode_print [constants]\n");
    return 2;
  }
  zamd::InflateScratch* const inflate_scratch = new zamd::InflateScratch;
  zamd::PngUnfilterScratch* const scratch = new zamd::PngUnfilterScratch;
  UnfilterPar* const par = new UnfilterPar;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream fields(line);
    int mode = 0, force_wide = 0;
    unsigned entry_cap = 0;
    std::string capacity, hex;
    size_t in_shift = 0, out_shift = 0;
    if (!(fields >> mode >> capacity >> in_shift >> out_shift >> force_wide >> entry_cap >> hex) || in_shift > 15 || out_shift > 15) return 2;
    if (hex == "-") hex.clear();
    if (hex.size() % 2) return 2;
    const size_t n = hex.size() / 2;
    unsigned char* const in_block = Block(in_shift, n);
    unsigned char* const file = in_block + in_shift;
    for (size_t i = 0; i < n; ++i) {
      const int hi = Nibble(hex[2 * i]), lo = Nibble(hex[2 * i + 1]);
      if (hi < 0 || lo < 0) return 2;
      file[i] = static_cast<unsigned char>(hi * 16 + lo);
    }
    const bool size_only = capacity == "null";
    const size_t cap = size_only ? 0 : std::strtoull(capacity.c_str(), nullptr, 10);
    unsigned char* const out_block = Block(out_shift, cap);
    unsigned char* const out = out_block + out_shift;
    std::memset(out_block, 0xa5, out_shift + cap);
    *par = UnfilterPar();
    // ---- the walk, again with room where the first had too little
    const uint32_t cap0 = entry_cap ? entry_cap : zamd::kPngDecEntries;
    std::vector<zamd::PngChunkEntry> ent(cap0);
    zamd::PngWalkRecord rec;
    zamd::PngWalk(file, n, cap0, ent.data(), &rec);
    int walks = 1;
    if (rec.nentries > cap0) {
      ent.assign(rec.nentries, zamd::PngChunkEntry{});
      zamd::PngWalk(file, n, rec.nentries, ent.data(), &rec);
      ++walks;
    }
    ent.resize(rec.nentries);
    uint32_t palette[256] = {0};
    if (rec.has_plte && (rec.status == zamd::kPngDecOk || rec.status == zamd::kPngDecInterlace)) {
      for (uint32_t e = 0; e < rec.palettesize; ++e) palette[e] = zamd::PngPaletteRgba(file, rec, e);
    }
    zmx_png_decode_result result;
    zamd::PngResultFromWalk(rec, mode, rec.has_plte ? palette : nullptr, &result);
    uint64_t scan = 0;
    if (zamd::PngHeaderKnown(rec) && !zamd::PngScanBytes(rec, &scan)) return 3;
    bool wide = false;
    // ---- the CRCs
    if (result.status == ZMX_PNG_DECODE_OK) {
      std::vector<uint32_t> computed(ent.size());
      for (size_t k = 0; k < ent.size(); ++k) computed[k] = Crc32(file + ent[k].offset + 4, static_cast<size_t>(ent[k].length) + 4);
      zamd::PngCrcVerdict(ent.data(), computed.data(), static_cast<uint32_t>(ent.size()), &result);
    }
    // ---- the stream
    unsigned char* scan_block = nullptr;
    if (result.status == ZMX_PNG_DECODE_OK) {
      std::vector<unsigned char> idat;
      for (const zamd::PngChunkEntry& e : ent) {
        if (e.kind == zamd::kPngChunkIdat) idat.insert(idat.end(), file + e.offset + 8, file + e.offset + 8 + e.length);
      }
      if (idat.empty()) {
        result.status = ZMX_PNG_DECODE_STREAM;
        result.detail = ZMX_INFLATE_TRUNCATED;
      } else {
        // (the stream in a block that ends with it; the scanlines in a slice that begins at a 16-byte boundary and ends on
        // whole words, as the driver's)
        unsigned char* const stream = Block(0, idat.size());
        std::memcpy(stream, idat.data(), idat.size());
        if (!size_only) {
          scan_block = Block(0, Align16(static_cast<size_t>(scan)));
          std::memset(scan_block, 0x5a, Align16(static_cast<size_t>(scan)));
        }
        zamd::InflateJob job = {stream, idat.size(), scan_block, scan, 0};
        zamd::InflateResult r;
        zamd::InflateWalk(zamd::kInflateZlib, job, inflate_scratch, InflatePar(), &r);
        const zmx_inflate_result got = {r.outsize, r.consumed, r.status, r.block, r.stored_check, r.stored_isize};
        zamd::PngStreamVerdict(got, scan, &result);
        if (result.status == ZMX_PNG_DECODE_OK && !size_only && Adler32(scan_block, static_cast<size_t>(scan)) != r.stored_check) {
          result.status = ZMX_PNG_DECODE_STREAM;
          result.detail = ZMX_INFLATE_CHECKSUM;
        }
        std::free(stream);
      }
    }
    // ---- the unfilter
    if (result.status == ZMX_PNG_DECODE_OK && !size_only) {
      if (result.outsize > cap) {
        result.status = ZMX_PNG_DECODE_CAPACITY;
      } else {
        const size_t linebytes = static_cast<size_t>(zamd::PngLineBytes(rec.width, zamd::PngBpp(rec.colortype, rec.bitdepth)));
        wide = force_wide || linebytes > zamd::kPngCarryBytes;
        zamd::PngUnfilterJob J;
        J.rec = rec;
        J.file = file;
        J.scan = scan_block;
        J.out = out;
        J.limit = result.outsize;
        unsigned char* const carry = wide ? Block(0, 2 * Align16(linebytes)) : nullptr;
        J.carry[0] = carry;
        J.carry[1] = carry ? carry + Align16(linebytes) : nullptr;
        J.mode = static_cast<uint32_t>(mode);
        J.index = 0;
        zamd::PngUnfilterResult u = {zamd::kPngDecOk, 0};
        // (the scratch begins every case as the last one left it, as a wave's LDS does)
        if (!wide) {
          zamd::PngUnfilterBands(J, scratch, 0, 0xffffffffu, *par, &u);
        } else {
          const uint32_t bands = (rec.height + zamd::kPngDecLanes - 1) / zamd::kPngDecLanes;
          for (uint32_t b = 0; b < bands && u.status == zamd::kPngDecOk; ++b) zamd::PngUnfilterBands(J, scratch, b, 1, *par, &u);
        }
        if (u.status != zamd::kPngDecOk) {
          result.status = u.status;
          result.detail = u.row;
        }
        std::free(carry);
      }
    }
    const bool whole = result.status == ZMX_PNG_DECODE_OK && !size_only;
    std::printf("%u %u %u %u %u %u %u %u %u %u %u %u %llu %llu %llu %u %u", result.status, result.detail, result.width, result.height, result.colortype,
                result.bitdepth, result.interlace, result.palettesize, result.has_key, result.key_r, result.key_g, result.key_b,
                static_cast<unsigned long long>(result.outsize), static_cast<unsigned long long>(result.outsize_own),
                static_cast<unsigned long long>(result.outsize_rgba8), Crc32(result.palette, sizeof(result.palette)),
                whole ? Crc32(out, static_cast<size_t>(result.outsize)) : 0u);
    if (!par->write_lo) std::printf(" - -");
    else std::printf(" %lld %lld", static_cast<long long>(par->write_lo - out), static_cast<long long>(par->write_hi - out));
    std::printf(" %d %d\n", walks, wide ? 1 : 0);
    std::free(scan_block);
    std::free(in_block);
    std::free(out_block);
  }
  delete par;
  delete scratch;
  delete inflate_scratch;
  return 0;
}
