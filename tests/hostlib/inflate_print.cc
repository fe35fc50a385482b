// The rules of device/zmx_inflate.h as a plain C++ program (tests/test_cpu_inflate_cases.py): the kernel's own walk,
// InflateWalk, with the 64 lanes run one after the other.  No device.
//   inflate_print
//     stdin: lines "FORMAT CAPACITY IN_SHIFT OUT_SHIFT HEX" — FORMAT 0 gzip, 1 zlib, 2 deflate (ZopfliFormat); CAPACITY
//     the destination's bytes, or "null" for the size-only mode; the stream's first byte IN_SHIFT bytes and the
//     destination's OUT_SHIFT bytes behind a 16-byte boundary; HEX the stream ("-": empty).  Both buffers are heap blocks
//     that end with the range, so that a sanitizer sees a byte too many.  Per line it prints
//       "STATUS OUTSIZE CONSUMED BLOCK STORED_CHECK STORED_ISIZE OUT_CRC READ_LO READ_HI WRITE_LO WRITE_HI"
//     the result's fields; the CRC-32 of the min(OUTSIZE, CAPACITY) bytes stored; the lowest and one past the highest
//     byte read, relative to the stream's first, and written, relative to the destination's ("- -": none).
//   inflate_print constants
//     prints "RING STRETCH LIT_ROOT DIST_ROOT SCRATCH_BYTES".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "zmx_inflate.h"

namespace {

struct HostPar {
  mutable const unsigned char *read_lo = nullptr, *read_hi = nullptr, *write_lo = nullptr, *write_hi = nullptr;
  template <class F>
  void Each(F f) const {
    for (uint32_t lane = 0; lane < zamd::kInflateLanes; ++lane) f(lane);
  }
  uint32_t U32(uint32_t v) const { return v; }
  static void Note(const unsigned char* p, uint64_t n, const unsigned char** lo, const unsigned char** hi) {
    if (n == 0) return;
    if (!*lo || p < *lo) *lo = p;
    if (!*hi || p + n > *hi) *hi = p + n;
  }
  void NoteRead(const void* p, uint64_t n) const { Note(static_cast<const unsigned char*>(p), n, &read_lo, &read_hi); }
  void NoteWrite(const void* p, uint64_t n) const { Note(static_cast<const unsigned char*>(p), n, &write_lo, &write_hi); }
};

uint32_t Crc32(const unsigned char* p, size_t n) {
  uint32_t crc = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc & 1) ? (crc >> 1) ^ 0xedb88320u : crc >> 1;
  }
  return ~crc;
}

// a heap block of shift + n bytes that begins at a 16-byte boundary
unsigned char* Block(size_t shift, size_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, shift + n ? shift + n : 1) != 0) std::abort();
  return static_cast<unsigned char*>(p);
}

int Nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

void Range(const unsigned char* lo, const unsigned char* hi, const unsigned char* base) {
  if (!lo) std::printf(" - -");
  else std::printf(" %lld %lld", static_cast<long long>(lo - base), static_cast<long long>(hi - base));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "constants") == 0) {
    std::printf("%u %u %u %u %zu\n", zamd::kInflateRing, zamd::kInflateStretch, zamd::kInflateLitRoot, zamd::kInflateDistRoot,
                sizeof(zamd::InflateScratch));
    return 0;
  }
  if (argc != 1) {
    std::fprintf(stderr, "usage: inflate_print [constants]\n");
    return 2;
  }
  zamd::InflateScratch* scratch = new zamd::InflateScratch;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream fields(line);
    unsigned format = 0;
    std::string capacity, hex;
    size_t in_shift = 0, out_shift = 0;
    if (!(fields >> format >> capacity >> in_shift >> out_shift >> hex) || in_shift > 15 || out_shift > 15) return 2;
    if (hex == "-") hex.clear();
    if (hex.size() % 2) return 2;
    const size_t n = hex.size() / 2;
    unsigned char* const in_block = Block(in_shift, n);
    for (size_t i = 0; i < n; ++i) {
      const int hi = Nibble(hex[2 * i]), lo = Nibble(hex[2 * i + 1]);
      if (hi < 0 || lo < 0) return 2;
      in_block[in_shift + i] = static_cast<unsigned char>(hi * 16 + lo);
    }
    const bool size_only = capacity == "null";
    const size_t cap = size_only ? 0 : std::strtoull(capacity.c_str(), nullptr, 10);
    unsigned char* const out_block = Block(out_shift, cap);
    std::memset(out_block, 0xa5, out_shift + cap);
    // (the scratch begins every case as the last one left it, as a wave's LDS does)
    zamd::InflateJob job = {in_block + in_shift, n, size_only ? nullptr : out_block + out_shift, cap, 0};
    zamd::InflateResult r;
    HostPar par;
    zamd::InflateWalk(format, job, scratch, par, &r);
    const size_t stored = size_only ? 0 : r.outsize < cap ? static_cast<size_t>(r.outsize) : cap;
    std::printf("%u %llu %llu %u %u %u %u", r.status, static_cast<unsigned long long>(r.outsize), static_cast<unsigned long long>(r.consumed),
                r.block, r.stored_check, r.stored_isize, Crc32(out_block + out_shift, stored));
    Range(par.read_lo, par.read_hi, in_block + in_shift);
    Range(par.write_lo, par.write_hi, out_block + out_shift);
    std::printf("\n");
    std::free(in_block);
    std::free(out_block);
  }
  delete scratch;
  return 0;
}
