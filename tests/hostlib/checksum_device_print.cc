// The plain-C++ rules of device/zmx_checksum_device.h and the PNG frame of host/device_output_plan.h as a program
// (tests/test_cpu_checksum_device_rules.py), linked with checksum.cc.  No device.
//   checksum_device_print sums
//     stdin: lines "FILL LEN SHIFT" — LEN bytes of FILL (zeros | ones: 0xFF | random: a generator seeded with LEN), the
//     range beginning SHIFT (0 .. 3) bytes behind a 4-byte-aligned address.  Per line it prints
//       "NPIECES CRC ADLER SEALED_CRC_HEX BASE_OFFSET"
//     what the piece split, the device combine and the finish give: the pieces come from a host loop that mimics
//     k_checksum_pieces — boundaries counted from the range's END, the leftmost piece short (its missing leading bytes
//     being zeros, which change nothing) —, the values from ChecksumFinishRange, the kernel's own code; SEALED: the four
//     bytes ChecksumSeal writes for the CRC; BASE_OFFSET: what ChecksumAlignedBase says of the range's first byte.
//     The test makes the same bytes with the same generator (Fill below) and asks zlib.
//   checksum_device_print frame WIDTH HEIGHT COLORTYPE BITDEPTH IDAT_BYTES
//     prints "HEADER_HEX TAIL_HEX": PngFrameHeader of PngPrefix's bytes with the IDAT's length filled in by
//     PngFrameSetLength, and the bytes PngFrameTrailer puts behind the Adler-32; "refused" (exit status 1) when the
//     length does not fit a chunk.
//   checksum_device_print bound WIDTH HEIGHT COLORTYPE BITDEPTH
//     prints zamd::PngBound and the scanlines' size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_output_plan.h"
#include "zmx_checksum_device.h"

namespace {

// the test's generator (tests/test_cpu_checksum_device_rules.py: _random_bytes)
void Fill(const std::string& fill, std::vector<unsigned char>* bytes, size_t shift) {
  uint32_t x = static_cast<uint32_t>(bytes->size() - shift) * 2654435761u + 12345u;
  for (size_t i = shift; i < bytes->size(); ++i) {
    if (fill == "zeros") (*bytes)[i] = 0;
    else if (fill == "ones") (*bytes)[i] = 0xff;
    else {
      x = x * 1664525u + 1013904223u;
      (*bytes)[i] = static_cast<unsigned char>(x >> 24);
    }
  }
}

// One piece as the kernel leaves it: the bytes [lo, hi) of `in`, hi the piece's end.
zamd::ChecksumPiece PieceOf(const unsigned char* in, long long lo, long long hi) {
  uint32_t crc = 0;
  uint64_t sum = 0, wsum = 0;
  for (long long p = lo; p < hi; ++p) {
    crc ^= in[p];
    for (int k = 0; k < 8; ++k) crc = (crc & 1) ? (crc >> 1) ^ zamd::kCrcPoly : crc >> 1;
    sum = (sum + in[p]) % zamd::kAdlerBase;
    wsum = (wsum + static_cast<uint64_t>(hi - p) % zamd::kAdlerBase * in[p]) % zamd::kAdlerBase;
  }
  return {crc, static_cast<uint32_t>(sum), static_cast<uint32_t>(wsum)};
}

int Sums() {
  char fill[32];
  unsigned long long len = 0, shift = 0;
  const uint32_t xpiece = zamd::Gf2XPow8(zamd::kChecksumPieceBytes);
  while (std::scanf("%31s %llu %llu", fill, &len, &shift) == 3) {
    if (shift > 3) return 2;
    // (over-aligned storage, so that SHIFT is the range's distance from a 4-byte boundary)
    std::vector<uint32_t> words((len + shift + 3) / 4 + 1, 0xa5a5a5a5u);
    std::vector<unsigned char> bytes(len + shift, 0xa5);
    Fill(fill, &bytes, shift);
    unsigned char* store = reinterpret_cast<unsigned char*>(words.data());
    std::memcpy(store, bytes.data(), bytes.size());
    zamd::ChecksumRange R;
    R.p = store + shift;
    R.len = len;
    R.first_piece = 0;
    R.npieces = zamd::ChecksumPieces(len);
    R.seal = nullptr;
    R.xlen = zamd::Gf2XPow8(len);
    R.pad = 0;
    long long begin = 0;
    const unsigned char* base = zamd::ChecksumAlignedBase(R.p, &begin);
    const long long end = begin + static_cast<long long>(len);
    std::vector<zamd::ChecksumPiece> pieces(R.npieces);
    for (uint64_t j = 0; j < R.npieces; ++j) {
      const long long hi = end - static_cast<long long>(j) * zamd::kChecksumPieceBytes;
      long long lo = hi - static_cast<long long>(zamd::kChecksumPieceBytes);
      if (lo < begin) lo = begin;
      pieces[j] = PieceOf(base, lo, hi);
    }
    const uint32_t crc = zamd::ChecksumFinishRange(zamd::kChecksumDeviceCrc, R, pieces.data(), xpiece);
    const uint32_t adler = zamd::ChecksumFinishRange(zamd::kChecksumDeviceAdler, R, pieces.data(), xpiece);
    unsigned char sealed[4];
    zamd::ChecksumSeal(crc, sealed);
    std::printf("%llu %u %u %02x%02x%02x%02x %lld\n", static_cast<unsigned long long>(R.npieces), crc, adler, sealed[0], sealed[1], sealed[2],
                sealed[3], begin);
  }
  return 0;
}

void Hex(const std::vector<uint8_t>& v) {
  for (uint8_t b : v) std::printf("%02x", b);
}

int Frame(char** argv) {
  const uint32_t width = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10));
  const uint32_t height = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  const uint32_t colortype = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
  const uint32_t bitdepth = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  const uint64_t idat = std::strtoull(argv[6], nullptr, 10);
  zamd::PngFrame frame;
  frame.file_prefix.resize(zamd::kPngPrefixBytes);
  zamd::PngPrefix(width, height, colortype, bitdepth, frame.file_prefix.data());
  zamd::OutputPlan plan;
  plan.literals = zamd::PngFrameHeader(frame);
  plan.total_bits = 8 * (frame.file_prefix.size() + idat + zamd::kPngTrailerBytes);
  if (!zamd::PngFrameSetLength(frame, &plan)) {
    std::printf("refused\n");
    return 1;
  }
  Hex(plan.literals);
  std::printf(" ");
  Hex(zamd::PngFrameTrailer({}));
  std::printf("\n");
  return 0;
}

int Bound(char** argv) {
  const uint32_t width = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10));
  const uint32_t height = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  const uint32_t colortype = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
  const uint32_t bitdepth = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  std::printf("%zu %zu\n", zamd::PngBound(width, height, colortype, bitdepth),
              static_cast<size_t>(height) * (zamd::PngLineBytes(width, colortype, bitdepth) + 1));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "sums") == 0) return Sums();
  if (argc == 7 && std::strcmp(argv[1], "frame") == 0) return Frame(argv);
  if (argc == 6 && std::strcmp(argv[1], "bound") == 0) return Bound(argv);
  std::fprintf(stderr, "usage: checksum_device_print sums | frame W H CT DEPTH IDAT | bound W H CT DEPTH\n");
  return 2;
}
