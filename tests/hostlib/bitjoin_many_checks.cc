// The host-only rules behind zmx_bitjoin_many_device and the packed form of zmx_compress_device_batch_packed, as a program
// (tests/test_cpu_bitjoin_many_rules.py):
//   bitjoin_many_checks dests NDST NPIECES [DST TOTAL_BITS FIRST_PIECE NPIECES CAPACITY]... [SRC SRC_BIT NBITS DST_BIT]...
//                                              zamd::CheckBitDests (host/entry_checks.h); with NDST or NPIECES non-zero and no
//                                              entry at all: null tables.  CAPACITY -1 in the first destination: a null
//                                              capacity array (every destination has exactly its bytes)
//   bitjoin_many_checks offsets ALIGN SIZE...  zamd::PackedOffsets (host/device_output_plan.h): the offsets, then the end
//   bitjoin_many_checks align ALIGN            zamd::PackedAlignOk: "ok" or "bad"
//   bitjoin_many_checks bound FORMAT ALIGN INSIZE...   zamd::CompressBatchBound
// DST and SRC are addresses as decimal numbers (0: null); nothing is read through them.  Prints the refusal's message, or
// "ok", or the numbers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_output_plan.h"
#include "entry_checks.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const auto num = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
  if (!std::strcmp(argv[1], "dests") && argc >= 4) {
    const size_t ndst = num(2), npieces = num(3);
    std::string msg;
    if (argc == 4) {
      msg = zamd::CheckBitDests<zmx_bit_dest, zmx_bit_piece>("zmx_bitjoin_many_device", ndst, nullptr, nullptr, npieces, nullptr);
    } else {
      if (static_cast<size_t>(argc) != 4 + 5 * ndst + 4 * npieces) return 2;
      std::vector<zmx_bit_dest> dests;
      std::vector<size_t> capacity;
      std::vector<zmx_bit_piece> pieces;
      int i = 4;
      const bool exact = ndst != 0 && !std::strcmp(argv[4 + 4], "-1");
      for (size_t d = 0; d < ndst; ++d, i += 5) {
        dests.push_back({reinterpret_cast<void*>(static_cast<uintptr_t>(num(i))), num(i + 1), num(i + 2), num(i + 3)});
        capacity.push_back(exact ? 0 : num(i + 4));
      }
      for (size_t p = 0; p < npieces; ++p, i += 4) {
        pieces.push_back({reinterpret_cast<const void*>(static_cast<uintptr_t>(num(i))), num(i + 1), num(i + 2), num(i + 3)});
      }
      msg = zamd::CheckBitDests("zmx_bitjoin_many_device", ndst, dests.empty() ? nullptr : dests.data(), exact ? nullptr : capacity.data(),
                                npieces, pieces.empty() ? nullptr : pieces.data());
    }
    std::printf("%s\n", msg.empty() ? "ok" : msg.c_str());
    return 0;
  }
  if (!std::strcmp(argv[1], "offsets") && argc >= 3) {
    std::vector<size_t> size, offset;
    for (int i = 3; i < argc; ++i) size.push_back(num(i));
    offset.resize(size.size());
    const size_t end = zamd::PackedOffsets(size.size(), size.data(), num(2), offset.data());
    for (size_t v : offset) std::printf("%zu ", v);
    std::printf("%zu\n", end);
    return 0;
  }
  if (!std::strcmp(argv[1], "align") && argc == 3) {
    std::printf("%s\n", zamd::PackedAlignOk(num(2)) ? "ok" : "bad");
    return 0;
  }
  if (!std::strcmp(argv[1], "bound") && argc >= 4) {
    std::vector<size_t> insize;
    for (int i = 4; i < argc; ++i) insize.push_back(num(i));
    std::printf("%zu\n", zamd::CompressBatchBound(static_cast<ZopfliFormat>(num(2)), insize.size(), insize.data(), num(3)));
    return 0;
  }
  return 2;
}
