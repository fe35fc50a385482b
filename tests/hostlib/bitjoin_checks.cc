// The host-only rules behind zmx_bitjoin_device and zmx_compress_bound, as a program (tests/test_cpu_bitjoin_rules.py):
//   bitjoin_checks pieces TOTAL_BITS DST_CAPACITY [SRC SRC_BIT NBITS DST_BIT]...   zamd::CheckBitPieces (host/entry_checks.h)
//   bitjoin_checks apart PIECE DST DST_BYTES SRC_LO SRC_HI                         zamd::CheckBitPieceApart
//   bitjoin_checks bound FORMAT INSIZE                                             zamd::CompressBound (host/device_output_plan.h)
// SRC, DST, SRC_LO, SRC_HI are addresses as decimal numbers (0: null); nothing is read through them.  Prints the
// refusal's message, or "ok", or the bound.
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
  std::string msg;
  if (!std::strcmp(argv[1], "pieces") && argc >= 4 && (argc - 4) % 4 == 0) {
    std::vector<zmx_bit_piece> pieces;
    for (int i = 4; i < argc; i += 4) {
      pieces.push_back({reinterpret_cast<const void*>(static_cast<uintptr_t>(num(i))), num(i + 1), num(i + 2), num(i + 3)});
    }
    msg = zamd::CheckBitPieces("zmx_bitjoin_device", pieces.size(), pieces.empty() ? nullptr : pieces.data(), num(2), num(3));
  } else if (!std::strcmp(argv[1], "apart") && argc == 7) {
    msg = zamd::CheckBitPieceApart("zmx_bitjoin_device", num(2), num(3), num(4), num(5), num(6));
  } else if (!std::strcmp(argv[1], "bound") && argc == 4) {
    std::printf("%zu\n", zamd::CompressBound(static_cast<ZopfliFormat>(num(2)), num(3)));
    return 0;
  } else {
    return 2;
  }
  std::printf("%s\n", msg.empty() ? "ok" : msg.c_str());
  return 0;
}
