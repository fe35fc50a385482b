// Which (litlen, dist) pairs are LZ77 symbols (lz77.h:44-49; the reference asserts these in ZopfliStoreLitLenDist,
// lz77.c:119, and in its symbol lookups): what zmx_cost_stores_create_host lets through to the device, where a symbol
// is an index into a wave's histogram.
//   dist == 0   a literal: litlen <= 255
//   dist != 0   a match:   3 <= litlen <= 258, 1 <= dist <= 32768
#pragma once
#include <cstddef>
#include <cstdint>

#include "symbols.h"

namespace zamd {

inline bool ValidSymbol(uint16_t litlen, uint16_t dist) {
  return dist == 0 ? litlen <= 255 : (litlen >= kMinMatch && litlen <= kMaxMatch && dist <= kWindow);
}

// the index of the first pair of litlens[0 .. n), dists[0 .. n) that is no symbol, or n
inline size_t FirstInvalidSymbol(const uint16_t* litlens, const uint16_t* dists, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (!ValidSymbol(litlens[i], dists[i])) return i;
  }
  return n;
}

}  // namespace zamd
