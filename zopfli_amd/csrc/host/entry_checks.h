// What the zmx_* entries refuse of their arguments before they touch anything: the rules and their texts, as plain
// functions that the device layer (device/drv_tables.h, a part of zmx_hip.hip) and the host test library's stand-in for it
// (tests/hostlib/zmx_oracle_backend.cc) both run.  No HIP, no globals: each function returns the refusal's message —
// `who`, the entry's name, then ": ", then the text — or an empty string when there is nothing to refuse.  Either side
// turns a message into its own ZMX_ERR_REFUSED.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "symbols.h"

namespace zamd {

inline std::string Refusal(const char* who, const std::string& text) { return std::string(who) + ": " + text; }

// ---- the tables an entry is handed
enum TableNeeds {
  kAnyTables,     // the stores are enough (they survive zmx_tables_trim)
  kUntrimmed,     // ... the match records and what goes with them
  kWithDp,        // ... and DP rows, codes, windows and tasks (not zmx_tables_build_matches)
};
inline std::string CheckTables(const char* who, bool exist, bool trimmed, bool matches_only, TableNeeds needs) {
  if (!exist) return Refusal(who, "no tables");
  if (needs >= kUntrimmed && trimmed) return Refusal(who, "these tables were trimmed to their stores (zmx_tables_trim)");
  if (needs >= kWithDp && matches_only) return Refusal(who, "these tables hold matches only (zmx_tables_build_matches)");
  return std::string();
}
// zmx_squeeze_run: tables of no block have nothing to run, whatever they were built with
inline TableNeeds SqueezeRunNeeds(size_t nblocks) { return nblocks == 0 ? kUntrimmed : kWithDp; }

// ---- a block, and symbols [0, nsym) of the store in `slot` of `block`
inline std::string CheckBlock(const char* who, size_t nblocks, size_t block) {
  return block < nblocks ? std::string() : Refusal(who, "bad block");
}
// capacity(): how many symbols the store can hold from where it begins (asked only of a block and slot that exist)
template <class Capacity>
inline std::string CheckStoreRef(const char* who, size_t nblocks, size_t block, int slot, size_t nsym, Capacity capacity) {
  if (block >= nblocks || (slot != 0 && slot != 1)) return Refusal(who, "bad block or slot");
  if (nsym > capacity()) return Refusal(who, "nsym exceeds the store");
  return std::string();
}

// ---- the length arrays of zmx_trace_length_arrays
// What the trace kernels cannot bound themselves: a cell h may hold 0 (GetBestLengths never reached it), 1 or a length
// 3 .. min(h, 258) — a step back from h that stays inside the block, so cell 0 holds 0 alone.
inline bool PathCell(size_t h, unsigned v) {
  const size_t longest = h < static_cast<size_t>(kMaxMatch) ? h : static_cast<size_t>(kMaxMatch);
  return v <= longest && (v <= 1 || v >= static_cast<unsigned>(kMinMatch));
}
// bsize(b): the bytes of block b of the tables, which have table_blocks of them
template <class BlockSize>
inline std::string CheckLengthArrays(const char* who, size_t table_blocks, BlockSize bsize, size_t nblocks,
                                     const uint16_t* const* length_arrays, const size_t* entries, const int32_t* slot) {
  if (nblocks != table_blocks) return Refusal(who, "one length array per block of the tables");
  for (size_t b = 0; b < nblocks; ++b) {
    const size_t B = bsize(b);
    if (slot[b] != 0 && slot[b] != 1) return Refusal(who, "slot must be 0 or 1");
    if (entries[b] != B + 1) {
      return Refusal(who, "block " + std::to_string(b) + " has " + std::to_string(B) + " + 1 cells, not " + std::to_string(entries[b]));
    }
    for (size_t h = 0; h <= B; ++h) {
      const unsigned v = length_arrays[b][h];
      if (!PathCell(h, v)) {
        return Refusal(who, "block " + std::to_string(b) + ", cell " + std::to_string(h) + " holds " + std::to_string(v) + ": no step of a path");
      }
    }
  }
  return std::string();
}

// ---- the piece table of zmx_bitjoin_device (device/zmx_bitjoin.h)
// What needs no runtime: the table itself.  Piece: zmx_bit_piece { src, src_bit, nbits, dst_bit }.  The pieces are sorted by
// dst_bit and none — an empty one included — begins before the one in front of it ends; no number reaches 2^60 bits, so no
// sum of two overflows.
constexpr uint64_t kBitPieceMaxBits = 1ull << 60;
template <class Piece>
inline std::string CheckBitPieces(const char* who, size_t n, const Piece* pieces, uint64_t total_bits, uint64_t dst_capacity) {
  if (n != 0 && pieces == nullptr) return Refusal(who, "null piece table");
  uint64_t end = 0;
  for (size_t i = 0; i < n; ++i) {
    const Piece& q = pieces[i];
    const std::string piece = "piece " + std::to_string(i);
    if (q.src_bit >= kBitPieceMaxBits || q.nbits >= kBitPieceMaxBits || q.dst_bit >= kBitPieceMaxBits) {
      return Refusal(who, piece + ": a bit count of 2^60 or more");
    }
    if (q.nbits != 0 && q.src == nullptr) return Refusal(who, piece + ": null pointer with a non-zero size");
    if (q.dst_bit < end) {
      return Refusal(who, piece + (i != 0 && q.dst_bit < pieces[i - 1].dst_bit ? ": the pieces are not sorted by dst_bit"
                                                                                 : ": it overlaps the piece before it"));
    }
    end = q.dst_bit + q.nbits;
  }
  if (total_bits < end) return Refusal(who, "total_bits " + std::to_string(total_bits) + " is below the last piece's end, " + std::to_string(end));
  if (total_bits / 8 > dst_capacity || (total_bits / 8 == dst_capacity && total_bits % 8 != 0)) {
    return Refusal(who, "total_bits " + std::to_string(total_bits) + " is above 8 * dst_capacity, " + std::to_string(dst_capacity) + " bytes");
  }
  return std::string();
}
// The bytes that hold a bit of a piece, as addresses [*lo, *hi) (nbits != 0).
template <class Piece>
inline void BitPieceBytes(const Piece& q, uintptr_t* lo, uintptr_t* hi) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(q.src);
  *lo = at + static_cast<uintptr_t>(q.src_bit / 8);
  *hi = at + static_cast<uintptr_t>((q.src_bit + q.nbits + 7) / 8);
}
// The destination dst[0, dst_bytes) may not share a byte with piece i's [src_lo, src_hi).
inline std::string CheckBitPieceApart(const char* who, size_t i, uintptr_t dst, uint64_t dst_bytes, uintptr_t src_lo, uintptr_t src_hi) {
  if (src_lo < dst + dst_bytes && dst < src_hi) return Refusal(who, "piece " + std::to_string(i) + ": the destination overlaps this source");
  return std::string();
}

// ---- the destinations of zmx_bitjoin_many_device and of zmx_compress_device_batch_to_device
// Byte ranges [lo, hi) that may not share a byte, each with the number its owner knows it by.  Sorted once, so that a
// thousand destinations against ten thousand sources are no product: Add, then Sort, then Overlap and Hit.
class ApartRanges {
 public:
  void Add(uintptr_t lo, uintptr_t hi, size_t id) {
    if (lo < hi) ranges_.push_back({lo, hi, id});
  }
  void Sort() {
    std::sort(ranges_.begin(), ranges_.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
  }
  // two ranges that share a byte (the later one in address order in *b), when there are any
  bool Overlap(size_t* a, size_t* b) const {
    for (size_t i = 1; i < ranges_.size(); ++i) {
      if (ranges_[i].lo < ranges_[i - 1].hi) {
        *a = ranges_[i - 1].id;
        *b = ranges_[i].id;
        return true;
      }
    }
    return false;
  }
  // a range that shares a byte with [lo, hi), when there is one (the ranges being apart: Overlap said so)
  bool Hit(uintptr_t lo, uintptr_t hi, size_t* id) const {
    if (lo >= hi) return false;
    // the last range that begins below hi: the ones in front of it end at or below its lo
    auto it = std::lower_bound(ranges_.begin(), ranges_.end(), hi, [](const Range& r, uintptr_t v) { return r.lo < v; });
    if (it == ranges_.begin() || (it - 1)->hi <= lo) return false;
    *id = (it - 1)->id;
    return true;
  }

 private:
  struct Range { uintptr_t lo, hi; size_t id; };
  std::vector<Range> ranges_;
};

// What zmx_bitjoin_many_device refuses of its tables without asking the runtime.  Dest: zmx_bit_dest { dst, total_bits,
// first_piece, npieces }; destination d has capacity[d] bytes (capacity null: exactly (total_bits + 7) / 8).  The piece
// ranges are consecutive and end at npieces; each destination's pieces follow CheckBitPieces; no two destinations share
// a byte, and no piece's source bytes share one with any destination.
template <class Dest, class Piece>
inline std::string CheckBitDests(const char* who, size_t ndst, const Dest* dests, const size_t* capacity, size_t npieces,
                                 const Piece* pieces) {
  if (ndst != 0 && dests == nullptr) return Refusal(who, "null destination table");
  if (npieces != 0 && pieces == nullptr) return Refusal(who, "null piece table");
  uint64_t next = 0;
  for (size_t d = 0; d < ndst; ++d) {
    const std::string dest = "destination " + std::to_string(d);
    if (dests[d].first_piece != next) return Refusal(who, dest + ": its pieces do not follow those of the destination before it");
    if (dests[d].npieces > npieces - next) return Refusal(who, dest + ": its pieces leave the table of " + std::to_string(npieces));
    next += dests[d].npieces;
  }
  if (next != npieces) return Refusal(who, "the destinations take " + std::to_string(next) + " pieces of " + std::to_string(npieces));
  ApartRanges apart;
  for (size_t d = 0; d < ndst; ++d) {
    const Dest& e = dests[d];
    const std::string dest = std::string(who) + ": destination " + std::to_string(d);
    if (e.total_bits >= kBitPieceMaxBits) return Refusal(dest.c_str(), "a bit count of 2^60 or more");
    const uint64_t nbytes = (e.total_bits + 7) / 8;
    const std::string msg = CheckBitPieces(dest.c_str(), static_cast<size_t>(e.npieces), e.npieces ? pieces + e.first_piece : nullptr,
                                           e.total_bits, capacity ? capacity[d] : nbytes);
    if (!msg.empty()) return msg;
    if (nbytes != 0 && e.dst == nullptr) return Refusal(dest.c_str(), "null pointer with a non-zero size");
    const uintptr_t at = reinterpret_cast<uintptr_t>(e.dst);
    apart.Add(at, at + static_cast<uintptr_t>(nbytes), d);
  }
  apart.Sort();
  size_t a = 0, b = 0;
  if (apart.Overlap(&a, &b)) {
    return Refusal(who, "destination " + std::to_string(std::max(a, b)) + " overlaps destination " + std::to_string(std::min(a, b)));
  }
  for (size_t d = 0; d < ndst; ++d) {
    for (uint64_t i = 0; i < dests[d].npieces; ++i) {
      const Piece& q = pieces[dests[d].first_piece + i];
      if (q.nbits == 0) continue;
      uintptr_t lo = 0, hi = 0;
      BitPieceBytes(q, &lo, &hi);
      if (apart.Hit(lo, hi, &a)) {
        return Refusal(who, "destination " + std::to_string(d) + ": piece " + std::to_string(i) + ": destination " + std::to_string(a) +
                                " overlaps this source");
      }
    }
  }
  return std::string();
}

}  // namespace zamd
