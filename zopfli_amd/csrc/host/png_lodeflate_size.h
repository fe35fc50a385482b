// The size of a deflate block as LodePNG's deflateDynamic writes it (lodepng.cpp:1807-2027), from the block's symbol
// counts alone: what zmx_png_deflate_sizes_device does on the host with the histograms k_png_lo_parse brings down.
// A restatement in the project's own words (as oracle/zopfli_oracle.c is for zopfli); tools/models/png_lodeflate_model.cc
// holds it against lodepng_zlib_compress.  The exact code lengths matter, not only their cost: the tree's own encoding
// depends on them, so the length-limited code is LodePNG's boundary package-merge with its tie behaviour
// (lodepng_huffman_code_lengths, :967-1043), not zopfli's.  Plain C++, no device code.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zamd {

constexpr unsigned kLoNumLl = 286, kLoNumD = 30, kLoNumCl = 19;

// One deflate block's parse in numbers: how often each literal/length and distance symbol is used (ll[256] is set by
// the reader, whatever it holds) and the sum of the length and distance extra bits.
struct LoBlockCounts {
  uint32_t ll[kLoNumLl];
  uint32_t d[kLoNumD];
  uint64_t extra_bits;
};

// LodePNG's blocks of a buffer of `insize` bytes (lodepng_deflatev, :2086-2094).
inline size_t LoBlockSize(size_t insize) {
  size_t b = insize / 8u + 8u;
  if (b < 65536u) b = 65536u;
  if (b > 262144u) b = 262144u;
  return b;
}
inline size_t LoNumBlocks(size_t insize) {
  const size_t b = LoBlockSize(insize), k = (insize + b - 1) / b;
  return k ? k : 1;
}

// Length-limited code lengths, LodePNG's way: the symbols in use sorted by count (a stable sort: equal counts stay in
// symbol order), then the boundary package-merge of Katajainen, Moffat and Turpin with two look-ahead chains per list.
// Where a package and the next leaf weigh the same the package is taken (`sum > leaf` takes the leaf).  No symbol in
// use: lengths[0] = lengths[1] = 1; one: that symbol and symbol 0 (or 1) get one bit each.
inline void LoCodeLengths(const uint32_t* counts, size_t numcodes, unsigned maxbits, unsigned* lengths) {
  struct Leaf { int weight; unsigned symbol; };
  struct Chain { int weight; unsigned leaves; int tail; };   // `leaves`: how many of the sorted leaves the chain's head covers
  std::vector<Leaf> leaf;
  for (size_t i = 0; i < numcodes; ++i) {
    lengths[i] = 0;
    if (counts[i] > 0) leaf.push_back({static_cast<int>(counts[i]), static_cast<unsigned>(i)});
  }
  const size_t present = leaf.size();
  if (present == 0) {
    lengths[0] = lengths[1] = 1;
    return;
  }
  if (present == 1) {
    lengths[leaf[0].symbol] = 1;
    lengths[leaf[0].symbol == 0 ? 1 : 0] = 1;
    return;
  }
  std::stable_sort(leaf.begin(), leaf.end(), [](const Leaf& a, const Leaf& b) { return a.weight < b.weight; });
  std::vector<Chain> pool;
  pool.reserve(2 * present * maxbits + 8);
  pool.push_back({leaf[0].weight, 1, -1});
  pool.push_back({leaf[1].weight, 2, -1});
  std::vector<int> older(maxbits, 0), newer(maxbits, 1);
  const long wanted = static_cast<long>(2 * present - 2);
  struct Step {
    std::vector<Chain>& pool;
    std::vector<int>& older;
    std::vector<int>& newer;
    const std::vector<Leaf>& leaf;
    long wanted;
    void Run(int list, long round) {
      const unsigned covered = pool[newer[list]].leaves;
      const size_t present = leaf.size();
      if (list == 0) {
        if (covered >= present) return;
        older[0] = newer[0];
        pool.push_back({leaf[covered].weight, covered + 1, -1});
        newer[0] = static_cast<int>(pool.size()) - 1;
        return;
      }
      const int package = pool[older[list - 1]].weight + pool[newer[list - 1]].weight;
      older[list] = newer[list];
      if (covered < present && package > leaf[covered].weight) {
        pool.push_back({leaf[covered].weight, covered + 1, pool[newer[list]].tail});
        newer[list] = static_cast<int>(pool.size()) - 1;
        return;
      }
      pool.push_back({package, covered, newer[list - 1]});
      newer[list] = static_cast<int>(pool.size()) - 1;
      if (round + 1 < wanted) {   // (the last round's lower lists are never looked at again)
        Run(list - 1, round);
        Run(list - 1, round);
      }
    }
  } step{pool, older, newer, leaf, wanted};
  for (long round = 2; round != wanted; ++round) step.Run(static_cast<int>(maxbits) - 1, round);
  for (int at = newer[maxbits - 1]; at >= 0; at = pool[at].tail) {
    for (unsigned k = 0; k < pool[at].leaves; ++k) ++lengths[leaf[k].symbol];
  }
}

// HuffmanTree_makeFromFrequencies' (:1046) trim: trailing unused symbols go, down to `mincodes`.
inline size_t LoTrimmedCodes(const uint32_t* counts, size_t numcodes, size_t mincodes) {
  while (numcodes > mincodes && counts[numcodes - 1] == 0) --numcodes;
  return numcodes;
}

// What deflateDynamic makes of a block's counts, for the tests to look at: the two trees' lengths, the code-length
// tree's lengths and how many of them are written.
struct LoBlockTrees {
  unsigned ll[kLoNumLl], d[kLoNumD], cl[kLoNumCl];
  size_t numcodes_ll, numcodes_d, numcodes_cl;
  uint64_t tree_bits;   // 14 + 3 * numcodes_cl + the run-length coded lengths
};

// The bits of one dynamic block: 3 of header, the trees, the symbols, their extra bits and the end code.
inline uint64_t LoDynamicBlockBits(const LoBlockCounts& in, LoBlockTrees* trees_out = nullptr) {
  static const unsigned kClOrder[kLoNumCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  LoBlockCounts c = in;
  c.ll[256] = 1;   // exactly one end code
  LoBlockTrees t = LoBlockTrees();
  t.numcodes_ll = LoTrimmedCodes(c.ll, kLoNumLl, 257);
  t.numcodes_d = LoTrimmedCodes(c.d, kLoNumD, 2);
  LoCodeLengths(c.ll, t.numcodes_ll, 15, t.ll);
  LoCodeLengths(c.d, t.numcodes_d, 15, t.d);
  // the two trees' lengths joined, then run-length coded LodePNG's way (:1910-1942): three or more zeros become 17
  // (up to 10) or 18 (up to 138); a non-zero value followed by j >= 3 repeats is written once, then 16s of six, then a
  // 16 for a rest of 3 .. 5; a rest below 3 is left for the next round, which writes it out plainly.
  std::vector<unsigned> joined(t.ll, t.ll + t.numcodes_ll);
  joined.insert(joined.end(), t.d, t.d + t.numcodes_d);
  const size_t total = joined.size();
  uint32_t cl_counts[kLoNumCl] = {0};
  uint64_t repeat_bits = 0;
  for (size_t i = 0; i < total; ++i) {
    size_t same = 0;
    while (i + same + 1 < total && joined[i + same + 1] == joined[i]) ++same;
    if (joined[i] == 0 && same >= 2) {
      size_t run = same + 1;
      if (run <= 10) {
        ++cl_counts[17];
        repeat_bits += 3;
      } else {
        if (run > 138) run = 138;
        ++cl_counts[18];
        repeat_bits += 7;
      }
      i += run - 1;
    } else if (same >= 3) {
      const size_t sixes = same / 6, rest = same % 6;
      ++cl_counts[joined[i]];
      cl_counts[16] += static_cast<uint32_t>(sixes);
      repeat_bits += 2 * sixes;
      if (rest >= 3) {
        ++cl_counts[16];
        repeat_bits += 2;
        i += same;
      } else {
        i += same - rest;
      }
    } else {
      ++cl_counts[joined[i]];
    }
  }
  LoCodeLengths(cl_counts, kLoNumCl, 7, t.cl);
  t.numcodes_cl = kLoNumCl;
  while (t.numcodes_cl > 4 && t.cl[kClOrder[t.numcodes_cl - 1]] == 0) --t.numcodes_cl;
  t.tree_bits = 14 + 3 * t.numcodes_cl + repeat_bits;
  for (unsigned s = 0; s < kLoNumCl; ++s) t.tree_bits += static_cast<uint64_t>(cl_counts[s]) * t.cl[s];
  uint64_t bits = 3 + t.tree_bits + c.extra_bits;
  for (size_t s = 0; s < t.numcodes_ll; ++s) bits += static_cast<uint64_t>(c.ll[s]) * t.ll[s];
  for (size_t s = 0; s < t.numcodes_d; ++s) bits += static_cast<uint64_t>(c.d[s]) * t.d[s];
  if (trees_out) *trees_out = t;
  return bits;
}

// lodepng_zlib_compress' length for a buffer whose blocks' counts are `blocks`: two bytes of header, the blocks end to
// end without alignment, Adler-32.
inline uint64_t LoZlibBytes(const LoBlockCounts* blocks, size_t numblocks) {
  uint64_t bits = 0;
  for (size_t b = 0; b < numblocks; ++b) bits += LoDynamicBlockBits(blocks[b]);
  return 2 + (bits + 7) / 8 + 4;
}

}  // namespace zamd
