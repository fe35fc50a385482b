// Model (CPU) of the parallel formulation k_png_brute (zopfli_amd/csrc/device/zmx_png_brute.h) uses for LodePNG's
// LFS_BRUTE_FORCE row search (lodepng.cpp:5585-5632): the zlib size of one filtered scanline under LodePNG's fixed-tree
// deflate (encodeLZ77, :1593-1740), computed as
//   1. per position p: the hash H[p] (getHash, :1544-1561) and the zero count Z[p] (countZeros where H[p] == 0, else 0);
//   2. per position p: the value C[p] that inserting p writes into chain[p & M] — the slot of the last q < p with the
//      same hash, or, when there is none, what the slot already held (C[p - W], or the slot itself when p < W); the same
//      CZ[p] for chainz under the key Z;
//   3. per position, independently: LodePNG's match search with the state "positions 0..pos inserted", where slot s
//      holds what its latest position pos - ((pos - s) & M) wrote (the initial state when that is below 0);
//   4. one serial lazy-matching scan over the (length, offset) results, summing fixed-code bits (:2029-2072).
// Plain C++ with nothing of LodePNG in it: tools/models/png_brute_model.cc holds it against lodepng_zlib_compress, and
// tests/hostlib/png_brute_print.cc prints it for the suite.  PngBruteModelRules states the rules a wrong kernel would most
// likely get wrong; the default is LodePNG's, and only the suite's program ever sets another.
#ifndef ZMX_PNG_BRUTE_MODEL_H_
#define ZMX_PNG_BRUTE_MODEL_H_

#include <cstddef>
#include <vector>

namespace png_brute_model {

struct Rules {
  bool lazy_258_everywhere = false;   // wrong: maxlazymatch 258 at every window (LodePNG: 64 below 8192)
  unsigned zero_cap = 258;            // wrong: 257
  bool no_far_3_rule = false;         // wrong: a match of 3 at an offset above 4096 is emitted (LodePNG: a literal)
  unsigned tail_shift = 8;            // wrong: 4 (the short hash of the last two positions shifts by 8 per byte)
  bool keep_is_self = false;          // wrong: a link that keeps what its slot held always reads the slot's own number
  bool no_nicematch = false;          // wrong: the search goes on after a match of 128 or more
};

struct Size {
  size_t bits;    // 3 + the symbols under the fixed code + 7
  size_t bytes;   // 2 + ceil(bits / 8) + 4: the zlib stream
};

const unsigned kKeep = 0xffffu;

inline unsigned HashAt(const unsigned char* f, size_t n, size_t p, unsigned tail_shift = 8) {
  if (p + 2 < n) return (f[p] ^ (f[p + 1] << 4u) ^ (f[p + 2] << 8u)) & 65535u;
  unsigned r = 0;
  for (size_t i = 0; p + i < n; ++i) r ^= static_cast<unsigned>(f[p + i]) << (tail_shift * i);
  return r & 65535u;
}

inline unsigned LengthExtra(unsigned l) { return (l <= 10 || l == 258) ? 0 : (31 - __builtin_clz(l - 3)) - 2; }
inline unsigned DistExtra(unsigned d) { return d <= 4 ? 0 : (31 - __builtin_clz(d - 1)) - 1; }
inline unsigned LitBits(unsigned c) { return c < 144 ? 8 : 9; }

inline Size ModelSize(const unsigned char* f, size_t n, unsigned W, const Rules& rules = Rules()) {
  const unsigned M = W - 1, maxchain = W >= 8192 ? W : W / 8, nice = 128;
  const unsigned maxlazy = (W >= 8192 || rules.lazy_258_everywhere) ? 258 : 64;
  std::vector<unsigned> H(n), Z(n), C(n), CZ(n), L(n), D(n);
  // 1. hash and zero count (the zero runs from their starts, then masked by H == 0)
  for (size_t p = 0; p < n; ++p) H[p] = HashAt(f, n, p, rules.tail_shift);
  {
    unsigned run = 0;   // the zeros from p on
    for (size_t p = n; p-- > 0;) {
      run = f[p] == 0 ? run + 1 : 0;
      Z[p] = H[p] == 0 ? (run < rules.zero_cap ? run : rules.zero_cap) : 0;
    }
  }
  // 2. the chain links: last earlier position with the same key, else KEEP, resolved per residue class
  std::vector<long> head(65536, -1), headz(259, -1);
  for (size_t p = 0; p < n; ++p) {
    C[p] = head[H[p]] >= 0 ? static_cast<unsigned>(head[H[p]]) & M : kKeep;
    CZ[p] = headz[Z[p]] >= 0 ? static_cast<unsigned>(headz[Z[p]]) & M : kKeep;
    head[H[p]] = static_cast<long>(p);
    headz[Z[p]] = static_cast<long>(p);
  }
  for (size_t r = 0; r < n && r < W; ++r) {
    unsigned pc = static_cast<unsigned>(r), pz = static_cast<unsigned>(r);
    for (size_t p = r; p < n; p += W) {
      if (C[p] == kKeep) C[p] = pc;
      if (CZ[p] == kKeep) CZ[p] = pz;
      if (!rules.keep_is_self) {
        pc = C[p];
        pz = CZ[p];
      }
    }
  }
  // 3. the search at every position on its own
  for (size_t pos = 0; pos < n; ++pos) {
    const unsigned wpos = static_cast<unsigned>(pos) & M, hv = H[pos], nz = Z[pos];
    const size_t last = n < pos + 258 ? n : pos + 258;
    auto at = [&](unsigned s) { return static_cast<long>(pos) - static_cast<long>((wpos - s) & M); };  // slot's owner
    unsigned length = 0, offset = 0, hashpos = C[pos], prev_offset = 0, chainlength = 0;
    for (;;) {
      if (chainlength++ >= maxchain) break;
      const unsigned cur = hashpos <= wpos ? wpos - hashpos : wpos - hashpos + W;
      if (cur < prev_offset) break;
      prev_offset = cur;
      const long q = at(hashpos);
      if (cur > 0) {
        size_t fo = pos, ba = pos - cur;
        if (nz >= 3) {
          unsigned skip = Z[q];
          if (skip > nz) skip = nz;
          fo += skip;
          ba += skip;
        }
        while (fo != last && f[ba] == f[fo]) { ++fo; ++ba; }
        const unsigned cl = static_cast<unsigned>(fo - pos);
        if (cl > length) {
          length = cl;
          offset = cur;
          if (cl >= nice && !rules.no_nicematch) break;
        }
      }
      const unsigned chainv = q >= 0 ? C[q] : hashpos;
      if (hashpos == chainv) break;
      if (nz >= 3 && length > nz) {
        hashpos = q >= 0 ? CZ[q] : hashpos;
        const long q2 = at(hashpos);
        if (q2 < 0 || Z[q2] != nz) break;
      } else {
        hashpos = chainv;
        const long q2 = at(hashpos);
        if (q2 < 0 || H[q2] != hv) break;
      }
    }
    L[pos] = length;
    D[pos] = offset;
  }
  // 4. the lazy scan
  size_t bits = 3 + 7;
  unsigned lazy = 0, ll = 0, lo = 0;
  for (size_t pos = 0; pos < n; ++pos) {
    unsigned length = L[pos], offset = D[pos];
    if (!lazy && length >= 3 && length <= maxlazy && length < 258) { lazy = 1; ll = length; lo = offset; continue; }
    if (lazy) {
      lazy = 0;
      if (length > ll + 1) bits += LitBits(f[pos - 1]);
      else { length = ll; offset = lo; --pos; }
    }
    if (length < 3 || (length == 3 && offset > 4096 && !rules.no_far_3_rule)) bits += LitBits(f[pos]);
    else {
      bits += (length <= 114 ? 7 : 8) + LengthExtra(length) + 5 + DistExtra(offset);
      pos += length - 1;
    }
  }
  return Size{bits, 6 + (bits + 7) / 8};
}

}  // namespace png_brute_model

#endif  // ZMX_PNG_BRUTE_MODEL_H_
