// The match record: what the table build writes once per block position and almost every later phase reads.
//   recs[]    per block position, 8 words = 32 bytes = the ZopfliFindLongestMatch result:
//               word 0 = length | dist << 16
//               word 1 = same | literal << 16 | ncp << 24        (ncp 0..8, 0xff = overflow)
//               words 2..7: 8 change points of sublen in ascending length, a 24-bit field each, field e at bit 24 e
//               (3 bytes: len - 3, dist lo, dist hi); the fields from number ncp on are zero
//               overflow (more than 8 change points): word 2 = offset into pool[], word 3 low 16 bits = their number
//               (words 4..7 keep what they held of the first eight fields; nobody reads it)
//   pool[]    per overflow change point, u32 = len | dist << 16, a record's entries in ascending length
// sublen[len] is the distance of the first change point with a length >= len.  The record's length is its last change
// point's (a record of length < 3 has none).
// Every kernel and the host's probe pack and unpack the record through these functions; a CPU program
// (tests/hostlib/record_print.cc) runs them against a model of the comment above.  This header compiles without HIP.
#ifndef ZMX_RECORD_H_
#define ZMX_RECORD_H_

#include <stdint.h>

#if defined(__HIPCC__)
// (always inlined: a kernel compiles to the code of the expression written out in its place)
#define ZMX_RECORD_HD __host__ __device__ __attribute__((always_inline))
#else
#define ZMX_RECORD_HD
#endif

namespace zamd {

constexpr uint32_t kRecWords = 8;          // u32 per record
constexpr uint32_t kRecInlineCps = 8;      // change points a record holds itself
constexpr uint32_t kRecOverflow = 0xffu;   // word 1's count field of a record whose change points are in pool[]

// ---- the header words
ZMX_RECORD_HD inline uint32_t RecWord0(uint32_t length, uint32_t dist) { return length | (dist << 16); }
// count: the number of change points (0 .. 8), or kRecOverflow
ZMX_RECORD_HD inline uint32_t RecWord1(uint32_t same, uint32_t literal, uint32_t count) {
  return same | (literal << 16) | (count << 24);
}
ZMX_RECORD_HD inline uint32_t RecLength(uint32_t w0) { return w0 & 0xffffu; }
ZMX_RECORD_HD inline uint32_t RecDist(uint32_t w0) { return w0 >> 16; }
ZMX_RECORD_HD inline uint32_t RecSame(uint32_t w1) { return w1 & 0xffffu; }
ZMX_RECORD_HD inline uint32_t RecLiteral(uint32_t w1) { return (w1 >> 16) & 255u; }
ZMX_RECORD_HD inline uint32_t RecCount(uint32_t w1) { return w1 >> 24; }
ZMX_RECORD_HD inline bool RecIsOverflow(uint32_t w1) { return RecCount(w1) == kRecOverflow; }
ZMX_RECORD_HD inline uint32_t RecPoolOffset(uint32_t w2) { return w2; }
ZMX_RECORD_HD inline uint32_t RecPoolCount(uint32_t w3) { return w3 & 0xffffu; }

// ---- a pool entry
ZMX_RECORD_HD inline uint32_t RecPoolEntry(uint32_t length, uint32_t dist) { return length | (dist << 16); }
ZMX_RECORD_HD inline uint32_t RecPoolLength(uint32_t x) { return x & 0xffffu; }
ZMX_RECORD_HD inline uint32_t RecPoolDist(uint32_t x) { return x >> 16; }

// ---- an inline change point: a 24-bit field
ZMX_RECORD_HD inline uint32_t RecCpField(uint32_t length, uint32_t dist) { return (length - 3u) | (dist << 8); }
ZMX_RECORD_HD inline uint32_t RecCpThreshold(uint32_t f) { return f & 255u; }   // length - 3
ZMX_RECORD_HD inline uint32_t RecCpLength(uint32_t f) { return (f & 255u) + 3u; }
ZMX_RECORD_HD inline uint32_t RecCpDist(uint32_t f) { return (f >> 8) & 0xffffu; }
// (of a field with nothing above its 24 bits)
ZMX_RECORD_HD inline uint32_t RecCpPoolEntry(uint32_t f) { return ((f & 255u) + 3u) | ((f >> 8) << 16); }

// Field e (0 .. 7) of the payload w[0 .. 5] = words 2 .. 7; bits above the field's 24 may be set (RecCpLength and
// RecCpDist mask them off).
ZMX_RECORD_HD inline uint32_t RecCpFieldOfWords(const uint32_t* w, uint32_t e) {
  const uint32_t bit = 24u * e;
  const uint32_t lo32 = w[bit >> 5] >> (bit & 31);
  return (bit & 31) > 8 ? (lo32 | (w[(bit >> 5) + 1 > 5 ? 5 : (bit >> 5) + 1] << (32 - (bit & 31)))) : lo32;
}
// Eight fields v[0 .. 7], nothing above their 24 bits, packed into the payload's six words.
ZMX_RECORD_HD inline void RecCpPackFields(const uint32_t* v, uint32_t* w) {
  w[0] = v[0] | (v[1] << 24);
  w[1] = (v[1] >> 8) | (v[2] << 16);
  w[2] = (v[2] >> 16) | (v[3] << 8);
  w[3] = v[4] | (v[5] << 24);
  w[4] = (v[5] >> 8) | (v[6] << 16);
  w[5] = (v[6] >> 16) | (v[7] << 8);
}

// The payload as three 64-bit accumulators c2 : c1 : c0 (a kernel that finds the change points one at a time keeps it
// in registers like this): appending field number ncp (0 .. 7), reading field e back, the six words.
ZMX_RECORD_HD inline void RecCpAppend(uint64_t& c0, uint64_t& c1, uint64_t& c2, uint32_t ncp, uint32_t f) {
  const uint64_t v = (uint64_t)f;
  const uint32_t bit = 24u * ncp, wi = bit >> 6, sh = bit & 63u;
  const uint64_t lo = v << sh, hi = sh > 40 ? v >> (64u - sh) : 0ull;
  c0 |= wi == 0 ? lo : 0ull;
  c1 |= wi == 1 ? lo : wi == 0 ? hi : 0ull;
  c2 |= wi == 2 ? lo : wi == 1 ? hi : 0ull;
}
ZMX_RECORD_HD inline uint32_t RecCpFieldOfAcc(uint64_t c0, uint64_t c1, uint64_t c2, uint32_t e) {
  const uint32_t bit = 24u * e, wi = bit >> 6, sh = bit & 63u;
  const uint64_t a = wi == 0 ? c0 : wi == 1 ? c1 : c2, b2 = wi == 0 ? c1 : c2;
  return (uint32_t)((sh > 40 ? (a >> sh) | (b2 << (64u - sh)) : a >> sh) & 0xffffffu);
}
ZMX_RECORD_HD inline void RecCpAccWords(uint64_t c0, uint64_t c1, uint64_t c2, uint32_t* w) {
  w[0] = (uint32_t)c0; w[1] = (uint32_t)(c0 >> 32);
  w[2] = (uint32_t)c1; w[3] = (uint32_t)(c1 >> 32);
  w[4] = (uint32_t)c2; w[5] = (uint32_t)(c2 >> 32);
}

// ---- sublen[len] of a record that holds its change points itself, by thresholds (k_codes): the eight fields' length - 3
// as bytes of t0 (fields 0 .. 3) and t1 (4 .. 7), 255 from number ncp on.  RecCpThresholdPut adds field e's to t0 / t1
// (zero before the first); RecCpThresholdIndex finds the first field with a threshold >= x = len - 3 in three steps.
// Ascending thresholds and 255 behind them: a record with fewer than 8 change points whose last length is 258 resolves
// x = 255 to that change point, the first 255; an x above every threshold of a full record resolves to field 7.
ZMX_RECORD_HD inline void RecCpThresholdPut(uint32_t& t0, uint32_t& t1, uint32_t e, uint32_t ncp, uint32_t f) {
  const uint32_t thr = e < ncp ? RecCpThreshold(f) : 255u;
  if (e < 4) t0 |= thr << (8 * e); else t1 |= thr << (8 * (e - 4));
}
ZMX_RECORD_HD inline uint32_t RecCpThresholdIndex(uint32_t t0, uint32_t t1, uint32_t x) {
  uint32_t idx = ((t0 >> 24) < x) ? 4u : 0u;
  uint32_t half = idx ? t1 : t0;
  if (((half >> 8) & 255u) < x) { idx += 2; half >>= 16; }
  if ((half & 255u) < x) idx += 1;
  return idx;
}

// ---- sublen[len] of an overflow record: the index of the first of its n entries pool[off ..] with a length >= len
// (n: none)
ZMX_RECORD_HD inline uint32_t RecPoolFind(const uint32_t* pool, uint32_t off, uint32_t n, uint32_t len) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (RecPoolLength(pool[off + mid]) < len) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- a record's change points in order, wherever they are: f(length, dist) for each
// (the two halves: a record that holds its n change points itself — field e as its three bytes, little-endian words —
//  and one whose n change points are pool[off ..])
template <class F>
ZMX_RECORD_HD inline void RecWalkInlineCps(const uint32_t* rec, uint32_t n, F&& f) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(rec) + 8;
  for (uint32_t e = 0; e < n; ++e) f((uint32_t)b[3 * e] + 3u, (uint32_t)b[3 * e + 1] | ((uint32_t)b[3 * e + 2] << 8));
}
template <class F>
ZMX_RECORD_HD inline void RecWalkPoolCps(const uint32_t* pool, uint32_t off, uint32_t n, F&& f) {
  for (uint32_t e = 0; e < n; ++e) {
    const uint32_t x = pool[off + e];
    f(RecPoolLength(x), RecPoolDist(x));
  }
}
template <class F>
ZMX_RECORD_HD inline void RecWalkCps(const uint32_t* rec, const uint32_t* pool, F&& f) {
  if (!RecIsOverflow(rec[1])) RecWalkInlineCps(rec, RecCount(rec[1]), f);
  else RecWalkPoolCps(pool, RecPoolOffset(rec[2]), RecPoolCount(rec[3]), f);
}

}  // namespace zamd

#endif  // ZMX_RECORD_H_
