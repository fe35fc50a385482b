// k_inflate: n deflate / zlib / gzip streams in device memory decoded into device memory, one launch (zmx_inflate_device*,
// drv_inflate.h).  Any conforming stream, not only this library's; validity is zlib 1.2.11's (inftrees.c, inflate.c).
//   geometry     one wavefront — a workgroup of 64 lanes — walks one stream from its first bit to its last; workgroup w
//                takes jobs[w], which the host lists longest input first.  No workgroup waits for another.
//   the walk     is wave-uniform: every lane holds the same bit reservoir and takes the same branches.  The lanes part
//                only where a rule below takes a `lane`: the table build, the copy of a match or of a stored block inside
//                the window, the flush.
//   the window   a ring of kInflateRing bytes in LDS: the last 32 768 bytes of output for the matches, and in front of
//                them what is not flushed yet.  Whenever kInflateStretch bytes are pending they go to d_out: bytes up to
//                the first 16-byte boundary of the destination, 16-byte stores, bytes.  Matches are resolved in the ring,
//                never from d_out.  Nothing at or beyond d_out + capacity is stored; the walk goes on without storing, so
//                that outsize is what the stream takes (d_out null: the size-only mode).
//   the codes    a primary table a code alphabet (the next kInflateLitRoot / kInflateDistRoot bits give symbol and
//                length); a code longer than that has no entry and is found by the canonical walk over count[] and
//                sorted[] — at most 15 steps, for codes that by their length are rare.  Nothing's size depends on the
//                lengths the stream declares.
//   LDS          sizeof(InflateScratch) = 46 208 bytes a wave: three waves a CU (160 KiB).
//   bounds       every loop consumes at least one input bit a pass or leaves; no bit at or behind 8 * insize is taken
//                (InflateBits refills from [in, in + insize) alone, the last bytes one by one); ring indices are taken
//                modulo kInflateRing; a store to d_out is clipped to capacity before its split.
// Every rule is a __host__ __device__ function and the walk is a template over `Par`, which says how the 64 lanes run:
// side by side with a barrier on the device (InflateDevicePar below), one after the other in a CPU program
// (tests/hostlib/inflate_print.cc), which so runs the very code of the kernel.  The header compiles without HIP; the kernel
// is there for the device layer only (ZMX_INFLATE_KERNELS).
#ifndef ZMX_INFLATE_H_
#define ZMX_INFLATE_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZMX_INF_HD __host__ __device__
#else
#define ZMX_INF_HD
#endif

namespace zamd {

// (ZMX_INFLATE_* of include/zopfli_amd.h: drv_inflate.h holds the two against each other)
enum InflateStatus : uint32_t {
  kInflateOk = 0,
  kInflateHeader,           // a zlib or gzip header that is none
  kInflateDict,             // zlib's FDICT
  kInflateBlockType,        // block type 3
  kInflateStoredLen,        // LEN != ~NLEN
  kInflateTooManySymbols,   // HLIT > 286 or HDIST > 30
  kInflateRepeat,           // a repeat with no previous length, or past HLIT + HDIST
  kInflateOversubscribed,
  kInflateIncomplete,
  kInflateNoEndCode,        // no code for symbol 256
  kInflateBadCode,          // a bit pattern no code owns
  kInflateBadSymbol,        // literal/length 286, 287; distance 30, 31
  kInflateDistance,         // behind the first byte of the output
  kInflateTruncated,
  kInflateCapacity,
  kInflateChecksum,         // (set by the host: host/inflate.cc)
  kInflateSize,             // (likewise)
  kInflateStatuses
};

constexpr uint32_t kInflateGzip = 0, kInflateZlib = 1, kInflateDeflate = 2;   // (ZopfliFormat)
constexpr uint32_t kInflateLanes = 64;
constexpr uint32_t kInflateWindow = 32768;
constexpr uint32_t kInflateMaxMatch = 258;
constexpr uint32_t kInflateStretch = 4096;   // what one flush takes
constexpr uint32_t kInflateRing = 40960;     // >= window + stretch + 2 matches; a multiple of 16
constexpr uint32_t kInflateLitRoot = 10, kInflateDistRoot = 8;
constexpr uint32_t kInflateLitSymbols = 288, kInflateDistSymbols = 32, kInflateMaxBits = 15;
static_assert(kInflateRing >= kInflateWindow + kInflateStretch + 2 * kInflateMaxMatch, "a match never reaches what is not flushed");
static_assert(kInflateRing % 16 == 0, "the flush reads 16 bytes without a wrap inside an aligned group");

struct InflateJob {
  const unsigned char* in;
  uint64_t insize;
  unsigned char* out;     // null: size only
  uint64_t capacity;
  uint64_t index;         // the caller's number of the stream (the jobs are sorted; the host's, not read by the kernel)
};
struct InflateResult {    // (zmx_inflate_result)
  uint64_t outsize, consumed;
  uint32_t status, block, stored_check, stored_isize;
};
static_assert(sizeof(InflateResult) == 32, "32 bytes a stream");

// One canonical code: how many codes of each length, the symbols in canonical order, each symbol's code.
struct InflateCode {
  uint16_t count[kInflateMaxBits + 1];
  uint16_t sorted[kInflateLitSymbols];
  uint16_t code[kInflateLitSymbols];
};
// A wave's LDS.
struct InflateScratch {
  unsigned char ring[kInflateRing];
  uint16_t lit_table[1u << kInflateLitRoot];     // symbol << 4 | length; 0: no code of at most root bits here
  uint16_t dist_table[1u << kInflateDistRoot];
  unsigned char lens[kInflateLitSymbols + kInflateDistSymbols];
  InflateCode lit, dist;                          // (dist holds the code-length code while the lengths are read)
};

// ---- the containers
// zlib: CMF, FLG.  *pos: the first byte of the deflate data.
ZMX_INF_HD inline uint32_t InflateZlibHeader(const unsigned char* in, uint64_t insize, uint64_t* pos) {
  if (insize < 2) return kInflateTruncated;
  const uint32_t cmf = in[0], flg = in[1];
  if (((cmf << 8) | flg) % 31 != 0) return kInflateHeader;
  if ((cmf & 15) != 8 || (cmf >> 4) > 7) return kInflateHeader;
  if (flg & 0x20) return kInflateDict;
  *pos = 2;
  return kInflateOk;
}
// gzip: the ten fixed bytes, then FEXTRA, FNAME, FCOMMENT, FHCRC as FLG names them (skipped, not checked).
ZMX_INF_HD inline uint32_t InflateGzipHeader(const unsigned char* in, uint64_t insize, uint64_t* pos) {
  if (insize < 10) {
    // (what is there must still begin a header: zlib says so at the first wrong byte)
    if (insize >= 1 && in[0] != 0x1f) return kInflateHeader;
    if (insize >= 2 && in[1] != 0x8b) return kInflateHeader;
    if (insize >= 3 && in[2] != 8) return kInflateHeader;
    if (insize >= 4 && (in[3] & 0xe0)) return kInflateHeader;
    return kInflateTruncated;
  }
  if (in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || (in[3] & 0xe0)) return kInflateHeader;
  const uint32_t flg = in[3];
  uint64_t p = 10;
  if (flg & 4) {
    if (insize - p < 2) return kInflateTruncated;
    const uint64_t xlen = in[p] | (static_cast<uint64_t>(in[p + 1]) << 8);
    p += 2;
    if (insize - p < xlen) return kInflateTruncated;
    p += xlen;
  }
  for (uint32_t field = 8; field <= 16; field <<= 1) {   // FNAME, FCOMMENT: up to and including a zero byte
    if (!(flg & field)) continue;
    for (;;) {
      if (p >= insize) return kInflateTruncated;
      if (in[p++] == 0) break;
    }
  }
  if (flg & 2) {
    if (insize - p < 2) return kInflateTruncated;
    p += 2;
  }
  *pos = p;
  return kInflateOk;
}
// The trailer at byte p: gzip's CRC-32 and ISIZE (least significant byte first), zlib's Adler-32 (most significant first).
ZMX_INF_HD inline uint32_t InflateTrailer(uint32_t format, const unsigned char* in, uint64_t insize, uint64_t p, InflateResult* r) {
  const uint64_t need = format == kInflateGzip ? 8 : format == kInflateZlib ? 4 : 0;
  if (insize - p < need) return kInflateTruncated;
  if (format == kInflateGzip) {
    r->stored_check = in[p] | (static_cast<uint32_t>(in[p + 1]) << 8) | (static_cast<uint32_t>(in[p + 2]) << 16) | (static_cast<uint32_t>(in[p + 3]) << 24);
    r->stored_isize = in[p + 4] | (static_cast<uint32_t>(in[p + 5]) << 8) | (static_cast<uint32_t>(in[p + 6]) << 16) | (static_cast<uint32_t>(in[p + 7]) << 24);
  } else if (format == kInflateZlib) {
    r->stored_check = (static_cast<uint32_t>(in[p]) << 24) | (static_cast<uint32_t>(in[p + 1]) << 16) | (static_cast<uint32_t>(in[p + 2]) << 8) | in[p + 3];
  }
  r->consumed = p + need;
  return kInflateOk;
}

// ---- the bit reservoir: bits [8 * next - nbits, 8 * next) of the input, the next one lowest
struct InflateBits {
  const unsigned char* in;
  uint64_t insize, next, hold;
  uint32_t nbits;
};
// At least 57 bits, or all that are left.  Four bytes at once while four are left, else byte by byte: no byte outside
// [in, in + insize) is read.  `par.U32` makes a loaded value the wave's (every lane loaded the same).
template <class Par>
ZMX_INF_HD inline void InflateRefill(InflateBits* b, const Par& par) {
  if (b->nbits <= 32 && b->insize - b->next >= 4) {
    uint32_t w;
    memcpy(&w, b->in + b->next, 4);   // (little-endian on both sides)
    par.NoteRead(b->in + b->next, 4);
    b->hold |= static_cast<uint64_t>(par.U32(w)) << b->nbits;
    b->next += 4;
    b->nbits += 32;
  }
  while (b->nbits <= 56 && b->next < b->insize) {
    par.NoteRead(b->in + b->next, 1);
    b->hold |= static_cast<uint64_t>(par.U32(b->in[b->next])) << b->nbits;
    ++b->next;
    b->nbits += 8;
  }
}
ZMX_INF_HD inline void InflateDrop(InflateBits* b, uint32_t n) {
  b->hold >>= n;
  b->nbits -= n;
}
// n <= 32 bits into *v; false: the input ends first
template <class Par>
ZMX_INF_HD inline bool InflateTake(InflateBits* b, uint32_t n, uint32_t* v, const Par& par) {
  if (b->nbits < n) InflateRefill(b, par);
  if (b->nbits < n) return false;
  *v = static_cast<uint32_t>(b->hold & ((1ull << n) - 1));
  InflateDrop(b, n);
  return true;
}
// bytes of input behind which the next bit lies
ZMX_INF_HD inline uint64_t InflateBytesUsed(const InflateBits& b) { return b.next - b.nbits / 8; }

// ---- symbols
// literal/length symbol 257 + k (k <= 28): the length's base and extra bits
ZMX_INF_HD inline void InflateLengthOf(uint32_t k, uint32_t* base, uint32_t* extra) {
  if (k < 8) { *base = 3 + k; *extra = 0; }
  else if (k == 28) { *base = 258; *extra = 0; }
  else { *extra = (k >> 2) - 1; *base = 3 + ((4 + (k & 3)) << *extra); }
}
// distance symbol d (d <= 29)
ZMX_INF_HD inline void InflateDistOf(uint32_t d, uint32_t* base, uint32_t* extra) {
  if (d < 4) { *base = 1 + d; *extra = 0; }
  else { *extra = (d >> 1) - 1; *base = 1 + ((2 + (d & 1)) << *extra); }
}
// the order of the code-length code's lengths (RFC 1951, 3.2.7)
ZMX_INF_HD inline uint32_t InflateClenOrder(uint32_t i) {
  // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
  if (i < 3) return 16 + i;
  if (i == 3) return 0;
  const uint32_t j = i - 4;   // 8, 7, 9, 6, ...
  return (j & 1) ? 7 - (j >> 1) : 8 + (j >> 1);
}
// the fixed codes' length of symbol s of the 288 + 32
ZMX_INF_HD inline uint32_t InflateFixedLen(uint32_t s) {
  return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
}
ZMX_INF_HD inline uint32_t InflateReverse(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1) << (len - 1 - i);
  return r;
}

// ---- the table build, per lane
enum InflateCodeKind { kInflateCodeLens, kInflateCodeLit, kInflateCodeDist };
// Lane L = 1 .. 15 counts the codes of length L (lane 0: the symbols without a code).
ZMX_INF_HD inline void InflateCountLane(const unsigned char* lens, uint32_t n, InflateCode* C, uint32_t lane) {
  if (lane > kInflateMaxBits) return;
  uint32_t c = 0;
  for (uint32_t s = 0; s < n; ++s) c += lens[s] == lane;
  C->count[lane] = static_cast<uint16_t>(c);
}
// zlib's verdict on the counts (inftrees.c:inflate_table): over-subscribed; incomplete, unless a literal/length or
// distance set is a single one-bit code or a distance set has no code at all.
ZMX_INF_HD inline uint32_t InflateCheckCounts(const InflateCode& C, uint32_t n, InflateCodeKind kind) {
  if (C.count[0] == n) return kind == kInflateCodeDist ? kInflateOk : kInflateIncomplete;
  int32_t left = 1;
  uint32_t max = 0;
  for (uint32_t len = 1; len <= kInflateMaxBits; ++len) {
    left = (left << 1) - static_cast<int32_t>(C.count[len]);
    if (left < 0) return kInflateOversubscribed;
    if (C.count[len]) max = len;
  }
  if (left > 0 && (kind == kInflateCodeLens || max != 1)) return kInflateIncomplete;
  return kInflateOk;
}
// Lane L = 1 .. 15 gives the symbols of length L, in ascending order, their places in sorted[] and their codes.
ZMX_INF_HD inline void InflateAssignLane(const unsigned char* lens, uint32_t n, InflateCode* C, uint32_t lane) {
  if (lane == 0 || lane > kInflateMaxBits) return;
  uint32_t at = 0, code = 0;
  for (uint32_t len = 1; len <= lane; ++len) {
    code = (code + (len > 1 ? C->count[len - 1] : 0)) << 1;
    if (len < lane) at += C->count[len];
  }
  for (uint32_t s = 0; s < n; ++s) {
    if (lens[s] != lane) continue;
    C->sorted[at++] = static_cast<uint16_t>(s);
    C->code[s] = static_cast<uint16_t>(code++);
  }
}
// The primary table: lane by lane emptied, then symbol s = lane, lane + 64, ... of at most `root` bits written to every
// index whose low bits are its code, first bit lowest.  Two symbols never share an index: the codes are prefix-free.
ZMX_INF_HD inline void InflateClearLane(uint16_t* table, uint32_t root, uint32_t lane) {
  for (uint32_t i = lane; i < (1u << root); i += kInflateLanes) table[i] = 0;
}
ZMX_INF_HD inline void InflateFillLane(const unsigned char* lens, uint32_t n, const InflateCode& C, uint16_t* table, uint32_t root, uint32_t lane) {
  for (uint32_t s = lane; s < n; s += kInflateLanes) {
    const uint32_t len = lens[s];
    if (len == 0 || len > root) continue;
    const uint16_t entry = static_cast<uint16_t>((s << 4) | len);
    for (uint32_t i = InflateReverse(C.code[s], len); i < (1u << root); i += 1u << len) table[i] = entry;
  }
}
// counts, verdict, order and codes, table (table null: the code-length code, which is walked)
template <class Par>
ZMX_INF_HD inline uint32_t InflateBuild(const unsigned char* lens, uint32_t n, InflateCodeKind kind, InflateCode* C, uint16_t* table, uint32_t root,
                                        const Par& par) {
  par.Each([&](uint32_t lane) {
    InflateCountLane(lens, n, C, lane);
    if (table) InflateClearLane(table, root, lane);
  });
  const uint32_t verdict = InflateCheckCounts(*C, n, kind);
  if (verdict != kInflateOk) return verdict;
  par.Each([&](uint32_t lane) { InflateAssignLane(lens, n, C, lane); });
  if (table) par.Each([&](uint32_t lane) { InflateFillLane(lens, n, *C, table, root, lane); });
  return kInflateOk;
}

// ---- the symbol step: the next symbol of code C.  The table where the code is short, else the canonical walk, a bit at a
// time: kInflateTruncated where the input ends inside the code, kInflateBadCode where no code owns the fifteen bits.
template <class Par>
ZMX_INF_HD inline uint32_t InflateSymbol(InflateBits* b, const uint16_t* table, uint32_t root, const InflateCode& C, uint32_t* sym, const Par& par) {
  if (b->nbits < kInflateMaxBits) InflateRefill(b, par);
  if (table) {
    const uint32_t e = par.U32(table[b->hold & ((1u << root) - 1)]);
    if (e != 0) {
      const uint32_t len = e & 15;
      if (len > b->nbits) return kInflateTruncated;
      InflateDrop(b, len);
      *sym = e >> 4;
      return kInflateOk;
    }
  }
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= kInflateMaxBits; ++len) {
    if (len > b->nbits) return kInflateTruncated;
    code |= static_cast<uint32_t>(b->hold >> (len - 1)) & 1;
    const uint32_t count = par.U32(C.count[len]);
    if (code < first + count) {
      *sym = par.U32(C.sorted[index + (code - first)]);
      InflateDrop(b, len);
      return kInflateOk;
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return kInflateBadCode;
}

// ---- the length decoding of a dynamic block: HLIT, HDIST, HCLEN, the code-length code, the HLIT + HDIST lengths with
// their repeats (which run across the two alphabets' boundary) into S->lens; *nlen, *ndist: the alphabets' sizes.
template <class Par>
ZMX_INF_HD inline uint32_t InflateDynamicLengths(InflateBits* b, InflateScratch* S, uint32_t* nlen, uint32_t* ndist, const Par& par) {
  uint32_t v = 0;
  if (!InflateTake(b, 14, &v, par)) return kInflateTruncated;
  *nlen = (v & 31) + 257;
  *ndist = ((v >> 5) & 31) + 1;
  const uint32_t ncode = (v >> 10) + 4;
  if (*nlen > 286 || *ndist > 30) return kInflateTooManySymbols;
  // (the nineteen lengths come three bits at a time; all lanes write the same values)
  for (uint32_t i = 0; i < 19; ++i) {
    uint32_t len = 0;
    if (i < ncode && !InflateTake(b, 3, &len, par)) return kInflateTruncated;
    S->lens[InflateClenOrder(i)] = static_cast<unsigned char>(len);
  }
  uint32_t status = InflateBuild(S->lens, 19, kInflateCodeLens, &S->dist, static_cast<uint16_t*>(nullptr), 0, par);
  if (status != kInflateOk) return status;
  // (nothing reads the nineteen after the build — the walk goes by S->dist —, so the lengths take their place in S->lens)
  const uint32_t total = *nlen + *ndist;
  uint32_t have = 0, prev = 0;
  while (have < total) {
    uint32_t sym = 0;
    status = InflateSymbol(b, static_cast<const uint16_t*>(nullptr), 0, S->dist, &sym, par);
    if (status != kInflateOk) return status;
    if (sym < 16) {
      S->lens[have++] = static_cast<unsigned char>(sym);
      prev = sym;
      continue;
    }
    uint32_t repeat = 0, len = 0;
    if (sym == 16) {
      if (!InflateTake(b, 2, &repeat, par)) return kInflateTruncated;
      if (have == 0) return kInflateRepeat;
      repeat += 3;
      len = prev;
    } else if (sym == 17) {
      if (!InflateTake(b, 3, &repeat, par)) return kInflateTruncated;
      repeat += 3;
    } else {
      if (!InflateTake(b, 7, &repeat, par)) return kInflateTruncated;
      repeat += 11;
    }
    if (have + repeat > total) return kInflateRepeat;
    for (uint32_t i = 0; i < repeat; ++i) S->lens[have++] = static_cast<unsigned char>(len);
    prev = len;
  }
  return kInflateOk;
}

// ---- the window's index arithmetic
ZMX_INF_HD inline uint32_t InflateRingAt(uint32_t base, uint32_t i) { return (base + i) % kInflateRing; }
// A match of `len` bytes at distance `dist` whose first byte goes to ring[wpos]: byte i comes from start + i % dist, which
// lies in front of the match, so dist < len needs no special case.  Lane `lane` copies bytes lane, lane + 64, ...
ZMX_INF_HD inline void InflateMatchLane(unsigned char* ring, uint32_t wpos, uint32_t dist, uint32_t len, uint32_t lane) {
  const uint32_t start = (wpos + kInflateRing - dist) % kInflateRing;
  for (uint32_t i = lane; i < len; i += kInflateLanes) {
    ring[InflateRingAt(wpos, i)] = ring[InflateRingAt(start, dist >= len ? i : i % dist)];
  }
}
// n bytes of the input into the ring (a stored block's)
template <class Par>
ZMX_INF_HD inline void InflateStoredLane(unsigned char* ring, uint32_t wpos, const unsigned char* src, uint32_t n, uint32_t lane, const Par& par) {
  for (uint32_t i = lane; i < n; i += kInflateLanes) {
    par.NoteRead(src + i, 1);
    ring[InflateRingAt(wpos, i)] = src[i];
  }
}

// ---- the flush's split: n bytes to `dst` as head bytes up to the first 16-byte boundary, 16-byte groups, tail bytes
ZMX_INF_HD inline void InflateFlushSplit(const unsigned char* dst, uint64_t n, uint32_t* head, uint32_t* groups, uint32_t* tail) {
  const uint64_t to_boundary = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
  const uint64_t h = to_boundary < n ? to_boundary : n;
  *head = static_cast<uint32_t>(h);
  *groups = static_cast<uint32_t>((n - h) / 16);
  *tail = static_cast<uint32_t>((n - h) % 16);
}
struct alignas(16) InflateGroup { uint32_t w[4]; };
// Lane `lane`'s share of n <= 2 * kInflateStretch bytes from ring[rpos ...] to dst.
template <class Par>
ZMX_INF_HD inline void InflateFlushLane(const unsigned char* ring, uint32_t rpos, unsigned char* dst, uint32_t n, uint32_t lane, const Par& par) {
  uint32_t head = 0, groups = 0, tail = 0;
  InflateFlushSplit(dst, n, &head, &groups, &tail);
  for (uint32_t i = lane; i < head; i += kInflateLanes) {
    par.NoteWrite(dst + i, 1);
    dst[i] = ring[InflateRingAt(rpos, i)];
  }
  for (uint32_t g = lane; g < groups; g += kInflateLanes) {
    const uint32_t from = InflateRingAt(rpos, head + 16 * g);
    InflateGroup v;
    if (from % 4 == 0) {   // (and so no wrap inside a word: the ring is a multiple of 16)
      for (uint32_t k = 0; k < 4; ++k) {
        const unsigned char* p = ring + InflateRingAt(from, 4 * k);
        v.w[k] = p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
      }
    } else {
      for (uint32_t k = 0; k < 4; ++k) {
        uint32_t w = 0;
        for (uint32_t j = 0; j < 4; ++j) w |= static_cast<uint32_t>(ring[InflateRingAt(from, 4 * k + j)]) << (8 * j);
        v.w[k] = w;
      }
    }
    unsigned char* to = dst + head + 16 * static_cast<uint64_t>(g);
    par.NoteWrite(to, 16);
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<InflateGroup*>(to) = v;   // one 16-byte store: `to` is aligned
#else
    memcpy(to, &v, 16);
#endif
  }
  unsigned char* const last = dst + head + 16 * static_cast<uint64_t>(groups);
  for (uint32_t i = lane; i < tail; i += kInflateLanes) {
    par.NoteWrite(last + i, 1);
    last[i] = ring[InflateRingAt(rpos, head + 16 * groups + i)];
  }
}

// What the walk has put out: `total` bytes, the first `flushed` of them gone from the ring's care.
struct InflateOut {
  unsigned char* out;
  uint64_t capacity;   // (0 where out is null)
  uint64_t total, flushed;
};
ZMX_INF_HD inline uint32_t InflateWpos(const InflateOut& o) { return static_cast<uint32_t>(o.total % kInflateRing); }
// n pending bytes leave the ring: those below capacity are stored
template <class Par>
ZMX_INF_HD inline void InflateFlush(InflateScratch* S, InflateOut* o, uint32_t n, const Par& par) {
  const uint64_t end = o->flushed + n < o->capacity ? o->flushed + n : o->capacity;
  if (o->flushed < end) {
    const uint32_t m = static_cast<uint32_t>(end - o->flushed), rpos = static_cast<uint32_t>(o->flushed % kInflateRing);
    unsigned char* const dst = o->out + o->flushed;
    par.Each([&](uint32_t lane) { InflateFlushLane(S->ring, rpos, dst, m, lane, par); });
  }
  o->flushed += n;
}
template <class Par>
ZMX_INF_HD inline void InflateFlushStretches(InflateScratch* S, InflateOut* o, const Par& par) {
  while (o->total - o->flushed >= kInflateStretch) InflateFlush(S, o, kInflateStretch, par);
}

// ---- the blocks
template <class Par>
ZMX_INF_HD inline uint32_t InflateStoredBlock(InflateBits* b, InflateScratch* S, InflateOut* o, const Par& par) {
  InflateDrop(b, b->nbits % 8);
  uint32_t v = 0;
  if (!InflateTake(b, 32, &v, par)) return kInflateTruncated;
  const uint32_t len = v & 0xffff;
  if (len != ((v >> 16) ^ 0xffff)) return kInflateStoredLen;
  // the bytes come from the input itself: the reservoir holds whole bytes, which are given back
  uint64_t p = InflateBytesUsed(*b);
  b->next = p;
  b->hold = 0;
  b->nbits = 0;
  if (b->insize - p < len) return kInflateTruncated;
  uint32_t left = len;
  while (left != 0) {
    const uint32_t n = left < kInflateStretch ? left : kInflateStretch;
    const uint32_t wpos = InflateWpos(*o);
    const unsigned char* const src = b->in + p;
    par.Each([&](uint32_t lane) { InflateStoredLane(S->ring, wpos, src, n, lane, par); });
    o->total += n;
    p += n;
    left -= n;
    InflateFlushStretches(S, o, par);
  }
  b->next = p;
  return kInflateOk;
}
// the symbols of a block up to its end code
template <class Par>
ZMX_INF_HD inline uint32_t InflateSymbols(InflateBits* b, InflateScratch* S, InflateOut* o, const Par& par) {
  for (;;) {
    uint32_t sym = 0;
    uint32_t status = InflateSymbol(b, S->lit_table, kInflateLitRoot, S->lit, &sym, par);
    if (status != kInflateOk) return status;
    if (sym < 256) {
      S->ring[InflateWpos(*o)] = static_cast<unsigned char>(sym);   // (every lane the same byte)
      ++o->total;
    } else if (sym == 256) {
      return kInflateOk;
    } else {
      if (sym > 285) return kInflateBadSymbol;
      uint32_t base = 0, extra = 0, bits = 0;
      InflateLengthOf(sym - 257, &base, &extra);
      if (!InflateTake(b, extra, &bits, par)) return kInflateTruncated;
      const uint32_t len = base + bits;
      status = InflateSymbol(b, S->dist_table, kInflateDistRoot, S->dist, &sym, par);
      if (status != kInflateOk) return status;
      if (sym > 29) return kInflateBadSymbol;
      InflateDistOf(sym, &base, &extra);
      if (!InflateTake(b, extra, &bits, par)) return kInflateTruncated;
      const uint32_t dist = base + bits;
      if (dist > o->total) return kInflateDistance;
      const uint32_t wpos = InflateWpos(*o);
      par.Each([&](uint32_t lane) { InflateMatchLane(S->ring, wpos, dist, len, lane); });
      o->total += len;
    }
    InflateFlushStretches(S, o, par);
  }
}

// ---- the walk of one stream
template <class Par>
ZMX_INF_HD inline void InflateWalk(uint32_t format, const InflateJob& job, InflateScratch* S, const Par& par, InflateResult* r) {
  r->outsize = r->consumed = 0;
  r->status = r->block = r->stored_check = r->stored_isize = 0;
  uint64_t pos = 0;
  uint32_t status = kInflateOk;
  if (format == kInflateZlib || format == kInflateGzip) {
    const uint64_t peek = job.insize;   // (the header's bytes are read one by one, inside the range)
    status = format == kInflateZlib ? InflateZlibHeader(job.in, peek, &pos) : InflateGzipHeader(job.in, peek, &pos);
    if (status == kInflateOk) par.NoteRead(job.in, pos);
  }
  if (status != kInflateOk) {
    r->status = status;
    return;
  }
  InflateBits b = {job.in, job.insize, pos, 0, 0};
  InflateOut o = {job.out, job.out ? job.capacity : 0, 0, 0};
  for (;;) {
    uint32_t v = 0;
    if (!InflateTake(&b, 3, &v, par)) { status = kInflateTruncated; break; }
    const uint32_t type = v >> 1;
    if (type == 0) {
      status = InflateStoredBlock(&b, S, &o, par);
    } else if (type == 3) {
      status = kInflateBlockType;
    } else {
      uint32_t nlen = kInflateLitSymbols, ndist = kInflateDistSymbols;
      if (type == 1) {
        par.Each([&](uint32_t lane) {
          for (uint32_t s = lane; s < kInflateLitSymbols + kInflateDistSymbols; s += kInflateLanes) S->lens[s] = static_cast<unsigned char>(InflateFixedLen(s));
        });
      } else {
        status = InflateDynamicLengths(&b, S, &nlen, &ndist, par);
        if (status == kInflateOk && par.U32(S->lens[256]) == 0) status = kInflateNoEndCode;
      }
      if (status == kInflateOk) status = InflateBuild(S->lens, nlen, kInflateCodeLit, &S->lit, S->lit_table, kInflateLitRoot, par);
      if (status == kInflateOk) status = InflateBuild(S->lens + nlen, ndist, kInflateCodeDist, &S->dist, S->dist_table, kInflateDistRoot, par);
      if (status == kInflateOk) status = InflateSymbols(&b, S, &o, par);
    }
    if (status != kInflateOk || (v & 1)) break;
    ++r->block;
  }
  if (o.total != o.flushed) InflateFlush(S, &o, static_cast<uint32_t>(o.total - o.flushed), par);
  r->outsize = o.total;
  if (status == kInflateOk) {
    InflateDrop(&b, b.nbits % 8);
    const uint64_t p = InflateBytesUsed(b);
    status = InflateTrailer(format, job.in, job.insize, p, r);
    if (status == kInflateOk) par.NoteRead(job.in + p, r->consumed - p);
  }
  if (status != kInflateOk) r->consumed = (8 * b.next - b.nbits + 7) / 8;
  if (status == kInflateOk && job.out && o.total > job.capacity) status = kInflateCapacity;
  r->status = status;
}

}  // namespace zamd

#ifdef ZMX_INFLATE_KERNELS

struct InflateParams {
  const zamd::InflateJob* jobs;
  zamd::InflateResult* results;
  u32 njobs, format;
};

// The 64 lanes of the wave side by side; a barrier on either side of a lane-parallel rule orders it against the walk's own
// LDS accesses and against the rule before it (one wave: the barrier costs its waits alone).
struct InflateDevicePar {
  template <class F>
  __device__ void Each(F f) const {
    __syncthreads();
    f(threadIdx.x);
    __syncthreads();
  }
  __device__ u32 U32(u32 v) const { return static_cast<u32>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }
  __device__ void NoteRead(const void*, u64) const {}
  __device__ void NoteWrite(const void*, u64) const {}
};

__global__ __launch_bounds__(64) void k_inflate(InflateParams P) {
  __shared__ zamd::InflateScratch S;
  if (blockIdx.x >= P.njobs) return;
  const zamd::InflateJob job = P.jobs[blockIdx.x];
  zamd::InflateResult r;
  zamd::InflateWalk(P.format, job, &S, InflateDevicePar(), &r);
  if (threadIdx.x == 0) P.results[blockIdx.x] = r;   // (the host puts it into the caller's slot, job.index)
}

#endif  // ZMX_INFLATE_KERNELS

#endif  // ZMX_INFLATE_H_
