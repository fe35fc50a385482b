// zmx_png_deflate_sizes_device: the length lodepng_zlib_compress gives for buffers in device memory under LodePNG's
// default settings (btype 2, minmatch 3, nicematch 128, lazy matching) at the caller's window — what zopflipng's
// filter-strategy trials compare (zopflipng_lib.cc AutoChooseFilterStrategy: window 8192).  Only the size is made: the
// kernels bring every deflate block down to its 286 + 30 symbol counts and its extra bits, and host/png_lodeflate_size.h
// turns those into bits the way deflateDynamic writes them.
//
// The parse is encodeLZ77's (lodepng.cpp:1593-1740) in the parallel form zmx_png_brute.h states for one row and proves
// against LodePNG: the hash state a search sees is "positions 0..pos inserted", a function of the data alone, so the
// searches are independent and only the lazy parse is serial.  What a whole buffer adds:
//   blocks   lodepng_deflatev cuts the buffer into blocks of insize / 8 + 8 bytes within [65536, 262144] and calls
//            encodeLZ77 per block with the block's end as `insize`: getHash takes its short form in a block's last two
//            positions, countZeros and every match stop at the block's end, and `numzeros` and the lazy state start from 0.
//            The Hash itself is initialised once per buffer: links and matches reach back over block ends.
//   links    C[p] (what inserting p writes into chain[p & M]) needs the last q < p of the WHOLE buffer with H[q] == H[p],
//            however far back, else it keeps what the slot held.  A buffer is cut into tiles of `tile_len` positions:
//              k_png_lo_links   one workgroup per tile walks it 256 positions at a time with a head table of its own
//                               (65536 hash keys and 259 zero-run keys, in global memory: k_png_brute's step 3).  A
//                               position whose key has no earlier position in the tile is marked ASK.  The tile's table
//                               ends as "the last position of every key in this tile";
//              k_png_lo_ask     a lane per position: an ASK walks the earlier tiles' tables from the nearest one back;
//                               none has the key: KEEP;
//              k_png_lo_keep    a lane per position: a KEEP takes C[p - W], C[p - 2W] ... until one is no KEEP, or the
//                               slot itself below W (chain[i] == i, "uninitialised").
//            A tile-sized table costs a quarter of the tile's own arrays at 262144 positions per tile, and the tiles of
//            all buffers of a call run side by side; a keyed sort would move 12 bytes per position several times.
//   search   k_png_lo_search, a lane per position, k_png_brute's step 4 on global arrays.
//   parse    k_png_lo_parse, one wave per deflate block: the wave stages 2048 results and bytes at a time in the LDS, every
//            lane replays the lazy parse on them in step (uniform control flow, broadcast reads) and lane 0 counts.
// Per position the scratch holds H << 16 | C, Z << 16 | CZ and length | offset << 16: twelve bytes.
//
// The rules are __host__ __device__ functions of a lane's index, so a CPU program (tests/hostlib/png_lodeflate_print.cc)
// runs the very code of the kernels, lanes one after the other, at any tile length.  This header compiles without HIP;
// the kernels are there for the device layer only (ZMX_PNG_LODEFLATE_KERNELS).
#ifndef ZMX_PNG_LODEFLATE_H_
#define ZMX_PNG_LODEFLATE_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define ZMX_LO_HD __host__ __device__
#else
#define ZMX_LO_HD
#endif

namespace zamd {

constexpr uint32_t kLoThreads = 256;            // a workgroup of the per-position kernels, and the links' chunk
constexpr uint32_t kLoTileLen = 262144;         // positions per tile on the device
constexpr uint32_t kLoTableLen = 65536 + 260;   // a tile's head table: hash keys, then zero-run keys 0 .. 258
constexpr uint32_t kLoAsk = 0xfffeu, kLoKeep = 0xffffu;   // (slots are below 32768)
constexpr uint32_t kLoParseChunk = 2048;
constexpr uint32_t kLoCountWords = 286 + 30 + 2;   // a block's counts as the kernel writes them: ll, d, extra bits (low, high)

struct LoBuf {
  const unsigned char* data;
  uint64_t n;            // bytes
  uint64_t base;         // where its positions start in the per-position arrays
  uint32_t blocksize;    // lodepng_deflatev's
  uint32_t first_tile;   // its first tile in the call's tile list
};

struct LoTile {   // also a deflate block in the parse's list
  uint64_t start;        // within the buffer
  uint32_t len;
  uint32_t buf;
};

struct LoParams {
  const LoBuf* bufs;
  const LoTile* tiles;
  const LoTile* blocks;
  uint32_t* HC;          // [positions] H << 16 | C
  uint32_t* ZC;          // [positions] Z << 16 | CZ
  uint32_t* LD;          // [positions] length | offset << 16
  uint32_t* tables;      // [tiles][kLoTableLen] position in the tile + 1, 0: none; zero before k_png_lo_links
  uint32_t* counts;      // [blocks][kLoCountWords]
  uint32_t window, ntiles, nblocks, tile_len;
};

// The lists of a call (host): the buffers with their places in the per-position arrays, their tiles and their deflate
// blocks.  `data` pointers are the caller's; `blocksize` is lodepng_deflatev's (host/png_lodeflate_size.h LoBlockSize).
struct LoPlan {
  std::vector<LoBuf> bufs;
  std::vector<LoTile> tiles, blocks;
  std::vector<uint32_t> first_block;   // [bufs + 1] into `blocks`
  uint64_t positions = 0;
  uint32_t longest_tile = 0;
};

inline LoPlan LoMakePlan(size_t n, const void* const* data, const size_t* sizes, uint32_t tile_len) {
  LoPlan plan;
  for (size_t b = 0; b < n; ++b) {
    LoBuf B;
    B.data = static_cast<const unsigned char*>(data[b]);
    B.n = sizes[b];
    B.base = plan.positions;
    uint64_t bs = B.n / 8u + 8u;
    bs = bs < 65536u ? 65536u : bs > 262144u ? 262144u : bs;
    B.blocksize = static_cast<uint32_t>(bs);
    B.first_tile = static_cast<uint32_t>(plan.tiles.size());
    plan.bufs.push_back(B);
    plan.first_block.push_back(static_cast<uint32_t>(plan.blocks.size()));
    for (uint64_t s = 0; s < B.n; s += tile_len) {
      const uint32_t len = static_cast<uint32_t>(B.n - s < tile_len ? B.n - s : tile_len);
      plan.tiles.push_back({s, len, static_cast<uint32_t>(b)});
      if (len > plan.longest_tile) plan.longest_tile = len;
    }
    for (uint64_t s = 0; s < B.n; s += bs) {
      plan.blocks.push_back({s, static_cast<uint32_t>(B.n - s < bs ? B.n - s : bs), static_cast<uint32_t>(b)});
    }
    plan.positions += B.n;
  }
  plan.first_block.push_back(static_cast<uint32_t>(plan.blocks.size()));
  return plan;
}

ZMX_LO_HD inline uint64_t LoBlockEnd(const LoBuf& B, uint64_t p) {
  const uint64_t e = (p / B.blocksize + 1) * B.blocksize;
  return e < B.n ? e : B.n;
}

ZMX_LO_HD inline uint32_t LoLog2(uint32_t v) {
  uint32_t r = 0;
  while (v >>= 1) ++r;
  return r;
}
ZMX_LO_HD inline uint32_t LoLengthExtra(uint32_t l) { return (l <= 10u || l == 258u) ? 0u : LoLog2(l - 3u) - 2u; }
ZMX_LO_HD inline uint32_t LoLengthSymbol(uint32_t l) { return l == 258u ? 285u : 257u + 4u * LoLengthExtra(l) + ((l - 3u) >> LoLengthExtra(l)); }
ZMX_LO_HD inline uint32_t LoDistExtra(uint32_t d) { return d <= 4u ? 0u : LoLog2(d - 1u) - 1u; }
ZMX_LO_HD inline uint32_t LoDistSymbol(uint32_t d) { return 2u * LoDistExtra(d) + ((d - 1u) >> LoDistExtra(d)); }

// ---- k_png_lo_hash: position `i` of tile `t`: the hash and the zero run, the links still empty
ZMX_LO_HD inline void LoHashLane(const LoParams& P, uint32_t t, uint32_t i) {
  const LoTile T = P.tiles[t];
  const LoBuf B = P.bufs[T.buf];
  const uint64_t p = T.start + i, e = LoBlockEnd(B, p);
  const unsigned char* f = B.data;
  uint32_t h;
  if (p + 2 < e) h = (uint32_t)f[p] ^ ((uint32_t)f[p + 1] << 4) ^ ((uint32_t)f[p + 2] << 8);
  else h = (uint32_t)f[p] ^ (p + 1 < e ? (uint32_t)f[p + 1] << 8 : 0u);
  h &= 65535u;
  uint32_t z = 0;
  if (h == 0) {
    while (z < 258u && p + z < e && f[p + z] == 0) ++z;
  }
  P.HC[B.base + p] = h << 16;
  P.ZC[B.base + p] = z << 16;
}

// ---- k_png_lo_links: a chunk of kLoThreads positions of tile `t` from `b0`, in three phases with a barrier between
// them; s_key[0 / 1] and s_next[0 / 1] are the workgroup's arrays of kLoThreads entries for the hash and the zero run.
ZMX_LO_HD inline void LoLinksLoad(const LoParams& P, uint32_t t, uint32_t b0, uint32_t lane, uint32_t* s_h, uint32_t* s_z,
                                  unsigned char* s_nexth, unsigned char* s_nextz) {
  const LoTile T = P.tiles[t];
  const uint64_t g = P.bufs[T.buf].base + T.start + b0 + lane;
  const bool live = b0 + lane < T.len;
  s_h[lane] = live ? P.HC[g] >> 16 : 0xffffffffu;
  s_z[lane] = live ? P.ZC[g] >> 16 : 0xffffffffu;
  s_nexth[lane] = 0;
  s_nextz[lane] = 0;
}

ZMX_LO_HD inline void LoLinksFind(const LoParams& P, uint32_t t, uint32_t b0, uint32_t lane, const uint32_t* s_h, const uint32_t* s_z,
                                  unsigned char* s_nexth, unsigned char* s_nextz) {
  const LoTile T = P.tiles[t];
  if (b0 + lane >= T.len) return;
  const uint32_t M = P.window - 1u;
  const uint64_t p0 = T.start + b0;
  const uint64_t g = P.bufs[T.buf].base + p0 + lane;
  const uint32_t* table = P.tables + (uint64_t)t * kLoTableLen;
  const uint32_t h = s_h[lane], z = s_z[lane];
  int j = (int)lane - 1;
  while (j >= 0 && s_h[j] != h) --j;
  uint32_t c;
  if (j >= 0) {
    c = (uint32_t)(p0 + (uint32_t)j) & M;
    s_nexth[j] = 1;
  } else {
    const uint32_t v = table[h];
    c = v ? (uint32_t)(T.start + v - 1u) & M : kLoAsk;
  }
  int k = (int)lane - 1;
  while (k >= 0 && s_z[k] != z) --k;
  uint32_t cz;
  if (k >= 0) {
    cz = (uint32_t)(p0 + (uint32_t)k) & M;
    s_nextz[k] = 1;
  } else {
    const uint32_t v = table[65536u + z];
    cz = v ? (uint32_t)(T.start + v - 1u) & M : kLoAsk;
  }
  P.HC[g] = (h << 16) | c;
  P.ZC[g] = (z << 16) | cz;
}

ZMX_LO_HD inline void LoLinksPublish(const LoParams& P, uint32_t t, uint32_t b0, uint32_t lane, const uint32_t* s_h, const uint32_t* s_z,
                                     const unsigned char* s_nexth, const unsigned char* s_nextz) {
  const LoTile T = P.tiles[t];
  if (b0 + lane >= T.len) return;
  uint32_t* table = P.tables + (uint64_t)t * kLoTableLen;
  if (!s_nexth[lane]) table[s_h[lane]] = b0 + lane + 1u;
  if (!s_nextz[lane]) table[65536u + s_z[lane]] = b0 + lane + 1u;
}

// ---- k_png_lo_ask: position `i` of tile `t`: a link marked ASK looks through the buffer's earlier tiles, nearest first
ZMX_LO_HD inline uint32_t LoAskWalk(const LoParams& P, uint32_t t, uint32_t first_tile, uint32_t key) {
  for (uint32_t u = t; u > first_tile;) {
    --u;
    const uint32_t v = P.tables[(uint64_t)u * kLoTableLen + key];
    if (v) return (uint32_t)(P.tiles[u].start + v - 1u) & (P.window - 1u);
  }
  return kLoKeep;
}

ZMX_LO_HD inline void LoAskLane(const LoParams& P, uint32_t t, uint32_t i) {
  const LoTile T = P.tiles[t];
  const LoBuf B = P.bufs[T.buf];
  const uint64_t g = B.base + T.start + i;
  const uint32_t hc = P.HC[g], zc = P.ZC[g];
  if ((hc & 0xffffu) == kLoAsk) P.HC[g] = (hc & 0xffff0000u) | LoAskWalk(P, t, B.first_tile, hc >> 16);
  if ((zc & 0xffffu) == kLoAsk) P.ZC[g] = (zc & 0xffff0000u) | LoAskWalk(P, t, B.first_tile, 65536u + (zc >> 16));
}

// ---- k_png_lo_keep: position `i` of tile `t`: a link marked KEEP takes what the slot held.  Other lanes resolve their
// own KEEPs meanwhile; a word read is either still KEEP (the walk goes on) or final, and both give the same end.
ZMX_LO_HD inline uint32_t LoKeepWalk(const uint32_t* A, uint64_t base, uint64_t p, uint32_t W) {
  while (p >= W) {
    p -= W;
    const uint32_t c = A[base + p] & 0xffffu;
    if (c != kLoKeep) return c;
  }
  return (uint32_t)p;   // the slot itself
}

ZMX_LO_HD inline void LoKeepLane(const LoParams& P, uint32_t t, uint32_t i) {
  const LoTile T = P.tiles[t];
  const LoBuf B = P.bufs[T.buf];
  const uint64_t p = T.start + i, g = B.base + p;
  const uint32_t hc = P.HC[g], zc = P.ZC[g];
  if ((hc & 0xffffu) == kLoKeep) P.HC[g] = (hc & 0xffff0000u) | LoKeepWalk(P.HC, B.base, p, P.window);
  if ((zc & 0xffffu) == kLoKeep) P.ZC[g] = (zc & 0xffff0000u) | LoKeepWalk(P.ZC, B.base, p, P.window);
}

// ---- k_png_lo_search: position `i` of tile `t`: the longest-match search (lodepng.cpp:1636-1689) on the state
// "0..pos inserted".  Slot s holds what its latest position pos - ((pos - s) & M) wrote; `node` is HC of the position
// the slot `hashpos` holds, carried from the step that checked its hash.
ZMX_LO_HD inline void LoSearchLane(const LoParams& P, uint32_t t, uint32_t i) {
  const LoTile T = P.tiles[t];
  const LoBuf B = P.bufs[T.buf];
  const uint32_t W = P.window, M = W - 1u;
  const uint32_t maxchain = W >= 8192u ? W : W / 8u;
  const uint64_t pos = T.start + i, e = LoBlockEnd(B, pos);
  const uint64_t last = e < pos + 258u ? e : pos + 258u;
  const unsigned char* F = B.data;
  const uint32_t* HC = P.HC + B.base;
  const uint32_t* ZC = P.ZC + B.base;
  const uint32_t wpos = (uint32_t)pos & M, self = HC[pos], hv = self >> 16, nz = ZC[pos] >> 16;
  uint32_t length = 0, offset = 0, hashpos = self & 0xffffu, prev_offset = 0, chainlength = 0;
  uint32_t node = ((wpos - hashpos) & M) <= pos ? HC[pos - ((wpos - hashpos) & M)] : 0u;
  for (;;) {
    if (chainlength++ >= maxchain) break;
    const uint32_t cur = hashpos <= wpos ? wpos - hashpos : wpos - hashpos + W;
    if (cur < prev_offset) break;
    prev_offset = cur;
    if (cur > pos) break;       // a slot no position has written yet: LodePNG only reaches those as chain[i] == i
    const uint64_t q = pos - cur;
    if (cur > 0) {
      uint64_t fo = pos, ba = q;
      if (nz >= 3u) {
        const uint32_t zq = ZC[q] >> 16, skip = zq < nz ? zq : nz;
        fo += skip;
        ba += skip;
      }
      while (fo != last && F[ba] == F[fo]) { ++fo; ++ba; }
      const uint32_t cl = (uint32_t)(fo - pos);
      if (cl > length) {
        length = cl;
        offset = cur;
        if (cl >= 128u) break;  // nicematch
      }
    }
    const uint32_t chainv = node & 0xffffu;
    if (hashpos == chainv) break;
    if (nz >= 3u && length > nz) {
      hashpos = ZC[q] & 0xffffu;
      const uint32_t c2 = (wpos - hashpos) & M;
      if (c2 > pos || (ZC[pos - c2] >> 16) != nz) break;
      node = HC[pos - c2];
    } else {
      hashpos = chainv;
      const uint32_t c2 = (wpos - hashpos) & M;
      if (c2 > pos) break;
      node = HC[pos - c2];
      if ((node >> 16) != hv) break;
    }
  }
  P.LD[B.base + pos] = length | (offset << 16);
}

// ---- k_png_lo_parse: the lazy parse of one deflate block (lodepng.cpp:1691-1736).  `Stage` gives the result and the
// byte of a position of the block (on the device: from the LDS, refilled by the whole wave); `Count` counts a symbol.
template <typename Stage, typename Count>
ZMX_LO_HD inline uint64_t LoParseBlock(uint32_t len, uint32_t window, Stage&& stage, Count&& count) {
  const uint32_t maxlazy = window >= 8192u ? 258u : 64u;
  uint64_t extra = 0;
  uint32_t lazy = 0, ll = 0, lo = 0, lazybyte = 0;
  for (uint32_t pos = 0; pos < len; ++pos) {
    uint32_t byte = 0;
    const uint32_t v = stage(pos, &byte);
    uint32_t length = v & 0xffffu, offset = v >> 16;
    if (!lazy && length >= 3u && length <= maxlazy && length < 258u) {
      lazy = 1;
      ll = length;
      lo = offset;
      lazybyte = byte;
      continue;
    }
    if (lazy) {
      lazy = 0;
      if (length > ll + 1u) {
        count(lazybyte);
      } else {          // the earlier match stands: back to its position
        length = ll;
        offset = lo;
        byte = lazybyte;
        --pos;
      }
    }
    if (length < 3u || (length == 3u && offset > 4096u)) {
      count(byte);
    } else {
      count(LoLengthSymbol(length));
      count(286u + LoDistSymbol(offset));
      extra += LoLengthExtra(length) + LoDistExtra(offset);
      pos += length - 1u;
    }
  }
  return extra;
}

}  // namespace zamd

#ifdef ZMX_PNG_LODEFLATE_KERNELS

// grid (x, tiles from tile0): the workgroups of a row stride over their tile's positions
__global__ __launch_bounds__(zamd::kLoThreads) void k_png_lo_hash(zamd::LoParams P, u32 tile0) {
  const u32 t = tile0 + blockIdx.y, len = P.tiles[t].len;
  for (u32 i = blockIdx.x * zamd::kLoThreads + threadIdx.x; i < len; i += gridDim.x * zamd::kLoThreads) zamd::LoHashLane(P, t, i);
}

__global__ __launch_bounds__(zamd::kLoThreads) void k_png_lo_links(zamd::LoParams P) {
  __shared__ u32 s_h[zamd::kLoThreads], s_z[zamd::kLoThreads];
  __shared__ u8 s_nexth[zamd::kLoThreads], s_nextz[zamd::kLoThreads];
  const u32 t = blockIdx.x, len = P.tiles[t].len;
  for (u32 b0 = 0; b0 < len; b0 += zamd::kLoThreads) {
    zamd::LoLinksLoad(P, t, b0, threadIdx.x, s_h, s_z, s_nexth, s_nextz);
    __syncthreads();
    zamd::LoLinksFind(P, t, b0, threadIdx.x, s_h, s_z, s_nexth, s_nextz);
    __syncthreads();
    zamd::LoLinksPublish(P, t, b0, threadIdx.x, s_h, s_z, s_nexth, s_nextz);
    __threadfence_block();
    __syncthreads();
  }
}

__global__ __launch_bounds__(zamd::kLoThreads) void k_png_lo_ask(zamd::LoParams P, u32 tile0) {
  const u32 t = tile0 + blockIdx.y, len = P.tiles[t].len;
  for (u32 i = blockIdx.x * zamd::kLoThreads + threadIdx.x; i < len; i += gridDim.x * zamd::kLoThreads) zamd::LoAskLane(P, t, i);
}

__global__ __launch_bounds__(zamd::kLoThreads) void k_png_lo_keep(zamd::LoParams P, u32 tile0) {
  const u32 t = tile0 + blockIdx.y, len = P.tiles[t].len;
  for (u32 i = blockIdx.x * zamd::kLoThreads + threadIdx.x; i < len; i += gridDim.x * zamd::kLoThreads) zamd::LoKeepLane(P, t, i);
}

__global__ __launch_bounds__(zamd::kLoThreads) void k_png_lo_search(zamd::LoParams P, u32 tile0) {
  const u32 t = tile0 + blockIdx.y, len = P.tiles[t].len;
  for (u32 i = blockIdx.x * zamd::kLoThreads + threadIdx.x; i < len; i += gridDim.x * zamd::kLoThreads) zamd::LoSearchLane(P, t, i);
}

// one wave per deflate block
__global__ __launch_bounds__(64) void k_png_lo_parse(zamd::LoParams P) {
  __shared__ u32 s_ld[zamd::kLoParseChunk];
  __shared__ u8 s_f[zamd::kLoParseChunk];
  __shared__ u32 s_cnt[316];
  const u32 lane = threadIdx.x;
  const zamd::LoTile K = P.blocks[blockIdx.x];
  const zamd::LoBuf B = P.bufs[K.buf];
  const u32* LD = P.LD + B.base + K.start;
  const u8* F = B.data + K.start;
  for (u32 i = lane; i < 316u; i += 64u) s_cnt[i] = 0;
  u32 c0 = 0, c1 = 0;   // the staged positions [c0, c1) of the block; the same in every lane
  const u64 extra = zamd::LoParseBlock(
      K.len, P.window,
      [&](u32 pos, u32* byte) {
        if (pos >= c1) {
          __syncthreads();
          c0 = pos;
          c1 = K.len - c0 < zamd::kLoParseChunk ? K.len : c0 + zamd::kLoParseChunk;
          for (u32 i = lane; i < c1 - c0; i += 64u) {
            s_ld[i] = LD[c0 + i];
            s_f[i] = F[c0 + i];
          }
          __syncthreads();
        }
        *byte = s_f[pos - c0];
        return s_ld[pos - c0];
      },
      [&](u32 symbol) {
        if (lane == 0) ++s_cnt[symbol];
      });
  __syncthreads();
  u32* out = P.counts + (u64)blockIdx.x * zamd::kLoCountWords;
  for (u32 i = lane; i < 316u; i += 64u) out[i] = s_cnt[i];
  if (lane == 0) {
    out[316] = (u32)extra;
    out[317] = (u32)(extra >> 32);
  }
}

#endif  // ZMX_PNG_LODEFLATE_KERNELS
#endif  // ZMX_PNG_LODEFLATE_H_
