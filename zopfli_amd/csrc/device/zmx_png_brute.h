// LodePNG's LFS_BRUTE_FORCE row search on the device: for every scanline, which of the five PNG filter
// types gives the smallest zlib stream of that row alone under LodePNG's own fixed-tree deflate (lodepng.cpp:5585-5632:
// `zlib_compress` of each filtered version with btype 1, the caller's window, minmatch 3, nicematch 128, lazy matching;
// the first smallest in BYTES wins).  zopflipng's `b` strategy.  Included only by zmx_hip.hip.
//
// The size is encodeLZ77's (:1593-1740) exactly, in a parallel form (tools/models/png_brute_model.cc checks it against
// lodepng_zlib_compress on the CPU).  LodePNG inserts every position of the row into its hash state once, in order, and
// searches at a position right after inserting it (the lazy roll-back re-inserts a position into the same state).  So
// the search at `pos` sees "positions 0..pos inserted", and that state is a function of the row alone:
//   H[p]   getHash (:1544-1561, the short hash within two bytes of the end);
//   Z[p]   countZeros where H[p] == 0, else 0 (the `numzeros` rule, :1626-1631);
//   C[p]   what inserting p writes into chain[p & M]: the slot of the last q < p with H[q] == H[p] (`head` is never
//          cleared), else what the slot held before — C[p - W], or the slot itself ("uninitialised") when p < W;
//   CZ[p]  the same for chainz under the key Z;
// and slot s, read during the search at pos, holds what its latest position pos - ((pos - s) & M) wrote.  Stale `val`,
// `chain[i] == i` and the wrap test `current_offset < prev_offset` then end the walks as in LodePNG, rows longer than
// the window included.  One job = one (row, filter type), one workgroup at a time:
//   1. the filtered row F (filterScanline, :5379-5421) from the raw row and the raw row above;
//   2. H and the zero runs (from their starts), Z = the run where H == 0;
//   3. C / CZ 1024 positions at a time: a lane finds its key's last earlier lane in the chunk, else asks the head tables
//      (`head` in global scratch, 65536 entries; `headz` in LDS); the chunk's last lane of every key updates them; the
//      "keep" links are resolved afterwards per residue class mod W;
//   4. the match search at every position, a lane per position (the chain walk bounded by maxchainlength);
//   5. one lane replays the lazy parse (:1691-1736) over the per-position (length, offset) and sums the fixed-code bits:
//      size = 2 + ceil((3 + bits + 7) / 8) + 4.
// The per-position arrays (F, then H << 16 | C and Z << 16 | CZ packed: one load per chain step gives the hash to check
// AND the next link) live in the dynamic LDS when the row fits (rows of up to 16839 bytes: 4096 RGBA pixels fit), else in the
// workgroup's slice of the global scratch; the search results (length | offset << 16) go to the scratch and are read
// back into the LDS (over the packed arrays, dead by then) for the serial scan.  The grid is persistent so that the
// scratch is bounded.  k_png_brute_pick then takes the first smallest of the five sizes per row.
#pragma once

#define PNGB_THREADS 1024u
#define PNGB_KEEP 0xffffu
#define PNGB_HEAD_BYTES (65536u * 4u)
#define PNGB_LDS_MAX (148u * 1024u)   // dynamic LDS beside the static ~11 KiB, within the CU's 160 KiB

struct PngBruteParams {
  const u8* image;       // height rows of linebytes bytes
  u32 linebytes, height, bytewidth, window;
  u32 jobs;              // height * 5: job = row * 5 + type
  u8* scratch;           // per workgroup: head[65536] (u32, position + 1), LD[n], then the per-position arrays unless in LDS
  u64 scratch_stride;    // bytes per workgroup
  u32 in_lds;            // the per-position arrays live in the dynamic LDS
  u64* sizes;            // [jobs] the zlib size of the row under each type
  u64* bits = nullptr;   // [jobs] or null: step 5's bit count before it is rounded to bytes (zmx_internal_png_brute_sizes)
};

// bytes of the per-position arrays of a row of n bytes: F (u8, padded to 4), HC, ZC (u32)
__host__ __device__ __forceinline__ u64 pngb_row_bytes(u32 n) { return (u64)((n + 3u) & ~3u) + 8ull * n; }

__device__ __forceinline__ u32 pngb_length_extra(u32 l) { return (l <= 10u || l == 258u) ? 0u : (31u - (u32)__clz((int)(l - 3u))) - 2u; }
__device__ __forceinline__ u32 pngb_dist_extra(u32 d) { return d <= 4u ? 0u : (31u - (u32)__clz((int)(d - 1u))) - 1u; }

__global__ __launch_bounds__(PNGB_THREADS) void k_png_brute(PngBruteParams P) {
  extern __shared__ __align__(16) u8 s_dyn[];
  __shared__ u32 s_h[PNGB_THREADS], s_z[PNGB_THREADS];
  __shared__ u8 s_nexth[PNGB_THREADS], s_nextz[PNGB_THREADS];
  __shared__ int s_headz[259];
  const u32 tid = threadIdx.x;
  const u32 n = P.linebytes, bw = P.bytewidth, W = P.window, M = W - 1u;
  const u32 n4 = (n + 3u) & ~3u;
  const u32 maxchain = W >= 8192u ? W : W / 8u, maxlazy = W >= 8192u ? 258u : 64u;
  u8* const mine = P.scratch + (u64)blockIdx.x * P.scratch_stride;
  u32* const head = reinterpret_cast<u32*>(mine);
  u32* const LDg = reinterpret_cast<u32*>(mine + PNGB_HEAD_BYTES);
  u8* const base = P.in_lds ? s_dyn : mine + PNGB_HEAD_BYTES + 4ull * n;
  u8* const F = base;
  u32* const HC = reinterpret_cast<u32*>(base + n4);   // H << 16 | C
  u32* const ZC = HC + n;                              // Z << 16 | CZ
  u32* const LD = P.in_lds ? HC : LDg;                 // (the scan's copy of the results)
  for (u32 job = blockIdx.x; job < P.jobs; job += gridDim.x) {
    const u32 y = job / 5u, t = job - 5u * y;
    const u8* row = P.image + (u64)y * n;
    const u8* prev = y ? row - n : nullptr;
    // 1. the filtered row (lodepng.cpp:5379-5421, as k_png_filter_types), the head tables cleared
    for (u32 x = tid; x < n; x += PNGB_THREADS) {
      const int s = row[x];
      const int a = x >= bw ? row[x - bw] : 0;
      const int b = prev ? prev[x] : 0;
      const int c = (prev && x >= bw) ? prev[x - bw] : 0;
      int v = s;
      if (t == 1u) v = s - a;
      else if (t == 2u) v = s - b;
      else if (t == 3u) v = s - ((a + b) >> 1);
      else if (t == 4u) v = s - (int)pngf_paeth(a, b, c);
      F[x] = (u8)(v & 255);
    }
#pragma unroll 1
    for (u32 i = tid; i < 65536u; i += PNGB_THREADS) head[i] = 0u;
    for (u32 i = tid; i < 259u; i += PNGB_THREADS) s_headz[i] = -1;
    __syncthreads();
    // 2. hash (getHash) and the zero runs, written by the lane at each run's start (capped at 258 and the row's end)
    for (u32 p = tid; p < n; p += PNGB_THREADS) {
      u32 h;
      if (p + 2u < n) h = (u32)F[p] ^ ((u32)F[p + 1] << 4) ^ ((u32)F[p + 2] << 8);
      else h = (u32)F[p] ^ (p + 1u < n ? (u32)F[p + 1] << 8 : 0u);
      HC[p] = (h & 65535u) << 16;
      if (F[p] != 0) {
        ZC[p] = 0;
      } else if (p == 0 || F[p - 1] != 0) {
        u32 e = p;
#pragma unroll 1
        while (e < n && F[e] == 0) ++e;
#pragma unroll 1
        for (u32 k = p; k < e; ++k) ZC[k] = min(e - k, 258u) << 16;
      }
    }
    __syncthreads();
    for (u32 p = tid; p < n; p += PNGB_THREADS)
      if ((HC[p] >> 16) != 0) ZC[p] = 0;
    __syncthreads();
    // 3. the chain links, a chunk of PNGB_THREADS positions at a time
    for (u32 b0 = 0; b0 < n; b0 += PNGB_THREADS) {
      const u32 p = b0 + tid;
      const bool live = p < n;
      const u32 h = live ? HC[p] >> 16 : 0xffffffffu, z = live ? ZC[p] >> 16 : 0xffffffffu;
      s_h[tid] = h;
      s_z[tid] = z;
      s_nexth[tid] = 0;
      s_nextz[tid] = 0;
      __syncthreads();
      if (live) {
        int j = (int)tid - 1;
        while (j >= 0 && s_h[j] != h) --j;
        u32 c;
        if (j >= 0) {
          c = (b0 + (u32)j) & M;
          s_nexth[j] = 1;
        } else {
          const u32 hp = head[h];
          c = hp ? (hp - 1u) & M : PNGB_KEEP;
        }
        int k = (int)tid - 1;
        while (k >= 0 && s_z[k] != z) --k;
        u32 cz;
        if (k >= 0) {
          cz = (b0 + (u32)k) & M;
          s_nextz[k] = 1;
        } else {
          const int hz = s_headz[z];
          cz = hz >= 0 ? (u32)hz & M : PNGB_KEEP;
        }
        HC[p] = (h << 16) | c;
        ZC[p] = (z << 16) | cz;
      }
      __syncthreads();
      if (live) {
        if (!s_nexth[tid]) head[h] = p + 1u;
        if (!s_nextz[tid]) s_headz[z] = (int)p;
      }
      __syncthreads();
    }
    // ... the links that keep what the slot held: C[p - W], or the slot itself (one lane per residue class)
    for (u32 r = tid; r < n && r < W; r += PNGB_THREADS) {
      u32 pc = r, pz = r;
      for (u32 p = r; p < n; p += W) {
        const u32 hc = HC[p], zc = ZC[p];
        u32 c = hc & 0xffffu, cz = zc & 0xffffu;
        if (c == PNGB_KEEP) HC[p] = (hc & 0xffff0000u) | (c = pc);
        if (cz == PNGB_KEEP) ZC[p] = (zc & 0xffff0000u) | (cz = pz);
        pc = c;
        pz = cz;
      }
    }
    __syncthreads();
    // 4. the longest-match search at every position (lodepng.cpp:1636-1689) on the state "0..pos inserted";
    //    `node` = HC of the position slot `hashpos` holds, carried from the step that checked its hash
    for (u32 pos = tid; pos < n; pos += PNGB_THREADS) {
      const u32 wpos = pos & M, self = HC[pos], hv = self >> 16, nz = ZC[pos] >> 16;
      const u32 last = min(n, pos + 258u);
      u32 length = 0, offset = 0, hashpos = self & 0xffffu, prev_offset = 0, chainlength = 0;
      u32 node = ((wpos - hashpos) & M) <= pos ? HC[pos - ((wpos - hashpos) & M)] : 0u;
      for (;;) {
        if (chainlength++ >= maxchain) break;
        const u32 cur = hashpos <= wpos ? wpos - hashpos : wpos - hashpos + W;
        if (cur < prev_offset) break;
        prev_offset = cur;
        if (cur > pos) break;     // a slot no position has written yet: LodePNG only reaches those as chain[i] == i
        const u32 q = pos - cur;  // the position that slot `hashpos` holds
        if (cur > 0) {
          u32 fo = pos, ba = q;
          if (nz >= 3u) {
            const u32 skip = min(ZC[q] >> 16, nz);
            fo += skip;
            ba += skip;
          }
#pragma unroll 1
          while (fo != last && F[ba] == F[fo]) { ++fo; ++ba; }
          const u32 cl = fo - pos;
          if (cl > length) {
            length = cl;
            offset = cur;
            if (cl >= 128u) break;     // nicematch
          }
        }
        const u32 chainv = node & 0xffffu;
        if (hashpos == chainv) break;
        if (nz >= 3u && length > nz) {
          hashpos = ZC[q] & 0xffffu;
          const u32 c2 = (wpos - hashpos) & M;
          if (c2 > pos || (ZC[pos - c2] >> 16) != nz) break;
          node = HC[pos - c2];
        } else {
          hashpos = chainv;
          const u32 c2 = (wpos - hashpos) & M;
          if (c2 > pos) break;
          node = HC[pos - c2];
          if ((node >> 16) != hv) break;
        }
      }
      LDg[pos] = length | (offset << 16);
    }
    __syncthreads();
    if (P.in_lds) {           // the results into the LDS, over the packed arrays
      for (u32 p = tid; p < n; p += PNGB_THREADS) LD[p] = LDg[p];
      __syncthreads();
    }
    // 5. the lazy parse and the fixed-code bits (lodepng.cpp:1691-1736, :2029-2072)
    if (tid == 0) {
      u64 bits = 3u + 7u;
      u32 lazy = 0, ll = 0, lo = 0;
      for (u32 pos = 0; pos < n; ++pos) {
        const u32 v = LD[pos];
        u32 length = v & 0xffffu, offset = v >> 16;
        if (!lazy && length >= 3u && length <= maxlazy && length < 258u) {
          lazy = 1;
          ll = length;
          lo = offset;
          continue;
        }
        if (lazy) {
          lazy = 0;
          if (length > ll + 1u) {
            bits += F[pos - 1] < 144 ? 8u : 9u;
          } else {
            length = ll;
            offset = lo;
            --pos;
          }
        }
        if (length < 3u || (length == 3u && offset > 4096u)) {
          bits += F[pos] < 144 ? 8u : 9u;
        } else {
          bits += (length <= 114u ? 7u : 8u) + pngb_length_extra(length) + 5u + pngb_dist_extra(offset);
          pos += length - 1u;
        }
      }
      P.sizes[job] = 6u + (bits + 7u) / 8u;
      if (P.bits) P.bits[job] = bits;
    }
    __syncthreads();
  }
}

// the first smallest of the five sizes of every row (lodepng.cpp:5621)
__global__ __launch_bounds__(256) void k_png_brute_pick(const u64* __restrict__ sizes, u32 height, u8* __restrict__ types) {
  const u32 y = blockIdx.x * 256u + threadIdx.x;
  if (y >= height) return;
  u32 best = 0;
  u64 smallest = 0;
  for (u32 t = 0; t < 5u; ++t) {
    const u64 s = sizes[(u64)y * 5u + t];
    if (t == 0 || s < smallest) { best = t; smallest = s; }
  }
  types[y] = (u8)best;
}
