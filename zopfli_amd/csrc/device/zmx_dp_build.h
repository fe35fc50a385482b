// What the table build leaves for the chain's kernels, once per table set: the window records (k_mkdesc), the tasks'
// starts at cut points of the DP (k_cutpoints), the kind of each task (k_taskkind).  Included only by zmx_hip.hip,
// after zmx_dp4.h (SegTask) and before zmx_dp5.h, whose job reads the records.
#pragma once

// What k_dp5_spec needs to fetch the rows of a 32-position window (aligned to the block start).  The rows of
// consecutive positions are consecutive in codes[] (dph's offsets are a running sum of the row lengths), so the
// wave copies the window's codes into LDS in one piece and lane l finds code l - u - 1 of row u at index
// rel[u] + l of the copy.  Everything a window needs besides the codes is ONE 40-word record (wmeta), fetched by
// ONE vector load a window ahead: words 0..31 = (rel[u] + 32) << 16 | kend[u], 32 / 33 = where the window's rows
// start / end in the block's codes, 34 = the window's class (1 = 32 positions, none flagged for the long-run
// shortcut, no edge beyond cell register 0; 2 = none flagged, edges of any length; 0 = neither).
//
// Why this shape — what round 2 measured on the way (all bit-exact, profiles/): a 16-byte buffer descriptor per
// position and a buffer_load per row: the CU's address unit is busy 16 cycles per wave-wide load whatever the
// lanes do, 256 cycles per position with 16 waves; descriptors built by SALU from packed row lengths: 30
// instructions per position around a chain step of six, and a wave issues one instruction per four cycles at
// best; s_load for the per-window words: SMEM shares its counter with LDS, so nothing scalar can be in flight
// across a window; and, throughout, three dependent memory round trips per window that four waves per SIMD do
// not hide (95 % of a window's 9 000 cycles were waiting).
#define D5_WM 40u          // words per window in wmeta[]
#define D5_WF_CODELESS 0x100u   // winflag / wmeta word 34, beside the window's kind in the low byte: a row without codes (k_rowscan)
struct MkDescParams {
  const BlockDesc* blocks;
  const uint2* dph;
  u32* wmeta;           // [windows + 1 per block][D5_WM]
  u32* winroff;         // [windows + 1 per block] = wmeta word 32 (the scalar path of windows nobody prefetched)
  const u32* win_off;   // [nb] first window of each block in winflag[] / winroff[] / wmeta[]
  u32* winflag;         // [windows + 1 per block] = wmeta word 34
};

__global__ __launch_bounds__(256) void k_mkdesc(MkDescParams P) {
  const BlockDesc bd = P.blocks[blockIdx.y];
  const u32 B = (u32)(bd.inend - bd.instart);
  const u32 p = blockIdx.x * 256u + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  uint2 dhw = make_uint2(0, 0);
  if (p < B) dhw = P.dph[bd.pos_off + p];
  // (whole waves take part in the ballots and the shuffle; a wave covers two windows)
  const bool flagged = p >= B || ((dhw.y >> 16) & 1u) != 0;
  const u64 not1 = __ballot(flagged || (dhw.y & 0xffffu) + (lane & 31u) >= 64u);    // an edge beyond cell register 0
  // flagged for the shortcut, or short — or a wide run row (k_rowscan): those go position by position, where their
  // weights come from the run-row table instead of six scattered code loads (d5_run_job)
  const u64 not2 = __ballot(flagged || (((dhw.y >> 17) & 1u) != 0 && (dhw.y & 0xffffu) >= 64u));
  // a row that reaches beyond cell register 1: kind 3 = kind 2 with such rows.  The text variant of the job takes it as
  // kind 2 (the rest of such a row on demand: rare there); the run variant position by position with staged codes
  // (the last 257 positions of every run of class Z are such rows: 1 800 cycles a position as kind 2)
  const u64 far3 = __ballot(p < B && (dhw.y & 0xffffu) + (lane & 31u) >= 128u);
  const u32 first = (u32)__shfl((int)dhw.x, (int)(lane & 32u), 64);                  // row offset of the window's first position
  const u32 w = P.win_off[blockIdx.y] + (p >> 5);
  u32* wm = P.wmeta + (u64)w * D5_WM;
  const u32 kend = dhw.y & 0xffffu;
  const u32 klay = dph_layout_len(dhw.y);      // (what the row takes in codes[]: nothing for a wide run row)
  const u64 nocodes = __ballot(p < B && (dhw.y & DPH_CODELESS) != 0);
  if (p < ((B + 31u) & ~31u)) wm[p & 31u] = p < B ? ((dhw.x - first + 32u - ((p & 31u) + 1u)) << 16) | kend : 0u;
  if ((lane & 31u) == 0 && p < B) {
    const u32 sh = lane & 32u;
    // (bit 8, D5_WF_CODELESS: a row of the window has no codes — such a window is of kind 0, and a task that holds one is
    //  re-run by the lean one-wave job, never by k_dp4's pipeline, whose ring expects every row's codes)
    const u32 f = ((u32)(not1 >> sh) == 0 ? 1u : (u32)(not2 >> sh) != 0 ? 0u : (u32)(far3 >> sh) == 0 ? 2u : 3u) |
                  ((u32)(nocodes >> sh) != 0 ? D5_WF_CODELESS : 0u);
    P.winflag[w] = f;
    P.winroff[w] = dhw.x;
    wm[32] = dhw.x;
    wm[34] = f;
  }
  if (p < B && ((p & 31u) == 31u || p + 1 == B)) wm[33] = dhw.x + klay;           // where the window's rows end
  if (p + 1 == B) {      // one record past the last window: where the block's rows end, class 0
    P.winroff[w + 1] = dhw.x + klay;
    P.winflag[w + 1] = 0;
    wm[D5_WM + 32] = dhw.x + klay;
    wm[D5_WM + 33] = dhw.x + klay;
    wm[D5_WM + 34] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// CUT POINTS.  A position q that no DP edge crosses — p + kend(p) <= q for every p < q (kend: the longest
// match at p, or 1 for the literal: dph[p].y) — splits GetBestLengths exactly: every cell beyond q gets its
// value through cell q alone, so a chain started at q from ONE cell is the true chain shifted by a constant,
// with no warm-up and nothing left to chance (a long-run shortcut cannot span a cut either: the run's own
// matches would cross it).  Text has one every ~25 positions (largest gap seen: 688), data made of long runs
// almost none.  One wave per task looks for the last cut point q in [pout - depth, pout) — in [1, pout) where
// pout <= depth + 258: the scan then starts at the block's first position, its prefix maximum is the true one
// everywhere, and an older cut point is as exact and still cheaper than a warm-up — and makes it the task's
// start (SegTask.q, which then need not be a multiple of 32: k_dp5_spec starts at the window that holds it,
// with the level in that window's cell); tasks without one keep the warm-up.
// ---------------------------------------------------------------------------------------------
struct CutParams {
  const BlockDesc* blocks;
  const uint2* dph;
  SegTask* tasks;
  u32 depth;
  u32 warm;        // the warm-up a task without a cut point would get
  u32* found;      // [2]: tasks that got a cut point, sum of (pout - q) over them
  u32* wide;       // [tasks]: 1 = no cut point, and the warm-up stretch holds long-run material (see below)
};

// A task that finds no cut point has to rely on coalescence (zmx_dp4.h) over its warm-up stretch.  Inside and
// behind runs of equal bytes that does not happen: the long-run shortcut (squeeze.c:251-271) copies 258 cells
// unmixed, and where every row is 258 edges of one distance the paths run side by side — measured on class Z,
// 90 % of such tasks were re-run serially.  So a task whose warm-up stretch holds a shortcut position or a run row
// of 64+ edges is not started at all: the host merges it into its predecessor (BuildTables), whose own start IS a
// cut point (or the block's head) — tasks become the stretches between cut points there, every one exact by
// construction, and the only thing left to verify is the level.
__global__ __launch_bounds__(64) void k_cutpoints(CutParams P) {
  const u32 t = blockIdx.x;
  const SegTask K = P.tasks[t];
  if (K.pout == 0) return;      // the head of a block starts from the block's true state
  const BlockDesc bd = P.blocks[K.block];
  const uint2* dph = P.dph + bd.pos_off;
  const u32 lane = threadIdx.x;
  const u32 lo = K.pout > P.depth + ZMX_MAX_MATCH ? K.pout - P.depth - ZMX_MAX_MATCH : 0u;
  const u32 wlo = K.pout > P.warm ? K.pout - P.warm : 0u;
  // the prefix maximum from lo on is the true one for q >= lo + 258 (no edge is longer), and for every q if lo = 0
  const u32 q_min = lo == 0 ? 1u : lo + ZMX_MAX_MATCH;
  // the whole warm-up stretch is looked at for long-run material, also where it begins before lo (a warm-up longer than
  // depth + 258): a prefix maximum from an earlier start is as true from q_min on
  const u32 scan_lo = wlo < lo ? wlo : lo;
  u32 carry = 0, best = SEG_NONE;
  bool wide = false;
  for (u32 p0 = scan_lo; p0 < K.pout; p0 += 64) {
    const u32 p = p0 + lane;
    const u32 y = p < K.pout ? dph[p].y : 0u;
    const u32 r = p < K.pout ? p + (y & 0xffffu) : 0u;
    wide |= p >= wlo && (((y >> 16) & 1u) != 0 || (((y >> 17) & 1u) != 0 && (y & 0xffffu) >= 64u));
    u32 incl = wave_scan_max(r);
    incl = incl > carry ? incl : carry;
    // q = p + 1 is a cut point; not pout itself: the start cell has no source, and the cells from pout on are
    // compared with the predecessor's, sources included
    const u64 ok = __ballot(p + 1 < K.pout && p + 1 >= q_min && incl <= p + 1);
    if (ok) best = p0 + (63u - (u32)__builtin_clzll(ok)) + 1u;
    carry = rdlane_u32(incl, 63);
  }
  const bool any_wide = __any(wide);
  if (lane == 0) {
    P.wide[t] = best == SEG_NONE && any_wide ? 1u : 0u;
    if (best != SEG_NONE) {
      P.tasks[t].q = best;
      atomicAdd(&P.found[0], 1u);
      atomicAdd(&P.found[1], K.pout - best);
    }
  }
}

// Which of the two k_dp5_spec variants a task is for: 1 = at least a quarter of its 32-position windows are of the
// generic kind (shortcut positions, wide run rows: k_mkdesc), i.e. it walks runs of equal bytes.  One wave per task.
struct TaskKindParams {
  const SegTask* tasks;
  const BlockDesc* blocks;
  const u32* winflag;
  const u32* win_off;
  u32* kind;
};
__global__ __launch_bounds__(64) void k_taskkind(TaskKindParams P) {
  const u32 t = blockIdx.x;
  const SegTask K = P.tasks[t];
  const BlockDesc bd = P.blocks[K.block];
  const u32 B = (u32)(bd.inend - bd.instart);
  const u32* wf = P.winflag + P.win_off[K.block];
  const u32 w0 = K.q >> 5, w1 = ((K.pend < B ? K.pend : B) + 31u) >> 5;
  u32 g = 0;
  for (u32 w = w0 + threadIdx.x; w < w1; w += 64) g += (wf[w] & 0xffu) == 0 || (wf[w] & 0xffu) == 3 ? 1u : 0u;
  g = wave_scan_add(g);
  if (threadIdx.x == 63) P.kind[t] = 4u * g >= (w1 - w0) && g >= 4u ? 1u : 0u;
}
