// Driver part: building a table set phase by phase — SegL, SegHead, LayoutBlocks through FillTableParams, BuildTables, the three
// build entries.  Needs drv_context.h (PoolAlloc, PoolScope, MatchKernel, MatchOrder) and drv_tables.h (zmx_tables, CheckTables).
#pragma once

constexpr u32 kMatchGrid = 1024;  // persistent workgroups: 256 CUs x 4 (LDS-limited)
constexpr u32 kMatchGrid5 = 1536; // k_match5: 256 CUs x 6 workgroups of 4 waves (its scratch is k_match2's: 1536 x 256 <= 1024 x 512 lanes)

extern "C" {
// Task length of the chain (zmx_dp4.h).  A task is one serial wave, and a run is at least a task, a second-pass task and the
// serial re-runs long: with little to do (small calls: zopflipng's IDATs, files of a MB or less) short tasks cut
// that latency (1 MB: 53 -> 47 ms, 64 KiB: 32 -> 24 ms) although every task pays its 512-position warm-up; with
// a full batch 2048 and 4096 run alike and the longer tasks walk fewer positions.  ZOPFLI_AMD_SEG_L overrides
// (0 = no tasks: the serial chain).
static unsigned SegL(u64 total_positions) {
  if (Knobs().seg_l_set) return Knobs().seg_l;
  // (a shard of a dealt call: the call's positions on this device, not the context's share — zamd::CallPositions.  Through
  //  ZopfliCompress 100 MB of text are three shares of 33 M positions, which took 1024 below: 112.2 ms a step against 107.0
  //  with 2048, three lines a side, spread 0.2 and 0.8 ms: profiles/chain_stretch.txt)
  total_positions = std::max<u64>(total_positions, zamd::CallPositions());
  // (with the tasks started at cut points, below, the warm-up is ~70 positions instead of 512 and 2048 beats 4096
  //  for a full batch too: half the positions re-run where a task crosses a binade, 4.17 -> 3.75 ms per run of 100 MB;
  //  1024 loses to the per-task set-up again: 4.2 ms)
  // (a call of 64 KiB is 64 tasks of 1024 positions on 256 CUs: 512 halves the latency of every pass — 18.6 -> 16.8 ms
  //  for the call —, at 1 MB 512 loses to the per-task set-up again: 39 -> 44 ms)
  // (round 5: with k_dp4_fix judging a chunk's tasks at once the per-task set-up is gone and short tasks win further up —
  //  64 KiB: 256 13.2 ms against 13.8 with 512; 1 MB: 512 23.1 against 24.1 with 1024; 4 MB: 512 33.6 against 38.1;
  //  100 MB: 2048 3.63 ms per run against 3.94 with 1024 — tools/r05_segl.sh)
  return total_positions <= (128u << 10) ? 256u : total_positions <= (16u << 20) ? 512u : total_positions <= (48u << 20) ? 1024u : 2048u;
}
// The exact head of a block (positions run from the true initial state; the values double every few hundred
// positions there and speculative tasks would not stay inside a binade).  It is one serial wave: with few blocks in
// the batch the whole run waits for it (short: 4096), with many it hides behind the other tasks and a long head
// saves the serial re-runs of the early tasks (8192; 16384 and 4096 are within 1 %).  ZOPFLI_AMD_SEG_HEAD overrides.
static unsigned SegHead(size_t nb) {
  const unsigned v = Knobs().seg_head;
  return v ? v : (nb >= 48 ? 8192u : 0u);       // (0: as long as a task)
}

// ---------------------------------------------------------------------------------------------
// BuildTables, phase by phase.  Every phase works on `c->stream` and returns 0, or what BuildTables returns for the
// failure (-1 with the error set: HIPCHK).
// ---------------------------------------------------------------------------------------------

// Phase 1: where each block's window, positions and length-array entries lie, and the totals (t->total_b positions,
// t->total_l window entries, t->tile_off); *la_total = length-array entries, *max_window = the longest window.
static int LayoutBlocks(zmx_ctx* c, const zmx_block* blocks, size_t nb, zmx_tables* t, u64* la_total, u64* max_window) {
  t->nb = nb;
  t->blocks.resize(nb);
  t->bsize.resize(nb);
  t->store_begin[0].assign(nb, 0);
  t->store_begin[1].assign(nb, 0);
  std::vector<u32> tile_off(nb + 1, 0);
  u64 pos_off = 0, reg_off = 0, la_off = 0, max_l = 0;
  for (size_t b = 0; b < nb; ++b) {
    if (blocks[b].inend < blocks[b].instart || blocks[b].inend > c->insize) {
      return FailMsg("zmx_tables_build: block outside the resident input");
    }
    BlockDesc& d = t->blocks[b];
    d.instart = blocks[b].instart;
    d.inend = blocks[b].inend;
    d.ws = d.instart > ZMX_WINDOW ? d.instart - ZMX_WINDOW : 0;
    if (!c->seg_starts.empty()) {
      // the segment of the block's first byte (the last of several that start there: the empty ones hold no block)
      const size_t k = static_cast<size_t>(std::upper_bound(c->seg_starts.begin(), c->seg_starts.end(), d.instart) -
                                           c->seg_starts.begin()) - 1;
      const u64 seg_end = k + 1 < c->seg_starts.size() ? c->seg_starts[k + 1] : c->insize;
      if (d.inend > seg_end) return FailMsg("zmx_tables_build: block spans two input segments (zmx_set_input_segments)");
      d.ws = std::max<u64>(d.ws, c->seg_starts[k]);
    }
    d.pos_off = pos_off;
    d.reg_off = reg_off;
    d.la_off = la_off;
    const u64 B = d.inend - d.instart, L = d.inend - d.ws;
    if (B > 0x7fff0000ull) return FailMsg("zmx_tables_build: block too large (positions are 32-bit)");
    t->bsize[b] = static_cast<u32>(B);
    pos_off += B;
    reg_off += (L + 7) & ~7ull;
    la_off += (B + 1 + 7) & ~7ull;
    max_l = std::max(max_l, L);
    tile_off[b + 1] = tile_off[b] + static_cast<u32>((B + MT - 1) / MT);
  }
  t->total_b = pos_off;
  t->total_l = reg_off;
  t->tile_off = tile_off;
  *la_total = la_off;
  *max_window = max_l;
  return 0;
}

// Phase 2 (host only): what a table set over sub-blocks of `parent`'s blocks takes from the parent.
struct ReusePlan {
  bool reuse = false;
  std::vector<u64> src_pos;       // per block: its first record in the parent's d_recs
  std::vector<u64> link_lo;       // per block: first links[] index the recomputed tiles read (its L: none)
  std::vector<u32> tile_list;     // the tiles whose records are computed again
};
// `tail_r` (an input that came from device memory): every block's zamd::TailRunStart, from k_tail_runs.
static ReusePlan PlanReuse(const zmx_ctx* c, const zmx_tables* t, const zmx_tables* parent, const std::vector<uint64_t>& tail_r) {
  const size_t nb = t->nb;
  const u64 pos_off = t->total_b;
  const std::vector<u32>& tile_off = t->tile_off;
  ReusePlan plan;
  bool reuse = parent != nullptr && parent->nb > 0 && (c->h_in != nullptr || tail_r.size() == nb) && parent->d_recs != nullptr &&
               parent->total_b + pos_off < (3ull << 30);
  if (reuse) {
    plan.src_pos.resize(nb);
    plan.link_lo.resize(nb);
    size_t pb = 0;
    for (size_t b = 0; b < nb && reuse; ++b) {
      const BlockDesc& d = t->blocks[b];
      while (pb < parent->nb && parent->blocks[pb].inend < d.inend) ++pb;   // both lists are ascending
      if (pb == parent->nb || d.instart < parent->blocks[pb].instart || d.inend > parent->blocks[pb].inend) {
        reuse = false;
        break;
      }
      const BlockDesc& pd = parent->blocks[pb];
      plan.src_pos[b] = pd.pos_off + (d.instart - pd.instart);
      const u64 B = d.inend - d.instart;
      plan.link_lo[b] = d.inend - d.ws;
      if (B == 0 || d.inend == pd.inend) continue;   // same end: every record is the same
      // first position whose record may differ
      u64 t0 = B > ZMX_MAX_MATCH ? d.inend - ZMX_MAX_MATCH : d.instart;
      const u64 r = c->h_in ? zamd::TailRunStart(c->h_in, d.instart, d.inend) : tail_r[b];
      if (r < t0) t0 = r;
      const u32 tile_first = static_cast<u32>((t0 - d.instart) / MT);
      for (u32 tile = tile_first; tile < tile_off[b + 1] - tile_off[b]; ++tile) {
        plan.tile_list.push_back(tile_off[b] + tile);
      }
      // the walks of those tiles stay inside the 32 KiB before them (lz77.c:464)
      const u64 first_index = d.instart + static_cast<u64>(tile_first) * MT - d.ws;
      plan.link_lo[b] = first_index > ZMX_WINDOW ? first_index - ZMX_WINDOW : 0;
    }
  }
  plan.reuse = reuse;
  return plan;
}

// Phase 2, for an input the host holds no copy of: where every block's tail run begins (k_tail_runs), a u64 a block.
static int TailRuns(zmx_ctx* c, const zmx_tables* t, std::vector<uint64_t>* r) {
  const size_t nb = t->nb;
  std::vector<uint64_t> blocks(2 * nb);
  for (size_t b = 0; b < nb; ++b) {
    blocks[2 * b] = t->blocks[b].instart;      // (LayoutBlocks has checked them against the resident input)
    blocks[2 * b + 1] = t->blocks[b].inend;
  }
  PoolScope tmp(c);
  uint64_t* d_blocks = nullptr;
  uint64_t* d_r = nullptr;
  HIPCHK(tmp.Upload(&d_blocks, blocks.data(), 2 * nb, "d_blocks"));
  HIPCHK(tmp.AllocT(&d_r, nb, "d_r"));
  TailRunParams P;
  P.in = c->d_in;
  P.blocks = d_blocks;
  P.r = d_r;
  hipLaunchKernelGGL(k_tail_runs, dim3(static_cast<unsigned>(nb)), dim3(64), 0, c->stream, P);
  KCHK(c, "k_tail_runs");
  r->resize(nb);
  HIPCHK(hipMemcpyAsync(r->data(), d_r, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// Phase 3: the table set's arrays and the mirrors of a squeeze run's input and output.
static int AllocTableArrays(zmx_ctx* c, zmx_tables* t, u64 la_off) {
  const size_t nb = t->nb;
  const u64 pos_off = t->total_b;
  const u64 reg_off = t->total_l;
  const std::vector<u32>& tile_off = t->tile_off;
  HIPCHK(PoolAlloc(c, &t->d_blocks, nb));
  HIPCHK(PoolAlloc(c, &t->d_tile_off, nb + 1));
  HIPCHK(PoolAlloc(c, &t->d_same16, reg_off));
  HIPCHK(PoolAlloc(c, &t->d_links, reg_off));
  HIPCHK(PoolAlloc(c, &t->d_recs, pos_off * 8));
  HIPCHK(PoolAlloc(c, &t->d_la, la_off));
  HIPCHK(PoolAlloc(c, &t->d_store[0], pos_off));
  HIPCHK(PoolAlloc(c, &t->d_store[1], pos_off));
  t->run = RunLayout(nb);
  HIPCHK(PoolAlloc(c, &t->d_runin, t->run.in_bytes));
  HIPCHK(PoolAlloc(c, &t->d_runout, t->run.out_bytes));
  HIPCHK(c->pool.PinnedTake(&t->h_runin, t->run.in_bytes, &t->h_runin_cap));
  HIPCHK(c->pool.PinnedTake(&t->h_runout, t->run.out_bytes, &t->h_runout_cap));
  HIPCHK(hipMemsetAsync(t->run.stats(t->d_runout), 0, RunLayout::stats_and_flags_bytes(), c->stream));
  HIPCHK(PoolAlloc(c, &t->d_dph, pos_off));
  HIPCHK(PoolAlloc(c, &t->d_block_edges, nb));
  t->badpos_words = pos_off / 32 + 4;
  HIPCHK(PoolAlloc(c, &t->d_badpos, t->badpos_words));
  HIPCHK(PoolAlloc(c, &t->d_code_base, nb));
  HIPCHK(PoolAlloc(c, &t->d_wtab, nb * ZMX_WTAB));
  HIPCHK(PoolAlloc(c, &t->d_badcodes, nb * 40));
  HIPCHK(PoolAlloc(c, &t->d_counters, 48));
  HIPCHK(hipMemcpyAsync(t->d_blocks, t->blocks.data(), nb * sizeof(BlockDesc), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(t->d_tile_off, tile_off.data(), (nb + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(t->run.flags(t->d_runout), 0, RunLayout::kFlags * sizeof(u32), c->stream));
  return 0;
}

// What the hash-link phase leaves for the match phase (temporaries of one build: back to the pool when it ends).
struct MatchBuild {
  PoolScope hash_tmp;
  u16* d_lev = nullptr;    // k_levels / k_rank2 (ZOPFLI_AMD_MATCH=5), alive until the match kernel has run
  u16* d_tot2 = nullptr;
  u16* d_rank2 = nullptr;
  uint4* d_xrec = nullptr;
  u32* d_tot12 = nullptr;
  unsigned long long* d_energy = nullptr;   // k_hits (kernel 0 = per block: k_match5 where the chains are long)
  u32* d_cmax = nullptr;                    // k_hits: the chunks' largest classes (k_rank2)
  u8* d_est = nullptr;                      // k_hits: every position's class size as 32 - clz (k_match2's order), or null
  bool skip_any = false, skip_all = false;  // some / all blocks of this build take k_match5
  double skip_positions = 0;                // positions of those blocks
  unsigned long long* d_m5stats = nullptr;  // k_match5's per-wave sums
  bool join_stream2 = false;
  explicit MatchBuild(zmx_ctx* c) : hash_tmp(c) {}
};

// Phase 4: hash links (k_same, k_chain) and, for the blocks that take it, what the skip-walk k_match5 reads.
// d_link_lo = null: whole blocks.
static int LaunchHash(zmx_ctx* c, zmx_tables* t, int mk, u64 max_l, const u64* d_link_lo, MatchBuild& m) {
  const size_t nb = t->nb;
  const u64 reg_off = t->total_l;
  if (max_l == 0) return 0;
  const dim3 g1(static_cast<unsigned>((max_l + 256 * SAME_CH - 1) / (256 * SAME_CH)), static_cast<unsigned>(nb));
  hipLaunchKernelGGL(k_same, g1, dim3(256), 0, c->stream, c->d_in, t->d_blocks, t->d_same16, d_link_lo);
  KCHK(c, "k_same");
  const dim3 g2(static_cast<unsigned>((max_l + CH_EMIT - 1) / CH_EMIT), static_cast<unsigned>(nb), 2);
  hipLaunchKernelGGL(k_chain, g2, dim3(64), CH_LDS_BYTES, c->stream, c->d_in, t->d_blocks, t->d_same16, t->d_links, d_link_lo);
  KCHK(c, "k_chain");
  const bool walks = mk == 5 || mk == 0;     // k_hits decides or k_rank2 needs its maxima
  const bool order = mk != 5 && MatchOrder();  // k_match2 runs and wants the estimates (kernel 2 too: its A/B with 0 stays like for like)
  if ((walks || order) && d_link_lo == nullptr) {
    // The skip-walk (k_match5) for the blocks whose chains are long: k_hits estimates the hits per position the
    // reference's walk would make, block by block; kernel 5 forces it for every block.  (Whole blocks only: a
    // table built from a parent recomputes a few tiles with k_match2.)
    m.skip_any = mk == 5;
    if (mk == 5) for (size_t b = 0; b < nb; ++b) m.skip_positions += static_cast<double>(t->blocks[b].inend - t->blocks[b].instart);
    const unsigned hits_chunks = static_cast<unsigned>((max_l + RK_CH - 1) / RK_CH);
    {
      // k_hits: the blocks' hit estimates (kernel 0: which walk a block gets) and the chunks' largest classes (k_rank2:
      // where the 8192-hit cap can bind)
      if (!m.d_energy) HIPCHK(m.hash_tmp.AllocT(&m.d_energy, nb, "d_energy"));
      if (walks && !m.d_cmax) HIPCHK(m.hash_tmp.AllocT(&m.d_cmax, nb * static_cast<size_t>(hits_chunks) + 1, "d_cmax"));
      if (order && !m.d_est) HIPCHK(m.hash_tmp.AllocT(&m.d_est, reg_off, "d_est"));
      HIPCHK(hipMemsetAsync(m.d_energy, 0, nb * sizeof(unsigned long long), c->stream));
      if (m.d_cmax) HIPCHK(hipMemsetAsync(m.d_cmax, 0, (nb * static_cast<size_t>(hits_chunks) + 1) * sizeof(u32), c->stream));
      HitsParams hp;
      hp.in = c->d_in;
      hp.blocks = t->d_blocks;
      hp.same16 = t->d_same16;
      hp.energy = m.d_energy;
      hp.cmax = m.d_cmax;
      hp.est = m.d_est;
      const dim3 g5(hits_chunks, static_cast<unsigned>(nb));
      hipLaunchKernelGGL(k_hits, g5, dim3(RK_THREADS), 0, c->stream, hp);
      KCHK(c, "k_hits");
    }
    if (!walks) return 0;
    if (mk == 0) {
      std::vector<unsigned long long> energy(nb);
      HIPCHK(hipMemcpyAsync(energy.data(), m.d_energy, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      size_t on = 0;
      for (size_t b = 0; b < nb; ++b) {
        if (energy[b] > Knobs().match_hits * (t->blocks[b].inend - t->blocks[b].ws)) {
          ++on;
          m.skip_positions += static_cast<double>(t->blocks[b].inend - t->blocks[b].instart);
        }
      }
      m.skip_any = on != 0;
      m.skip_all = on == nb;
    }
    if (m.skip_any) {
      if (!m.d_lev) HIPCHK(m.hash_tmp.AllocT(&m.d_lev, static_cast<size_t>(LV_N) * reg_off, "d_lev"));
      if (!m.d_tot2) HIPCHK(m.hash_tmp.AllocT(&m.d_tot2, 2 * reg_off, "d_tot"));
      if (!m.d_rank2) HIPCHK(m.hash_tmp.AllocT(&m.d_rank2, 2 * reg_off, "d_rank"));
      if (!m.d_tot12) HIPCHK(m.hash_tmp.AllocT(&m.d_tot12, reg_off, "d_tot12"));
      if (!m.d_xrec) HIPCHK(m.hash_tmp.AllocT(&m.d_xrec, 2 * reg_off, "d_xrec"));
      LevelParams lp;
      lp.in = c->d_in;
      lp.blocks = t->d_blocks;
      lp.lev = m.d_lev;
      lp.total_l = reg_off;
      lp.energy = mk == 0 ? m.d_energy : nullptr;
      lp.thr = Knobs().match_hits;
      const dim3 g4(static_cast<unsigned>((max_l + LV_CH - 1) / LV_CH), static_cast<unsigned>(nb), LV_N);
      hipLaunchKernelGGL(k_levels, g4, dim3(64), 0, c->stream, lp);
      KCHK(c, "k_levels");
      RankParams rp;
      rp.in = c->d_in;
      rp.blocks = t->d_blocks;
      rp.links = t->d_links;
      rp.same16 = t->d_same16;
      rp.lev = m.d_lev;
      rp.total_l = reg_off;
      rp.tot = m.d_tot2;
      rp.rank = m.d_rank2;
      rp.xrec = m.d_xrec;
      rp.tot12 = m.d_tot12;
      rp.energy = lp.energy;
      rp.thr = lp.thr;
      rp.cmax = m.d_cmax;
      rp.cmax_stride = hits_chunks;
      const dim3 g3(static_cast<unsigned>((max_l + RK_CH - 1) / RK_CH), static_cast<unsigned>(nb));
      hipLaunchKernelGGL(k_rank2, g3, dim3(RK_THREADS), 0, c->stream, rp);
      KCHK(c, "k_rank2");
    }
  }
  return 0;
}
static int BuildHashLinks(zmx_ctx* c, zmx_tables* t, int mk, u64 max_l, const ReusePlan& plan, MatchBuild& m) {
  const size_t nb = t->nb;
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  u64* d_link_lo = nullptr;
  if (plan.reuse) HIPCHK(m.hash_tmp.Upload(&d_link_lo, plan.link_lo.data(), nb, "d_link_lo"));
  if (LaunchHash(c, t, mk, max_l, d_link_lo, m) != 0) return -1;
  t->links_partial = plan.reuse;
  return 0;
}

// Phase 5's match-table kernel over `total_tiles` tiles (all of them, or those of tile_list)
static int LaunchMatch(zmx_ctx* c, zmx_tables* t, int mk, MatchBuild& m, u32* pool, u32 pool_cap, u32 total_tiles, const u32* d_tiles, bool prof) {
  const size_t nb = t->nb;
  if (total_tiles == 0) return 0;
  MatchParams mp;
  mp.in = c->d_in;
  mp.blocks = t->d_blocks;
  mp.tile_off = t->d_tile_off;
  mp.nb = static_cast<u32>(nb);
  mp.total_tiles = total_tiles;
  mp.links = t->d_links;
  mp.recs = t->d_recs;
  mp.pool = pool;
  mp.pool_cap = pool_cap;
  mp.counters = t->d_counters;
  mp.scratch = c->d_scratch;
  mp.tile_list = d_tiles;
  mp.skip_energy = nullptr;
  mp.skip_thr = 0;
  mp.est = d_tiles == nullptr ? m.d_est : nullptr;
  if ((mk == 5 || mk == 0) && d_tiles == nullptr && m.skip_any) {
    if (!c->d_scratch5) HIPCHK(PoolAllocT(c, &c->d_scratch5, static_cast<size_t>(kMatchGrid5) * M5_THREADS * SCRATCH_CPS, "d_scratch5"));
    Match5Params q;
    q.m = mp;
    q.m.scratch = c->d_scratch5;
    q.xrec = m.d_xrec;
    q.tot12 = m.d_tot12;
    q.energy = mk == 0 ? m.d_energy : nullptr;
    q.thr = Knobs().match_hits;
    const size_t m5_waves = static_cast<size_t>(kMatchGrid5) * (M5_THREADS / 64);
    if (!m.d_m5stats) HIPCHK(m.hash_tmp.AllocT(&m.d_m5stats, 2 * m5_waves, "d_m5stats"));
    HIPCHK(hipMemsetAsync(m.d_m5stats, 0, 2 * m5_waves * sizeof(unsigned long long), c->stream));
    q.wave_stats = m.d_m5stats;
    {
      // positions a wave takes at a time: larger pieces keep the lanes busier (fewer ends of a piece, where lanes
      // wait for the piece's longest walks), smaller ones the waves when there are few tiles.  100 MB, pieces of 512 /
      // 1024 / 2048 positions: T 22.4 / 20.0 / 20.4 ms, P 30.1 / 27.9 / 29.5, B 97.1 / 93.1 / 100.0
      const u64 waves = static_cast<u64>(kMatchGrid5) * (M5_THREADS / 64);
      q.sub_shift = mp.total_tiles >= 4 * waves ? 1u : 2u;
    }
    if (mk == 5 || m.skip_all) {
      hipLaunchKernelGGL(k_match5, dim3(kMatchGrid5), dim3(M5_THREADS), 0, c->stream, q);   // (no profile counts: tools/match_skip_model.c has the entries touched)
      KCHK(c, "k_match5");
      return 0;
    }
    // Some blocks each: k_match5 on the second stream beside k_match2 (which passes over k_match5's blocks) — the
    // skip-walk of a few heavy blocks is a handful of long-running waves, the rest of the device is k_match2's.
    HIPCHK(hipEventRecord(c->ev2[0], c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream2, c->ev2[0], 0));
    hipLaunchKernelGGL(k_match5, dim3(kMatchGrid5), dim3(M5_THREADS), 0, c->stream2, q);
    HIPCHK(hipGetLastError());
    c->stream2_outstanding = true;
    HIPCHK(hipEventRecord(c->ev2[1], c->stream2));
    m.join_stream2 = true;
    mp.skip_energy = m.d_energy;
    mp.skip_thr = Knobs().match_hits;
  }
  const bool filt = Knobs().match_filter;
  if (prof && filt) hipLaunchKernelGGL((k_match2<true, true>), dim3(kMatchGrid), dim3(M2_THREADS), 0, c->stream, mp);
  else if (prof) hipLaunchKernelGGL((k_match2<true, false>), dim3(kMatchGrid), dim3(M2_THREADS), 0, c->stream, mp);
  else if (filt) hipLaunchKernelGGL((k_match2<false, true>), dim3(kMatchGrid), dim3(M2_THREADS), 0, c->stream, mp);
  else hipLaunchKernelGGL((k_match2<false, false>), dim3(kMatchGrid), dim3(M2_THREADS), 0, c->stream, mp);
  if (m.join_stream2) {
    m.join_stream2 = false;
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev2[1], 0));
    c->stream2_outstanding = false;      // (whatever reuses the arrays does so in `stream`'s order, behind the kernel)
  }
  KCHK(c, "k_match2");
  return 0;
}

// Phase 5: the match records: copied from the parent where the plan says so, else computed with a pool of their own.
static int BuildMatchRecords(zmx_ctx* c, zmx_tables* t, zmx_tables* parent, int mk, u64 max_l, const ReusePlan& plan, MatchBuild& m) {
  const size_t nb = t->nb;
  const u64 pos_off = t->total_b;
  const std::vector<u32>& tile_off = t->tile_off;
  bool reuse = plan.reuse;
  if (!c->d_scratch) HIPCHK(PoolAllocT(c, &c->d_scratch, static_cast<size_t>(kMatchGrid) * M2_THREADS * SCRATCH_CPS, "d_scratch"));
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  double match_positions = 0;
  double m5_lane_iters = 0, m5_iters = 0;   // k_match5's own counts
  if (reuse) {
    // copy every record, adopt the parent's change-point pool (copied records point into it) and
    // recompute the listed tiles; on pool overflow fall through to the full build
    u64* d_src_pos = nullptr;
    u32* d_tile_list = nullptr;
    PoolScope tmp(c);
    HIPCHK(tmp.Upload(&d_src_pos, plan.src_pos.data(), nb, "d_src_pos"));
    HIPCHK(tmp.Upload(&d_tile_list, plan.tile_list.data(), plan.tile_list.size(), "d_tile_list"));
    CopyRecsParams cp;
    cp.blocks = t->d_blocks;
    cp.src_pos = d_src_pos;
    cp.src = reinterpret_cast<const uint4*>(parent->d_recs);
    cp.dst = reinterpret_cast<uint4*>(t->d_recs);
    u64 max_b = 0;
    for (size_t b = 0; b < nb; ++b) max_b = std::max<u64>(max_b, t->bsize[b]);
    const unsigned gx = static_cast<unsigned>(std::min<u64>(std::max<u64>((max_b * 2 + 256 * 16 - 1) / (256 * 16), 1), 4096));
    hipLaunchKernelGGL(k_copy_recs, dim3(gx, static_cast<unsigned>(nb)), dim3(256), 0, c->stream, cp);
    KCHK(c, "k_copy_recs");
    // the pool cursor continues where the parent's stopped
    HIPCHK(hipMemsetAsync(t->d_counters, 0, 48 * sizeof(u32), c->stream));
    HIPCHK(hipMemcpyAsync(t->d_counters, parent->d_counters, sizeof(u32), hipMemcpyDeviceToDevice, c->stream));
    if (LaunchMatch(c, t, mk, m, parent->d_pool, parent->pool_cap, static_cast<u32>(plan.tile_list.size()), d_tile_list, false) != 0) return -1;
    u32 counters[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(counters, t->d_counters, sizeof(counters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((counters[1] & 1u) == 0) {
      t->d_pool = parent->d_pool;          // ownership moves: the parent must not be used for records again
      t->pool_cap = parent->pool_cap;
      parent->d_pool = nullptr;
      parent->pool_cap = 0;
      parent->params.trace.pool = nullptr;
    } else {
      reuse = false;                       // pool overflow: build everything with a pool of our own,
      if (LaunchHash(c, t, mk, max_l, nullptr, m) != 0) return -1;   // which needs the hash arrays of whole blocks
      t->links_partial = false;
    }
  }

  // Change points beyond the 8 inline ones go to a pool; start with 4 entries per
  // position and grow on overflow (worst case 256 per position).
  // (ZOPFLI_AMD_POOL_ENTRIES: test hook, the first pool has that many entries in all, so that the
  // overflow / retry path and the fall-through from a reused parent pool run on small inputs)
  const u64 pool_entries = Knobs().pool_entries;
  u64 per_pos = 4;
  for (bool first_try = true; !reuse; first_try = false) {
    u64 cap = std::max<u64>(pos_off * per_pos, 1u << 16);
    if (first_try && pool_entries) cap = pool_entries;
    if (cap > 0xfffffff0ull) cap = 0xfffffff0ull;
    PoolFree(c, t->d_pool);
    t->d_pool = nullptr;
    HIPCHK(PoolAlloc(c, &t->d_pool, cap));
    t->pool_cap = static_cast<u32>(cap);
    HIPCHK(hipMemsetAsync(t->d_counters, 0, 48 * sizeof(u32), c->stream));
    if (LaunchMatch(c, t, mk, m, t->d_pool, t->pool_cap, tile_off[nb], nullptr, Knobs().prof) != 0) return -1;
    u32 counters[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(counters, t->d_counters, sizeof(counters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    match_positions += static_cast<double>(pos_off);
    if (m.d_m5stats) {      // (of the last attempt: the pool may grow and the kernel run again)
      const size_t m5_waves = static_cast<size_t>(kMatchGrid5) * (M5_THREADS / 64);
      std::vector<unsigned long long> ws(2 * m5_waves);
      HIPCHK(hipMemcpy(ws.data(), m.d_m5stats, ws.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      m5_lane_iters = m5_iters = 0;
      for (size_t w = 0; w < m5_waves; ++w) { m5_lane_iters += static_cast<double>(ws[2 * w]); m5_iters += static_cast<double>(ws[2 * w + 1]); }
    }
    if (counters[1] & 2u) {
      u32 dbg[8] = {0};
      HIPCHK(hipMemcpy(dbg, t->d_counters + 32, sizeof(dbg), hipMemcpyDeviceToHost));
      char buf[320];
      std::snprintf(buf, sizeof(buf), "zmx_tables_build: k_match5's wave loop did not end (state %08x xd %u curd %u bestlen %u limit %u nlink %u eqd %u "
                    "li %u idx %u same %u cur %u bestdist %u)", dbg[0], dbg[1], dbg[2], dbg[3] & 0xffffu, dbg[3] >> 16, dbg[4] & 0xffffu, dbg[4] >> 16,
                    dbg[5], dbg[6] & 0xffffu, dbg[6] >> 16, dbg[7] & 0xffffu, dbg[7] >> 16);
      return FailFault(buf);
    }
    if ((counters[1] & 1u) == 0) break;
    if (per_pos >= 256) return FailMsg("zmx_tables_build: change-point pool overflow");
    per_pos *= 8;
  }
  {
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[2]));
    float ms_hash = 0, ms_match = 0;
    HIPCHK(hipEventElapsedTime(&ms_hash, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&ms_match, c->ev[1], c->ev[2]));
    zmx_stats& ts = zamd::ThreadStats();   // (thread-local: no lock)
    ts.match[0] += ms_match * 1e-3;
    ts.match[1] += ms_hash * 1e-3;
    ts.match[2] += 1;
    ts.match[3] += reuse ? static_cast<double>(plan.tile_list.size()) * MT : match_positions;
    if (m.skip_any && !reuse) {
      ts.match5[0] += m5_lane_iters;
      ts.match5[1] += m5_iters;
      ts.match5[2] += m.skip_positions;
    }
    if (Knobs().prof && !reuse) {
      unsigned long long hc[2] = {0, 0};
      HIPCHK(hipMemcpy(hc, t->d_counters + 4, sizeof(hc), hipMemcpyDeviceToHost));
      const double pos = static_cast<double>(pos_off);
      std::fprintf(stderr, "%s: %.2f ms for %.0f positions: %.1f chain hits per "
                   "position, %.1f of 64 lanes with a hit per wave-loop iteration; %.1f SIMD cycles per hit (2.4 GHz, 1024 SIMDs)\n", mk == 5 || mk == 0 ? "k_match5 / k_match2 (hits = entries touched)" : "k_match2", ms_match, pos,
                   static_cast<double>(hc[0]) / pos, static_cast<double>(hc[0]) / static_cast<double>(hc[1] ? hc[1] : 1),
                   ms_match * 1e-3 * 2.4e9 * 1024 / static_cast<double>(hc[0] ? hc[0] : 1));
      if (mk != 5) {
        // what the runtime says of the instantiation that ships (kMatchGrid counts on 4: the window and the order's 4 KB in LDS)
        int wgs = 0;
        if (Knobs().match_filter) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, k_match2<false, true>, M2_THREADS, 0));
        else HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, k_match2<false, false>, M2_THREADS, 0));
        std::fprintf(stderr, "k_match2: %d workgroups of %u threads resident per CU; positions handed out %s\n", wgs, M2_THREADS,
                     m.d_est ? "by k_hits' estimate, longest first" : "in ascending order");
      }
    }
  }
  return 0;
}

// Phase 6: DP rows, the edges as codes and the window descriptors.  kTooLarge: come back with fewer blocks.
static int BuildDpRows(zmx_ctx* c, zmx_tables* t) {
  const size_t nb = t->nb;
  const std::vector<u32>& tile_off = t->tile_off;
  // DP row layout (k_rowscan), then the edges as weight codes (k_codes) and a buffer descriptor per row
  RowScanParams rp;
  rp.blocks = t->d_blocks;
  rp.recs = t->d_recs;
  rp.dph = t->d_dph;
  rp.block_edges = t->d_block_edges;
  // (ZOPFLI_AMD_RUN_CODES=1: codes for every row, as in round 5; the serial chain — ZOPFLI_AMD_SEG_L=0, k_dp4's pipeline
  //  over whole blocks — needs them)
  rp.codeless = !Knobs().run_codes && SegL(t->total_b) != 0 ? 1u : 0u;
  hipLaunchKernelGGL(k_rowscan, dim3(static_cast<unsigned>(nb)), dim3(1024), 0, c->stream, rp);
  KCHK(c, "k_rowscan");
  t->block_edges.resize(nb);
  HIPCHK(hipMemcpyAsync(t->block_edges.data(), t->d_block_edges, nb * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  {
    // ZOPFLI_AMD_CODE_BUDGET_MB: what the codes of one batch may take (two bytes per DP edge; a position
    // has 1..258 edges).  Beyond it the caller is told to come back with fewer blocks (kTooLarge).
    const u64 env_mb = Knobs().code_budget_mb;
    const u64 budget = (env_mb ? env_mb * (1ull << 20) : static_cast<u64>(c->code_budget)) / sizeof(u16);
    std::vector<u64> code_base(nb, 0);
    u64 cur = 0;
    for (size_t b = 0; b < nb; ++b) {
      if (t->block_edges[b] > 0xffff0000ull) return FailMsg("zmx_tables_build: block too large (DP row offsets are 32-bit)");
      code_base[b] = cur;
      cur += ((t->block_edges[b] + DP_PIECE - 1) & ~static_cast<u64>(DP_PIECE - 1)) + DP_PIECE;   // (the ring's DMA reads whole pieces)
    }
    if (cur > budget && nb > 1) {
      return FailTooLarge("zmx_tables_build: the batch needs more room for its DP edges than ZOPFLI_AMD_CODE_BUDGET_MB allows");
    }
    HIPCHK(PoolAlloc(c, &t->d_codes, cur + 2048));   // (k_dp5_spec stages whole KB: it reads a little past a window's rows)
    HIPCHK(hipMemcpyAsync(t->d_code_base, code_base.data(), nb * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    CodeParams kp;
    kp.blocks = t->d_blocks;
    kp.tile_off = t->d_tile_off;
    kp.nb_total = static_cast<u32>(nb);
    kp.recs = t->d_recs;
    kp.pool = t->d_pool;
    kp.dph = t->d_dph;
    kp.codes = t->d_codes;
    kp.code_base = t->d_code_base;
    if (tile_off[nb]) hipLaunchKernelGGL(k_codes, dim3(tile_off[nb]), dim3(256), 0, c->stream, kp);
    KCHK(c, "k_codes");
    // row lengths, first rows and flags of the 32-position windows of k_dp5_spec
    t->win_off.assign(nb + 1, 0);
    for (size_t b = 0; b < nb; ++b) t->win_off[b + 1] = t->win_off[b] + (t->bsize[b] + 31) / 32 + 1;   // (+ 1: where the block's rows end)
    HIPCHK(PoolAlloc(c, &t->d_winflag, t->win_off[nb]));
    HIPCHK(PoolAlloc(c, &t->d_winroff, t->win_off[nb]));
    HIPCHK(PoolAlloc(c, &t->d_wmeta, (static_cast<size_t>(t->win_off[nb]) + 2) * D5_WM));
    HIPCHK(PoolAlloc(c, &t->d_win_off, nb + 1));
    HIPCHK(hipMemcpyAsync(t->d_win_off, t->win_off.data(), (nb + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    MkDescParams mp;
    mp.blocks = t->d_blocks;
    mp.dph = t->d_dph;
    mp.wmeta = t->d_wmeta;
    mp.winroff = t->d_winroff;
    mp.win_off = t->d_win_off;
    mp.winflag = t->d_winflag;
    u32 max_b = 1;
    for (size_t b = 0; b < nb; ++b) max_b = std::max(max_b, t->bsize[b]);
    hipLaunchKernelGGL(k_mkdesc, dim3((max_b + 255) / 256, static_cast<unsigned>(nb)), dim3(256), 0, c->stream, mp);
    KCHK(c, "k_mkdesc");
    HIPCHK(hipStreamSynchronize(c->stream));   // (code_base is a local)
  }
  return 0;
}

// Phase 7: the chain's tasks (zmx_dp4.h): SEG_L positions each, the last one of a block takes the remainder
static int BuildChainTasks(zmx_ctx* c, zmx_tables* t) {
  const size_t nb = t->nb;
  const u32 L = SegL(t->total_b), warm = Knobs().seg_warm;
  const u32 head = std::max(SegHead(nb), L);
  t->task_off.assign(nb + 1, 0);
  t->tasks.clear();
  for (size_t b = 0; b < nb; ++b) {
    const u32 B = t->bsize[b];
    // the head [0, head), then tasks of L positions; the last one takes the remainder
    const u32 n = (L == 0 || B < head + L) ? 1u : 1u + (B - head) / L;
    for (u32 s = 0; s < n; ++s) {
      SegTask k;
      k.block = static_cast<u32>(b);
      k.pout = s == 0 ? 0u : head + (s - 1) * L;
      k.q = s == 0 ? 0u : k.pout - std::min(warm, k.pout);
      k.pend = s + 1 == n ? B + 1 : head + s * L;
      t->tasks.push_back(k);
    }
    t->task_off[b + 1] = static_cast<u32>(t->tasks.size());
  }
  const size_t nt = t->tasks.size();
  HIPCHK(PoolAlloc(c, &t->d_tasks, nt));
  HIPCHK(PoolAlloc(c, &t->d_task_off, nb + 1));
  HIPCHK(PoolAlloc(c, &t->d_lvl, nt));
  HIPCHK(PoolAlloc(c, &t->d_entry, nt));
  HIPCHK(PoolAlloc(c, &t->d_exit, nt));
  HIPCHK(PoolAlloc(c, &t->d_mid, nt));
  HIPCHK(PoolAlloc(c, &t->d_chk, nt));
  HIPCHK(PoolAlloc(c, &t->d_over, nt * SEG_OVER));
  t->redo_cap = nt;
  HIPCHK(PoolAlloc(c, &t->d_redo, 4 + nt * 4 + nt * 2));   // counters, k_dpscan's entries, its recheck list
  HIPCHK(hipMemcpyAsync(t->d_tasks, t->tasks.data(), nt * sizeof(SegTask), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(t->d_task_off, t->task_off.data(), (nb + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(t->run.stats(t->d_runout), 0, RunLayout::kStats * sizeof(u32), c->stream));
  // start the tasks at cut points of the DP where there is one close enough (zmx_dp_build.h: k_cutpoints);
  // ZOPFLI_AMD_SEG_CUTS = how far before a task's first owned position to look, 0 = every task warms up
  // (the search costs 1.1 ms per 100 MB at 1024, the configuration the whole GPU suite ran with; 512 would halve
  //  it and finds the same cut point for 99.8 % of the tasks of text)
  const u32 cut_depth = Knobs().seg_cuts;
  if (cut_depth && nt) {
    PoolScope tmp(c);
    u32* d_found = nullptr;
    u32* d_wide = nullptr;
    HIPCHK(tmp.AllocT(&d_found, 2, "d_found"));
    HIPCHK(tmp.AllocT(&d_wide, nt, "d_wide"));
    HIPCHK(hipMemsetAsync(d_found, 0, 2 * sizeof(u32), c->stream));
    HIPCHK(hipMemsetAsync(d_wide, 0, nt * sizeof(u32), c->stream));
    CutParams cp;
    cp.blocks = t->d_blocks;
    cp.dph = t->d_dph;
    cp.tasks = t->d_tasks;
    cp.depth = cut_depth;
    cp.warm = warm;
    cp.found = d_found;
    cp.wide = d_wide;
    hipLaunchKernelGGL(k_cutpoints, dim3(static_cast<unsigned>(nt)), dim3(64), 0, c->stream, cp);
    KCHK(c, "k_cutpoints");
    u32 found[2] = {0, 0};
    std::vector<u32> wide(nt);
    HIPCHK(hipMemcpyAsync(found, d_found, sizeof(found), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(wide.data(), d_wide, nt * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(t->tasks.data(), t->d_tasks, nt * sizeof(SegTask), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // merge the tasks that must not speculate (k_cutpoints) into their predecessors: the predecessor walks on to
    // the merged task's end.  (The head of a block is never merged: pout = 0.)
    size_t merged = 0;
    std::vector<SegTask> kept;
    kept.reserve(nt);
    std::vector<u32> off(nb + 1, 0);
    for (size_t b = 0; b < nb; ++b) {
      for (u32 k = t->task_off[b]; k < t->task_off[b + 1]; ++k) {
        if (k > t->task_off[b] && wide[k]) {
          kept.back().pend = t->tasks[k].pend;
          ++merged;
        } else {
          kept.push_back(t->tasks[k]);
        }
      }
      off[b + 1] = static_cast<u32>(kept.size());
    }
    t->merged_tasks = merged;
    if (merged) {
      t->tasks.swap(kept);
      t->task_off.swap(off);
      HIPCHK(hipMemcpyAsync(t->d_tasks, t->tasks.data(), t->tasks.size() * sizeof(SegTask), hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(t->d_task_off, t->task_off.data(), (nb + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (Knobs().prof) {
      std::fprintf(stderr, "k_cutpoints: %u of %zu tasks start at a cut point, %.1f positions before their first owned one on average; "
                   "%zu tasks merged into their predecessors (long-run material in the warm-up stretch), %zu tasks left\n",
                   found[0], nt, found[0] ? static_cast<double>(found[1]) / found[0] : 0.0, merged, t->tasks.size());
    }
  }
  return 0;
}

// Phase 8: the workgroup lists.
static int BuildWorkgroupLists(zmx_ctx* c, zmx_tables* t) {
  const size_t nb = t->nb;
  // k_dp5_spec's workgroups: a stretch of tasks of one block each (they share the block's weight table in
  // LDS); the workgroups that hold a head (several times the length of the other tasks) go first.  Tasks that
  // walk runs of equal bytes (k_taskkind) get workgroups of their own, listed after the others: they are run by the
  // kernel's other variant, beside the rest.
  const size_t ntk = t->tasks.size();
  std::vector<u32> kind(ntk, 0);
  if (ntk) {
    PoolScope tmp(c);
    u32* d_kind = nullptr;
    HIPCHK(tmp.AllocT(&d_kind, ntk, "d_kind"));
    TaskKindParams kp;
    kp.tasks = t->d_tasks;
    kp.blocks = t->d_blocks;
    kp.winflag = t->d_winflag;
    kp.win_off = t->d_win_off;
    kp.kind = d_kind;
    hipLaunchKernelGGL(k_taskkind, dim3(static_cast<unsigned>(ntk)), dim3(64), 0, c->stream, kp);
    KCHK(c, "k_taskkind");
    HIPCHK(hipMemcpyAsync(kind.data(), d_kind, ntk * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  // The lists: per block and kind the tasks in order, the text tasks' lists first, then the run tasks'.  A workgroup
  // takes a stretch of ZOPFLI_AMD_SEG_STRETCH consecutive entries of one list (at 4: a task a wave, as before there were
  // stretches); its descriptor is (first entry, entries).
  const u32 S = Knobs().seg_stretch;
  std::vector<u32> list[2];
  std::vector<uint2> desc[2][2];        // [kind][0: holds the block's head, 1: the others]
  for (size_t b = 0; b < nb; ++b) {
    const u32 a0 = t->task_off[b], a1 = t->task_off[b + 1];
    for (int kd = 0; kd < 2; ++kd) {
      const u32 l0 = static_cast<u32>(list[kd].size());
      for (u32 k = a0; k < a1; ++k)
        if ((kind[k] ? 1 : 0) == kd) list[kd].push_back(k);
      const u32 l1 = static_cast<u32>(list[kd].size());
      for (u32 i = l0; i < l1; i += S) {
        const bool has_head = i == l0 && list[kd][l0] == a0;
        desc[kd][has_head ? 0 : 1].push_back(make_uint2(i, std::min(S, l1 - i)));
      }
    }
  }
  // (the run tasks' list lies behind the text tasks' in one array)
  const u32 shift = static_cast<u32>(list[0].size());
  std::vector<uint2> wg;
  for (int kd = 0; kd < 2; ++kd)
    for (int rest = 0; rest < 2; ++rest)
      for (uint2 d : desc[kd][rest]) wg.push_back(make_uint2(d.x + (kd ? shift : 0u), d.y));
  t->n_wg = static_cast<u32>(desc[0][0].size() + desc[0][1].size());
  t->n_wg_runs = static_cast<u32>(desc[1][0].size() + desc[1][1].size());
  list[0].insert(list[0].end(), list[1].begin(), list[1].end());
  HIPCHK(PoolAlloc(c, &t->d_wg_tasks, list[0].size() + 4));
  HIPCHK(PoolAlloc(c, &t->d_wg_desc, wg.size() + 1));
  if (!wg.empty()) {
    HIPCHK(hipMemcpyAsync(t->d_wg_tasks, list[0].data(), list[0].size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(t->d_wg_desc, wg.data(), wg.size() * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));   // `list` and `wg` are locals
  return 0;
}

// Phase 9: trace segments (zmx_trace.h)
static int BuildTraceSegments(zmx_ctx* c, zmx_tables* t) {
  const size_t nb = t->nb;
  t->seg_off.assign(nb + 1, 0);
  for (size_t b = 0; b < nb; ++b) t->seg_off[b + 1] = t->seg_off[b] + (t->bsize[b] + TS_SEG - 1) / TS_SEG;
  HIPCHK(PoolAlloc(c, &t->d_seg_off, nb + 1));
  HIPCHK(PoolAlloc(c, &t->d_extab, static_cast<size_t>(t->seg_off[nb]) * GS_STATES));   // shared by the trace (TS_ENT per segment)
  HIPCHK(PoolAlloc(c, &t->d_seginfo, t->seg_off[nb]));
  HIPCHK(hipMemcpyAsync(t->d_seg_off, t->seg_off.data(), (nb + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// Last: the kernels' parameter blocks, as far as they depend on the table set alone (TableParams).  No array of the set
// moves after this (but its pool may go to a set built from it: BuildMatchRecords).
static void FillTableParams(zmx_tables* t, bool with_dp) {
  const u32 nb = static_cast<u32>(t->nb);
  GreedySegParams& gp = t->params.greedy;
  gp.blocks = t->d_blocks;
  gp.seg_off = t->d_seg_off;
  gp.nb = nb;
  gp.recs = t->d_recs;
  gp.hist_out = t->run.hist(t->d_runout);
  gp.nsym_out = t->run.nsym(t->d_runout);
  gp.extab = t->d_extab;
  gp.seginfo = t->d_seginfo;
  if (!with_dp) return;
  const RunLayout& run = t->run;
  WtabParams& wp = t->params.wtab;
  wp.cost = run.cost(t->d_runin);
  wp.mincost = run.mincost(t->d_runin);
  wp.wtab = t->d_wtab;
  wp.badcodes = t->d_badcodes;
  wp.stats = t->run.stats(t->d_runout);
  BadScanParams& bp = t->params.badscan;
  bp.blocks = t->d_blocks;
  bp.tile_off = t->d_tile_off;
  bp.nb_total = nb;
  bp.dph = t->d_dph;
  bp.codes = t->d_codes;
  bp.code_base = t->d_code_base;
  bp.badcodes = t->d_badcodes;
  bp.badpos = t->d_badpos;
  Dp4Params& cp = t->params.dp;      // (block0, task0, redo_pass = 0, est_bits, prof, mid = null: per run)
  cp.blocks = t->d_blocks;
  cp.dph = t->d_dph;
  cp.cost = wp.cost;
  cp.mincost = wp.mincost;
  cp.codes = t->d_codes;
  cp.code_base = t->d_code_base;
  cp.block_edges = t->d_block_edges;
  cp.wtab = t->d_wtab;
  cp.la = t->d_la;
  cp.badpos = t->d_badpos;
  cp.tasks = t->d_tasks;
  cp.task_off = t->d_task_off;
  cp.lvl = t->d_lvl;
  cp.entry = t->d_entry;
  cp.exit = t->d_exit;
  cp.chk = t->d_chk;
  cp.over = t->d_over;
  cp.wmax = run.wmax(t->d_runin);
  cp.tiemask = run.tiemask(t->d_runin);
  cp.stats = t->run.stats(t->d_runout);
  cp.wg_tasks = t->d_wg_tasks;
  cp.redo_count = t->d_redo;
  cp.redo_wg = t->d_redo + 4;
  cp.recheck = t->d_redo + 4 + t->redo_cap * 4;
  cp.redo_parity = 0;
  cp.wg_desc = t->d_wg_desc;
  cp.flags = t->run.flags(t->d_runout);
  cp.wmeta = t->d_wmeta;
  cp.winroff = t->d_winroff;
  cp.winflag = t->d_winflag;
  cp.win_off = t->d_win_off;
  TraceSegParams& tp = t->params.trace;      // (block0, seg0 = 0)
  tp.blocks = t->d_blocks;
  tp.seg_off = t->d_seg_off;
  tp.nb_total = nb;
  tp.recs = t->d_recs;
  tp.pool = t->d_pool;
  tp.la = t->d_la;
  tp.slot = t->run.slot(t->d_runin);
  tp.store0 = t->d_store[0];
  tp.store1 = t->d_store[1];
  tp.hist_out = t->run.hist(t->d_runout);
  tp.nsym_out = t->run.nsym(t->d_runout);
  tp.flags = t->run.flags(t->d_runout);
  tp.extab = t->d_extab;
  tp.seginfo = t->d_seginfo;
}

static int BuildTables(zmx_ctx* c, const zmx_block* blocks, size_t nb, zmx_tables* t, zmx_tables* parent, bool with_dp) {
  const int mk = MatchKernel();   // (one choice per build: zmx_set_match_kernel may be called meanwhile)
  t->matches_only = !with_dp;
  u64 la_off = 0, max_l = 0;
  if (const int rc = LayoutBlocks(c, blocks, nb, t, &la_off, &max_l)) return rc;
  if (nb == 0) return 0;
  std::vector<uint64_t> tail_r;
  if (parent != nullptr && c->h_in == nullptr) {
    if (const int rc = TailRuns(c, t, &tail_r)) return rc;
  }
  const ReusePlan plan = PlanReuse(c, t, parent, tail_r);
  if (const int rc = AllocTableArrays(c, t, la_off)) return rc;
  MatchBuild m(c);
  if (const int rc = BuildHashLinks(c, t, mk, max_l, plan, m)) return rc;
  if (const int rc = BuildMatchRecords(c, t, parent, mk, max_l, plan, m)) return rc;
  // (zmx_tables_build_matches: the greedy pass over master blocks that will be split wants the matches only; the codes
  //  of its DP edges — two bytes for each of up to 258 edges a position, 52 GB for 100 MB of long runs — would be
  //  written, never read, and held while the tables of the split blocks allocate their own)
  if (with_dp) {
    if (const int rc = BuildDpRows(c, t)) return rc;
    if (const int rc = BuildChainTasks(c, t)) return rc;
    if (const int rc = BuildWorkgroupLists(c, t)) return rc;
  }
  if (const int rc = BuildTraceSegments(c, t)) return rc;
  FillTableParams(t, with_dp);
  return 0;
}

int zmx_tables_build(zmx_ctx* c, const zmx_block* blocks, size_t nblocks, zmx_tables** out) {
  return zmx_tables_build_from(c, nullptr, blocks, nblocks, out);
}

// A new table set over `blocks`: 0, -1 with the error set, or kTooLarge.
static int BuildTablesEntry(zmx_ctx* c, zmx_tables* parent, const zmx_block* blocks, size_t nblocks, bool with_dp, zmx_tables** out) {
  DEVICE_ENTRY(c->device);
  zmx_tables* t = new zmx_tables();
  g_last_oom = false;
  const int rc = BuildTables(c, blocks, nblocks, t, parent, with_dp);
  if (rc) {
    zmx_tables_free(c, t);
    // out of device memory (other contexts of the device hold theirs): the caller may come back with fewer blocks,
    // as for a batch beyond the code budget
    return rc == -1 && g_last_oom && nblocks > 1 ? kTooLarge : rc;
  }
  *out = t;
  return 0;
}

int zmx_tables_build_matches(zmx_ctx* c, const zmx_block* blocks, size_t nblocks, zmx_tables** out) {
  return BuildTablesEntry(c, nullptr, blocks, nblocks, false, out);
}

// `parent` (optional): a table set over blocks that contain the new ones.  The match record of a
// position depends on its block only through the block end: limit = min(258, end -
// pos), same[] truncated at the end, zero bytes in the hashes of the last two positions.  So the
// records of a sub-block equal the parent's except where pos + 258 > end or pos lies in the run
// of equal bytes that reaches the end — only the tiles holding such positions are recomputed,
// everything else is copied.  Hash links (k_same, k_chain) are rebuilt: they are cheap.
int zmx_tables_build_from(zmx_ctx* c, zmx_tables* parent, const zmx_block* blocks, size_t nblocks, zmx_tables** out) {
  if (parent != nullptr && CheckTables("zmx_tables_build_from", parent, zamd::kUntrimmed) != 0) return -1;
  return BuildTablesEntry(c, parent, blocks, nblocks, true, out);
}
}  // extern "C"
