// Driver part: a table set — RunLayout, TableParams, zmx_tables, release / free / trim — and the adapters of host/entry_checks.h
// that every later entry calls.  Built by drv_build.h.  Needs drv_errors.h and drv_context.h (PoolFree, PinnedGive).
#pragma once

// What a squeeze run takes and gives, each side ONE array on the device and one pinned mirror on the host, so that a run
// has one copy down and one up (eight small copies a run were 3 ms of copy kernels per 15 runs).  This is the only place
// that says where the parts lie: in = cost | mincost | wmax | tiemask | est | slot, out = hist | nsym | stats | flags.
// The accessors take the base of either copy, the device's or the pinned one.
struct RunLayout {
  static constexpr size_t kStats = ZMX_SEG_N, kFlags = 4;   // words: the task statistics (zmx_seg_stat, the device's reading; k_wtab zeroes them), the consistency flags
  size_t in_cost = 0, in_mincost = 0, in_wmax = 0, in_tiemask = 0, in_est = 0, in_slot = 0, in_bytes = 0;
  size_t out_hist = 0, out_nsym = 0, out_stats = 0, out_flags = 0, out_bytes = 0;
  RunLayout() = default;
  explicit RunLayout(size_t nb) {
    in_mincost = in_cost + nb * ZMX_HIST * sizeof(double);
    in_wmax = in_mincost + nb * sizeof(double);
    in_tiemask = in_wmax + nb * sizeof(float);
    in_est = in_tiemask + nb * sizeof(u32);
    in_slot = in_est + nb * sizeof(float);
    in_bytes = in_slot + nb * sizeof(int);
    out_nsym = out_hist + nb * ZMX_HIST * sizeof(u32);
    out_stats = out_nsym + nb * sizeof(u32);
    out_flags = out_stats + kStats * sizeof(u32);
    out_bytes = out_flags + kFlags * sizeof(u32);
  }
  double* cost(unsigned char* in) const { return reinterpret_cast<double*>(in + in_cost); }         // [nb][ZMX_HIST]
  double* mincost(unsigned char* in) const { return reinterpret_cast<double*>(in + in_mincost); }   // [nb]
  float* wmax(unsigned char* in) const { return reinterpret_cast<float*>(in + in_wmax); }           // [nb] (RunInfo)
  u32* tiemask(unsigned char* in) const { return reinterpret_cast<u32*>(in + in_tiemask); }         // [nb]
  float* est(unsigned char* in) const { return reinterpret_cast<float*>(in + in_est); }             // [nb] estimated block cost
  int* slot(unsigned char* in) const { return reinterpret_cast<int*>(in + in_slot); }               // [nb]
  u32* hist(unsigned char* out) const { return reinterpret_cast<u32*>(out + out_hist); }            // [nb][ZMX_HIST]
  u32* nsym(unsigned char* out) const { return reinterpret_cast<u32*>(out + out_nsym); }            // [nb]
  u32* stats(unsigned char* out) const { return reinterpret_cast<u32*>(out + out_stats); }          // [kStats]
  u32* flags(unsigned char* out) const { return reinterpret_cast<u32*>(out + out_flags); }          // [kFlags]
  // the statistics and the flags behind them, as one range (out_flags = out_stats + stats_bytes above)
  static constexpr size_t stats_and_flags_bytes() { return (kStats + kFlags) * sizeof(u32); }
};

// The kernel parameters that depend on the table set alone, filled when the set is built (FillTableParams).  A launch
// copies its block and sets what varies per run.  Zeroed again when the arrays go (ReleaseTableArrays).
struct TableParams {
  GreedySegParams greedy;   // .store: per call
  WtabParams wtab;          // (these four: sets with DP rows only)
  BadScanParams badscan;
  Dp4Params dp;             // per run: est_bits, prof, mid, task0, redo_pass and the switches' fields
  TraceSegParams trace;
};

struct zmx_tables {
  size_t nb = 0;
  std::vector<BlockDesc> blocks;
  std::vector<u32> bsize;
  std::vector<u32> store_begin[2];  // first valid entry of each block's store slot
  size_t total_b = 0, total_l = 0;
  BlockDesc* d_blocks = nullptr;
  u32* d_tile_off = nullptr;
  u16* d_same16 = nullptr;
  ushort4* d_links = nullptr;
  bool links_partial = false;     // built from a parent: the hash arrays exist only where the match kernel read them
  size_t merged_tasks = 0;        // tasks merged into their predecessors (BuildTables): the set has long tasks
  bool matches_only = false;      // built by zmx_tables_build_matches: no DP rows, codes, windows or tasks
  bool trimmed = false;           // zmx_tables_trim: only the stores are left
  u32* d_recs = nullptr;
  u32* d_pool = nullptr;
  u32 pool_cap = 0;
  u16* d_la = nullptr;
  u32* d_store[2] = {nullptr, nullptr};
  uint2* d_dph = nullptr;         // per position: DP row offset, kend | shortcut flag (k_rowscan)
  u64* d_block_edges = nullptr;   // per block: DP edges
  u32* d_badpos = nullptr;        // bit per position: it owns a match edge below mincost (k_badscan, per run)
  size_t badpos_words = 0;
  bool badpos_clean = false;      // the bitmap is all zero (no run since the last memset has marked a position)
  u64* d_code_base = nullptr;     // per block: first slot in d_codes
  u16* d_codes = nullptr;         // the DP edges as weight codes (k_codes)
  double* d_wtab = nullptr;       // [nb][ZMX_WTAB] the weights of the current run (k_wtab)
  u32* d_badcodes = nullptr;      // [nb][40] the weights below mincost (k_wtab)
  u32* d_seg_off = nullptr;       // per block: first trace segment (cumulative)
  u32* d_extab = nullptr;         // per trace segment: exit table (k_trace_exits)
  uint2* d_seginfo = nullptr;     // per trace segment: entry, symbol offset (k_trace_link)
  std::vector<u32> seg_off;
  std::vector<u64> block_edges;
  std::vector<u32> tile_off;
  u32* d_counters = nullptr;  // 48 words, see MatchParams (24 .. 31: k_match5's tile cursors, 32 .. 39: its watchdog's dump)
  // a squeeze run's input and output, on the device and mirrored in pinned memory, laid out by `run`
  RunLayout run;
  unsigned char* d_runin = nullptr;
  unsigned char* d_runout = nullptr;
  unsigned char* h_runin = nullptr;
  unsigned char* h_runout = nullptr;
  size_t h_runin_cap = 0, h_runout_cap = 0;
  TableParams params = {};
  u64* d_prof = nullptr;      // nb * ZMX_PROF_N counters when ZOPFLI_AMD_PROF is set
  // the chain's tasks (zmx_dp4.h)
  std::vector<SegTask> tasks;
  std::vector<u32> task_off;  // [nb + 1]
  SegTask* d_tasks = nullptr;
  u32* d_task_off = nullptr;
  u32* d_wg_tasks = nullptr;       // the blocks' task lists per kind, and ...
  uint2* d_wg_desc = nullptr;      // ... k_dp5_spec's workgroups: a stretch (first entry, entries) of one list each
  u32 n_wg = 0;
  u32 n_wg_runs = 0;               // ... of which the last n_wg_runs hold run tasks (k_taskkind): k_dp5_spec<.., true>
  u32* d_wmeta = nullptr;          // per 32-position window: 40 words, what k_dp5_spec needs to fetch its rows (k_mkdesc)
  u32* d_winroff = nullptr;        // per 32-position window: offset of its first row in the block's codes (k_mkdesc)
  u32* d_winflag = nullptr;        // per 32-position window: fast path possible (k_mkdesc)
  u32* d_win_off = nullptr;        // [nb]
  std::vector<u32> win_off;
  float* d_lvl = nullptr;
  SegSnap* d_entry = nullptr;
  SegSnap* d_exit = nullptr;
  SegSnap* d_mid = nullptr;      // per task: the state where it first came near the end of its binade (zmx_dp5.h)
  SegCheck* d_chk = nullptr;
  u16* d_over = nullptr;      // [tasks][SEG_OVER]
  u32* d_redo = nullptr;      // [3 counters + 1 pad + redo_cap * 4 + redo_cap * 2]: k_dpscan's entries of tasks to run a second time, its recheck list
  size_t redo_cap = 0;        // the tasks d_redo was sized for (before any were merged)
  std::vector<u32> h_hist;    // the histograms of the last greedy parse / squeeze run (host copy)
  bool have_hist = false;
  u32 squeeze_runs = 0;
  // host cache for the parity probe
  std::vector<std::vector<u32>> probe_recs;
  std::vector<u32> probe_pool;
  bool probe_pool_ready = false;
};

extern "C" {
// Gives back the device arrays of a table set — all of them, or all but the two LZ77 stores (zmx_tables_trim).
static void ReleaseTableArrays(zmx_ctx* c, zmx_tables* t, bool keep_stores) {
  auto rel = [&](auto*&... p) { ((PoolFree(c, p), p = nullptr), ...); };
  rel(t->d_blocks, t->d_tile_off, t->d_same16, t->d_links, t->d_recs, t->d_pool, t->d_la, t->d_dph, t->d_block_edges);
  rel(t->d_badpos, t->d_code_base, t->d_codes, t->d_wtab, t->d_badcodes, t->d_seg_off, t->d_extab, t->d_seginfo);
  rel(t->d_counters, t->d_prof, t->d_tasks, t->d_task_off, t->d_wg_tasks, t->d_wmeta, t->d_runin, t->d_runout);
  rel(t->d_winroff, t->d_winflag, t->d_win_off, t->d_lvl, t->d_entry, t->d_exit, t->d_mid, t->d_chk, t->d_over, t->d_redo, t->d_wg_desc);
  PinnedGive(c, &t->h_runin, t->h_runin_cap);
  PinnedGive(c, &t->h_runout, t->h_runout_cap);
  // nothing that pointed into those arrays stays behind (the entries refuse such tables: CheckTables)
  t->params = TableParams{};
  if (!keep_stores) rel(t->d_store[0], t->d_store[1]);
}

void zmx_tables_free(zmx_ctx* c, zmx_tables* t) {
  if (!t) return;
  DeviceGuard dev_guard(c ? c->device : 0);
  // (an error return between a launch on the second stream and its join leaves that kernel in flight: nothing of
  //  this table set may go back to the pool under it)
  if (c && c->stream2) (void)hipStreamSynchronize(c->stream2);
  ReleaseTableArrays(c, t, false);
  delete t;
}

// What zmx_encode_blocks and zmx_store_download read of a table set are its two stores (and the host's notes on where
// each block's symbols lie): everything else — 32 bytes of match record per position, the DP codes, window records, the
// chain's snapshots — can go once the parses are final.  deflate.cc trims the tables of the optimal batch before it
// builds the tables of the fixed-tree re-parses: on incompressible or short input, where most blocks ask for one, the
// peak otherwise doubles.
int zmx_tables_trim(zmx_ctx* c, zmx_tables* t) {
  if (!t) return 0;
  DEVICE_ENTRY(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));      // (nothing of this table set may still be in flight)
  HIPCHK(hipStreamSynchronize(c->stream2));
  ReleaseTableArrays(c, t, true);
  t->trimmed = true;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// What the entries check of their arguments before they touch anything.  `who` is the entry's name: the messages
// start with it.  The rules and their texts are host/entry_checks.h's; here they meet the tables.
// ---------------------------------------------------------------------------------------------
static int Refused(const std::string& refusal) { return refusal.empty() ? 0 : FailMsg(refusal); }
static int CheckTables(const char* who, const zmx_tables* t, zamd::TableNeeds needs) {
  return Refused(zamd::CheckTables(who, t != nullptr, t && t->trimmed, t && t->matches_only, needs));
}
static int CheckBlock(const char* who, const zmx_tables* t, size_t block) {
  return Refused(zamd::CheckBlock(who, t->nb, block));
}
// symbols [0, nsym) of the store in `slot` of `block`
static int CheckStoreRef(const char* who, const zmx_tables* t, size_t block, int slot, size_t nsym) {
  return Refused(zamd::CheckStoreRef(who, t->nb, block, slot, nsym,
                                     [&] { return static_cast<size_t>(t->bsize[block] - t->store_begin[slot][block]); }));
}
}  // extern "C"
