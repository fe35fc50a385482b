// Driver part: the parses — zmx_lz77_greedy, RunInfo, ReportSqueezeProf, TraceAndCollect, LaunchSpec, LaunchFix, zmx_squeeze_run,
// zmx_trace_length_arrays.  Needs drv_context.h (KernelTiming, PoolAlloc) and drv_tables.h (zmx_tables, RunLayout, the checks).
#pragma once

extern "C" {
int zmx_lz77_greedy(zmx_ctx* c, zmx_tables* t, int slot, uint32_t* nsym, uint32_t* hist) {
  if (const int rc = CheckTables("zmx_lz77_greedy", t, zamd::kUntrimmed)) return rc;
  if (t->nb == 0) return 0;
  if (slot != 0 && slot != 1) return FailMsg("zmx_lz77_greedy: slot must be 0 or 1");
  DEVICE_ENTRY(c->device);
  GreedySegParams gp = t->params.greedy;
  gp.store = t->d_store[slot];
  const unsigned nseg = t->seg_off[t->nb];
  if (nseg) hipLaunchKernelGGL(k_greedy_exits, dim3(nseg), dim3(GS_THREADS), 0, c->stream, gp);
  KCHK(c, "k_greedy_exits");
  hipLaunchKernelGGL(k_greedy_link, dim3(static_cast<unsigned>(t->nb)), dim3(64), 0, c->stream, gp);
  KCHK(c, "k_greedy_link");
  if (nseg) hipLaunchKernelGGL(k_greedy_emit, dim3(nseg), dim3(64), 0, c->stream, gp);
  KCHK(c, "k_greedy_emit");
  HIPCHK(hipMemcpyAsync(nsym, t->run.nsym(t->d_runout), t->nb * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hist, t->run.hist(t->d_runout), t->nb * ZMX_HIST * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < t->nb; ++b) t->store_begin[slot][b] = 0;
  t->h_hist.assign(hist, hist + t->nb * ZMX_HIST);
  t->have_hist = true;
  return 0;
}

// What the acceptance test of the chain's tasks (zmx_dp4.h) needs to know about a run's cost model:
// an upper bound of every edge weight, the binades in which a weight can tie in the float rounding,
// and a first guess of the block's cost.  The weights are the 256 literal costs and
// ((lbits + dbits) + ll[lsym]) + d[dsym] for the 29 x 30 symbol pairs (squeeze.c:155).
static void RunInfo(const double* cost, const u32* hist, u32 B, float* wmax_out, u32* tiemask_out, float* est_out,
                    double mincost = 0.0, bool* below_mincost = nullptr) {
  const double* ll = cost;
  const double* d = cost + ZMX_NUM_LL;
  auto lbits = [](int s) { return s < 265 || s == 285 ? 0 : (s - 261) / 4; };
  auto dbits = [](int s) { return s < 4 ? 0 : s / 2 - 1; };
  double w[256 + 29 * 30];
  int n = 0;
  for (int i = 0; i < 256; ++i) w[n++] = ll[i];
  for (int ls = 257; ls <= 285; ++ls)
    for (int ds = 0; ds < 30; ++ds) w[n++] = (static_cast<double>(lbits(ls) + dbits(ds)) + ll[ls]) + d[ds];
  double wmax = 0;
  for (int i = 0; i < n; ++i) wmax = std::max(wmax, w[i]);
  // a match weight below mincost (possible only through rounding in the cost model): k_wtab finds the same ones with
  // the same arithmetic, and only then do k_badscan and its bitmap have anything to do (zmx_squeeze_run)
  if (below_mincost) {
    bool any = false;
    for (int i = 256; i < n; ++i) any |= w[i] < mincost;
    *below_mincost = any;
  }
  // dbl(w + c) = c + RNE(w / 2^(e-52)) 2^(e-52) for a float c of binade e; the float rounding of that
  // sum ties iff the remainder modulo the float ulp 2^(e-23) is exactly half of it, i.e. iff
  // r = RNE(w 2^(52-e)) has r mod 2^29 = 2^28.  Integer arithmetic on the mantissa: w = m 2^x.
  u32 mask = 0;
  for (int i = 0; i < n; ++i) {
    if (!(w[i] > 0)) continue;                       // (0 shifts nothing)
    int x;
    const double fr = std::frexp(w[i], &x);          // w = fr 2^x, 0.5 <= fr < 1
    const uint64_t m = static_cast<uint64_t>(std::ldexp(fr, 53));   // 53-bit integer, exact
    x -= 53;                                         // w = m 2^x
    {
      // r mod 2^29 = 2^28 needs 28 equal bits in a row somewhere in m — zeros, or ones that a rounding carry
      // turns into zeros, or nothing but zeros below the leading bit (shifts past the mantissa's end).  Entropy
      // costs are log2 values with random mantissas: this test, not the loop over the binades, is what they cost
      // (the loop was 0.25 ms per block and run, a quarter of what the host spent between two runs).
      auto run27 = [](uint64_t y) {                  // 27 ones in a row in y?
        uint64_t a = y & (y >> 1);
        a &= a >> 2; a &= a >> 4; a &= a >> 8;       // 16 in a row
        return (a & (a >> 11)) != 0;
      };
      const uint64_t mask53 = (1ull << 53) - 1;
      if (!run27(~m & mask53) && !run27(m) && (m & ((1ull << 26) - 1)) != 0) continue;
    }
    for (int e = 4; e < 32; ++e) {
      const int sh = -(x + 52 - e);                  // r = RNE(m / 2^sh)
      uint64_t r;
      if (sh <= 0) {
        if (-sh >= 29) continue;                     // r is a multiple of 2^29
        r = m << -sh;
      } else if (sh >= 64) {
        continue;                                    // r = 0
      } else {
        const uint64_t q = m >> sh, rem = m & ((1ull << sh) - 1), half = 1ull << (sh - 1);
        r = q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0);
      }
      if ((r & 0x1fffffffull) == 0x10000000ull) mask |= 1u << e;
    }
  }
  *wmax_out = static_cast<float>(wmax) + 1.0f;
  *tiemask_out = mask;
  // no parse to go by (the fixed-tree re-parse, deflate.c:770-781, which is tried on blocks that
  // compress badly): close to 8 bits per byte; the run refines the tasks' levels itself
  double est = 8.0 * B;
  if (hist) {
    est = 0;
    for (int i = 0; i < ZMX_NUM_LL; ++i) est += hist[i] * (ll[i] + (i > 256 ? lbits(i) : 0));
    for (int i = 0; i < 30; ++i) est += hist[ZMX_NUM_LL + i] * (d[i] + dbits(i));
  }
  *est_out = static_cast<float>(est);
}

// Test hook (tests/test_cpu_abi.py): the acceptance facts of one cost model, no device involved.
void zmx_internal_run_info(const double* cost320, float* wmax, uint32_t* tiemask) {
  float est;
  RunInfo(cost320, nullptr, 0, wmax, tiemask, &est);
}

// ZOPFLI_AMD_PROF: what the counters of the run that just ended say (t->d_prof), on stderr.
static int ReportSqueezeProf(zmx_tables* t, const double* ksec, const u32* segstats) {
  const size_t nb = t->nb;
  std::vector<u64> pr(nb * ZMX_PROF_N);
  HIPCHK(hipMemcpy(pr.data(), t->d_prof, pr.size() * sizeof(u64), hipMemcpyDeviceToHost));
  double a[ZMX_PROF_N] = {};
  for (size_t b = 0; b < nb; ++b)
    for (unsigned k = 0; k < ZMX_PROF_N; ++k) a[k] += static_cast<double>(pr[b * ZMX_PROF_N + k]);
  std::fprintf(stderr, "squeeze prof: edges %.2f ms chain %.2f ms trace %.2f ms; chain wave busy %.1f cycles/position, "
               "%.0f steps, fast %.1f%% of %.0f positions walked (%zu in the blocks); tasks %u accepted %u re-run "
               "state %u values %u level %u tie %u (%u positions, %u by the lean job)\n",
               ksec[0] * 1e3, ksec[1] * 1e3, ksec[2] * 1e3, a[PF_TASK_CYC] / a[PF_POS], a[PF_STEPS],
               100.0 * a[PF_FAST] / (a[PF_FAST] + a[PF_SLOW] + 1e-9), a[PF_POS], t->total_b, segstats[ZMX_SEG_TASKS], segstats[ZMX_SEG_ACCEPTED], segstats[ZMX_SEG_RERUN_STATE],
               segstats[ZMX_SEG_RERUN_VALUES], segstats[ZMX_SEG_RERUN_LEVEL], segstats[ZMX_SEG_RERUN_TIE], segstats[ZMX_SEG_POSITIONS_RERUN], segstats[ZMX_SEG_DEV_LEAN]);
  {
    double mx = 0, hd = 0;
    for (size_t b = 0; b < nb; ++b) { mx = std::max(mx, static_cast<double>(pr[b * ZMX_PROF_N + PF_D5_LONGEST])); hd = std::max(hd, static_cast<double>(pr[b * ZMX_PROF_N + PF_D5_HEAD])); }
    std::fprintf(stderr, "  k_dp5_spec: longest task %.0f cycles, longest head task %.0f cycles; %.1f%% of the positions walked by the integer step (cycles per position there: fetch issue %.1f, fetch wait %.1f, gather + chain %.1f)\n", mx, hd, 100.0 * a[PF_D5_INT_POS] / (a[PF_POS] + 1e-9), a[PF_D5_INT_CYC] / (a[PF_D5_INT_POS] + 1e-9), a[PF_D5_INT_CYC + 1] / (a[PF_D5_INT_POS] + 1e-9), a[PF_D5_INT_CYC + 2] / (a[PF_D5_INT_POS] + 1e-9));
  }
  // the fixed cost around the tasks, by every pass of k_dp5_spec and k_dp5_stretch (what a counter means: ZmxProf, zmx_kernels.h)
  if (a[PF_SETUP_WAVES] > 0 && a[PF_ALIVE_CYC] > 0) {
    std::fprintf(stderr, "  k_dp5_spec fixed cost: set-up %.0f cycles a wave (%.0f waves with a task), %.2f%% of the workgroups' wave cycles; finished waves waiting for their workgroup %.2f%%; in tasks %.2f%%\n",
                 a[PF_SETUP_CYC] / a[PF_SETUP_WAVES], a[PF_SETUP_WAVES], 100.0 * a[PF_SETUP_CYC] / a[PF_ALIVE_CYC], 100.0 * a[PF_IDLE_CYC] / a[PF_ALIVE_CYC], 100.0 * a[PF_TASK_CYC] / a[PF_ALIVE_CYC]);
  }
  std::fprintf(stderr, "  redo list: %.0f tasks in %.0f entries\n", a[PF_REDO_TASKS], a[PF_REDO_ENTRIES]);
  std::fprintf(stderr, "  k_dp5_spec integer windows, cycles per position: class decision %.1f, waiting for the prefetched record and codes %.1f, prefetch issue %.1f\n",
               a[PF_D5_INTWIN] / (a[PF_D5_INT_POS] + 1e-9), a[PF_D5_INTWIN + 1] / (a[PF_D5_INT_POS] + 1e-9), a[PF_D5_INTWIN + 2] / (a[PF_D5_INT_POS] + 1e-9));
  std::fprintf(stderr, "  k_dp5_spec windows: integer %.1f%% of positions at %.0f cycles each, class 1 in doubles %.1f%% at %.0f, class 2 %.1f%% at %.0f, generic %.1f%% at %.0f\n",
               100.0 * a[PF_D5_CLASS_POS] / (a[PF_POS] + 1e-9), a[PF_D5_CLASS_CYC] / (a[PF_D5_CLASS_POS] + 1e-9), 100.0 * a[PF_D5_CLASS_POS + 1] / (a[PF_POS] + 1e-9), a[PF_D5_CLASS_CYC + 1] / (a[PF_D5_CLASS_POS + 1] + 1e-9),
               100.0 * a[PF_D5_CLASS_POS + 2] / (a[PF_POS] + 1e-9), a[PF_D5_CLASS_CYC + 2] / (a[PF_D5_CLASS_POS + 2] + 1e-9), 100.0 * a[PF_D5_CLASS_POS + 3] / (a[PF_POS] + 1e-9), a[PF_D5_CLASS_CYC + 3] / (a[PF_D5_CLASS_POS + 3] + 1e-9));
  std::fprintf(stderr, "  k_dp5_spec generic windows, cycles each: shortcut %.0f (%.0f of them), run row integer %.0f (%.0f), run row doubles %.0f (%.0f), other row %.0f (%.0f), window header %.0f (%.0f)\n",
               a[PF_D5_GEN] / (a[PF_D5_GEN + 1] + 1e-9), a[PF_D5_GEN + 1], a[PF_D5_GEN + 2] / (a[PF_D5_GEN + 3] + 1e-9), a[PF_D5_GEN + 3], a[PF_D5_GEN + 4] / (a[PF_D5_GEN + 5] + 1e-9), a[PF_D5_GEN + 5], a[PF_D5_GEN + 6] / (a[PF_D5_GEN + 7] + 1e-9), a[PF_D5_GEN + 7], a[PF_D5_GEN + 8] / (a[PF_D5_GEN + 9] + 1e-9), a[PF_D5_GEN + 9]);
  std::fprintf(stderr, "  k_dp5_spec positions: run interior %.0f in unrolled windows, %.0f in loops with room, %.0f with checks; general step: %.0f run rows, %.0f other rows; class 2: %.0f rows that reach register 2\n",
               a[PF_D5_GEN_POS], a[PF_D5_GEN_POS + 1], a[PF_D5_GEN_POS + 2], a[PF_D5_GEN_POS + 3], a[PF_D5_GEN_POS + 4], a[PF_D5_GEN_POS + 5]);
  {
    const double gen = a[PF_D5_GEN_CYC + 3] - a[PF_D5_GEN_CYC + 1] - a[PF_D5_GEN_CYC + 2] - a[PF_D5_OTHER_CYC];     // (the loop over a window's positions, less its stretches)
    std::fprintf(stderr, "  k_dp5_spec generic windows, cycles: headers %.3g, run stretches: whole windows %.3g (%.0f per position), others %.3g (%.0f); stretches of other rows %.3g (%.0f); the general step %.3g (%.0f per position incl. shortcuts)\n",
                 a[PF_D5_GEN_CYC], a[PF_D5_GEN_CYC + 1], a[PF_D5_GEN_CYC + 1] / (a[PF_D5_GEN_POS] + 1e-9), a[PF_D5_GEN_CYC + 2], a[PF_D5_GEN_CYC + 2] / (a[PF_D5_GEN_POS + 1] + a[PF_D5_GEN_POS + 2] + 1e-9), a[PF_D5_OTHER_CYC], a[PF_D5_OTHER_CYC] / (a[PF_D5_OTHER_POS] + 1e-9), gen, gen / (a[PF_D5_GEN_POS + 3] + a[PF_D5_GEN_POS + 4] + a[PF_D5_GEN + 1] + 1e-9));
  }
  const char* nm[5] = {"32", "16", "8", "8 (two registers)", "generic"};
  for (int i = 0; i < 5; ++i)
    std::fprintf(stderr, "  path %-18s %5.1f%% of positions, %6.1f cycles/position\n", nm[i], 100.0 * a[PF_D4_PATH + 1 + 2 * i] / a[PF_POS],
                 a[PF_D4_PATH + 2 * i] / (a[PF_D4_PATH + 1 + 2 * i] + 1e-9));
  const u32 wave_base[2] = {PF_D4_WAVE1, PF_D4_WAVE2};
  for (int w = 0; w < 2; ++w)
    std::fprintf(stderr, "  producer wave %d, cycles/step: walk %.0f ring %.0f tiles %.0f barrier %.0f\n", w + 1,
                 a[wave_base[w]] / a[PF_STEPS], a[wave_base[w] + 1] / a[PF_STEPS], a[wave_base[w] + 2] / a[PF_STEPS], a[wave_base[w] + 3] / a[PF_STEPS]);
  return 0;
}

// The tail of a squeeze run, shared with zmx_trace_length_arrays: TraceBackwards + FollowPath (squeeze.c:317, :338) over
// la[] as it stands on the device — k_trace_exits, k_trace_link, k_trace_emit (zmx_trace.h) — and the run's results.
// ONE host round trip: the results travel behind the last kernel and the host waits for the copy (waiting for ev[3]
// first and only then asking for the copy was two).  The task statistics come along (zeroed by the next run's k_wtab).
// On success the stores of slot[b] are the blocks' (store_begin) and the histograms are kept for the next run's guess.
static int TraceAndCollect(zmx_ctx* c, zmx_tables* t, const TraceSegParams& tp, const int32_t* slot, uint32_t* nsym,
                           uint32_t* hist, bool timing, u32* segstats, const char* who) {
  const size_t nb = t->nb;
  const unsigned nblk = static_cast<unsigned>(nb);
  const unsigned nseg = t->seg_off[nb];
  if (nseg) hipLaunchKernelGGL(k_trace_exits, dim3(nseg), dim3(TS_THREADS), 0, c->stream, tp);
  KCHK(c, "k_trace_exits");
  hipLaunchKernelGGL(k_trace_link, dim3(nblk), dim3(64), 0, c->stream, tp);
  KCHK(c, "k_trace_link");
  if (nseg) hipLaunchKernelGGL(k_trace_emit, dim3(nseg), dim3(64), 0, c->stream, tp);
  KCHK(c, "k_trace_emit");
  if (timing) HIPCHK(hipEventRecord(c->ev[3], c->stream));
  HIPCHK(hipMemcpyAsync(t->h_runout, t->d_runout, t->run.out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const u32* o_flags = t->run.flags(t->h_runout);
  std::memcpy(hist, t->run.hist(t->h_runout), nb * ZMX_HIST * sizeof(u32));
  std::memcpy(nsym, t->run.nsym(t->h_runout), nb * sizeof(u32));
  std::memcpy(segstats, t->run.stats(t->h_runout), RunLayout::kStats * sizeof(u32));
  if (o_flags[1]) {
    char buf[128];
    std::snprintf(buf, sizeof(buf), "%s: device consistency flags 0x%x", who, o_flags[1]);
    return FailFault(buf);
  }
  t->h_hist.assign(hist, hist + nb * ZMX_HIST);
  t->have_hist = true;
  for (size_t b = 0; b < nb; ++b) t->store_begin[slot[b]][b] = t->bsize[b] - nsym[b];
  return 0;
}

constexpr unsigned kRedoGrid = 1024;   // the redo pass: 256 CUs x 4 workgroups (LDS-limited)
// The speculative pass over `grid` workgroups of four waves each: the variant for run tasks or the one for the others, with
// the profile counters when the run has them.  k_dp5_spec, a task a wave, where no stretch is longer than the four
// waves, and for the redo pass of a table set with run tasks; k_dp5_stretch, whose waves pull tasks until the stretch is
// empty, for longer stretches and for the packed redo list.
static void LaunchSpec(hipStream_t stream, unsigned grid, bool run_tasks, const Dp4Params& p) {
  const dim3 g(grid), b(64 * D5_WG);
  const bool pull = p.redo_pass ? p.redo_pack > 1 : Knobs().seg_stretch > D5_WG || Knobs().seg_pull;
  if (pull) {
    if (run_tasks) {
      if (p.prof) hipLaunchKernelGGL((k_dp5_stretch<true, 2, true>), g, b, 0, stream, p);
      else hipLaunchKernelGGL((k_dp5_stretch<false, 2, true>), g, b, 0, stream, p);
    } else {
      if (p.prof) hipLaunchKernelGGL((k_dp5_stretch<true, 4, false>), g, b, 0, stream, p);
      else hipLaunchKernelGGL((k_dp5_stretch<false, 4, false>), g, b, 0, stream, p);
    }
  } else if (run_tasks) {
    if (p.prof) hipLaunchKernelGGL((k_dp5_spec<true, 2, true>), g, b, 0, stream, p);
    else hipLaunchKernelGGL((k_dp5_spec<false, 2, true>), g, b, 0, stream, p);
  } else {
    if (p.prof) hipLaunchKernelGGL((k_dp5_spec<true, 4, false>), g, b, 0, stream, p);
    else hipLaunchKernelGGL((k_dp5_spec<false, 4, false>), g, b, 0, stream, p);
  }
}
// k_dp4_fix, a workgroup per block: the serial pass that accepts the tasks or runs them again
static void LaunchFix(hipStream_t stream, unsigned nblk, const Dp4Params& p) {
  const dim3 b(64 * (D3_NB + 2));
  if (p.prof) hipLaunchKernelGGL(k_dp4_fix<true>, dim3(nblk), b, 0, stream, p);
  else hipLaunchKernelGGL(k_dp4_fix<false>, dim3(nblk), b, 0, stream, p);
}

int zmx_squeeze_run(zmx_ctx* c, zmx_tables* t, const double* cost, const double* mincost, const int32_t* slot,
                    uint32_t* nsym, uint32_t* hist) {
  if (const int rc = CheckTables("zmx_squeeze_run", t, zamd::SqueezeRunNeeds(t ? t->nb : 0))) return rc;
  if (t->nb == 0) return 0;
  DEVICE_ENTRY(c->device);
  for (size_t b = 0; b < t->nb; ++b) {
    if (slot[b] != 0 && slot[b] != 1) return FailMsg("zmx_squeeze_run: slot must be 0 or 1");
  }
  const size_t nb = t->nb;
  const zamd::DeviceKnobs& knobs = Knobs();
  bool any_below_mincost = false;
  // the run's input in the pinned mirror: costs, mincosts, slots, and per block what the chain's acceptance test has
  // to know about this cost model (RunInfo)
  {
    const RunLayout& run = t->run;
    float* wmax = run.wmax(t->h_runin);
    u32* tiemask = run.tiemask(t->h_runin);
    float* est = run.est(t->h_runin);
    std::memcpy(run.cost(t->h_runin), cost, nb * ZMX_HIST * sizeof(double));
    std::memcpy(run.mincost(t->h_runin), mincost, nb * sizeof(double));
    std::memcpy(run.slot(t->h_runin), slot, nb * sizeof(int));
    const u32* hh = t->have_hist ? t->h_hist.data() : nullptr;
    std::vector<char> below(nb, 0);
    zamd::ParallelFor(nb, [&](size_t b) {
      bool bad = false;
      RunInfo(cost + b * ZMX_HIST, hh ? hh + b * ZMX_HIST : nullptr, t->bsize[b], &wmax[b], &tiemask[b], &est[b], mincost[b], &bad);
      below[b] = bad ? 1 : 0;
    });
    for (size_t b = 0; b < nb; ++b) any_below_mincost |= below[b] != 0;
  }
  HIPCHK(hipMemcpyAsync(t->d_runin, t->h_runin, t->run.in_bytes, hipMemcpyHostToDevice, c->stream));
  if (knobs.prof && !t->d_prof) HIPCHK(PoolAlloc(c, &t->d_prof, nb * ZMX_PROF_N));
  if (t->d_prof) HIPCHK(hipMemsetAsync(t->d_prof, 0, nb * ZMX_PROF_N * sizeof(u64), c->stream));
  // the chain's parameters: the table set's block and what this run adds
  Dp4Params cp = t->params.dp;
  cp.est_bits = t->squeeze_runs == 0 ? t->run.est(t->d_runin) : nullptr;
  cp.prof = t->d_prof;
  cp.mid = knobs.seg_mid ? t->d_mid : nullptr;
  cp.level_scale = knobs.seg_scale;
  cp.debug = knobs.seg_debug;
  cp.fix_lean_min = knobs.fix_lean;
  cp.int_path = knobs.int_path;
  cp.chain_fast = knobs.shortcut_chain;
  // k_badscan's bitmap: all zero unless some block of this run has a match weight below mincost (RunInfo) — nearly never,
  // and then neither the memset nor the scan is launched (two of a run's ~20 stream operations; a small call is mostly
  // the gaps between them)
  const bool scan_bad = any_below_mincost;
  if (scan_bad || !t->badpos_clean) HIPCHK(hipMemsetAsync(t->d_badpos, 0, t->badpos_words * sizeof(u32), c->stream));
  t->badpos_clean = !scan_bad;
  double ksec[3] = {0, 0, 0};
  const bool timing = KernelTiming();
  {
    const unsigned nblk = static_cast<unsigned>(nb);
    const unsigned tiles = t->tile_off[nb];
    const unsigned ntask = t->task_off[nb];
    if (timing) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    // the run's weights per block, and (rarely) the positions that own an edge below mincost
    hipLaunchKernelGGL(k_wtab, dim3(nblk), dim3(256), 0, c->stream, t->params.wtab);
    KCHK(c, "k_wtab");
    if (tiles && scan_bad) hipLaunchKernelGGL(k_badscan, dim3(tiles), dim3(256), 0, c->stream, t->params.badscan);
    KCHK(c, "k_badscan");
    if (timing) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    // the chain: every task speculatively on all CUs (four tasks of a block per workgroup, the workgroups
    // with a head first), then the per-block walk that accepts or re-runs
    {
      // the run tasks on a second stream, beside the others: few and long (one wave may walk 100 000 positions)
      if (t->n_wg_runs) {
        HIPCHK(hipEventRecord(c->ev2[0], c->stream));
        HIPCHK(hipStreamWaitEvent(c->stream2, c->ev2[0], 0));
        Dp4Params cr = cp;
        cr.task0 = t->n_wg;
        LaunchSpec(c->stream2, t->n_wg_runs, true, cr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev2[1], c->stream2));
      }
      if (t->n_wg) {
        LaunchSpec(c->stream, t->n_wg, false, cp);
        HIPCHK(hipGetLastError());
      }
      if (t->n_wg_runs) HIPCHK(hipStreamWaitEvent(c->stream, c->ev2[1], 0));
      if (GuardOn()) HIPCHK(hipStreamSynchronize(c->stream2));
      KCHK(c, "k_dp5_spec");
    }
    if (ntask > nblk) {
      hipLaunchKernelGGL(k_dpcheck, dim3(ntask), dim3(64), 0, c->stream, cp);
      KCHK(c, "k_dpcheck");
      // a second speculative run, from the level the chain of shifts implies, for the tasks that only
      // missed their level (ZOPFLI_AMD_SEG_REDO=0: leave them to the serial pass)
      // (ZOPFLI_AMD_SEG_REDO = how many such passes, default 1.  More settle more tasks before the serial pass — class Z:
      //  87 / 92 / 93 % accepted with 1 / 2 / 3 — but every pass waits for its longest task: 1 264 / 1 362 / 1 601 ms)
      for (int pass = 0; pass < knobs.seg_redo; ++pass) {
        // (the lists' counters were zeroed by the check before: zmx_dp4.h)
        Dp4Params c2 = cp;
        c2.redo_pass = 1;
        c2.est_bits = nullptr;
        c2.redo_parity = pass & 1;
        c2.redo_pack = t->n_wg_runs != 0 ? 1 : 4;
        hipLaunchKernelGGL(k_dpscan, dim3(nblk), dim3(64), 0, c->stream, c2);
        KCHK(c, "k_dpscan");
        // (text: the list holds up to four tasks of a block per entry — about 1 % of the tasks — and the workgroups stride
        //  over it: a grid of the device's resident workgroups at most.  A table set with run tasks keeps a task an entry and
        //  a workgroup a task, by the variant for run tasks: what is run again there is mostly theirs, few and long, and
        //  packed it measured slower — class Z, profiles/chain_stretch.txt)
        LaunchSpec(c->stream, c2.redo_pack > 1 ? std::min(ntask, kRedoGrid) : ntask, t->n_wg_runs != 0, c2);
        KCHK(c, "k_dp5_spec (redo)");
        // only the checks of the listed tasks and their successors can have changed
        hipLaunchKernelGGL(k_dprecheck, dim3(std::min(ntask, DPRECHECK_GRID)), dim3(64), 0, c->stream, c2);
        KCHK(c, "k_dprecheck");
      }
      LaunchFix(c->stream, nblk, cp);
      KCHK(c, "k_dp4_fix");
    }
    if (timing) HIPCHK(hipEventRecord(c->ev[2], c->stream));
  }
  // the walk back over length_array, the symbols, and the run's ONE host round trip (TraceAndCollect)
  u32 segstats[RunLayout::kStats];
  if (const int rc = TraceAndCollect(c, t, t->params.trace, slot, nsym, hist, timing, segstats, "zmx_squeeze_run")) return rc;
  for (int i = 0; i < 3 && timing; ++i) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
    ksec[i] += ms * 1e-3;
  }
  ++t->squeeze_runs;
  {
    zmx_stats& ts = zamd::ThreadStats();   // (thread-local: no lock)
    for (int i = 0; i < 3; ++i) ts.kernel_seconds[i] += ksec[i];
    ts.squeeze_launches += 1;
    // (the host's last slot is the positions of the blocks, not the device's count of lean jobs: zmx_seg_stat)
    for (int i = 0; i < ZMX_SEG_N; ++i) ts.seg[i] += i == ZMX_SEG_POSITIONS ? static_cast<double>(t->total_b) : segstats[i];
  }
  if (t->d_prof) return ReportSqueezeProf(t, ksec, segstats);
  return 0;
}

// Test entry: the tail of a squeeze run on length arrays the caller hands in (tests/test_gpu_walk_edges.py).  What the
// kernels cannot bound themselves is refused here, before any launch: a cell h may hold 0 (GetBestLengths never reached
// it), 1 or a length 3 .. min(h, 258).  Whether the path meets a 0, or a length its record does not hold, is the
// device's own business (flags 2 and 4 of k_trace_emit).
int zmx_trace_length_arrays(zmx_ctx* c, zmx_tables* t, size_t nblocks, const uint16_t* const* length_arrays,
                            const size_t* entries, const int32_t* slot, uint32_t* nsym, uint32_t* hist) {
  if (const int rc = CheckTables("zmx_trace_length_arrays", t, zamd::kWithDp)) return rc;
  if (const int rc = Refused(zamd::CheckLengthArrays("zmx_trace_length_arrays", t->nb, [&](size_t b) { return size_t{t->bsize[b]}; },
                                                     nblocks, length_arrays, entries, slot))) return rc;
  const size_t nb = t->nb;
  if (nb == 0) return 0;
  DEVICE_ENTRY(c->device);
  // la[] rows as LayoutBlocks laid them out (padded to 8 entries), in one blocking copy
  const BlockDesc& last = t->blocks[nb - 1];
  std::vector<u16> rows(last.la_off + ((static_cast<u64>(t->bsize[nb - 1]) + 1 + 7) & ~7ull), 0);
  for (size_t b = 0; b < nb; ++b) std::memcpy(rows.data() + t->blocks[b].la_off, length_arrays[b], entries[b] * sizeof(u16));
  HIPCHK(hipMemcpy(t->d_la, rows.data(), rows.size() * sizeof(u16), hipMemcpyHostToDevice));
  int* h_slot = t->run.slot(t->h_runin);
  std::memcpy(h_slot, slot, nb * sizeof(int));
  HIPCHK(hipMemcpyAsync(t->run.slot(t->d_runin), h_slot, nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
  // (the flag words are zeroed when the tables are built and by nothing a squeeze run launches: this call judges its
  //  own arrays alone, and what it reports must not fail the next call on these tables too)
  HIPCHK(hipMemsetAsync(t->run.flags(t->d_runout), 0, RunLayout::kFlags * sizeof(u32), c->stream));
  u32 segstats[RunLayout::kStats];
  const int rc = TraceAndCollect(c, t, t->params.trace, slot, nsym, hist, false, segstats, "zmx_trace_length_arrays");
  if (rc) (void)hipMemsetAsync(t->run.flags(t->d_runout), 0, RunLayout::kFlags * sizeof(u32), c->stream);
  return rc;
}
}  // extern "C"
