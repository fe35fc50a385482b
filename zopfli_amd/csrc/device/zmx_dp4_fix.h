// k_dp4_fix: the serial pass of the chain.  It uses the jobs of both files: d4_run_job (zmx_dp4.h) and d5_run_job
// (zmx_dp5.h), and the integer table's record of zmx_dp5_spec.h.  Included only by zmx_hip.hip, after those.
#pragma once

// ---------------------------------------------------------------------------------------------
// FIX: one workgroup per block walks the block's tasks in order, accepts every task whose entry
// state is the true state up to a shift that keeps the task inside its binade, and runs the others
// again from the true state — the serial chain, for exactly the stretches that need it.  A re-run uses
// k_dp4's four-wave pipeline (d4_run_job: 57 cycles per position on text, but a ring restart and two
// bubble steps per long-run shortcut and 14 positions per step where rows are 258 wide), or, for a
// task with at least P.fix_lean_min windows of the generic kind (shortcut flags, long rows), the lean
// one-wave job of k_dp5_spec (d5_run_job in load mode: a shortcut is a handful of LDS operations).
// ---------------------------------------------------------------------------------------------
#define FIX_CH 256u       // tasks whose summaries k_dp4_fix holds in LDS at a time
template <bool PROF>
__global__ __launch_bounds__(64 * (D3_NB + 2)) void k_dp4_fix(Dp4Params P) {
  D4_LDS_DECL
  const u32 b = P.block0 + blockIdx.x;
  const BlockDesc bd = P.blocks[b];
  const u32 B = (u32)(bd.inend - bd.instart);
  if (B == 0) return;
  const u32 t0 = P.task_off[b], t1 = P.task_off[b + 1];
  const u32 lane = threadIdx.x & 63;
  const bool lead = threadIdx.x == 0;
  const double wmax = (double)P.wmax[b] + 1.0;
  const u32 tiemask = P.tiemask[b];
  for (u32 i = threadIdx.x; i < ZMX_WTAB; i += blockDim.x) s_wtab[i] = P.wtab[(u64)b * ZMX_WTAB + i];
  __syncthreads();
  __shared__ __align__(8) double s_w1[D5_W1];
  __shared__ u8 s_sym1[D5_W1];
  __shared__ __align__(8) uint2 s_ri[32];
  d5_build_w1(s_wtab, s_w1, s_sym1);
  u16* la_block = P.la + bd.la_off;
  d4_copy_over(P, t0, B, la_block);   // the head is exact
  double delta_prev = 0.0;     // what has to be added to exit[t - 1] to get the true values
  bool rerun_prev = false;     // exit[t - 1] was rewritten by this workgroup: P.chk[t] is stale
  u32 n_ok = 0, n_state = 0, n_level = 0, n_tie = 0, n_pos = 0, n_values = 0, n_lean = 0, n_mid = 0;
  const u32* winflag = P.winflag + P.win_off[b];
  const u64 cyc0 = __builtin_readcyclecounter();
  u64 cyc_run = 0;
  // The walk reads a few words per task and almost always just accepts it: with a dependent global load or two
  // per task, 240 tasks a block, the walk — not the re-runs — was most of this kernel's 0.75 ms.  So: the tasks'
  // summaries come into LDS FIX_CH at a time in one sweep, and what an accepted task leaves to do (its overshoot
  // cells into length_array, its level for the next run) is done for the whole chunk afterwards, all threads at once.
  __shared__ double s_ck_d[FIX_CH], s_dl[FIX_CH];
  __shared__ float s_ck_vmin[FIX_CH], s_vmax[FIX_CH];
  __shared__ u32 s_ck_match[FIX_CH], s_xbase[FIX_CH], s_pend[FIX_CH], s_acc[FIX_CH];
  __shared__ double s_wsum[4], s_dprev;
  __shared__ u32 s_wfail[4];
  static_assert(FIX_CH == 64 * (D3_NB + 2), "the sweep judges a chunk's tasks a thread each");
  for (u32 c0 = t0 + 1; c0 < t1; c0 += FIX_CH) {
  const u32 cn = t1 - c0 < FIX_CH ? t1 - c0 : FIX_CH;
  for (u32 i = threadIdx.x; i < cn; i += blockDim.x) {
    const SegCheck k = P.chk[c0 + i];
    s_ck_d[i] = k.d; s_ck_vmin[i] = k.vmin; s_ck_match[i] = k.match;
    s_vmax[i] = P.exit[c0 + i].vmax;
    s_xbase[i] = P.exit[c0 + i].base + P.exit[c0 + i].skip;   // (where the task's own cells end: d4_copy_over)
    s_pend[i] = P.tasks[c0 + i].pend;
    s_acc[i] = 0;
    s_dl[i] = 0.0;
  }
  __syncthreads();
  for (u32 t = c0; t < c0 + cn; ++t) {
    // The walk, a SWEEP at a time (round 5): nearly every task is simply accepted, and deciding so one task after the
    // other — four waves doing the same dozen double-precision operations — was 1 200 cycles a task, 0.25 ms of this
    // kernel's 0.43 per 1 MB block.  All tasks of the chunk from t on are judged at once, a thread each: their shifts are a
    // prefix sum of the checks' differences (sums of multiples of float ulps: exact in any order, as in k_dpscan), the
    // acceptance test is the one below with that shift; everything up to the first task that fails is accepted, and
    // that task takes the serial step — which re-runs it — as before.  (Not behind a re-run: the next task's check is stale.)
    if (!rerun_prev) {
      const u32 ti0 = t - c0;
      const u32 i = threadIdx.x;                       // (FIX_CH = the workgroup's threads: a thread per task of the chunk)
      const bool act = i >= ti0 && i < cn;
      double incl = act ? s_ck_d[i] : 0.0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += up;
      }
      if (lane == 63) s_wsum[threadIdx.x >> 6] = incl;
      __syncthreads();
      double before = 0.0;
      for (u32 w = 0; w < (threadIdx.x >> 6); ++w) before += s_wsum[w];
      const double delta_i = delta_prev + before + incl;
      const bool ok_i = act && s_ck_match[i] == 1 && d4_accept(s_ck_vmin[i], (double)s_vmax[i], delta_i, wmax, tiemask) == 0;
      const u64 failm = __ballot(act && !ok_i);
      if (lane == 0) s_wfail[threadIdx.x >> 6] = failm ? (threadIdx.x & ~63u) + (u32)__ffsll((long long)failm) - 1u : 0xffffffffu;
      __syncthreads();
      u32 first_fail = cn;
      for (u32 w = 0; w < (blockDim.x >> 6); ++w) first_fail = s_wfail[w] < first_fail ? s_wfail[w] : first_fail;
      if (act && i < first_fail) { s_acc[i] = 1; s_dl[i] = delta_i; }
      if (first_fail > ti0 && i == first_fail - 1u) s_dprev = delta_i;
      __syncthreads();
      if (first_fail > ti0) { delta_prev = s_dprev; n_ok += first_fail - ti0; }
      t = c0 + first_fail;
      if (t >= c0 + cn) break;
    }
    const u32 ti = t - c0;
    SegCheck ck;
    if (rerun_prev) ck = d4_check(&P.exit[t - 1], &P.entry[t], lane);   // every wave computes the same
    else { ck.d = s_ck_d[ti]; ck.vmin = s_ck_vmin[ti]; ck.match = s_ck_match[ti]; }
    const double delta = delta_prev + ck.d;
    // the guess to start the next run of this task from
    if (lead) s_dl[ti] = delta;
    bool ok = ck.match == 1;
    u32 why = 0;
    if (ok) {
      why = d4_accept(ck.vmin, (double)s_vmax[ti], delta, wmax, tiemask);
      ok = why == 0;
    }
    if (P.debug == 6 && ck.match == 0 && threadIdx.x < 64) {
      // where the two states differ: the first cell whose reach, source or value shape is not the same
      const SegSnap* E = &P.exit[t - 1];
      const SegSnap* N = &P.entry[t];
      u32 first = 0xffffffffu;
      for (int s6 = 0; s6 < 6; ++s6) {
        const u32 i = 64u * s6 + lane;
        const bool ef = E->c[i] < 1e29f, nf = N->c[i] < 1e29f;
        if ((ef != nf || E->l[i] != N->l[i]) && i < first) first = i;
      }
      for (int o = 32; o >= 1; o >>= 1) { const u32 v = __shfl_xor(first, o, 64); first = v < first ? v : first; }
      if (lane == 0) {
        const u32 i = first < SEG_CELLS ? first : 0;
        printf("diff b %u t %u pout %u base %u/%u noshort %u/%u skip %u/%u first cell %u: exit c %.4f l %u | entry c %.4f l %u | q %u\n", b, t - t0, P.tasks[t].pout,
               E->base, N->base, E->noshort, N->noshort, E->skip, N->skip, first, (double)E->c[i], E->l[i], (double)N->c[i], N->l[i], P.tasks[t].q);
      }
    }
    if (P.debug == 1 && lead) {
      printf("fix b %u t %u pout %u: match %u d %.6f delta %.6f vmin %.4f vmax %.4f why %u ok %d entry base %u exit-1 base %u\n", b,
             t - t0, P.tasks[t].pout, ck.match, ck.d, delta, (double)ck.vmin, (double)P.exit[t].vmax, why, ok ? 1 : 0,
             P.entry[t].base, P.exit[t - 1].base);
    }
    if (ok) {
      if (lead) s_acc[ti] = 1;
      delta_prev = delta;
      rerun_prev = false;
      ++n_ok;
      continue;
    }
    if (ck.match == 0) ++n_state; else if (ck.match == 2) ++n_values; else if (why == 1) ++n_level; else ++n_tie;
    const SegTask T = P.tasks[t];
    D4Job J;
    J.start = P.exit[t - 1].base;
    J.noshort = P.exit[t - 1].noshort;
    J.pout = 0;
    J.pend = T.pend;
    J.over_lo = SEG_NONE;    // (this workgroup is the only writer of the block's length_array now)
    J.spec = false;
    J.load = true;
    J.level = 0.0f;
    J.delta = delta_prev;
    J.init = &P.exit[t - 1];
    J.entry = nullptr;
    J.exit = &P.exit[t];
    J.over = nullptr;
    // The task matched its predecessor and only grew out of its binade: if what it did up to its mid snapshot passes the
    // test (the same test, with the largest source value of that prefix), the prefix stands — its lengths are in
    // length_array already — and the re-run starts at the snapshot, from the task's own cells plus the shift.
    bool from_mid = false;
    if (ck.match == 1 && why == 1 && P.mid != nullptr) {
      const u32 mb_ = P.mid[t].base;
      if (mb_ != SEG_NONE && mb_ > P.entry[t].base && mb_ < (T.pend < B ? T.pend : B) &&
          d4_accept(ck.vmin, (double)P.mid[t].vmax, delta, wmax, tiemask) == 0) {
        from_mid = true;
        J.start = mb_;
        J.noshort = P.mid[t].noshort;
        J.delta = delta;
        J.init = &P.mid[t];
        ++n_mid;
      }
    }
    J.la_lo = J.start;
    n_pos += (T.pend < B ? T.pend : B) - (J.start < B ? J.start : B);
    // windows of the task that k_dp5_spec's fast paths cannot take (k_mkdesc)
    const u32 w0 = J.start >> 5, w1 = ((T.pend < B ? T.pend : B) + 31u) >> 5;
    u32 generic = 0, mine = 0, nocodes = 0;
    for (u32 w = w0 + threadIdx.x; w < w1; w += blockDim.x) {
      generic += (winflag[w] & 0xffu) == 0 ? 1u : 0u;
      nocodes |= winflag[w] & D5_WF_CODELESS;
      ++mine;
    }
    // (the barriers also mean: every wave has read the old exit[t] / exit[t - 1])
    // (automatic, P.fix_lean_min < 0: the lean job where most of the windows are of the generic kind — runs of equal
    //  bytes: its run-row path reads no codes, the pipeline's ring would restart at every shortcut.  Counted per
    //  thread: a merged task has thousands of windows)
    const int n_generic = __syncthreads_count((int)generic);
    const int n_major = __syncthreads_count(mine > 0 && 2 * generic >= mine ? 1 : 0);
    const int n_have = __syncthreads_count(mine > 0 ? 1 : 0);
    const int n_nocodes = __syncthreads_count(nocodes != 0 ? 1 : 0);   // (a wide run row without codes: only the lean job's tables know its weights)
    // (a predecessor that stopped inside a shortcut's window — skip — can only be continued by the job that knows
    //  about it)
    const bool lean = (!from_mid && P.exit[t - 1].skip != 0) || n_nocodes > 0 || (P.fix_lean_min >= 0 ? n_generic >= P.fix_lean_min : 2 * n_major >= n_have);
    const u64 cr0 = __builtin_readcyclecounter();
    if (lean) {
      ++n_lean;
      const D5IntTab IT = d5_inttab(false, 0u, 0u);   // (no table)
      if (threadIdx.x < 64) {
        d5_run_job<PROF, true>(P, J, b, bd, s_wtab, s_xc, s_xl, s_ring, *reinterpret_cast<const uint2 (*)[ZMX_WTAB]>(&s_t1[0][0]), IT, s_w1, s_sym1, s_ri,
                               reinterpret_cast<uint2*>(&s_t2[0][0]));   // (s_rk: the pipeline's tiles are idle in this job)
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    } else {
      d4_run_job<PROF>(P, J, b, bd, s_ring, s_wtab, s_t1, s_t2, s_tab, s_desc, s_tabc, s_xc, s_xl, s_lout);
    }
    cyc_run += __builtin_readcyclecounter() - cr0;
    delta_prev = 0.0;
    rerun_prev = true;
  }
  __syncthreads();
  // the chunk's accepted tasks: their cells beyond pend (d4_copy_over), one task per wave at a time; and every
  // task's level for the next run
  // (sixteen lanes a task, sixteen tasks at a time: a task's copy is one or two dependent global round trips of a few dozen
  //  cells, and with a wave per task — four in flight — those round trips were a third of this kernel on text)
  for (u32 i = threadIdx.x >> 4; i < cn; i += blockDim.x >> 4) {
    if (!s_acc[i]) continue;
    const u32 pend = s_pend[i], stop = s_xbase[i];
    if (pend > B) continue;                   // the last task of the block runs to the end
    const u16* over = P.over + (u64)(c0 + i) * SEG_OVER;
    for (u32 k = threadIdx.x & 15u; pend + k < stop && pend + k <= B; k += 16) la_block[pend + k] = over[k];
  }
  for (u32 i = threadIdx.x; i < cn; i += blockDim.x) P.lvl[c0 + i] = (float)((double)P.lvl[c0 + i] + s_dl[i]);
  __syncthreads();
  }
  if (P.debug >= 2 && lead) {
    printf("fix b %u: %u tasks ok %u state %u values %u level %u (%u of them from their mid snapshot) tie %u lean %u, %u positions re-run, %llu cycles in all, %llu in re-runs\n", b,
           t1 - t0, n_ok, n_state, n_values, n_level, n_mid, n_tie, n_lean, n_pos, (unsigned long long)(__builtin_readcyclecounter() - cyc0),
           (unsigned long long)cyc_run);
  }
  if (lead && P.stats) {
    atomicAdd(&P.stats[ZMX_SEG_TASKS], t1 - t0);
    atomicAdd(&P.stats[ZMX_SEG_ACCEPTED], n_ok);
    atomicAdd(&P.stats[ZMX_SEG_RERUN_STATE], n_state);
    atomicAdd(&P.stats[ZMX_SEG_RERUN_LEVEL], n_level);
    atomicAdd(&P.stats[ZMX_SEG_RERUN_TIE], n_tie);
    atomicAdd(&P.stats[ZMX_SEG_POSITIONS_RERUN], n_pos);
    atomicAdd(&P.stats[ZMX_SEG_RERUN_VALUES], n_values);
    atomicAdd(&P.stats[ZMX_SEG_DEV_LEAN], n_lean);
  }
}
