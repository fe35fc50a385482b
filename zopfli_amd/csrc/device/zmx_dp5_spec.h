// k_dp5_spec and k_dp5_stretch: the speculative pass over the chain's tasks, d5_run_job (zmx_dp5.h) a task a wave, and
// the set-up the two kernels share.  Included only by zmx_hip.hip, after zmx_dp5.h.
#pragma once

// ---- the set-up of a speculative workgroup, one definition for both kernels: the tables in LDS, the level a task
// starts from, the integer table, the task's job, the PROF bookkeeping around the tasks
#define D5_WG 4u
// The workgroup's LDS (RUNS: the kernel's template parameter), and the PROF words: when the waves of the workgroup
// finished (sum, latest, how many).
#define D5_LDS_DECL                                                                                                       \
  __shared__ __align__(16) double s_wtab[ZMX_WTAB];                                                                       \
  /* per wave: the staged codes of a window (4 KB + the alignment slack), or the cells of a long-run shortcut */          \
  __shared__ __align__(16) unsigned char s_buf[D5_WG][D5_STAGE_BYTES];                                                    \
  __shared__ __align__(8) uint2 s_itab[ZMX_WTAB];                                                                         \
  __shared__ __align__(8) double s_w1[D5_W1];                                                                             \
  __shared__ u8 s_sym1[D5_W1];                                                                                            \
  __shared__ __align__(8) uint2 s_ri[D5_WG][32];                                                                          \
  __shared__ __align__(8) uint2 s_rk[RUNS ? D5_WG : 1u][RUNS ? D5_RKN : 1u];                                              \
  __shared__ u32 s_rmax;
#define D5_PROF_LDS_DECL __shared__ unsigned long long s_pf_sum, s_pf_max; __shared__ u32 s_pf_done;

// The level a speculative task starts from: task t of `block` (B positions), first position q.
__device__ __forceinline__ float d5_task_level(const Dp4Params& P, u32 t, u32 block, u32 q, u32 B) {
  float lv = P.est_bits ? P.est_bits[block] * ((float)q / (float)B) : P.lvl[t];
  if (!P.redo_pass) lv *= P.level_scale;
  return lv >= 16.0f ? lv : 16.0f;
}
// ... of a task whose record is still in global memory
__device__ __forceinline__ float d5_task_level(const Dp4Params& P, u32 t) {
  const SegTask K = P.tasks[t];
  return d5_task_level(P, t, K.block, K.q, (u32)(P.blocks[K.block].inend - P.blocks[K.block].instart));
}

// Whether a workgroup of block b gets an integer table (D5IntTab) for a task whose level has the bit pattern lb, and for
// which binade: e.  Not where the binade is out of range or a weight can tie in it.
__device__ __forceinline__ bool d5_inttab_binade(const u32* tiemask, u32 b, u32 lb, int& e) {
  e = (int)(lb >> 23) - 127;
  return e >= 4 && e < 31 && ((tiemask[b] >> (e & 31)) & 1u) == 0;
}
// The table's record: on = d5_build_inttab built it for the binade of lo, rmax = what it left in s_rmax.
__device__ __forceinline__ D5IntTab d5_inttab(bool on, u32 lo, u32 rmax) {
  D5IntTab IT;
  IT.on = on; IT.lo = lo;
  IT.span = !on ? 0u : rmax < 0x100000u ? 33u * rmax : 0x40000000u;
  return IT;
}

// The job J of task t (T: its record; B: the positions of its block) in the speculative pass, all of it but how it
// starts: J.spec, J.la_lo and J.level are the kernel's, which knows where the task's level is.  A macro: as a function,
// in every shape tried, it cost the PROF instantiations for run tasks vector spills (profiles/chain_setup.txt).
#define D5_SPEC_JOB(J, P, t, T, B)                                                                                        \
  J.start = T.q & ~31u; J.cell = T.q & 31u;   /* windows lie at multiples of 32 from the block start */                   \
  J.noshort = 0; J.pout = T.pout; J.pend = T.pend;                                                                        \
  J.load = false; J.delta = 0; J.init = nullptr;                                                                          \
  J.entry = &P.entry[t]; J.exit = &P.exit[t];                                                                             \
  /* (round 3: run tasks only — the long ones, tens of thousands of positions between two cut points; round 5: text   */ \
  /*  tasks too: a block has a binade boundary per doubling of its cost whatever its size, and in a SMALL call the     */ \
  /*  serial re-runs of the tasks that cross one were most of k_dp4_fix: 0.66 ms per run of a 1 MB call)               */ \
  J.mid = T.pout != 0 && P.mid != nullptr ? &P.mid[t] : nullptr;                                                          \
  J.over_lo = T.pend <= B ? T.pend : SEG_NONE;                                                                            \
  J.over = P.over + (u64)t * SEG_OVER;

// PROF, the fixed cost around the tasks (PF_SETUP_CYC .. PF_ALIVE_CYC of block b0), a wave's lane 0 for the wave.
// The set-up is done: from workgroup (or entry) start, t_wg0, to the wave's first position.
__device__ __forceinline__ void d5_prof_setup_done(const Dp4Params& P, u32 b0, u64 t_wg0) {
  atomicAdd(&P.prof[(u64)b0 * ZMX_PROF_N + PF_SETUP_CYC], (u64)__builtin_readcyclecounter() - t_wg0);
  atomicAdd(&P.prof[(u64)b0 * ZMX_PROF_N + PF_SETUP_WAVES], 1ull);
}
// A wave is done — with its tasks, or without one.  The last of the four adds, for all of them, (latest finish) - (own
// finish): wave cycles spent finished in a live workgroup.
__device__ __forceinline__ void d5_prof_wave_done(const Dp4Params& P, u32 b0, u64 t_wg0, unsigned long long& s_pf_sum,
                                                  unsigned long long& s_pf_max, u32& s_pf_done) {
  const unsigned long long te = (unsigned long long)((u64)__builtin_readcyclecounter() - t_wg0);
  atomicAdd(&s_pf_sum, te);
  atomicMax(&s_pf_max, te);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (atomicAdd(&s_pf_done, 1u) == D5_WG - 1u) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    atomicAdd(&P.prof[(u64)b0 * ZMX_PROF_N + PF_IDLE_CYC], (u64)(D5_WG * s_pf_max - s_pf_sum));
    atomicAdd(&P.prof[(u64)b0 * ZMX_PROF_N + PF_ALIVE_CYC], (u64)(D5_WG * s_pf_max));
  }
}

// k_dp5_spec: a workgroup = four waves = up to four tasks of ONE block and one kind — a stretch (P.wg_desc) of at most
// four entries of the block's task list (P.wg_tasks), a task a wave —, sharing the run's weight table in LDS; after the
// table is in place the waves go their own ways.  This is the form the main pass runs by default: the window loop of
// d5_run_job is at the edge of its register budget, and a loop over tasks around it (k_dp5_stretch, below) costs it 7 %.
template <bool PROF, int WAVES, bool RUNS>
__global__ __launch_bounds__(64 * D5_WG, WAVES) void k_dp5_spec(Dp4Params P) {
  D5_LDS_DECL
  D5_PROF_LDS_DECL
  const u64 t_wg0 = PROF ? (u64)__builtin_readcyclecounter() : 0ull;
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (the redo pass of a table set with run tasks: k_dpscan's entries of one task each, a workgroup per entry)
  if (P.redo_pass && blockIdx.x >= *P.redo_count) return;
  const uint2 wd = P.redo_pass ? make_uint2(0u, 1u) : P.wg_desc[P.task0 + blockIdx.x];
  const u32* wg = P.redo_pass ? P.redo_wg + (u64)blockIdx.x * D5_WG : P.wg_tasks + wd.x;
  const u32 t0 = wg[0];
  const u32 b0 = P.tasks[t0].block;
  for (u32 i = threadIdx.x; i < ZMX_WTAB; i += 64 * D5_WG) s_wtab[i] = P.wtab[(u64)b0 * ZMX_WTAB + i];
  if (threadIdx.x == 0) { s_rmax = 0; if (PROF) { s_pf_sum = 0; s_pf_max = 0; s_pf_done = 0; } }
  __syncthreads();
  d5_build_w1(s_wtab, s_w1, s_sym1);
  auto prof_done = [&]() {
    if (PROF && P.prof && (threadIdx.x & 63u) == 0) d5_prof_wave_done(P, b0, t_wg0, s_pf_sum, s_pf_max, s_pf_done);
  };
  // the binade of the workgroup's integer table (D5IntTab): that of its first speculative task
  D5IntTab IT = d5_inttab(false, 0u, 0u);
  {
    const u32 tl = P.tasks[t0].pout != 0 ? t0 : wd.y > 1u ? wg[1] : SEG_NONE;
    if (tl != SEG_NONE && P.int_path) {
      const u32 lb = __float_as_uint(d5_task_level(P, tl));
      int e;
      if (d5_inttab_binade(P.tiemask, b0, lb, e)) {
        d5_build_inttab(s_wtab, s_itab, s_rmax, e);
        __syncthreads();
        IT = d5_inttab(true, lb & 0x7f800000u, s_rmax);
      }
    }
  }
  if (wave >= wd.y) { prof_done(); return; }
  const u32 t = wg[wave];
  const SegTask T = P.tasks[t];
  const BlockDesc bd = P.blocks[T.block];
  const u32 B = (u32)(bd.inend - bd.instart);
  if (B == 0) { prof_done(); return; }
  D4Job J;
  D5_SPEC_JOB(J, P, t, T, B)
  if (T.pout == 0) {       // the head of the block
    J.spec = false;
    J.la_lo = 1;
    J.level = 0.0f;
  } else {
    J.spec = true;
    J.la_lo = SEG_NONE;
    J.level = d5_task_level(P, t);
    if (P.est_bits && (threadIdx.x & 63) == 0) P.lvl[t] = J.level;
  }
  if (PROF && P.prof && (threadIdx.x & 63u) == 0) d5_prof_setup_done(P, b0, t_wg0);
  d5_run_job<PROF, RUNS>(P, J, T.block, bd, s_wtab, reinterpret_cast<float*>(s_buf[wave]), reinterpret_cast<u16*>(s_buf[wave] + 4u * DP_XN),
                   reinterpret_cast<u16*>(s_buf[wave]), s_itab, IT, s_w1, s_sym1, s_ri[wave], s_rk[RUNS ? wave : 0u]);
  prof_done();
}

// k_dp5_stretch: one workgroup = four waves = a STRETCH of tasks of ONE block and one kind: `count` consecutive entries of the block's
// task list (P.wg_desc, P.wg_tasks), sharing the run's weight table in LDS.  The set-up — the weight table, the run-row
// weights, the integer table, the tasks' records and levels — is done once per stretch; after it the waves go their own
// ways: each pulls the next entry from a counter in LDS and walks it, until the stretch is empty.  Which wave walks a
// task, and when, does not enter the task's output.  NO workgroup barrier lies behind the set-up in the main pass: a
// wave that finds the stretch empty leaves while the others work.
// The redo pass (P.redo_pass) runs k_dpscan's list instead: entries of up to four tasks of one block, the workgroups
// striding over them; every wave stays for every entry there, so the barriers between two entries are met by all four.
#define D5_STRETCH_MAX 32u   // entries of a stretch at most (ZOPFLI_AMD_SEG_STRETCH): their records are held in LDS
template <bool PROF, int WAVES, bool RUNS>
__global__ __launch_bounds__(64 * D5_WG, WAVES) void k_dp5_stretch(Dp4Params P) {
  D5_LDS_DECL
  // the stretch: its next entry, and per entry the task's id, record and starting level
  __shared__ u32 s_next;
  __shared__ u32 s_hdr[4];         // the stretch's block, entries (0 for an empty block), integer table: built, binade
  __shared__ u32 s_tid[D5_STRETCH_MAX];
  __shared__ __align__(16) SegTask s_task[D5_STRETCH_MAX];
  __shared__ float s_lvl[D5_STRETCH_MAX];
  D5_PROF_LDS_DECL
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 lane = threadIdx.x & 63u;
  u32 item = P.redo_pass ? blockIdx.x : P.task0 + blockIdx.x;
  const u32 n_items = P.redo_pass ? *P.redo_count : item + 1u;
  for (; item < n_items; item += gridDim.x) {
    const u64 t_wg0 = PROF ? (u64)__builtin_readcyclecounter() : 0ull;     // (PROF counts per entry: each has its set-up)
    const u32* list;
    u32 count = 0;
    if (P.redo_pass) {
      list = P.redo_wg + (u64)item * D5_WG;
      while (count < D5_WG && list[count] != SEG_NONE) ++count;
    } else {
      const uint2 d = P.wg_desc[item];
      list = P.wg_tasks + d.x;
      count = d.y < D5_STRETCH_MAX ? d.y : D5_STRETCH_MAX;
    }
    if (count == 0) continue;          // (every thread alike; no list holds such an entry)
    const u32 b0 = P.tasks[list[0]].block;
    const BlockDesc bd = P.blocks[b0];
    const u32 B = (u32)(bd.inend - bd.instart);
    for (u32 i = threadIdx.x; i < ZMX_WTAB; i += 64 * D5_WG) s_wtab[i] = P.wtab[(u64)b0 * ZMX_WTAB + i];
    // the entries' records, and the level a speculative task starts from
    for (u32 i = threadIdx.x; i < count; i += 64 * D5_WG) {
      const u32 tt = list[i];
      const SegTask K = P.tasks[tt];
      float lv = 0.0f;
      if (K.pout != 0) {
        lv = d5_task_level(P, tt, b0, K.q, B);
        if (P.est_bits) P.lvl[tt] = lv;
      }
      s_tid[i] = tt;
      s_task[i] = K;
      s_lvl[i] = lv;
    }
    if (threadIdx.x == 0) { s_rmax = 0; s_next = 0; if (PROF) { s_pf_sum = 0; s_pf_max = 0; s_pf_done = 0; } }
    __syncthreads();
    d5_build_w1(s_wtab, s_w1, s_sym1);
    // the binade of the workgroup's integer table (D5IntTab): that of the stretch's first speculative task;
    // a task of the stretch in another binade walks in doubles
    {
      const u32 il = s_task[0].pout != 0 ? 0u : 1u;
      bool on = false;
      u32 lb = 0;
      if (il < count && P.int_path) {
        lb = __float_as_uint(s_lvl[il]);
        int e;
        if (d5_inttab_binade(P.tiemask, b0, lb, e)) {
          d5_build_inttab(s_wtab, s_itab, s_rmax, e);
          on = true;
        }
      }
      // what the waves need per task goes through LDS: held in registers across the tasks it cost the window loop its own
      if (threadIdx.x == 0) { s_hdr[0] = b0; s_hdr[1] = B != 0 ? count : 0u; s_hdr[2] = on ? 1u : 0u; s_hdr[3] = lb & 0x7f800000u; }
      __syncthreads();
    }
    bool first_job = true;
    for (;;) {
      u32 i = 0;
      if (lane == 0) i = atomicAdd(&s_next, 1u);
      i = (u32)__builtin_amdgcn_readfirstlane((int)i);
      if (i >= (u32)__builtin_amdgcn_readfirstlane((int)s_hdr[1])) break;
      // The parameters a task needs only on its way into the window loop are read again from the kernel's argument
      // segment, task by task (scalar loads that hit the constant cache).  Read once at the kernel's start they would
      // have to stay in scalar registers across the loop over the tasks, and the window loop paid for them in spills.
      typedef const __attribute__((address_space(4))) unsigned char* kargp;
      kargp kq = (kargp)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(kq));
      Dp4Params Pj = P;                 // (a member that is not listed below stays the kernel's own copy: right, only dearer)
#define D5_KARG(F) Pj.F = *reinterpret_cast<const __attribute__((address_space(4))) decltype(Dp4Params::F)*>(kq + offsetof(Dp4Params, F));
      D5_KARG(blocks) D5_KARG(dph) D5_KARG(cost) D5_KARG(mincost) D5_KARG(codes) D5_KARG(code_base) D5_KARG(la) D5_KARG(prof)
      D5_KARG(badpos) D5_KARG(entry) D5_KARG(exit) D5_KARG(mid) D5_KARG(wmax) D5_KARG(tiemask) D5_KARG(wmeta) D5_KARG(winroff)
      D5_KARG(winflag) D5_KARG(win_off) D5_KARG(over) D5_KARG(int_path) D5_KARG(chain_fast) D5_KARG(debug) D5_KARG(flags)
#undef D5_KARG
      const Dp4Params& P = Pj;
      const u32 b0 = (u32)__builtin_amdgcn_readfirstlane((int)s_hdr[0]);
      const BlockDesc bd = P.blocks[b0];
      const u32 B = (u32)(bd.inend - bd.instart);
      D5IntTab IT;
      IT.on = __builtin_amdgcn_readfirstlane((int)s_hdr[2]) != 0;
      IT.lo = (u32)__builtin_amdgcn_readfirstlane((int)s_hdr[3]);
      {
        const u32 rm = (u32)__builtin_amdgcn_readfirstlane((int)s_rmax);
        IT.span = !IT.on ? 0u : rm < 0x100000u ? 33u * rm : 0x40000000u;
      }
      const u32 t = (u32)__builtin_amdgcn_readfirstlane((int)s_tid[i]);
      SegTask T;
      T.block = b0;
      T.q = (u32)__builtin_amdgcn_readfirstlane((int)s_task[i].q);
      T.pout = (u32)__builtin_amdgcn_readfirstlane((int)s_task[i].pout);
      T.pend = (u32)__builtin_amdgcn_readfirstlane((int)s_task[i].pend);
      D4Job J;
      D5_SPEC_JOB(J, P, t, T, B)
      if (T.pout == 0) {       // the head of the block
        J.spec = false;
        J.la_lo = 1;
        J.level = 0.0f;
      } else {
        J.spec = true;
        J.la_lo = SEG_NONE;
        J.level = __uint_as_float((u32)__builtin_amdgcn_readfirstlane((int)__float_as_uint(s_lvl[i])));
      }
      if (PROF && P.prof && first_job && lane == 0) d5_prof_setup_done(P, b0, t_wg0);
      first_job = false;
      d5_run_job<PROF, RUNS>(P, J, b0, bd, s_wtab, reinterpret_cast<float*>(s_buf[wave]), reinterpret_cast<u16*>(s_buf[wave] + 4u * DP_XN),
                       reinterpret_cast<u16*>(s_buf[wave]), s_itab, IT, s_w1, s_sym1, s_ri[wave], s_rk[RUNS ? wave : 0u]);
      // the wave's staging area, s_ri and s_rk are the next job's: nothing of this one — LDS-DMA, stores, LDS reads — is
      // still on its way
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    if (PROF && P.prof && lane == 0) d5_prof_wave_done(P, b0, t_wg0, s_pf_sum, s_pf_max, s_pf_done);
    if (!P.redo_pass) return;
    __syncthreads();     // the tables in LDS are the next entry's
  }
}
