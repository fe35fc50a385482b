// The ZOPFLI_AMD_* switches of the device layer (the driver parts drv_*.h that zmx_hip.hip lists), in one place: what
// each is, how its text is read, and the process-wide instance.  Host only — no HIP here, so that tests/hostlib/knob_print.cc compiles it with plain g++.  The
// switches of the host layer (api.cc, deflate.cc, block_split.cc, block_cache.h, thread_pool.h) are host/host_knobs.h.
#pragma once

#include <algorithm>
#include <cstdlib>

namespace zamd {

struct DeviceKnobs {
  bool guard = false;            // ZOPFLI_AMD_GUARD: red zones around every device allocation, checked after every launch
  unsigned long long guard_selftest = 0;   // ZOPFLI_AMD_GUARD_SELFTEST=N: the N-th check finds a byte the check itself broke
  bool prof = false;             // ZOPFLI_AMD_PROF (set at all): profiling instantiations of the kernels, reports on stderr
  bool kernel_timing = false;    // ZOPFLI_AMD_KERNEL_TIMING: a squeeze run's phase times; unset = whether PROF is set
  bool bc_prof = false;          // ZOPFLI_AMD_BC_PROF (set at all): k_block_cost's phases per launch on stderr
  int match = 0;                 // ZOPFLI_AMD_MATCH: 0 = k_match5 or k_match2 per block, 5 = k_match5, anything else (the removed 3 and 4 too) = 2
  bool match_order = true;       // ZOPFLI_AMD_MATCH_ORDER: k_match2 hands out a tile's positions longest walk first
  bool match_filter = true;      // ZOPFLI_AMD_MATCH_FILTER: k_match2's four-byte candidate filter; 0 keeps the one-byte test
  unsigned long long match_hits = 300;     // ZOPFLI_AMD_MATCH_HITS: kernel 0, blocks whose estimated hits per position exceed this take k_match5
  unsigned long long pool_entries = 0;     // ZOPFLI_AMD_POOL_ENTRIES: test hook, entries of the first change-point pool (0 = by the input)
  bool run_codes = false;        // ZOPFLI_AMD_RUN_CODES: codes for every DP row (the serial chain needs them)
  unsigned long long code_budget_mb = 0;   // ZOPFLI_AMD_CODE_BUDGET_MB: what the codes of one batch may take (0 = the context's budget)
  bool seg_l_set = false;        // ZOPFLI_AMD_SEG_L is set: seg_l holds, whatever the size of the batch
  unsigned seg_l = 4096;         // ZOPFLI_AMD_SEG_L: positions per chain task, a multiple of 64; 0 = no tasks, the serial chain
  unsigned seg_head = 0;         // ZOPFLI_AMD_SEG_HEAD: the exact head of a block, a multiple of 64; 0 = by the number of blocks
  unsigned seg_warm = 512;       // ZOPFLI_AMD_SEG_WARM: warm-up positions before a task, rounded up to 64, 64 .. 2^20
  unsigned seg_cuts = 1024;      // ZOPFLI_AMD_SEG_CUTS: how far before a task k_cutpoints looks for a cut point; 0 = every task warms up
  bool seg_mid = true;           // ZOPFLI_AMD_SEG_MID: 0 = no mid snapshots (tasks that leave their binade are re-run whole)
  unsigned seg_stretch = 4;      // ZOPFLI_AMD_SEG_STRETCH: tasks of one block per workgroup of the speculative pass, 1 .. 32; up to 4 a task a wave (k_dp5_spec), beyond the waves pull them (k_dp5_stretch)
  bool seg_pull = false;         // ZOPFLI_AMD_SEG_PULL: 1 = k_dp5_stretch runs the main pass at stretches of 4 and fewer too (A/B, test hook)
  int seg_redo = 1;              // ZOPFLI_AMD_SEG_REDO: second speculative passes for tasks that only missed their level
  float seg_scale = 1.0f;        // ZOPFLI_AMD_SEG_SCALE: scale of the tasks' level estimates (test hook: wrong binades)
  int seg_debug = 0;             // ZOPFLI_AMD_SEG_DEBUG: per-task trace of the chain kernels
  int fix_lean = -1;             // ZOPFLI_AMD_FIX_LEAN: 0 = every serial re-run by the lean one-wave job, large = none, unset = by the task's windows
  int int_path = 1;              // ZOPFLI_AMD_INT_PATH: 0 = every window in the reference's doubles
  int shortcut_chain = 1;        // ZOPFLI_AMD_SHORTCUT_CHAIN: 0 = long-run shortcuts window by window
};

// `get` is getenv or a stand-in for it: const char* get(const char* name), null when the variable is not set.
template <typename GetEnv>
DeviceKnobs ParseDeviceKnobs(GetEnv get) {
  auto clamped = [&](const char* name, unsigned dflt, unsigned lo, unsigned hi) {
    const char* e = get(name);
    if (!e) return dflt;
    const long v = std::atol(e);
    return v < static_cast<long>(lo) ? lo : v > static_cast<long>(hi) ? hi : static_cast<unsigned>(v);
  };
  auto integer = [&](const char* name, int dflt) { const char* e = get(name); return e ? std::atoi(e) : dflt; };
  auto on = [&](const char* name, bool dflt) { const char* e = get(name); return e ? std::atoi(e) != 0 : dflt; };
  auto count = [&](const char* name) { const char* e = get(name); return e ? static_cast<unsigned long long>(std::atoll(e)) : 0ull; };
  DeviceKnobs k;
  k.guard = on("ZOPFLI_AMD_GUARD", false);
  k.guard_selftest = count("ZOPFLI_AMD_GUARD_SELFTEST");
  k.prof = get("ZOPFLI_AMD_PROF") != nullptr;
  k.kernel_timing = on("ZOPFLI_AMD_KERNEL_TIMING", k.prof);
  k.bc_prof = get("ZOPFLI_AMD_BC_PROF") != nullptr;
  const int match = integer("ZOPFLI_AMD_MATCH", 0);
  k.match = match == 0 || match == 5 ? match : 2;
  k.match_order = on("ZOPFLI_AMD_MATCH_ORDER", true);
  k.match_filter = on("ZOPFLI_AMD_MATCH_FILTER", true);
  if (const char* e = get("ZOPFLI_AMD_MATCH_HITS")) k.match_hits = static_cast<unsigned long long>(std::max<long>(0, std::atol(e)));
  k.pool_entries = count("ZOPFLI_AMD_POOL_ENTRIES");
  k.run_codes = on("ZOPFLI_AMD_RUN_CODES", false);
  if (const char* e = get("ZOPFLI_AMD_CODE_BUDGET_MB")) k.code_budget_mb = static_cast<unsigned long long>(std::max<long>(1, std::atol(e)));
  k.seg_l_set = get("ZOPFLI_AMD_SEG_L") != nullptr;
  k.seg_l = clamped("ZOPFLI_AMD_SEG_L", 4096, 0, 1u << 24) & ~63u;
  k.seg_head = clamped("ZOPFLI_AMD_SEG_HEAD", 0, 0, 1u << 24) & ~63u;
  k.seg_warm = (clamped("ZOPFLI_AMD_SEG_WARM", 512, 64, 1u << 20) + 63u) & ~63u;
  k.seg_cuts = clamped("ZOPFLI_AMD_SEG_CUTS", 1024, 0, 1u << 16);
  k.seg_mid = clamped("ZOPFLI_AMD_SEG_MID", 1, 0, 1) != 0;
  k.seg_stretch = clamped("ZOPFLI_AMD_SEG_STRETCH", 4, 1, 32);
  k.seg_pull = on("ZOPFLI_AMD_SEG_PULL", false);
  k.seg_redo = integer("ZOPFLI_AMD_SEG_REDO", 1);
  if (const char* e = get("ZOPFLI_AMD_SEG_SCALE")) k.seg_scale = static_cast<float>(std::atof(e));
  k.seg_debug = integer("ZOPFLI_AMD_SEG_DEBUG", 0);
  k.fix_lean = integer("ZOPFLI_AMD_FIX_LEAN", -1);
  k.int_path = integer("ZOPFLI_AMD_INT_PATH", 1);
  k.shortcut_chain = integer("ZOPFLI_AMD_SHORTCUT_CHAIN", 1);
  return k;
}

// The process's switches, read from the environment at the first use of the device layer.
inline const DeviceKnobs& Knobs() {
  static const DeviceKnobs k = ParseDeviceKnobs([](const char* name) -> const char* { return std::getenv(name); });
  return k;
}

}  // namespace zamd
