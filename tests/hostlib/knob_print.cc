// TEST-ONLY: prints the device layer's switches (zopfli_amd/csrc/device/zmx_knobs.h) as parsed from this process's
// environment, one "field=value" line each.  tests/test_cpu_knobs.py sets the environment and reads the lines.
#include <cstdio>
#include <cstdlib>

#include "zmx_knobs.h"

int main() {
  const zamd::DeviceKnobs k = zamd::ParseDeviceKnobs([](const char* name) -> const char* { return std::getenv(name); });
  std::printf("guard=%d\n", k.guard ? 1 : 0);
  std::printf("guard_selftest=%llu\n", k.guard_selftest);
  std::printf("prof=%d\n", k.prof ? 1 : 0);
  std::printf("kernel_timing=%d\n", k.kernel_timing ? 1 : 0);
  std::printf("bc_prof=%d\n", k.bc_prof ? 1 : 0);
  std::printf("match=%d\n", k.match);
  std::printf("match_order=%d\n", k.match_order ? 1 : 0);
  std::printf("match_filter=%d\n", k.match_filter ? 1 : 0);
  std::printf("match_hits=%llu\n", k.match_hits);
  std::printf("pool_entries=%llu\n", k.pool_entries);
  std::printf("run_codes=%d\n", k.run_codes ? 1 : 0);
  std::printf("code_budget_mb=%llu\n", k.code_budget_mb);
  std::printf("seg_l_set=%d\n", k.seg_l_set ? 1 : 0);
  std::printf("seg_l=%u\n", k.seg_l);
  std::printf("seg_head=%u\n", k.seg_head);
  std::printf("seg_warm=%u\n", k.seg_warm);
  std::printf("seg_cuts=%u\n", k.seg_cuts);
  std::printf("seg_mid=%d\n", k.seg_mid ? 1 : 0);
  std::printf("seg_redo=%d\n", k.seg_redo);
  std::printf("seg_scale=%.9g\n", static_cast<double>(k.seg_scale));
  std::printf("seg_debug=%d\n", k.seg_debug);
  std::printf("fix_lean=%d\n", k.fix_lean);
  std::printf("int_path=%d\n", k.int_path);
  std::printf("shortcut_chain=%d\n", k.shortcut_chain);
  return 0;
}
