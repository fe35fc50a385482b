// TEST-ONLY: prints the switches as parsed from this process's environment, one "field=value" line each: the device layer's
// (zopfli_amd/csrc/device/zmx_knobs.h) with no argument, the host layer's process table with "host", its pool table for N
// visible devices with "pool N" (zopfli_amd/csrc/host/host_knobs.h).  tests/test_cpu_knobs.py sets the environment and
// reads the lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_knobs.h"
#include "zmx_knobs.h"

namespace {

const char* Env(const char* name) { return std::getenv(name); }

int PrintHost() {
  const zamd::HostKnobs k = zamd::ParseHostKnobs(Env);
  std::printf("split_mb=%ld\n", k.split_mb);
  std::printf("split_ways=%zu\n", k.split_ways);
  std::printf("split_runs=%d\n", k.split_runs ? 1 : 0);
  std::printf("stream_prio=%d\n", k.stream_prio);
  std::printf("small_prio=%d\n", k.small_prio ? 1 : 0);
  std::printf("upload_order=%d\n", k.upload_order ? 1 : 0);
  std::printf("deal_by_cost=%d\n", k.deal_by_cost ? 1 : 0);
  std::printf("shard_weights=");
  for (size_t i = 0; i < k.shard_weights.size(); ++i) std::printf(i ? ",%g" : "%g", k.shard_weights[i]);
  std::printf("\n");
  std::printf("deal_after=%zu\n", k.deal_after);
  std::printf("round_parts=%zu\n", k.round_parts);
  std::printf("parts_per_batch=%zu\n", k.parts_per_batch);
  std::printf("test_fail_shard=%ld\n", k.test_fail_shard);
  std::printf("keep_heap=%d\n", k.keep_heap);
  std::printf("batch_split=%d\n", k.batch_split);
  std::printf("device_split=%d\n", k.device_split);
  std::printf("device_split_from=%ld\n", k.device_split_from);
  std::printf("device_split_min=%zu\n", k.device_split_min);
  std::printf("device_encode=%d\n", k.device_encode ? 1 : 0);
  std::printf("verify=%d\n", k.verify ? 1 : 0);
  std::printf("trace_call=%d\n", k.trace_call ? 1 : 0);
  std::printf("prof=%d\n", k.prof ? 1 : 0);
  std::printf("threads=%u\n", k.threads);
  std::printf("threads_set=%d\n", k.threads_set ? 1 : 0);
  std::printf("wide_threads=%u\n", k.wide_threads);
  std::printf("host_cache_mb=%zu\n", k.host_cache_mb);
  std::printf("host_cache_min=%zu\n", k.host_cache_min);
  return 0;
}

int PrintPool(int visible) {
  const zamd::PoolKnobs k = zamd::ParsePoolKnobs(Env, visible);
  std::printf("devices=");
  for (size_t i = 0; i < k.devices.size(); ++i) std::printf(i ? ",%d" : "%d", k.devices[i]);
  std::printf("\n");
  std::printf("lanes=%zu\n", k.lanes);
  std::printf("small_lanes=%zu\n", k.small_lanes);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return PrintHost();
  if (argc > 2 && std::strcmp(argv[1], "pool") == 0) return PrintPool(std::atoi(argv[2]));
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
