// Device layer of libzopfli_amd.so (C ABI part 2 of include/zopfli_amd.h): HBM residency, launch orchestration and the
// parity probes.  gfx950 only; there is no host fallback — every entry point reports an error if the device or a launch
// fails.  One translation unit, and this file is its table of contents: the kernel headers (zmx_*.h), then the parts of
// the host-side driver (drv_*.h) in dependency order.  A part says in its first lines what it needs from those before it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../host/zmx_internal.h"   // the seam to the host layer; its statistics slots are k_wtab's and k_dp4_fix's too

// ---- the kernels (the order is the order of the code object)
#include "zmx_kernels.h"     // types, BlockDesc, hash links, rows, codes, record copies, verify
#include "zmx_match2.h"      // k_match2: the match table, a lane per position
#include "zmx_match5.h"      // k_match5: the exact skip-walk for long chains
#include "zmx_dp4.h"         // the chain's tasks: snapshots, the four-wave job, k_dpcheck, k_dprecheck, k_dpscan
#include "zmx_dp_build.h"    // once per table set: k_mkdesc (window records), k_cutpoints, k_taskkind
#include "zmx_dp5.h"         // d5_run_job: a task walked by one wave, the integer chain step
#include "zmx_dp5_spec.h"    // k_dp5_spec, k_dp5_stretch: the speculative pass, and the set-up the two share
#include "zmx_dp4_fix.h"     // k_dp4_fix: the serial pass, which runs the jobs of zmx_dp4.h and zmx_dp5.h
#include "zmx_encode.h"      // the bit writer
#include "zmx_checksum.h"    // CRC-32 / Adler-32 pieces
#define ZMX_CHECKSUM_DEVICE_KERNELS
#include "zmx_checksum_device.h"   // ... of any device memory, finished on the device
#define ZMX_INFLATE_KERNELS
#include "zmx_inflate.h"     // k_inflate: deflate, zlib and gzip streams decoded, a wave a stream
#define ZMX_PNG_DECODE_KERNELS
#include "zmx_png_decode.h"  // k_png_chunks, k_png_unfilter: a PNG's chunks walked, its scanlines unfiltered, a wave an image
#include "zmx_trace.h"       // the walk back over length_array, in segments
#include "zmx_greedy.h"      // the greedy parse, same segmentation
#include "zmx_png.h"         // LodePNG's MINSUM / ENTROPY filter choice
#include "zmx_png_brute.h"   // LodePNG's brute-force filter choice
#include "zmx_blockcost.h"   // block sizes of ranges of symbol sequences
#define ZMX_PROBE_KERNELS
#include "zmx_probe.h"       // probe counts, tail runs, the record digest
#define ZMX_GATHER_KERNELS
#include "zmx_gather.h"      // many device buffers end to end
#define ZMX_BITJOIN_KERNELS
#include "zmx_bitjoin.h"     // many bit strings joined into one
#define ZMX_PNG_ROWS_KERNELS
#include "zmx_png_rows.h"    // the filtered scanlines of a PNG
#define ZMX_PNG_COLOR_KERNELS
#include "zmx_png_color.h"   // LodePNG's colour statistics and colour conversion
#define ZMX_PNG_INDEX_KERNELS
#include "zmx_png_index.h"   // index images: where each value first appears, the table-driven conversion
#define ZMX_PNG_PACK_KERNELS
#include "zmx_png_pack.h"    // strided, planar, typed sources into PNG byte order, n of them in one launch
#define ZMX_PNG_UNPACK_KERNELS
#include "zmx_png_unpack.h"  // own-mode pixels into strided, planar, typed sinks, n of them in one launch
#define ZMX_PNG_LOSSY_KERNELS
#include "zmx_png_lossy.h"   // zopflipng's --lossy_transparent: statistics, the carry scan, the rewrite
#define ZMX_PNG_LODEFLATE_KERNELS
#include "zmx_png_lodeflate.h"   // LodePNG's own deflate, sized: hash, links over tiles, search, the lazy parse per block
#include "zmx_knobs.h"       // the ZOPFLI_AMD_* switches
#include "zopfli_amd.h"
#include "../host/deal.h"
#include "../host/entry_checks.h"
#include "../host/inflate_plan.h"
#include "../host/png_decode_plan.h"
#include "../host/png_color_choose.h"
#include "../host/png_index.h"
#include "../host/png_brute_launch.h"
#include "../host/png_lodeflate_size.h"
#include "../host/png_source.h"
#include "../host/png_sink.h"
#include "../host/symbol_check.h"
#include "../host/thread_pool.h"

// ---- the driver
#include "drv_errors.h"      // the thread's error state, HIPCHK, KCHK, DeviceGuard and DEVICE_ENTRY
#include "zmx_pool.h"        // DevicePool: a context's device memory and pinned buffers (and k_guard_check)
#include "drv_context.h"     // zmx_ctx, PoolScope and its Upload, create / destroy / priority, the process-wide setters
#include "drv_input.h"       // the resident input, device-pointer checks, the seam to the host layer, probe counts, the gather
#include "drv_tables.h"      // RunLayout, TableParams, zmx_tables, free / trim, the entry checks' adapters
#include "drv_build.h"       // BuildTables phase by phase and the three build entries
#include "drv_squeeze.h"     // the greedy pass, RunInfo, the squeeze run, the trace test entry
#include "drv_stores.h"      // store download, verify, encode
#include "drv_bitjoin.h"     // output that stays on the device: the bit join, the bit writer without the way down
#include "drv_checksum.h"    // zmx_checksum, zmx_checksums
#include "drv_checksum_device.h"   // zmx_checksum_device, the seal of a PNG left in device memory
#include "drv_inflate.h"     // k_inflate's launch, zmx_inflate_device_ctx
#include "drv_png_unpack.h"  // zmx_png_unpack_device; the sinks' checks and k_png_unpack's launch
#include "drv_png_decode.h"  // the PNG decode: the run every entry shares, zmx_png_decode_device_ctx, zmx_png_decode_sink_device_ctx
#include "drv_png.h"         // the PNG entries: row searches on host and device images, the filtered scanlines, colour statistics and conversion, index images, LodePNG's zlib sizes
#include "drv_png_pack.h"    // zmx_png_pack_device
#include "drv_blockcost.h"   // zmx_cost_stores and its five entries
#include "drv_probes.h"      // the parity probes: digest, longest match, hash links, length array, DP rows
