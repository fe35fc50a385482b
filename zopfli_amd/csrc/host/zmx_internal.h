// The seam between the host layer (csrc/host/*.cc) and the device layer (csrc/device/zmx_hip.hip, which
// lists its parts: the definitions are in drv_input.h and drv_squeeze.h) that is no part of
// the public ABI (include/zopfli_amd.h), declared ONCE.  Host to device: every zmx_internal_* function.  The device
// layer defines them and includes this header, as every caller does and as the host test library's stand-in for the
// device layer does (tests/hostlib/zmx_oracle_backend.cc), so a parameter list that changes on one side only does not
// compile.  Device to host: the statistics, which the host layer owns.
// The library is built with -fvisibility=hidden, so all this stays inside it; ZMX_INTERNAL_EXPORT marks the
// functions that tests and tools reach from outside (here and nowhere else).
#pragma once
#include <cstddef>
#include <cstdint>

#include "zopfli_amd.h"

#define ZMX_INTERNAL_EXPORT __attribute__((visibility("default")))

// How the chain's tasks of a run fared, by slot: what k_dp4_fix adds up on the device (RunLayout::kStats words of the
// run's output), what zmx_stats::seg sums per thread and what zmx_last_seg_stats hands out, in the order of the keys of
// zopfli_amd/api.py (SEG_STAT_KEYS; tests/test_cpu_abi.py holds the two against each other).
// The last slot is two things.  On the DEVICE it is ZMX_SEG_DEV_LEAN, the serial re-runs the lean one-wave job took:
// ReportSqueezeProf reads that, from the run's own words.  On the HOST it is ZMX_SEG_POSITIONS, the positions of the
// run's blocks, which zmx_squeeze_run puts there in the device's count's place: AddStats, zmx_last_seg_stats and
// api.py read that.
enum zmx_seg_stat {
  ZMX_SEG_TASKS,            // tasks of the run's blocks, heads included
  ZMX_SEG_ACCEPTED,         // accepted as the speculative pass left them
  ZMX_SEG_RERUN_STATE,      // run again serially: the entry state was not the predecessor's exit state
  ZMX_SEG_RERUN_LEVEL,      // ... the shift takes the task out of its binade
  ZMX_SEG_RERUN_TIE,        // ... a weight can tie in the task's binade
  ZMX_SEG_POSITIONS_RERUN,  // positions of the tasks run again
  ZMX_SEG_RERUN_VALUES,     // run again: same structure, other values
  ZMX_SEG_POSITIONS,        // (host) positions in the blocks
  ZMX_SEG_N,
  ZMX_SEG_DEV_LEAN = ZMX_SEG_POSITIONS   // (device) re-runs by the lean one-wave job
};

// Kernel, match and task statistics, summed per calling THREAD since the start of its call.  Only the host layer
// reads, takes and adds them (api.cc: zmx_last_*, and a call's shard threads hand theirs to the caller's at the join),
// so it owns them, as it owns zamd::ThreadTiming; the device layer adds to them where it times its kernels.
struct zmx_stats {
  double kernel_seconds[3];  // k_wtab + k_badscan, chain kernels (k_dp5_spec + k_dp5_stretch + k_dpcheck + k_dprecheck + k_dpscan + k_dp4_fix), k_trace (HIP events)
  double squeeze_launches;
  double match5[3];          // k_match5: entries in flight summed over lanes and iterations, wave iterations, positions it walked
  double match[4];           // match kernel seconds, k_same + k_chain (+ k_levels ...) seconds, table builds, positions matched
  double seg[ZMX_SEG_N];     // by zmx_seg_stat, the host's reading of the last slot
};
namespace zamd {
struct InflateJob;          // (device/zmx_inflate.h)
zmx_stats& ThreadStats();   // the calling thread's (thread-local: no lock)
// The positions the call in progress on this thread has on its device in all, 0 = no more than the table set at hand:
// set around a dealt call's shard (api.cc: RunShard), read where a table set picks its task length (drv_build.h: SegL).
unsigned long long& CallPositions();
}

extern "C" {

// ---- errors
// Makes `msg` the calling thread's last error (zmx_last_error) and `cls` its class (zmx_last_error_class, a ZMX_ERR_*).
void zmx_internal_set_error(const char* msg, int cls);

// ---- a context and its resident input
// The HIP device the context runs on.
int zmx_internal_device(zmx_ctx* ctx);
// The size of the resident input in bytes.
size_t zmx_internal_input_size(zmx_ctx* ctx);
// The caller's host copy of the resident input (borrowed until the next zmx_set_input); null when the input came from
// device memory (zmx_set_input_device).
const unsigned char* zmx_internal_input_host(zmx_ctx* ctx);
// Bytes [begin, end) of the resident input, device to host (the bytes of a stored block when the input came from device
// memory: the host has no copy of its own).  0, or -1 with the error set (ZMX_ERR_REFUSED: a range outside the input).
int zmx_internal_input_fetch(zmx_ctx* ctx, size_t begin, size_t end, unsigned char* dst);
// k_probe_counts over n <= 65535 ranges (begin, end) of `bytes` — device memory of the context's device; null: the
// resident input —, the caller having checked the ranges against it: counts[r][zamd::kProbeCounts].  0, or -1 with the
// error set.
int zmx_internal_probe_counts(zmx_ctx* ctx, const void* bytes, size_t n, const uint64_t* ranges, uint32_t* counts);
// The context's memory pool in numbers (DevicePool::Stats says which); reads only.
ZMX_INTERNAL_EXPORT void zmx_internal_pool_stats(zmx_ctx* ctx, uint64_t out[8]);

// ---- device memory that is no context's
// 0 when [p, p + n) is plain device memory, with its HIP device in *device; else -1 with the error set
// (ZMX_ERR_REFUSED, the message starts with `who`).
int zmx_internal_device_pointer(const char* who, const void* p, size_t n, int* device);
// The same for n ranges [p[i], p[i] + nbytes[i]), before anything is done with any of them (zmx_compress_device_batch).
int zmx_internal_device_pointers(const char* who, size_t n, const void* const* p, const size_t* nbytes);
// A plain allocation of `device` that its caller owns (the staging buffer of zmx_compress_device_batch: it outlives the
// context it was filled on, which goes back to the pool while the shards copy from it).  0, or -1 with the error set.
int zmx_internal_device_alloc(int device, size_t n, void** p);
// Frees what zmx_internal_device_alloc gave (null: nothing).
void zmx_internal_device_free(int device, void* p);
// n bytes from d_src to d_dst, both plain memory of `device` that the caller has checked; done when it returns.  0, or -1
// with the error set.
int zmx_internal_device_copy(int device, void* d_dst, const void* d_src, size_t n);

// ---- output that stays in device memory
// zmx_bitjoin_device(ctx, n, pieces, total_bits, d_dst, dst_capacity) whose pieces with is_literal[i] != 0 come from
// `literals`: their src holds the byte offset in that buffer, which is uploaded once into memory of the context for the
// time of the join.  `pieces` is rewritten.  0, or -1 with the error set.
int zmx_internal_bitjoin_literals(zmx_ctx* ctx, const unsigned char* literals, size_t nliterals, size_t n, zmx_bit_piece* pieces,
                                  const unsigned char* is_literal, uint64_t total_bits, void* d_dst, size_t dst_capacity);
// The same for zmx_bitjoin_many_device(ctx, ndst, dests, capacity, npieces, pieces): one literals buffer for the pieces of
// all destinations (zmx_compress_device_batch_to_device, batch.cc).
int zmx_internal_bitjoin_many_literals(zmx_ctx* ctx, const unsigned char* literals, size_t nliterals, size_t ndst, const zmx_bit_dest* dests,
                                       const size_t* capacity, size_t npieces, zmx_bit_piece* pieces, const unsigned char* is_literal);
// zmx_internal_device_pointers for ranges that must lie on ONE device (the destinations of a batch): *device is that
// device, -1 when every range is empty.  Refused (the message starts with `who` and names the range): what
// zmx_internal_device_pointer refuses of any of them, and a range on another device than the ones before it.
int zmx_internal_device_pointers_one_device(const char* who, size_t n, const void* const* p, const size_t* nbytes, int* device);

// zmx_checksum_device(ctx, kind, n, d_ptr, nbytes, ...) over ranges the caller has checked, whose value i goes to the four
// bytes at d_seal[i], most significant first, instead of the host: the IDAT's CRC-32 of a PNG left in device memory
// (device_output.cc, batch.cc).  Two launches for all n, nothing comes down.  0, or -1 with the error set.
int zmx_internal_checksum_seal(zmx_ctx* ctx, int kind, size_t n, const void* const* d_ptr, const size_t* nbytes, unsigned char* const* d_seal);

// ---- inflate on the device (inflate.cc)
// k_inflate over n <= zamd::kInflateRoundJobs jobs (device/zmx_inflate.h, in the order they are to start) whose ranges the
// caller has checked: memory of the context's device.  results[jobs[k].index] is job k's.  One launch; 32 n bytes come
// down.  0, or -1 with the error set (a device failure: a stream's status is no error of the run).
int zmx_internal_inflate_run(zmx_ctx* ctx, int format, size_t n, const zamd::InflateJob* jobs, zmx_inflate_result* results);

// ---- PNG decode on the device (png_decode.cc)
// The whole decode of n <= 2^24 files whose ranges the caller has checked — memory of the context's device, the destinations
// apart from the files and from each other —: k_png_chunks, the chunks' CRC-32s, the gather of split IDATs, k_inflate, the
// Adler-32s, k_png_unfilter (device/drv_png_decode.h says what comes down).  info_only: the walk and the CRCs alone.
// `hooks` may be null.  Every result is filled in; 0, or -1 with the error set, its message starting with `who` (a device
// failure or a refusal: a file's status is no error of the run).
int zmx_internal_png_decode_run(zmx_ctx* ctx, const char* who, int mode, int info_only, size_t n, const void* const* d_file,
                                const size_t* filesize, void* const* d_out, const size_t* capacity, zmx_png_decode_result* results,
                                const zmx_png_decode_hooks* hooks);

// The same into sinks (include/zopfli_amd.h: zmx_png_sink): the sinks are checked here — each one, its extent against the
// runtime, against the other sinks and against the files —, a file whose size is not its sink's ends ZMX_PNG_DECODE_SHAPE
// before its stream is read, and one k_png_unpack launch stores every file that ended OK.
int zmx_internal_png_decode_sink_run(zmx_ctx* ctx, const char* who, size_t n, const void* const* d_file, const size_t* filesize,
                                     const zmx_png_sink* sinks, zmx_png_decode_result* results, const zmx_png_decode_hooks* hooks);

// ---- a PNG from an image in device memory (png_encode.cc)
// The filter types of `strategy` (a ZMX_PNG_FILTER_*; _BRUTE with window `windowsize`; _PREDEFINED: the `height` host
// bytes at `predefined`, each at most 4) and then the filtered scanlines of d_image (zmx_png_filter_rows_device) into
// d_out: height * (linebytes + 1) bytes of the context's device that the caller owns.  The image is checked as
// zmx_png_filter_rows_device checks its own.  0, or -1 with the error set.
int zmx_internal_png_scanlines(zmx_ctx* ctx, const void* d_image, size_t linebytes, size_t height, size_t bytewidth, int strategy,
                               unsigned windowsize, const unsigned char* predefined, void* d_out);

// ---- a PNG with its colour mode reduced (png_encode.cc: zmx_png_optimize_device)
// zmx_internal_png_scanlines of the image converted to `mode` first (zmx_png_convert_device, into memory of the context's
// pool); a null `mode`: of the image as it is.  d_out: height * ((width * bpp + 7) / 8 + 1) bytes of the context's device
// that the caller owns.  0, or -1 with the error set.
int zmx_internal_png_reduced_scanlines(zmx_ctx* ctx, const zmx_png_image* image, const zmx_png_color_mode* mode, int strategy,
                                       unsigned windowsize, const unsigned char* predefined, void* d_out);

// ---- zopflipng's lossy options in front of the two (png_encode.cc: the _lossy entries)
// What the entries encode instead of `image`: with `to8` (a 16-bit image) its 8-bit image in the same colour type
// (k_png_convert), with `transparent` zmx_png_lossy_transparent_device's rewrite of that, or of the image itself — both into
// d_buf, height * width * channels * (to8 ? 1 : bitdepth / 8) bytes of the context's device that the caller owns.  *work
// is `image` with the pointer and the depth of what was made; where nothing had to be rewritten (no transparent pixel) it
// still points at the caller's pixels.  The image is checked as zmx_png_color_stats_device checks its own.  0, or -1 with
// the error set, its message starting with `who`, the entry's name.
int zmx_internal_png_lossy_image(zmx_ctx* ctx, const char* who, const zmx_png_image* image, int to8, int transparent, void* d_buf,
                                 zmx_png_image* work);

// ---- zopflipng's filter-strategy trials (png_encode.cc: zmx_png_choose_strategy_device, ZMX_PNG_FILTER_AUTO)
// The scanlines of trial k = 0 .. ntrials - 1 of an image that lies converted at d_rows (`height` rows of `rowbytes` bytes,
// `bytewidth` the distance to the left neighbour) at d_out + k * height * (rowbytes + 1), in zopflipng's order: the types
// 0 .. 4, MINSUM, ENTROPY and, for ntrials = 8, the `height` host bytes at `predefined`, each at most 4.  Both are memory of
// the context's device; d_out the caller owns.  0, or -1 with the error set, its message starting with `who`.
int zmx_internal_png_trial_scanlines(zmx_ctx* ctx, const char* who, const void* d_rows, size_t rowbytes, size_t height, size_t bytewidth,
                                     const unsigned char* predefined, int ntrials, void* d_out);

// ---- strided, planar and typed sources in front of the PNG entries (png_encode.cc: the _source entries)
// zmx_png_pack_device(ctx, n, sources, d_out, capacity) whose refusals begin with `who`, the entry's name.
int zmx_internal_png_pack(zmx_ctx* ctx, const char* who, size_t n, const zmx_png_source* sources, void* const* d_out, const size_t* capacity);

// ---- for tests and tools
// The copies of the calling thread's last zmx_gather_device — k_gather and the other devices' pieces — in milliseconds
// (HIP events on the context's stream), taken while kernel timing is on (zmx_set_kernel_timing); else 0.  For
// tools/batch_files.py --device.
ZMX_INTERNAL_EXPORT double zmx_internal_gather_ms(void);
// The same for the calling thread's last zmx_bitjoin_device: k_bitjoin alone.  For tools/device_output.py.
ZMX_INTERNAL_EXPORT double zmx_internal_bitjoin_ms(void);
// The same for k_png_rows of the calling thread's last zmx_png_filter_rows_device.  For tools/png_device.py.
ZMX_INTERNAL_EXPORT double zmx_internal_png_rows_ms(void);
// The same for the calling thread's last zmx_png_color_stats_device and zmx_png_convert_device: k_png_color_stats,
// k_png_color_key (0: not launched), k_png_convert.  For tools/png_reduce.py.
ZMX_INTERNAL_EXPORT void zmx_internal_png_color_ms(double out[3]);
// The same for the calling thread's last zmx_png_lossy_transparent_device: k_png_lossy_stats, k_png_lossy_carry,
// k_png_lossy_fill (0: not launched).  For tools/png_lossy.py.
ZMX_INTERNAL_EXPORT void zmx_internal_png_lossy_ms(double out[3]);
// The same for the calling thread's last zmx_png_index_use_device and zmx_png_index_convert_device: k_png_index_use,
// k_png_index_convert.  For tools/png_index.py.
ZMX_INTERNAL_EXPORT void zmx_internal_png_index_ms(double out[2]);
// The same for the calling thread's last zmx_png_deflate_sizes_device: k_png_lo_hash, k_png_lo_links, k_png_lo_ask,
// k_png_lo_keep, k_png_lo_search, k_png_lo_parse.  For tools/png_auto.py.
ZMX_INTERNAL_EXPORT void zmx_internal_png_lodeflate_ms(double out[6]);
// Test hook (tests/test_gpu_png_lodeflate_seams.py): zmx_png_deflate_sizes_device with the same checks, in tiles of
// `tile_len` positions (0: the device's own, kLoTileLen; more is refused, and so is a call of more than 1024 tiles), that
// also hands over what its kernels left in device memory.  hc, zc, ld ([all buffers' positions] words each, the buffers
// one after the other) and counts ([all buffers' deflate blocks][kLoCountWords]) are host arrays; each may be null.
ZMX_INTERNAL_EXPORT int zmx_internal_png_lodeflate_arrays(zmx_ctx* ctx, size_t n, const void* const* d_in, const size_t* insize,
                                                          unsigned windowsize, unsigned tile_len, uint32_t* hc, uint32_t* zc,
                                                          uint32_t* ld, uint32_t* counts, uint64_t* zlib_bytes);
// Test hook (tests/test_gpu_png_brute_sizes.py): zmx_png_filter_types_brute of a host image with the same checks, which
// also hands over what k_png_brute computed for every job = row * 5 + type: sizes[5 * height], the zlib bytes it wrote;
// bits[5 * height], its fixed-code bit count before rounding (3 + data + 7); types[height] from k_png_brute_pick.  Two
// knobs that no other caller has (host/png_brute_launch.h): force_scratch (0 / 1) puts the per-position arrays into the
// global scratch whatever the row length; max_workgroups caps the grid (0: the driver's own choice).
ZMX_INTERNAL_EXPORT int zmx_internal_png_brute_sizes(zmx_ctx* ctx, const unsigned char* image, size_t linebytes, size_t height,
                                                     size_t bytewidth, unsigned windowsize, int force_scratch, unsigned max_workgroups,
                                                     uint64_t* sizes, uint64_t* bits, unsigned char* types);
// The same for the calling thread's last zmx_checksum_device (or seal): k_checksum_pieces, k_checksum_finish.  For
// tools/png_device_output.py.
ZMX_INTERNAL_EXPORT void zmx_internal_checksum_device_ms(double out[2]);
// The same for the calling thread's last k_inflate launch (an inflate call's last round).  For tools/inflate_device.py.
ZMX_INTERNAL_EXPORT double zmx_internal_inflate_ms(void);
// The same for the calling thread's last PNG decode: k_png_chunks (all its launches), k_png_unfilter (likewise).  For
// tools/png_decode.py.
ZMX_INTERNAL_EXPORT void zmx_internal_png_decode_ms(double out[2]);
// The same call by the host's clock, whether kernel timing is on or not: the walk with its records down, the chunks'
// CRC-32s, the gather and k_inflate, the Adler-32s, k_png_unfilter with its results down.
ZMX_INTERNAL_EXPORT void zmx_internal_png_decode_phase_ms(double out[5]);
// The same for the calling thread's last zmx_png_unpack_device: k_png_unpack.  For tools/png_sink.py.
ZMX_INTERNAL_EXPORT double zmx_internal_png_unpack_ms(void);
// The same for the calling thread's last zmx_png_pack_device: k_png_pack.  For tools/png_source.py.
ZMX_INTERNAL_EXPORT double zmx_internal_png_pack_ms(void);
// Test hook (tests/test_cpu_abi.py): the acceptance facts of one cost model (320 costs: 288 litlen, 32 distance) as a
// squeeze run computes them — *wmax, *tiemask —, no device involved.
ZMX_INTERNAL_EXPORT void zmx_internal_run_info(const double* cost320, float* wmax, uint32_t* tiemask);

}  // extern "C"
