// zmx_compress_batch: n independent ZopfliCompress calls in one pass over the devices.
//
// The inputs are put end to end once and cut into their own master blocks (deflate.c:916-923 per input), and the parts
// of all inputs are dealt over the contexts like the master blocks of one large call (dealing.h).  What keeps the
// inputs apart is the floor of the window: a context is told where each input starts (zmx_set_input_segments), so a
// block's window reaches back to max(start of its input, instart - 32768) and never into the input before it — the
// reference's hash is reset and warmed from that point for each block (lz77.c:551-552, hash.c:100-137), so every
// input gets exactly the stream it gets alone.  The containers' checksums come from the same resident bytes, one
// zmx_checksums call per shard for all of its inputs; each input is then merged on its own at bit 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "deal.h"
#include "deflate.h"
#include "dealing.h"
#include "symbols.h"
#include "thread_pool.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"
#include "../device/zmx_probe.h"

namespace {

int Refuse(const std::string& msg) {
  zmx_internal_set_error(msg.c_str(), ZMX_ERR_REFUSED);
  return -1;
}

// a round's parts span at most this many bytes: a shard plus its window stays below 2^32 (the device layer's positions
// are 32-bit), as the rounds of 2000 master blocks of a single call
constexpr size_t kRoundBytes = static_cast<size_t>(2000) * zamd::kMasterBlock;
// the bytes of the parts one DeflateParts call takes: what 256 master blocks of a single call hold
constexpr size_t kGroupBytes = static_cast<size_t>(256) * zamd::kMasterBlock;

void PushByte(unsigned v, unsigned char** out, size_t* outsize) {
  const uint8_t b = static_cast<uint8_t>(v);
  zamd::AppendToOutput(&b, 1, out, outsize);
}

// Where the inputs of a batch lie: n host arrays, or n ranges of device memory.
struct BatchBytes {
  const unsigned char* const* host = nullptr;
  const void* const* device = nullptr;
};

// The bytes [lo, lo + size) of the inputs' concatenation in device memory: a plain allocation the call owns, not the
// context that filled it — that one is back in the pool while the shards copy from here (a call that held it would
// starve a pool of one context).
struct Staging {
  int device = -1;
  void* p = nullptr;
  size_t lo = 0, size = 0;
  Staging() = default;
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() { zmx_internal_device_free(device, p); }
};

// A round of a device batch, on one pooled context: the inputs' bytes [stage->lo, round's end) gathered into `stage`,
// and the counts behind the dealing taken from them — one range per part, over that part's own bytes (PlanShards'
// MasterBlockCost), and one over the round (ContextsPerDevice's LooksLikeRuns).
int StageRound(const void* const* d_in, const std::vector<size_t>& start, size_t file_lo, size_t file_hi,
               const std::vector<zamd::Part>& round, size_t lo, Staging* stage, zamd::DeviceInput* dev) {
  const size_t hi = round.back().inend;
  std::vector<const void*> src;
  std::vector<size_t> len;
  for (size_t f = file_lo; f <= file_hi; ++f) {
    const size_t s = std::max(start[f], lo), e = std::min(start[f + 1], hi);
    if (e <= s) continue;
    src.push_back(static_cast<const unsigned char*>(d_in[f]) + (s - start[f]));
    len.push_back(e - s);
  }
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    stage->device = zmx_internal_device(ctx);
    stage->lo = lo;
    stage->size = hi - lo;
    if (zmx_internal_device_alloc(stage->device, stage->size, &stage->p) != 0) return -1;
    if (zmx_gather_device(ctx, src.size(), src.data(), len.data(), stage->p) != 0) return -1;
    zamd::AddDeviceTraffic(static_cast<double>(stage->size));
    if (round.size() < 2) return 0;   // (one part: one shard on one context, whatever its bytes)
    const size_t nranges = round.size() + 1;
    std::vector<uint64_t> ranges;
    for (const zamd::Part& p : round) {
      ranges.push_back(p.instart - lo);
      ranges.push_back(p.inend - lo);
    }
    ranges.push_back(round.front().instart - lo);
    ranges.push_back(hi - lo);
    std::vector<uint32_t> counts(nranges * zamd::kProbeCounts);
    constexpr size_t kSlice = 65535;   // ranges of one launch (zmx_internal_probe_counts)
    for (size_t r = 0; r < nranges; r += kSlice) {
      if (zmx_internal_probe_counts(ctx, stage->p, std::min(kSlice, nranges - r), &ranges[2 * r],
                                    &counts[r * zamd::kProbeCounts]) != 0) return -1;
    }
    dev->cost.resize(round.size());
    for (size_t i = 0; i < round.size(); ++i) {
      const uint32_t* k = &counts[i * zamd::kProbeCounts];
      dev->cost[i] = zamd::CostFromCounts(round[i].inend - round[i].instart, k[zamd::kProbes], k[zamd::kRuns], k[zamd::kFew]);
    }
    const uint32_t* k = &counts[round.size() * zamd::kProbeCounts];
    dev->runs.assign(1, zamd::RunsFromCounts(k[zamd::kProbes4k], k[zamd::kHits]) ? 1 : 0);
    dev->round_parts = round.size();
    dev->first_part = 0;
    return 0;
  });
}

// The n ZopfliCompress calls of `who` (an entry point's name), the inputs lying where `bytes` says.
int CompressBatch(const char* who, const ZopfliOptions* options, ZopfliFormat output_type, size_t n, const BatchBytes& bytes,
                  const size_t* insize, unsigned char** out, size_t* outsize) {
  const std::string w(who);
  if (!options) return Refuse(w + ": no options");
  if (output_type != ZOPFLI_FORMAT_GZIP && output_type != ZOPFLI_FORMAT_ZLIB && output_type != ZOPFLI_FORMAT_DEFLATE) {
    return Refuse(w + ": invalid ZopfliFormat " + std::to_string(static_cast<int>(output_type)));
  }
  if (n == 0) return 0;
  if ((!bytes.host && !bytes.device) || !insize || !out || !outsize) return Refuse(w + ": null array");
  if (bytes.host) {
    for (size_t i = 0; i < n; ++i) {
      if (insize[i] && !bytes.host[i]) return Refuse(w + ": null input with a non-zero size");
    }
  } else if (zmx_internal_device_pointers(who, n, bytes.device, insize) != 0) {
    return -1;   // (every pointer before anything is done with any: the device layer's refusal stands)
  }
  zamd::ResetCallStats();
  const double tr0 = zamd::CallWallMs();

  // ---- the inputs end to end, each cut into its own master blocks
  std::vector<size_t> start(n + 1, 0);
  for (size_t i = 0; i < n; ++i) start[i + 1] = start[i] + insize[i];
  const size_t total = start[n];
  std::unique_ptr<unsigned char[]> cat;   // (device inputs: none — stored chunks carry their bytes)
  if (bytes.host) {
    cat.reset(new unsigned char[total ? total : 1]);
    zamd::ParallelFor(n, [&](size_t i) { if (insize[i]) std::memcpy(cat.get() + start[i], bytes.host[i], insize[i]); });
  }
  std::vector<zamd::Part> parts;
  std::vector<size_t> part_file, first_part(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    first_part[i] = parts.size();
    for (zamd::Part p : zamd::InputMasterBlocks(insize[i], true)) {
      p.instart += start[i];
      p.inend += start[i];
      parts.push_back(p);
      part_file.push_back(i);
    }
  }
  first_part[n] = parts.size();

  // ---- checksums of the containers: per shard, the bytes of each of its inputs it holds, put together in stream order
  const int kind = output_type == ZOPFLI_FORMAT_GZIP ? ZMX_CRC32 : output_type == ZOPFLI_FORMAT_ZLIB ? ZMX_ADLER32 : -1;
  std::vector<size_t> sum_limit(n);   // the bytes the trailer covers (zlib_container.c:54 truncates the size to unsigned)
  for (size_t i = 0; i < n; ++i) sum_limit[i] = kind == ZMX_ADLER32 ? static_cast<unsigned>(insize[i]) : insize[i];
  std::vector<uint32_t> sum(n, kind == ZMX_ADLER32 ? 1u : 0u);
  struct ShardSums {
    std::vector<size_t> file;
    std::vector<uint64_t> len;
    std::vector<uint32_t> value;
  };
  std::vector<ShardSums> shard_sums;
  std::mutex shard_mu;

  zamd::ShardHooks hooks;
  hooks.group_bytes = kGroupBytes;
  hooks.split_on_device = true;
  hooks.floor = [&](size_t pos) {
    // the last input that starts at or before pos (several start there when some are empty: all at the same byte)
    const size_t i = static_cast<size_t>(std::upper_bound(start.begin(), start.begin() + static_cast<long>(n), pos) -
                                         start.begin()) - 1;
    return start[i];
  };
  const std::vector<zamd::Part>* round_parts = nullptr;
  size_t round_first = 0;   // index of the round's first part in `parts`
  hooks.uploaded = [&](size_t shard, zmx_ctx* ctx, size_t base, size_t first, size_t last) -> int {
    const std::vector<zamd::Part>& rp = *round_parts;
    const size_t f0 = part_file[round_first + first], f1 = part_file[round_first + last - 1];
    const size_t lo = rp[first].instart, hi = rp[last - 1].inend;
    std::vector<uint64_t> seg;
    for (size_t f = f0; f <= f1; ++f) seg.push_back(std::max(start[f], base) - base);
    if (zmx_set_input_segments(ctx, seg.data(), seg.size()) != 0) return -1;
    ShardSums ss;
    if (kind >= 0) {
      std::vector<uint64_t> b, e;
      for (size_t f = f0; f <= f1; ++f) {
        const size_t s = std::max(start[f], lo), t = std::min(start[f] + sum_limit[f], hi);
        if (t <= s) continue;
        ss.file.push_back(f);
        b.push_back(s - base);
        e.push_back(t - base);
      }
      ss.len.resize(b.size());
      ss.value.resize(b.size());
      for (size_t k = 0; k < b.size(); ++k) ss.len[k] = e[k] - b[k];
      if (!b.empty() && zmx_checksums(ctx, kind, b.size(), b.data(), e.data(), ss.value.data()) != 0) return -1;
    }
    std::lock_guard<std::mutex> g(shard_mu);
    if (shard_sums.size() <= shard) shard_sums.resize(shard + 1);
    shard_sums[shard] = std::move(ss);
    return 0;
  };

  // ---- rounds of at most kRoundBytes, each dealt over the contexts
  std::vector<zamd::Chunk> chunks;
  std::vector<size_t> part_chunks;
  for (size_t a = 0; a < parts.size();) {
    size_t b = a + 1;
    while (b < parts.size() && parts[b].inend - parts[a].instart <= kRoundBytes) ++b;
    const std::vector<zamd::Part> round(parts.begin() + static_cast<long>(a), parts.begin() + static_cast<long>(b));
    round_parts = &round;
    round_first = a;
    shard_sums.clear();
    Staging stage;
    zamd::DeviceInput dev;
    if (bytes.device) {
      // from the floor of the window of the round's first part (RunShard's base): its input's first byte, unless the
      // input began in a round before this one
      const size_t first = round.front().instart;
      const size_t lo = std::max(hooks.floor(first), first > zamd::kWindow ? first - zamd::kWindow : 0);
      if (StageRound(bytes.device, start, part_file[a], part_file[b - 1], round, lo, &stage, &dev) != 0) return -1;
      dev.upload = [&stage](zmx_ctx* ctx, size_t base, size_t nbytes) {
        if (base < stage.lo || nbytes > stage.size - (base - stage.lo)) {
          zmx_internal_set_error("device batch: a shard reaches outside the round's staging buffer", ZMX_ERR_REFUSED);
          return -1;
        }
        return zmx_set_input_device(ctx, static_cast<const unsigned char*>(stage.p) + (base - stage.lo), nbytes);
      };
    }
    const int rc = zamd::RunPartsDealt(*options, 2, cat.get(), round, &chunks, &part_chunks, &hooks, bytes.device ? &dev : nullptr);
    if (rc) {
      zmx_internal_set_error(hooks.error.c_str(), hooks.error_class);
      return -1;
    }
    for (const ShardSums& ss : shard_sums) {
      for (size_t k = 0; k < ss.file.size(); ++k) sum[ss.file[k]] = zmx_checksum_combine(kind, sum[ss.file[k]], ss.value[k], ss.len[k]);
    }
    a = b;
  }
  if (part_chunks.size() != parts.size()) return Refuse(w + ": chunks do not match the parts");
  const double tr1 = zamd::CallWallMs();

  // ---- each input merged on its own at bit 0 (ZopfliGzipCompress / ZopfliZlibCompress / ZopfliDeflate)
  std::vector<size_t> first_chunk(parts.size() + 1, 0);
  for (size_t p = 0; p < parts.size(); ++p) first_chunk[p + 1] = first_chunk[p] + part_chunks[p];
  auto assemble = [&](size_t i) {
    unsigned char** o = &out[i];
    size_t* os = &outsize[i];
    const std::vector<zamd::Chunk> mine(std::make_move_iterator(chunks.begin() + static_cast<long>(first_chunk[first_part[i]])),
                                        std::make_move_iterator(chunks.begin() + static_cast<long>(first_chunk[first_part[i + 1]])));
    unsigned char bp = 0;
    if (output_type == ZOPFLI_FORMAT_GZIP) {
      static const unsigned char header[10] = {31, 139, 8, 0, 0, 0, 0, 0, 2, 3};  // gzip_container.c:90-101
      zamd::AppendToOutput(header, 10, o, os);
    } else if (output_type == ZOPFLI_FORMAT_ZLIB) {
      const unsigned cmf = 120, flevel = 3, fdict = 0;  // zlib_container.c:56-63
      unsigned cmfflg = 256 * cmf + fdict * 32 + flevel * 64;
      cmfflg += 31 - cmfflg % 31;
      PushByte(cmfflg / 256, o, os);
      PushByte(cmfflg % 256, o, os);
    }
    const size_t offset = *os;
    zamd::MergeChunks(mine, cat.get(), &bp, o, os, options->verbose != 0);
    if (options->verbose) {    // deflate.c:925-930
      std::fprintf(stderr, "Original Size: %lu, Deflate: %lu, Compression: %f%% Removed\n",
                   static_cast<unsigned long>(insize[i]), static_cast<unsigned long>(*os - offset),
                   100.0 * static_cast<double>(insize[i] - (*os - offset)) / static_cast<double>(insize[i]));
    }
    if (output_type == ZOPFLI_FORMAT_GZIP) {
      for (int k = 0; k < 4; ++k) PushByte((sum[i] >> (8 * k)) & 255, o, os);
      for (int k = 0; k < 4; ++k) PushByte((insize[i] >> (8 * k)) & 255, o, os);
      if (options->verbose) {   // gzip_container.c:112-116
        std::fprintf(stderr, "Original Size: %d, Gzip: %d, Compression: %f%% Removed\n", static_cast<int>(insize[i]),
                     static_cast<int>(*os), 100.0 * static_cast<double>(insize[i] - *os) / static_cast<double>(insize[i]));
      }
    } else if (output_type == ZOPFLI_FORMAT_ZLIB) {
      for (int k = 3; k >= 0; --k) PushByte((sum[i] >> (8 * k)) & 255, o, os);
      if (options->verbose) {   // zlib_container.c:76-80
        std::fprintf(stderr, "Original Size: %d, Zlib: %d, Compression: %f%% Removed\n", static_cast<int>(insize[i]),
                     static_cast<int>(*os), 100.0 * static_cast<double>(insize[i] - *os) / static_cast<double>(insize[i]));
      }
    }
  };
  // (verbose: the lines of the n calls in input order, so one input after the other)
  if (options->verbose) {
    for (size_t i = 0; i < n; ++i) assemble(i);
  } else {
    zamd::ParallelFor(n, assemble);
  }
  if (zamd::TraceCallOn()) {
    std::fprintf(stderr, "%s(%zu inputs, %zu parts, %zu bytes): parts %.2f ms, merge %.2f ms\n", who, n, parts.size(), total,
                 tr1 - tr0, zamd::CallWallMs() - tr1);
  }
  return 0;
}

}  // namespace

extern "C" int zmx_compress_batch(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                                  const unsigned char* const* in, const size_t* insize, unsigned char** out,
                                  size_t* outsize) {
  BatchBytes bytes;
  bytes.host = in;
  return CompressBatch("zmx_compress_batch", options, output_type, n, bytes, insize, out, outsize);
}

extern "C" int zmx_compress_device_batch(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                                         const void* const* d_in, const size_t* insize, unsigned char** out,
                                         size_t* outsize) {
  BatchBytes bytes;
  bytes.device = d_in;
  return CompressBatch("zmx_compress_device_batch", options, output_type, n, bytes, insize, out, outsize);
}
