// zmx_compress_batch: n independent ZopfliCompress calls in one pass over the devices.
//
// The inputs are put end to end once and cut into their own master blocks (deflate.c:916-923 per input), and the parts
// of all inputs are dealt over the contexts like the master blocks of one large call (dealing.h).  What keeps the
// inputs apart is the floor of the window: a context is told where each input starts (zmx_set_input_segments), so a
// block's window reaches back to max(start of its input, instart - 32768) and never into the input before it — the
// reference's hash is reset and warmed from that point for each block (lz77.c:551-552, hash.c:100-137), so every
// input gets exactly the stream it gets alone.  The containers' checksums come from the same resident bytes, one
// zmx_checksums call per shard for all of its inputs; each input is then merged on its own at bit 0 — on the host, or,
// for zmx_compress_device_batch_to_device and zmx_compress_device_batch_packed, by one bit join on the device (JoinStreams).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "deal.h"
#include "deflate.h"
#include "dealing.h"
#include "device_output_plan.h"
#include "entry_checks.h"
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

// Where the streams of a device batch go when they stay in device memory (zmx_compress_device_batch_to_device,
// zmx_compress_device_batch_packed): n destinations of the caller's, or one arena whose destinations follow from the
// streams' sizes.  The entry has checked the pointers; `device` is the one device they lie on.
struct DeviceOut {
  void* const* d_out = nullptr;      // separate destinations, with ...
  const size_t* capacity = nullptr;  // ... their room in bytes
  unsigned char* arena = nullptr;    // packed (align != 0): stream i at arena + outoffset[i]
  size_t arena_capacity = 0, align = 0;
  size_t* outoffset = nullptr;
  int device = -1;
  const zamd::PngFrame* frames = nullptr;   // a frame around every stream (device_output_plan.h): PNG files, sealed after the join
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
               const std::vector<zamd::Part>& round, size_t lo, Staging* stage, zamd::DeviceInput* dev, int only_device = -1) {
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
  }, only_device);
}

// dev.finish of a batch whose streams stay in device memory: input i's stream is the container's header, its own chunks
// from bit 0 and its trailer — exactly what `assemble` below builds on the host —, planned as bit pieces
// (device_output_plan.h).  All sizes are known from the plans before anything is written; the plans' literals go up as
// one buffer, their pieces as one table with a destination per input, and one launch joins them.  `d_cat`: the device
// memory that the stored chunks' positions refer to.
int JoinStreams(const std::string& w, zmx_ctx* ctx, ZopfliFormat output_type, size_t n, const size_t* insize,
                const std::vector<uint32_t>& sum, const std::vector<zamd::Chunk>& chunks, const std::vector<size_t>& part_chunks,
                const std::vector<size_t>& first_part, const unsigned char* d_cat, const DeviceOut& to, size_t* outsize) {
  if (part_chunks.size() != first_part[n]) return Refuse(w + ": chunks do not match the parts");
  std::vector<size_t> first_chunk(part_chunks.size() + 1, 0);
  for (size_t p = 0; p < part_chunks.size(); ++p) first_chunk[p + 1] = first_chunk[p] + part_chunks[p];
  std::vector<zamd::OutputPlan> plans(n);
  const std::vector<uint8_t> header = zamd::ContainerHeader(output_type);
  zamd::ParallelFor(n, [&](size_t i) {
    std::vector<uint8_t> trailer = zamd::ContainerTrailer(output_type, sum[i], insize[i]);
    if (to.frames) trailer = zamd::PngFrameTrailer(std::move(trailer));
    plans[i] = zamd::PlanOutput(to.frames ? zamd::PngFrameHeader(to.frames[i]) : header, chunks.data() + first_chunk[first_part[i]],
                                chunks.data() + first_chunk[first_part[i + 1]], d_cat, trailer);
  });
  // ---- the sizes, and with them the destinations, before anything is written
  std::vector<size_t> size(n), offset(n, 0);
  for (size_t i = 0; i < n; ++i) size[i] = static_cast<size_t>(plans[i].total_bits / 8);
  std::string short_of;
  for (size_t i = 0; to.frames && i < n && short_of.empty(); ++i) {
    if (!zamd::PngFrameSetLength(to.frames[i], &plans[i])) short_of = "the zlib stream of image " + std::to_string(i) + " does not fit an IDAT chunk";
  }
  if (to.align != 0) {
    const size_t end = zamd::PackedOffsets(n, size.data(), to.align, offset.data());
    for (size_t i = 0; i < n; ++i) to.outoffset[i] = offset[i];
    if (short_of.empty() && end > to.arena_capacity) short_of = "the streams take " + std::to_string(end) + " bytes, the arena has " + std::to_string(to.arena_capacity);
  } else {
    for (size_t i = 0; i < n && short_of.empty(); ++i) {
      if (size[i] > to.capacity[i]) {
        short_of = "stream " + std::to_string(i) + " takes " + std::to_string(size[i]) + " bytes, d_out[" + std::to_string(i) + "] has " +
                   std::to_string(to.capacity[i]);
      }
    }
  }
  if (!short_of.empty()) {
    for (size_t i = 0; i < n; ++i) outsize[i] = size[i];
    return Refuse(w + ": " + short_of);
  }
  // ---- one literals buffer, one piece table, a destination per input
  size_t nliterals = 0, npieces = 0;
  for (const zamd::OutputPlan& plan : plans) {
    nliterals += plan.literals.size();
    npieces += plan.pieces.size();
  }
  std::vector<unsigned char> literals;
  std::vector<zmx_bit_piece> pieces;
  std::vector<unsigned char> is_literal;
  std::vector<zmx_bit_dest> dests(n);
  literals.reserve(nliterals);
  pieces.reserve(npieces);
  is_literal.reserve(npieces);
  double device_blocks = 0, host_blocks = 0;
  for (size_t i = 0; i < n; ++i) {
    const zamd::OutputPlan& plan = plans[i];
    void* dst = to.align != 0 ? static_cast<void*>(to.arena + offset[i]) : to.d_out[i];
    dests[i] = {dst, plan.total_bits, pieces.size(), plan.pieces.size()};
    for (const zamd::PlanPiece& q : plan.pieces) {
      is_literal.push_back(q.literal);
      pieces.push_back({q.literal ? reinterpret_cast<const void*>(q.lit + literals.size()) : q.dev, q.src_bit, q.nbits, q.dst_bit});
    }
    literals.insert(literals.end(), plan.literals.begin(), plan.literals.end());
    device_blocks += static_cast<double>(plan.device_blocks);
    host_blocks += static_cast<double>(plan.host_blocks);
  }
  if (zmx_internal_bitjoin_many_literals(ctx, literals.data(), literals.size(), n, dests.data(), nullptr, pieces.size(), pieces.data(),
                                         is_literal.data()) != 0) return -1;
  if (to.frames) {
    // every IDAT's CRC-32 over its type and the joined stream, into the placeholder behind it: two launches for all files
    std::vector<const void*> from(n);
    std::vector<size_t> covered(n);
    std::vector<unsigned char*> seal(n);
    for (size_t i = 0; i < n; ++i) {
      unsigned char* const file = static_cast<unsigned char*>(dests[i].dst);
      const size_t prefix = to.frames[i].file_prefix.size();
      from[i] = file + prefix - 4;
      covered[i] = 4 + static_cast<size_t>(zamd::PngFrameIdatBytes(size[i], prefix));
      seal[i] = file + size[i] - zamd::kPngTrailerBytes;
    }
    if (zmx_internal_checksum_seal(ctx, ZMX_CRC32, n, from.data(), covered.data(), seal.data()) != 0) return -1;
  }
  const double traffic[4] = {0, static_cast<double>(literals.size()), device_blocks, host_blocks};
  zamd::SetOutputTraffic(traffic);
  for (size_t i = 0; i < n; ++i) outsize[i] = size[i];
  return 0;
}

// The n ZopfliCompress calls of `who` (an entry point's name), the inputs lying where `bytes` says.  `to` (device inputs
// only, `out` null): the streams stay in device memory — the shards keep their blocks' bits where the device wrote them,
// and one zmx_bitjoin_many_device puts all n streams together while the call still holds its contexts; on a destination
// that is too small outsize[] (and to->outoffset[]) hold what is needed, and nothing is written.
int CompressBatch(const char* who, const ZopfliOptions* options, ZopfliFormat output_type, size_t n, const BatchBytes& bytes,
                  const size_t* insize, unsigned char** out, size_t* outsize, const DeviceOut* to = nullptr) {
  const std::string w(who);
  if (!options) return Refuse(w + ": no options");
  if (output_type != ZOPFLI_FORMAT_GZIP && output_type != ZOPFLI_FORMAT_ZLIB && output_type != ZOPFLI_FORMAT_DEFLATE) {
    return Refuse(w + ": invalid ZopfliFormat " + std::to_string(static_cast<int>(output_type)));
  }
  if (n == 0) return 0;
  if ((!bytes.host && !bytes.device) || !insize || (!out && !to) || !outsize) return Refuse(w + ": null array");
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
  if (to && parts.back().inend - parts.front().instart > kRoundBytes) {
    return Refuse(w + ": " + std::to_string(total) + " bytes of inputs are more than one round (" + std::to_string(kRoundBytes) +
                  "): not joined on the device");
  }

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
  const auto combine_sums = [&] {
    for (const ShardSums& ss : shard_sums) {
      for (size_t k = 0; k < ss.file.size(); ++k) sum[ss.file[k]] = zmx_checksum_combine(kind, sum[ss.file[k]], ss.value[k], ss.len[k]);
    }
  };
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
      if (StageRound(bytes.device, start, part_file[a], part_file[b - 1], round, lo, &stage, &dev, to ? to->device : -1) != 0) return -1;
      dev.upload = [&stage](zmx_ctx* ctx, size_t base, size_t nbytes) {
        if (base < stage.lo || nbytes > stage.size - (base - stage.lo)) {
          zmx_internal_set_error("device batch: a shard reaches outside the round's staging buffer", ZMX_ERR_REFUSED);
          return -1;
        }
        return zmx_set_input_device(ctx, static_cast<const unsigned char*>(stage.p) + (base - stage.lo), nbytes);
      };
    }
    if (to) {
      // (the one round: the staging buffer holds every input's bytes, and is where the join reads the stored blocks')
      dev.device_output = true;
      dev.only_device = to->device;
      dev.finish = [&](zmx_ctx* ctx, std::vector<zamd::Chunk>* all, uint32_t) {
        combine_sums();   // (shard_sums is complete: the shards are collected)
        return JoinStreams(w, ctx, output_type, n, insize, sum, *all, part_chunks, first_part,
                           static_cast<const unsigned char*>(stage.p) - stage.lo, *to, outsize);
      };
    }
    const int rc = zamd::RunPartsDealt(*options, 2, cat.get(), round, &chunks, &part_chunks, &hooks, bytes.device ? &dev : nullptr);
    if (rc) {
      // (a shard's failure is in both; a lease that found no context and dev.finish's are in dev alone)
      if (bytes.device && !dev.error.empty()) zmx_internal_set_error(dev.error.c_str(), dev.error_class);
      else zmx_internal_set_error(hooks.error.c_str(), hooks.error_class);
      return -1;
    }
    if (!to) combine_sums();
    a = b;
  }
  if (part_chunks.size() != parts.size()) return Refuse(w + ": chunks do not match the parts");
  const double tr1 = zamd::CallWallMs();
  if (to) {
    if (zamd::TraceCallOn()) {
      std::fprintf(stderr, "%s(%zu inputs, %zu parts, %zu bytes): parts and join %.2f ms\n", who, n, parts.size(), total, tr1 - tr0);
    }
    return 0;
  }

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

namespace {

// What both device-output entries refuse before anything runs: the arguments, the inputs as zmx_compress_device_batch
// refuses them, and the `ndst` destinations d_out[i][0, capacity[i]) — null with a non-zero capacity, not plain device
// memory, on different devices, sharing a byte with one another or with an input.  1: nothing to do (n = 0).
int CheckDeviceOut(const std::string& w, const ZopfliOptions* options, ZopfliFormat output_type, size_t n, const void* const* d_in,
                   const size_t* insize, size_t ndst, void* const* d_out, const size_t* capacity, size_t* outsize, int* device) {
  if (!options) return Refuse(w + ": no options");
  if (output_type != ZOPFLI_FORMAT_GZIP && output_type != ZOPFLI_FORMAT_ZLIB && output_type != ZOPFLI_FORMAT_DEFLATE) {
    return Refuse(w + ": invalid ZopfliFormat " + std::to_string(static_cast<int>(output_type)));
  }
  if (n == 0) return 1;
  if (!d_in || !insize || !d_out || !capacity || !outsize) return Refuse(w + ": null array");
  for (size_t i = 0; i < n; ++i) outsize[i] = 0;
  if (zmx_internal_device_pointers(w.c_str(), n, d_in, insize) != 0) return -1;
  const std::string wd = w + ": d_out";
  if (zmx_internal_device_pointers_one_device(wd.c_str(), ndst, d_out, capacity, device) != 0) return -1;
  zamd::ApartRanges apart;
  for (size_t i = 0; i < ndst; ++i) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_out[i]);
    apart.Add(at, at + capacity[i], i);
  }
  apart.Sort();
  size_t a = 0, b = 0;
  if (apart.Overlap(&a, &b)) return Refuse(wd + "[" + std::to_string(std::max(a, b)) + "] overlaps d_out[" + std::to_string(std::min(a, b)) + "]");
  for (size_t i = 0; i < n; ++i) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_in[i]);
    if (apart.Hit(at, at + insize[i], &a)) return Refuse(wd + "[" + std::to_string(a) + "] overlaps d_in[" + std::to_string(i) + "]");
  }
  return 0;
}

}  // namespace

extern "C" int zmx_compress_device_batch_to_device(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                                                   const void* const* d_in, const size_t* insize, void* const* d_out,
                                                   const size_t* capacity, size_t* outsize) {
  static const char* const kWho = "zmx_compress_device_batch_to_device";
  DeviceOut to;
  if (const int rc = CheckDeviceOut(kWho, options, output_type, n, d_in, insize, n, d_out, capacity, outsize, &to.device)) return rc < 0 ? -1 : 0;
  to.d_out = d_out;
  to.capacity = capacity;
  BatchBytes bytes;
  bytes.device = d_in;
  return CompressBatch(kWho, options, output_type, n, bytes, insize, nullptr, outsize, &to);
}

namespace {

int BatchPacked(const char* kWho, const ZopfliOptions* options, ZopfliFormat output_type, size_t n, const void* const* d_in, const size_t* insize,
                const zamd::PngFrame* frames, void* d_arena, size_t capacity, size_t align, size_t* outoffset, size_t* outsize) {
  DeviceOut to;
  to.frames = frames;
  void* const arena[1] = {d_arena};
  if (const int rc = CheckDeviceOut(kWho, options, output_type, n, d_in, insize, 1, arena, &capacity, outsize, &to.device)) return rc < 0 ? -1 : 0;
  if (!outoffset) return Refuse(std::string(kWho) + ": null array");
  for (size_t i = 0; i < n; ++i) outoffset[i] = 0;
  if (!zamd::PackedAlignOk(align)) return Refuse(std::string(kWho) + ": align " + std::to_string(align) + " is not a power of two from 1 to 4096");
  to.arena = static_cast<unsigned char*>(d_arena);
  to.arena_capacity = capacity;
  to.align = align;
  to.outoffset = outoffset;
  BatchBytes bytes;
  bytes.device = d_in;
  return CompressBatch(kWho, options, output_type, n, bytes, insize, nullptr, outsize, &to);
}

}  // namespace

extern "C" int zmx_compress_device_batch_packed(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                                                const void* const* d_in, const size_t* insize, void* d_arena, size_t capacity,
                                                size_t align, size_t* outoffset, size_t* outsize) {
  return BatchPacked("zmx_compress_device_batch_packed", options, output_type, n, d_in, insize, nullptr, d_arena, capacity, align, outoffset,
                     outsize);
}

int zamd::CompressDeviceBatchPackedFramed(const char* who, const ZopfliOptions* options, size_t n, const void* const* d_in, const size_t* insize,
                                          const zamd::PngFrame* frames, void* d_arena, size_t capacity, size_t align, size_t* outoffset,
                                          size_t* outsize) {
  return BatchPacked(who, options, ZOPFLI_FORMAT_ZLIB, n, d_in, insize, frames, d_arena, capacity, align, outoffset, outsize);
}
