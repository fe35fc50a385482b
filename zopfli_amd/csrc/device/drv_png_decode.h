// Driver part: PNG decode on the device (zmx_png_decode.h).  Holds the run that every decode entry shares
// (zmx_internal_png_decode_run: the chunk walk, the CRCs, the gather of split IDATs, k_inflate, the Adler-32s, k_png_unfilter;
// with sinks — zmx_internal_png_decode_sink_run — the unfilter writes _OWN pixels into a buffer of the call's own and one
// k_png_unpack launch stores them through the sinks) and zmx_png_decode_device_ctx and zmx_png_decode_sink_device_ctx, the
// steps on a context the caller holds.
// Needs drv_context.h (zmx_ctx, PoolScope, KernelTiming), drv_input.h (DeviceRangeChecker, zmx_gather_device),
// drv_checksum_device.h (RunChecksumDevice), drv_inflate.h (zmx_internal_inflate_run), drv_png_unpack.h (PngSinksCheck,
// PngUnpackAddJob, PngUnpackEnqueue), host/png_decode_plan.h.
#pragma once
#include <chrono>

static_assert(zamd::kPngDecOk == ZMX_PNG_DECODE_OK && zamd::kPngDecSignature == ZMX_PNG_DECODE_SIGNATURE && zamd::kPngDecIhdr == ZMX_PNG_DECODE_IHDR &&
                  zamd::kPngDecInterlace == ZMX_PNG_DECODE_INTERLACE && zamd::kPngDecChunk == ZMX_PNG_DECODE_CHUNK &&
                  zamd::kPngDecCritical == ZMX_PNG_DECODE_CRITICAL && zamd::kPngDecCrc == ZMX_PNG_DECODE_CRC && zamd::kPngDecPlte == ZMX_PNG_DECODE_PLTE &&
                  zamd::kPngDecTrns == ZMX_PNG_DECODE_TRNS && zamd::kPngDecStream == ZMX_PNG_DECODE_STREAM && zamd::kPngDecSize == ZMX_PNG_DECODE_SIZE &&
                  zamd::kPngDecFilter == ZMX_PNG_DECODE_FILTER && zamd::kPngDecCapacity == ZMX_PNG_DECODE_CAPACITY &&
                  zamd::kPngDecShape == ZMX_PNG_DECODE_SHAPE,
              "the kernels' statuses are the ABI's");
static_assert(zamd::kPngDecOwn == ZMX_PNG_DECODE_OWN && zamd::kPngDecRgba8 == ZMX_PNG_DECODE_RGBA8, "the kernels' modes are the ABI's");
static_assert(sizeof(zamd::PngUnfilterScratch) <= 18 * 1024, "a wave's LDS: eight waves a CU");

namespace {

constexpr size_t kPngDecodeMaxFiles = size_t{1} << 24;   // what one call's arrays and grids take

inline size_t PngAlign16(size_t v) { return (v + 15) & ~size_t{15}; }

// k_png_chunks over `refs` (their slots index `records` and `palettes`), the records and `nentries` entries down.
int PngWalkLaunch(zmx_ctx* c, PoolScope* tmp, const std::vector<zamd::PngFileRef>& refs, zamd::PngWalkRecord* d_records, u32* d_palettes,
                  size_t nentries, std::vector<zamd::PngChunkEntry>* entries, bool timed, double* ms) {
  zamd::PngFileRef* d_refs = nullptr;
  zamd::PngChunkEntry* d_entries = nullptr;
  HIPCHK(tmp->Upload(&d_refs, refs.data(), refs.size(), "png_decode_files"));
  HIPCHK(tmp->AllocT(&d_entries, nentries, "png_decode_entries"));
  PngChunksParams P;
  P.files = d_refs;
  P.records = d_records;
  P.entries = d_entries;
  P.palettes = d_palettes;
  P.nfiles = static_cast<u32>(refs.size());
  if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
  hipLaunchKernelGGL(k_png_chunks, dim3(static_cast<unsigned>((refs.size() + 63) / 64)), dim3(64), 0, c->stream, P);
  KCHK(c, "k_png_chunks");
  if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
  entries->resize(nentries);
  HIPCHK(hipMemcpyAsync(entries->data(), d_entries, nentries * sizeof(zamd::PngChunkEntry), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
    *ms += t;
  }
  return 0;
}

static thread_local double g_png_decode_ms[2] = {0, 0};   // (zmx_internal_png_decode_ms)
// the host's clock at the phases' ends: the walk, the CRCs, the gather and k_inflate, the Adler-32s, the unfilter
static thread_local double g_png_decode_phase_ms[5] = {0, 0, 0, 0, 0};   // (zmx_internal_png_decode_phase_ms)

// The run.  `sinks` null: file i's pixels in `mode` go to d_out[i].  Else (mode _OWN, d_out and capacity null): a file
// whose size is its sink's is unfiltered into a buffer of the call's own and stored through sinks[i] by k_png_unpack, one
// launch for all of them behind the unfilter.
int PngDecodeRun(zmx_ctx* c, const char* who, int mode, int info_only, size_t n, const void* const* d_file, const size_t* filesize,
                 void* const* d_out, const size_t* capacity, const zmx_png_sink* sinks, zmx_png_decode_result* results,
                 const zmx_png_decode_hooks* hooks) {
  g_png_decode_ms[0] = g_png_decode_ms[1] = 0;
  for (double& t : g_png_decode_phase_ms) t = 0;
  if (n == 0) return 0;
  if (n > kPngDecodeMaxFiles) return FailMsg(std::string(who) + ": too many files for one call");
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  const u32 cap0 = hooks && hooks->idat_capacity ? hooks->idat_capacity : zamd::kPngDecEntries;
  const bool force_wide = hooks && hooks->force_wide;
  std::vector<void*> own_out;        // (sinks: where the unfilter writes, and how much)
  std::vector<size_t> own_capacity;
  const auto stored = [&](size_t i) { return !info_only && d_out && d_out[i]; };
  auto clock = std::chrono::steady_clock::now();
  const auto phase_done = [&](int phase) {   // (every phase ends with the stream drained)
    const auto now = std::chrono::steady_clock::now();
    g_png_decode_phase_ms[phase] = std::chrono::duration<double, std::milli>(now - clock).count();
    clock = now;
  };
  const auto run = [&]() -> int {
    // ---- the chunk walk: the records, the entries, the palettes
    std::vector<zamd::PngWalkRecord> rec(n);
    std::vector<std::vector<zamd::PngChunkEntry>> ent(n);
    std::vector<u32> palettes;
    {
      zamd::PngWalkRecord* d_records = nullptr;
      u32* d_palettes = nullptr;
      HIPCHK(tmp.AllocT(&d_records, n, "png_decode_records"));
      HIPCHK(tmp.AllocT(&d_palettes, 256 * n, "png_decode_palettes"));
      std::vector<zamd::PngFileRef> refs(n);
      for (size_t i = 0; i < n; ++i) {
        refs[i] = {static_cast<const unsigned char*>(d_file[i]), filesize[i], static_cast<uint64_t>(i) * cap0, cap0, static_cast<u32>(i)};
      }
      std::vector<zamd::PngChunkEntry> flat;
      if (const int rc = PngWalkLaunch(c, &tmp, refs, d_records, d_palettes, n * cap0, &flat, timed, &g_png_decode_ms[0])) return rc;
      HIPCHK(hipMemcpyAsync(rec.data(), d_records, n * sizeof(zamd::PngWalkRecord), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      // (a file with more checked chunks than the first walk had room for: walked again, with room)
      std::vector<zamd::PngFileRef> again;
      size_t again_entries = 0;
      for (size_t i = 0; i < n; ++i) {
        if (rec[i].nentries <= cap0) {
          ent[i].assign(flat.begin() + i * cap0, flat.begin() + i * cap0 + rec[i].nentries);
          continue;
        }
        again.push_back({static_cast<const unsigned char*>(d_file[i]), filesize[i], again_entries, rec[i].nentries, static_cast<u32>(i)});
        again_entries += rec[i].nentries;
      }
      if (!again.empty()) {
        if (const int rc = PngWalkLaunch(c, &tmp, again, d_records, d_palettes, again_entries, &flat, timed, &g_png_decode_ms[0])) return rc;
        for (const zamd::PngFileRef& f : again) ent[f.slot].assign(flat.begin() + f.entry_first, flat.begin() + f.entry_first + f.entry_cap);
      }
      bool any_palette = false;
      for (size_t i = 0; i < n; ++i) any_palette = any_palette || rec[i].has_plte;
      if (any_palette) {
        palettes.resize(256 * n);
        HIPCHK(hipMemcpyAsync(palettes.data(), d_palettes, 256 * n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
      }
    }
    std::vector<uint64_t> scan(n, 0);
    for (size_t i = 0; i < n; ++i) {
      zamd::PngResultFromWalk(rec[i], mode, palettes.empty() ? nullptr : palettes.data() + 256 * i, &results[i]);
      if (zamd::PngHeaderKnown(rec[i]) && !zamd::PngScanBytes(rec[i], &scan[i])) {
        return FailMsg(std::string(who) + ": file " + std::to_string(i) + ": the header's scanlines take 2^40 bytes or more");
      }
    }
    phase_done(0);
    // ---- the chunks' CRC-32s: one launch pair over the checked chunks of every file that walked to its end
    {
      std::vector<const void*> ptrs;
      std::vector<size_t> sizes;
      for (size_t i = 0; i < n; ++i) {
        if (results[i].status != ZMX_PNG_DECODE_OK) continue;
        for (const zamd::PngChunkEntry& e : ent[i]) {
          ptrs.push_back(static_cast<const unsigned char*>(d_file[i]) + e.offset + 4);
          sizes.push_back(static_cast<size_t>(e.length) + 4);
        }
      }
      if (!ptrs.empty()) {
        std::vector<uint32_t> values(ptrs.size());
        if (const int rc = RunChecksumDevice(c, ZMX_CRC32, ptrs.size(), ptrs.data(), sizes.data(), nullptr, values.data())) return rc;
        size_t k = 0;
        for (size_t i = 0; i < n; ++i) {
          if (results[i].status != ZMX_PNG_DECODE_OK) continue;
          zamd::PngCrcVerdict(ent[i].data(), values.data() + k, static_cast<uint32_t>(ent[i].size()), &results[i]);
          k += ent[i].size();
        }
      }
    }
    phase_done(1);
    if (info_only) return 0;
    if (sinks) {
      // ---- a file whose size is not its sink's ends here; the others get their _OWN pixels' room
      size_t own_total = 0;
      std::vector<size_t> own_at(n, 0);
      for (size_t i = 0; i < n; ++i) {
        if (results[i].status != ZMX_PNG_DECODE_OK) continue;
        if (results[i].width != sinks[i].width || results[i].height != sinks[i].height) {
          results[i].status = ZMX_PNG_DECODE_SHAPE;
          results[i].detail = 0;
          continue;
        }
        own_at[i] = own_total;
        own_total += PngAlign16(static_cast<size_t>(results[i].outsize_own));
      }
      if (own_total > c->code_budget) return FailMsg(std::string(who) + ": the call's pixels are beyond the context's budget");
      unsigned char* d_own = nullptr;
      HIPCHK(tmp.AllocT(&d_own, own_total + 16, "png_decode_own"));
      d_own = reinterpret_cast<unsigned char*>(PngAlign16(reinterpret_cast<uintptr_t>(d_own)));
      own_out.assign(n, nullptr);
      own_capacity.assign(n, 0);
      for (size_t i = 0; i < n; ++i) {
        if (results[i].status != ZMX_PNG_DECODE_OK) continue;
        own_out[i] = d_own + own_at[i];
        own_capacity[i] = static_cast<size_t>(results[i].outsize_own);
      }
      d_out = own_out.data();
      capacity = own_capacity.data();
    }
    // ---- where each stream lies: one IDAT with bytes is read in place, several are put end to end
    std::vector<size_t> which;                       // the files that have a stream, in the caller's order
    std::vector<const void*> in;                     // (null: gathered, see gather_at)
    std::vector<size_t> insize, gather_at;
    std::vector<const void*> piece_ptr;
    std::vector<size_t> piece_size;
    size_t gathered = 0, scan_total = 0;
    std::vector<size_t> scan_at(n, 0);
    for (size_t i = 0; i < n; ++i) {
      if (results[i].status != ZMX_PNG_DECODE_OK) continue;
      size_t pieces = 0;
      const zamd::PngChunkEntry* one = nullptr;
      for (const zamd::PngChunkEntry& e : ent[i]) {
        if (e.kind != zamd::kPngChunkIdat || e.length == 0) continue;
        ++pieces;
        one = &e;
      }
      if (pieces == 0) {
        results[i].status = ZMX_PNG_DECODE_STREAM;
        results[i].detail = ZMX_INFLATE_TRUNCATED;
        continue;
      }
      which.push_back(i);
      if (pieces == 1) {
        in.push_back(static_cast<const unsigned char*>(d_file[i]) + one->offset + 8);
        insize.push_back(one->length);
        gather_at.push_back(0);
      } else {
        in.push_back(nullptr);
        insize.push_back(static_cast<size_t>(rec[i].idat_bytes));
        gather_at.push_back(gathered);
        for (const zamd::PngChunkEntry& e : ent[i]) {
          if (e.kind != zamd::kPngChunkIdat || e.length == 0) continue;
          piece_ptr.push_back(static_cast<const unsigned char*>(d_file[i]) + e.offset + 8);
          piece_size.push_back(e.length);
        }
        gathered += static_cast<size_t>(rec[i].idat_bytes);
      }
      if (stored(i)) {
        scan_at[i] = scan_total;
        scan_total += PngAlign16(static_cast<size_t>(scan[i]));   // (slices begin at 16-byte boundaries and end on whole words)
      }
    }
    if (scan_total > c->code_budget) return FailMsg(std::string(who) + ": the call's scanlines are beyond the context's budget");
    unsigned char *d_gather = nullptr, *d_scan = nullptr;
    if (gathered != 0) {
      HIPCHK(tmp.AllocT(&d_gather, gathered, "png_decode_idat"));
      if (const int rc = zmx_gather_device(c, piece_ptr.size(), piece_ptr.data(), piece_size.data(), d_gather)) return rc;
    }
    HIPCHK(tmp.AllocT(&d_scan, scan_total + 16, "png_decode_scanlines"));
    d_scan = reinterpret_cast<unsigned char*>(PngAlign16(reinterpret_cast<uintptr_t>(d_scan)));
    // ---- k_inflate: every stream into exactly its scanlines (a file without a destination: the size alone)
    std::vector<zmx_inflate_result> inflated(which.size());
    if (!which.empty()) {
      std::vector<void*> out(which.size());
      std::vector<size_t> cap(which.size());
      for (size_t k = 0; k < which.size(); ++k) {
        const size_t i = which[k];
        if (!in[k]) in[k] = d_gather + gather_at[k];
        out[k] = stored(i) ? d_scan + scan_at[i] : nullptr;
        cap[k] = static_cast<size_t>(scan[i]);
      }
      const std::vector<zamd::InflateJob> jobs = zamd::InflateJobs(which.size(), in.data(), insize.data(), out.data(), cap.data());
      for (size_t r = 0; r < zamd::InflateRounds(which.size()); ++r) {
        size_t begin = 0, end = 0;
        zamd::InflateRound(which.size(), r, &begin, &end);
        if (const int rc = zmx_internal_inflate_run(c, ZOPFLI_FORMAT_ZLIB, end - begin, jobs.data() + begin, inflated.data())) return rc;
      }
      for (size_t k = 0; k < which.size(); ++k) zamd::PngStreamVerdict(inflated[k], scan[which[k]], &results[which[k]]);
      phase_done(2);
      // ---- the Adler-32s of what was stored, one launch pair
      std::vector<size_t> summed;
      std::vector<const void*> ptrs;
      std::vector<size_t> sizes;
      for (size_t k = 0; k < which.size(); ++k) {
        const size_t i = which[k];
        if (results[i].status != ZMX_PNG_DECODE_OK || !stored(i)) continue;
        summed.push_back(k);
        ptrs.push_back(d_scan + scan_at[i]);
        sizes.push_back(static_cast<size_t>(scan[i]));
      }
      if (!summed.empty()) {
        std::vector<uint32_t> values(summed.size());
        if (const int rc = RunChecksumDevice(c, ZMX_ADLER32, summed.size(), ptrs.data(), sizes.data(), nullptr, values.data())) return rc;
        for (size_t j = 0; j < summed.size(); ++j) {
          if (values[j] == inflated[summed[j]].stored_check) continue;
          results[which[summed[j]]].status = ZMX_PNG_DECODE_STREAM;
          results[which[summed[j]]].detail = ZMX_INFLATE_CHECKSUM;
        }
      }
    }
    phase_done(3);
    // ---- k_png_unfilter: the images that fit their destinations; the wide ones band by band
    std::vector<zamd::PngUnfilterJob> jobs[2];   // [0] the LDS carry, [1] the wide path
    size_t carry_total = 0;
    uint32_t wide_bands = 0;
    for (size_t i = 0; i < n; ++i) {
      if (results[i].status != ZMX_PNG_DECODE_OK || !stored(i)) continue;
      if (results[i].outsize > capacity[i]) {
        results[i].status = ZMX_PNG_DECODE_CAPACITY;
        continue;
      }
      zamd::PngUnfilterJob J;
      J.rec = rec[i];
      J.file = static_cast<const unsigned char*>(d_file[i]);
      J.scan = d_scan + scan_at[i];
      J.out = static_cast<unsigned char*>(d_out[i]);
      J.limit = results[i].outsize;
      J.carry[0] = J.carry[1] = nullptr;
      J.mode = static_cast<uint32_t>(mode);
      J.index = static_cast<uint32_t>(i);
      const size_t linebytes = static_cast<size_t>(zamd::PngLineBytes(rec[i].width, zamd::PngBpp(rec[i].colortype, rec[i].bitdepth)));
      const bool wide = force_wide || linebytes > zamd::kPngCarryBytes;
      if (wide) {
        J.carry[0] = reinterpret_cast<unsigned char*>(carry_total);   // (offsets until the rows are allocated)
        J.carry[1] = reinterpret_cast<unsigned char*>(carry_total + PngAlign16(linebytes));
        carry_total += 2 * PngAlign16(linebytes);
        wide_bands = std::max(wide_bands, (rec[i].height + zamd::kPngDecLanes - 1) / zamd::kPngDecLanes);
      }
      jobs[wide ? 1 : 0].push_back(J);
    }
    if (!jobs[1].empty()) {
      unsigned char* d_carry = nullptr;
      HIPCHK(tmp.AllocT(&d_carry, carry_total, "png_decode_carry"));
      for (zamd::PngUnfilterJob& J : jobs[1]) {
        J.carry[0] = d_carry + reinterpret_cast<uintptr_t>(J.carry[0]);
        J.carry[1] = d_carry + reinterpret_cast<uintptr_t>(J.carry[1]);
      }
    }
    std::vector<zamd::PngUnfilterResult> unf[2];
    zamd::PngUnfilterResult* d_unf[2] = {nullptr, nullptr};
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    for (int w = 0; w < 2; ++w) {
      if (jobs[w].empty()) continue;
      zamd::PngUnfilterJob* d_jobs = nullptr;
      HIPCHK(tmp.Upload(&d_jobs, jobs[w].data(), jobs[w].size(), "png_decode_jobs"));
      HIPCHK(tmp.AllocT(&d_unf[w], jobs[w].size(), "png_decode_unfiltered"));
      HIPCHK(hipMemsetAsync(d_unf[w], 0, jobs[w].size() * sizeof(zamd::PngUnfilterResult), c->stream));
      PngUnfilterParams P;
      P.jobs = d_jobs;
      P.results = d_unf[w];
      P.njobs = static_cast<u32>(jobs[w].size());
      const uint32_t launches = w == 0 ? 1 : wide_bands;
      for (uint32_t b = 0; b < launches; ++b) {
        P.band_first = b;
        P.band_count = w == 0 ? 0xffffffffu : 1;
        hipLaunchKernelGGL(k_png_unfilter, dim3(P.njobs), dim3(zamd::kPngDecLanes), 0, c->stream, P);
        KCHK(c, "k_png_unfilter");
      }
      unf[w].resize(jobs[w].size());
      HIPCHK(hipMemcpyAsync(unf[w].data(), d_unf[w], jobs[w].size() * sizeof(zamd::PngUnfilterResult), hipMemcpyDeviceToHost, c->stream));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (timed) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
      g_png_decode_ms[1] = t;
    }
    phase_done(4);
    for (int w = 0; w < 2; ++w) {
      for (size_t k = 0; k < jobs[w].size(); ++k) {
        if (unf[w][k].status == zamd::kPngDecOk) continue;
        results[jobs[w][k].index].status = unf[w][k].status;
        results[jobs[w][k].index].detail = unf[w][k].row;
      }
    }
    if (sinks) {
      // ---- k_png_unpack: every file that ended OK, one launch
      std::vector<zamd::PngUnpackJob> unpack;
      std::vector<uint32_t> unpack_palettes;
      for (size_t i = 0; i < n; ++i) {
        if (results[i].status == ZMX_PNG_DECODE_OK) PngUnpackAddJob(sinks[i], results[i], d_out[i], &unpack, &unpack_palettes);
      }
      if (const int rc = PngUnpackEnqueue(c, &tmp, unpack, unpack_palettes, false)) return rc;
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
  };
  if (const int rc = run()) {
    (void)hipStreamSynchronize(c->stream);   // (what was queued may still read the call's arrays: drained before `tmp` gives them back)
    return rc;
  }
  return 0;
}

// What the sink entries refuse of their sinks against their files: PngSinksCheck, and no extent may share a byte with a file.
int PngDecodeSinksCheck(zmx_ctx* c, const std::string& w, size_t n, const void* const* d_file, const size_t* filesize, const zmx_png_sink* sinks) {
  zamd::ApartRanges extents;
  if (const int rc = PngSinksCheck(c, w, n, sinks, &extents)) return rc;
  for (size_t i = 0; i < n; ++i) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_file[i]);
    size_t hit = 0;
    if (extents.Hit(at, at + filesize[i], &hit)) return FailMsg(w + ": sink " + std::to_string(hit) + ": its extent overlaps file " + std::to_string(i));
  }
  return 0;
}

}  // namespace

extern "C" {
void zmx_internal_png_decode_ms(double out[2]) {
  out[0] = g_png_decode_ms[0];
  out[1] = g_png_decode_ms[1];
}
void zmx_internal_png_decode_phase_ms(double out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = g_png_decode_phase_ms[i];
}

int zmx_internal_png_decode_run(zmx_ctx* c, const char* who, int mode, int info_only, size_t n, const void* const* d_file, const size_t* filesize,
                                void* const* d_out, const size_t* capacity, zmx_png_decode_result* results, const zmx_png_decode_hooks* hooks) {
  return PngDecodeRun(c, who, mode, info_only, n, d_file, filesize, d_out, capacity, nullptr, results, hooks);
}

int zmx_internal_png_decode_sink_run(zmx_ctx* c, const char* who, size_t n, const void* const* d_file, const size_t* filesize,
                                     const zmx_png_sink* sinks, zmx_png_decode_result* results, const zmx_png_decode_hooks* hooks) {
  if (n == 0) return 0;
  if (n > kPngDecodeMaxFiles) return FailMsg(std::string(who) + ": too many files for one call");
  if (const int rc = PngDecodeSinksCheck(c, who, n, d_file, filesize, sinks)) return rc;
  return PngDecodeRun(c, who, ZMX_PNG_DECODE_OWN, 0, n, d_file, filesize, nullptr, nullptr, sinks, results, hooks);
}

int zmx_png_decode_device_ctx(zmx_ctx* c, int mode, size_t n, const void* const* d_file, const size_t* filesize, void* const* d_out,
                              const size_t* capacity, zmx_png_decode_result* results, const zmx_png_decode_hooks* hooks) {
  static const char* const kWho = "zmx_png_decode_device_ctx";
  if (!c) return FailMsg("zmx_png_decode_device_ctx: no context");
  if (!zamd::PngDecodeModeOk(mode)) return FailMsg(std::string(kWho) + ": unknown mode " + std::to_string(mode));
  if (n == 0) return 0;
  if (!d_file || !filesize || !results || (d_out && !capacity)) return FailMsg("zmx_png_decode_device_ctx: null array");
  // ---- every range checked before anything is launched
  DeviceRangeChecker in_checker, out_checker;
  for (size_t i = 0; i < n; ++i) {
    int device = -1;
    const std::string w = std::string(kWho) + ": file " + std::to_string(i);
    if (filesize[i] != 0 && !d_file[i]) return FailMsg(w + ": null pointer with a non-zero size");
    if (const int rc = in_checker.Check(w.c_str(), d_file[i], filesize[i], &device)) return rc;
    if (device >= 0 && device != c->device) return FailMsg(w + " is not memory of the context's device");
    if (!d_out || !d_out[i]) continue;
    const std::string wo = std::string(kWho) + ": destination " + std::to_string(i);
    if (const int rc = out_checker.Check(wo.c_str(), d_out[i], capacity[i], &device)) return rc;
    if (device >= 0 && device != c->device) return FailMsg(wo + " is not memory of the context's device");
  }
  const std::string apart = zamd::CheckPngDecodeApart(kWho, n, d_file, filesize, d_out, capacity);
  if (!apart.empty()) return FailMsg(apart);
  std::vector<zmx_png_decode_result> got(n);
  if (const int rc = zmx_internal_png_decode_run(c, kWho, mode, 0, n, d_file, filesize, d_out, capacity, got.data(), hooks)) return rc;
  std::copy(got.begin(), got.end(), results);
  int error_class = ZMX_ERR_NONE;
  const std::string verdict = zamd::PngDecodeVerdict(kWho, n, results, d_out ? capacity : nullptr, &error_class);
  if (verdict.empty()) return 0;
  g_err = verdict;
  g_err_class = error_class;
  return -1;
}

int zmx_png_decode_sink_device_ctx(zmx_ctx* c, size_t n, const void* const* d_file, const size_t* filesize, const zmx_png_sink* sinks,
                                   zmx_png_decode_result* results, const zmx_png_decode_hooks* hooks) {
  static const char* const kWho = "zmx_png_decode_sink_device_ctx";
  if (!c) return FailMsg(std::string(kWho) + ": no context");
  if (n == 0) return 0;
  if (!d_file || !filesize || !sinks || !results) return FailMsg(std::string(kWho) + ": null array");
  DeviceRangeChecker in_checker;
  for (size_t i = 0; i < n; ++i) {
    int device = -1;
    const std::string w = std::string(kWho) + ": file " + std::to_string(i);
    if (filesize[i] != 0 && !d_file[i]) return FailMsg(w + ": null pointer with a non-zero size");
    if (const int rc = in_checker.Check(w.c_str(), d_file[i], filesize[i], &device)) return rc;
    if (device >= 0 && device != c->device) return FailMsg(w + " is not memory of the context's device");
  }
  std::vector<zmx_png_decode_result> got(n);
  if (const int rc = zmx_internal_png_decode_sink_run(c, kWho, n, d_file, filesize, sinks, got.data(), hooks)) return rc;
  std::copy(got.begin(), got.end(), results);
  int error_class = ZMX_ERR_NONE;
  const std::string verdict = zamd::PngDecodeVerdict(kWho, n, results, nullptr, &error_class);
  if (verdict.empty()) return 0;
  g_err = verdict;
  g_err_class = error_class;
  return -1;
}
}  // extern "C"
