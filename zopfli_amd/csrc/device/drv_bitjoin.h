// Driver part: output that stays in device memory — zmx_bitjoin_device (k_bitjoin, zmx_bitjoin.h), zmx_bitjoin_many_device
// (k_bitjoin_many: many destinations, one launch), zmx_encode_blocks_device
// with zmx_bits_job / zmx_bits_free (the bit writer of drv_stores.h without the way down).
// Needs drv_context.h (PoolScope, PoolAllocT), drv_input.h (CheckDevicePointer), drv_tables.h
// (zmx_tables, CheckTables, CheckStoreRef, Refused).
#pragma once

static_assert(sizeof(zmx_bit_piece) == sizeof(zamd::BitPiece) && offsetof(zmx_bit_piece, src_bit) == offsetof(zamd::BitPiece, src_bit) &&
              offsetof(zmx_bit_piece, nbits) == offsetof(zamd::BitPiece, nbits) && offsetof(zmx_bit_piece, dst_bit) == offsetof(zamd::BitPiece, dst_bit),
              "zmx_bit_piece is the kernel's BitPiece");
static_assert(sizeof(zmx_bit_dest) == sizeof(zamd::BitDest) && offsetof(zmx_bit_dest, total_bits) == offsetof(zamd::BitDest, total_bits) &&
              offsetof(zmx_bit_dest, first_piece) == offsetof(zamd::BitDest, first_piece) && offsetof(zmx_bit_dest, npieces) == offsetof(zamd::BitDest, npieces),
              "zmx_bit_dest is the kernel's BitDest");
static_assert(zamd::kBitPieceMaxBits == zamd::kBitjoinMaxBits, "the entry check's limit is the kernel's");

// The bits of the jobs of one zmx_encode_blocks_device call, where the kernels wrote them.
struct zmx_bits {
  u32* d_out = nullptr;             // a pooled allocation of the context that made it
  std::vector<size_t> out_off;      // [njobs + 1] byte offset of every job's bits, 8-byte aligned
  std::vector<u32> bit_start;
  std::vector<u64> nbits;
};

// CheckDevicePointer for the sources of a piece table: a stream's pieces come from a handful of allocations in turn (the
// literals, a bit buffer per context, the input), so the runtime is asked once for each of them.
struct KnownRanges {
  struct Range { uintptr_t lo; size_t size; int device; };
  std::vector<Range> ranges;
  int Check(size_t piece, const void* p, size_t n, int* device_out) {
    return Check("zmx_bitjoin_device: piece " + std::to_string(piece), p, n, device_out);
  }
  int Check(const std::string& who, const void* p, size_t n, int* device_out) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(p);
    for (const Range& r : ranges) {
      if (at >= r.lo && at - r.lo <= r.size && n <= r.size - (at - r.lo)) {
        *device_out = r.device;
        return 0;
      }
    }
    uintptr_t lo = 0;
    size_t size = 0;
    if (const int rc = CheckDevicePointer(who.c_str(), p, n, device_out, &lo, &size)) return rc;
    if (ranges.size() < 64) ranges.push_back({lo, size, *device_out});
    return 0;
  }
};

extern "C" {
static thread_local double g_bitjoin_ms = 0;   // (zmx_internal_bitjoin_ms)
double zmx_internal_bitjoin_ms(void) { return g_bitjoin_ms; }

int zmx_bitjoin_device(zmx_ctx* c, size_t n, const zmx_bit_piece* pieces, uint64_t total_bits, void* d_dst, size_t dst_capacity) {
  static const char* const kWho = "zmx_bitjoin_device";
  g_bitjoin_ms = 0;
  if (!c) return FailMsg("zmx_bitjoin_device: no context");
  if (const int rc = Refused(zamd::CheckBitPieces(kWho, n, pieces, total_bits, dst_capacity))) return rc;
  if (total_bits == 0) return 0;
  // ---- every range checked before anything is launched
  const size_t dst_bytes = static_cast<size_t>((total_bits + 7) / 8);
  int dst_device = -1;
  if (const int rc = CheckDevicePointer("zmx_bitjoin_device: the destination", d_dst, dst_bytes, &dst_device)) return rc;
  if (dst_device != c->device) return FailMsg("zmx_bitjoin_device: the destination is not memory of the context's device");
  KnownRanges known;
  const uintptr_t dlo = reinterpret_cast<uintptr_t>(d_dst);
  for (size_t i = 0; i < n; ++i) {
    if (pieces[i].nbits == 0) continue;
    uintptr_t lo = 0, hi = 0;
    zamd::BitPieceBytes(pieces[i], &lo, &hi);
    int device = -1;
    // (from src itself: the string begins inside the allocation that its bits lie in)
    if (const int rc = known.Check(i, pieces[i].src, hi - reinterpret_cast<uintptr_t>(pieces[i].src), &device)) return rc;
    if (device != c->device) return FailMsg("zmx_bitjoin_device: piece " + std::to_string(i) + ": the source is not memory of the context's device");
    if (const int rc = Refused(zamd::CheckBitPieceApart(kWho, i, dlo, dst_bytes, lo, hi))) return rc;
  }
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (the table: held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  const auto enqueue = [&]() -> int {
    zmx_bit_piece* d_pieces = nullptr;
    HIPCHK(tmp.Upload(&d_pieces, pieces, n, "bitjoin_pieces"));
    zamd::BitjoinTable T;
    T.piece = reinterpret_cast<const zamd::BitPiece*>(d_pieces);
    T.n = n;
    T.dst = static_cast<unsigned char*>(d_dst);
    T.total_bits = total_bits;
    // (the grid: tiles of the destination up to the cap, whatever n and the total)
    const uint64_t nvec = zamd::BitjoinVectors(T.dst, total_bits);
    const uint64_t ntiles = (nvec + zamd::kBitjoinTileVecs - 1) / zamd::kBitjoinTileVecs;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(ntiles, zamd::kBitjoinMaxBlocks));
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_bitjoin, dim3(grid), dim3(zamd::kBitjoinThreads), 0, c->stream, T, ntiles);
    KCHK(c, "k_bitjoin");
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    return 0;
  };
  if (const int rc = enqueue()) {
    (void)hipStreamSynchronize(c->stream);   // (what was queued may still read the table: drained before `tmp` gives it back)
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_bitjoin_ms = ms;
  }
  return 0;
}

int zmx_internal_bitjoin_literals(zmx_ctx* c, const unsigned char* literals, size_t nliterals, size_t n, zmx_bit_piece* pieces,
                                  const unsigned char* is_literal, uint64_t total_bits, void* d_dst, size_t dst_capacity) {
  unsigned char* d_literals = nullptr;
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (zmx_bitjoin_device drains the stream before it returns, on its failing paths too)
  HIPCHK(tmp.Upload(&d_literals, literals, nliterals, "bitjoin_literals"));
  for (size_t i = 0; i < n; ++i) {
    if (is_literal[i]) pieces[i].src = d_literals + reinterpret_cast<uintptr_t>(pieces[i].src);
  }
  const int rc = zmx_bitjoin_device(c, n, pieces, total_bits, d_dst, dst_capacity);
  if (rc) (void)hipStreamSynchronize(c->stream);   // (a refusal launches nothing: the upload may still be on its way)
  return rc;
}

int zmx_bitjoin_many_device(zmx_ctx* c, size_t ndst, const zmx_bit_dest* dests, const size_t* capacity, size_t npieces,
                            const zmx_bit_piece* pieces) {
  static const char* const kWho = "zmx_bitjoin_many_device";
  g_bitjoin_ms = 0;
  if (!c) return FailMsg("zmx_bitjoin_many_device: no context");
  if (const int rc = Refused(zamd::CheckBitDests(kWho, ndst, dests, capacity, npieces, pieces))) return rc;
  // ---- every range checked before anything is uploaded or launched; the tiles of every destination
  KnownRanges known;
  std::vector<uint64_t> tile_start(ndst + 1, 0);
  for (size_t d = 0; d < ndst; ++d) {
    const zmx_bit_dest& e = dests[d];
    const std::string dest = std::string(kWho) + ": destination " + std::to_string(d);
    const unsigned char* dst = static_cast<const unsigned char*>(e.dst);
    tile_start[d + 1] = tile_start[d] + zamd::BitjoinTiles(dst, e.total_bits);
    if (e.total_bits == 0) continue;     // (its pieces are all empty: nothing is read or written)
    int device = -1;
    if (const int rc = known.Check(dest, e.dst, static_cast<size_t>((e.total_bits + 7) / 8), &device)) return rc;
    if (device != c->device) return FailMsg(dest + " is not memory of the context's device");
    for (uint64_t i = 0; i < e.npieces; ++i) {
      const zmx_bit_piece& q = pieces[e.first_piece + i];
      if (q.nbits == 0) continue;
      uintptr_t lo = 0, hi = 0;
      zamd::BitPieceBytes(q, &lo, &hi);
      const std::string piece = dest + ": piece " + std::to_string(i);
      if (const int rc = known.Check(piece, q.src, hi - reinterpret_cast<uintptr_t>(q.src), &device)) return rc;
      if (device != c->device) return FailMsg(piece + ": the source is not memory of the context's device");
    }
  }
  const uint64_t ntiles = tile_start[ndst];
  if (ntiles == 0) return 0;
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (the tables: held until the stream is drained, on the failing paths too — below)
  const bool timed = KernelTiming();
  const auto enqueue = [&]() -> int {
    zmx_bit_piece* d_pieces = nullptr;
    zmx_bit_dest* d_dests = nullptr;
    uint64_t* d_tile_start = nullptr;
    HIPCHK(tmp.Upload(&d_pieces, pieces, npieces, "bitjoin_pieces"));
    HIPCHK(tmp.Upload(&d_dests, dests, ndst, "bitjoin_dests"));
    HIPCHK(tmp.Upload(&d_tile_start, tile_start.data(), ndst + 1, "bitjoin_tile_start"));
    zamd::BitjoinManyTable M;
    M.piece = reinterpret_cast<const zamd::BitPiece*>(d_pieces);
    M.dest = reinterpret_cast<const zamd::BitDest*>(d_dests);
    M.tile_start = d_tile_start;
    M.ndst = ndst;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(ntiles, zamd::kBitjoinMaxBlocks));
    if (timed) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_bitjoin_many, dim3(grid), dim3(zamd::kBitjoinThreads), 0, c->stream, M, ntiles);
    KCHK(c, "k_bitjoin_many");
    if (timed) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    return 0;
  };
  if (const int rc = enqueue()) {
    (void)hipStreamSynchronize(c->stream);   // (what was queued may still read the tables: drained before `tmp` gives them back)
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    g_bitjoin_ms = ms;
  }
  return 0;
}

int zmx_internal_bitjoin_many_literals(zmx_ctx* c, const unsigned char* literals, size_t nliterals, size_t ndst, const zmx_bit_dest* dests,
                                       const size_t* capacity, size_t npieces, zmx_bit_piece* pieces, const unsigned char* is_literal) {
  unsigned char* d_literals = nullptr;
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);   // (zmx_bitjoin_many_device drains the stream before it returns, on its failing paths too)
  HIPCHK(tmp.Upload(&d_literals, literals, nliterals, "bitjoin_literals"));
  for (size_t i = 0; i < npieces; ++i) {
    if (is_literal[i]) pieces[i].src = d_literals + reinterpret_cast<uintptr_t>(pieces[i].src);
  }
  const int rc = zmx_bitjoin_many_device(c, ndst, dests, capacity, npieces, pieces);
  (void)hipStreamSynchronize(c->stream);   // (a refusal, or a join of no tile, launches nothing: the upload may still be on its way)
  return rc;
}

void zmx_bits_free(zmx_ctx* c, zmx_bits* bits) {
  if (!bits) return;
  if (bits->d_out) {
    if (c) {
      DeviceGuard dev_guard(c->device);
      PoolFree(c, bits->d_out);
    } else {
      PoolFree(nullptr, bits->d_out);
    }
  }
  delete bits;
}

size_t zmx_bits_jobs(const zmx_bits* bits) { return bits ? bits->nbits.size() : 0; }

int zmx_bits_job(const zmx_bits* bits, size_t job, const void** d_bits, uint64_t* bit_start, uint64_t* nbits) {
  if (!bits || job >= bits->nbits.size()) return FailMsg("zmx_bits_job: no such job");
  if (d_bits) *d_bits = reinterpret_cast<const unsigned char*>(bits->d_out) + bits->out_off[job];
  if (bit_start) *bit_start = bits->bit_start[job];
  if (nbits) *nbits = bits->nbits[job];
  return 0;
}

// zmx_encode_blocks (drv_stores.h) — the same jobs, the same three kernels, the same nbits check — into an allocation that
// outlives the call; nothing comes down but the flag.
int zmx_encode_blocks_device(zmx_ctx* c, zmx_tables* t, size_t njobs, const zmx_enc_job* jobs, const uint32_t* codes,
                             zmx_bits** out) {
  if (!out) return FailMsg("zmx_encode_blocks_device: null argument");
  *out = nullptr;
  if (njobs != 0) {
    if (const int rc = CheckTables("zmx_encode_blocks_device", t, zamd::kAnyTables)) return rc;
  }
  std::unique_ptr<zmx_bits> bits(new zmx_bits());
  std::vector<EncJob> ej(njobs);
  std::vector<u32> tile_job;
  bits->out_off.assign(njobs + 1, 0);
  for (size_t j = 0; j < njobs; ++j) {
    const zmx_enc_job& q = jobs[j];
    if (const int rc = CheckStoreRef("zmx_encode_blocks_device", t, q.block, q.slot, q.nsym)) return rc;
    bits->out_off[j + 1] = bits->out_off[j] + (((q.bit_start + q.nbits + 7) / 8 + 8 + 7) & ~static_cast<size_t>(7));
    bits->bit_start.push_back(q.bit_start);
    bits->nbits.push_back(q.nbits);
    EncJob& e = ej[j];
    e.sym_off = t->blocks[q.block].pos_off + t->store_begin[q.slot][q.block];
    e.out_word = bits->out_off[j] / 4;
    e.nbits = q.nbits;
    e.nsym = q.nsym;
    e.slot = static_cast<u32>(q.slot);
    e.bit_start = q.bit_start;
    e.tile0 = static_cast<u32>(tile_job.size());
    e.code = static_cast<u32>(j);
    e.pad = 0;
    const u32 ntiles = q.nsym / ENC_TILE + 1;
    for (u32 k = 0; k < ntiles; ++k) tile_job.push_back(static_cast<u32>(j));
  }
  if (njobs == 0) {
    *out = bits.release();
    return 0;
  }
  DEVICE_ENTRY(c->device);
  const size_t ntile = tile_job.size(), out_words = bits->out_off[njobs] / 4;
  // the bits first: whichever way the call ends below, they go back to the pool after the stream is drained
  struct Drained {
    zmx_ctx* c; std::unique_ptr<zmx_bits>* bits; bool keep = false;
    ~Drained() {
      if (keep) return;
      (void)hipStreamSynchronize(c->stream);
      if ((*bits)->d_out) PoolFree(c, (*bits)->d_out);
      (*bits)->d_out = nullptr;
    }
  };
  HIPCHK(PoolAllocT(c, &bits->d_out, out_words + 2, "d_bits"));
  Drained drained{c, &bits};
  EncJob* d_jobs = nullptr;
  u32 *d_tile_job = nullptr, *d_codes = nullptr, *d_tile_bits = nullptr, *d_flag = nullptr;
  u64* d_tile_off = nullptr;
  PoolScope tmp(c);
  HIPCHK(tmp.Upload(&d_jobs, ej.data(), njobs, "d_jobs"));
  HIPCHK(tmp.Upload(&d_tile_job, tile_job.data(), ntile, "d_tile_job"));
  HIPCHK(tmp.Upload(&d_codes, codes, njobs * 320, "d_codes"));
  HIPCHK(tmp.AllocT(&d_tile_bits, ntile, "d_tile_bits"));
  HIPCHK(tmp.AllocT(&d_tile_off, ntile, "d_tile_off"));
  HIPCHK(tmp.AllocT(&d_flag, 4, "d_flag"));
  HIPCHK(hipMemsetAsync(bits->d_out, 0, (out_words + 2) * sizeof(u32), c->stream));
  HIPCHK(hipMemsetAsync(d_flag, 0, 4 * sizeof(u32), c->stream));
  EncParams P;
  P.jobs = d_jobs;
  P.tile_job = d_tile_job;
  P.codes = d_codes;
  P.store[0] = t->d_store[0];
  P.store[1] = t->d_store[1];
  P.tile_bits = d_tile_bits;
  P.tile_off = d_tile_off;
  P.out = bits->d_out;
  P.flags = d_flag;
  P.njobs = static_cast<u32>(njobs);
  hipLaunchKernelGGL(k_enc_len, dim3(static_cast<unsigned>(ntile)), dim3(ENC_THREADS), 0, c->stream, P);
  KCHK(c, "k_enc_len");
  hipLaunchKernelGGL(k_enc_scan, dim3(static_cast<unsigned>(njobs)), dim3(64), 0, c->stream, P);
  KCHK(c, "k_enc_scan");
  hipLaunchKernelGGL(k_enc_emit, dim3(static_cast<unsigned>(ntile)), dim3(ENC_THREADS), 0, c->stream, P);
  KCHK(c, "k_enc_emit");
  u32 flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, d_flag, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (flag) return FailMsg("zmx_encode_blocks_device: the symbols of a block take a different number of bits than the histogram says");
  drained.keep = true;
  *out = bits.release();
  return 0;
}
}  // extern "C"
