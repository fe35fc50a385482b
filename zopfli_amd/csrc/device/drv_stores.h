// Driver part: the LZ77 stores of a table set — zmx_store_download, zmx_store_download_batch, zmx_verify_stores, zmx_encode_blocks.
// Needs drv_context.h (PoolScope, StageReserve) and drv_tables.h (zmx_tables, CheckTables, CheckStoreRef).
#pragma once

extern "C" {
// A store's symbols (u32 = litlen | dist << 16, zmx_kernels.h) as the reference's two u16 arrays.
static void UnpackSymbols(const u32* sym, size_t n, uint16_t* litlens, uint16_t* dists) {
  for (size_t i = 0; i < n; ++i) {
    litlens[i] = static_cast<uint16_t>(sym[i] & 0xffffu);
    dists[i] = static_cast<uint16_t>(sym[i] >> 16);
  }
}

int zmx_store_download(zmx_ctx* c, zmx_tables* t, size_t block, int slot, uint16_t* litlens, uint16_t* dists,
                       size_t nsym) {
  if (const int rc = CheckTables("zmx_store_download", t, zamd::kAnyTables)) return rc;
  if (const int rc = CheckStoreRef("zmx_store_download", t, block, slot, nsym)) return rc;
  if (nsym == 0) return 0;
  const u32 begin = t->store_begin[slot][block];
  DEVICE_ENTRY(c->device);
  std::vector<u32> tmp(nsym);
  HIPCHK(hipMemcpyAsync(tmp.data(), t->d_store[slot] + t->blocks[block].pos_off + begin, nsym * sizeof(u32),
                        hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  UnpackSymbols(tmp.data(), nsym, litlens, dists);
  return 0;
}

int zmx_store_download_batch(zmx_ctx* c, zmx_tables* t, size_t n, const size_t* block, const int32_t* slot,
                             const size_t* nsym, uint16_t* const* litlens, uint16_t* const* dists) {
  if (const int rc = CheckTables("zmx_store_download_batch", t, zamd::kAnyTables)) return rc;
  std::vector<size_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if (const int rc = CheckStoreRef("zmx_store_download_batch", t, block[i], slot[i], nsym[i])) return rc;
    off[i + 1] = off[i] + nsym[i];
  }
  if (off[n] == 0) return 0;
  DEVICE_ENTRY(c->device);
  if (const int rc = StageReserve(c, off[n])) return rc;
  // every store in one go into pinned memory, one synchronisation, then the split into the
  // reference's two u16 arrays on the host workers
  for (size_t i = 0; i < n; ++i) {
    if (nsym[i] == 0) continue;
    const u32* src = t->d_store[slot[i]] + t->blocks[block[i]].pos_off + t->store_begin[slot[i]][block[i]];
    HIPCHK(hipMemcpyAsync(c->h_stage + off[i], src, nsym[i] * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  const u32* stage = c->h_stage;
  zamd::ParallelFor(n, [&](size_t i) { UnpackSymbols(stage + off[i], nsym[i], litlens[i], dists[i]); });
  return 0;
}

int zmx_verify_stores(zmx_ctx* c, zmx_tables* t, size_t n, const size_t* block, const int32_t* slot, const size_t* nsym) {
  if (const int rc = CheckTables("zmx_verify_stores", t, zamd::kUntrimmed)) return rc;
  if (n == 0) return 0;
  std::vector<VerifyJob> vj(n);
  for (size_t i = 0; i < n; ++i) {
    if (const int rc = CheckStoreRef("zmx_verify_stores", t, block[i], slot[i], nsym[i])) return rc;
    vj[i].sym_off = t->blocks[block[i]].pos_off + t->store_begin[slot[i]][block[i]];
    vj[i].instart = t->blocks[block[i]].instart;
    vj[i].inend = t->blocks[block[i]].inend;
    vj[i].nsym = static_cast<u32>(nsym[i]);
    vj[i].slot = static_cast<u32>(slot[i]);
  }
  DEVICE_ENTRY(c->device);
  PoolScope tmp(c);
  VerifyJob* d_jobs = nullptr;
  u32* d_bad = nullptr;
  HIPCHK(tmp.Upload(&d_jobs, vj.data(), n, "d_jobs"));
  HIPCHK(tmp.AllocT(&d_bad, 2 * n, "d_bad"));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, 2 * n * sizeof(u32), c->stream));    // k_verify keeps the minimum: the first failure
  VerifyParams P;
  P.jobs = d_jobs;
  P.in = c->d_in;
  P.store[0] = t->d_store[0];
  P.store[1] = t->d_store[1];
  P.bad = d_bad;
  hipLaunchKernelGGL(k_verify, dim3(static_cast<unsigned>(n)), dim3(256), 0, c->stream, P);
  KCHK(c, "k_verify");
  std::vector<u32> bad(2 * n);
  HIPCHK(hipMemcpyAsync(bad.data(), d_bad, 2 * n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; ++i) {
    if (bad[2 * i] == 0xffffffffu) continue;
    static const char* why[4] = {"", "length or distance out of range", "the bytes it stands for are not the input's", "the symbols do not add up to the block"};
    char msg[200];
    std::snprintf(msg, sizeof(msg), "zmx_verify_stores: block %zu, symbol %u: %s", block[i], (bad[2 * i] >> 2) - 1, why[bad[2 * i] & 3]);
    return FailFault(msg);   // (the device found the parse wrong: another context may fare better)
  }
  return 0;
}

int zmx_encode_blocks(zmx_ctx* c, zmx_tables* t, size_t njobs, const zmx_enc_job* jobs, const uint32_t* codes,
                      unsigned char* const* out) {
  if (njobs == 0) return 0;
  if (const int rc = CheckTables("zmx_encode_blocks", t, zamd::kAnyTables)) return rc;
  std::vector<EncJob> ej(njobs);
  std::vector<u32> tile_job;
  std::vector<size_t> out_off(njobs + 1, 0);     // in the device / staging buffer, 8-byte aligned
  for (size_t j = 0; j < njobs; ++j) {
    const zmx_enc_job& q = jobs[j];
    if (const int rc = CheckStoreRef("zmx_encode_blocks", t, q.block, q.slot, q.nsym)) return rc;
    out_off[j + 1] = out_off[j] + (((q.bit_start + q.nbits + 7) / 8 + 8 + 7) & ~static_cast<size_t>(7));
    EncJob& e = ej[j];
    e.sym_off = t->blocks[q.block].pos_off + t->store_begin[q.slot][q.block];
    e.out_word = out_off[j] / 4;
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
  DEVICE_ENTRY(c->device);
  const size_t ntile = tile_job.size(), out_words = out_off[njobs] / 4;
  EncJob* d_jobs = nullptr;
  u32 *d_tile_job = nullptr, *d_codes = nullptr, *d_tile_bits = nullptr, *d_out = nullptr, *d_flag = nullptr;
  u64* d_tile_off = nullptr;
  PoolScope tmp(c);
  HIPCHK(tmp.Upload(&d_jobs, ej.data(), njobs, "d_jobs"));
  HIPCHK(tmp.Upload(&d_tile_job, tile_job.data(), ntile, "d_tile_job"));
  HIPCHK(tmp.Upload(&d_codes, codes, njobs * 320, "d_codes"));
  HIPCHK(tmp.AllocT(&d_tile_bits, ntile, "d_tile_bits"));
  HIPCHK(tmp.AllocT(&d_tile_off, ntile, "d_tile_off"));
  HIPCHK(tmp.AllocT(&d_out, out_words + 2, "d_out"));
  HIPCHK(tmp.AllocT(&d_flag, 4, "d_flag"));
  HIPCHK(hipMemsetAsync(d_out, 0, (out_words + 2) * sizeof(u32), c->stream));
  HIPCHK(hipMemsetAsync(d_flag, 0, 4 * sizeof(u32), c->stream));
  EncParams P;
  P.jobs = d_jobs;
  P.tile_job = d_tile_job;
  P.codes = d_codes;
  P.store[0] = t->d_store[0];
  P.store[1] = t->d_store[1];
  P.tile_bits = d_tile_bits;
  P.tile_off = d_tile_off;
  P.out = d_out;
  P.flags = d_flag;
  P.njobs = static_cast<u32>(njobs);
  hipLaunchKernelGGL(k_enc_len, dim3(static_cast<unsigned>(ntile)), dim3(ENC_THREADS), 0, c->stream, P);
  KCHK(c, "k_enc_len");
  hipLaunchKernelGGL(k_enc_scan, dim3(static_cast<unsigned>(njobs)), dim3(64), 0, c->stream, P);
  KCHK(c, "k_enc_scan");
  hipLaunchKernelGGL(k_enc_emit, dim3(static_cast<unsigned>(ntile)), dim3(ENC_THREADS), 0, c->stream, P);
  KCHK(c, "k_enc_emit");
  // down through the pinned staging buffer, then into the caller's memory on the host workers
  if (const int rc = StageReserve(c, out_words + 1)) return rc;
  u32 flag = 0;
  HIPCHK(hipMemcpyAsync(c->h_stage, d_out, out_words * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&flag, d_flag, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (flag) return FailMsg("zmx_encode_blocks: the symbols of a block take a different number of bits than the histogram says");
  const unsigned char* stage = reinterpret_cast<const unsigned char*>(c->h_stage);
  zamd::ParallelFor(njobs, [&](size_t j) {
    const size_t nby = static_cast<size_t>((jobs[j].bit_start + jobs[j].nbits + 7) / 8);
    std::memcpy(out[j], stage + out_off[j], nby);
  });
  return 0;
}
}  // extern "C"
