// Driver part: the parity probes — zmx_match_digest (its kernel k_rec_digest: zmx_probe.h), zmx_find_longest_match,
// zmx_hash_links_download, zmx_length_array_download, zmx_dp_rows_download, zmx_chain_tasks_download.  Needs drv_context.h (PoolScope) and drv_tables.h (zmx_tables, the checks).
#pragma once

extern "C" {
int zmx_match_digest(zmx_ctx* c, zmx_tables* t, uint64_t* out2) {
  if (!t || t->trimmed || !t->d_recs) return FailMsg("zmx_match_digest: no match records in these tables");
  DEVICE_ENTRY(c->device);
  out2[0] = out2[1] = 0;
  if (t->nb == 0) return 0;
  PoolScope tmp(c);
  unsigned long long* d_out = nullptr;
  HIPCHK(tmp.AllocT(&d_out, 2, "d_digest"));
  HIPCHK(hipMemsetAsync(d_out, 0, 2 * sizeof(unsigned long long), c->stream));
  u64 max_b = 0;
  for (size_t b = 0; b < t->nb; ++b) max_b = std::max<u64>(max_b, t->bsize[b]);
  const unsigned gx = static_cast<unsigned>(std::min<u64>(std::max<u64>((max_b + 256 * 8 - 1) / (256 * 8), 1), 2048));
  hipLaunchKernelGGL(k_rec_digest, dim3(gx, static_cast<unsigned>(t->nb)), dim3(256), 0, c->stream, t->d_blocks, t->d_recs, t->d_pool, d_out);
  KCHK(c, "k_rec_digest");
  HIPCHK(hipMemcpyAsync(out2, d_out, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int zmx_find_longest_match(zmx_ctx* c, zmx_tables* t, size_t block, size_t pos, uint16_t* sublen,
                           uint16_t* distance, uint16_t* length) {
  if (const int rc = CheckTables("zmx_find_longest_match", t, zamd::kUntrimmed)) return rc;
  if (const int rc = CheckBlock("zmx_find_longest_match", t, block)) return rc;
  const BlockDesc& d = t->blocks[block];
  if (pos < d.instart || pos >= d.inend) return FailMsg("zmx_find_longest_match: pos outside the block");
  DEVICE_ENTRY(c->device);
  if (t->probe_recs.empty()) t->probe_recs.resize(t->nb);
  std::vector<u32>& recs = t->probe_recs[block];
  if (recs.empty()) {
    recs.resize(static_cast<size_t>(t->bsize[block]) * 8);
    HIPCHK(hipMemcpy(recs.data(), t->d_recs + d.pos_off * 8, recs.size() * sizeof(u32), hipMemcpyDeviceToHost));
  }
  const u32* r = &recs[(pos - d.instart) * 8];
  *length = static_cast<uint16_t>(zamd::RecLength(r[0]));
  *distance = static_cast<uint16_t>(zamd::RecDist(r[0]));
  if (!sublen) return 0;
  if (zamd::RecIsOverflow(r[1]) && !t->probe_pool_ready) {
    u32 used = 0;
    HIPCHK(hipMemcpy(&used, t->d_counters, sizeof(u32), hipMemcpyDeviceToHost));
    t->probe_pool.resize(used);
    if (used) HIPCHK(hipMemcpy(t->probe_pool.data(), t->d_pool, used * sizeof(u32), hipMemcpyDeviceToHost));
    t->probe_pool_ready = true;
  }
  unsigned prev = 2;  // sublen[3..] only; the reference also fills sublen[2] for 2-byte hits, which nobody reads
  zamd::RecWalkCps(r, t->probe_pool.data(), [&](u32 len, u32 dist) {
    for (unsigned l = prev + 1; l <= len; ++l) sublen[l] = static_cast<uint16_t>(dist);
    prev = len;
  });
  return 0;
}

int zmx_hash_links_download(zmx_ctx* c, zmx_tables* t, size_t block, uint16_t* same, uint16_t* prev1, uint16_t* prev2) {
  if (const int rc = CheckTables("zmx_hash_links_download", t, zamd::kUntrimmed)) return rc;
  if (const int rc = CheckBlock("zmx_hash_links_download", t, block)) return rc;
  DEVICE_ENTRY(c->device);
  if (t->links_partial) return FailMsg("zmx_hash_links_download: tables built from a parent hold the hash arrays only near the block ends");
  const BlockDesc& d = t->blocks[block];
  const size_t n = static_cast<size_t>(d.inend - d.ws);
  std::vector<ushort4> lk(n);
  if (n) HIPCHK(hipMemcpy(lk.data(), t->d_links + d.reg_off, n * sizeof(ushort4), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    prev1[i] = lk[i].x;
    prev2[i] = lk[i].y;
    same[i] = lk[i].z;
  }
  return 0;
}

int zmx_length_array_download(zmx_ctx* c, zmx_tables* t, size_t block, uint16_t* out) {
  if (const int rc = CheckTables("zmx_length_array_download", t, zamd::kUntrimmed)) return rc;
  if (const int rc = CheckBlock("zmx_length_array_download", t, block)) return rc;
  DEVICE_ENTRY(c->device);
  HIPCHK(hipMemcpy(out, t->d_la + t->blocks[block].la_off, (static_cast<size_t>(t->bsize[block]) + 1) * sizeof(u16),
                   hipMemcpyDeviceToHost));
  return 0;
}

int zmx_dp_rows_download(zmx_ctx* c, zmx_tables* t, size_t block, uint64_t* block_edges, uint32_t* dph, uint16_t* codes,
                         uint32_t* winflag, uint32_t* winroff, uint32_t* wmeta) {
  if (const int rc = CheckTables("zmx_dp_rows_download", t, zamd::kWithDp)) return rc;
  if (const int rc = CheckBlock("zmx_dp_rows_download", t, block)) return rc;
  DEVICE_ENTRY(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));
  const BlockDesc& d = t->blocks[block];
  const size_t B = t->bsize[block];
  u64 edges = 0, code_base = 0;
  HIPCHK(hipMemcpy(&edges, t->d_block_edges + block, sizeof(u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&code_base, t->d_code_base + block, sizeof(u64), hipMemcpyDeviceToHost));
  *block_edges = edges;
  if (dph && B) HIPCHK(hipMemcpy(dph, t->d_dph + d.pos_off, B * sizeof(uint2), hipMemcpyDeviceToHost));
  if (codes && edges) HIPCHK(hipMemcpy(codes, t->d_codes + code_base, edges * sizeof(u16), hipMemcpyDeviceToHost));
  const size_t w0 = t->win_off[block], nw = t->win_off[block + 1] - w0;
  if (winflag) HIPCHK(hipMemcpy(winflag, t->d_winflag + w0, nw * sizeof(u32), hipMemcpyDeviceToHost));
  if (winroff) HIPCHK(hipMemcpy(winroff, t->d_winroff + w0, nw * sizeof(u32), hipMemcpyDeviceToHost));
  if (wmeta) HIPCHK(hipMemcpy(wmeta, t->d_wmeta + w0 * D5_WM, nw * D5_WM * sizeof(u32), hipMemcpyDeviceToHost));
  return 0;
}

int zmx_chain_tasks_download(zmx_ctx* c, zmx_tables* t, uint64_t* counts4, uint32_t* tasks, uint32_t* task_off, uint32_t* wg_tasks,
                             uint32_t* wg_desc) {
  if (const int rc = CheckTables("zmx_chain_tasks_download", t, zamd::kWithDp)) return rc;
  DEVICE_ENTRY(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));
  // (every task is in exactly one of the two lists: BuildWorkgroupLists)
  const size_t nt = t->tasks.size(), nwg = static_cast<size_t>(t->n_wg) + t->n_wg_runs;
  counts4[0] = nt;
  counts4[1] = t->merged_tasks;
  counts4[2] = t->n_wg;
  counts4[3] = t->n_wg_runs;
  static_assert(sizeof(SegTask) == 4 * sizeof(u32) && sizeof(uint2) == 2 * sizeof(u32), "the caller's rows");
  if (tasks && nt) HIPCHK(hipMemcpy(tasks, t->d_tasks, nt * sizeof(SegTask), hipMemcpyDeviceToHost));
  if (task_off && t->nb) HIPCHK(hipMemcpy(task_off, t->d_task_off, (t->nb + 1) * sizeof(u32), hipMemcpyDeviceToHost));
  if (wg_tasks && nwg) HIPCHK(hipMemcpy(wg_tasks, t->d_wg_tasks, nt * sizeof(u32), hipMemcpyDeviceToHost));
  if (wg_desc && nwg) HIPCHK(hipMemcpy(wg_desc, t->d_wg_desc, nwg * sizeof(uint2), hipMemcpyDeviceToHost));
  return 0;
}
}  // extern "C"
