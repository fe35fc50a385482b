// TEST-ONLY implementation of the zmx_* device layer on top of oracle/.
//
// Linked (by tests/hostlib/Makefile) with the product's host sources into
// tests/_build/libzopfli_hosttest.so so that the host logic (block splitter,
// block cost model, iteration control, encoder, containers) can be checked
// against the real reference on machines without a GPU.  The product library
// libzopfli_amd.so never links this file: its zmx_* symbols come from the HIP
// device layer only.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zopfli_amd.h"
#include "block_cost.h"
#include "block_split.h"
#include "checksum.h"
#include "entry_checks.h"
#include "huffman.h"
#include "lz77_store.h"
#include "symbol_check.h"
#include "zmx_internal.h"
extern "C" {
#include "zopfli_oracle.h"
}

struct zmx_ctx {
  std::vector<unsigned char> input;
};

struct BlockData {
  zmx_block blk;
  zo_table* table = nullptr;
  std::vector<uint16_t> litlens[2], dists[2];
  size_t nsym[2] = {0, 0};
  std::vector<uint16_t> length_array;
};

struct zmx_tables {
  std::vector<BlockData> blocks;
  bool matches_only = false, trimmed = false;   // (what zmx_trace_length_arrays refuses, as the device layer does)
};

static thread_local std::string g_err;
static thread_local int g_err_class = ZMX_ERR_NONE;   // what kind of failure g_err is (zmx_last_error_class)

static int Fail(const std::string& m) {
  zmx_internal_set_error(m.c_str(), ZMX_ERR_DEVICE);
  return -1;
}
// The entry checks are the device layer's own (host/entry_checks.h): a message they return is a refusal.
static int Refuse(const std::string& refusal) {
  if (refusal.empty()) return 0;
  zmx_internal_set_error(refusal.c_str(), ZMX_ERR_REFUSED);
  return -1;
}
static int CheckTables(const char* who, const zmx_tables* t, zamd::TableNeeds needs) {
  return Refuse(zamd::CheckTables(who, t != nullptr, t && t->trimmed, t && t->matches_only, needs));
}
static int CheckBlock(const char* who, const zmx_tables* t, size_t block) {
  return Refuse(zamd::CheckBlock(who, t->blocks.size(), block));
}
static int CheckStoreRef(const char* who, const zmx_tables* t, size_t block, int slot, size_t nsym) {
  return Refuse(zamd::CheckStoreRef(who, t->blocks.size(), block, slot, nsym, [&] { return t->blocks[block].nsym[slot]; }));
}

extern "C" {

// (ZOPFLI_HOSTTEST_DEVICES pretends to that many devices: the multi-device sharding of api.cc on CPU)
int zmx_device_count(void) {
  const char* e = std::getenv("ZOPFLI_HOSTTEST_DEVICES");
  return e ? std::atoi(e) : 1;
}
const char* zmx_last_error(void) { return g_err.c_str(); }
int zmx_has_experiments(void) { return 0; }
void zmx_set_kernel_timing(int) {}
int zmx_last_error_class(void) { return g_err_class; }
void zmx_internal_set_error(const char* msg, int cls) { g_err = msg; g_err_class = cls; }

int zmx_ctx_create(int, zmx_ctx** ctx) {
  *ctx = new zmx_ctx();
  return 0;
}
void zmx_ctx_destroy(zmx_ctx* ctx) { delete ctx; }

int zmx_set_input(zmx_ctx* ctx, const unsigned char* in, size_t insize) {
  ctx->input.assign(in, in + insize);
  return 0;
}
size_t zmx_internal_input_size(zmx_ctx* ctx) { return ctx->input.size(); }
const unsigned char* zmx_internal_input_host(zmx_ctx* ctx) { return ctx->input.data(); }
// (every input stays on the host: nothing to fetch.  No kernels either: nothing adds to the statistics, they read zeros.)
int zmx_internal_input_fetch(zmx_ctx*, size_t, size_t, unsigned char*) {
  return Fail("stored block of a device input: this build cannot fetch its bytes");
}
int zmx_hash_links_download(zmx_ctx*, zmx_tables*, size_t, uint16_t*, uint16_t*, uint16_t*) { return Fail("not in the host test library"); }
int zmx_dp_rows_download(zmx_ctx*, zmx_tables*, size_t, uint64_t*, uint32_t*, uint16_t*, uint32_t*, uint32_t*, uint32_t*) { return Fail("not in the host test library"); }
int zmx_chain_tasks_download(zmx_ctx*, zmx_tables*, uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*) { return Fail("not in the host test library"); }
int zmx_match_digest(zmx_ctx*, zmx_tables*, uint64_t*) { return Fail("not in the host test library"); }
int zmx_set_match_kernel(int) { return 0; }   // (no kernels here)
void zmx_set_oom_hook(zmx_oom_hook_t) {}
int zmx_ctx_set_share(zmx_ctx*, unsigned) { return 0; }
int zmx_ctx_trim_cache(zmx_ctx*) { return 0; }
int zmx_ctx_set_priority(zmx_ctx*, int) { return 0; }
int zmx_png_filter_types(zmx_ctx*, const unsigned char*, size_t, size_t, size_t, unsigned char*, unsigned char*) { return Fail("not in the host test library"); }
// (the RCCL gather of dist.cc is not part of the host-logic test library)
int zmx_dist_unique_id(unsigned char*) { return Fail("no RCCL in the host test library"); }
int zmx_dist_init(zmx_ctx*, int, int, const unsigned char*, zmx_dist**) { return Fail("no RCCL in the host test library"); }
void zmx_dist_destroy(zmx_dist*) {}
int zmx_dist_comm_count(zmx_dist*) { return -1; }
int zmx_dist_gather(zmx_dist*, const unsigned char*, size_t, unsigned char**, size_t*) { return Fail("no RCCL in the host test library"); }

int zmx_tables_build(zmx_ctx* ctx, const zmx_block* blocks, size_t nblocks, zmx_tables** tables) {
  zmx_tables* t = new zmx_tables();
  t->blocks.resize(nblocks);
  for (size_t b = 0; b < nblocks; ++b) {
    BlockData& d = t->blocks[b];
    d.blk = blocks[b];
    d.table = zo_table_build(ctx->input.data(), blocks[b].instart, blocks[b].inend);
    const size_t B = blocks[b].inend - blocks[b].instart;
    for (int s = 0; s < 2; ++s) {
      d.litlens[s].resize(B + 1);
      d.dists[s].resize(B + 1);
    }
    d.length_array.resize(B + 1);
  }
  *tables = t;
  return 0;
}

int zmx_tables_trim(zmx_ctx*, zmx_tables* t) { t->trimmed = true; return 0; }

int zmx_tables_build_matches(zmx_ctx* ctx, const zmx_block* blocks, size_t nblocks, zmx_tables** tables) {
  const int rc = zmx_tables_build(ctx, blocks, nblocks, tables);
  if (rc == 0) (*tables)->matches_only = true;
  return rc;
}

int zmx_tables_build_from(zmx_ctx* ctx, zmx_tables*, const zmx_block* blocks, size_t nblocks, zmx_tables** tables) {
  return zmx_tables_build(ctx, blocks, nblocks, tables);
}

void zmx_tables_free(zmx_ctx*, zmx_tables* t) {
  if (!t) return;
  for (auto& d : t->blocks) zo_table_free(d.table);
  delete t;
}

int zmx_lz77_greedy(zmx_ctx*, zmx_tables* t, int slot, uint32_t* nsym, uint32_t* hist) {
  if (const int rc = CheckTables("zmx_lz77_greedy", t, zamd::kUntrimmed)) return rc;
  for (size_t b = 0; b < t->blocks.size(); ++b) {
    BlockData& d = t->blocks[b];
    d.nsym[slot] = zo_greedy(d.table, d.litlens[slot].data(), d.dists[slot].data());
    nsym[b] = static_cast<uint32_t>(d.nsym[slot]);
    zo_histogram(d.litlens[slot].data(), d.dists[slot].data(), d.nsym[slot], hist + b * ZMX_HIST);
  }
  return 0;
}

int zmx_squeeze_run(zmx_ctx*, zmx_tables* t, const double* cost, const double* mincost, const int32_t* slot,
                    uint32_t* nsym, uint32_t* hist) {
  if (const int rc = CheckTables("zmx_squeeze_run", t, zamd::SqueezeRunNeeds(t ? t->blocks.size() : 0))) return rc;
  for (size_t b = 0; b < t->blocks.size(); ++b) {
    BlockData& d = t->blocks[b];
    const int s = slot[b];
    const double* ll = cost + b * ZMX_HIST;
    zo_get_best_lengths(d.table, ll, ll + ZMX_NUM_LL, mincost[b], d.length_array.data());
    d.nsym[s] = zo_trace_follow(d.table, d.length_array.data(), d.litlens[s].data(), d.dists[s].data());
    nsym[b] = static_cast<uint32_t>(d.nsym[s]);
    zo_histogram(d.litlens[s].data(), d.dists[s].data(), d.nsym[s], hist + b * ZMX_HIST);
  }
  return 0;
}

// (CPU stand-in for the trace kernels on given length arrays: the device layer's refusals by the same rule, then a plain
// backward walk over the oracle's table.  Like the device it steps over a 0 as over a 1 and reports it (flag 2), and
// reports a length the record at the symbol's start does not hold (flag 4).)
int zmx_trace_length_arrays(zmx_ctx*, zmx_tables* t, size_t nblocks, const uint16_t* const* length_arrays,
                            const size_t* entries, const int32_t* slot, uint32_t* nsym, uint32_t* hist) {
  if (const int rc = CheckTables("zmx_trace_length_arrays", t, zamd::kWithDp)) return rc;
  auto bsize = [&](size_t b) { return t->blocks[b].blk.inend - t->blocks[b].blk.instart; };
  if (const int rc = Refuse(zamd::CheckLengthArrays("zmx_trace_length_arrays", t->blocks.size(), bsize, nblocks, length_arrays,
                                                    entries, slot))) return rc;
  unsigned flags = 0;
  std::vector<std::vector<uint16_t>> path(nblocks);
  for (size_t b = 0; b < nblocks; ++b) {
    BlockData& d = t->blocks[b];
    const size_t B = d.blk.inend - d.blk.instart;
    d.length_array.assign(length_arrays[b], length_arrays[b] + B + 1);
    path[b] = d.length_array;
    for (size_t h = B; h > 0;) {
      unsigned len = path[b][h];
      if (len == 0) { flags |= 2u; len = path[b][h] = 1; }
      if (len >= 3) {
        uint16_t sublen[259] = {0}, dist = 0, longest = 0;
        zo_find_longest_match(d.table, d.blk.instart + h - len, sublen, &dist, &longest);
        if (len > longest || sublen[len] == 0) flags |= 4u;
      }
      h -= len;
    }
  }
  if (flags) {
    char buf[96];
    std::snprintf(buf, sizeof(buf), "zmx_trace_length_arrays: device consistency flags 0x%x", flags);
    return Fail(buf);
  }
  for (size_t b = 0; b < nblocks; ++b) {
    BlockData& d = t->blocks[b];
    const int s = slot[b];
    d.nsym[s] = zo_trace_follow(d.table, path[b].data(), d.litlens[s].data(), d.dists[s].data());
    nsym[b] = static_cast<uint32_t>(d.nsym[s]);
    zo_histogram(d.litlens[s].data(), d.dists[s].data(), d.nsym[s], hist + b * ZMX_HIST);
  }
  return 0;
}

int zmx_store_download(zmx_ctx*, zmx_tables* t, size_t block, int slot, uint16_t* litlens, uint16_t* dists,
                       size_t nsym) {
  if (const int rc = CheckTables("zmx_store_download", t, zamd::kAnyTables)) return rc;
  if (const int rc = CheckStoreRef("zmx_store_download", t, block, slot, nsym)) return rc;
  BlockData& d = t->blocks[block];
  std::memcpy(litlens, d.litlens[slot].data(), nsym * 2);
  std::memcpy(dists, d.dists[slot].data(), nsym * 2);
  return 0;
}

int zmx_store_download_batch(zmx_ctx* c, zmx_tables* t, size_t n, const size_t* block, const int32_t* slot,
                             const size_t* nsym, uint16_t* const* litlens, uint16_t* const* dists) {
  if (const int rc = CheckTables("zmx_store_download_batch", t, zamd::kAnyTables)) return rc;
  for (size_t i = 0; i < n; ++i) {
    if (const int rc = CheckStoreRef("zmx_store_download_batch", t, block[i], slot[i], nsym[i])) return rc;
  }
  for (size_t i = 0; i < n; ++i) {
    const int rc = zmx_store_download(c, t, block[i], slot[i], litlens[i], dists[i], nsym[i]);
    if (rc) return rc;
  }
  return 0;
}

// (CPU stand-in for the device's verify pass)
int zmx_verify_stores(zmx_ctx* c, zmx_tables* t, size_t n, const size_t* block, const int32_t* slot, const size_t* nsym) {
  if (const int rc = CheckTables("zmx_verify_stores", t, zamd::kUntrimmed)) return rc;
  for (size_t i = 0; i < n; ++i) {
    if (const int rc = CheckStoreRef("zmx_verify_stores", t, block[i], slot[i], nsym[i])) return rc;
  }
  for (size_t i = 0; i < n; ++i) {
    const BlockData& d = t->blocks[block[i]];
    size_t pos = d.blk.instart;
    for (size_t k = 0; k < nsym[i]; ++k) {
      const unsigned litlen = d.litlens[slot[i]][k], dist = d.dists[slot[i]][k];
      if (dist == 0) {
        if (pos >= d.blk.inend || c->input[pos] != litlen) { return Fail("zmx_verify_stores: literal"); }
        pos += 1;
      } else {
        if (litlen < 3 || litlen > 258 || dist > pos || pos + litlen > d.blk.inend) { return Fail("zmx_verify_stores: range"); }
        for (unsigned q = 0; q < litlen; ++q) {
          if (c->input[pos + q] != c->input[pos + q - dist]) { return Fail("zmx_verify_stores: bytes"); }
        }
        pos += litlen;
      }
    }
    if (pos != d.blk.inend) { return Fail("zmx_verify_stores: coverage"); }
  }
  return 0;
}

// (CPU stand-in for k_checksum: the same pieces, lanes and tree, walked one after the other, so that the
// CPU suite exercises the arithmetic of host/checksum.cc the way the device feeds it)
int zmx_checksum(zmx_ctx* c, int kind, size_t begin, size_t end, uint32_t* value) {
  using namespace zamd;
  if (kind != ZMX_CRC32 && kind != ZMX_ADLER32) { return Fail("zmx_checksum: unknown kind"); }
  if (begin > end || end > c->input.size()) { return Fail("zmx_checksum: range outside the resident input"); }
  const size_t n = end - begin, npieces = (n + kChecksumPieceBytes - 1) / kChecksumPieceBytes;
  uint32_t xpow[8];
  ChecksumTreePowers(xpow);
  std::vector<ChecksumPiece> pieces(npieces);
  for (size_t w = 0; w < npieces; ++w) {
    const long long wg_end = static_cast<long long>(end) - static_cast<long long>(w) * kChecksumPieceBytes;
    uint32_t cr[256], sa[256], sb[256];
    for (int t = 0; t < 256; ++t) {
      const long long hi = wg_end - static_cast<long long>(255 - t) * kChecksumLaneBytes;
      long long p = hi - kChecksumLaneBytes;
      if (p < static_cast<long long>(begin)) p = static_cast<long long>(begin);
      uint32_t crc = 0, sum = 0, wsum = 0;
      for (; p < hi; ++p) {
        const uint32_t d = c->input[static_cast<size_t>(p)];
        crc ^= d;
        for (int k = 0; k < 8; ++k) crc = (crc & 1) ? (crc >> 1) ^ kCrcPoly : crc >> 1;
        sum += d;
        wsum += static_cast<uint32_t>(hi - p) * d;
      }
      cr[t] = crc; sa[t] = sum % kAdlerBase; sb[t] = wsum % kAdlerBase;
    }
    for (uint32_t s = 1, k = 0; s < 256; s <<= 1, ++k) {
      for (uint32_t t = 0; t < 256; t += 2 * s) {
        cr[t] = Gf2MulMod(cr[t], xpow[k]) ^ cr[t + s];
        sb[t] = static_cast<uint32_t>((sb[t] + static_cast<uint64_t>((s * kChecksumLaneBytes) % kAdlerBase) * sa[t] + sb[t + s]) % kAdlerBase);
        sa[t] = (sa[t] + sa[t + s]) % kAdlerBase;
      }
    }
    pieces[w] = ChecksumPiece{cr[0], sa[0], sb[0]};
  }
  *value = kind == ZMX_CRC32 ? FinishCrc32(pieces.data(), npieces, n) : FinishAdler32(pieces.data(), npieces, n);
  return 0;
}

// (CPU stand-in for the device bit writer: the same contract, symbol by symbol)
int zmx_encode_blocks(zmx_ctx*, zmx_tables* t, size_t njobs, const zmx_enc_job* jobs, const uint32_t* codes,
                      unsigned char* const* out) {
  if (njobs == 0) return 0;
  if (const int rc = CheckTables("zmx_encode_blocks", t, zamd::kAnyTables)) return rc;
  for (size_t j = 0; j < njobs; ++j) {
    if (const int rc = CheckStoreRef("zmx_encode_blocks", t, jobs[j].block, jobs[j].slot, jobs[j].nsym)) return rc;
  }
  for (size_t j = 0; j < njobs; ++j) {
    const zmx_enc_job& q = jobs[j];
    const BlockData& d = t->blocks[q.block];
    const uint32_t* cd = codes + j * 320;
    unsigned char* o = out[j];
    uint64_t pos = q.bit_start;
    auto put = [&](uint64_t v, unsigned n) {
      for (unsigned i = 0; i < n; ++i, ++pos) o[pos >> 3] |= static_cast<unsigned char>(((v >> i) & 1u) << (pos & 7));
    };
    auto flog2 = [](unsigned v) { return 31 - __builtin_clz(v); };
    for (size_t i = 0; i < q.nsym; ++i) {
      const unsigned litlen = d.litlens[q.slot][i], dist = d.dists[q.slot][i];
      if (dist == 0) {
        put(cd[litlen] & 0xffffu, cd[litlen] >> 16);
        continue;
      }
      unsigned ls, le;
      if (litlen < 11) { ls = 254 + litlen; le = 0; }
      else if (litlen == 258) { ls = 285; le = 0; }
      else { le = static_cast<unsigned>(flog2(litlen - 3) - 2); ls = 261 + 4 * le + (((litlen - 3) >> le) & 3); }
      unsigned ds, de;
      if (dist < 5) { ds = dist - 1; de = 0; }
      else { const int l = flog2(dist - 1); ds = static_cast<unsigned>(2 * l) + (((dist - 1) >> (l - 1)) & 1); de = static_cast<unsigned>(l - 1); }
      put(cd[ls] & 0xffffu, cd[ls] >> 16);
      put((litlen - 3) & ((1u << le) - 1), le);
      put(cd[288 + ds] & 0xffffu, cd[288 + ds] >> 16);
      put((dist - 1) & ((1u << de) - 1), de);
    }
    put(cd[256] & 0xffffu, cd[256] >> 16);
    if (pos - q.bit_start != q.nbits) return -1;
  }
  return 0;
}

int zmx_find_longest_match(zmx_ctx*, zmx_tables* t, size_t block, size_t pos, uint16_t* sublen,
                           uint16_t* distance, uint16_t* length) {
  if (const int rc = CheckTables("zmx_find_longest_match", t, zamd::kUntrimmed)) return rc;
  if (const int rc = CheckBlock("zmx_find_longest_match", t, block)) return rc;
  zo_find_longest_match(t->blocks[block].table, pos, sublen, distance, length);
  return 0;
}

int zmx_length_array_download(zmx_ctx*, zmx_tables* t, size_t block, uint16_t* out) {
  if (const int rc = CheckTables("zmx_length_array_download", t, zamd::kUntrimmed)) return rc;
  if (const int rc = CheckBlock("zmx_length_array_download", t, block)) return rc;
  const auto& la = t->blocks[block].length_array;
  std::memcpy(out, la.data(), la.size() * 2);
  return 0;
}

// ---- f-1's device entry points, TEST-ONLY stand-ins: the sequences as host stores, the sizes by the host's own block-cost
// code (so that DeflateParts' device-split path — queries, the mixing of device and host rounds — runs on CPU)
struct zmx_cost_stores {
  std::vector<zamd::Lz77Store> stores;
};
int zmx_cost_stores_create(zmx_ctx*, zmx_tables* t, size_t nstores, const size_t* piece_first, const size_t* block,
                           const int32_t* slot, const size_t* nsym, zmx_cost_stores** out) {
  *out = nullptr;
  if (nstores == 0) return Refuse("zmx_cost_stores_create: no sequence");
  if (const int rc = CheckTables("zmx_cost_stores_create", t, zamd::kAnyTables)) return rc;
  for (size_t p = 0; p < piece_first[nstores]; ++p) {
    if (const int rc = CheckStoreRef("zmx_cost_stores_create", t, block[p], slot[p], nsym[p])) return rc;
  }
  zmx_cost_stores* s = new zmx_cost_stores();
  s->stores.resize(nstores);
  for (size_t q = 0; q < nstores; ++q) {
    // (a sequence counts its own bytes, as on the device: its pieces may be prefixes of stores, in any order of the input)
    size_t pos = 0;
    for (size_t p = piece_first[q]; p < piece_first[q + 1]; ++p) {
      const BlockData& d = t->blocks[block[p]];
      s->stores[q].Append(d.litlens[slot[p]].data(), d.dists[slot[p]].data(), nsym[p], pos);
      pos = s->stores[q].ByteRange(0, s->stores[q].size());
    }
  }
  *out = s;
  return 0;
}
int zmx_cost_stores_create_host(zmx_ctx*, size_t nstores, const uint16_t* const* litlens, const uint16_t* const* dists,
                                const size_t* nsym, zmx_cost_stores** out) {
  *out = nullptr;
  // (the device layer's refusal, by the same rule: symbol_check.h)
  for (size_t q = 0; q < nstores; ++q) {
    const size_t bad = zamd::FirstInvalidSymbol(litlens[q], dists[q], nsym[q]);
    if (bad < nsym[q]) {
      return Refuse("zmx_cost_stores_create_host: sequence " + std::to_string(q) + ", symbol " + std::to_string(bad) + " is no LZ77 symbol");
    }
  }
  zmx_cost_stores* s = new zmx_cost_stores();
  s->stores.resize(nstores);
  for (size_t q = 0; q < nstores; ++q) s->stores[q].Append(litlens[q], dists[q], nsym[q], 0);
  *out = s;
  return 0;
}
void zmx_cost_stores_free(zmx_ctx*, zmx_cost_stores* s) { delete s; }
int zmx_cost_positions(zmx_ctx*, zmx_cost_stores* s, size_t n, const uint32_t* pairs, uint64_t* bytes) {
  for (size_t i = 0; i < n; ++i) {
    if (pairs[2 * i] >= s->stores.size() || pairs[2 * i + 1] > s->stores[pairs[2 * i]].size()) { return Fail("zmx_cost_positions: an index outside its sequence"); }
    bytes[i] = s->stores[pairs[2 * i]].ByteRange(0, pairs[2 * i + 1]);
  }
  return 0;
}
int zmx_block_costs(zmx_ctx*, zmx_cost_stores* s, size_t n, const uint32_t* r, double* cost) {
  // (ZOPFLI_HOSTTEST_COSTS_FAIL_AFTER=k: the k-th call and every later one fails — the host's fall-back in mid-search)
  static const long fail_after = [] { const char* e = std::getenv("ZOPFLI_HOSTTEST_COSTS_FAIL_AFTER"); return e ? std::atol(e) : -1L; }();
  static std::atomic<long> calls{0};
  if (fail_after >= 0 && calls.fetch_add(1) >= fail_after) { return Fail("zmx_block_costs: injected failure"); }
  for (size_t i = 0; i < n; ++i) {
    if (r[3 * i] >= s->stores.size() || r[3 * i + 1] > r[3 * i + 2] || r[3 * i + 2] > s->stores[r[3 * i]].size()) { return Fail("zmx_block_costs: a range outside its sequence"); }
    cost[i] = zamd::CalculateBlockSizeAutoType(s->stores[r[3 * i]], r[3 * i + 1], r[3 * i + 2]);
  }
  return 0;
}

// ---- hooks for unit tests of the product's host arithmetic against the real reference
// (tests/test_cpu_oracle_vs_reference.py)
__attribute__((visibility("default"))) int zamd_test_code_lengths(const size_t* freq, int n, int maxbits, unsigned* lengths) {
  return zamd::LengthLimitedCodeLengths(freq, n, maxbits, lengths) ? 0 : 1;
}

__attribute__((visibility("default"))) double zamd_test_block_size_auto(const uint16_t* litlens, const uint16_t* dists, size_t n,
                                                                          size_t lstart, size_t lend) {
  zamd::Lz77Store s(nullptr);
  s.Append(litlens, dists, n, 0);
  return zamd::CalculateBlockSizeAutoType(s, lstart, lend);
}

__attribute__((visibility("default"))) size_t zamd_test_block_split(const uint16_t* litlens, const uint16_t* dists, size_t n,
                                                                      size_t maxblocks, size_t* points, size_t cap) {
  zamd::Lz77Store s(nullptr);
  s.Append(litlens, dists, n, 0);
  std::vector<size_t> pts;
  zamd::BlockSplitLz77(s, maxblocks, &pts);
  for (size_t i = 0; i < pts.size() && i < cap; ++i) points[i] = pts[i];
  return pts.size();
}

// BlockSplitLz77Batch over `copies` views of the sequence cut at different lengths (n, n - n / 7, n - 2 n / 7, ...):
// the split points of view v go to points[v * cap ..], their number to counts[v]
__attribute__((visibility("default"))) void zamd_test_block_split_batch(const uint16_t* litlens, const uint16_t* dists, size_t n, size_t copies,
                                                                          size_t maxblocks, size_t* points, size_t* counts, size_t cap) {
  std::vector<zamd::Lz77Store> stores;
  stores.reserve(copies);
  std::vector<const zamd::Lz77Store*> ptrs;
  for (size_t v = 0; v < copies; ++v) {
    stores.emplace_back(nullptr);
    stores.back().Append(litlens, dists, n - v * (n / 7), 0);
    ptrs.push_back(&stores.back());
  }
  std::vector<std::vector<size_t>> pts;
  zamd::BlockSplitLz77Batch(ptrs, maxblocks, &pts);
  for (size_t v = 0; v < copies; ++v) {
    counts[v] = pts[v].size();
    for (size_t i = 0; i < pts[v].size() && i < cap; ++i) points[v * cap + i] = pts[v][i];
  }
}

}  // extern "C"
