// The rules of zopfli_amd/csrc/device/zmx_png_lodeflate.h and zopfli_amd/csrc/host/png_lodeflate_size.h as a plain C++
// program: the kernels' lanes one after the other (a barrier of k_png_lo_links is the end of a loop over the lanes),
// the parse's staging straight from the arrays.
//   png_lodeflate_print size WINDOW TILE FILE...   the files are the buffers of ONE call: prints a zlib size per file
//   png_lodeflate_print arrays WINDOW TILE OUT FILE...   the same call; also writes HC, ZC, LD ([positions] each) and counts
//                                                  ([blocks][kLoCountWords]) as the lanes left them to OUT: raw
//                                                  little-endian uint32, one array after the other, in the plan's order
// TILE 0 is the device's tile length.
//   png_lodeflate_print huff FILE                  every byte a literal (no matches): the size from the bytes' counts per block
//   png_lodeflate_print lengths MAXBITS COUNT...   LoCodeLengths of the counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "png_lodeflate_size.h"
#include "zmx_png_lodeflate.h"

namespace {

std::vector<unsigned char> ReadFile(const char* path) {
  std::vector<unsigned char> data;
  FILE* fp = fopen(path, "rb");
  if (!fp) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  unsigned char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, fp)) > 0) data.insert(data.end(), buf, buf + got);
  fclose(fp);
  return data;
}

struct Arrays {   // of one call, as the device's scratch holds them when k_png_lo_parse has ended
  std::vector<uint32_t> HC, ZC, LD, counts;
};

std::vector<uint64_t> Sizes(const std::vector<std::vector<unsigned char>>& bufs, unsigned window, unsigned tile_len, Arrays* arrays = nullptr) {
  if (tile_len == 0) tile_len = zamd::kLoTileLen;
  std::vector<const void*> ptrs;
  std::vector<size_t> sizes;
  for (const auto& b : bufs) { ptrs.push_back(b.data()); sizes.push_back(b.size()); }
  zamd::LoPlan plan = zamd::LoMakePlan(bufs.size(), ptrs.data(), sizes.data(), tile_len);
  std::vector<uint32_t> HC(plan.positions), ZC(plan.positions), LD(plan.positions);
  std::vector<uint32_t> tables(plan.tiles.size() * static_cast<size_t>(zamd::kLoTableLen), 0);
  std::vector<uint32_t> counts(plan.blocks.size() * static_cast<size_t>(zamd::kLoCountWords), 0);
  zamd::LoParams P;
  P.bufs = plan.bufs.data();
  P.tiles = plan.tiles.data();
  P.blocks = plan.blocks.data();
  P.HC = HC.data();
  P.ZC = ZC.data();
  P.LD = LD.data();
  P.tables = tables.data();
  P.counts = counts.data();
  P.window = window;
  P.ntiles = static_cast<uint32_t>(plan.tiles.size());
  P.nblocks = static_cast<uint32_t>(plan.blocks.size());
  P.tile_len = tile_len;
  const uint32_t T = zamd::kLoThreads;
  for (uint32_t t = 0; t < P.ntiles; ++t)
    for (uint32_t i = 0; i < plan.tiles[t].len; ++i) zamd::LoHashLane(P, t, i);
  for (uint32_t t = 0; t < P.ntiles; ++t) {
    uint32_t s_h[zamd::kLoThreads], s_z[zamd::kLoThreads];
    unsigned char s_nexth[zamd::kLoThreads], s_nextz[zamd::kLoThreads];
    for (uint32_t b0 = 0; b0 < plan.tiles[t].len; b0 += T) {
      for (uint32_t l = 0; l < T; ++l) zamd::LoLinksLoad(P, t, b0, l, s_h, s_z, s_nexth, s_nextz);
      for (uint32_t l = T; l-- > 0;) zamd::LoLinksFind(P, t, b0, l, s_h, s_z, s_nexth, s_nextz);   // (any order: here the last lane first)
      for (uint32_t l = 0; l < T; ++l) zamd::LoLinksPublish(P, t, b0, l, s_h, s_z, s_nexth, s_nextz);
    }
  }
  for (uint32_t t = P.ntiles; t-- > 0;)
    for (uint32_t i = 0; i < plan.tiles[t].len; ++i) zamd::LoAskLane(P, t, i);
  for (uint32_t t = P.ntiles; t-- > 0;)     // (the later tiles first: their walks meet unresolved KEEPs)
    for (uint32_t i = plan.tiles[t].len; i-- > 0;) zamd::LoKeepLane(P, t, i);
  for (uint32_t t = 0; t < P.ntiles; ++t)
    for (uint32_t i = 0; i < plan.tiles[t].len; ++i) zamd::LoSearchLane(P, t, i);
  std::vector<zamd::LoBlockCounts> blocks(plan.blocks.size(), zamd::LoBlockCounts());
  for (uint32_t b = 0; b < P.nblocks; ++b) {
    const zamd::LoTile K = plan.blocks[b];
    const zamd::LoBuf B = plan.bufs[K.buf];
    uint32_t* cnt = counts.data() + static_cast<size_t>(b) * zamd::kLoCountWords;
    const uint64_t extra = zamd::LoParseBlock(
        K.len, window,
        [&](uint32_t pos, uint32_t* byte) {
          *byte = B.data[K.start + pos];
          return LD[B.base + K.start + pos];
        },
        [&](uint32_t symbol) { ++cnt[symbol]; });
    for (int i = 0; i < 286; ++i) blocks[b].ll[i] = cnt[i];
    for (int i = 0; i < 30; ++i) blocks[b].d[i] = cnt[286 + i];
    blocks[b].extra_bits = extra;
    cnt[316] = static_cast<uint32_t>(extra);          // (as k_png_lo_parse leaves them)
    cnt[317] = static_cast<uint32_t>(extra >> 32);
  }
  std::vector<uint64_t> out;
  for (size_t b = 0; b < bufs.size(); ++b) {
    out.push_back(zamd::LoZlibBytes(blocks.data() + plan.first_block[b], plan.first_block[b + 1] - plan.first_block[b]));
  }
  if (arrays) {
    arrays->HC.swap(HC);
    arrays->ZC.swap(ZC);
    arrays->LD.swap(LD);
    arrays->counts.swap(counts);
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 5 && std::strcmp(argv[1], "size") == 0) {
    std::vector<std::vector<unsigned char>> bufs;
    for (int i = 4; i < argc; ++i) bufs.push_back(ReadFile(argv[i]));
    for (const uint64_t s : Sizes(bufs, static_cast<unsigned>(atoi(argv[2])), static_cast<unsigned>(atoi(argv[3])))) {
      printf("%llu\n", static_cast<unsigned long long>(s));
    }
    return 0;
  }
  if (argc >= 6 && std::strcmp(argv[1], "arrays") == 0) {
    std::vector<std::vector<unsigned char>> bufs;
    for (int i = 5; i < argc; ++i) bufs.push_back(ReadFile(argv[i]));
    Arrays a;
    const std::vector<uint64_t> sizes = Sizes(bufs, static_cast<unsigned>(atoi(argv[2])), static_cast<unsigned>(atoi(argv[3])), &a);
    FILE* fp = fopen(argv[4], "wb");
    if (!fp) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    bool ok = true;
    for (const std::vector<uint32_t>* v : {&a.HC, &a.ZC, &a.LD, &a.counts}) {   // (the hosts this runs on are little-endian)
      ok = ok && fwrite(v->data(), sizeof(uint32_t), v->size(), fp) == v->size();
    }
    ok = fclose(fp) == 0 && ok;
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    for (const uint64_t s : sizes) printf("%llu\n", static_cast<unsigned long long>(s));
    return 0;
  }
  if (argc == 3 && std::strcmp(argv[1], "huff") == 0) {
    const std::vector<unsigned char> data = ReadFile(argv[2]);
    const size_t bs = zamd::LoBlockSize(data.size()), nb = zamd::LoNumBlocks(data.size());
    std::vector<zamd::LoBlockCounts> blocks(nb, zamd::LoBlockCounts());
    for (size_t p = 0; p < data.size(); ++p) ++blocks[p / bs].ll[data[p]];
    printf("%llu\n", static_cast<unsigned long long>(zamd::LoZlibBytes(blocks.data(), nb)));
    return 0;
  }
  if (argc >= 4 && std::strcmp(argv[1], "lengths") == 0) {
    std::vector<uint32_t> counts;
    for (int i = 3; i < argc; ++i) counts.push_back(static_cast<uint32_t>(strtoul(argv[i], nullptr, 10)));
    std::vector<unsigned> lengths(counts.size() < 2 ? 2 : counts.size());
    zamd::LoCodeLengths(counts.data(), counts.size(), static_cast<unsigned>(atoi(argv[2])), lengths.data());
    for (size_t i = 0; i < counts.size(); ++i) printf("%u ", lengths[i]);
    printf("\n");
    return 0;
  }
  fprintf(stderr, "usage: png_lodeflate_print size WINDOW TILE FILE... | arrays WINDOW TILE OUT FILE... | huff FILE | lengths MAXBITS COUNT...\n");
  return 2;
}
