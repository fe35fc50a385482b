// The match record of device/zmx_record.h on the CPU: the functions every kernel packs and unpacks it with, run by a
// plain C++ program over a table of records (tests/test_cpu_record_format.py holds the output against its own model of
// the header's layout comment).
//   record_print TABLE
// TABLE, a record per line, all decimal: FRONT BACK LENGTH DIST SAME LITERAL N, then N pairs LEN DIST, the change points
// of sublen in ascending length.  A record with N > 8 puts its change points into the pool behind FRONT entries that are
// not its own, with BACK such entries behind them.
// Every record is packed both ways — the three 64-bit accumulators k_match2 appends to, and k_match5's eight slots
// packed into six words — and the two must give the same eight words, and the same first eight pool entries.  Then
// every reader decodes it.  An overflow record is decoded twice: from the whole pool, and from a heap array that ends
// with the record's last entry (a read behind it is the sanitizer's to find); the two must agree.  Per record:
//   rec   the eight words, hex
//   hdr   length dist same literal count overflow pool-offset pool-count
//   cps   the change points RecWalkCps visits, LEN:DIST each
//   walk / scan / acc / thr / pool   sublen[3 .. 258] by each reader ("-": the reader is not for this record):
//         the walk; k_trace_emit's scan over the six words; the same scan over the accumulators; k_codes' threshold
//         search; the search in the pool.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zmx_record.h"

namespace {

struct Row {
  uint32_t front, back, length, dist, same, literal;
  std::vector<uint32_t> len, d;
};

uint32_t Junk(size_t i) { return zamd::RecPoolEntry(3u + static_cast<uint32_t>(i % 200), 30000u + static_cast<uint32_t>(i % 2000)); }

int Fail(size_t row, const char* what) {
  std::printf("record %zu: %s\n", row, what);
  return 1;
}

void PrintSublen(const char* name, const std::vector<uint32_t>& s) {
  std::printf("%s", name);
  for (uint32_t len = 3; len <= 258; ++len) std::printf(" %u", s[len]);
  std::printf("\n");
}

// sublen[] as the host's probe fills it from the walk (drv_probes.h)
std::vector<uint32_t> ByWalk(const uint32_t* rec, const uint32_t* pool) {
  std::vector<uint32_t> s(259, 0);
  uint32_t prev = 2;
  zamd::RecWalkCps(rec, pool, [&](uint32_t len, uint32_t dist) {
    for (uint32_t l = prev + 1; l <= len; ++l) s[l] = dist;
    prev = len;
  });
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: record_print TABLE\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Row> rows;
  for (;;) {
    Row r;
    unsigned n = 0;
    if (std::fscanf(f, "%u %u %u %u %u %u %u", &r.front, &r.back, &r.length, &r.dist, &r.same, &r.literal, &n) != 7) break;
    for (unsigned i = 0; i < n; ++i) {
      unsigned l = 0, d = 0;
      if (std::fscanf(f, "%u %u", &l, &d) != 2) return 2;
      r.len.push_back(l);
      r.d.push_back(d);
    }
    rows.push_back(r);
  }
  std::fclose(f);

  // the pool of the whole table: FRONT foreign entries, the record's own, BACK foreign entries, record after record
  std::vector<uint32_t> pool, off(rows.size(), 0);
  for (size_t i = 0; i < rows.size(); ++i) {
    const Row& r = rows[i];
    if (r.len.size() <= zamd::kRecInlineCps) continue;
    for (uint32_t k = 0; k < r.front; ++k) pool.push_back(Junk(pool.size()));
    off[i] = static_cast<uint32_t>(pool.size());
    for (size_t e = 0; e < r.len.size(); ++e) pool.push_back(zamd::RecPoolEntry(r.len[e], r.d[e]));
    for (uint32_t k = 0; k < r.back; ++k) pool.push_back(Junk(pool.size()));
  }

  for (size_t i = 0; i < rows.size(); ++i) {
    const Row& r = rows[i];
    const uint32_t n = static_cast<uint32_t>(r.len.size());
    const uint32_t held = n < zamd::kRecInlineCps ? n : zamd::kRecInlineCps;

    // ---- pack, both ways
    uint64_t c0 = 0, c1 = 0, c2 = 0;
    uint32_t v[8];
    for (uint32_t e = 0; e < 8; ++e) {
      if (e < held) zamd::RecCpAppend(c0, c1, c2, e, zamd::RecCpField(r.len[e], r.d[e]));
      v[e] = e < held ? zamd::RecCpField(r.len[e], r.d[e]) : 0u;
    }
    uint32_t ra[zamd::kRecWords], rb[zamd::kRecWords];
    ra[0] = rb[0] = zamd::RecWord0(r.length, r.dist);
    ra[1] = rb[1] = zamd::RecWord1(r.same, r.literal, n <= zamd::kRecInlineCps ? n : zamd::kRecOverflow);
    zamd::RecCpAccWords(c0, c1, c2, ra + 2);
    zamd::RecCpPackFields(v, rb + 2);
    if (n > zamd::kRecInlineCps) {
      ra[2] = rb[2] = off[i];
      ra[3] = rb[3] = n;
      // (the first eight pool entries: k_match2 takes them out of its accumulators)
      for (uint32_t e = 0; e < 8; ++e) {
        if (zamd::RecCpPoolEntry(zamd::RecCpFieldOfAcc(c0, c1, c2, e)) != pool[off[i] + e]) return Fail(i, "pool entry out of the accumulators differs");
      }
    }
    if (std::memcmp(ra, rb, sizeof ra) != 0) return Fail(i, "the two packings differ");
    const uint32_t* rec = ra;

    std::printf("rec");
    for (uint32_t k = 0; k < zamd::kRecWords; ++k) std::printf(" %08" PRIx32, rec[k]);
    const bool ovf = zamd::RecIsOverflow(rec[1]);
    std::printf("\nhdr %u %u %u %u %u %d %u %u\n", zamd::RecLength(rec[0]), zamd::RecDist(rec[0]), zamd::RecSame(rec[1]),
                zamd::RecLiteral(rec[1]), zamd::RecCount(rec[1]), ovf ? 1 : 0, ovf ? zamd::RecPoolOffset(rec[2]) : 0u,
                ovf ? zamd::RecPoolCount(rec[3]) : 0u);

    // ---- decode
    std::printf("cps");
    zamd::RecWalkCps(rec, pool.data(), [](uint32_t len, uint32_t dist) { std::printf(" %u:%u", len, dist); });
    std::printf("\n");
    const std::vector<uint32_t> walk = ByWalk(rec, pool.data());
    PrintSublen("walk", walk);
    if (!ovf) {
      const uint32_t ncp = zamd::RecCount(rec[1]);
      const uint32_t* w = rec + 2;
      std::vector<uint32_t> scan(259, 0), acc(259, 0), thr(259, 0);
      uint32_t t0 = 0, t1 = 0;
      for (uint32_t e = 0; e < 8; ++e) {
        if (zamd::RecCpFieldOfAcc(c0, c1, c2, e) != (zamd::RecCpFieldOfWords(w, e) & 0xffffffu)) return Fail(i, "field of the accumulators differs");
        zamd::RecCpThresholdPut(t0, t1, e, ncp, zamd::RecCpFieldOfWords(w, e));
      }
      for (uint32_t len = 3; len <= 258; ++len) {
        for (int k = 7; k >= 0; --k) {
          const uint32_t x = zamd::RecCpFieldOfWords(w, static_cast<uint32_t>(k));
          if (static_cast<uint32_t>(k) < ncp && zamd::RecCpLength(x) >= len) scan[len] = zamd::RecCpDist(x);
          const uint32_t y = zamd::RecCpFieldOfAcc(c0, c1, c2, static_cast<uint32_t>(k));
          if (static_cast<uint32_t>(k) < ncp && zamd::RecCpLength(y) >= len) acc[len] = zamd::RecCpDist(y);
        }
        thr[len] = zamd::RecCpDist(zamd::RecCpFieldOfWords(w, zamd::RecCpThresholdIndex(t0, t1, len - 3)));
      }
      PrintSublen("scan", scan);
      PrintSublen("acc", acc);
      PrintSublen("thr", thr);
      std::printf("pool -\n");
    } else {
      const uint32_t po = zamd::RecPoolOffset(rec[2]), pn = zamd::RecPoolCount(rec[3]);
      // a heap array that ends with the record's last entry
      uint32_t* tight = static_cast<uint32_t*>(std::malloc(static_cast<size_t>(po + pn) * sizeof(uint32_t)));
      if (!tight) return 2;
      std::memcpy(tight, pool.data(), static_cast<size_t>(po + pn) * sizeof(uint32_t));
      std::vector<uint32_t> find(259, 0);
      for (uint32_t len = 3; len <= 258; ++len) {
        const uint32_t at = zamd::RecPoolFind(pool.data(), po, pn, len);
        if (zamd::RecPoolFind(tight, po, pn, len) != at) return Fail(i, "the search differs between the two pools");
        if (at < pn) find[len] = zamd::RecPoolDist(tight[po + at]);
      }
      if (ByWalk(rec, tight) != walk) return Fail(i, "the walk differs between the two pools");
      std::free(tight);
      std::printf("scan -\nacc -\nthr -\n");
      PrintSublen("pool", find);
    }
  }
  std::printf("ok %zu\n", rows.size());
  return 0;
}
