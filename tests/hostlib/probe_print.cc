// The rules of device/zmx_probe.h on the CPU: the __host__ __device__ functions k_probe_counts and k_tail_runs are made
// of, run by a plain C++ program (tests/test_cpu_probe_counts.py compares its lines with zamd::MasterBlockCost and
// zamd::LooksLikeRuns of the host library).
//   probe_print FILE BEGIN END [BEGIN END ...]
// prints for every range of the file's bytes one line:
//   probes runs few probes4k hits  cost (the double's bits, hex)  runs (1 or 0)  tail (TailRunStart, or END when empty)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deal.h"
#include "zmx_probe.h"

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 2) % 2 != 0) {
    std::fprintf(stderr, "usage: probe_print FILE BEGIN END [BEGIN END ...]\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<unsigned char> data;
  unsigned char buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
  std::fclose(f);
  // (an exact-size copy on the heap: a probe or a walk that leaves the range is the sanitizer's to find)
  unsigned char* bytes = static_cast<unsigned char*>(std::malloc(data.size() ? data.size() : 1));
  if (!data.empty()) std::memcpy(bytes, data.data(), data.size());
  for (int a = 2; a + 1 < argc; a += 2) {
    const uint64_t begin = std::strtoull(argv[a], nullptr, 10), end = std::strtoull(argv[a + 1], nullptr, 10);
    if (begin > end || end > data.size()) return 2;
    uint32_t c[zamd::kProbeCounts];
    zamd::ProbeRange(bytes, begin, end, c);
    const double cost = zamd::CostFromCounts(end - begin, c[zamd::kProbes], c[zamd::kRuns], c[zamd::kFew]);
    uint64_t bits;
    std::memcpy(&bits, &cost, sizeof(bits));
    const uint64_t tail = end > begin ? zamd::TailRunStart(bytes, begin, end) : end;
    std::printf("%u %u %u %u %u %016" PRIx64 " %d %" PRIu64 "\n", c[0], c[1], c[2], c[3], c[4], bits,
                zamd::RunsFromCounts(c[zamd::kProbes4k], c[zamd::kHits]) ? 1 : 0, tail);
  }
  std::free(bytes);
  return 0;
}
