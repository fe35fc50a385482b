// TEST-ONLY: the planning functions of the dealer (zopfli_amd/csrc/host/deal.h) from the command line, one line of
// integers each.  tests/test_cpu_dealing.py calls it.
//   deal_print priorities 0,0,1        ShardPriorities
//   deal_print after 0,1,0             UploadAfter
//   deal_print ranges NPARTS NDEV WEIGHTS [COSTS]   ShardRanges: the ndev + 1 boundaries ("-" = no weights)
//   deal_print runs FILE               LooksLikeRuns over the whole file: 1 or 0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "deal.h"

namespace {

std::vector<double> Numbers(const char* text) {
  std::vector<double> v;
  if (std::strcmp(text, "-") == 0) return v;
  for (const char* p = text; *p;) {
    char* end = nullptr;
    v.push_back(std::strtod(p, &end));
    if (end == p) { v.pop_back(); break; }
    p = *end == ',' ? end + 1 : end;
  }
  return v;
}

template <typename T>
int Print(const std::vector<T>& v) {
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %ld" : "%ld", static_cast<long>(v[i]));
  std::printf("\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if ((what == "priorities" || what == "after") && argc == 3) {
    std::vector<int> device_of;
    for (double d : Numbers(argv[2])) device_of.push_back(static_cast<int>(d));
    return what == "after" ? Print(zamd::UploadAfter(device_of)) : Print(zamd::ShardPriorities(device_of));
  }
  if (what == "ranges" && (argc == 5 || argc == 6)) {
    const size_t nparts = static_cast<size_t>(std::atol(argv[2])), ndev = static_cast<size_t>(std::atol(argv[3]));
    const std::vector<double> cost = argc == 6 ? Numbers(argv[5]) : std::vector<double>();
    if (ndev == 0 || nparts < ndev || (argc == 6 && cost.size() != nparts)) return 2;
    return Print(zamd::ShardRanges(nparts, ndev, cost.empty() ? nullptr : cost.data(), Numbers(argv[4])));
  }
  if (what == "runs" && argc == 3) {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<unsigned char> data;
    unsigned char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    std::printf("%d\n", zamd::LooksLikeRuns(data.data(), 0, data.size()) ? 1 : 0);
    return 0;
  }
  std::fprintf(stderr, "usage: deal_print priorities|after LIST | ranges NPARTS NDEV WEIGHTS [COSTS] | runs FILE\n");
  return 2;
}
