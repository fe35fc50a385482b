// What LodePNG makes of a PNG file, from LodePNG's own code: lodepng_decode without colour conversion (the file's own colour
// type and depth) and lodepng_decode32.  tests/golden/make_png_decode_golden.py records what it prints.  Nothing is copied:
// the reference's sources are compiled in from wherever they lie,
//   g++ -O2 -w -I $LODEPNG_DIR tools/models/png_decode_model.cc $LODEPNG_DIR/lodepng.cpp -o png_decode_model
//   png_decode_model     stdin: a file per line as hex ("-": empty); per file it prints
//     "ERROR WIDTH HEIGHT COLORTYPE BITDEPTH OWN_HEX ERROR32 RGBA8_HEX" — LodePNG's error number of either call (0: none), the
//     header as decoded, the pixels as hex ("-": none).  Below 8 bits LodePNG's own-mode rows are packed bit after bit with
//     no padding at a row's end.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "lodepng.h"

static void Hex(const unsigned char* p, size_t n) {
  if (n == 0 || !p) {
    std::printf("-");
    return;
  }
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "-") line.clear();
    std::vector<unsigned char> file(line.size() / 2);
    for (size_t i = 0; i < file.size(); ++i) file[i] = static_cast<unsigned char>(std::strtoul(line.substr(2 * i, 2).c_str(), nullptr, 16));
    lodepng::State state;
    state.decoder.color_convert = 0;
    unsigned w = 0, h = 0;
    unsigned char* own = nullptr;
    const unsigned error = lodepng_decode(&own, &w, &h, &state, file.data(), file.size());
    std::printf("%u %u %u %u %u ", error, w, h, static_cast<unsigned>(state.info_png.color.colortype), state.info_png.color.bitdepth);
    Hex(own, error ? 0 : lodepng_get_raw_size(w, h, &state.info_png.color));
    std::free(own);
    unsigned char* rgba = nullptr;
    const unsigned error32 = lodepng_decode32(&rgba, &w, &h, file.data(), file.size());
    std::printf(" %u ", error32);
    Hex(rgba, error32 ? 0 : 4 * static_cast<size_t>(w) * h);
    std::free(rgba);
    std::printf("\n");
  }
  return 0;
}
