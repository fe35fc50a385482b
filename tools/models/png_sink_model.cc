// What LodePNG's lodepng_convert makes of a PNG file's pixels, from LodePNG's own code: lodepng_decode without colour
// conversion (the file's own mode: its palette with the tRNS alpha, its tRNS key), then lodepng_convert into each of the 8
// modes grey, grey + alpha, RGB, RGBA at 8 and 16 bits.  (lodepng_decode with a raw mode is not used: it refuses 16-bit grey
// outputs with error 56.)  tests/golden/make_png_sink_golden.py records what it prints.  Nothing is copied: the
// reference's sources are compiled in from wherever they lie,
//   g++ -O2 -w -I $LODEPNG_DIR tools/models/png_sink_model.cc $LODEPNG_DIR/lodepng.cpp -o png_sink_model
//   png_sink_model     stdin: a file per line as hex; per file it prints
//     "ERROR WIDTH HEIGHT" and then, for channels 1, 2, 3, 4 and in each for depth 8, 16, " ERROR HEX": lodepng_convert's
//     error number and the converted image as hex (16-bit samples high byte first, as LodePNG holds them; "-": none).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "lodepng.h"

int main() {
  std::string line;
  const LodePNGColorType types[4] = {LCT_GREY, LCT_GREY_ALPHA, LCT_RGB, LCT_RGBA};
  while (std::getline(std::cin, line)) {
    std::vector<unsigned char> file(line.size() / 2);
    for (size_t i = 0; i < file.size(); ++i) file[i] = static_cast<unsigned char>(std::strtoul(line.substr(2 * i, 2).c_str(), nullptr, 16));
    lodepng::State state;
    state.decoder.color_convert = 0;
    unsigned w = 0, h = 0;
    unsigned char* own = nullptr;
    const unsigned error = lodepng_decode(&own, &w, &h, &state, file.data(), file.size());
    std::printf("%u %u %u", error, w, h);
    for (int c = 0; c < 4 && !error; ++c) {
      for (unsigned depth = 8; depth <= 16; depth += 8) {
        LodePNGColorMode out;
        lodepng_color_mode_init(&out);
        out.colortype = types[c];
        out.bitdepth = depth;
        std::vector<unsigned char> image(lodepng_get_raw_size(w, h, &out));
        const unsigned e = lodepng_convert(image.data(), own, &out, &state.info_png.color, w, h);
        std::printf(" %u ", e);
        if (e || image.empty()) std::printf("-");
        else for (unsigned char b : image) std::printf("%02x", b);
        lodepng_color_mode_cleanup(&out);
      }
    }
    std::free(own);
    std::printf("\n");
  }
  return 0;
}
