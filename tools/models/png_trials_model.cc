// The trial file sizes of zopflipng's automatic filter-strategy choice, from zopflipng's own code: its TryOptimize
// (zopflipng_lib.cc) is called for a PNG file the way AutoChooseFilterStrategy calls it — LodePNG's own deflate at window
// 8192, the strategies zero, one, two, three, four, minimum sum, entropy, predefined — after the decoding and the lossy
// steps of ZopfliPNGOptimize.  tests/golden/make_png_trials_golden.py records what it prints.  Nothing is copied: the
// reference's sources are compiled in from wherever they lie,
//   g++ -O2 -w -I $PNGSRC tools/models/png_trials_model.cc $PNGSRC/zopflipng_lib.cc $PNGSRC/lodepng/lodepng.cpp \
//       $PNGSRC/lodepng/lodepng_util.cpp <the objects of the reference's libzopfli> -o png_trials_model
//   png_trials_model FILE.png KEEPCOLORTYPE LOSSY_TRANSPARENT LOSSY_8BIT     prints the eight sizes and the chosen index
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lodepng/lodepng.h"
#include "zopflipng_lib.h"

// (zopflipng_lib.cc's, not in its header)
unsigned TryOptimize(const std::vector<unsigned char>& image, unsigned w, unsigned h, const lodepng::State& inputstate, bool bit16,
                     bool keep_colortype, const std::vector<unsigned char>& origfile, ZopfliPNGFilterStrategy filterstrategy, bool use_zopfli,
                     int windowsize, const ZopfliPNGOptions* png_options, std::vector<unsigned char>* out);
void LossyOptimizeTransparent(lodepng::State* inputstate, unsigned char* image, unsigned w, unsigned h);

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const bool keep = atoi(argv[2]) != 0, lossy_transparent = atoi(argv[3]) != 0, lossy_8bit = atoi(argv[4]) != 0;
  std::vector<unsigned char> file, image;
  if (lodepng::load_file(file, argv[1]) != 0) return 2;
  unsigned w = 0, h = 0;
  lodepng::State inputstate;
  if (lodepng::decode(image, w, h, inputstate, file) != 0) return 3;
  bool bit16 = false;
  if (inputstate.info_png.color.bitdepth == 16 && (keep || !lossy_8bit)) {
    image.clear();
    if (lodepng::decode(image, w, h, file, LCT_RGBA, 16) != 0) return 3;
    bit16 = true;
  }
  if (lossy_transparent && !bit16) LossyOptimizeTransparent(&inputstate, &image[0], w, h);
  const ZopfliPNGFilterStrategy order[8] = {kStrategyZero,  kStrategyOne,    kStrategyTwo,     kStrategyThree,
                                            kStrategyFour,  kStrategyMinSum, kStrategyEntropy, kStrategyPredefined};
  size_t best = 0, bestsize = 0;
  for (size_t k = 0; k < 8; ++k) {
    std::vector<unsigned char> out;
    if (TryOptimize(image, w, h, inputstate, bit16, keep, file, order[k], false, 8192, 0, &out) != 0) return 4;
    if (bestsize == 0 || out.size() < bestsize) {
      bestsize = out.size();
      best = k;
    }
    printf("%zu ", out.size());
  }
  printf("%zu\n", best);
  return 0;
}
