// TEST INFRASTRUCTURE — the oracle of the k_png_lo_* kernels below the zlib size: LodePNG's own LZ77 stage, block by block.
// `hash_init` and `encodeLZ77` are static functions of lodepng.cpp (:1507, :1593); this translation unit includes that file
// where it lies in the reference's tree (nothing copied) and puts C symbols in front of them.  Only tests/ loads the
// resulting library.
#include "lodepng.cpp"

// The blocks lodepng_deflatev (:2074) cuts `in` into under btype 2, each through encodeLZ77 with the default settings
// (minmatch 3, nicematch 128, lazy matching) at `window` on ONE Hash, as deflateDynamic (:1807) calls it; every block's
// uivector counted the way k_png_lo_parse counts (zmx_png_lodeflate.h kLoCountWords): 286 literal/length counts, 30
// distance counts, the extra bits' number as two words (low, high).  A match is four entries: the length symbol, its extra
// bits' value, the distance symbol, its extra bits' value.  `counts` has room for `cap` blocks; the blocks beyond are not
// written.  Returns the number of blocks, 0 on an error of LodePNG's.
extern "C" __attribute__((visibility("default"))) size_t ref_png_lo_counts(const unsigned char* in, size_t n, unsigned window, unsigned* counts,
                                                                            size_t cap) {
  LodePNGCompressSettings settings;
  lodepng_compress_settings_init(&settings);
  size_t blocksize = n / 8u + 8;
  if (blocksize < 65536) blocksize = 65536;
  if (blocksize > 262144) blocksize = 262144;
  size_t numblocks = (n + blocksize - 1) / blocksize;
  if (numblocks == 0) numblocks = 1;
  Hash hash;
  unsigned error = hash_init(&hash, window);
  for (size_t b = 0; b != numblocks && !error; ++b) {
    const size_t start = b * blocksize, end = start + blocksize > n ? n : start + blocksize;
    uivector lz77;
    uivector_init(&lz77);
    error = encodeLZ77(&lz77, &hash, in, start, end, window, settings.minmatch, settings.nicematch, settings.lazymatching);
    if (!error && b < cap) {
      unsigned* c = counts + b * 318;
      unsigned long long extra = 0;
      for (size_t i = 0; i != 318; ++i) c[i] = 0;
      for (size_t i = 0; i != lz77.size; ++i) {
        const unsigned symbol = lz77.data[i];
        ++c[symbol];
        if (symbol > 256) {
          const unsigned dist = lz77.data[i + 2];
          ++c[286 + dist];
          extra += LENGTHEXTRA[symbol - FIRST_LENGTH_CODE_INDEX] + DISTANCEEXTRA[dist];
          i += 3;
        }
      }
      c[316] = (unsigned)(extra & 0xffffffffu);
      c[317] = (unsigned)(extra >> 32);
    }
    uivector_cleanup(&lz77);
  }
  hash_cleanup(&hash);
  return error ? 0 : numblocks;
}

// lodepng_zlib_compress' length under the default settings at `window`; 0 on an error of LodePNG's.
extern "C" __attribute__((visibility("default"))) size_t ref_png_lo_zlib_size(const unsigned char* in, size_t n, unsigned window) {
  LodePNGCompressSettings settings;
  lodepng_compress_settings_init(&settings);
  settings.windowsize = window;
  unsigned char* out = 0;
  size_t outsize = 0;
  const unsigned error = lodepng_zlib_compress(&out, &outsize, in, n, &settings);
  lodepng_free(out);
  return error ? 0 : outsize;
}
