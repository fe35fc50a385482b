// TEST INFRASTRUCTURE — the oracle of k_png_brute below the filter type: what LodePNG's LFS_BRUTE_FORCE search compares,
// per row and per filter type.  `filterScanline`, `hash_init` and `encodeLZ77` are static functions of lodepng.cpp (:5379,
// :1507, :1593); this translation unit includes that file where it lies in the reference's tree (nothing copied) and puts
// a C symbol in front of them.  Only tests/ loads the resulting library.
#include "lodepng.cpp"

// For every job = row * 5 + type of an image of `height` rows of `linebytes` bytes (pixels of `bytewidth` bytes): the row
// filtered with `type` against the row above (none for row 0), then
//   bits[job]       3 + the symbols' bits + 7 under the fixed code: encodeLZ77 over the whole filtered row on a fresh Hash
//                   at `window`, minmatch 3, nicematch 128, lazy matching — what deflateFixed (:2029) does with the one
//                   block lodepng_deflatev (:2074) makes of the input under btype 1;
//   bytes[job]      the length lodepng_zlib_compress gives the filtered row with btype 1 at `window`: what filter()
//                   (:5585-5632) compares;
//   reach[job][6]   the emitted matches: their number, the largest offset, how many have length 258, how many length 3, the
//                   length of the first one, the largest length.
// Returns 0, or LodePNG's error.
extern "C" __attribute__((visibility("default"))) unsigned ref_png_brute_sizes(const unsigned char* image, size_t linebytes, size_t height,
                                                                                size_t bytewidth, unsigned window, unsigned long long* bits,
                                                                                unsigned long long* bytes, unsigned* reach) {
  LodePNGCompressSettings settings;
  lodepng_compress_settings_init(&settings);
  settings.btype = 1;
  settings.windowsize = window;
  unsigned char* row = (unsigned char*)lodepng_malloc(linebytes ? linebytes : 1);
  if (!row) return 83;
  unsigned error = 0;
  for (size_t y = 0; y != height && !error; ++y) {
    const unsigned char* prev = y ? image + (y - 1) * linebytes : 0;
    for (unsigned type = 0; type != 5 && !error; ++type) {
      const size_t job = y * 5 + type;
      filterScanline(row, image + y * linebytes, prev, linebytes, bytewidth, (unsigned char)type);
      Hash hash;
      uivector lz77;
      uivector_init(&lz77);
      error = hash_init(&hash, window);
      if (!error) error = encodeLZ77(&lz77, &hash, row, 0, linebytes, window, settings.minmatch, settings.nicematch, settings.lazymatching);
      if (!error) {
        unsigned long long b = 3 + 7;
        unsigned* r = reach + job * 6;
        r[0] = r[1] = r[2] = r[3] = r[4] = r[5] = 0;
        for (size_t i = 0; i != lz77.size; ++i) {
          const unsigned symbol = lz77.data[i];
          b += symbol < 144 ? 8 : symbol < 256 ? 9 : symbol < 280 ? 7 : 8;
          if (symbol > 256) {
            const unsigned length = LENGTHBASE[symbol - FIRST_LENGTH_CODE_INDEX] + lz77.data[i + 1];
            const unsigned dist = lz77.data[i + 2];
            const unsigned offset = DISTANCEBASE[dist] + lz77.data[i + 3];
            b += LENGTHEXTRA[symbol - FIRST_LENGTH_CODE_INDEX] + 5 + DISTANCEEXTRA[dist];
            if (r[0] == 0) r[4] = length;
            if (length > r[5]) r[5] = length;
            ++r[0];
            if (offset > r[1]) r[1] = offset;
            if (length == 258) ++r[2];
            if (length == 3) ++r[3];
            i += 3;
          }
        }
        bits[job] = b;
      }
      hash_cleanup(&hash);
      uivector_cleanup(&lz77);
      if (!error) {
        unsigned char* out = 0;
        size_t outsize = 0;
        error = lodepng_zlib_compress(&out, &outsize, row, linebytes, &settings);
        lodepng_free(out);
        bytes[job] = outsize;
      }
    }
  }
  lodepng_free(row);
  return error;
}

// The filter type LodePNG's filter() with LFS_BRUTE_FORCE puts in front of every row of the same image when its deflate
// window is `window`: types[height].  The image goes in as 8-bit grey, grey + alpha, RGB or RGBA (bytewidth 1 .. 4) or their
// 16-bit forms (bytewidth 6, 8): filter() only takes the bytes per pixel from the mode.  Error 31 where linebytes is no
// whole number of such pixels.
extern "C" __attribute__((visibility("default"))) unsigned ref_png_brute_types(const unsigned char* image, size_t linebytes, size_t height,
                                                                                size_t bytewidth, unsigned window, unsigned char* types) {
  LodePNGColorMode mode;
  lodepng_color_mode_init(&mode);
  switch (bytewidth) {
    case 1: mode.colortype = LCT_GREY; mode.bitdepth = 8; break;
    case 2: mode.colortype = LCT_GREY_ALPHA; mode.bitdepth = 8; break;
    case 3: mode.colortype = LCT_RGB; mode.bitdepth = 8; break;
    case 4: mode.colortype = LCT_RGBA; mode.bitdepth = 8; break;
    case 6: mode.colortype = LCT_RGB; mode.bitdepth = 16; break;
    case 8: mode.colortype = LCT_RGBA; mode.bitdepth = 16; break;
    default: return 31;
  }
  if (linebytes % bytewidth != 0) return 31;
  LodePNGEncoderSettings settings;
  lodepng_encoder_settings_init(&settings);
  settings.filter_palette_zero = 0;
  settings.filter_strategy = LFS_BRUTE_FORCE;
  settings.zlibsettings.windowsize = window;
  unsigned char* out = (unsigned char*)lodepng_malloc(height * (linebytes + 1) + 1);
  if (!out) return 83;
  const unsigned error = filter(out, image, (unsigned)(linebytes / bytewidth), (unsigned)height, &mode, &settings);
  for (size_t y = 0; y != height && !error; ++y) types[y] = out[y * (linebytes + 1)];
  lodepng_free(out);
  return error;
}
