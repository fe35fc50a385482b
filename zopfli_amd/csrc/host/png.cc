// The pooled form of zopflipng's brute-force row search (include/zopfli_amd.h): zmx_png_filter_types_brute
// on one of the entry points' contexts, as zmx_png_filter_types_pooled is in api.cc — what libzopflipng_amd.so calls.
// (Outside api.cc, which calls no device function the device layer added since: the host-only test library links
// api.cc against a stand-in for that layer.)
#include "dealing.h"
#include "zopfli_amd.h"

extern "C" int zmx_png_filter_types_brute_pooled(const unsigned char* image, size_t linebytes, size_t height,
                                                 size_t bytewidth, unsigned windowsize, unsigned char* types) {
  return zamd::OnPooledContext([&](zmx_ctx* ctx) {
    return zmx_png_filter_types_brute(ctx, image, linebytes, height, bytewidth, windowsize, types);
  });
}
