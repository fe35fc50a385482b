// zmx_compress_device_to_device: ZopfliCompress of bytes in device memory INTO device memory.
//
// The call runs as zmx_compress_device's does (device_input.cc, dealing.h) with two differences.  The shards run with
// g_device_output set, so the blocks the device writes keep their bits where they are (deflate.cc: kDeviceBits chunks) and
// the stored blocks' bytes are not fetched.  And where a host call merges its chunks into a malloc'ed array, this one
// plans the stream as a table of bit pieces (device_output_plan.h) — container header, block headers and trees, LEN / NLEN,
// the trailer and whatever blocks the host had to write from one small uploaded buffer; the symbols' bits from the bit
// writer's buffers; stored bytes from the caller's input — and one zmx_bitjoin_device puts it together in d_out, while the
// call still holds its contexts (the bit buffers are theirs).  The stream's size is known from the plan, before anything
// is written.
// zamd::CompressDeviceToDevice is that call with an optional FRAME (device_output_plan.h: PngFrame) for the PNG entries of
// png_encode.cc: the file's prefix and 78 01 in place of the container's header, a CRC placeholder and IEND behind the
// trailer, and after the join — on the same hold of the contexts — the IDAT's CRC-32 sealed into the placeholder by
// zmx_internal_checksum_seal.  Without a frame nothing differs: the same plan, the same launches.
#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "dealing.h"
#include "device_output_plan.h"
#include "host_knobs.h"
#include "symbols.h"
#include "zmx_internal.h"
#include "zopfli_amd.h"

namespace {

int Refuse(const std::string& msg) {
  zmx_internal_set_error(msg.c_str(), ZMX_ERR_REFUSED);
  return -1;
}

}  // namespace

extern "C" size_t zmx_compress_bound(ZopfliFormat output_type, size_t insize) { return zamd::CompressBound(output_type, insize); }

extern "C" size_t zmx_compress_batch_bound(ZopfliFormat output_type, size_t n, const size_t* insize, size_t align) {
  if (n == 0 || !insize || !zamd::PackedAlignOk(align)) return 0;
  return zamd::CompressBatchBound(output_type, n, insize, align);
}

int zamd::CompressDeviceToDevice(const char* kWho, const ZopfliOptions* options, ZopfliFormat output_type, const void* d_in, size_t insize,
                                 void* d_out, size_t capacity, size_t* outsize, const zamd::PngFrame* frame) {
  if (!options || !outsize) return Refuse(std::string(kWho) + ": null argument");
  *outsize = 0;
  if (output_type != ZOPFLI_FORMAT_GZIP && output_type != ZOPFLI_FORMAT_ZLIB && output_type != ZOPFLI_FORMAT_DEFLATE) {
    return Refuse(std::string(kWho) + ": invalid ZopfliFormat " + std::to_string(static_cast<int>(output_type)));
  }
  int in_device = -1, out_device = -1;
  if (zmx_internal_device_pointer(kWho, d_in, insize, &in_device) != 0) return -1;
  if (capacity != 0 && d_out == nullptr) return Refuse(std::string(kWho) + ": d_out: null pointer with a non-zero size");
  if (zmx_internal_device_pointer((std::string(kWho) + ": d_out").c_str(), d_out, capacity, &out_device) != 0) return -1;
  if (insize != 0 && capacity != 0) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (a < b + capacity && b < a + insize) return Refuse(std::string(kWho) + ": d_out overlaps d_in");
    // (the join reads the stored blocks' bytes from d_in itself: one device, as for the contexts — the limits in the header)
    if (in_device != out_device) return Refuse(std::string(kWho) + ": d_in and d_out lie on different devices");
  }
  const size_t round_parts = std::max<size_t>(zamd::HostSwitches().round_parts, 1);
  const std::vector<zamd::Part> parts = zamd::InputMasterBlocks(insize, true);
  if (parts.size() > round_parts) {
    return Refuse(std::string(kWho) + ": " + std::to_string(parts.size()) + " master blocks are more than one round (ZOPFLI_AMD_ROUND_PARTS = " +
                  std::to_string(round_parts) + "): not joined on the device");
  }
  zamd::ResetCallStats();
  zamd::DeviceInput dev;
  dev.round_parts = round_parts;
  dev.upload = [&](zmx_ctx* ctx, size_t base, size_t n) {
    return zmx_set_input_device(ctx, static_cast<const unsigned char*>(d_in) + base, n);
  };
  dev.device_output = true;
  dev.only_device = out_device >= 0 ? out_device : in_device;
  bool too_small = false;
  size_t written = 0;
  dev.finish = [&](zmx_ctx* ctx, std::vector<zamd::Chunk>* chunks, uint32_t sum) {
    std::vector<uint8_t> trailer = zamd::ContainerTrailer(output_type, sum, insize);
    if (frame) trailer = zamd::PngFrameTrailer(std::move(trailer));
    zamd::OutputPlan plan = zamd::PlanOutput(frame ? zamd::PngFrameHeader(*frame) : zamd::ContainerHeader(output_type), *chunks,
                                             static_cast<const unsigned char*>(d_in), trailer);
    const size_t need = static_cast<size_t>(plan.total_bits / 8);
    if (frame && !zamd::PngFrameSetLength(*frame, &plan)) {
      too_small = true;
      written = need;
      return Refuse(std::string(kWho) + ": the zlib stream does not fit an IDAT chunk");
    }
    if (need > capacity) {
      too_small = true;
      written = need;
      return Refuse(std::string(kWho) + ": the stream takes " + std::to_string(need) + " bytes, d_out has " + std::to_string(capacity));
    }
    std::vector<zmx_bit_piece> pieces(plan.pieces.size());
    std::vector<unsigned char> is_literal(plan.pieces.size());
    for (size_t i = 0; i < pieces.size(); ++i) {
      const zamd::PlanPiece& q = plan.pieces[i];
      is_literal[i] = q.literal;
      pieces[i] = {q.literal ? reinterpret_cast<const void*>(q.lit) : q.dev, q.src_bit, q.nbits, q.dst_bit};
    }
    if (zmx_internal_bitjoin_literals(ctx, plan.literals.data(), plan.literals.size(), pieces.size(), pieces.data(), is_literal.data(),
                                      plan.total_bits, d_out, capacity) != 0) return -1;
    if (frame) {
      // the IDAT's CRC-32 over its type and the joined stream, into the placeholder behind it
      unsigned char* const file = static_cast<unsigned char*>(d_out);
      const size_t prefix = frame->file_prefix.size();
      const void* from = file + prefix - 4;
      const size_t covered = 4 + static_cast<size_t>(zamd::PngFrameIdatBytes(need, prefix));
      unsigned char* seal = file + need - zamd::kPngTrailerBytes;
      if (zmx_internal_checksum_seal(ctx, ZMX_CRC32, 1, &from, &covered, &seal) != 0) return -1;
    }
    const double traffic[4] = {0, static_cast<double>(plan.literals.size()), static_cast<double>(plan.device_blocks),
                               static_cast<double>(plan.host_blocks)};
    zamd::SetOutputTraffic(traffic);
    written = need;
    return 0;
  };
  // (one master block: one shard on one context, whatever its bytes — nothing reads the counts)
  if (insize > zamd::kMasterBlock && zamd::ProbeDeviceInput(d_in, insize, in_device, &dev) != 0) return -1;
  zamd::ChecksumRequest sum{output_type == ZOPFLI_FORMAT_GZIP ? ZMX_CRC32 : ZMX_ADLER32,
                            output_type == ZOPFLI_FORMAT_GZIP ? insize : static_cast<unsigned>(insize), 0};   // (zlib_container.c:54 truncates)
  if (zamd::RunPartsToDevice(*options, parts, output_type == ZOPFLI_FORMAT_DEFLATE ? nullptr : &sum, &dev) != 0) {
    zmx_internal_set_error(dev.error.c_str(), dev.error_class);
    if (too_small) *outsize = written;
    return -1;
  }
  *outsize = written;
  return 0;
}

extern "C" int zmx_compress_device_to_device(const ZopfliOptions* options, ZopfliFormat output_type, const void* d_in,
                                             size_t insize, void* d_out, size_t capacity, size_t* outsize) {
  return zamd::CompressDeviceToDevice("zmx_compress_device_to_device", options, output_type, d_in, insize, d_out, capacity, outsize, nullptr);
}
