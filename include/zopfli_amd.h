/*
 * zopfli_amd — MI355X-native drop-in for the LZ77 optimal-parse hot path of
 * google/zopfli.  C ABI of libzopfli_amd.so.
 *
 * Part 1 is the reference's own public surface (same names, same struct
 * layout, same ownership rules), so existing callers of libzopfli — the CLI
 * (zopfli_bin.c:112), the cgo binding (go/zopfli/zopfli.go:46) and zopflipng's
 * CustomPNGDeflate (zopflipng_lib.cc:60) — link against this library unchanged.
 *
 * Part 2 is the thin device layer the host code calls into ("zmx_*"): plain
 * pointers and sizes, opaque handles, int status (0 = ok), no exceptions.
 * Each entry point names the reference function whose work it replaces.
 * There is no CPU fallback: every zmx_* call fails (non-zero) and the
 * Zopfli* calls abort with a message if no gfx950 device is usable.
 */
#ifndef ZOPFLI_AMD_H_
#define ZOPFLI_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libzopfli_amd.so is built with -fvisibility=hidden: exactly the functions declared here are
 * exported (plus one test hook). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Errors.  The reference's entry points return void; like the reference (which exit()s when malloc
 * fails, util.h:135-155) the Zopfli* functions below print a message to stderr and exit(EXIT_FAILURE)
 * when the device side fails: no usable gfx950 device, a HIP error such as an allocation that does
 * not fit in HBM, or a single deflate block whose DP edges do not fit 32-bit row offsets (more than
 * 2^32 - 65536 match-length candidates in one block: some 150 - 300 MB of input in ONE block, which only
 * ZopfliDeflatePart with blocksplitting = 0 can ask for — ZopfliDeflate and ZopfliCompress cut their
 * input into 1 000 000-byte master blocks first).  The zmx_* functions of part 2 return non-zero instead
 * and leave a message for zmx_last_error().
 *
 * Devices and threads.  The Zopfli* functions run on ONE device unless told otherwise: ZOPFLI_AMD_DEVICE,
 * else LOCAL_RANK, else device 0; ZOPFLI_AMD_DEVICES = "all" | a count | a list of indices deals the master
 * blocks of a call over several.  They may be called from several threads at once (as the reference's may):
 * a device has ZOPFLI_AMD_LANES contexts (default 3), a call takes what it needs and later callers wait. */

/* ------------------------------------------------------------------ Part 1 */

/* reference: src/zopfli/zopfli.h:33-64 (six ints, this order) */
typedef struct ZopfliOptions {
  int verbose;
  int verbose_more;
  int numiterations;
  int blocksplitting;
  int blocksplittinglast; /* unused, kept for layout compatibility */
  int blocksplittingmax;
} ZopfliOptions;

/* reference: src/zopfli/zopfli.h:70-74 */
typedef enum {
  ZOPFLI_FORMAT_GZIP,
  ZOPFLI_FORMAT_ZLIB,
  ZOPFLI_FORMAT_DEFLATE
} ZopfliFormat;

/* reference: src/zopfli/util.c:28 — numiterations 15, blocksplitting 1, max 15 */
void ZopfliInitOptions(ZopfliOptions* options);

/* reference: src/zopfli/zopfli_lib.c:28.  Appends to the malloc'ed array
 * (*out, *outsize); caller frees.  Capacity keeps the reference's
 * power-of-two invariant (util.h:135-155) so callers may keep appending. */
void ZopfliCompress(const ZopfliOptions* options, ZopfliFormat output_type,
                    const unsigned char* in, size_t insize,
                    unsigned char** out, size_t* outsize);

/* reference: src/zopfli/deflate.c:908 (deflate.h:58).  `bp` = bits already used
 * in the last output byte (0..7), carried between calls. */
void ZopfliDeflate(const ZopfliOptions* options, int btype, int final,
                   const unsigned char* in, size_t insize,
                   unsigned char* bp, unsigned char** out, size_t* outsize);

/* reference: src/zopfli/deflate.c:811 (deflate.h:67).  Reads only
 * in[max(0,instart-32768) .. inend). */
void ZopfliDeflatePart(const ZopfliOptions* options, int btype, int final,
                       const unsigned char* in, size_t instart, size_t inend,
                       unsigned char* bp, unsigned char** out, size_t* outsize);

/* reference: src/zopfli/gzip_container.c:84 */
void ZopfliGzipCompress(const ZopfliOptions* options,
                        const unsigned char* in, size_t insize,
                        unsigned char** out, size_t* outsize);

/* reference: src/zopfli/zlib_container.c:50 */
void ZopfliZlibCompress(const ZopfliOptions* options,
                        const unsigned char* in, size_t insize,
                        unsigned char** out, size_t* outsize);

/* reference: src/zopfli/lz77.h:44-62 — the LZ77 symbol sequence of the reference's own API, as far as the two
 * functions below read it: litlens / dists (lz77.c:98: a literal is (byte, 0), a match (length, distance)), their
 * number, and pos (the byte position of every symbol in the input).  The cumulative histograms the reference keeps
 * beside them (ll_symbol ... d_counts) are not read here. */
typedef struct ZopfliLZ77Store {
  unsigned short* litlens;
  unsigned short* dists;
  size_t size;
  const unsigned char* data;
  size_t* pos;
  unsigned short* ll_symbol;
  unsigned short* d_symbol;
  size_t* ll_counts;
  size_t* d_counts;
} ZopfliLZ77Store;

/* reference: src/zopfli/deflate.c:584-608 (deflate.h:79).  Size in bits of symbols [lstart, lend) as one block of
 * type `btype` (0 stored, 1 fixed, 2 dynamic: tree included).  Host arithmetic (the block-cost code the block
 * splitter and the iteration driver use: host/block_cost.cc); no device call. */
double ZopfliCalculateBlockSize(const ZopfliLZ77Store* lz77, size_t lstart, size_t lend, int btype);

/* reference: src/zopfli/deflate.c:610-621 (deflate.h:85): the smallest of the three. */
double ZopfliCalculateBlockSizeAutoType(const ZopfliLZ77Store* lz77, size_t lstart, size_t lend);

/* ------------------------------------------------------------------ Part 2 */

typedef struct zmx_ctx zmx_ctx;       /* one HIP device + stream + resident input */
typedef struct zmx_tables zmx_tables; /* match tables + LZ77 stores of a batch of blocks */

/* One deflate block: bytes [instart, inend) of the resident input.  Matches may
 * reach back to max(0, instart-32768) — or to the start of the block's segment, when
 * zmx_set_input_segments declared some — and never extend past inend
 * (lz77.c:551-552, squeeze.c:229-230). */
typedef struct zmx_block {
  uint64_t instart;
  uint64_t inend;
} zmx_block;

#define ZMX_NUM_LL 288
#define ZMX_NUM_D 32
#define ZMX_HIST (ZMX_NUM_LL + ZMX_NUM_D) /* litlen bins then dist bins */

int zmx_device_count(void);
/* The message of the last failed zmx_* call on the calling thread. */
const char* zmx_last_error(void);
/* ... and what kind of failure it was.  Callers that decide whether doing the work again elsewhere can help (api.cc: a
 * failed shard is done again on another context) go by this code, never by the message's text. */
#define ZMX_ERR_NONE 0
#define ZMX_ERR_DEVICE 1         /* a HIP call failed or the device misbehaved: another context / device may fare better */
#define ZMX_ERR_OUT_OF_MEMORY 2  /* hipErrorOutOfMemory: likewise (another context may have the room) */
#define ZMX_ERR_REFUSED 3        /* the request itself is refused — bad arguments, a size limit, a pool that still
                                    overflows after the device layer's own retries: it would fail the same way anywhere */
int zmx_last_error_class(void);
/* The host arrays of a call (symbol stores, bit buffers) take their memory from a cache of large blocks the library keeps
 * between calls (at most ZOPFLI_AMD_HOST_CACHE_MB, default 1024; zopfli_amd/csrc/host/block_cache.h) instead of changing
 * the host process's malloc settings.  This frees everything cached and returns the number of bytes given back. */
size_t zmx_host_cache_trim(void);
/* always 0; kept for ABI */
int zmx_has_experiments(void);

int zmx_ctx_create(int device, zmx_ctx** ctx);
void zmx_ctx_destroy(zmx_ctx* ctx);

/* Copies the whole input to HBM once; the kernels work on that copy.  The host side keeps reading a
 * few bytes of `in` itself (the ends of blocks when match tables are reused, the bytes of stored
 * blocks): `in` must stay valid and unchanged until the next zmx_set_input or zmx_ctx_destroy on
 * this context.  The calling thread's current HIP device is left as it was. */
int zmx_set_input(zmx_ctx* ctx, const unsigned char* in, size_t insize);

/* The same for bytes that already lie in device memory (a tensor, a checkpoint shard, a rendered frame): `d_in` is a
 * device pointer, of this context's device or of another one (the bytes are copied into the context's own buffer with
 * hipMemcpyDefault semantics, padded as for zmx_set_input).  The caller's buffer is only read, and only during the
 * call: it need not outlive it, and the host keeps no pointer to the input — what it used to read of `in` (block ends,
 * stored blocks' bytes) it takes from the context's copy.  The data must be complete when the call is made: the caller
 * synchronises the stream that produced it.  Refused on the host, before any copy or launch (ZMX_ERR_REFUSED): a null
 * pointer with a non-zero size, a pointer that is not device memory (host memory, pinned or not), managed memory, a
 * range that leaves its allocation.  insize = 0 is valid with any pointer. */
int zmx_set_input_device(zmx_ctx* ctx, const void* d_in, size_t insize);

/* d_dst[0, sum nbytes) = the bytes of d_src[0], d_src[1], ... end to end.  Every source and the destination are checked as
 * zmx_set_input_device checks its pointer (ZMX_ERR_REFUSED before any launch: null with a size, host or managed memory,
 * a range that leaves its allocation), and so is a destination that overlaps a source or that does not lie on the
 * context's device.  Sources on the context's device go through one kernel launch (k_gather, device/zmx_gather.h: at
 * most 2048 workgroups whatever n and the total); sources on another device take one hipMemcpyDefault copy each.
 * Empty pieces are allowed, with any pointer.  The resident input is not touched.  Synchronous.  (While kernel timing
 * is on — zmx_set_kernel_timing — the call records two events around its copies, like the squeeze runs' phase times;
 * the measuring tool reads the milliseconds through zmx_internal_gather_ms.  Off, it records none.) */
int zmx_gather_device(zmx_ctx* ctx, size_t n, const void* const* d_src, const size_t* nbytes, void* d_dst);

/* Declares the resident input (the last zmx_set_input, which resets it to one segment) to be the concatenation of nseg
 * independent inputs: segment i is bytes [starts[i], starts[i + 1]), the last one ends at the input's end; starts[0] = 0,
 * the starts never decrease and none lies past the end (empty segments are allowed).  From this call on the window of a
 * block built by zmx_tables_build* reaches back to max(start of its segment, instart - 32768) instead of
 * max(0, instart - 32768): each input is compressed as if it were alone.  A block that spans two segments is refused
 * (ZMX_ERR_REFUSED). */
int zmx_set_input_segments(zmx_ctx* ctx, const uint64_t* starts, size_t nseg);

/* Kernel A.  For every block: the static hash arrays (hash.c:100-137 val/same/
 * prev links as pure functions of the data and inend) and, for every position,
 * the result of ZopfliFindLongestMatch(limit 258, sublen) (lz77.c:407-542):
 * longest length, its distance and the sublen step function.  Replaces the
 * hash replay + longest-match cache (cache.c) of the reference. */
int zmx_tables_build(zmx_ctx* ctx, const zmx_block* blocks, size_t nblocks, zmx_tables** tables);

/* The same without what only zmx_squeeze_run reads (the DP rows and their weight codes: two bytes for each of the up to
 * 258 edges of a position): for zmx_lz77_greedy, zmx_store_download / zmx_verify of its store, and as `parent` of
 * zmx_tables_build_from — the greedy pass over a master block that is about to be split (blocksplitter.c:296).
 * zmx_squeeze_run on such tables fails. */
int zmx_tables_build_matches(zmx_ctx* ctx, const zmx_block* blocks, size_t nblocks, zmx_tables** tables);

/* The same, for blocks that lie inside blocks of `parent` (both lists ascending), e.g. the deflate
 * blocks a master block was split into (deflate.c:854-869) after the greedy pass over the master
 * block (blocksplitter.c:296): ZopfliFindLongestMatch depends on the block only through its end
 * (lz77.c:448-450, hash.c:107-108,121), so the parent's results are reused for every position but
 * those near the new block ends.  `parent` stays valid for zmx_tables_free only.  parent = NULL
 * is zmx_tables_build. */
int zmx_tables_build_from(zmx_ctx* ctx, zmx_tables* parent, const zmx_block* blocks, size_t nblocks,
                          zmx_tables** tables);
void zmx_tables_free(zmx_ctx* ctx, zmx_tables* tables);

/* Gives back everything of a table set but its two LZ77 stores: afterwards only zmx_store_download*, zmx_encode_blocks
 * and zmx_tables_free work on it (the others fail with a message).  For the caller that keeps the tables of a finished
 * batch around for the device's bit writer while it builds the next ones (deflate.c:760: the fixed-tree re-parses). */
int zmx_tables_trim(zmx_ctx* ctx, zmx_tables* tables);

/* ZopfliLZ77Greedy (lz77.c:544-630) on every block, into store slot `slot`
 * (0 or 1).  nsym[b] = symbols emitted, hist[b*ZMX_HIST..] = their histogram
 * (litlen bins 0..287 then dist bins 0..31, end symbol not counted). */
int zmx_lz77_greedy(zmx_ctx* ctx, zmx_tables* tables, int slot, uint32_t* nsym, uint32_t* hist);

/* One LZ77OptimalRun (squeeze.c:429): GetBestLengths (:217) forward DP with the
 * given per-block cost model, TraceBackwards (:317), FollowPath (:338).
 * cost[b*ZMX_HIST..] = ll_symbols[288] then d_symbols[32] in bits, mincost[b] =
 * GetCostModelMinCost (:163).  slot[b] selects the store written for block b.
 * The oracle defines the meaning of any other mincost[b]: GetBestLengths with the mincost it is given (:293 skips an
 * edge of length k at j when costs[j + k] <= mincost + costs[j], with exactly that value). */
int zmx_squeeze_run(zmx_ctx* ctx, zmx_tables* tables, const double* cost, const double* mincost,
                    const int32_t* slot, uint32_t* nsym, uint32_t* hist);

/* Copies store `slot` of block `block` (nsym entries) to the host: litlens[i] is
 * a literal byte when dists[i]==0, else a match length (lz77.h:44-49). */
int zmx_store_download(zmx_ctx* ctx, zmx_tables* tables, size_t block, int slot,
                       uint16_t* litlens, uint16_t* dists, size_t nsym);

/* The same for n stores at once (one device-to-host transfer set, one synchronisation):
 * store slot[i] of block block[i], nsym[i] entries, into litlens[i] / dists[i]. */
int zmx_store_download_batch(zmx_ctx* ctx, zmx_tables* tables, size_t n, const size_t* block,
                             const int32_t* slot, const size_t* nsym, uint16_t* const* litlens,
                             uint16_t* const* dists);

/* ZopfliVerifyLenDist (lz77.c:270-295) over whole stores, on the device: every literal is the input byte at its
 * position, every (length, distance) is in range and copies equal bytes, and the symbols cover the block exactly.
 * The reference asserts this for each symbol it stores (lz77.c:115, debug builds); here it is a separate pass,
 * run by the Zopfli* entry points on every parse they keep when ZOPFLI_AMD_VERIFY is set.  Returns 0 or fails
 * with the first offending block and symbol in zmx_last_error. */
int zmx_verify_stores(zmx_ctx* ctx, zmx_tables* tables, size_t n, const size_t* block, const int32_t* slot,
                      const size_t* nsym);

/* The deflate bit writer on the device: AddLZ77Data + the end symbol (deflate.c:297-333, :735-737) of a compressed
 * block whose LZ77 symbols are a whole store of `tables` — only the bits come down, not the symbols.
 * codes[j * 320 + s] = (Huffman code of symbol s, bit-reversed as the stream wants it) | (code length << 16) for
 * the 288 litlen symbols, then the 32 distance symbols, of job j (LengthsToSymbols, tree.c:50-69, on the host).
 * Job j's symbols start at bit `bit_start` of out[j] (the caller puts the block header and the tree in front: those
 * bits come back zero), out[j] has room for (bit_start + nbits + 7) / 8 bytes; `nbits` = what the caller expects
 * the symbols and the end symbol to take (from the histogram) and is checked. */
typedef struct zmx_enc_job {
  uint32_t block;      /* block of the table set */
  int32_t slot;        /* which of its two stores */
  uint32_t nsym;       /* symbols in that store */
  uint32_t bit_start;
  uint64_t nbits;
} zmx_enc_job;
int zmx_encode_blocks(zmx_ctx* ctx, zmx_tables* tables, size_t njobs, const zmx_enc_job* jobs,
                      const uint32_t* codes, unsigned char* const* out);

/* The same bit writer — the same jobs and codes, the same three kernels, the same check of `nbits` — whose bits stay in
 * device memory: *bits owns one allocation of the context that outlives the call (zmx_bits_free gives it back, on the
 * same context, once nothing reads it any more); nothing is copied to the host but the flag of the check.
 * zmx_bits_job: job `job`'s bit string — *d_bits is 8-byte aligned device memory, the symbols are bits
 * [*bit_start, *bit_start + *nbits) of it, deflate's bit order; bits [0, *bit_start), where the block's header and tree
 * go, are zero (in zmx_bitjoin_device the header is a piece of its own).  njobs = 0 gives an empty set. */
typedef struct zmx_bits zmx_bits;
int zmx_encode_blocks_device(zmx_ctx* ctx, zmx_tables* tables, size_t njobs, const zmx_enc_job* jobs,
                             const uint32_t* codes, zmx_bits** bits);
size_t zmx_bits_jobs(const zmx_bits* bits);
int zmx_bits_job(const zmx_bits* bits, size_t job, const void** d_bits, uint64_t* bit_start, uint64_t* nbits);
void zmx_bits_free(zmx_ctx* ctx, zmx_bits* bits);

/* A bit-granular gather: n bit strings of device memory joined into the bit string at d_dst in one launch (k_bitjoin,
 * device/zmx_bitjoin.h: at most 2048 workgroups whatever n and the total).  Bit k of a string at p is
 * (p[k / 8] >> (k % 8)) & 1, deflate's order.  Piece i is bits [src_bit, src_bit + nbits) of the string at src and
 * becomes bits [dst_bit, dst_bit + nbits) of the destination.  The pieces are sorted by dst_bit and none, an empty one
 * included, begins before the one in front of it ends; total_bits is at least the last piece's end.
 * Every byte of d_dst[0, (total_bits + 7) / 8) is written exactly once, whole; bits that no piece covers — gaps, the tail
 * of the last byte — are 0; no byte beyond is written, and the destination need not be zeroed first.  Nothing is read
 * but the aligned 4-byte words that hold a bit of a piece.  d_dst and every src may have any byte alignment.
 * Refused on the host before any launch (ZMX_ERR_REFUSED; where a piece is at fault the message names it, "piece i"):
 * a null pointer with bits, host or managed memory, a range that leaves its allocation, a destination that overlaps a
 * source or is not memory of the context's device, a source on another device, pieces that are unsorted or overlap, a
 * bit count of 2^60 or more, total_bits below the last piece's end or above 8 * dst_capacity.  total_bits = 0 returns 0
 * and launches nothing.  Synchronous.  (Timed while kernel timing is on, as zmx_gather_device is.) */
typedef struct zmx_bit_piece {
  const void* src;
  uint64_t src_bit;
  uint64_t nbits;
  uint64_t dst_bit;
} zmx_bit_piece;
int zmx_bitjoin_device(zmx_ctx* ctx, size_t n, const zmx_bit_piece* pieces, uint64_t total_bits, void* d_dst,
                       size_t dst_capacity);

/* zmx_bitjoin_device for ndst destinations in ONE launch (k_bitjoin_many: still at most 2048 workgroups, whatever ndst,
 * npieces and the total) and one synchronisation.  Destination d is the bit string at dests[d].dst, made from pieces
 * [first_piece, first_piece + npieces) of the one table `pieces`; a piece's dst_bit counts from its own destination, and
 * within a destination the pieces follow zmx_bitjoin_device's rules.  The piece ranges of consecutive destinations are
 * consecutive: dests[0].first_piece = 0, and the last range ends at npieces.  capacity[d] is the room at dests[d].dst in
 * bytes (a null `capacity`: exactly (total_bits + 7) / 8 each).
 * Every byte of every dst[0, (total_bits + 7) / 8) is written exactly once and no byte outside those ranges, so
 * destinations may lie back to back at any byte alignment, two of them inside one 16-byte vector; a destination of
 * total_bits 0 is not touched.  Refused before any upload or launch (ZMX_ERR_REFUSED; the message names "destination d",
 * and "piece i" counted within it): a null table with a non-zero count, piece ranges that are not consecutive or leave
 * npieces, whatever zmx_bitjoin_device refuses of a destination and its pieces, two destinations that share a byte, a
 * piece whose source bytes share a byte with any destination, memory that is not the context's device's.  ndst = 0, or
 * no destination with a bit, returns 0 and launches nothing.  Synchronous; timed as zmx_bitjoin_device is. */
typedef struct zmx_bit_dest {
  void* dst;
  uint64_t total_bits;
  uint64_t first_piece;
  uint64_t npieces;
} zmx_bit_dest;
int zmx_bitjoin_many_device(zmx_ctx* ctx, size_t ndst, const zmx_bit_dest* dests, const size_t* capacity, size_t npieces,
                            const zmx_bit_piece* pieces);

/* CRC-32 (gzip_container.c:75, the value ZopfliGzipCompress writes at :107-110) or Adler-32
 * (zlib_container.c:29, written at :71-74) of bytes [begin, end) of the resident input
 * (zmx_set_input), computed on the device; f-2 of SURVEY 8.  `value` is the finished checksum of
 * the range on its own.  Ranges that lie on different devices or ranks are put together with
 * zmx_checksum_combine(kind, checksum of A, checksum of B, bytes in B) = checksum of A followed
 * by B (host arithmetic only, no context needed). */
#define ZMX_CRC32 0
#define ZMX_ADLER32 1
int zmx_checksum(zmx_ctx* ctx, int kind, size_t begin, size_t end, uint32_t* value);
/* The same for n ranges [begin[i], end[i]) at once (one launch set, one synchronisation): values[i] = the checksum of
 * range i on its own; an empty range gives the initial value (CRC-32 0, Adler-32 1).  For the containers of a batch of
 * inputs (zmx_compress_batch). */
int zmx_checksums(zmx_ctx* ctx, int kind, size_t n, const uint64_t* begin, const uint64_t* end, uint32_t* values);
uint32_t zmx_checksum_combine(int kind, uint32_t a, uint32_t b, uint64_t len_b);
/* The same for n ranges of ARBITRARY device memory: values[i] = the checksum of d_ptr[i][0, nbytes[i]) on its own.  A range
 * may start at any byte address, have any length and lie in any allocation of the context's device; no byte outside a
 * range is read.  k_checksum_pieces (k_checksum's geometry: 256 KiB pieces counted from the range's end) and
 * k_checksum_finish (device/zmx_checksum_device.h) follow each other on the context's stream, each ONE launch for any n:
 * the pieces are combined and the checksum finished on the device, and only 4 * n bytes come down.  An empty range gives
 * the initial value (CRC-32 0, Adler-32 1); n = 0 returns 0 and launches nothing.  Refused before any launch
 * (ZMX_ERR_REFUSED), `values` untouched: a null array, an unknown kind, and — the message naming "range i" — a null
 * pointer with bytes, host or managed memory, a range that leaves its allocation, memory of another device than the
 * context's.  Synchronous; the caller synchronises the streams that produced the bytes. */
int zmx_checksum_device(zmx_ctx* ctx, int kind, size_t n, const void* const* d_ptr, const size_t* nbytes, uint32_t* values);

/* Parity probe: the ZopfliFindLongestMatch result for one position of one
 * block, expanded to the reference's sublen[259] convention. */
int zmx_find_longest_match(zmx_ctx* ctx, zmx_tables* tables, size_t block, size_t pos,
                           uint16_t* sublen, uint16_t* distance, uint16_t* length);

/* -------- zopflipng's per-row filter search
 *
 * The PNG filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) LodePNG's encoder picks for each of `height` scanlines
 * of `linebytes` bytes under its LFS_MINSUM and LFS_ENTROPY strategies (lodepng.cpp:5444-5570; the search zopflipng
 * runs per strategy trial, zopflipng_lib.cc:160-305), computed on the device from the raw (already colour-converted,
 * non-interlaced) image; `bytewidth` = bytes per pixel, 1 below 8 bits per pixel.  Either output may be null.  The
 * types go back to LodePNG as LFS_PREDEFINED (`predefined_filters`): the scanlines it then writes are the ones its own
 * search would have produced.  zmx_png_filter_types_pooled is the same on one of the contexts of the Zopfli* entry
 * points (what libzopflipng_amd.so calls). */
int zmx_png_filter_types(zmx_ctx* ctx, const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                         unsigned char* minsum_types, unsigned char* entropy_types);
int zmx_png_filter_types_pooled(const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                                unsigned char* minsum_types, unsigned char* entropy_types);

/* The filter type LodePNG's LFS_BRUTE_FORCE strategy picks for each scanline (lodepng.cpp:5585-5632): every row is
 * filtered the five ways, each version zlib-compressed alone by LodePNG's fixed-tree deflate (window `windowsize`,
 * minmatch 3, nicematch 128, lazy matching) and the first smallest in bytes wins.  zopflipng's `b` strategy deflates
 * with window 32768; LodePNG's default is 2048.  Geometry as zmx_png_filter_types; `types` gets `height` bytes.  A
 * window that is 0, not a power of two or above 32768 is refused (ZMX_ERR_REFUSED; LodePNG's errors 60 / 90);
 * height 0 returns 0.  zmx_png_filter_types_brute_pooled is the same on one of the entry points' contexts. */
int zmx_png_filter_types_brute(zmx_ctx* ctx, const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                               unsigned windowsize, unsigned char* types);
int zmx_png_filter_types_brute_pooled(const unsigned char* image, size_t linebytes, size_t height, size_t bytewidth,
                                      unsigned windowsize, unsigned char* types);

/* The same row searches on an image that already lies in DEVICE memory, the types left there: d_types[0, height), memory
 * of the context's device as the image is.  `strategy`: ZMX_PNG_FILTER_ZERO .. _FOUR fill the types with 0 .. 4, _MINSUM
 * and _ENTROPY run zmx_png_filter_types' kernel, _BRUTE runs zmx_png_filter_types_brute's with window `windowsize`
 * (read for _BRUTE only).  The numbers are LodePNG's LodePNGFilterStrategy where it has them (lodepng.h:680-698);
 * _PREDEFINED is for zmx_png_encode_device alone.  Both pointers are checked as zmx_png_filter_rows_device checks its
 * own; the types may not overlap the image.  height = 0 returns 0.  Synchronous. */
#define ZMX_PNG_FILTER_ZERO 0
#define ZMX_PNG_FILTER_ONE 1
#define ZMX_PNG_FILTER_TWO 2
#define ZMX_PNG_FILTER_THREE 3
#define ZMX_PNG_FILTER_FOUR 4
#define ZMX_PNG_FILTER_MINSUM 5
#define ZMX_PNG_FILTER_ENTROPY 6
#define ZMX_PNG_FILTER_BRUTE 7
#define ZMX_PNG_FILTER_PREDEFINED 8
int zmx_png_filter_types_device(zmx_ctx* ctx, const void* d_image, size_t linebytes, size_t height, size_t bytewidth,
                                int strategy, unsigned windowsize, void* d_types);

/* The filtered scanlines of an image in device memory (k_png_rows, device/zmx_png_rows.h: one launch of at most 2048
 * workgroups): d_out[r * (linebytes + 1)] = d_types[r], and the `linebytes` bytes behind it are row r of d_image filtered
 * that way (lodepng.cpp:5379-5421 filterScanline: None, Sub, Up, Average, Paeth; `bytewidth` the distance to the left
 * neighbour, zeros above row 0 and to the left of a row's first `bytewidth` bytes) — the bytes LodePNG's encoder hands to
 * its deflate.  Every byte of d_out[0, height * (linebytes + 1)) is written exactly once and none outside; d_out may have
 * any alignment.  Refused before any launch (ZMX_ERR_REFUSED): a null pointer, host or managed memory, a range that
 * leaves its allocation, memory of another device than the context's, an output that overlaps the image or the types, a
 * `capacity` below height * (linebytes + 1), linebytes 0 or above 2^31 - 1, a height above 2^31 - 1, a bytewidth that is
 * not 1 .. 8.  A type byte above 4 is found by the kernel: the call fails (ZMX_ERR_REFUSED), the message names the first
 * such row ("row N"), and what d_out then holds is not defined.  height = 0 returns 0.  Synchronous; the caller
 * synchronises the streams that produced the image and the types. */
int zmx_png_filter_rows_device(zmx_ctx* ctx, const void* d_image, size_t linebytes, size_t height, size_t bytewidth,
                               const void* d_types, void* d_out, size_t capacity);

/* An image in device memory (a rendered frame, a tensor) as a zopfli-optimised PNG file.  *out, *outsize follow the
 * reference's append convention, as zmx_compress_device's do, and end holding the file that
 *   zopflipng --keepcolortype --always_zopflify --filters=<strategy>
 * writes for a PNG of the same pixels, colour type and bit depth that has no other chunks: the signature, IHDR, ONE
 * IDAT and IEND, the IDAT's payload being 78 01, ZopfliDeflate(btype 2, final 1) of LodePNG's filtered scanlines and
 * their Adler-32.  The match is byte for byte when options->numiterations is what zopflipng would take: its rule —
 * num_iterations (15) for less than 200 000 bytes of scanlines, else num_iterations_large (5), zopflipng_lib.cc:56-58 —
 * is the caller's business, as is every other field of `options`.
 * `strategy`: a ZMX_PNG_FILTER_* (zopflipng's --filters= 0 1 2 3 4 m e b); _BRUTE searches with window 32768, as
 * zopflipng's final encode does (zopflipng_lib.cc:360); _PREDEFINED takes `predefined`, `height` host bytes of at most 4
 * each (otherwise `predefined` is not read).
 * No pixel visits the host (zmx_last_input_traffic()[0] is 0): the row search and k_png_rows run on a context of the
 * image's device into a buffer of the call's own, and zmx_compress_device(ZOPFLI_FORMAT_ZLIB) of that buffer makes the
 * stream; only the stream comes down, and the container is put around it on the host.
 * Refused before anything runs (ZMX_ERR_REFUSED), *out and *outsize unchanged: a null argument, width or height 0, a
 * colour type other than 0, 2, 4, 6, a bit depth other than 8 or 16, an unknown strategy, _PREDEFINED without types or
 * with a type above 4, and what zmx_png_filter_rows_device refuses of the pixels' pointer.  Any later failure leaves them
 * unchanged as well.
 * `strategy` may also be ZMX_PNG_FILTER_AUTO (further down): zopflipng's own choice, made by
 * zmx_png_choose_strategy_device(reduce_color = 0) on the same hold of the context, after the lossy rewrite where one is
 * asked for; the file is then the one zopflipng --keepcolortype --always_zopflify writes with NO --filters for an input
 * whose rows carry filter type 0 — or, where `predefined` is given, the types at `predefined` (the eighth trial; if it
 * wins, the file is _PREDEFINED's).
 * Palette input: done (zmx_png_index_encode_device, further down).  Out of scope: interlace, ancillary chunks
 * (libzopflipng_amd.so does those, from a file — its own strategy
 * trials still run LodePNG on host threads).  Colour-type reduction is zmx_png_optimize_device's; the file left in device
 * memory is zmx_png_encode_device_to_device's, further down. */
typedef struct zmx_png_image {
  const void* d_pixels;  /* height rows of linebytes bytes, PNG byte order (16-bit samples big-endian), rows back to back */
  uint32_t width, height, colortype /* 0, 2, 4, 6 */, bitdepth /* 8, 16 */;
} zmx_png_image;
int zmx_png_encode_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                          const unsigned char* predefined, unsigned char** out, size_t* outsize);
/* n images in one call: every out[i], outsize[i] ends as zmx_png_encode_device(options, &images[i], strategy, ...)
 * leaves it, byte for byte, whatever the other images and their order.  The types and rows are made image by image (two
 * or three launches each) into ONE buffer, and ONE zmx_compress_device_batch(ZOPFLI_FORMAT_ZLIB) over its slices makes
 * the streams, so icons and tiles share the table builds and squeeze runs of one large call.  The images lie on one
 * device.  _PREDEFINED is refused; otherwise the refusals are the single call's, for any image, and no out[i] is changed
 * by a call that fails.  n = 0 returns 0.  ZMX_PNG_FILTER_AUTO chooses image by image (seven trials each: a batch passes
 * no predefined types) before the one zmx_compress_device_batch. */
int zmx_png_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                unsigned char** out, size_t* outsize);

/* -------- zopflipng's automatic filter-strategy choice (its default: no --filters)
 *
 * The length lodepng_zlib_compress returns for each of n buffers in device memory under LodePNG's default settings
 * (btype 2, use_lz77 1, minmatch 3, nicematch 128, lazymatching 1) with window `windowsize`: zlib_bytes[i] is
 * 2 + ceil(deflate bits / 8) + 4 for d_in[i][0, insize[i]).  Only the size is made, never the stream.  The kernels of
 * device/zmx_png_lodeflate.h parse all buffers of the call side by side — LodePNG's deflate blocks of insize / 8 + 8 bytes
 * within [65536, 262144], its hash chains with their stale slots, its lazy matching — and bring every block down to its
 * 286 + 30 symbol counts and extra bits; host/png_lodeflate_size.h makes LodePNG's dynamic trees of those and adds up the
 * bits.  A few KB per deflate block come down, no byte of the buffers does.  The scratch is 12 bytes per input byte and
 * 257 KiB per 262144 bytes (and per buffer).
 * Refused before any launch (ZMX_ERR_REFUSED), zlib_bytes untouched: a null argument, n = 0, a buffer of 0 bytes, a window
 * LodePNG refuses (0, not a power of two, above 32768), more than 2^40 bytes in all, and what zmx_png_filter_rows_device
 * refuses of a pointer.  Any later failure leaves zlib_bytes untouched as well.  Synchronous; the caller synchronises the
 * streams that produced the buffers. */
int zmx_png_deflate_sizes_device(zmx_ctx* ctx, size_t n, const void* const* d_in, const size_t* insize, unsigned windowsize,
                                 uint64_t* zlib_bytes);

/* zopflipng's AutoChooseFilterStrategy (zopflipng_lib.cc:270-305) for an image in device memory: the PNG file LodePNG's
 * own encoder would write (its deflate at window 8192) is sized under the strategies 0, 1, 2, 3, 4, MINSUM, ENTROPY and
 * PREDEFINED in that order — never BRUTE — and *strategy is the ZMX_PNG_FILTER_* of the first strictly smallest file;
 * file_bytes[k] is trial k's file size.  The rows of all trials go into one buffer of the call's own
 * (zmx_png_filter_types_device's and zmx_png_filter_rows_device's kernels) and ONE zmx_png_deflate_sizes_device sizes
 * them; the container's bytes for the mode are added on the host.
 *   reduce_color = 0  the image's own colour type and depth (zopflipng --keepcolortype)
 *   reduce_color = 1  zmx_png_choose_color's mode of the image's statistics; as in zopflipng's TryOptimize, a palette
 *                     trial whose file is below 4096 bytes is sized as RGB / RGBA at 8 bits as well and counts with the
 *                     smaller of its two sizes
 *   predefined        `height` host bytes of at most 4 each: the eighth trial.  Null: that trial is skipped and
 *                     file_bytes[7] = 0 — zopflipng's answer for an input PNG whose rows all carry filter type 0, whose
 *                     predefined trial repeats trial 0 and cannot win.
 * Refusals are zmx_png_optimize_device's of the image (with reduce_color = 0: zmx_png_encode_device's), a null context,
 * strategy or file_bytes, a predefined type above 4; *strategy and file_bytes are written by a call that succeeds only.
 * Synchronous; no pixel visits the host. */
#define ZMX_PNG_FILTER_AUTO 10 /* (9 is no strategy and stays refused) */
int zmx_png_choose_strategy_device(zmx_ctx* ctx, const zmx_png_image* image, int reduce_color,
                                   const unsigned char* predefined /* may be null */, int* strategy, uint64_t file_bytes[8]);

/* -------- colour-type reduction: what zopflipng does to an image without --keepcolortype
 *
 * LodePNG's colour statistics (lodepng.cpp lodepng_compute_color_stats) of an image in device memory, every rule stated
 * on the pixel's RGBA expansion as zopflipng sees it (grey gives r = g = b, no alpha channel gives the maximum):
 *   colored    some pixel has r != g or r != b
 *   alpha      some alpha is neither 0 nor the maximum, or the transparent pixels have more than one RGB, or an opaque
 *              pixel has theirs
 *   key        otherwise, when some alpha is 0: the transparent pixels' one RGB in key_r, key_g, key_b as 16-bit values
 *              (an 8-bit value with its byte twice); zeros without a key
 *   bits       1, 2, 4 or 8: what the grey values need (8 when colored or alpha); 16 for a 16-bit image some sample of
 *              which has two different bytes — the statistics are then taken on 16-bit values and no colours are counted
 *              (numcolors 0); a 16-bit image whose bytes are all equal counts as the 8-bit image of its high bytes
 *   numcolors  the distinct RGBA values, 257 for "more than 256"; palette holds them r, g, b, a in the order of their
 *              first appearance in raster order (zeros behind them, and all zeros for 257)
 * k_png_color_stats (device/zmx_png_color.h) reads the image once with at most 2048 workgroups; k_png_color_key reads
 * it again only when a key is possible.  A few kilobytes come down, no pixel does; the result is the same from run to
 * run.  The image is refused (ZMX_ERR_REFUSED) as zmx_png_encode_device refuses its own, its pointer as
 * zmx_png_filter_rows_device refuses one, and an image of 2^32 pixels or more.  Synchronous. */
typedef struct zmx_png_color_stats {
  uint32_t colored, key, alpha, numcolors, bits;
  uint16_t key_r, key_g, key_b, reserved;
  unsigned char palette[1024];
} zmx_png_color_stats;
int zmx_png_color_stats_device(zmx_ctx* ctx, const zmx_png_image* image, zmx_png_color_stats* out);

/* The colour mode LodePNG's auto_choose_color takes for these statistics of an image of `numpixels` pixels: host
 * arithmetic only.  colortype 0, 2, 3, 4 or 6; bitdepth 1, 2, 4, 8 or 16; for colour type 3 the palette (palettesize
 * entries r, g, b, a); for 0 and 2 the key where key_defined, masked to the depth.  A key on at most 16 pixels becomes
 * alpha, a palette is not taken for fewer than two pixels a colour or where grey is no deeper.  -1 (ZMX_ERR_REFUSED) for a
 * null argument. */
typedef struct zmx_png_color_mode {
  uint32_t colortype, bitdepth, palettesize, key_defined;
  uint16_t key_r, key_g, key_b, reserved;
  unsigned char palette[1024];
} zmx_png_color_mode;
int zmx_png_choose_color(const zmx_png_color_stats* stats, uint64_t numpixels, zmx_png_color_mode* out);

/* The image in another colour mode (lodepng.cpp lodepng_convert), device memory to device memory: d_out gets `height`
 * rows of (width * bpp + 7) / 8 bytes back to back, bpp = channels * bitdepth (one channel for a palette).  Grey below 8
 * bits keeps the top bits of r, a palette pixel becomes its colour's rank (of two equal entries the later one), pixels
 * below 8 bits are packed most significant bits first and every row is padded with zero bits; 8-bit output of a 16-bit
 * image keeps the high bytes; channels the mode has not are dropped without a look at them (the key is the container's
 * business).  k_png_convert writes every byte of the output exactly once and none outside; d_out may have any alignment.
 * Refused before any launch (ZMX_ERR_REFUSED): what zmx_png_color_stats_device refuses of the image, a mode PNG has not, a
 * palette of 0 or more than 2^bitdepth entries, 16-bit output of an 8-bit image, a `capacity` below the output's size, an
 * output that is no device memory of the context's device or overlaps the image.  A pixel whose colour the palette lacks
 * is found by the kernel: the call fails (ZMX_ERR_REFUSED), the message names the first such pixel ("pixel N"), and what
 * d_out then holds is not defined.  Synchronous. */
int zmx_png_convert_device(zmx_ctx* ctx, const zmx_png_image* image, const zmx_png_color_mode* mode, void* d_out, size_t capacity);

/* zmx_png_encode_device with the colour mode reduced first: *out, *outsize end holding the file that
 *   zopflipng --always_zopflify --filters=<strategy>
 * (no --keepcolortype) writes for a PNG of these pixels that has no other chunks — the signature, IHDR, PLTE for a
 * palette, tRNS for a palette with alpha or a key, ONE IDAT, IEND — byte for byte under the same conditions.  The mode is
 * zmx_png_choose_color's of the image's statistics; where that is a palette and the file comes out below 4096 bytes, a
 * second file is made as RGB or RGBA at 8 bits (zopflipng_lib.cc TryOptimize) and replaces the first when it is strictly
 * smaller.  The strategy applies to palette and sub-8-bit rows as to any other, with a left neighbour one byte away.
 * Where the chosen mode is the image's own nothing is converted and the file is zmx_png_encode_device's.  No pixel visits
 * the host.  Conventions, refusals and failure behaviour are zmx_png_encode_device's; an image of 2^32 pixels or more
 * is refused as well.
 * ZMX_PNG_FILTER_AUTO: zmx_png_choose_strategy_device(reduce_color = 1) chooses on the same hold of the context, with the
 * statistics the entry has taken; both tries of a small palette file are made with the chosen strategy, as zopflipng's
 * are.  The file is the one zopflipng --always_zopflify writes with no --filters.
 * Palette input: done (zmx_png_index_optimize_device, further down).  Out of scope: interlace, ancillary chunks
 * (libzopflipng_amd.so does those, from a file).
 * --lossy_transparent and --lossy_8bit are the _lossy entries' further down, the file left in device memory is
 * zmx_png_optimize_device_to_device's. */
int zmx_png_optimize_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                            const unsigned char* predefined, unsigned char** out, size_t* outsize);
/* n images in one call: every file is the single call's.  Statistics and conversion run image by image on one hold of a
 * context, ONE zmx_compress_device_batch(ZOPFLI_FORMAT_ZLIB) runs over all scanlines and one more over the second tries,
 * if any image takes one.  Otherwise as zmx_png_encode_device_batch. */
int zmx_png_optimize_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                  unsigned char** out, size_t* outsize);

/* -------- zopflipng's --lossy_transparent and --lossy_8bit on an image in device memory
 *
 * zopflipng's rewrite of the pixels nobody sees (zopflipng_lib.cc LossyOptimizeTransparent), device memory to device
 * memory.  Every pixel is read as 8-bit r, g, b, a (grey + alpha gives r = g = b), the N = width * height pixels in
 * raster order, rows back to back:
 *   key      no pixel has 0 < a < 255
 *   palette  at most 256 colours, every pixel with a = 0 counting as one colour
 *   mode 1   (key or palette) every pixel with a = 0 gets the RGB of the FIRST pixel with a = 0
 *   mode 2   (otherwise) a pixel with a = 0 gets the RGB of the last pixel before it — in the whole image, not its row —
 *            that had a > 0, and (0, 0, 0) where there was none
 *   mode 0   no pixel has a = 0, or the colour type is 0 or 2 (no statistics are taken for those: partial_alpha and
 *            numcolors are 0): d_out gets a copy of the image
 * Alpha and the pixels with a > 0 never change.  d_out gets `height` rows of `linebytes` in the image's own format, in
 * every mode; d_out == image->d_pixels rewrites in place.  For a 16-bit image the call takes the caller at their word:
 * the pixels are read through their HIGH bytes, and the high bytes of r, g, b of a pixel whose alpha's high byte is 0 are
 * rewritten, the low bytes left — something zopflipng never does (it leaves a 16-bit image alone) and the entries below
 * never ask for.
 * k_png_lossy_stats, k_png_lossy_carry (mode 2 only) and k_png_lossy_fill (device/zmx_png_lossy.h) run one after the
 * other on the context's stream, at most 2048 workgroups each, none waiting for another; a few words come down, no pixel
 * does.  Refused before any launch (ZMX_ERR_REFUSED): what zmx_png_color_stats_device refuses of the image, a `capacity`
 * below the image's size, an output that is no device memory of the context's device, an output that overlaps the image
 * without being the image.  Synchronous; the caller synchronises the stream that produced the image. */
#define ZMX_PNG_LOSSY_TRANSPARENT 1u
#define ZMX_PNG_LOSSY_8BIT 2u
typedef struct zmx_png_lossy_info {
  uint32_t mode;            /* 0 no transparent pixel (d_out = the image), 1 fixed, 2 carry */
  uint32_t partial_alpha;   /* some 0 < a < 255 */
  uint32_t numcolors;       /* transparent pixels as one colour; 257 = more than 256 */
  uint32_t fill_r, fill_g, fill_b;   /* mode 1: the colour; else 0 */
  uint64_t first_transparent;        /* pixel index, UINT64_MAX without one */
} zmx_png_lossy_info;
int zmx_png_lossy_transparent_device(zmx_ctx* ctx, const zmx_png_image* image, void* d_out, size_t capacity,
                                     zmx_png_lossy_info* info /* may be null */);

/* zmx_png_encode_device and zmx_png_optimize_device with zopflipng's lossy options: `lossy` is 0 or an OR of
 * ZMX_PNG_LOSSY_*, anything else is refused.  The encode entry ends holding the file
 *   zopflipng --keepcolortype --always_zopflify --filters=<strategy> [--lossy_transparent] [--lossy_8bit]
 * writes, the optimize entry the same without --keepcolortype, byte for byte under the conditions of the entries above.
 * The flags mean what they mean to zopflipng (zopflipng_lib.cc:415-428), the combinations that do nothing included:
 *   _8BIT         a 16-bit image is encoded as the 8-bit image of its high bytes (same colour type, made by
 *                 k_png_convert) — for the optimize entry; the encode entry accepts and ignores it
 *   _TRANSPARENT  zmx_png_lossy_transparent_device's rewrite of an image that is 8-bit by then; nothing happens to a
 *                 16-bit image unless the optimize entry has _8BIT as well
 * lossy = 0 gives zmx_png_encode_device's / zmx_png_optimize_device's file.  The caller's image is never written: the
 * rewritten and the 8-bit image go to a buffer of the call's own, on the hold of the context that makes the statistics
 * and the rows, and everything after is the entries' path on that buffer — the choice of the mode, the second try below
 * 4096 bytes, the row search, one zmx_compress_device[_batch](ZLIB).  No pixel visits the host.  The batches rewrite image
 * by image with the batch's flags.  Conventions, refusals, failure behaviour and _PREDEFINED are the entries' above; the
 * encode entries refuse as well, before anything runs, an image of 2^32 pixels or more that _TRANSPARENT would rewrite
 * (grey + alpha or RGBA at 8 bits), as the optimize entries refuse any such image. */
int zmx_png_encode_device_lossy(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_optimize_device_lossy(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                  const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_encode_device_batch_lossy(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                      unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_optimize_device_batch_lossy(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                        unsigned lossy, unsigned char** out, size_t* outsize);

/* -------- the PNG entries with the file LEFT IN DEVICE MEMORY
 *
 * d_out[0, *outsize) ends holding, byte for byte, the file that zmx_png_encode_device_lossy / zmx_png_optimize_device_lossy
 * appends to an empty output for the same options, image, strategy, predefined types and `lossy` (an argument here: these
 * entries have no _lossy twins) — every strategy, _AUTO and _PREDEFINED included, both lossy flags and their no-op
 * combinations.  No byte of the file, the stream or the pixels visits the host (zmx_last_input_traffic()[0] and
 * zmx_last_output_traffic()[0] are 0; [1] of the latter: the uploaded literals, as for zmx_compress_device_to_device).
 * d_out may have any byte alignment; every byte of the file is written and no byte outside it.
 * Everything in front of the compression is the host-output entries' first hold of the context.  The stream then goes
 * zmx_compress_device_to_device's way with a FRAME around it: in front of the stream's first bit the file's prefix with the
 * IDAT's length filled in and LodePNG's 78 01, behind the Adler-32 four placeholder bytes and IEND — all literals of the one
 * bit join.  After the join, while the call still holds its contexts, zmx_checksum_device's two kernels run over the
 * IDAT's type and payload where they lie and seal the CRC-32 into the placeholder.
 * The plan gives the file's size before anything is written: a `capacity` that is too small, or a stream that does not fit
 * the 31 bits of a chunk's length, returns -1 (ZMX_ERR_REFUSED) with *outsize = the size needed and d_out untouched.
 * zmx_png_bound(width, height, colortype, bitdepth) — the INPUT's mode — is always enough for both single entries
 * (host/device_output_plan.h derives it); 0 for a mode the entries refuse.
 * zmx_png_optimize_device_to_device, palette files: which of the two tries is kept is known only once the first is made, so
 * a palette file is made into a buffer of the call's own, the second try of one below 4096 bytes into another, and one
 * device-to-device copy puts the kept file into d_out; `capacity` is held against the kept file's size.
 * zmx_png_encode_device_batch_packed: zmx_png_encode_device_batch's front half, then zmx_compress_device_batch_packed's plan
 * with a frame per stream — ONE k_bitjoin_many launch writes all files, ONE k_checksum_pieces and ONE k_checksum_finish
 * launch seal all n.  File i lies at d_arena + outoffset[i], outoffset[i] = the end of file i - 1 rounded up to `align`
 * (a power of two, 1 .. 4096); the bytes between files are not written.  An arena that is too small: outoffset[] and
 * outsize[] report what is needed and nothing is written.  zmx_png_batch_bound = every image's bound rounded up to
 * `align`, summed.  _PREDEFINED is refused, as in the host-output batch; n = 0 returns 0.
 * Limits, inherited from the to-device compress entries: one round (ZOPFLI_AMD_ROUND_PARTS master blocks of scanlines for
 * the single entries, 2 000 000 000 bytes for the batch); the image(s) and the destination on ONE device of the library's;
 * the destination overlapping neither an image nor anything made from it.  Refused as well, before anything runs: what
 * the host-output entries refuse, a destination that is not plain device memory or leaves its allocation.
 * Out of scope: a to-device batch form of OPTIMIZE — its second tries need a second packed pass and a gather of the kept
 * files. */
size_t zmx_png_bound(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth);
int zmx_png_encode_device_to_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                    const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize);
int zmx_png_optimize_device_to_device(const ZopfliOptions* options, const zmx_png_image* image, int strategy,
                                      const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize);
size_t zmx_png_batch_bound(size_t n, const zmx_png_image* images, size_t align);
int zmx_png_encode_device_batch_packed(const ZopfliOptions* options, size_t n, const zmx_png_image* images, int strategy,
                                       unsigned lossy, void* d_arena, size_t capacity, size_t align, size_t* outoffset,
                                       size_t* outsize);

/* -------- strided, planar, float and 16-bit sources
 *
 * What a GPU program holds instead of a zmx_png_image: a (C, H, W) or (N, C, H, W) tensor, float samples in [0, 1],
 * native (little-endian) 16-bit ones, a frame with a row pitch, BGRA, bottom-up, a crop or a [::2] view.  A zmx_png_source
 * says where sample (y, x, c) lies; its PACKED image is the zmx_png_image of colour type 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4
 * channels at `bitdepth`, rows back to back, PNG channel k of a pixel being source channel order[k].
 * The value rule is exact:
 *   U8 -> 8 the byte; U16 -> 16 the value, high byte first; U8 -> 16 and U16 -> 8 are refused (ZMX_PNG_LOSSY_8BIT of the
 *   optimize entries is the way to 8 bits); F16 and BF16 are widened to fp32 exactly and follow the F32 rule;
 *   F32 -> 8 or 16, maxv = 255.0f or 65535.0f: q = (uint32) clamp(fl32(fl32(x * maxv) + 0.5f), 0, maxv) — the multiply
 *   and the add each rounded to fp32, the conversion truncating, a NaN giving 0: torchvision's
 *   mul(maxv).add_(0.5).clamp_(0, maxv).to(int), what numpy.float32 arithmetic gives.
 * zmx_png_source_image: host arithmetic — the packed image's mode in *image (d_pixels null) and its size in *nbytes
 * (either may be null); -1 (ZMX_ERR_REFUSED) for a source the entries refuse without asking the runtime about its memory.
 * zmx_png_pack_device: the packed images of n sources at d_out[i] (capacity[i] bytes, any byte alignment), by ONE launch
 * of k_png_pack (device/zmx_png_pack.h) on the context's stream, whatever n: every byte of every packed image is written
 * exactly once, none outside, no source is written.  Synchronous; n = 0 returns 0.
 * Refused before any launch (ZMX_ERR_REFUSED), the message naming the source's index: a null argument, width or height 0,
 * channels outside 1 .. 4, an unknown sample type, a bit depth other than 8 or 16, the two refused conversions, an `order`
 * that is no permutation of 0 .. channels - 1, d_data or a stride that is no multiple of the sample's size, a row of 2^31
 * bytes or more, an EXTENT — from the lowest to one past the highest byte any sample touches, by the signs of the three
 * strides — that overflows 64 bits, is not plain device memory of the context's device or leaves its allocation, a
 * capacity below the packed size, a destination that is no device memory of that device or overlaps a source's extent or
 * another destination.
 * The zmx_png_*_source_* entries: the file, or files, that the entry of the same name without _source gives for the packed
 * images, byte for byte — every strategy, _AUTO, _PREDEFINED where that entry takes it, both lossy flags; its conventions,
 * refusals and failure behaviour unchanged, and the refusals above made before anything runs.  All packed images go into
 * one buffer of the call's own by one k_png_pack launch on the first hold of a context; no pixel visits the host
 * (zmx_last_input_traffic()[0] stays 0).  The to-device destinations may not overlap a source's extent either.  The bounds
 * are those of zmx_png_source_image's mode (0 for a refused source). */
#define ZMX_PNG_SAMPLE_U8 0
#define ZMX_PNG_SAMPLE_U16 1 /* native, i.e. little-endian */
#define ZMX_PNG_SAMPLE_F16 2
#define ZMX_PNG_SAMPLE_BF16 3
#define ZMX_PNG_SAMPLE_F32 4
typedef struct zmx_png_source {
  const void* d_data;                   /* sample (y, x, c) lies at d_data + y*stride_y + x*stride_x + c*stride_c (bytes) */
  int64_t stride_y, stride_x, stride_c; /* bytes; multiples of the sample's size; any sign; 0 allowed (a broadcast) */
  uint32_t width, height, channels /* 1 .. 4 */, sample /* ZMX_PNG_SAMPLE_* */;
  uint32_t bitdepth;                    /* of the PNG: 8 or 16 */
  uint8_t order[4];                     /* PNG channel k of a pixel is source channel order[k]; a permutation of 0 .. channels-1 */
} zmx_png_source;
int zmx_png_source_image(const zmx_png_source* src, zmx_png_image* image /* d_pixels left null */, size_t* nbytes);
int zmx_png_pack_device(zmx_ctx* ctx, size_t n, const zmx_png_source* sources, void* const* d_out, const size_t* capacity);
int zmx_png_encode_source_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                 const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_optimize_source_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                   const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_encode_source_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                       unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_optimize_source_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                         unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_encode_source_device_to_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                           const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                           size_t* outsize);
int zmx_png_optimize_source_device_to_device(const ZopfliOptions* options, const zmx_png_source* source, int strategy,
                                             const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity,
                                             size_t* outsize);
int zmx_png_encode_source_device_batch_packed(const ZopfliOptions* options, size_t n, const zmx_png_source* sources, int strategy,
                                              unsigned lossy, void* d_arena, size_t capacity, size_t align, size_t* outoffset,
                                              size_t* outsize);
size_t zmx_png_source_bound(const zmx_png_source* source);
size_t zmx_png_source_batch_bound(size_t n, const zmx_png_source* sources, size_t align);

/* -------- palette, 1/2/4-bit grey and index images in device memory
 *
 * A label map (one byte a pixel plus a colour map), a binary mask (one bit a pixel), a 2- or 4-bit atlas: `height` rows of
 * (width * bitdepth + 7) / 8 bytes back to back, the first pixel in a byte's top bits, the bits behind a row's last pixel
 * anything.  Colour type 3 with a palette of 1 .. 2^bitdepth host entries r, g, b, a at 1, 2, 4 or 8 bits, or colour type
 * 0 at 1, 2 or 4 bits, which goes through the same code with the grey ramp v * 255 / (2^bitdepth - 1) as its palette.
 * zopflipng decodes such a PNG to RGBA8 — value i becomes palette[i] — and everything it and LodePNG then do follows from
 * the palette and ONE fact about the pixels: at which pixel each of the 256 values first appears.  So the device work is
 * one read of the image and one table-driven rewrite; nothing is expanded to RGBA, and --lossy_transparent is a change of
 * the host's table.
 *   zmx_png_index_use_device      first[v] = the smallest raster pixel index (row * width + column) at which value v
 *                                 occurs, 2^64 - 1 for a value no pixel has.  k_png_index_use (device/zmx_png_index.h)
 *                                 reads the image once with at most 2048 workgroups; padding bits are no pixels; a
 *                                 minimum of positions, equal from run to run.  Values at or above palettesize are
 *                                 reported like any other.
 *   zmx_png_index_color_stats     host arithmetic (host/png_index.h): the statistics zmx_png_color_stats_device gives for
 *                                 the RGBA8 expansion of the image — after zopflipng's rewrite of the transparent pixels
 *                                 where `lossy` has ZMX_PNG_LOSSY_TRANSPARENT (every used entry with alpha 0 gets the RGB of
 *                                 the first transparent pixel; _8BIT does nothing here).  A colour's first appearance is the
 *                                 minimum over the values that carry it.  Refused: a value at or above palettesize
 *                                 that occurs (the message names its first pixel, "pixel N").
 *   zmx_png_index_table           host arithmetic: the 256 entries that take the image into `mode` (after the same rewrite):
 *                                 the rank in the mode's palette (of two equal entries the later, as LodePNG's colour tree
 *                                 keeps it), the grey value's top bits, or the bytes grey alpha / r g b / r g b a, the first
 *                                 in the entry's low byte.
 *   zmx_png_index_keep_plan       host arithmetic: the mode of zopflipng --keepcolortype's file — the input's own, with the
 *                                 whole palette in the input's order, unused entries included; after _TRANSPARENT the
 *                                 palette shrunk to the entries whose own colour still occurs, as zopflipng_lib.cc:137-155
 *                                 shrinks it — and the table into it.
 *   zmx_png_index_convert_device  the image through `table` into `mode`: a palette or grey at 1, 2, 4, 8 bits, grey + alpha,
 *                                 RGB or RGBA at 8.  d_out gets `height` rows of (width * bpp + 7) / 8 bytes, packed most
 *                                 significant bits first, rows padded with ZERO bits; k_png_index_convert writes every
 *                                 byte of the output exactly once and none outside, source and destination at any
 *                                 alignment.  A pixel whose value is at or above palettesize is found by the kernel: the
 *                                 call fails (ZMX_ERR_REFUSED), the message names the first such pixel ("pixel N"), and what
 *                                 d_out then holds is not defined.
 * The two device steps are synchronous and check their pointers as zmx_png_filter_rows_device checks its own.  Refused
 * before any launch (ZMX_ERR_REFUSED), by every entry of this section: width or height 0, another colour type or depth,
 * palettesize 0 or above 2^bitdepth, an image of 2^32 pixels or more; by the convert step a mode outside the list above and
 * a `capacity` below the output's size.
 *
 * zmx_png_index_encode_device: *out, *outsize (zmx_png_encode_device's conventions) end holding the file
 *   zopflipng --keepcolortype --always_zopflify --filters=<strategy> [--lossy_transparent]
 * writes for a PNG of this image that has no other chunks; zmx_png_index_optimize_device the file of the same command
 * WITHOUT --keepcolortype — byte for byte zmx_png_optimize_device_lossy's file of the RGBA8 expansion, second try below
 * 4096 bytes included, for every strategy and both lossy flags.  One k_png_index_use, the host step, one
 * k_png_index_convert (two with a second try; one more for each mode ZMX_PNG_FILTER_AUTO's trials need), then the row
 * search, the filtered scanlines and the compression of the existing entries.  No pixel and no index visits the host
 * (zmx_last_input_traffic()[0] is 0); the caller's image is never written.  `strategy`, `predefined`, `lossy`, refusals and
 * failure behaviour are zmx_png_encode_device_lossy's / zmx_png_optimize_device_lossy's, with the image refused as above and
 * a value at or above palettesize refused once the first kernel has found it (*out, *outsize untouched).
 * zmx_png_index_choose_strategy_device is zmx_png_choose_strategy_device for such an image, `lossy` applied first.
 * The _to_device forms leave the file in device memory as zmx_png_encode_device_to_device does — the same frame, one bit
 * join, the CRC-32 sealed on the device, no byte of the file on the host —; zmx_png_index_bound(width, height, colortype,
 * bitdepth) is always enough for both (sized for RGBA at 8 bits, which the second try can be; 0 for an image the entries
 * refuse).  The batches give every out[i], outsize[i] the single entry's file, image by image one k_png_index_use, the host
 * step and one k_png_index_convert, then ONE zmx_compress_device_batch(ZLIB) over all scanlines and one more for the second
 * tries; _PREDEFINED is the single call's; n = 0 returns 0.
 * Out of scope: a packed to-device batch of these, interlace, ancillary chunks, a tRNS key on grey input. */
typedef struct zmx_png_index_image {
  const void* d_pixels;        /* height rows of (width * bitdepth + 7) / 8 bytes, first pixel in a byte's top bits, rows back to back */
  uint32_t width, height;
  uint32_t colortype;          /* 3 (palette) or 0 (grey) */
  uint32_t bitdepth;           /* 3: 1, 2, 4, 8    0: 1, 2, 4 */
  uint32_t palettesize;        /* 3: 1 .. 2^bitdepth    0: not read */
  unsigned char palette[1024]; /* host memory: r, g, b, a per entry */
} zmx_png_index_image;
int zmx_png_index_use_device(zmx_ctx* ctx, const zmx_png_index_image* image, uint64_t first[256]);
int zmx_png_index_color_stats(const zmx_png_index_image* image, const uint64_t first[256], unsigned lossy, zmx_png_color_stats* out);
int zmx_png_index_table(const zmx_png_index_image* image, const uint64_t first[256], unsigned lossy, const zmx_png_color_mode* mode,
                        uint32_t table[256]);
int zmx_png_index_keep_plan(const zmx_png_index_image* image, const uint64_t first[256], unsigned lossy, zmx_png_color_mode* mode,
                            uint32_t table[256]);
int zmx_png_index_convert_device(zmx_ctx* ctx, const zmx_png_index_image* image, const zmx_png_color_mode* mode, const uint32_t table[256],
                                 void* d_out, size_t capacity);
int zmx_png_index_choose_strategy_device(zmx_ctx* ctx, const zmx_png_index_image* image, int reduce_color, unsigned lossy,
                                         const unsigned char* predefined, int* strategy, uint64_t file_bytes[8]);
int zmx_png_index_encode_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_index_optimize_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                  const unsigned char* predefined, unsigned lossy, unsigned char** out, size_t* outsize);
size_t zmx_png_index_bound(uint32_t width, uint32_t height, uint32_t colortype, uint32_t bitdepth);
int zmx_png_index_encode_device_to_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                          const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize);
int zmx_png_index_optimize_device_to_device(const ZopfliOptions* options, const zmx_png_index_image* image, int strategy,
                                            const unsigned char* predefined, unsigned lossy, void* d_out, size_t capacity, size_t* outsize);
int zmx_png_index_encode_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy,
                                      unsigned lossy, unsigned char** out, size_t* outsize);
int zmx_png_index_optimize_device_batch(const ZopfliOptions* options, size_t n, const zmx_png_index_image* images, int strategy,
                                        unsigned lossy, unsigned char** out, size_t* outsize);

/* Parity probe over whole tables: two 64-bit sums over all positions of a hash of the logical content of the match
 * records (block, position, length, distance, same, literal, every change point of sublen).  Equal digests of two
 * table sets over the same blocks = the same ZopfliFindLongestMatch results at every position. */
int zmx_match_digest(zmx_ctx* ctx, zmx_tables* tables, uint64_t* out2);

/* Parity probe: the static hash arrays of one block for positions max(0, instart - 32768) .. inend - 1
 * (from the start of the block's segment instead, when that is later: zmx_set_input_segments)
 * (inend - windowstart entries each): same[] (hash.c:116-126) and the distances to the previous
 * position of the same hash / of the same second hash (hash.c:110-114, 129-135; 0 = none).
 * Fails for tables built with zmx_tables_build_from and a parent: those hold the hash arrays only
 * where the recomputed positions at the block ends read them. */
int zmx_hash_links_download(zmx_ctx* ctx, zmx_tables* tables, size_t block, uint16_t* same,
                            uint16_t* prev1, uint16_t* prev2);

/* Parity probe: length_array[0..blocksize] of the last zmx_squeeze_run. */
int zmx_length_array_download(zmx_ctx* ctx, zmx_tables* tables, size_t block, uint16_t* out);

/* Parity probe: what the table build lays out once for every squeeze run of one block of B positions (tables with DP
 * rows, untrimmed).  *block_edges is always set: the slots the block's rows take in codes[].  Every array may be null
 * (not copied), so a first call with all of them null asks for the size of `codes`:
 *   dph      2 B words: per position the row's offset in the block's codes, then kend | shortcut << 16 | run row << 17 |
 *            literal byte << 18 | codeless << 26 (kend = min(length, B - j), 1 below 3: squeeze.c:286; shortcut:
 *            squeeze.c:251-258; run row = length >= 3, best distance 1, one change point; codeless = a run row of 64
 *            or more edges, which takes no slots, unless ZOPFLI_AMD_RUN_CODES=1)
 *   codes    *block_edges weight codes, times 8: slot 0 of a row (1 + byte), slot 1 zero, slot k - 1 for k = 3..kend
 *            257 + 30 (length symbol of k - 257) + distance symbol of sublen[k]
 *   winflag, winroff   W = (B + 31) / 32 + 1 words each: the kind and the first row's offset of every 32-position window
 *            (aligned to the block start), then one closing record: kind 0, where the block's rows end
 *   wmeta    40 W words: per window, words 0..31 = (row offset - the window's first + 32 - (u + 1)) << 16 | kend of
 *            position u (0 for the padding of a last partial window), 32 / 33 = where the window's rows start / end,
 *            34 = the kind; 35..39 are not defined.  Kind: 1 = 32 positions inside the block, none shortcut-flagged,
 *            kend + u < 64 for all; else 0 = a position outside the block, a shortcut flag or a run row of 64 or more
 *            edges; else 2 = kend + u < 128 for all; else 3.  | 0x100: a row of the window is codeless.
 * Nothing is defined for an empty block beyond *block_edges = 0. */
int zmx_dp_rows_download(zmx_ctx* ctx, zmx_tables* tables, size_t block, uint64_t* block_edges, uint32_t* dph,
                         uint16_t* codes, uint32_t* winflag, uint32_t* winroff, uint32_t* wmeta);

/* Parity probe: how the table build cut the DP chain of the whole table set into tasks and packed them for the
 * speculative pass (tables with DP rows, untrimmed), read from the device copies the kernels see.  counts4 is always
 * set: tasks after the merge, tasks merged into their predecessors, workgroups of text tasks, workgroups of run tasks.
 * Every array may be null (not copied), so a first call with all of them null asks for the sizes:
 *   tasks     4 words per task: block, q (first position walked: a cut point of the DP, or pout - warm-up), pout,
 *             pend (blocksize + 1 for a block's last task); the tasks of a block are consecutive and tile it
 *   task_off  nblocks + 1 words: the first task of every block
 *   wg_tasks  one word per task: the text tasks' list (per block the task indices in order), then the run tasks'.
 *             A task's kind is stored nowhere else: it is the list that holds it
 *   wg_desc   2 words per workgroup (counts4[2] + counts4[3] of them): first entry in wg_tasks, entries; at most
 *             ZOPFLI_AMD_SEG_STRETCH entries of one block and one list, the text workgroups first and among those of
 *             a kind the ones that hold a block's first task first */
int zmx_chain_tasks_download(zmx_ctx* ctx, zmx_tables* tables, uint64_t* counts4, uint32_t* tasks, uint32_t* task_off,
                             uint32_t* wg_tasks, uint32_t* wg_desc);

/* Test entry: TraceBackwards + FollowPath (squeeze.c:317, :338) over length arrays the CALLER hands in — the tail of
 * zmx_squeeze_run (k_trace_exits, k_trace_link, k_trace_emit and the result copy: the same code) without the DP in
 * front of it.  length_arrays[b] has entries[b] = blocksize + 1 cells, as zmx_length_array_download returns them; they
 * replace the tables' own; slot[b], nsym, hist and the stores are as after zmx_squeeze_run.  Refused on the host, before
 * any launch (ZMX_ERR_REFUSED): trimmed or matches-only tables, nblocks or an entries[b] that is not the tables', a
 * slot that is not 0 or 1, a cell h that holds 2 or more than min(h, 258).  A cell may hold 0 (GetBestLengths' "never
 * reached"): the device judges whether the path meets one (flag 0x2) or takes a length the match record at its start
 * does not hold (flag 0x4), and the call fails with "device consistency flags 0x..." (ZMX_ERR_DEVICE) as
 * zmx_squeeze_run does; the next call on the same tables is not affected. */
int zmx_trace_length_arrays(zmx_ctx* ctx, zmx_tables* tables, size_t nblocks, const uint16_t* const* length_arrays,
                            const size_t* entries, const int32_t* slot, uint32_t* nsym, uint32_t* hist);

/* -------- f-1 of SURVEY 8: the block-split search's cost function on the device
 *
 * ZopfliCalculateBlockSizeAutoType (deflate.c:610-621) of MANY ranges of LZ77 symbol sequences at once: what every
 * probe of ZopfliBlockSplitLZ77 evaluates twice (blocksplitter.c:103-135: EstimateCost, SplitCost).  The sizes are
 * integers; they come back as doubles as the reference returns them, equal to the host's
 * ZopfliCalculateBlockSizeAutoType value for value (tests/test_gpu_parity.py::test_block_costs).
 *
 * A zmx_cost_stores object is a set of symbol sequences ("stores", lz77.h:44-62) resident on the device with their
 * sampled prefix histograms (lz77.c:98-149's ll_counts / d_counts, here every 1024 symbols):
 *   zmx_cost_stores_create       sequence s = the concatenation of the device stores (block[p], slot[p], nsym[p]) of
 *                                `tables` for p in [piece_first[s], piece_first[s + 1]) — the greedy store of a master
 *                                block (blocksplitter.c:296), or the optimal parses of its blocks joined
 *                                (deflate.c:866); nothing crosses the bus
 *   zmx_cost_stores_create_host  the same from host arrays (lz77.h:44-49 convention).  Every pair must be a symbol:
 *                                dist == 0 with litlen <= 255, or 3 <= litlen <= 258 with 1 <= dist <= 32768 (what the
 *                                reference asserts); anything else is refused on the host, before any allocation or
 *                                launch (ZMX_ERR_REFUSED, the message names the sequence and the symbol)
 *   zmx_block_costs              cost[i] = ZopfliCalculateBlockSizeAutoType(sequence ranges[3 i], lstart = ranges[3 i + 1],
 *                                lend = ranges[3 i + 2])
 * A sequence holds fewer than 2^22 symbols (a master block has at most 1 000 000). */
typedef struct zmx_cost_stores zmx_cost_stores;
int zmx_cost_stores_create(zmx_ctx* ctx, zmx_tables* tables, size_t nstores, const size_t* piece_first,
                           const size_t* block, const int32_t* slot, const size_t* nsym, zmx_cost_stores** out);
int zmx_cost_stores_create_host(zmx_ctx* ctx, size_t nstores, const uint16_t* const* litlens,
                                const uint16_t* const* dists, const size_t* nsym, zmx_cost_stores** out);
void zmx_cost_stores_free(zmx_ctx* ctx, zmx_cost_stores* stores);
int zmx_block_costs(zmx_ctx* ctx, zmx_cost_stores* stores, size_t n, const uint32_t* ranges, double* cost);
/* ZopfliLZ77GetByteRange (lz77.c:160-166) from the start of a sequence: bytes[i] = the input bytes that symbols
 * [0, pairs[2 i + 1]) of sequence pairs[2 i] stand for — where a split point lies (blocksplitter.c:303-314). */
int zmx_cost_positions(zmx_ctx* ctx, zmx_cost_stores* stores, size_t n, const uint32_t* pairs, uint64_t* bytes);

/* -------- many independent inputs in one call
 *
 * n independent ZopfliCompress calls in one: out[i], outsize[i] end as ZopfliCompress(options, output_type, in[i],
 * insize[i], &out[i], &outsize[i]) leaves them (appended to, reference convention; the caller frees) — byte for byte,
 * whatever the other inputs and their order.  The inputs' master blocks are dealt over the contexts and devices of the
 * Zopfli* entry points together, so small files share the table builds, squeeze runs and bit writes of one large call
 * (zmx_set_input_segments keeps each input's window inside it).  With options->verbose stderr carries the lines of the
 * n calls, in input order.  0 on success (n = 0 included); -1 with zmx_last_error / zmx_last_error_class, and no out[i]
 * changed, on failure. */
int zmx_compress_batch(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                       const unsigned char* const* in, const size_t* insize,
                       unsigned char** out, size_t* outsize);

/* ZopfliCompress of `insize` bytes of DEVICE memory at `d_in` (see zmx_set_input_device for what is taken and what is
 * refused): *out, *outsize end as ZopfliCompress(options, output_type, the same bytes on the host, ...) leaves them —
 * byte for byte, appended to a malloc'ed host array under the reference's convention; the caller frees.  The input never
 * visits the host: the contexts copy their shards device to device (any device of ZOPFLI_AMD_DEVICES, whichever the
 * pointer lies on), the dealing takes its estimates from counts made on the device, and only the bytes of stored
 * blocks — incompressible data — come down, to be written into the stream.  Same context pool, dealing, priorities,
 * shard retry and rounds as ZopfliCompress.  The data must be complete when the call is made (the caller synchronises
 * its own stream); the buffer is only read and may be reused as soon as the call returns.  0 on success; -1 with
 * zmx_last_error / zmx_last_error_class, and *out, *outsize unchanged, on failure. */
int zmx_compress_device(const ZopfliOptions* options, ZopfliFormat output_type, const void* d_in, size_t insize,
                        unsigned char** out, size_t* outsize);

/* zmx_compress_batch for inputs that lie in device memory: out[i], outsize[i] end as ZopfliCompress(options, output_type,
 * the bytes of d_in[i] on the host, insize[i], ...) leaves them, byte for byte, whatever the other inputs, their order,
 * their addresses (adjacent slices of one allocation are still independent inputs) and their devices.  Nothing of a
 * compressible input visits the host; only stored blocks' bytes come down.  The inputs are put end to end on the device
 * (zmx_gather_device into a staging buffer of the call's own, a round of at most 2 GB at a time), the dealing takes its
 * estimates from counts made there, and the shards copy their bytes from the staging buffer.  The buffers are only read,
 * only during the call; the caller synchronises the streams that produced them.  0 on success (n = 0 included); -1 with
 * zmx_last_error / zmx_last_error_class and NO out[i] changed on failure, a refused pointer anywhere in the list included. */
int zmx_compress_device_batch(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                              const void* const* d_in, const size_t* insize, unsigned char** out, size_t* outsize);

/* zmx_compress_device whose OUTPUT stays in device memory as well: afterwards d_out[0, *outsize) holds the bytes that
 * ZopfliCompress(options, output_type, the same bytes on the host, ...) gives from an empty output, byte for byte.  The
 * stream never visits the host: the blocks' symbols' bits stay where the device's bit writer put them, stored blocks'
 * bytes are read from d_in, and one launch (zmx_bitjoin_device) joins them with what the host still makes — the
 * container's header and trailer, every block's header and tree, LEN / NLEN of stored pieces, and the whole of a block
 * the device could not write (the second split attempt moved its ends, or ZOPFLI_AMD_DEVICE_ENCODE=0) — uploaded in one
 * small buffer.  What still crosses the bus upward: the parse's histograms and, with block splitting, the symbols the
 * host's split search reads, as for every entry; no byte of the stream.
 * d_in is checked as zmx_compress_device checks it, d_out[0, capacity) the same way; d_out may not overlap d_in and lies
 * on the same device (ZMX_ERR_REFUSED before anything runs).  The stream's size is known on the host before the join: if
 * it exceeds `capacity` the call fails with ZMX_ERR_REFUSED, *outsize = the size needed, and nothing is written to d_out.
 * Any failure leaves d_out unwritten, and *outsize means something in the capacity case only.  zmx_compress_bound(format,
 * insize) is a capacity that always does for blocksplittingmax 1 .. 64 (ZopfliInitOptions: 15; the derivation is in
 * zopfli_amd/csrc/host/device_output_plan.h).  Synchronous; the caller synchronises the stream that produced d_in.
 * Limits: a call of more than one round — ZOPFLI_AMD_ROUND_PARTS master blocks, 2000 by default: 2 GB — is refused
 * (rounds are not joined on the device); the call is dealt over the contexts of the ONE device that holds d_out,
 * whatever ZOPFLI_AMD_DEVICES names, and that device must be one of the library's; d_in lies on that device too (the
 * join reads stored blocks' bytes from it); options->verbose prints nothing about the blocks (the reference's lines are
 * made where the host merges a stream, which this entry never does). */
int zmx_compress_device_to_device(const ZopfliOptions* options, ZopfliFormat output_type, const void* d_in, size_t insize,
                                  void* d_out, size_t capacity, size_t* outsize);
size_t zmx_compress_bound(ZopfliFormat output_type, size_t insize);

/* zmx_compress_device_batch whose streams stay in device memory: afterwards d_out[i][0, outsize[i]) holds what
 * ZopfliCompress(options, output_type, the bytes of d_in[i] on the host, insize[i], ...) gives from an empty output, byte
 * for byte, for every i.  Everything up to the blocks' bits runs as in zmx_compress_device_batch — the same gather into
 * the call's staging buffer, the same counts, dealing and shards — and the n streams are then put together as
 * zmx_compress_device_to_device puts its one: every stream planned as bit pieces from bit 0 with its own container header
 * and trailer, the plans' small host-made parts uploaded as ONE buffer, and ONE launch (zmx_bitjoin_many_device) for all
 * destinations.  Stored blocks' bytes are read from the staging buffer, so the inputs may lie on any device.
 * All sizes are known on the host before anything is written: if any destination is too small the whole call fails with
 * ZMX_ERR_REFUSED, outsize[i] = the size needed for EVERY i, and nothing is written anywhere.  After any other failure
 * every outsize[i] is 0 and nothing was written.  zmx_compress_bound(format, insize[i]) is a capacity that always does.
 * Refused before anything runs (ZMX_ERR_REFUSED): the inputs as zmx_compress_device_batch refuses them; a destination
 * that is null with a non-zero capacity, is host or managed memory or leaves its allocation; destinations on different
 * devices; a destination that shares a byte with another destination or with an input.  n = 0 returns 0.
 * Limits: a batch of more than one round — 2 GB of inputs — is refused before anything is read; the call runs on the
 * contexts of the one device that holds the destinations, which must be one of the library's; options->verbose prints
 * nothing about the blocks.  Synchronous; the caller synchronises the streams that produced the inputs.
 * zmx_last_output_traffic: [0] 0, [1] the uploaded buffer, [2] / [3] the blocks the device and the host wrote, summed over
 * the batch; zmx_last_input_traffic as for zmx_compress_device_batch with [2] = 0: no stored byte comes down. */
int zmx_compress_device_batch_to_device(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                                        const void* const* d_in, const size_t* insize, void* const* d_out,
                                        const size_t* capacity, size_t* outsize);
/* The same streams packed into one arena: stream i lies at d_arena + outoffset[i], outoffset[0] = 0 and outoffset[i] =
 * the end of stream i - 1 rounded up to `align`, a power of two from 1 to 4096 (1: back to back).  The bytes between
 * streams are not written, and two streams may share a 16-byte vector: each byte of a stream is still written exactly
 * once.  The destinations follow from the plans' sizes; otherwise this is the call above, with the arena for its
 * destinations in every rule.  An arena that is too small: ZMX_ERR_REFUSED, outsize[] and outoffset[] hold what is needed
 * (the arena must reach outoffset[n - 1] + outsize[n - 1]), nothing written.  zmx_compress_batch_bound(format, n, insize,
 * align) is a capacity that always does: every input's zmx_compress_bound rounded up to `align`, summed (0 for n = 0 or
 * an `align` that is not taken). */
int zmx_compress_device_batch_packed(const ZopfliOptions* options, ZopfliFormat output_type, size_t n,
                                     const void* const* d_in, const size_t* insize, void* d_arena, size_t capacity,
                                     size_t align, size_t* outoffset, size_t* outsize);
size_t zmx_compress_batch_bound(ZopfliFormat output_type, size_t n, const size_t* insize, size_t align);

/* -------- whole-stream entry points on a resident input (bench, multi-GPU) */

/* ZopfliDeflate (deflate.c:908) of bytes [instart, inend) of the resident input,
 * cut into 1 000 000-byte master blocks counted from instart (util.h:60), bytes
 * before instart serving as dictionary — i.e. the consecutive ZopfliDeflatePart
 * calls of deflate.c:916-923 for that range.  The result is serialised as
 * position-independent chunks (compressed blocks as bit strings, stored blocks
 * as raw bytes) so that ranges compressed on different GPUs can be joined by
 * zmx_chunks_merge.  `final` marks the last block of the range as BFINAL.
 * *blob is malloc'ed; caller frees. */
int zmx_deflate_range(zmx_ctx* ctx, const ZopfliOptions* options, size_t instart, size_t inend,
                      int final, unsigned char** blob, size_t* blobsize);

/* Concatenates chunk blobs (in stream order) into a deflate bit stream appended
 * to (*out,*outsize) at bit pointer *bp, exactly as the consecutive
 * ZopfliDeflatePart calls would have produced it. */
int zmx_chunks_merge(const unsigned char* const* blobs, const size_t* blobsizes, size_t nblobs,
                     unsigned char* bp, unsigned char** out, size_t* outsize);

/* -------- one process per GPU: the gather of the ranks' blobs over RCCL (xGMI inside a node)
 *
 * ZopfliDeflate's master blocks are independent (deflate.c:916-923): rank r of `world` runs
 * zmx_deflate_range on its contiguous range of master blocks, the blobs are gathered to rank 0 and
 * merged there with zmx_chunks_merge.  librccl is loaded with dlopen on first use.  (Inside ONE
 * process the Zopfli* entry points of part 1 already deal the master blocks over every visible
 * device: ZOPFLI_AMD_DEVICES.) */
typedef struct zmx_dist zmx_dist;

/* Rank 0: a fresh ncclUniqueId (128 bytes) that the launcher hands to every rank (file, environment,
 * MPI, torch.distributed ...). */
int zmx_dist_unique_id(unsigned char* id128);
/* Collective: the communicator of `world` ranks, this process being `rank` on ctx's device. */
int zmx_dist_init(zmx_ctx* ctx, int rank, int world, const unsigned char* id128, zmx_dist** dist);
void zmx_dist_destroy(zmx_dist* dist);
/* The number of ranks RCCL itself reports for the communicator (ncclCommCount), or -1. */
int zmx_dist_comm_count(zmx_dist* dist);
/* Collective: every rank contributes `size` bytes.  On rank 0 *gathered is a malloc'ed buffer holding
 * the blobs of rank 0, 1, ... back to back and sizes[r] their lengths (sizes has `world` entries);
 * elsewhere *gathered = NULL and sizes is not written. */
int zmx_dist_gather(zmx_dist* dist, const unsigned char* blob, size_t size, unsigned char** gathered,
                    size_t* sizes);

/* Cost-aware dealing of master blocks over GPUs (host only, no device call; zopfli_amd/csrc/host/deal.cc).  Master blocks
 * are independent (deflate.c:916-923) but not equally expensive: one of long runs of equal bytes costs several times one
 * of text.  cost[b] = the estimated cost of master block b of in[0, insize) relative to a master block of text, a function
 * of the bytes alone (64-byte probes every 1024) so that every rank computes the same numbers; returns the number of master
 * blocks (ncost must be at least that).  zmx_deal_master_blocks: contiguous ranges balanced by cost,
 * first[s] .. first[s + 1] for shard s (first has shards + 1 entries).  ZopfliCompress / ZopfliDeflate deal a call over
 * their contexts this way; one-process-per-GPU launchers (zopfli_amd/sharding.py, bench.py) call these two. */
int zmx_master_block_costs(const unsigned char* in, size_t insize, double* cost, size_t ncost);
int zmx_deal_master_blocks(const double* cost, size_t nblocks, size_t shards, size_t* first);
/* zmx_master_block_costs of the context's resident input (zmx_set_input or zmx_set_input_device), the probes counted on
 * the device (k_probe_counts): the same doubles, bit for bit. */
int zmx_master_block_costs_device(zmx_ctx* ctx, double* cost, size_t ncost);

/* (The kernel, match and task statistics below are sums over the last Zopfli* / zmx_deflate_range call of the CALLING
 * THREAD — its shard threads' numbers included — reset when the call starts: concurrent callers read their own.)
 *
 * Timing breakdown of the last Zopfli* / zmx_deflate_range call on this
 * thread: seconds spent in [0] match tables [1] greedy [2] squeeze runs
 * [3] host cost model [4] block split [5] encode [6] the chain kernels of the squeeze runs (k_dp5_spec,
 * k_dp5_stretch, k_dpcheck, k_dprecheck, k_dpscan, k_dp4_fix: GetBestLengths; HIP events on the launch stream) [7] squeeze runs launched.
 * For bench.py's roofline object. */
int zmx_last_timing(double* out8);

/* Kernel-only seconds (HIP events) of the squeeze runs since the last Zopfli* /
 * zmx_deflate_range call started: [0] k_wtab + k_badscan (the run's weight tables) [1] the chain kernels
 * [2] k_trace_* (exits + link + emit) [3] squeeze runs launched. */
int zmx_last_kernel_timing(double* out4);
/* The phase times of the squeeze runs (above; zmx_last_timing's dp_kernel) cost four event records and three readings a
 * run, a third of a run's runtime calls: they are taken only when asked for — this call, ZOPFLI_AMD_KERNEL_TIMING=1 or
 * ZOPFLI_AMD_PROF.  (The match-table times of zmx_last_match_timing are always taken: once per table build.) */
void zmx_set_kernel_timing(int on);

/* Host tail of the last call on this thread, seconds: [0] best LZ77 stores device -> host
 * [1] chunk serialisation (zmx_deflate_range). */
int zmx_last_host_timing(double* out2);

/* Input bytes the last Zopfli* / zmx_compress_* / zmx_deflate_range call on this thread moved: [0] host to device
 * [1] device to device [2] device to host.  (A shard's upload includes the 32 KiB window before its first block;
 * zmx_compress_device_batch: [1] counts the gather into the staging buffer and the shards' copies from it.) */
int zmx_last_input_traffic(double* out3);

/* Where the last call's stream went: [0] its bytes device to host (for the Zopfli* entries and zmx_compress_device: the
 * whole stream, the other three 0) [1] its bytes host to device — the literals buffer of zmx_compress_device_to_device,
 * blocks the host wrote included — [2] blocks whose symbols' bits never left the device [3] blocks the host wrote and
 * uploaded. */
int zmx_last_output_traffic(double* out4);

/* Match-table builds since the last Zopfli* / zmx_deflate_range call started (HIP events):
 * [0] seconds in the match kernel (k_match2 / k_match5) [1] seconds in k_same +
 * k_chain [2] table builds [3] positions whose record
 * the match kernel computed (the others were copied from the parent tables). */
int zmx_last_match_timing(double* out4);
/* The skip-walk (k_match5) of the table builds since the last Zopfli* call started / zmx_deflate_range: out3 = entries in
 * flight summed over lanes and wave iterations (a position's walk touches ~10 entries whatever its chains' length), wave
 * iterations, positions the kernel walked (blocks k_hits sent to it).  Zero when every block took k_match2. */
int zmx_last_match_walk(double* out3);

/* Several contexts on one device (the Zopfli* entry points keep up to three per device).  The budgets are the DEVICE's,
 * not a context's: what the pools of all its contexts keep cached between batches counts against one third of its memory
 * together, what one batch's DP edges may take is a third; a table build that cannot allocate (the other contexts are
 * busy) returns -2, "come back with fewer blocks", like one beyond that budget.  zmx_ctx_trim_cache gives an IDLE
 * context's cached arrays back to the device; the hook (one per process, may be null) is called with the device index when
 * an allocation still fails after the failing context dropped its own cache — the owner of the contexts trims the idle
 * ones there — and the allocation is tried once more.  zmx_ctx_set_share keeps nothing (the budgets are the device's, however many share it): it refuses a null context and
 * returns 0. */
typedef void (*zmx_oom_hook_t)(int device);
void zmx_set_oom_hook(zmx_oom_hook_t hook);
int zmx_ctx_set_share(zmx_ctx* ctx, unsigned contexts_on_device);
int zmx_ctx_trim_cache(zmx_ctx* ctx);
/* Which streams the context's next calls run on: 0 = the pair it was created with, +1 / -1 = a pair of the highest /
 * lowest priority the device has.  Only while the context is idle.  The Zopfli* entry points give the contexts a call with
 * block splitting is dealt over three different priorities (ZOPFLI_AMD_STREAM_PRIO=0: never). */
int zmx_ctx_set_priority(zmx_ctx* ctx, int level);

/* Which match-table kernel the table builds that START after this call use (the ZOPFLI_AMD_MATCH environment
 * variable sets the initial choice): 0 = per block, k_match5 where k_hits estimates long chains, k_match2 elsewhere
 * (the default), 2 = k_chain + k_match2, 5 = k_chain + k_levels + k_rank2 + k_match5 (the exact skip-walk) for every
 * block.  All produce the same records; an A/B and test hook.  3 and 4 named kernels that were removed: the call fails
 * (as for any other value), and ZOPFLI_AMD_MATCH=3 or 4 falls back to 2. */
int zmx_set_match_kernel(int kernel);

/* k_match2 hands out a tile's 2048 positions longest walk first (on, the default, or ZOPFLI_AMD_MATCH_ORDER=1), by the
 * estimate k_hits keeps for every position, or in ascending order (0).  The records are the same either way; with the
 * order on, k_hits also runs when kernel 2 is forced.  Tables built from a parent are always built in ascending
 * order.  An A/B and test hook; always returns 0. */
int zmx_set_match_order(int on);

/* The chain's tasks (GetBestLengths cut into verified stretches, zmx_dp4.h) since the last Zopfli* /
 * zmx_deflate_range call started: [0] tasks [1] accepted as computed [2] re-run because the entry
 * state differed [3] because the guessed level left the binade [4] because a weight could tie
 * [5] positions re-run serially [6] re-run because the entry values differed by more than a shift
 * [7] block positions of all squeeze runs. */
int zmx_last_seg_stats(double* out8);

/* ---- Inflate on the device: raw deflate, zlib and gzip streams in device memory decoded into device memory.
 * What the *_to_device entries leave in HBM, read back where it lies; any conforming stream, not only this library's.
 * k_inflate (device/zmx_inflate.h): one wavefront a stream, a batch of n streams one launch.  A stream is valid exactly
 * where inflate() of zlib 1.2.11 accepts it.  Bytes behind the trailer are no error and a second gzip member is not
 * followed: `consumed` says where it begins.  Preset dictionaries (zlib's FDICT) are not taken.
 * How a stream ended: */
#define ZMX_INFLATE_OK 0
#define ZMX_INFLATE_HEADER 1            /* a zlib or gzip header that is none */
#define ZMX_INFLATE_DICT 2              /* zlib's FDICT is set */
#define ZMX_INFLATE_BLOCK_TYPE 3        /* block type 3 */
#define ZMX_INFLATE_STORED_LEN 4        /* a stored block's LEN is not ~NLEN */
#define ZMX_INFLATE_TOO_MANY_SYMBOLS 5  /* HLIT > 286 or HDIST > 30 */
#define ZMX_INFLATE_REPEAT 6            /* a repeat with no previous length, or one that runs past HLIT + HDIST */
#define ZMX_INFLATE_OVERSUBSCRIBED 7    /* an over-subscribed set of code lengths */
#define ZMX_INFLATE_INCOMPLETE 8        /* an incomplete set (but a literal/length or distance set of one one-bit code) */
#define ZMX_INFLATE_NO_END_CODE 9       /* no code for symbol 256 */
#define ZMX_INFLATE_BAD_CODE 10         /* a bit pattern no code owns */
#define ZMX_INFLATE_BAD_SYMBOL 11       /* literal/length symbol 286 or 287, distance symbol 30 or 31 */
#define ZMX_INFLATE_DISTANCE 12         /* a distance behind the first byte of the output */
#define ZMX_INFLATE_TRUNCATED 13        /* the input ends before the final block or the trailer does */
#define ZMX_INFLATE_CAPACITY 14         /* the output takes more than `capacity`: outsize says how much */
#define ZMX_INFLATE_CHECKSUM 15         /* the output's CRC-32 / Adler-32 is not the trailer's (the pooled entries) */
#define ZMX_INFLATE_SIZE 16             /* gzip's ISIZE is not the output's size mod 2^32 (the pooled entries) */
/* zmx_last_error_class() after a stream that is no valid stream (every status above but OK and CAPACITY): the data is at
 * fault, not the request or the device. */
enum { ZMX_ERR_DATA = 4 };

typedef struct {
  uint64_t outsize;       /* bytes the stream decodes to (up to where it failed) */
  uint64_t consumed;      /* bytes of input up to and including the trailer (up to the failing bit) */
  uint32_t status;        /* a ZMX_INFLATE_* */
  uint32_t block;         /* the index of the deflate block it stopped in */
  uint32_t stored_check;  /* the trailer's CRC-32 (gzip) or Adler-32 (zlib) */
  uint32_t stored_isize;  /* gzip's ISIZE */
} zmx_inflate_result;

/* The step, on a context the caller holds: stream i is d_in[i][0, insize[i]), its output goes to d_out[i][0, capacity[i]),
 * all plain memory of the context's device.  A null d_out[i] (or a null d_out) is the size-only mode: the same walk,
 * nothing stored.  Output beyond capacity[i] is not stored; the stream is walked to its end all the same, so that outsize
 * is what it takes (ZMX_INFLATE_CAPACITY).  No checksum is compared: the results carry the trailers.  Refused
 * (ZMX_ERR_REFUSED) before anything is launched: an unknown format, a pointer that is not device memory of the context's
 * device, a range that leaves its allocation, a destination that shares a byte with an input or with another destination
 * (the message names the index).  Returns 0 when every stream is ZMX_INFLATE_OK (n = 0: at once); -1 with every result
 * filled in when one is not: zmx_last_error() names the first failing index and its status (for CAPACITY also outsize),
 * zmx_last_error_class() is ZMX_ERR_REFUSED for CAPACITY, else ZMX_ERR_DATA. */
int zmx_inflate_device_ctx(zmx_ctx* ctx, ZopfliFormat format, size_t n, const void* const* d_in, const size_t* insize,
                           void* const* d_out, const size_t* capacity, zmx_inflate_result* results);
/* The same on a context from the library's pool, with the checksums verified: after k_inflate the output of every gzip or
 * zlib stream that ended OK with its output stored goes through zmx_checksum_device's two kernels (one launch pair for the
 * batch) and the values are compared with the trailers — ZMX_INFLATE_CHECKSUM — and gzip's ISIZE with outsize mod 2^32 —
 * ZMX_INFLATE_SIZE.  32 n bytes come down and then 4 n; no byte of a stream or of its output visits the host.  All
 * ranges must lie on one of the library's devices. */
int zmx_inflate_device_batch(ZopfliFormat format, size_t n, const void* const* d_in, const size_t* insize, void* const* d_out,
                             const size_t* capacity, zmx_inflate_result* results);
/* ... of one stream; *outsize as zmx_inflate_result.outsize. */
int zmx_inflate_device(ZopfliFormat format, const void* d_in, size_t insize, void* d_out, size_t capacity, size_t* outsize);

/* ---- PNG decode on the device: PNG files in device memory decoded into device memory — this library's *_to_device
 * output, a dataset shard copied up as it lies on disk, tiles from another rank.  Made for many small files in one call:
 * k_png_chunks walks the chunks of all files in one launch (a lane a file), the IDAT streams go through k_inflate (one
 * wavefront a stream: a single large image is bound by that kernel's one-wave rate, see README), the chunks' CRC-32s and
 * the streams' Adler-32s through zmx_checksum_device's kernels, and k_png_unfilter (device/zmx_png_decode.h, one wavefront
 * an image) undoes the five scanline filters and writes the pixels.  No byte of a file, of its stream or of its pixels
 * visits the host: what comes down is 88 bytes a file of chunk records, 24 a checked chunk, 32 a stream of inflate
 * results, 4 a checksum, 8 a file of unfilter results and 1 KiB a file of palettes when a file has a PLTE.
 * A file is valid exactly where LodePNG's lodepng_decode with default settings accepts it, but:
 *   - Adam7 files are recognised and not decoded (ZMX_PNG_DECODE_INTERLACE);
 *   - ancillary chunks other than tRNS are skipped unread, so a file LodePNG refuses only for the CONTENTS (or the CRC) of
 *     a gAMA, tEXt ... chunk is accepted here;
 *   - of several tRNS chunks behind one PLTE the last alone holds.
 * Bytes after IEND are no error; IDATs need not be adjacent and may be empty.
 * Out of scope: Adam7, the contents of ancillary chunks (gamma, ICC, text), APNG, a faster single large stream, and
 * libzopflipng_amd.so, which keeps LodePNG's decoder.  These entries write the two modes below; strided, planar, float,
 * 16-bit and little-endian output is the zmx_png_sink's, further down.  How a file ended (the order is the order the
 * checks are made in): */
#define ZMX_PNG_DECODE_OK 0
#define ZMX_PNG_DECODE_SIGNATURE 1   /* a bad signature, or a file shorter than 33 bytes */
#define ZMX_PNG_DECODE_IHDR 2        /* not IHDR first or its length not 13; width or height 0; an illegal colour type and
                                        depth; a compression or filter method not 0; interlace above 1 */
#define ZMX_PNG_DECODE_INTERLACE 3   /* interlace method 1, in a file whose chunks are in order */
#define ZMX_PNG_DECODE_CHUNK 4       /* no room for a chunk's 12 bytes before IEND; a length above 2^31 - 1; a chunk that
                                        runs past the file's end */
#define ZMX_PNG_DECODE_CRITICAL 5    /* an unknown critical chunk */
#define ZMX_PNG_DECODE_CRC 6         /* the stored CRC-32 of IHDR, a PLTE, a tRNS, an IDAT or IEND is not its type's and data's */
#define ZMX_PNG_DECODE_PLTE 7        /* colour type 3 without PLTE; 0 or more than 256 entries */
#define ZMX_PNG_DECODE_TRNS 8        /* longer than the palette (so also in front of PLTE); not 2 bytes for grey, 6 for RGB;
                                        present for colour types 4 and 6 */
#define ZMX_PNG_DECODE_STREAM 9      /* the IDAT bytes are no valid zlib stream (detail: the ZMX_INFLATE_*, CHECKSUM for the
                                        Adler-32); no IDAT byte at all: ZMX_INFLATE_TRUNCATED */
#define ZMX_PNG_DECODE_SIZE 10       /* the stream does not decode to exactly height * (1 + linebytes) bytes */
#define ZMX_PNG_DECODE_FILTER 11     /* a row's filter byte is above 4 (detail: the first such row) */
#define ZMX_PNG_DECODE_CAPACITY 12   /* the pixels take more than capacity[i]: outsize says how much; nothing is stored */
#define ZMX_PNG_DECODE_SHAPE 13      /* the sink entries: the file's width or height is not its sink's.  Checked after the walk
                                        and the CRCs, before the stream is read: nothing is inflated, nothing stored */

#define ZMX_PNG_DECODE_OWN 0    /* the file's own colour type and depth, in the layout the encode entries read:
                                   zmx_png_image.d_pixels for colour types 0, 2, 4, 6 at 8 or 16 bits (16-bit samples
                                   big-endian), zmx_png_index_image.d_pixels for palette images and grey below 8 bits (rows
                                   of (width * bitdepth + 7) / 8 bytes, the padding bits of a row's last byte zero) */
#define ZMX_PNG_DECODE_RGBA8 1  /* 4 * width * height bytes, what lodepng_decode32 gives: the palette with its tRNS alpha
                                   (an index at or above palettesize: 0, 0, 0, 255), grey replicated, low-bit grey scaled
                                   by v * 255 / (2^depth - 1), the high byte of 16-bit samples, alpha 0 for a pixel equal to
                                   the tRNS key at full depth */

typedef struct {
  uint32_t status;        /* a ZMX_PNG_DECODE_* */
  uint32_t detail;        /* _STREAM: the ZMX_INFLATE_*; _CRC, _CHUNK, _CRITICAL, _PLTE, _TRNS: the chunk's number in the
                             file (IHDR is 0); _FILTER: the row */
  uint32_t width, height, colortype, bitdepth, interlace;
  uint32_t palettesize;   /* entries of PLTE (0 without one) */
  uint32_t has_key, key_r, key_g, key_b;   /* tRNS of colour types 0 and 2, at the file's depth */
  uint64_t outsize;       /* bytes the pixels take in the asked mode (zmx_png_info_device: _OWN) */
  uint64_t outsize_own, outsize_rgba8;     /* ... in either mode */
  unsigned char palette[1024];  /* r, g, b, a per entry; alpha from tRNS, 255 where it is short */
} zmx_png_decode_result;

/* The chunk walk alone: everything of the results but the pixels, for n files d_file[i][0, filesize[i]) on one of the
 * library's devices.  The chunks' CRCs are compared; the stream is not read.  Returns and refuses as the decode entries. */
int zmx_png_info_device(size_t n, const void* const* d_file, const size_t* filesize, zmx_png_decode_result* results);
/* The decode on a context the caller holds: file i's pixels in `mode` go to d_out[i][0, capacity[i]), all plain memory of
 * the context's device.  A null d_out[i] (or a null d_out) is the size-only mode: the walk, the CRCs and the stream's size
 * check (k_inflate's size-only mode: the Adler-32 is not compared), nothing stored.  Refused (ZMX_ERR_REFUSED) before
 * anything runs: an unknown mode, a null array, a pointer that is not device memory of the context's device, a range that
 * leaves its allocation, a destination that shares a byte with a file or with another destination (the message names the
 * index); and after the walk, before any stream is read: a header whose scanlines take 2^40 bytes or more.  Returns 0
 * when every file is ZMX_PNG_DECODE_OK (n = 0: at once); else -1 with every result filled in: zmx_last_error() names the
 * first failing index and its status, zmx_last_error_class() is ZMX_ERR_REFUSED for _CAPACITY, else ZMX_ERR_DATA.  Files
 * beside a bad one decode normally.  What was written of an image that ends _FILTER is unspecified, but inside its
 * destination.  `hooks` may be null; tests use it. */
typedef struct {
  int force_wide;          /* every image takes the wide path (the band carry through global memory, a launch a band) */
  uint32_t idat_capacity;  /* chunk entries a file in the first walk (0: the library's own, 8) */
} zmx_png_decode_hooks;
int zmx_png_decode_device_ctx(zmx_ctx* ctx, int mode, size_t n, const void* const* d_file, const size_t* filesize,
                              void* const* d_out, const size_t* capacity, zmx_png_decode_result* results,
                              const zmx_png_decode_hooks* hooks);
/* The same on a context from the library's pool; all ranges must lie on one of the library's devices.
 * zmx_last_input_traffic()[0] and zmx_last_output_traffic()[0] are 0: nothing of a file or of its pixels crosses. */
int zmx_png_decode_device_batch(int mode, size_t n, const void* const* d_file, const size_t* filesize, void* const* d_out,
                                const size_t* capacity, zmx_png_decode_result* results);
/* ... of one file. */
int zmx_png_decode_device(int mode, const void* d_file, size_t filesize, void* d_out, size_t capacity, zmx_png_decode_result* result);

/* -------- decode into strided, planar, float and 16-bit tensors
 *
 * The mirror of zmx_png_source: a zmx_png_sink says where sample (y, x, c) of a decoded image GOES — a (C, H, W) float
 * plane set, one image of an (N, C, H, W) batch, a pitched BGRA frame, a crop, a bottom-up frame, a [::2] view.  `channels`
 * 1, 2, 3, 4 ask for grey, grey + alpha, RGB, RGBA (LodePNG's LCT_GREY, LCT_GREY_ALPHA, LCT_RGB, LCT_RGBA) at `bitdepth` 8
 * or 16; PNG channel k of a pixel goes to sink channel order[k].
 * The value rule: the integer v of a sample is what LodePNG's lodepng_convert gives from the file's own mode — its
 * palette with the tRNS alpha, its tRNS key — into the mode (that colour type, bitdepth):
 *   file depth 16 and bitdepth 16: the file's 16-bit values themselves, grey replicated into R, G, B; alpha 65535, or 0
 *     for a pixel equal to the key in every channel at full depth;
 *   every other pair: the RGBA8 value of ZMX_PNG_DECODE_RGBA8 (lodepng_decode32's, see above), at bitdepth 16 the byte
 *     replicated, v * 257;
 *   grey from a colour file: the R value (LodePNG's average is commented out);
 *   a palette index at or above palettesize: 0, 0, 0, 255.
 * From v to the sample: U8 needs bitdepth 8, the byte; U16 needs bitdepth 16, the value stored native (little-endian);
 * U8 at 16 and U16 at 8 are refused; F32 is fl32(v) / maxv, maxv = 255.0f or 65535.0f, ONE correctly rounded fp32
 * division (what numpy.float32(v) / numpy.float32(maxv) gives, never a multiply by a reciprocal); F16 and BF16 are that
 * quotient rounded to nearest-even into the type.
 * zmx_png_sink_check: host arithmetic — 0, or -1 (ZMX_ERR_REFUSED) for a sink that is refused without asking the runtime
 * about its memory.
 * zmx_png_unpack_device: d_own[i] holds an image's pixels as ZMX_PNG_DECODE_OWN writes them (outsize_own bytes) and
 * modes[i] says what they are — width, height, colortype, bitdepth, palettesize, palette, the key; a result of
 * zmx_png_info_device or of a decode serves as it is.  ONE launch of k_png_unpack (device/zmx_png_unpack.h) on the
 * context's stream stores all n images through their sinks: every byte of every sample of a sink is written exactly
 * once, no other byte — not the pitch's padding, not the bytes between [::2] samples —, no input is written.
 * Synchronous; n = 0 returns 0.  Refused besides the list below: a modes[i] that is not ZMX_PNG_DECODE_OK or whose colour
 * type and depth are not legal, a sink whose width or height is not the mode's, a d_own[i] range that is not memory of
 * the context's device.
 * The decode entries: zmx_png_decode_device_ctx / _batch / zmx_png_decode_device with sinks in the destinations' place.
 * The walk, the CRCs, k_inflate, the Adler-32s and k_png_unfilter run unchanged, the last into _OWN pixels in a buffer of
 * the call's own; ONE k_png_unpack launch then covers every file that ended OK.  A file whose width or height is not its
 * sink's ends ZMX_PNG_DECODE_SHAPE — nothing of it is inflated, nothing stored into its sink, its result carries the
 * header.  Every other status, the return value, zmx_last_error*, files beside a bad one and the traffic counters (both
 * 0) are as for zmx_png_decode_device_batch; what a sink holds after _FILTER is unspecified but inside its samples.
 * There is no size-only mode.  `hooks` as in zmx_png_decode_device_ctx.
 * Refused before anything runs (ZMX_ERR_REFUSED), the message naming the index: a null argument, width or height 0,
 * channels outside 1 .. 4, an unknown sample type, a bit depth other than 8 or 16, the two refused type/depth pairs, an
 * `order` that is no permutation, a d_data or a stride that is no multiple of the sample's size, a sink whose samples
 * can share a byte — of the three dimensions with an extent above 1, sorted by |stride| ascending, each |stride| must be
 * at least the sample's size plus the sum of |stride_j| * (extent_j - 1) over the smaller ones, so stride 0 is refused
 * here —, an EXTENT (as a source's) that overflows 64 bits, is not plain device memory of the context's device or leaves
 * its allocation, or that overlaps a file, the input pixels or another sink's extent.
 * Out of scope: Adam7, broadcast sinks, a colour-to-grey rule other than LodePNG's, gamma. */
typedef struct zmx_png_sink {
  void* d_data;                         /* sample (y, x, c) goes to d_data + y*stride_y + x*stride_x + c*stride_c (bytes) */
  int64_t stride_y, stride_x, stride_c; /* bytes; multiples of the sample's size; any sign */
  uint32_t width, height, channels /* 1 .. 4 */, sample /* ZMX_PNG_SAMPLE_* */;
  uint32_t bitdepth;                    /* of the values: 8 or 16 */
  uint8_t order[4];                     /* PNG channel k of a pixel goes to sink channel order[k] */
} zmx_png_sink;
int zmx_png_sink_check(const zmx_png_sink* sink);
int zmx_png_unpack_device(zmx_ctx* ctx, size_t n, const zmx_png_decode_result* modes, const void* const* d_own,
                          const zmx_png_sink* sinks);
int zmx_png_decode_sink_device_ctx(zmx_ctx* ctx, size_t n, const void* const* d_file, const size_t* filesize,
                                   const zmx_png_sink* sinks, zmx_png_decode_result* results, const zmx_png_decode_hooks* hooks);
int zmx_png_decode_sink_device_batch(size_t n, const void* const* d_file, const size_t* filesize, const zmx_png_sink* sinks,
                                     zmx_png_decode_result* results);
int zmx_png_decode_sink_device(const void* d_file, size_t filesize, const zmx_png_sink* sink, zmx_png_decode_result* result);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* ZOPFLI_AMD_H_ */
