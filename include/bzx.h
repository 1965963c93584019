/*
 * bzx.h -- C ABI of the MI355X-native bzip2 block-compression core (libbzx.so).
 *
 * This is the drop-in boundary for the per-block hot path of ohsnyt/bzip2-rust
 * (RLE1 -> BWT -> MTF -> RLE2 -> multi-table Huffman -> bit packing).  The reference has
 * no FFI of its own; the seam is the Rust function
 *     pub fn compress_block(block: &[u8], block_crc: u32) -> (Vec<u8>, u8)
 *                                               src/compression/compress_block.rs:24
 * its producer RLE1Block (src/tools/rle1.rs:33-263) and its consumer BitWriter
 * (src/bitstream/bitwriter.rs:42-172).  Every entry point below names the reference
 * interface it replaces.  INTEGRATION.md shows the Rust `extern "C"` block a maintainer
 * would add.  Plain pointers and sizes only; all functions return 0 or a negative
 * BZX_E_* code and never unwind.
 *
 * Output bits are those of C bzip2 1.0.8 (libbz2), which BASELINE.json's metric names;
 * where the Rust reference diverges from libbz2 libbz2 wins.
 *
 * There is NO CPU implementation behind this ABI: every compute entry point needs a HIP
 * device and fails with BZX_E_NODEVICE without one.
 */
#ifndef BZX_H
#define BZX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BZX_OK 0
#define BZX_E_NODEVICE (-1)   /* no HIP device / HIP runtime error at init */
#define BZX_E_PARAM (-2)      /* bad argument (null pointer, n == 0, n > 900000, level not 1..9) */
#define BZX_E_NOMEM (-3)      /* host or device allocation failed */
#define BZX_E_OUTBUF (-4)     /* output buffer too small */
#define BZX_E_HIP (-5)        /* HIP runtime error during a call (see bzx_last_error) */
#define BZX_E_STATE (-6)      /* call sequence error (stream API) */
#define BZX_E_DATA (-7)       /* decompression: not a bzip2 stream, damaged data, or a CRC mismatch (see bzx_last_error) */

#define BZX_MAX_BLOCK 900000u

typedef struct bzx_ctx bzx_ctx;

/* Library / device management (replaces the rayon global pool, compress.rs:128). */
const char *bzx_version(void);
const char *bzx_strerror(int code);
/* HIP error text of the last failing call on this context ("" if none). */
const char *bzx_last_error(const bzx_ctx *ctx);
/* device: HIP device ordinal.  max_blocks: expected batch size (slabs grow on demand). */
int bzx_ctx_create(int device, uint32_t max_blocks, bzx_ctx **out);
void bzx_ctx_destroy(bzx_ctx *ctx);
/* Run all work of this context on an existing HIP stream (hipStream_t passed as void*). */
int bzx_ctx_set_stream(bzx_ctx *ctx, void *hip_stream);

/*
 * compress_block (compress_block.rs:24-67).  blk = one RLE1'd block, crc = CRC of the raw
 * bytes it covers.  out receives the byte-aligned block image (48-bit magic, crc, randomised
 * bit, origPtr, symbol map, selectors, coding tables, payload), last byte zero padded;
 * *pad_bits = number of pad bits (0..7), i.e. BitPacker::padding (bitpacker.rs:20-21).
 * Host pointers.  cap >= n + n/50 + 1024 is always enough.
 * Thread-safe and re-entrant like the Rust function: the reference calls it from every rayon worker at once
 * (compress.rs:125-132).  Calls that arrive together on one context are collected into one device batch (the
 * first caller leads it, the others block until their block is done); a lone caller pays a 0.3 ms window.
 * All other entry points of a context are serialised against each other by an internal lock.
 */
int bzx_compress_block(bzx_ctx *ctx, const uint8_t *blk, size_t n, uint32_t crc, uint8_t *out, size_t cap,
                       size_t *out_len, uint8_t *pad_bits);

/*
 * Batched form: what the rayon fan-out over blocks (compress.rs:125-132) becomes.  All
 * nblk blocks are resident on the device at once and every stage kernel runs over the
 * whole batch.  Host pointers.
 */
int bzx_compress_blocks(bzx_ctx *ctx, uint32_t nblk, const uint8_t *const *blks, const size_t *ns,
                        const uint32_t *crcs, uint8_t *const *outs, const size_t *caps, size_t *out_lens,
                        uint8_t *pads);

/*
 * Stage entry points (host pointers), one per stage function of the reference, used by the
 * parity tests to compare each device stage with the oracle:
 *   bzx_stage_bwt       bwt_encode            src/bwt_algorithms/bwt_sort.rs:27
 *   bzx_stage_mtf       rle2_mtf_encode       src/tools/rle2_mtf.rs:23
 *   bzx_stage_huffman   huf_encode tables     src/huffman_coding/huffman.rs:87-374
 *   bzx_stage_encode    huf_encode, all of it (tables + bits) behind the block header, for a given symbol stream
 */
int bzx_stage_bwt(bzx_ctx *ctx, const uint8_t *blk, size_t n, uint8_t *bwt_out, uint32_t *orig_ptr,
                  uint32_t *status);
int bzx_stage_mtf(bzx_ctx *ctx, const uint8_t *bwt, size_t n, uint16_t *mtfv_out, uint32_t *n_mtf,
                  uint32_t freq_out[258], uint8_t in_use_out[256]);
int bzx_stage_huffman(bzx_ctx *ctx, const uint16_t *mtfv, uint32_t n_mtf, const uint32_t freq[258],
                      uint32_t alpha_size, uint32_t *n_groups, uint32_t *n_selectors, uint8_t *selectors,
                      uint8_t len_out[6][258], uint32_t code_out[6][258]);
/*
 * Test/diagnostic: the Huffman stage and the emit stage of ONE block over a symbol stream the caller supplies (mtfv ends
 * with EOB = alphabet - 1, every symbol is below the alphabet size, freq counts the symbols of mtfv; the alphabet is
 * the number of non-zero in_use entries + 2).  out/out_len/pad_bits: the byte-aligned block image as bzx_compress_block
 * gives it; selector_mtf: info->n_selectors entries (room for 18002); info: n = n_mtf - 1, periodic = 0, the section
 * sizes and the total as bzx_get_block_info reports them.  BZX_E_PARAM as bzx_stage_huffman, also for a symbol outside
 * the alphabet, orig_ptr >= 2^24 or a stream whose image would not fit a block's output slab (no block of real data
 * gets there); BZX_E_OUTBUF with *out_len = bytes needed when cap is too small.
 */
struct bzx_block_info;
int bzx_stage_encode(bzx_ctx *ctx, const uint16_t *mtfv, uint32_t n_mtf, const uint32_t freq[258],
                     const uint8_t in_use[256], uint32_t orig_ptr, uint32_t crc, uint8_t *out, size_t cap,
                     size_t *out_len, uint8_t *pad_bits, uint8_t *selector_mtf, struct bzx_block_info *info);
/*
 * Test/diagnostic: how this build's emit stage cuts a block's payload.  *tile_groups: 50-symbol groups per tile (a tile
 * is packed in LDS and written out by the whole workgroup); *tiles_per_item: consecutive tiles of one block a workgroup
 * takes per work item; *staging_bits: payload bits of a tile the LDS staging area holds at any bit phase -- at least
 * tile_groups * 850, the most a tile can have, so every tile goes through it.  Needs no context and no device.
 */
void bzx_emit_geometry(uint32_t *tile_groups, uint32_t *tiles_per_item, uint32_t *staging_bits);

/*
 * RLE1 + block split + per-block CRC (replaces RLE1Block, rle1.rs:33-263, and do_crc,
 * crc.rs:15-22) with libbz2's split rule.  Host pointers; whole input at once.
 * blocks_out: nblk_cap slabs of BZX_MAX_BLOCK bytes; ns/crcs: per block.  *nblk = blocks made.
 */
int bzx_split_rle1(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, uint8_t *blocks_out,
                   uint32_t nblk_cap, uint32_t *ns, uint32_t *crcs, uint32_t *nblk);

/*
 * Whole buffer -> .bz2 with every stage on the device (replaces compress(), compress.rs:40-136,
 * minus file I/O).  d_raw / d_out are DEVICE pointers (HBM); nothing but the final length
 * crosses PCIe.  cap >= len + len/50 + 4096.  Alignment: d_raw 16 bytes, d_out 4 bytes (BZX_E_PARAM otherwise,
 * with the reason in bzx_last_error): a view into a larger device tensor must start on such a boundary.
 * Cost: blocks that are an exact power u^k (inputs made of one repeated byte and the like) need
 * libbz2's tie order among identical rotations: ~0.1 s for an all-zero block instead of milliseconds, and up to
 * seconds for many copies of a long unit (measured worst case over the committed sweep of units of 1..30,011 bytes:
 * 29 copies of a 30,011-byte unit, 4.1 s for that one block).  Such blocks of one call are handled side by side; the
 * context serialises its entry points, so other callers of the SAME context wait that long (use one context per
 * caller where that matters).
 */
int bzx_compress_device(bzx_ctx *ctx, const void *d_raw, size_t len, int level, void *d_out, size_t cap,
                        size_t *out_len);
/* Same with host buffers (H2D, device pipeline, D2H). */
int bzx_compress_buffer(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, uint8_t *out, size_t cap,
                        size_t *out_len);

/*
 * Batched compression: count independent inputs -> count independent .bz2 streams, all on the device.  The form for
 * many small objects (files, records, pages): their blocks share device batches, so a batch of thousands of inputs
 * costs a few launches and host synchronisations per round instead of some twenty launches and three
 * synchronisations per input.
 * Stream i is byte-identical to bzx_compress_device on input i alone (and to libbz2's output at that level); an empty
 * input gives the 14-byte empty stream.  Stream i starts at d_out + out_offs[i] (offsets ascend with i and are
 * multiples of 4; the bytes between two streams are zero) and is out_lens[i] bytes long.  out_offs / out_lens are HOST
 * arrays of count entries.
 * d_raws: HOST array of count DEVICE pointers, each 16-byte aligned (NULL allowed where lens[i] == 0); d_out: DEVICE
 * buffer of cap bytes, 4-byte aligned.
 * Returns BZX_OK at once for count == 0 (nothing written); BZX_E_PARAM for a bad level, NULL arrays or a misaligned
 * pointer (bzx_last_error names the input); BZX_E_OUTBUF when the streams do not fit cap
 * (bzx_compress_batch_bound(count, lens) always fits).  After any error the context stays usable.
 * Rounds: the inputs run in device rounds of whole inputs with at most R blocks each, R = the larger of the block
 * slabs the context holds (at least the max_blocks of bzx_ctx_create, 16 for 0; more after a larger call) and the
 * blocks of the largest single input.  A small input is one block, so R is also the number of small inputs per round;
 * a slab costs about 28 MB of device memory: a larger max_blocks means fewer rounds and more memory.  A call costs one
 * host synchronisation for the block counts of all inputs, one per round and one at the end.
 * bzx_get_stats after a batch call: nblk, n_periodic, raw_bytes, rle1_bytes, mtf_symbols and out_bits are sums over
 * all streams, the stage times and sorter counters are summed over the rounds, ms_total is the device time of the
 * call.  bzx_get_block_info after a batch call returns BZX_E_STATE (no per-block figures are kept).
 */
/* Upper bound of the output of a batch: sum over i of round_up4(lens[i] + lens[i]/50 + 4096). */
size_t bzx_compress_batch_bound(uint32_t count, const size_t *lens);
int bzx_compress_batch_device(bzx_ctx *ctx, uint32_t count, const void *const *d_raws, const size_t *lens, int level,
                              void *d_out, size_t cap, size_t *out_offs, size_t *out_lens);
/* The same with host buffers: the inputs are staged to the device (H2D) and the streams come back (D2H).  The staged
 * inputs and the outputs of one call are all on the device at once (about twice the input), for that call only. */
int bzx_compress_batch_buffer(bzx_ctx *ctx, uint32_t count, const uint8_t *const *raws, const size_t *lens, int level,
                              uint8_t *out, size_t cap, size_t *out_offs, size_t *out_lens);

/*
 * Multi-GPU sharding (replaces the rayon fan-out over blocks, compress.rs:125-132, across
 * devices): bzip2 block i belongs to rank i mod world.  No collective happens inside the library; the
 * caller (one process per GPU) exchanges 8 bytes per block between the two calls:
 *   1. bzx_shard_prepare: split the whole input (block boundaries are a serial dependency over the
 *      stream, so every rank derives them from its copy of the raw bytes), run BWT/MTF/Huffman on this
 *      rank's blocks, write size-in-bits | crc << 32 of each to d_bits[i] (int64, device; other entries untouched).
 *   2. caller: all-reduce(sum) d_bits over the ranks.
 *   3. bzx_shard_emit_packed: lay out the whole stream from all sizes, emit this rank's block images back to
 *      back into d_packed (each on a 32-bit word boundary, with the bit phase it has in the final stream).
 *   4. caller: gather the packed buffers to one rank (each compressed byte crosses xGMI once).
 *   5. on that rank: bzx_shard_assemble_begin (zeroed stream + "BZh<level>" + footer + combined CRC), then
 *      bzx_shard_assemble_rank once per rank: word-wise OR of the images into their final positions.
 */
int bzx_shard_prepare(bzx_ctx *ctx, const void *d_raw, size_t len, int level, uint32_t rank, uint32_t world,
                      uint32_t *nblk_total, long long *d_bits, size_t bits_cap);
/*
 * The same with the split ANALYSIS sharded too (the reference's producer touches every byte once,
 * rle1.rs:89-223): the two per-byte passes of the block splitter -- run starts, and RLE1 byte counts of the 8 KiB tiles
 * that hold runs -- run on this rank's 1/world share of the tiles only; the ranks exchange 24 bytes per tile, and only
 * the chain of block boundaries (a serial dependency over the stream, libbz2's split rule) is walked by every rank.
 * d_tiles: int64[3 * P * world] on every rank, P = bzx_shard_scan_entries(len, world); array a (a = 0, 1, 2) starts at
 * d_tiles + a * P * world and rank r owns its entries [r * P, (r + 1) * P).
 *   1a. bzx_shard_scan_runs      then caller: all-gather, in place, of the rank's P entries of array 0
 *   1b. bzx_shard_scan_counts    then caller: all-gather, in place, of the rank's P entries of arrays 1 and 2
 *   1c. bzx_shard_prepare_scanned = bzx_shard_prepare without the per-byte passes; steps 2..5 as above.
 * A rank reads the raw bytes of its own tiles (plus the 4 bytes before them) in 1a/1b and of its own blocks afterwards.
 */
size_t bzx_shard_scan_entries(size_t len, uint32_t world);
int bzx_shard_scan_runs(bzx_ctx *ctx, const void *d_raw, size_t len, uint32_t rank, uint32_t world, long long *d_tiles);
int bzx_shard_scan_counts(bzx_ctx *ctx, const void *d_raw, size_t len, uint32_t rank, uint32_t world, long long *d_tiles);
int bzx_shard_prepare_scanned(bzx_ctx *ctx, const void *d_raw, size_t len, int level, uint32_t rank, uint32_t world,
                              long long *d_tiles, uint32_t *nblk_total, long long *d_bits, size_t bits_cap);
int bzx_shard_emit_packed(bzx_ctx *ctx, const long long *d_bits_all, void *d_packed, size_t cap, size_t *packed_len,
                          size_t *stream_len);
/* After bzx_shard_emit_packed: bytes of the longest packed buffer of any rank -- the common length a gather needs --
 * computed from the sizes every rank already holds: no further collective, no extra host round trip (world <= 64). */
int bzx_shard_packed_max(bzx_ctx *ctx, size_t *max_len);
int bzx_shard_assemble_begin(bzx_ctx *ctx, void *d_out, size_t cap, size_t *stream_len);
int bzx_shard_assemble_rank(bzx_ctx *ctx, const void *d_packed_r, uint32_t r, void *d_out);
/* bzx_shard_assemble_* only enqueue work on the context's stream; wait for it here (or on the caller's stream). */
int bzx_ctx_sync(bzx_ctx *ctx);

/*
 * Streaming forms.  The reference reads its input incrementally (RLE1Block::new(source: R, ...), rle1.rs:49-85;
 * Iterator::next :245-263) and overlaps production, compression and an ordered writer (compress.rs:66-132,
 * bitwriter.rs:77-132).  Block boundaries depend on everything before them, so a chunked caller
 * cannot split chunks independently; these entry points keep the state between calls.
 *
 * bzx_split_rle1_chunk: RLE1Block over a source that arrives in pieces.  Returns the blocks that are complete with
 * the bytes seen so far (layout as bzx_split_rle1); the last, unfinished block is withheld inside the context (its
 * pending run and partial block) and comes out of a later call or of the call with final != 0.  One stream per
 * context at a time.
 */
int bzx_split_rle1_chunk(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, int final, uint8_t *blocks_out,
                         uint32_t nblk_cap, uint32_t *ns, uint32_t *crcs, uint32_t *nblk_out);

/*
 * bzx_cstream_*: whole-stream compressor for host buffers fed in chunks of at most max_chunk bytes (0 = 256 MiB);
 * device memory is bounded by the chunk size, not by the input.  Copy of chunk k+1 to the device, compression of
 * chunk k and copy-back of chunk k-1 overlap (three HIP streams, double buffers); pass page-locked buffers
 * (bzx_host_alloc, or memory the caller registered with HIP) for truly asynchronous copies.
 *   feed: consumes raw[0..len); `out`/`cap` is the WHOLE output buffer, the same on every call; *produced = bytes
 *   of it that are final so far (a caller may write out[flushed..*produced) to its file after every call).
 *   The call with final != 0 (len may be 0) completes the stream: *produced = length of the .bz2.  feed after it:
 *   BZX_E_STATE.  BZX_E_PARAM (a NULL pointer, len > max_chunk, cap < 16) leaves the stream as it was.
 *   BZX_E_OUTBUF: `out` cannot hold the stream (bzx_compress_buffer: bytes needed so far in *out_len, a lower bound
 *   while chunks remain).  An error is sticky for the stream object: later feed calls return it again;
 *   bzx_cstream_end is still required and the bzx_ctx stays usable for the next stream.
 * bzx_compress_buffer is this over a whole buffer; its stream object is kept in the context and started anew by every
 * call, also after an error.
 */
typedef struct bzx_cstream bzx_cstream;
int bzx_cstream_begin(bzx_ctx *ctx, int level, size_t max_chunk, bzx_cstream **out);
int bzx_cstream_feed(bzx_cstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap,
                     size_t *produced);
void bzx_cstream_end(bzx_cstream *s);
void *bzx_host_alloc(size_t bytes);     /* page-locked host memory (NULL on failure) */
void bzx_host_free(void *p);

/*
 * Decompression on the device (replaces decompress(), decompress.rs:38-404 minus file I/O; bwt_decode
 * bwt_sort.rs:91-130, rle2_mtf_decode_fast rle2_mtf.rs:191-287, rle1_decode rle1.rs:267-316): one .bz2 stream ->
 * raw bytes; every block CRC and the combined CRC are verified (a mismatch is BZX_E_DATA, unlike the reference, which
 * logs it and continues, decompress.rs:379-386).  The blocks of the input are decoded side by side.
 * _device: d_bz2 / d_out are DEVICE pointers (d_out 16-byte aligned); _buffer: host pointers.
 * _device decodes ONE stream: bytes after its end-of-stream marker are ignored unless they begin another stream
 * ("BZh1".."BZh9" with at least 14 bytes left), which is refused with BZX_E_DATA "another bzip2 stream follows the
 * first ..." (a concatenated .bz2 is not decoded in part); a fault of the first stream itself -- damage, a CRC, an
 * output too small -- is reported in preference.  _buffer decodes every stream of a concatenated .bz2; bytes after
 * the last one that do not begin a stream are ignored.
 * Both are bzx_decompress_batch_* with count = 1 (below) and share its rules:
 *   BZX_E_OUTBUF: *out_len = the exact decoded size of the whole input (all streams of it), nothing is written.
 *   BZX_E_DATA: *out_len = 0 and out is not written by _buffer, wherever in the input the damage lies (_device may
 *   have written d_out).  A damaged block CRC is named "block CRC mismatch in block N", N counted over the input.
 *   No fixed limit on the block-magic candidates of an input (chance matches of the magic in compressed data).
 *   Memory: the context grows to one block slab (about 28 MB) per block-magic candidate of the whole input, not of
 *   its longest stream; bzx_dstream_* decodes in bounded device memory.  An allocation that fails is BZX_E_NOMEM and
 *   the context stays usable.  _buffer holds the input and cap bytes of output on the device for the call and leaves
 *   no page-locked memory of their size behind.
 *   bzx_get_stats afterwards: nblk and raw_bytes, summed over the streams; the other fields keep what the last
 *   compression left.  bzx_get_block_info returns BZX_E_STATE.
 * Accepted streams are those libbz2 1.0.8 accepts -- 2..6 tables, 1..32767 selectors (the first 18002 are used),
 * code lengths 1..20, incomplete prefix codes, RLE1 count bytes 0..255, blocks of up to 100000 * level bytes --
 * with ONE exception: a block whose randomised bit is set (written by bzip2 0.9.0 and older; never by bzip2 >= 0.9.5
 * nor by the reference) is refused with BZX_E_DATA and the error text "randomised block ...", where libbz2 decodes it.
 */
int bzx_decompress_device(bzx_ctx *ctx, const void *d_bz2, size_t len, void *d_out, size_t cap, size_t *out_len);
int bzx_decompress_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint8_t *out, size_t cap, size_t *out_len);

/*
 * Batched decompression: count independent .bz2 inputs decoded in one call, the counterpart of
 * bzx_compress_batch_*.  Input i is a .bz2 file: one stream or several concatenated.
 * The rule: given enough room, output i and status[i] are what bzx_decompress_buffer returns for input i alone -- the
 * same bytes and BZX_OK, or BZX_E_DATA -- with its edge rules: an input shorter than 14 bytes or without a BZh1..9
 * header is refused; bytes after a stream that do not begin another stream are ignored; a "BZh<d>" after a stream
 * that does not decode refuses the input; randomised blocks, blocks longer than 100000 * level, selectors outside
 * 1..32767 are refused.
 * Independence: an input's status and bytes do not depend on its neighbours, in the call or in memory; nothing
 * outside [srcs[i], srcs[i] + src_lens[i]) is read.
 * Pointers: d_srcs and d_outs are HOST arrays of count DEVICE pointers.  Inputs may have any alignment; outputs must
 * be 16-byte aligned (as for bzx_decompress_device).  An output may be NULL where caps[i] == 0.
 * Output too small (per input): if the decoded size of input i exceeds caps[i], status[i] = BZX_E_OUTBUF,
 * out_lens[i] = the exact size needed, outs[i] is not written and the input's block CRCs are not checked.  Damage
 * found before the size is known is BZX_E_DATA.  After BZX_OK out_lens[i] is the decoded length, after BZX_E_DATA 0.
 * Returns BZX_OK when every status[i] is BZX_OK; otherwise status[k] for the lowest failing k, and bzx_last_error
 * names input k and the reason.  Errors of the whole call -- BZX_E_PARAM (NULL arrays, a misaligned output, a NULL
 * output with caps[i] > 0), BZX_E_NOMEM, BZX_E_HIP -- are returned as themselves and every status[i] is set to that
 * code.  count == 0 returns BZX_OK.  After any error the context stays usable.
 * Rounds: the inputs run in device rounds of whole inputs with at most R blocks each, R = the larger of the block
 * slabs the context holds and the block count of the largest input (block-magic candidates, chance matches
 * included).  A call costs one host synchronisation after the magic scan (a second one only if the candidate table
 * overflows, which takes chance matches of the magic) and two per round; none per input or stream.
 * _buffer stages the inputs on the device in groups of at most 256 MiB of compressed bytes (or one larger input),
 * and each round's outputs packed in a device area bounded by the round's decoded bytes (per input, the smaller of
 * caps[i] and 259/5 of its inverse-BWT output), not by the sum of caps; one copy per round brings them back.
 * bzx_get_stats after a batch call: nblk (blocks decoded), raw_bytes (decoded bytes) and ms_total;
 * bzx_get_block_info returns BZX_E_STATE.
 */
int bzx_decompress_batch_device(bzx_ctx *ctx, uint32_t count, const void *const *d_srcs, const size_t *src_lens,
                                void *const *d_outs, const size_t *caps, size_t *out_lens, int *status);
int bzx_decompress_batch_buffer(bzx_ctx *ctx, uint32_t count, const uint8_t *const *srcs, const size_t *src_lens,
                                uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);

/*
 * bzx_dstream_*: streaming decompression, the counterpart of bzx_cstream_* (replaces decompress()'s reader loop,
 * decompress.rs:38-404): the .bz2 arrives in pieces of any size, the decoded bytes leave in pieces of any size, and the
 * device memory is fixed at bzx_dstream_begin.  Shaped like the inflate loop of libbz2 / zlib, because the output of
 * a piece of input is unbounded (a few hundred bytes of .bz2 decode to hundreds of megabytes of zeros).
 *   feed: takes bz2[0, len), accepts *consumed <= len bytes of it and writes *produced <= cap decoded bytes to out;
 *   the caller presents the unconsumed rest again.  final != 0: no bytes follow those presented.  *done becomes 1
 *   once everything is decoded, verified and delivered.  A call with len >= 1 and cap >= 1 (or final) makes progress:
 *   it consumes input, or produces output, or sets *done.  len == 0 without final does nothing and returns BZX_OK.
 *   feed may only buffer: accepted bytes are copied to the device at once, but a window is decoded when max_chunk
 *   bytes have been accepted or at final, so one-byte feeds cost a copy each and not a launch each.
 * The rule: for any way of cutting the input into feed calls and any sequence of cap values, the concatenated output
 * and the final status are what bzx_decompress_buffer returns for the whole input with enough room -- the same bytes
 * and BZX_OK, or BZX_E_DATA -- with its edge rules: every stream of a concatenated .bz2 is decoded; bytes after a
 * stream that do not begin another stream ("BZh1".."BZh9" with at least 14 bytes left) are ignored -- the decision
 * waits until 14 bytes or final have arrived, and once it has fallen *done can be set before final; a "BZh<d>" after
 * a stream that does not decode refuses the input; randomised blocks, blocks longer than 100000 x level and selector
 * counts outside 1..32767 are refused; the end of the input inside a header, block or footer is BZX_E_DATA.  (One
 * difference: a block image longer than 2,400,000 bytes -- no coder writes one: 18,002 groups of 50 symbols of 20
 * bits are 2,250,250 -- is refused as damaged.)
 * Only verified bytes leave: a block's bytes are delivered after its CRC matched.  After BZX_E_DATA the bytes
 * delivered so far are a prefix of the true output made of whole verified blocks (what bzip2 -dc shows of a damaged
 * file); a call that returns an error has produced nothing.  The error is sticky: later feed calls return it again;
 * bzx_dstream_end is still required, and the context stays usable.  feed after *done is BZX_E_STATE.
 * Between begin and end the block slabs of the context belong to the stream (decoded blocks wait in them from one
 * feed to the next): a second bzx_dstream_begin and every other compute entry point of that context return
 * BZX_E_STATE (bzx_last_error says why) and leave the stream intact.
 * Memory: two device input buffers of max_chunk + 2.4 MB, two device and two page-locked output staging areas of
 * 48 MiB (a block expands to at most 259/5 x 900,000 = 46.62 MB), tables sized by max_chunk, and the R block slabs
 * the context holds at begin (at least the max_blocks of bzx_ctx_create; about 28 MB each).  Nothing grows with the
 * length of the input, the number of its blocks or streams, or its expansion ratio.  max_chunk: 0 = 128 MiB; values
 * below 16 bytes are raised to 16 (the withheld tail has room of its own; a small chunk only costs launches).
 * A window (the undecoded tail of the last one plus the accepted bytes) is decoded in rounds of at most R blocks; a
 * round whose output exceeds a staging area leaves in several passes.
 * Overlap: accepted bytes travel to the device beside the kernels of the window before, and a round's output travels
 * back beside the kernels of the next round (three HIP streams).  Pass page-locked memory (bzx_host_alloc) as bz2
 * for truly asynchronous copies; feed returns after the bytes it accepted have left the caller's buffer.
 * bzx_get_stats after *done: nblk, raw_bytes and ms_total (device time of the rounds), as after a batch call.
 */
typedef struct bzx_dstream bzx_dstream;
typedef struct {
    uint64_t in_bytes;          /* bytes accepted */
    uint64_t out_bytes;         /* bytes delivered */
    uint32_t nblk;              /* blocks verified */
    uint32_t nstreams;          /* streams finished (end-of-stream marker seen, combined CRC matched) */
    uint32_t slabs;             /* block slabs of the context (R) */
    uint32_t windows;           /* windows scanned */
    uint32_t rounds;            /* output passes: one host synchronisation each */
    uint32_t scans;             /* magic scans: one host synchronisation each */
    uint64_t device_bytes;      /* device memory of the stream object (without the context's slabs) */
    uint64_t pinned_bytes;      /* page-locked host memory of the stream object */
} bzx_dstream_info;
int bzx_dstream_begin(bzx_ctx *ctx, size_t max_chunk, bzx_dstream **out);
int bzx_dstream_feed(bzx_dstream *s, const uint8_t *bz2, size_t len, int final, size_t *consumed, uint8_t *out,
                     size_t cap, size_t *produced, int *done);
void bzx_dstream_end(bzx_dstream *s);
int bzx_dstream_get_info(const bzx_dstream *s, bzx_dstream_info *out);

/*
 * Block index and random access: "bytes [off, off + want) of what this .bz2 decodes to" without decoding what lies
 * before them.  bzip2 blocks are independent and start at any bit; an index entry says where a block starts, what it
 * decodes to and where that lies in the output.
 *
 * bzx_index_*: one entry per VERIFIED block of the input, in input order, over all streams of a concatenated .bz2.
 * It is the streaming decoder's state machine (scan, chain, rounds, passes; bzx_dstream_* above) with nothing copied
 * back: every block is decoded, expanded on the device and its CRC compared, and an entry exists only for a block whose
 * CRC matched.  Same edge rules: concatenated streams are followed, trailing bytes that begin no stream are ignored,
 * randomised blocks and blocks longer than 100000 x level are refused; an empty stream adds no entry and counts in
 * nstreams.  A damaged input gives BZX_E_DATA with the texts of bzx_dstream_feed; bzx_index_get then still returns the
 * entries of the verified prefix.  Device memory as for bzx_dstream_* (one output staging area instead of two, no
 * page-locked staging); between begin and end the context is busy as with an open bzx_dstream.
 *   feed: as bzx_dstream_feed without the output; *done = 1 once the last stream has been verified (bytes fed after
 *   that are counted in in_bytes and ignored).
 *   get: entries and totals so far; the pointer is valid until the next feed or bzx_index_end.
 *   bzx_index_build_buffer: begin, a loop over feed, end.  More blocks than cap_entries: BZX_E_OUTBUF with info->nblk =
 *   entries needed (the first cap_entries are written).  After BZX_E_DATA entries and info describe the verified prefix.
 *
 * Stored form (bzx --index writes FILE.bz2.bzxi), little-endian: a 64-byte header -- bytes 0..3 "BZXI", 4..7 version
 * (1), 8..15 in_bytes, 16..23 out_bytes, 24..31 nblk, 32..35 nstreams, 36..63 zero -- followed by nblk entries of 40
 * bytes laid out as the struct below.
 */
typedef struct {
    uint64_t bit;        /* bit offset of the block magic from the start of the input */
    uint64_t out_off;    /* decoded bytes of the whole input before this block */
    uint32_t out_len;    /* decoded bytes of this block (at most 259/5 x 900,000) */
    uint32_t crc;        /* stored block CRC */
    uint32_t img_bits;   /* bits from the magic to the bit after the block's last symbol */
    uint32_t stream;     /* ordinal of the stream the block belongs to */
    uint8_t level;       /* 1..9 of that stream */
    uint8_t reserved[7];
} bzx_index_entry;       /* 40 bytes, little-endian when stored */
typedef struct { uint64_t in_bytes, out_bytes; uint64_t nblk; uint32_t nstreams, reserved; } bzx_index_info;
typedef struct bzx_index bzx_index;
int bzx_index_begin(bzx_ctx *ctx, size_t max_chunk, bzx_index **out);
int bzx_index_feed(bzx_index *ix, const uint8_t *bz2, size_t len, int final, size_t *consumed, int *done);
int bzx_index_get(const bzx_index *ix, const bzx_index_entry **entries, bzx_index_info *info);
void bzx_index_end(bzx_index *ix);
int bzx_index_build_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, bzx_index_entry *entries, uint64_t cap_entries,
                           bzx_index_info *info);
/*
 * Salvage: the index of every intact block of a DAMAGED .bz2 (the counterpart of bzip2recover), and the gaps between
 * them.  A salvage index is an ordinary entry list: bzx_index_span, bzx_decompress_range_* and _ranges_* read through it
 * unchanged, and hold every block against its entry again before a byte leaves.  Damage is the expected case: these
 * calls return BZX_OK whatever the data (an empty input: 0 entries); BZX_E_PARAM / _STATE / _NOMEM / _HIP keep their
 * meaning, BZX_E_OUTBUF says that cap_entries, cap_gaps or cap is too small (the counts, or *out_len, then hold what is
 * needed and the first cap items are written).
 *
 * A block magic at bit b VERIFIES when the block decoded from b keeps its reader inside the input, has no structural
 * error, has its randomised bit clear, is no longer than 100000 x level, passes the inverse BWT and expands to bytes
 * whose CRC is the stored one: the checks of a block of bzx_index_*.
 *
 * The walk keeps a position P, a level, a count of end-of-stream markers and at most one open gap:
 *   start     "BZh1".."BZh9" at byte 0: level = the digit, P = 32.  Otherwise level = 9, P = 0 and a gap opens at bit 0
 *             with HEADER (a stream is assumed).
 *   magics    at bits >= P, in ascending order; those below P lie inside an accepted block or a footer and are ignored.
 *   verifies  an open gap closes at b; with none open and b > P the gap [P, b) is recorded (NO_MAGIC, and HEADER when the
 *             walk was between streams).  The block becomes an entry (bit = b, out_off = the running sum, stream = markers
 *             passed, level = the walk's; a block accepted between streams assumes a stream).  P = b + img_bits.
 *   does not  a gap opens at P unless one is open (with HEADER when the walk is between streams), takes the reason into
 *             `why` and counts the candidate.  P stays: the end of a block that did not verify is not trusted -- a
 *             damaged payload usually still decodes, to an end several blocks further on -- so every candidate behind it is
 *             tried as well, and the only test by position is "behind the last ACCEPTED block".
 *   marker    an end-of-stream magic at b whose 80 bits lie inside the input: an open gap closes at b, or [P, b) is
 *             recorded as above.  If the stream's header was read and no gap was opened or recorded since, the stored
 *             combined CRC is held against the fold of the stream's entries; a mismatch records the zero-length gap
 *             {b, b, COMBINED_CRC}.  The marker count and nstreams go up, P = the next byte boundary behind the footer.
 *             "BZh1".."BZh9" there with at least 14 bytes left: level = the digit, P += 32.  Otherwise level = 9 and the
 *             walk is between streams (trailing bytes without a magic are no gap).  A marker cut off by the end of the
 *             input counts as not there.
 *   end       at `final` an open gap closes at 8 x in_bytes and gains TRUNCATED when the walk is inside a stream; with
 *             none open and the walk inside a stream the gap [P, end) is recorded with TRUNCATED, also when it is empty.
 * Decisions this leaves open: an input without a header (an empty one included) is inside an assumed stream, so it ends
 * in a gap with HEADER | TRUNCATED; a block longer than its level allows counts as STRUCTURE even when its CRC matches;
 * a failed candidate between streams does not assume a stream (no TRUNCATED at the end).  An entry whose image ends
 * within 8 bytes of the end of a truncated input needs those bytes for a range read (bzx_index_span: byte_hi): give the
 * range reader the input followed by 8 zero bytes; bzx_salvage_buffer and bzx --recover do (over a copy of the input from
 * the first such block on: a few blocks at most).
 * On an undamaged input entries and info are bzx_index_build_buffer's, field for field, and there is no gap.
 *
 * bzx_salvage_begin: a third mode of the bzx_dstream_* machine; feed / get / end are bzx_index_feed / _get / _end.
 * *done becomes 1 only at `final`: the walk goes on looking behind an end-of-stream marker.  Device memory is fixed at
 * begin: that of bzx_index_begin, plus per-round tables of the candidates' classes, the trials' verdicts, entries and
 * gaps (a few dozen bytes per slab).  Host synchronisations: one per scan, one per pass, none per block, candidate or
 * gap.  Every candidate of a round that decodes is a trial: inverse BWT, expansion into the staging area, CRC; the walk
 * runs on the device behind the CRCs and reads the footer CRC and the next header there.  Only the gap list on the host
 * grows with the damage.
 * bzx_salvage_buffer: a salvage index, then bzx_decompress_range_buffer(.., 0, out_bytes, ..) over it: the good blocks
 * are decoded a second time, and the bytes leave through the range reader's checks.  Delivering bytes in the salvage pass
 * itself is deliberately not built.
 */
#define BZX_GAP_STRUCTURE    1u   /* a block magic in the gap starts a block that does not decode (damage, longer than its
                                     level allows, inverse BWT refused, reader passes the end of the input) */
#define BZX_GAP_BLOCK_CRC    2u   /* ... a block that decodes, whose computed CRC is not the stored one */
#define BZX_GAP_RANDOMISED   4u   /* ... a block with the randomised bit set (refused as everywhere in this library) */
#define BZX_GAP_NO_MAGIC     8u   /* neither a block nor an end-of-stream marker where the stream continues */
#define BZX_GAP_TRUNCATED   16u   /* the input ends inside a stream */
#define BZX_GAP_COMBINED_CRC 32u  /* zero-length gap at an end-of-stream marker: stored combined CRC != the blocks' */
#define BZX_GAP_HEADER      64u   /* no readable "BZh1".."BZh9" where a stream starts */
typedef struct { uint64_t bit_lo, bit_hi;   /* input bits [lo, hi) that no entry, header or footer accounts for */
                 uint64_t out_off;          /* salvaged bytes before the gap (where bytes are missing) */
                 uint32_t candidates;       /* block magics inside it that did not verify */
                 uint32_t why; } bzx_gap;   /* 32 bytes */
int bzx_salvage_begin(bzx_ctx *ctx, size_t max_chunk, bzx_index **out);   /* feed/get/end: bzx_index_feed/_get/_end */
int bzx_index_get_gaps(const bzx_index *ix, const bzx_gap **gaps, uint64_t *ngaps);   /* 0 gaps on a plain index */
int bzx_salvage_build_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, bzx_index_entry *entries, uint64_t cap_entries,
                             bzx_index_info *info, bzx_gap *gaps, uint64_t cap_gaps, uint64_t *ngaps);
int bzx_salvage_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint8_t *out, size_t cap, size_t *out_len,
                       bzx_gap *gaps, uint64_t cap_gaps, uint64_t *ngaps);
/*
 * The index straight from compression: with keeping switched on, a compression call leaves the index of the stream it
 * wrote, so the first range read needs no decode pass over the library's own output.
 * The rule: after a successful call of an entry point named below, the entries and the bzx_index_info are identical,
 * field for field and byte for byte (memcmp of the 40-byte entries, reserved zero), to what bzx_index_build_buffer returns
 * for the stream the call produced.  An empty input gives 0 entries and info = {in_bytes 14, out_bytes 0, nblk 0,
 * nstreams 1}.  The compressed bytes do not change: they stay byte-identical to libbz2.
 * Where a field comes from: bit = 32 + the sizes of the blocks before it; img_bits = the block's size; crc = its CRC;
 * out_len = the raw bytes the block splitter gave it, out_off their running sum; stream 0; level = the call's level.
 *   bzx_ctx_keep_index / bzx_mctx_keep_index: on != 0 switches keeping on.  The default is off, and off means off: no
 *   compression path gains a kernel launch, a copy, a host synchronisation or a host allocation.  _mctx_ applies to every
 *   entry's private context.  BZX_E_STATE while a bzx_cstream (bzx_mstream) of the caller is open on the object.
 *   Switching, either way, drops the index a get call would have returned.
 *   bzx_compress_get_index: the index of the last bzx_compress_device or bzx_compress_buffer call on the context; the
 *   pointer stays valid until the next of these two calls or bzx_ctx_destroy.  BZX_E_STATE when keeping is off, when no
 *   such call has happened or when the last one failed; BZX_E_PARAM for NULL arguments.  No other entry point disturbs
 *   it: not decompression, not range reads, and not the batch and stream compressors, which keep an index of their own.
 *   bzx_mctx_get_index: the same after bzx_mcompress_buffer.
 *   bzx_cstream_get_index / bzx_mstream_get_index: the entries of the blocks accounted for so far; the copy-back runs
 *   one chunk behind the feed, and the unfinished last block of a chunk appears with the chunk that finishes it.
 *   Mid-stream every entry returned is final and the list only grows: an earlier result is a prefix of every later one.
 *   info->nblk and info->out_bytes describe those entries; info->in_bytes and info->nstreams are 0 until the final
 *   feed has succeeded, then the stream length and 1.  Valid until the next feed or _end.  BZX_E_STATE when keeping was
 *   off at _begin, or after a feed that failed.
 *   bzx_compress_batch_get_index: after bzx_compress_batch_device / _buffer.  Stream i's entries are
 *   entries[first[i] .. first[i + 1]); first has *count + 1 values.  bit counts from the start of stream i, out_off from
 *   the start of input i and stream is 0: the slice is the index of stream i on its own, what
 *   bzx_index_build_buffer(out + out_offs[i], out_lens[i]) returns.  An empty input has an empty slice.  One small
 *   kernel and one copy per device round build it (bzx_bt_index_kernel); the host synchronisations of the call stay:
 *   one for the counts, one per round, one at the end.  Valid until the next batch call on the context.
 * Host memory with keeping on: 40 bytes per block, held in the stream object, the context or the batch call's vector
 * (the stream compressors already require the whole output buffer, so this is no new kind of growth).
 * Not covered: bzx_compress_block(s) -- the caller supplies RLE1'd blocks, so the library never sees raw lengths -- and
 * the bzx_shard_* family -- one process per GPU, so no one place sees all blocks.
 */
struct bzx_mctx;
struct bzx_mstream;        /* (bzx_mctx_* / bzx_mstream_*: below) */
int bzx_ctx_keep_index(bzx_ctx *ctx, int on);
int bzx_mctx_keep_index(struct bzx_mctx *m, int on);
int bzx_compress_get_index(const bzx_ctx *ctx, const bzx_index_entry **entries, bzx_index_info *info);
int bzx_cstream_get_index(const bzx_cstream *s, const bzx_index_entry **entries, bzx_index_info *info);
int bzx_mctx_get_index(const struct bzx_mctx *m, const bzx_index_entry **entries, bzx_index_info *info);
int bzx_mstream_get_index(const struct bzx_mstream *s, const bzx_index_entry **entries, bzx_index_info *info);
int bzx_compress_batch_get_index(const bzx_ctx *ctx, const bzx_index_entry **entries, const uint64_t **first,
                                 uint32_t *count);
/*
 * bzx_index_span (host only, no context): which entries and which input bytes the range [off, off + want) needs:
 * entries [*first, *first + *count) and input bytes [*byte_lo, *byte_hi) -- from the byte that holds the first block's
 * magic to the last block's img_bits, rounded up to a byte, + 8 (inside the file: a block is followed by ten bytes of
 * end-of-stream marker and CRC at least).  The range is clipped at the end of the output; an empty one gives
 * *count = 0.  BZX_E_PARAM: NULL pointers, or entries that are not in output order.
 *
 * bzx_decompress_range_device / _buffer.  The rule: out[0, *got) equals bytes [off, off + want) of what
 * bzx_decompress_buffer returns for the whole input, clipped at its end (off >= out_bytes or want == 0: *got = 0,
 * BZX_OK).  bz2[0, len) holds input bytes [base, base + len): the whole file (base 0) or just the span;
 * BZX_E_PARAM when it does not cover the span.  No magic scan: the covering entries say where the blocks are.
 * Every touched block is decoded in full, and before a byte leaves its expanded length is held against out_len and its
 * computed CRC against the CRC stored in the block and against entry.crc.  BZX_E_DATA with "index does not match the
 * input: ..." (no block magic at `bit`, another stored CRC, another decoded length or block size), the damaged-block
 * or the "block CRC mismatch in block N" text otherwise (N: the entry's number); *got = 0, and _buffer has not
 * written out (_device may have written d_out).  When several blocks fail, the text is that of the lowest-numbered one;
 * an entry of a corrupt index whose bytes lie outside bz2[0, len) (_buffer: outside the span) reads as zeros: BZX_E_DATA,
 * "no block magic at bit ...", and that text comes first.  The call is count = 1 of the many-range call below over one
 * piece, by the same code: blocks wholly inside the range expand at their final place in d_out, the at most two edge
 * blocks into a device staging pool of 2 x 259/5 x 900,000 bytes, from which one launch of bzx_rg_gather_kernel per
 * round puts the slices in place; _buffer uploads the span only and brings back one slice.  A range of more blocks than
 * the context holds slabs runs in rounds of that many blocks, one host synchronisation each; the round that holds the
 * first failing block is the last.  Device memory: the span and at most `want` bytes of output (_buffer: two buffers of
 * 4 MiB at least that the context keeps and grows, so a small read allocates nothing), the pool and a slice table of
 * 96 KiB (kept by the context from the first call on) and the context's slabs (a context holds 16 at
 * least from bzx_ctx_create on, about 450 MB, whatever max_blocks said; a range read never adds to them);
 * nothing depends on the length of the file.  d_bz2 and d_out may have any alignment.  The inverse BWT of these calls
 * is the many-lane walk (one workgroup per block; bzx_stage_ibwt below), since one to three blocks have nothing to hide
 * a one-lane pointer chase behind.  bzx_get_stats afterwards: nblk (blocks decoded) and raw_bytes (*got).
 */
int bzx_index_span(const bzx_index_entry *e, uint64_t n, uint64_t off, uint64_t want, uint64_t *first, uint64_t *count,
                   uint64_t *byte_lo, uint64_t *byte_hi);
int bzx_decompress_range_device(bzx_ctx *ctx, const void *d_bz2, size_t len, uint64_t base, const bzx_index_entry *e,
                                uint64_t n, uint64_t off, uint64_t want, void *d_out, size_t *got);
int bzx_decompress_range_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint64_t base, const bzx_index_entry *e,
                                uint64_t n, uint64_t off, uint64_t want, uint8_t *out, size_t *got);
/*
 * Many ranges in one call.  bzx_decompress_ranges_device / _buffer.  The rule: given room, range i leaves
 * out[out_offs[i], out_offs[i] + gots[i]) equal to what bzx_decompress_range_buffer(..., offs[i], wants[i], ...) returns
 * for that range alone, and status[i] is that call's BZX_OK or BZX_E_DATA.  The ranges may come in any order, overlap,
 * repeat, be empty or lie beyond the end (gots[i] = 0, BZX_OK).  The output is packed: out_offs[i] is the running sum of
 * the clipped lengths, computed from the index before any device work, and *need is that sum; *need > cap: BZX_E_OUTBUF,
 * nothing is touched.  Every distinct touched block is decoded ONCE however many ranges want bytes of it.
 *   The input comes in pieces: pieces[j].p holds input bytes [base, base + len), ascending and disjoint; one piece
 *   {p, 0, file length} is the whole file.  Every touched block's bytes [bit / 8, (bit + img_bits + 7) / 8 + 8) must lie
 *   inside ONE piece.  bzx_index_spans (host only, no context) names the pieces a list of ranges needs: the union of these
 *   intervals over the touched blocks, overlapping or adjacent ones merged, gaps left as gaps (a caller may merge further:
 *   a superset is always accepted); more than cap_pieces: BZX_E_OUTBUF with *npieces = pieces needed.
 *   Independence, as in bzx_decompress_batch_*: a range's bytes and status depend on the blocks it touches and on nothing
 *   else.  A damaged block, or an entry that does not match, fails exactly the ranges that touch it: BZX_E_DATA, gots[i] =
 *   0; _buffer does not write that range's slot of out (it copies back maximal runs of consecutive good ranges: one copy
 *   when all are good), _device may have written it.  The call returns BZX_OK when every status is, otherwise status[k] of
 *   the lowest failing k, and bzx_last_error reads "range k: " and the single call's text.  Only verified bytes leave: the
 *   checks of the single call, by the same code.
 *   Errors of the whole call are returned and set into every status[i]: BZX_E_PARAM (NULL arrays with count > 0; pieces
 *   not ascending and disjoint; a touched block not inside one piece -- the text names the range and the bytes; entries
 *   not in output order), BZX_E_OUTBUF, BZX_E_NOMEM, BZX_E_HIP, BZX_E_STATE (an open bzx_dstream or bzx_index).  count = 0:
 *   BZX_OK.  After any error the context stays usable.
 *   Memory: a block that one range alone touches and wholly contains expands at its final place in d_out; every other
 *   block expands into the staging pool -- about 93 MB, room for the two edge blocks of one range, at 256-byte aligned
 *   offsets -- from which ONE launch per round of bzx_rg_gather_kernel puts the slices of the verified
 *   blocks in place.  A round takes blocks in ascending order until it holds as many as the context has slabs or the next
 *   pool block does not fit.  Nothing but small tables grows (the block tables, a slice table of 24 bytes per 64 KiB of
 *   slice).  _buffer uploads the pieces that hold a touched block, and nothing else, into the span buffer the context
 *   keeps, and decodes into its kept output buffer of *need bytes.  d_out and the piece pointers may have any alignment.
 *   Host synchronisations: one per round and one at the end; none per range, block or slice.
 *   bzx_get_stats afterwards: nblk = DISTINCT blocks decoded, raw_bytes = the sum of gots.
 */
typedef struct { const void *p; uint64_t base; uint64_t len; } bzx_piece;   /* input bytes [base, base + len) at p */
int bzx_index_spans(const bzx_index_entry *e, uint64_t n, uint32_t count, const uint64_t *offs, const uint64_t *wants,
                    uint64_t *bases, uint64_t *lens, uint32_t cap_pieces, uint32_t *npieces);
int bzx_decompress_ranges_device(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                 uint64_t n, uint32_t count, const uint64_t *offs, const uint64_t *wants, void *d_out,
                                 size_t cap, size_t *out_offs, size_t *gots, int *status, size_t *need);
int bzx_decompress_ranges_buffer(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                 uint64_t n, uint32_t count, const uint64_t *offs, const uint64_t *wants, uint8_t *out,
                                 size_t cap, size_t *out_offs, size_t *gots, int *status, size_t *need);
/*
 * The gather kernel alone, for the parity tests (host pointers): slice i copies src[src_offs[i], + lens[i]) to
 * out[dst_offs[i], + lens[i]) on the device, through the same cutting into 64 KiB table entries and the same kernel as
 * the range reads.  The device copy of `out` starts from the caller's bytes, so what lies outside the slices comes back
 * unchanged.  BZX_E_PARAM when a slice leaves either buffer.  _time: the same under HIP events, *ms_best = the best of
 * `reps` launches (for the probe).
 */
int bzx_stage_gather(bzx_ctx *ctx, const uint8_t *src, size_t src_len, uint32_t nslices, const uint64_t *src_offs,
                     const uint64_t *dst_offs, const uint64_t *lens, uint8_t *out, size_t out_len);
int bzx_stage_gather_time(bzx_ctx *ctx, const uint8_t *src, size_t src_len, uint32_t nslices, const uint64_t *src_offs,
                          const uint64_t *dst_offs, const uint64_t *lens, uint8_t *out, size_t out_len, uint32_t reps,
                          float *ms_best);
/*
 * Records: "records [a, a + c) of what this .bz2 decodes to" -- lines of a text or JSONL dump -- on top of the block index
 * and the range reads.
 * The rule.  D[0, N) is what bzx_decompress_buffer returns for the whole input; delim is one byte value, 0..255; T is the
 * number of bytes of D equal to delim.
 *   rec_start(0) = 0;  rec_start(r) = the position of the r-th delimiter + 1 for 1 <= r <= T;  rec_start(r) = N for r > T.
 *   Records [a, a + c) are the bytes [rec_start(a), rec_start(a + c)): terminating delimiters are included, record T is the
 *   unterminated tail and may be empty, a + c saturates at 2^64 - 1.
 *   The record table of an index of n entries is uint64_t rec_before[n + 1]: rec_before[k] = delimiters in
 *   D[0, entries[k].out_off), rec_before[n] = T.  An empty index has the table {0}.
 *
 * The table from the index pass.  bzx_index_count_records(ix, delim): between bzx_index_begin and the first
 * bzx_index_feed; BZX_E_STATE after a feed and on an object from bzx_salvage_begin (its entries come from the device
 * walk: salvage is not covered), BZX_E_PARAM for a delim outside 0..255.  Off is the default and off means off: the index
 * pass launches, copies, allocates and synchronises as it did.  On, a pass gains one launch (bzx_rec_count_kernel, behind
 * the block CRCs, over the expanded bytes of the blocks the pass placed) and one 32-bit word per block in the copy that
 * brings its entries back; it gains no synchronisation.  The tables for that are allocated by this call.
 * bzx_index_get_records: the table of the entries bzx_index_get returns now, *n = their number (the table has *n + 1
 * values); valid as long as bzx_index_get's pointer; BZX_E_STATE when counting was not switched on.  After BZX_E_DATA it
 * describes the verified prefix, as the entries do.
 * bzx_index_build_records_buffer: bzx_index_build_buffer with counting on; rec_before has room for cap_entries + 1 values
 * and receives the table of the entries written (after BZX_E_OUTBUF: of the first cap_entries).
 *
 * The table from the raw side, for a stream this library compressed: bzx_records_count_device / _buffer count delim in
 * raw[e[k].out_off, + out_len) for every entry (the same kernel over pointer-and-length segments, sums on the host).
 * BZX_E_PARAM unless the entries tile [0, len): out_off is the running sum of out_len and the last one ends at len.  For
 * the index a compression call kept (bzx_compress_get_index and its siblings) the result equals what
 * bzx_index_build_records_buffer returns for the stream that call wrote.  _buffer holds the raw bytes on the device for
 * the call.
 *
 * Planners (host only, no context).  bzx_records_span: the entry that holds the r-th delimiter -- the smallest k with
 * rec_before[k + 1] >= r, so blocks without a delimiter are stepped over -- and *j = r - rec_before[k], in 1..the block's
 * count.  r == 0: *entry = 0, *j = 0.  r > T: *entry = n, *j = 0.  BZX_E_PARAM: NULL, rec_before[0] != 0, a table that
 * descends.
 * bzx_records_pieces: the byte intervals of the file that locating and reading the record ranges [rec_los[i], +
 * rec_cnts[i]) need, as bzx_index_spans names them for byte ranges: per range the entries from the one that holds
 * delimiter lo (entry 0 for lo == 0) to the one that holds delimiter lo + cnt, clipped to the index -- none when lo > T or
 * the range is [0, 0) -- each with its bytes [bit / 8, (bit + img_bits + 7) / 8 + 8), merged; BZX_E_OUTBUF with *npieces =
 * pieces needed.
 *
 * bzx_records_locate_device / _buffer: byte_offs[i] = rec_start(recs[i]).  The host resolves every query with
 * bzx_records_span; a query with j == 0 needs no device.  Every distinct touched block is decoded once, into the staging
 * pool of the range reads and through their checks against the entry, by the same code; then one launch per round of
 * bzx_rec_select_kernel answers all queries of the round: for (block, j) the position of the j-th delimiter and the
 * block's count.  A block whose count is not rec_before[k + 1] - rec_before[k] fails its queries: BZX_E_DATA, "record table
 * does not match the input: block K holds X delimiters, the table says Y".  A damaged block or a stale entry fails exactly
 * the queries that touch it, with the range reader's texts; status[i] is BZX_OK or BZX_E_DATA (byte_offs[i] = 0), the call
 * returns the status of the lowest failing query and bzx_last_error reads "query k: " and the text.  Errors of the whole
 * call (BZX_E_PARAM -- NULL arrays, pieces not ascending and disjoint, a touched block not inside one piece, a bad table
 * --, BZX_E_NOMEM, BZX_E_HIP, BZX_E_STATE) are set into every status.  Pieces as in bzx_decompress_ranges_*; _buffer
 * uploads the pieces that hold a touched block.  Rounds as there (as many blocks as the context has slabs, or as fit
 * the pool).  Host synchronisations: at most two per round (the blocks' verdicts, the answers), none per query.
 * Only decoded blocks are held against the table: a stale count in a block that no query decodes can select the wrong
 * records.  It can never select unverified bytes.
 *
 * bzx_decompress_records_device / _buffer.  The rule: range i leaves D[rec_start(lo_i), rec_start(lo_i + cnt_i)) at
 * out[out_offs[i], + gots[i]); the ranges may come in any order, overlap, repeat, be empty or lie beyond T.  One locate
 * call for all 2 x count boundaries, then one call of bzx_decompress_ranges_* with the byte ranges found: the output is
 * packed in list order, *need and BZX_E_OUTBUF as there.  A range whose boundary failed is BZX_E_DATA with gots[i] = 0;
 * the others are still delivered.  bzx_last_error reads "range k: " and the text.  At most 2^31 - 1 ranges.
 * Cost: the boundary blocks are decoded twice, once by the locate call and once by the ranges call, and _buffer uploads
 * the pieces twice -- the trade of bzx_salvage_buffer.  A fused pass with the layout on the device is deliberately not
 * built.
 */
int bzx_index_count_records(bzx_index *ix, int delim);
int bzx_index_get_records(const bzx_index *ix, const uint64_t **rec_before, uint64_t *n);
int bzx_index_build_records_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, int delim, bzx_index_entry *entries,
                                   uint64_t cap_entries, bzx_index_info *info, uint64_t *rec_before);
int bzx_records_count_device(bzx_ctx *ctx, const void *d_raw, size_t len, int delim, const bzx_index_entry *e, uint64_t n,
                             uint64_t *rec_before);
int bzx_records_count_buffer(bzx_ctx *ctx, const uint8_t *raw, size_t len, int delim, const bzx_index_entry *e, uint64_t n,
                             uint64_t *rec_before);
int bzx_records_span(const uint64_t *rec_before, uint64_t n, uint64_t r, uint64_t *entry, uint64_t *j);
int bzx_records_pieces(const bzx_index_entry *e, uint64_t n, const uint64_t *rec_before, uint32_t count,
                       const uint64_t *rec_los, const uint64_t *rec_cnts, uint64_t *bases, uint64_t *lens,
                       uint32_t cap_pieces, uint32_t *npieces);
int bzx_records_locate_device(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e, uint64_t n,
                              const uint64_t *rec_before, int delim, uint32_t count, const uint64_t *recs,
                              uint64_t *byte_offs, int *status);
int bzx_records_locate_buffer(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e, uint64_t n,
                              const uint64_t *rec_before, int delim, uint32_t count, const uint64_t *recs,
                              uint64_t *byte_offs, int *status);
int bzx_decompress_records_device(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                  uint64_t n, const uint64_t *rec_before, int delim, uint32_t count,
                                  const uint64_t *rec_los, const uint64_t *rec_cnts, void *d_out, size_t cap,
                                  size_t *out_offs, size_t *gots, int *status, size_t *need);
int bzx_decompress_records_buffer(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                  uint64_t n, const uint64_t *rec_before, int delim, uint32_t count,
                                  const uint64_t *rec_los, const uint64_t *rec_cnts, uint8_t *out, size_t cap,
                                  size_t *out_offs, size_t *gots, int *status, size_t *need);
/*
 * The two record kernels alone, for the parity tests (host pointers), over segments [seg_offs[i], + seg_lens[i]) of buf.
 * The device copy of buf starts on a 256-byte boundary, so seg_offs[i] mod 16 is the alignment the kernel sees.
 * _count: counts_out[i] = bytes of segment i equal to delim.  _select: pos_out[i] = the position, relative to the
 * segment, of its js[i]-th delimiter (counted from 1), UINT32_MAX when js[i] is 0 or above the count; cnt_out[i] = the
 * segment's count either way.  BZX_E_PARAM when a segment leaves buf or is 2^32 bytes or longer.
 */
int bzx_stage_rec_count(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                        const uint64_t *seg_lens, int delim, uint32_t *counts_out);
int bzx_stage_rec_select(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nq, const uint64_t *seg_offs,
                         const uint64_t *seg_lens, const uint32_t *js, int delim, uint32_t *pos_out, uint32_t *cnt_out);
/*
 * Find: "where does this byte string occur in what this .bz2 decodes to", answered by the index pass, which holds every
 * verified block expanded on the device anyway.  Offsets come back, not data; the index the same pass leaves reads the
 * surroundings of a hit (bzx_decompress_range_*, bzx_decompress_records_*).
 * The rule.  D[0, N) is what bzx_decompress_buffer returns for the whole input, all streams of a concatenated file;
 * pat[0, m) is 1..BZX_FIND_MAX_PATTERN bytes of any value.  A hit is a p with p + m <= N and D[p, p + m) == pat.  The hits
 * are all such p in ascending order, overlapping ones included ("aa" in "aaaa": 0, 1, 2); the borders of blocks, streams,
 * passes, rounds and windows do not exist for a hit.  total is their exact number; the list holds the first
 * min(total, max_hits) of them.  Only verified bytes count: after BZX_E_DATA list and total describe the verified prefix,
 * p + m <= the out_bytes of the entries bzx_index_get returns.
 *
 * bzx_index_find(ix, pat, m, max_hits): between bzx_index_begin and the first bzx_index_feed, as
 * bzx_index_count_records, and in any order with it on the same object; BZX_E_STATE after a feed and on an object from
 * bzx_salvage_begin, BZX_E_PARAM for NULL, m == 0 or m > BZX_FIND_MAX_PATTERN.  A second call replaces the pattern.  Off
 * is the default and off means off: the index pass launches, copies, allocates and synchronises as it did.  On, a pass
 * gains three launches behind its verdict (bzx_find.hip: count, scan, emit, over the verified bytes of its staging area) and,
 * in the copy that brings its entries back, its hit count, its first inline_hits hits and its first and last m - 1
 * verified bytes; a pass with at most inline_hits hits gains no synchronisation.  A pass with more launches emit again in
 * windows of window_hits hits -- one launch, one copy and one synchronisation each -- until the list holds max_hits;
 * beyond that hits are only counted.  A hit that straddles two passes is found on the host, in the carried last m - 1
 * verified bytes and the first ones of the new pass.  Device memory is allocated by this call and fixed; only the host
 * list grows, up to max_hits.
 * bzx_index_get_hits: what has been found so far -- a hit becomes visible with the pass that verifies its last byte, and
 * mid-stream an earlier result is a prefix of every later one; the pointer is valid as long as bzx_index_get's;
 * BZX_E_STATE when find was not switched on.
 * bzx_find_buffer: begin, find with max_hits = cap_hits, a loop over feed, end.  hits has room for cap_hits values;
 * *nlisted of them are written, *total may be larger, which is no error.  entries / cap_entries / info as in
 * bzx_index_build_buffer, BZX_E_OUTBUF and BZX_E_DATA included (after BZX_E_DATA the hits, the entries and info describe
 * the verified prefix); entries may be NULL with cap_entries == 0: then the index is not returned and too many blocks is
 * no error.
 * bzx_find_geometry (no context, no device): how the kernels cut a run of bytes -- the tile of start positions one
 * workgroup takes, on 16-byte boundaries of the address (a wave takes a quarter of it in steps of 64 lanes x 16 bytes) --
 * and the two list sizes above.
 * bzx_stage_find: the three kernels alone, for the parity tests (host pointers), over segments [seg_offs[i], +
 * seg_lens[i]) of buf.  The device copy of buf starts on a 256-byte boundary, so seg_offs[i] mod 16 is the alignment the
 * kernels see.  Segment i is searched on its own -- a hit lies wholly inside it, whatever bytes of buf follow --
 * and counts_out[i] is its count.  The hits of all segments are numbered in segment order and ascending within a segment;
 * numbers [skip, skip + cap) are written to hits_out as positions relative to their segment, *nwritten of them.
 * BZX_E_PARAM when a segment leaves buf or is 2^32 bytes or longer, and for a pattern as above.
 */
#define BZX_FIND_MAX_PATTERN 256
int bzx_index_find(bzx_index *ix, const uint8_t *pat, size_t m, uint64_t max_hits);
int bzx_index_get_hits(const bzx_index *ix, const uint64_t **hits, uint64_t *nlisted, uint64_t *total);
int bzx_find_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, const uint8_t *pat, size_t m, uint64_t *hits,
                    uint64_t cap_hits, uint64_t *nlisted, uint64_t *total, bzx_index_entry *entries, uint64_t cap_entries,
                    bzx_index_info *info);
void bzx_find_geometry(uint32_t *tile_bytes, uint32_t *inline_hits, uint32_t *window_hits);
int bzx_stage_find(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                   const uint64_t *seg_lens, const uint8_t *pat, size_t m, uint64_t skip, uint32_t cap, uint32_t *counts_out,
                   uint64_t *hits_out, uint32_t *nwritten);
/*
 * Grep: "print the lines of this .bz2 that contain the string" -- the hits of find, the line number of every hit, counted
 * on the device in the pass that finds it, and the record reader for the lines themselves.
 * The rule.  D, N, delim as for the records above.  line(p) = the number of q < p with D[q] == delim: the record that
 * holds byte p, rec_start(line(p)) <= p < rec_start(line(p) + 1); a byte that is itself a delimiter belongs to the record
 * it ends.  For the list hits[0, nlisted) of bzx_index_get_hits, lines[i] = line(hits[i]): non-descending, and the borders
 * of blocks, streams, passes, rounds and windows do not exist for it.  A pattern may contain delim; the line is that of
 * the hit's first byte.  After BZX_E_DATA the list describes the hits of the verified prefix, as hits does.
 *
 * bzx_index_find_lines(ix, delim): after bzx_index_find and before the first bzx_index_feed, in any order with
 * bzx_index_count_records (whose delimiter is its own: the two are independent).  BZX_E_STATE without find, after a feed
 * and on an object from bzx_salvage_begin; BZX_E_PARAM for a delim outside 0..255.  Off is the default and off means off:
 * a find without lines launches, copies, allocates and synchronises as it did.  On, the pass launches the lines forms of
 * the three find kernels IN PLACE of the plain ones -- still three launches: they count the delimiters in the walk over
 * the bytes they read anyway -- and the one copy grows by a record of 4,104 bytes (the pass's delimiter total and the
 * line words of its inline_hits hits); a pass with at most inline_hits hits still gains no synchronisation; every
 * further window is still one emit launch and one synchronisation, now with two copies (hits, lines).  This call
 * allocates the sections' delimiter counts and the second window on the device and in page-locked memory.  The host
 * keeps the 64-bit delimiter total of the passes so far; a device hit's line is that plus the 32-bit count the emit kernel
 * left, a hit that straddles two passes gets its line on the host, from the carried bytes.
 * bzx_index_get_hit_lines: the lines of the hits bzx_index_get_hits returns now, the same *nlisted; valid as long as that
 * call's pointer; BZX_E_STATE when lines were not switched on.
 *
 * bzx_grep_buffer: ONE index pass over bz2 with find (max_hits), lines and bzx_index_count_records(delim) switched on;
 * the distinct values of lines[], ascending, are recs[0, *nrecs); then ONE call of bzx_decompress_records_buffer over the
 * index and record table of that same pass, one range {recs[i], 1} each, the whole input as one piece: record recs[i] --
 * D[rec_start(recs[i]), rec_start(recs[i] + 1)), its terminating delimiter included, the unterminated last record without
 * one -- lies at out[out_offs[i], + lens[i]), packed.  A record with several hits is listed once.
 *   Refusals: BZX_E_PARAM for a pattern that contains delim (no record can hold it), a delim outside 0..255 and what
 *   bzx_find_buffer refuses.  BZX_E_OUTBUF with *nrecs = the records needed when cap_recs is too small (recs, out_offs and
 *   lens have room for cap_recs values), BZX_E_OUTBUF with *need = the bytes needed when cap is too small; after either
 *   nothing has been written to out.
 *   Truncation: *total_hits is exact; *truncated = 1 when it exceeds max_hits, and then the records are those of the
 *   listed hits only.  The exact number of matching records beyond the list is deliberately not built.
 *   Damage: the matching records of the verified prefix are delivered, the last one cut at the prefix's end, and the call
 *   returns BZX_E_DATA with the pass's text.
 *   Cost: every block that holds a matching record is decoded twice, by the pass and by the record read, and the record
 *   read uploads those blocks again -- the trade of bzx_salvage_buffer and bzx_decompress_records_*.  Delivering the
 *   lines from the pass itself is not built.
 * bzx_stage_find_lines: bzx_stage_find over the lines forms.  dcounts_out[i] = the bytes of segment i equal to delim;
 * lines_out[k] = the delimiters of the hit's OWN segment in front of the hit (a neighbouring segment's bytes never
 * count), written for the same numbers as hits_out.
 */
int bzx_index_find_lines(bzx_index *ix, int delim);
int bzx_index_get_hit_lines(const bzx_index *ix, const uint64_t **lines, uint64_t *nlisted);
int bzx_grep_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, const uint8_t *pat, size_t m, int delim, uint64_t max_hits,
                    uint64_t *recs, uint64_t cap_recs, uint64_t *nrecs, uint8_t *out, size_t cap, size_t *out_offs, size_t *lens,
                    size_t *need, uint64_t *total_hits, int *truncated);
int bzx_stage_find_lines(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                         const uint64_t *seg_lens, const uint8_t *pat, size_t m, int delim, uint64_t skip, uint32_t cap,
                         uint32_t *counts_out, uint32_t *dcounts_out, uint64_t *hits_out, uint64_t *lines_out,
                         uint32_t *nwritten);
/*
 * The inverse BWT alone, for the parity tests (host pointers): L[0, n) and orig_ptr < n -> the RLE1 image img_out[0, n)
 * and its expansion raw_out (at most raw_cap bytes are written; *raw_len is the whole expanded length).  wide = 0 runs
 * the one-lane walk of the one-shot, batch and stream decoders, wide = 1 the many-lane walk of the range reads; both
 * leave the same image, checkpoints, length and *status (0x200: the image ends in four equal bytes, which libbz2
 * refuses) for ANY L, a BWT or not.
 */
int bzx_stage_ibwt(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, int wide, uint8_t *img_out,
                   uint8_t *raw_out, size_t raw_cap, uint64_t *raw_len, uint32_t *status);
/* For the probes: the kernels of either walk alone (scatter, pack, walk; the checkpoint pass of the many-lane one) over
 * `copies` copies of that block side by side, under HIP events; *ms_best = the best of `reps` launches.  The context
 * grows to `copies` slabs. */
int bzx_stage_ibwt_time(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, int wide, uint32_t copies,
                        uint32_t reps, float *ms_best);

/* Per-call telemetry of the last bzx_compress_device/_buffer/_blocks/_batch_* call. */
typedef struct {
    uint32_t nblk;
    uint32_t n_periodic;        /* blocks flagged periodic */
    uint64_t raw_bytes;         /* N_b summed */
    uint64_t rle1_bytes;        /* n summed */
    uint64_t mtf_symbols;       /* nMTF summed */
    uint64_t out_bits;          /* compressed bits incl. stream header/footer when present */
    float ms_split, ms_bwt, ms_mtf, ms_huffman, ms_emit, ms_total;   /* HIP-event times of the stage kernels */
    uint32_t bwt_launches;      /* 1 per run of the stage kernels (kept for the ABI; a batch call sums its rounds);
                                   ms_bwt covers every sort kernel of the run */
    uint32_t n_redo;            /* blocks the bucket sorter handed to the general sorter (deep repeats, periodic) */
    uint32_t n_buckets;         /* bucket work items of the bucket sorter */
    float ms_bwt_split, ms_bwt_sort, ms_bwt_general;   /* parts of ms_bwt: split kernel, bucket sort kernel, everything after it */
    uint32_t n_open_buckets;      /* buckets that gave up after the refinement rounds (deep repeats) */
    uint32_t n_open_left;         /* ... whose lists of tied ranks the rank rounds did not empty (left to the general sorter) */
    uint32_t n_resume_left;       /* blocks the general sorter had to finish: such buckets, oversized groups and the groups
                                     that read their ranks, periodic blocks */
    float ms_bwt_rank;            /* part of ms_bwt_general: rank rounds over the open buckets */
    uint32_t n_from_scratch;      /* blocks the split kernel refused (sorted from scratch by the general sorter) */
    uint32_t n_unsorted;          /* buckets whose optimistic initial sort failed its check (their blocks went to the general sorter): 0 */
} bzx_stats;
int bzx_get_stats(const bzx_ctx *ctx, bzx_stats *out);

/*
 * Per-block figures of the last bzx_compress_device / bzx_compress_buffer / bzx_cstream_* / bzx_compress_block(s)
 * call, blocks in stream order (a chunked stream: as many as the context's descriptor table holds, i.e. at least
 * the max_blocks of bzx_ctx_create; BZX_E_PARAM beyond) -- what the reference logs per block at -vvv
 * (src/compression/compress_block.rs:58-63, src/huffman_coding/huffman.rs:176-181).  After a bzx_compress_batch_*
 * call or any decompression it returns BZX_E_STATE: those keep no per-block figures.
 */
typedef struct bzx_block_info {
    uint32_t n;               /* RLE1'd bytes in the block */
    uint32_t crc;             /* CRC-32/BZIP2 of the raw bytes it covers */
    uint32_t orig_ptr;        /* BWT: row of rotation 0 */
    uint32_t periodic;        /* 1: the block is u^k (tie order from the libbz2 replay) */
    uint32_t n_in_use;        /* distinct byte values */
    uint32_t n_mtf;           /* MTF/RLE2 symbols incl. EOB */
    uint32_t n_tables;        /* Huffman coding tables, 2..6 */
    uint32_t n_selectors;
    uint32_t bits_symbol_map, bits_selectors, bits_tables, bits_payload;
    uint64_t bits;            /* size of the block image (header .. last payload bit) */
} bzx_block_info;
int bzx_get_block_info(const bzx_ctx *ctx, uint32_t block, bzx_block_info *out);

/*
 * bzx_mctx_* / bzx_mstream_* / bzx_mcompress_buffer: ONE process, SEVERAL devices, one .bz2 (the
 * reference's single process that fans blocks out and concatenates the results in order, compress.rs:66-132, ordered
 * writer :74-122, bit concatenation bitwriter.rs:77-132).  A bzx_mctx owns one private bzx_ctx, three HIP streams and
 * buffers of its own per entry of devices[]; the chunks of the input are dealt round-robin over the entries and the
 * host assembles their outputs in order.  No peer access, no collective, no second process, no torch: the devices
 * talk to the host only.  (The bzx_shard_* family above is the form for one process per GPU.)
 * The rule: for every devices[], every way of cutting the input into feed calls and every level, the output is
 * byte-identical to bzx_compress_buffer on the whole input (hence to libbz2 1.0.8 at that level); an empty input gives
 * the 14-byte empty stream.
 * devices[]: HIP ordinals; the same ordinal may appear several times -- each entry gets a context, streams and buffers
 * of its own (two entries on one device keep two chunks in flight there).  ndev == 0, ndev > BZX_MAX_DEVICES, a NULL
 * list or NULL out: BZX_E_PARAM; an ordinal the runtime does not have: BZX_E_NODEVICE; a failed create leaks nothing.
 * max_blocks: as for bzx_ctx_create, per entry (a context grows to the blocks of its largest chunk, about 28 MB each).
 * bzx_mctx_last_error names the entry of devices[] a failure belongs to.  bzx_mctx_destroy ends a stream that is still
 * open on the object: its bzx_mstream handle is invalid afterwards and must not be passed to bzx_mstream_end.
 * Every call sets the calling thread's current HIP device (hipSetDevice is per thread) and leaves it at the entry it
 * touched last, which differs from call to call: a caller with HIP work of its own sets its device again.
 *   begin: one open stream per bzx_mctx (a second begin, or bzx_mcompress_buffer, while one is open: BZX_E_STATE).
 *   feed: one call is one chunk (len <= max_chunk, 0 = 256 MiB; BZX_E_PARAM beyond) and the k-th call goes to entry
 *   k mod ndev.  `out`/`cap` is the WHOLE output buffer, the same on every call; *produced = length of the prefix of
 *   out that can no longer change (never a word a later chunk still has to touch).  feed returns after the bytes it
 *   was given have left the caller's buffer.  The call with final != 0 (len may be 0) completes the stream:
 *   *produced = length of the .bz2.  feed after it: BZX_E_STATE.
 *   Errors as for bzx_cstream_feed / bzx_compress_buffer, sticky for the stream object likewise; bzx_mstream_end is
 *   still required and the bzx_mctx stays usable for the next stream.
 * What a chunk needs from its predecessor goes through the host: the raw bytes of the withheld, unfinished block (one
 * page-locked tail buffer, refilled from the caller's bytes after every split) and its bit position (a sum kept by the
 * host).  Every chunk is emitted at bit phase 0 into a device buffer of its entry as soon as its Huffman stage is
 * done; when the host learns the chunk's real start and that is not a multiple of 32, a shift kernel on the entry's
 * copy-back stream moves it to its phase before it travels to `out`; the word two chunks share is OR-merged by the
 * host.  Chunks are collected strictly in order.  BWT, MTF, Huffman and emit of a chunk wait for nothing of the chunk
 * before it; only the splits form a chain (the split of chunk k needs the tail chunk k-1's split left).
 * Threads: a single host thread issues all work; the calls on one bzx_mctx are serialised by a lock of its own.  feed
 * blocks in two places: the split's synchronisation on the entry being fed (which waits for that entry's chunk
 * k - ndev while the other entries run) and the copy-back of chunk k - ndev.  Pass page-locked buffers
 * (bzx_host_alloc; allocated as portable, known to every device of the process) for truly asynchronous copies: with pageable memory the
 * runtime stages each copy and blocks the issuing thread while it lasts, which here stalls the feeding of the other
 * entries as well.
 * Memory is fixed at begin: per entry two device input buffers of max_chunk + the longest withheld tail (about 46 MB),
 * two device output buffers sized as bzx_cstream_begin sizes them and one more of that size for the shifted copy; on
 * the host one page-locked tail buffer and a few descriptors per entry.  Nothing grows with the input.
 * bzx_mcompress_buffer is a loop over feed.  Chunk size: 16 MiB, doubled while ndev chunks do not cover the input and
 * the chunk is below 128 MiB (len <= ndev x 128 MiB: the smallest such power of two that gives every entry one chunk); beyond that one block per compute unit of the smallest device (256 x 900,000 bytes on
 * MI355X) -- the rule of bzx_compress_buffer, which it equals for ndev == 1.  An input of at most one chunk uses entry
 * 0 only.  Its stream object is kept in the bzx_mctx from call to call.
 * bzx_mctx_get_stats: nblk, n_periodic, raw_bytes, rle1_bytes, mtf_symbols and out_bits of the last finished stream;
 * the stage times are summed over all chunks and entries, ms_total is the largest device time of an entry.
 */
#define BZX_MAX_DEVICES 64
typedef struct bzx_mctx bzx_mctx;
typedef struct bzx_mstream bzx_mstream;
typedef struct {
    uint32_t ndev;              /* entries of devices[] */
    uint32_t chunks;            /* feed calls of the current / last stream */
    uint32_t shifted;           /* chunks whose output went through the shift kernel (start not on a 32-bit boundary) */
    uint32_t reserved;
    uint64_t nblk;              /* blocks collected so far */
    struct {
        int32_t device;         /* HIP ordinal */
        uint32_t chunks;        /* chunks with at least one block this entry compressed */
        uint64_t blocks;
        float ms_device;        /* HIP-event time of its stage kernels, summed over its chunks */
        uint32_t reserved;
        uint64_t device_bytes;  /* device memory the stream object holds for the entry (without its context's slabs) */
        uint64_t pinned_bytes;  /* page-locked host memory the stream object holds for it */
    } dev[BZX_MAX_DEVICES];
} bzx_mdev_info;
int bzx_mctx_create(const int *devices, uint32_t ndev, uint32_t max_blocks, bzx_mctx **out);
void bzx_mctx_destroy(bzx_mctx *m);
const char *bzx_mctx_last_error(const bzx_mctx *m);
int bzx_mcompress_buffer(bzx_mctx *m, const uint8_t *raw, size_t len, int level, uint8_t *out, size_t cap,
                         size_t *out_len);
int bzx_mstream_begin(bzx_mctx *m, int level, size_t max_chunk, bzx_mstream **out);
int bzx_mstream_feed(bzx_mstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap,
                     size_t *produced);
void bzx_mstream_end(bzx_mstream *s);
int bzx_mctx_get_stats(const bzx_mctx *m, bzx_stats *out);
int bzx_mctx_get_info(const bzx_mctx *m, bzx_mdev_info *out);
/*
 * The shift kernel alone, for the parity tests (host pointers): out = in shifted right by p bits (0..31) in
 * byte-stream bit order, most significant bit of byte 0 first: output bit i + p = input bit i, the first p bits zero.
 * out holds nbytes + 4 rounded up to 4 bytes.
 */
int bzx_stage_shift_bits(bzx_ctx *ctx, const uint8_t *in, size_t nbytes, uint32_t p, uint8_t *out);

/*
 * Stream assembler (replaces BitWriter, bitwriter.rs:42-172): header "BZh<level>", bit-granular
 * append of block images minus their padding, footer magic + combined CRC (crc.rs:25-27).
 * Host-side; used with bzx_compress_block(s) when the caller keeps the reference's structure.
 */
typedef struct bzx_stream bzx_stream;
int bzx_stream_begin(int level, bzx_stream **out);
int bzx_stream_append_block(bzx_stream *s, const uint8_t *data, size_t len, uint8_t pad_bits);
/* Finishes the stream; *data stays valid until bzx_stream_free. */
int bzx_stream_finish(bzx_stream *s, const uint8_t **data, size_t *len);
void bzx_stream_free(bzx_stream *s);

/* Deterministic synthetic inputs (include/bzx_synth.h), host buffers. seed 0 = default. */
void bzx_synth_text(uint64_t seed, uint8_t *out, size_t nbytes);
void bzx_synth_random(uint64_t seed, uint8_t *out, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif
