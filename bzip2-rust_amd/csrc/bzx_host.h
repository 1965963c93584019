// bzx_host.h -- host side shared by the library's .hip files (internal, not installed): the context, the stage runner
// and every function that one file defines and another calls.  Declared here once, so a prototype cannot drift from
// its definition.
#pragma once
#include <hip/hip_runtime.h>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/bzx.h"
#include "bzx_dc.h"
#include "bzx_device.h"
#include "bzx_mem.h"

struct BlockReq {
    const uint8_t *blk;
    size_t n;
    uint32_t crc;
    uint8_t *out;
    size_t cap;
    size_t out_len = 0;
    uint8_t pad = 0;
    int rc = 0;
    bool done = false;
};

struct bzx_ctx {
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // Calls on one context from several host threads are serialised (api_mu); bzx_compress_block calls that arrive
    // together (the reference's rayon workers, compress.rs:125-132) are collected into one device batch (bq_*).
    std::recursive_mutex api_mu;
    std::mutex bq_mu;
    std::condition_variable bq_cv;
    std::vector<struct BlockReq *> bq_pending;
    bool bq_leader = false;
    // second stream: the general sorter's early launch on the blocks the bucket sorter's split refused
    hipStream_t aux = nullptr;
    hipEvent_t ev_join = nullptr;
    hipEvent_t ev_b3 = nullptr, ev_b4 = nullptr;     // ... around the rank rounds
    hipEvent_t ev_b1 = nullptr, ev_b2 = nullptr;     // bucket sorter: after the split kernel, after the sort kernel
    bool bsort_used = false;
    PinMem<uint32_t> h_counters;                      // pinned copy of d_counters after a run
    std::string err;

    uint32_t cap_blocks = 0;   // block descriptor capacity (global block numbers)
    uint32_t cap_slabs = 0;    // per-block slab capacity (owned blocks)
    std::vector<DevMem<>> descs;   // the device arrays for cap_blocks
    uint32_t n_slots = 0;      // per-workgroup scratch slots
    BzxBatch B;                // device pointers (by value into kernels)
    std::vector<DevMem<>> slabs;   // the device arrays for cap_slabs
    std::vector<DevMem<>> slot_allocs;
    uint8_t *d_in = nullptr;   // block slab buffer (one of slabs)
    uint32_t *d_outbuf = nullptr;   // per-block output slabs (per-block entry points; one of slabs)
    DevMem<uint32_t> d_counters;
    DevMem<uint64_t> d_scalars;      // [0] total bits, [1] out bytes
    DevMem<unsigned long long> d_dbg;   // [128] phase timers, only when bzx_dbg_phase_timers(ctx, 1)
    PinMem<BzxBlock> h_blk;          // pinned mirror of the descriptors, cap_blocks of them
    PinMem<uint64_t> h_scalars;
    hipEvent_t ev[8];
    bzx_stats stats;

    // sharded run state (bzx_shard_prepare -> bzx_shard_emit)
    uint32_t shard_total = 0, shard_rank = 0, shard_world = 1;
    int shard_level = 0;
    uint64_t shard_packed_max = 0;   // bytes of the longest packed buffer of any rank (known after bzx_shard_emit_packed)
    size_t shard_len = 0;

    struct bzx_cstream *cs = nullptr;        // chunked stream compressor kept for bzx_compress_buffer
    std::vector<uint8_t> split_carry;        // bzx_split_rle1_chunk: raw bytes of the withheld block
    struct bzx_dstream *ds = nullptr;        // open streaming decompressor (bzx_dstream_begin .. _end): it owns the slabs

    // device split scratch (bzx_rle1.hip)
    DevMem<> split_ws;

    // batched compression (bzx_compress_batch_*): tables and scratch of the batched splitter and layout
    DevMem<> batch_ws;
    hipEvent_t ev_bt[3] = {nullptr, nullptr, nullptr};   // round: before its split part, before emit, after framing
    bool stats_batch = false;        // the stats describe a batch call or a decompression: no per-block figures
                                     // (bzx_get_block_info)

    // batched decompression (bzx_decompress_batch_*): device tables and pinned host mirrors, grown on demand
    DevMem<> dbatch_ws;
    PinMem<> dbatch_pin[2];                     // [0] candidates and round tables, [1] the _buffer form's bounce buffer

    // range reads (bzx_decompress_range_*, _ranges_*): the staging pool and the round tables, allocated by the first call
    DevMem<> range_ws;
    PinMem<> range_pin;
    uint32_t range_slabs = 0;                   // blocks the round tables hold
    DevMem<> range_io[2];                       // the _buffer form's span [0] and output [1] on the device, grown on demand
    DevMem<> range_sl;                          // the gather kernel's slice table, grown on demand
    // record reads (bzx_records_locate_*): a round's queries and answers, grown on demand
    DevMem<> rec_ws;
    PinMem<> rec_pin;

    // block index kept by the compressor (bzx_ctx_keep_index; off: nothing below is touched but the two flags a
    // compression call clears)
    bool keep_index = false;
    uint32_t n_cstreams = 0;                    // bzx_cstream objects the caller has open on this context
    bool cidx_ok = false;                       // cidx / cidx_info describe the last bzx_compress_device / _buffer call
    std::vector<bzx_index_entry> cidx;
    bzx_index_info cidx_info = {};
    bool bidx_ok = false;                       // bidx / bidx_first describe the last bzx_compress_batch_* call
    std::vector<bzx_index_entry> bidx;          // the entries of all streams, in input order
    std::vector<uint64_t> bidx_first;           // [count + 1] stream i owns bidx[bidx_first[i] .. bidx_first[i + 1])
};

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                      \
            return BZX_E_HIP;                                                                    \
        }                                                                                        \
    } while (0)

// The lock of an entry point: serialises the calls on one context (none without a context: the argument check that
// follows refuses the call).
static inline std::unique_lock<std::recursive_mutex> ctx_lock(bzx_ctx *ctx)
{
    return ctx ? std::unique_lock<std::recursive_mutex>(ctx->api_mu) : std::unique_lock<std::recursive_mutex>();
}

// Between bzx_dstream_begin and bzx_dstream_end the slabs hold the stream's decoded blocks: every other compute entry
// point of the context is refused (after its lock is taken; the stream stays intact).
static inline int refuse_streaming(bzx_ctx *ctx)
{
    ctx->err = "the context is busy with an open bzx_dstream (its block slabs hold the stream's decoded blocks): call "
               "bzx_dstream_end first";
    return BZX_E_STATE;
}
#define BZX_REFUSE_WHILE_STREAMING(ctx)                          \
    do {                                                         \
        if ((ctx) && (ctx)->ds) return refuse_streaming(ctx);    \
    } while (0)

static inline int level_ok(int level) { return level >= 1 && level <= 9; }

// Number of workgroups for a one-workgroup-per-block kernel over nblk blocks.
static inline uint32_t grid_for(const bzx_ctx *ctx, uint32_t nblk, uint32_t per_cu)
{
    uint32_t g = (uint32_t)ctx->n_cu * per_cu;
    return nblk < g ? nblk : g;
}

enum { STG_BWT = 1, STG_MTF = 2, STG_HUF = 4, STG_EMIT = 8, STG_ALL = 15 };

// ---- bzx_api.hip: context, stage runner, split, statistics
int ensure_blocks(bzx_ctx *ctx, uint32_t nblk, uint32_t nslab = 0);
int run_stages(bzx_ctx *ctx, uint32_t nblk, int stages, int out_level = 0, void *d_stream_out = nullptr,
               size_t stream_cap = 0, uint64_t *d_phase = nullptr);
int split_on_device(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, int level, uint32_t *nblk_out,
                    uint32_t own_first = 0, uint32_t own_step = 1, uint64_t *last_raw_start = nullptr,
                    uint64_t *gathered_tiles = nullptr);
int bzx_ctx_split_scratch(bzx_ctx *ctx, size_t bytes, void **p);
void collect_stage_times(bzx_ctx *ctx);
void fold_blocks(bzx_stats &st, const BzxBlock *blk, uint32_t first, uint32_t end, uint32_t step);

// ---- bzx_cstream.hip: what the chunked stream compressors (one device, several devices) share
// Buffer sizes for chunks of at most max_chunk bytes (0 = 256 MiB; rounded up to 16 bytes), good for every level:
// in_cap a chunk + the longest withheld tail, out_cap its output, blk_cap its blocks.
struct ChunkCaps { size_t max_chunk, in_cap, out_cap; uint32_t blk_cap; };
ChunkCaps chunk_caps(size_t max_chunk);
// Chunk of the one-shot calls: chunk_min doubled up to 128 MiB while below len, then one block per compute unit.
size_t buffer_chunk(size_t len, int n_cu, size_t chunk_min);
// What one device holds for a chunk pipeline beside its context.  alloc and free run with that device current.
struct ChunkLane {
    DevMem<uint8_t> d_in[2];
    DevMem<uint32_t> d_out[2];
    DevMem<uint64_t> d_phase;                     // [0] bit phase of the next chunk, [1] bits of the last laid-out chunk
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_d2h = nullptr;
    PinMem<uint64_t> h_info[2];                   // d_phase after the chunk emitted into d_out[slot]
    PinMem<BzxBlock> h_blk[2];                    // descriptors of the chunk's blocks (CRCs)
    PinMem<uint32_t> h_w0;                        // first word of a chunk's output (shared with its predecessor)
    size_t device_bytes = 0, pinned_bytes = 0;    // what alloc asked for
    bool alloc(size_t in_cap, size_t out_cap, uint32_t blk_cap);      // false: something failed; free() releases the rest
    void free();                                  // waits for the two copy streams, then releases the buffers, events and streams
};
// Where a finished chunk goes: bit phase of its first word, words it touches, byte offset of the first in `out`.
struct ChunkPlace { uint64_t phase, nwords; size_t off; };
// The stream as the host accounts for it, chunk by chunk.  What can fail returns a BZX_E_* code and its text in `err`.
struct ChunkAcct {
    int level = 9;
    uint32_t k = 0;                               // chunks fed
    uint64_t bits = 32;                           // stream bits accounted for so far (header included)
    uint32_t crc_comb = 0;
    uint64_t nblk_total = 0;
    bzx_stats st = {};                            // block figures of the stream so far
    bool finished = false;
    int sticky = BZX_OK;                          // the error a feed call returned: later feed calls return it again
    uint8_t *out = nullptr;
    size_t cap = 0, need_hint = 0;                // need_hint, after BZX_E_OUTBUF: bytes the output needs at least
    // the stream's block index (bzx_ctx_keep_index): one entry per block accounted for, 40 bytes each; empty when off
    bool keep = false;
    std::vector<bzx_index_entry> idx;
    uint64_t raw_off = 0;                         // raw bytes the entries cover
    uint64_t stream_bytes = 0;                    // length of the finished stream
    void reset(int l, bool keep_index = false)    // a new stream on the same object (the index keeps its memory)
    {
        std::vector<bzx_index_entry> v;
        v.swap(idx);
        *this = ChunkAcct();
        level = l;
        keep = keep_index;
        v.clear();
        idx.swap(v);
    }
    void begin_output(uint8_t *out, size_t cap);  // the caller's buffer of this feed call; chunk 0: the stream header
    int place_chunk(uint64_t cbits, ChunkPlace *p, std::string &err);
    void merge_first_word(const ChunkPlace &p, const uint32_t *h_w0);
    int account_chunk(const BzxBlock *h_blk, uint32_t nblk, uint64_t cbits, std::string &err);
    // the entries so far; in_bytes and nstreams are 0 until finish() has run (BZX_E_STATE when the index is not kept)
    int get_index(const bzx_index_entry **entries, bzx_index_info *info) const;
    // final feed call of len bytes, every chunk accounted for: footer, *produced, and nblk / raw_bytes / out_bits of st
    int finish(size_t len, size_t *produced, std::string &err);
};
// Appends the index entries of nblk blocks of one stream, in order, from their descriptors (crc, bits, raw_len): *bit and
// *raw_off are the running sums, before and after.  BZX_E_NOMEM when the vector cannot grow (nothing unwinds).
int index_append(std::vector<bzx_index_entry> &idx, const BzxBlock *h_blk, uint32_t nblk, int level, uint64_t *bit,
                 uint64_t *raw_off);
// combined CRC of a stream after one more block (crc.rs:25-27)
__host__ __device__ static inline uint32_t crc_fold(uint32_t comb, uint32_t crc) { return ((comb << 1) | (comb >> 31)) ^ crc; }

// ---- bzx_mdev.hip: shift of a finished chunk to its bit phase
void bzx_launch_shift_bits(const uint32_t *d_in, uint32_t n_words, uint32_t p, uint32_t *d_out, uint32_t n_cu,
                           hipStream_t stream);

// ---- launchers of the stage kernels
void bzx_launch_bwt(const BzxBatch &B, uint32_t grid, hipStream_t stream);                                  // bzx_bwt.hip
uint32_t bzx_bwt_max_blocks_per_cu();
void bzx_launch_bsplit(const BzxBatch &B, uint32_t grid, uint32_t grid_deep, hipStream_t stream);           // bzx_bsort.hip
void bzx_launch_bsort(const BzxBatch &B, uint32_t grid, hipStream_t stream);
void bzx_launch_brank(const BzxBatch &B, uint32_t grid, hipStream_t stream);
void bzx_launch_bgiant(const BzxBatch &B, uint32_t grid, hipStream_t stream);
uint32_t bzx_bsort_blocks_per_cu();
void bzx_launch_periodic(const BzxBatch &B, uint32_t grid, hipStream_t stream);                             // bzx_periodic.hip
void bzx_launch_mtf(const BzxBatch &B, uint32_t grid, hipStream_t stream);                                  // bzx_mtf.hip
void bzx_launch_huffman(const BzxBatch &B, uint32_t grid, hipStream_t stream);                              // bzx_huff.hip
// (the emit kernel's work item is a run of tiles of a block, so its grid is sized by residency on n_cu compute units)
void bzx_launch_emit(const BzxBatch &B, uint32_t n_cu, hipStream_t stream);                                 // bzx_emit.hip
void bzx_launch_layout(const BzxBatch &B, uint64_t first_bit, uint64_t stride_bits, uint64_t *d_total_bits,
                       hipStream_t stream, uint64_t *d_phase = nullptr);
void bzx_launch_stream_frame(const BzxBatch &B, int level, const uint64_t *d_total_bits, uint64_t *d_out_bytes,
                             hipStream_t stream);
void bzx_launch_bits_export(const BzxBatch &B, long long *bits, hipStream_t stream);
void bzx_launch_bits_import(const BzxBatch &B, const long long *bits, hipStream_t stream);
void bzx_launch_pack_layout(const BzxBatch &B, uint32_t first, uint32_t step, uint32_t nown, uint64_t *d_total,
                            hipStream_t stream);
void bzx_launch_pack_max(const BzxBatch &B, uint32_t world, uint64_t *d_out, hipStream_t stream);
void bzx_launch_zero_edges(const BzxBatch &B, const uint64_t *d_total, hipStream_t stream);
void bzx_launch_unpack(const BzxBatch &B, const uint32_t *packed, uint32_t first, uint32_t step, uint32_t nown,
                       uint32_t grid, hipStream_t stream);

// ---- bzx_rle1.hip: the block splitter
int bzx_split_launch_boundaries(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, int level, uint32_t max_blocks,
                                BzxSplitWs *ws_out);
uint64_t bzx_split_tiles_per_rank(size_t len, uint32_t world);
int bzx_split_shard_runs(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, uint32_t rank, uint32_t world, uint64_t *tiles);
int bzx_split_shard_counts(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, uint32_t rank, uint32_t world, uint64_t *tiles);
int bzx_split_shard_boundaries(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, int level, uint32_t max_blocks,
                               uint32_t world, uint64_t *tiles, BzxSplitWs *ws_out);
void bzx_split_launch_scatter(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, const BzxSplitWs &ws, uint32_t nblk,
                              uint8_t *d_slabs, BzxBlock *d_blk, uint32_t own_first, uint32_t own_step);
void bzx_launch_block_crcs(bzx_ctx *ctx, const uint8_t *d_raw, const uint64_t *d_bounds, uint32_t *d_nblk, BzxBlock *d_blk,
                           uint32_t nblk);
void bzx_split_scan(hipStream_t st, uint64_t *v, uint64_t n, int is_max, uint64_t *segtot);
uint64_t bzx_split_scan_words(uint64_t n);

// ---- bzx_decomp.hip: the decoder's kernels, over any set of blocks (one-shot and batch: bzx_dbatch.hip; bzx_dstream.hip)
void bzx_launch_dc_decode(const BzxBatch &B, const BzxDcSrc *src, hipStream_t stream);
void bzx_launch_dc_ibwt(const BzxBatch &B, uint8_t *img_slabs, hipStream_t stream);
void bzx_launch_dc_ibwt_wide(const BzxBatch &B, uint8_t *img_slabs, uint32_t n_hint, hipStream_t stream);   // one workgroup per block
void bzx_launch_dc_expand(const BzxBatch &B, const uint8_t *img_slabs, const BzxDcDst *dst, hipStream_t stream);
void bzx_launch_dc_crc(const BzxBatch &B, const BzxDcDst *dst, uint32_t *got, uint32_t n_cu, hipStream_t stream);

// ---- bzx_range.hip: what a round of a range read is made of (the record reads of bzx_records.hip decode their blocks
// through the same round, tables, pool and verdict)
#define RG_EDGE_BYTES ((size_t)(BZX_MAX_N / 5 * 259 + 16))      // an expanded block: 259/5 x 900,000, rounded up
#define RG_POOL_BYTES (2 * rg_al(RG_EDGE_BYTES))                // the pool: room for the two edge blocks of one range
static inline size_t rg_al(size_t x) { return (x + 255) & ~(size_t)255; }
// The input bytes a block needs: from the byte that holds its magic to its last bit, rounded up to a byte, + 8.
static inline void rg_block_bytes(const bzx_index_entry &x, uint64_t *lo, uint64_t *hi)
{
    *lo = x.bit / 8;
    *hi = (x.bit + x.img_bits + 7) / 8 + 8;
}
struct RgTables {
    BzxDcSrc *d_src;
    BzxDcDst *d_dst;
    uint32_t *d_len, *d_got, *d_flag, *h_got, *h_flag;
    uint8_t *pool;
};
int rg_tables(bzx_ctx *ctx, uint32_t R, RgTables *t);
int rg_round(bzx_ctx *ctx, const RgTables &t, uint32_t nb, const BzxDcSrc *src, const BzxDcDst *dst, const uint32_t *len,
             uint32_t n_hint);
int rg_verdict(bzx_ctx *ctx, const bzx_index_entry &x, uint64_t k, const BzxBlock &d, uint32_t flag, uint32_t got);
int rg_upload(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const uint8_t *held, const uint8_t **d_pc);

// ---- bzx_records.hip: the delimiter count of every segment (block) of a table, one 32-bit count each
// blk: the blocks' descriptors (a block with a status is skipped, its length is pack_word) or null (the length is
// seg[b].cap); a segment without a pointer is skipped.
void bzx_launch_rec_count(const BzxBlock *blk, const BzxDcDst *seg, uint32_t nseg, uint32_t delim, uint32_t *counts,
                          uint32_t n_cu, hipStream_t stream);

// ---- bzx_find.hip: the hits of a pattern in a run of device bytes [p, p + *len), *len read on the device
// Three launches: count (hits per section, a wave's 4 KiB of a tile), scan (sec[] becomes the exclusive sum, *after =
// *before + the run's count; with `edges` also the run's first and last min(m - 1, *len) bytes) and emit (hit number k of
// the numbering that starts at *before goes to out[k - skip] when skip <= k < skip + cap, as a position relative to p).
#define FIND_TILE_BYTES 16384u               // start positions of a workgroup's tile, cut on 16-byte boundaries of the address
#define FIND_SEC_BYTES (FIND_TILE_BYTES / 4) // ... of one wave's section of it
#define FIND_INLINE_HITS 1024u               // hits of a pass that travel with its record
#define FIND_WINDOW_HITS (1u << 20)          // hits per emit window behind them
struct BzxFindPat {                          // the pattern, a kernel argument: bytes 0 .. m - 1 of w, zeros behind
    uint32_t w[BZX_FIND_MAX_PATTERN / 4];
    uint32_t m;
};
struct BzxFindOut {                          // what a pass leaves for the host in front of its index records
    uint64_t count;                          // hits of the pass
    uint32_t nedge, pad_;                    // min(m - 1, verified bytes of the pass)
    uint8_t head[BZX_FIND_MAX_PATTERN], tail[BZX_FIND_MAX_PATTERN];      // its first and last nedge verified bytes
    uint32_t hits[FIND_INLINE_HITS];         // its first hits, relative to the staging area
};
struct BzxFindLines {                        // (bzx_index_find_lines) ... and behind BzxFindOut, in front of the records
    uint64_t dcount;                         // delimiters among the verified bytes of the pass
    uint32_t lines[FIND_INLINE_HITS];        // delimiters of the pass in front of hits[i]
};
static inline size_t bzx_find_sections(uint64_t len) { return (size_t)((len + 15 + FIND_SEC_BYTES - 1) / FIND_SEC_BYTES) + 1; }
uint32_t bzx_find_grid(uint64_t len, uint32_t n_cu);
bool bzx_find_pattern(const uint8_t *pat, size_t m, BzxFindPat *out);
void bzx_launch_find_count(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, uint32_t *sec, uint32_t grid,
                           hipStream_t stream);
void bzx_launch_find_scan(const uint8_t *p, const uint64_t *len, uint32_t m, uint32_t *sec, const uint64_t *before,
                          uint64_t *after, BzxFindOut *edges, hipStream_t stream);
void bzx_launch_find_emit(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, const uint32_t *sec,
                          const uint64_t *before, const uint64_t *after, uint64_t skip, uint32_t cap, uint32_t *out,
                          uint32_t grid, hipStream_t stream);
// The lines forms: dsec[] (bzx_find_sections() words, as sec[]) holds the delimiters per section of the whole run, then
// their exclusive sum; *dafter = the run's delimiters; lines_out[k - skip] = the run's delimiters in front of hit k.
void bzx_launch_find_count_lines(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, uint32_t delim, uint32_t *sec,
                                 uint32_t *dsec, uint32_t grid, hipStream_t stream);
void bzx_launch_find_scan_lines(const uint8_t *p, const uint64_t *len, uint32_t m, uint32_t *sec, uint32_t *dsec,
                                const uint64_t *before, uint64_t *after, uint64_t *dafter, BzxFindOut *edges, hipStream_t stream);
void bzx_launch_find_emit_lines(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, uint32_t delim, const uint32_t *sec,
                                const uint32_t *dsec, const uint64_t *before, const uint64_t *after, uint64_t skip, uint32_t cap,
                                uint32_t *out, uint32_t *lines_out, uint32_t grid, hipStream_t stream);
