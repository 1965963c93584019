// bzx_cstream.hip -- chunked stream compressor (include/bzx.h: bzx_cstream_*) and bzx_compress_buffer on top of it.
//
// The reference's driver reads the input incrementally (RLE1Block<R: Read>, rle1.rs:49-85,245-263), overlaps block
// production, compression and an ordered writer thread (compress.rs:66-132, bitwriter.rs:77-132).  Here the input
// arrives in CHUNKS: chunk k is copied to the device while chunk k-1 is compressed and the output of chunk k-2..k-1
// travels back, on three HIP streams with double buffers.  Block boundaries depend on the whole stream before them
// (SURVEY.md D1); a chunk is therefore split as "the raw bytes of the last, unfinished block of the previous chunk
// + the new bytes": the splitter's state is clean at a block start (a block is a whole number of run pieces), so
// restarting there reproduces exactly the blocks a one-shot split would cut.  All blocks but the last of a chunk
// are compressed; the last one is withheld until more input (or `final`) arrives.  Chunk outputs are bit-contiguous:
// the bit phase travels on the device (bzx_layout_kernel), the shared boundary word is OR-merged on the host, header
// and footer (+ combined CRC, crc.rs:25-27) are written by the host.
#include <string.h>
#include <new>
#include "bzx_host.h"

struct bzx_cstream {
    bzx_ctx *ctx = nullptr;
    int level = 9;
    size_t max_chunk = 0, in_cap = 0, out_cap = 0;
    uint8_t *d_in[2] = {nullptr, nullptr};
    uint32_t *d_out[2] = {nullptr, nullptr};
    uint64_t *d_phase = nullptr;            // [0] bit phase of the next chunk, [1] bits of the last laid-out chunk
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_d2h = nullptr;
    uint64_t *h_info[2] = {nullptr, nullptr};     // pinned: {phase in, bits} of the chunk emitted into d_out[slot]
    uint32_t *h_w0 = nullptr;                     // pinned: first word of a chunk's output (shared with its predecessor)
    BzxBlock *h_blk[2] = {nullptr, nullptr};      // pinned: descriptors of the chunk's blocks (CRCs)
    uint32_t blk_cap = 0;
    uint32_t k = 0;                         // chunks fed
    size_t carry_len = 0, carry_start = 0;  // raw bytes of the withheld block inside d_in[(k-1)&1]
    uint64_t bits = 32;                     // stream bits accounted for so far (header included)
    uint32_t crc_comb = 0;
    uint64_t nblk_total = 0;
    bzx_stats st = {};                      // block figures of the stream so far (n_periodic, rle1_bytes, mtf_symbols, raw_bytes)
    bool pend = false;                      // a chunk's output still sits in d_out[pend_slot]
    bool coll_issued = false;               // ... and its copy-back has been enqueued (cstream_collect), not yet awaited
    uint32_t pend_slot = 0, pend_nblk = 0;
    bool finished = false;
    uint8_t *out = nullptr;
    size_t cap = 0;
    size_t need_hint = 0;                   // after BZX_E_OUTBUF: bytes the output needs at least
};

extern "C" void bzx_cstream_end(bzx_cstream *s)
{
    if (!s) return;
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    if (s->ctx) (void)hipStreamSynchronize(s->ctx->stream);
    if (s->s_h2d) (void)hipStreamSynchronize(s->s_h2d);
    if (s->s_d2h) (void)hipStreamSynchronize(s->s_d2h);
    for (int i = 0; i < 2; i++) {
        if (s->d_in[i]) (void)hipFree(s->d_in[i]);
        if (s->d_out[i]) (void)hipFree(s->d_out[i]);
        if (s->ev_h2d[i]) (void)hipEventDestroy(s->ev_h2d[i]);
        if (s->ev_done[i]) (void)hipEventDestroy(s->ev_done[i]);
        if (s->h_info[i]) (void)hipHostFree(s->h_info[i]);
        if (s->h_blk[i]) (void)hipHostFree(s->h_blk[i]);
    }
    if (s->ev_d2h) (void)hipEventDestroy(s->ev_d2h);
    if (s->d_phase) (void)hipFree(s->d_phase);
    if (s->h_w0) (void)hipHostFree(s->h_w0);
    if (s->s_h2d) (void)hipStreamDestroy(s->s_h2d);
    if (s->s_d2h) (void)hipStreamDestroy(s->s_d2h);
    delete s;
}

// A block covers at most nblockMAX RLE1 bytes = nblockMAX / 5 runs of 255: the withheld raw tail never exceeds this.
size_t cstream_max_carry(int level) { return ((size_t)100000 * level / 5 + 2) * 255 + 4096; }

// Footer of a stream whose last block ends at bit `end`: magic, combined CRC (crc.rs:25-27), zero padding to a byte
// (bitwriter.rs:103-114,158-172); need = (end + 80 + 7) / 8 bytes of out are the stream.
void stream_write_footer(uint8_t *out, uint64_t end, size_t need, uint32_t crc_comb)
{
    const uint8_t foot[10] = {0x17, 0x72, 0x45, 0x38, 0x50, 0x90, (uint8_t)(crc_comb >> 24), (uint8_t)(crc_comb >> 16),
                              (uint8_t)(crc_comb >> 8), (uint8_t)crc_comb};
    const size_t ebyte = (size_t)(end >> 3);
    const uint32_t sh = (uint32_t)(end & 7u);
    // bytes from the end of the last word written on are untouched so far: clear, then OR the shifted footer in
    const size_t clear_from = (size_t)((end + 31) >> 5) * 4;
    for (size_t i = clear_from; i < need; i++) out[i] = 0;
    for (int i = 0; i < 10; i++) {
        out[ebyte + i] |= (uint8_t)(foot[i] >> sh);
        if (sh) out[ebyte + i + 1] |= (uint8_t)(foot[i] << (8 - sh));
    }
}

extern "C" int bzx_cstream_begin(bzx_ctx *ctx, int level, size_t max_chunk, bzx_cstream **out)
{
    if (!ctx || !out || !level_ok(level)) return BZX_E_PARAM;
    *out = nullptr;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (max_chunk == 0) max_chunk = (size_t)256 << 20;
    max_chunk = (max_chunk + 15) & ~(size_t)15;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bzx_cstream *s = new (std::nothrow) bzx_cstream();
    if (!s) return BZX_E_NOMEM;
    s->ctx = ctx;
    s->level = level;
    s->max_chunk = max_chunk;
    // Sized for EVERY level, not the one given here: bzx_compress_buffer keeps the stream object in the context and
    // starts the next stream on it at whatever level its caller asks for (cstream_reset) -- the withheld raw tail is
    // longest at level 9, the blocks of a chunk are most numerous at level 1.
    s->in_cap = max_chunk + cstream_max_carry(9) + 256;
    s->out_cap = (s->in_cap + s->in_cap / 50 + 65536) & ~(size_t)255;       // RLE1 +25 % never survives coding: 2 % + slack
    s->out_cap += s->in_cap / 4;
    s->blk_cap = (uint32_t)((s->in_cap + s->in_cap / 4) / ((size_t)100000 * 1 - 19) + 4);
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++) {
        ok = hipMalloc((void **)&s->d_in[i], s->in_cap) == hipSuccess && hipMalloc((void **)&s->d_out[i], s->out_cap) == hipSuccess &&
             hipEventCreateWithFlags(&s->ev_h2d[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s->ev_done[i], hipEventDisableTiming) == hipSuccess &&
             hipHostMalloc((void **)&s->h_info[i], 4 * sizeof(uint64_t), 0) == hipSuccess &&
             hipHostMalloc((void **)&s->h_blk[i], (size_t)s->blk_cap * sizeof(BzxBlock), 0) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&s->ev_d2h, hipEventDisableTiming) == hipSuccess &&
         hipMalloc((void **)&s->d_phase, 4 * sizeof(uint64_t)) == hipSuccess &&
         hipHostMalloc((void **)&s->h_w0, 16, 0) == hipSuccess &&
         hipStreamCreateWithFlags(&s->s_h2d, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&s->s_d2h, hipStreamNonBlocking) == hipSuccess &&
         hipMemsetAsync(s->d_phase, 0, 4 * sizeof(uint64_t), ctx->stream) == hipSuccess;
    if (!ok) {
        ctx->err = "bzx_cstream_begin: device or pinned allocation failed";
        bzx_cstream_end(s);
        return BZX_E_NOMEM;
    }
    *out = s;
    return BZX_OK;
}

// Brings the output of the chunk parked in d_out[pend_slot] to the caller's buffer (async on the copy-back stream)
// and accounts for its bits and block CRCs.  The chunk's layout has completed when this is called.
static int cstream_collect(bzx_cstream *s)
{
    bzx_ctx *ctx = s->ctx;
    if (!s->pend) return BZX_OK;
    const uint32_t slot = s->pend_slot;
    // h_info = {phase the NEXT chunk starts with, bits of this chunk}; this chunk started at the phase the host
    // accounting says
    const uint64_t phase = s->bits & 31u, cbits = s->h_info[slot][1];
    if (s->h_info[slot][0] != ((phase + cbits) & 31u)) {
        ctx->err = "chunked stream: bit phase out of step";
        return BZX_E_STATE;
    }
    const uint64_t nwords = (phase + cbits + 31) >> 5;
    const size_t off = (size_t)(s->bits >> 5) * 4;
    if (off + nwords * 4 > s->cap) {
        ctx->err = "output buffer too small for the compressed stream";
        s->need_hint = off + (size_t)((phase + cbits + 80 + 7) >> 3);
        return BZX_E_OUTBUF;
    }
    if (nwords * 4 > s->out_cap) {
        ctx->err = "chunk output larger than its device buffer";
        return BZX_E_HIP;
    }
    HIP_TRY(ctx, hipStreamWaitEvent(s->s_d2h, s->ev_done[slot], 0));
    if (nwords) {
        HIP_TRY(ctx, hipMemcpyAsync(s->h_w0, s->d_out[slot], 4, hipMemcpyDeviceToHost, s->s_d2h));
        if (nwords > 1)
            HIP_TRY(ctx, hipMemcpyAsync(s->out + off + 4, s->d_out[slot] + 1, (nwords - 1) * 4, hipMemcpyDeviceToHost, s->s_d2h));
    }
    HIP_TRY(ctx, hipEventRecord(s->ev_d2h, s->s_d2h));
    s->coll_issued = true;
    return BZX_OK;
}

// Second half: waits for the copy-back issued by cstream_collect, merges the word the chunk shares with its
// predecessor and folds its block CRCs.  Called AFTER the next chunk's stages have been enqueued, so the copy-back of
// chunk k-1 runs beside the compression of chunk k.
static int cstream_collect_finish(bzx_cstream *s)
{
    bzx_ctx *ctx = s->ctx;
    if (!s->pend || !s->coll_issued) return BZX_OK;
    s->coll_issued = false;
    const uint32_t slot = s->pend_slot;
    const uint64_t phase = s->bits & 31u, cbits = s->h_info[slot][1];
    const uint64_t nwords = (phase + cbits + 31) >> 5;
    const size_t off = (size_t)(s->bits >> 5) * 4;
    HIP_TRY(ctx, hipEventSynchronize(s->ev_d2h));
    if (nwords) {
        // the first word is shared with the predecessor (or with nothing: then the bytes there are still zero)
        uint8_t w[4];
        memcpy(w, s->h_w0, 4);
        if (phase == 0) memcpy(s->out + off, w, 4);
        else for (int i = 0; i < 4; i++) s->out[off + i] |= w[i];
    }
    fold_blocks(s->st, s->h_blk[slot], 0, s->pend_nblk, 1);
    for (uint32_t b = 0; b < s->pend_nblk; b++) {
        const BzxBlock &d = s->h_blk[slot][b];
        s->crc_comb = crc_fold(s->crc_comb, d.crc);
        // (bzx_get_block_info: the stream's descriptors in order, as far as the context's descriptor table reaches)
        if (ctx->h_blk && s->nblk_total + b < ctx->cap_blocks) ctx->h_blk[s->nblk_total + b] = d;
    }
    s->nblk_total += s->pend_nblk;
    s->bits += cbits;
    s->pend = false;
    return BZX_OK;
}

// Back to the state after bzx_cstream_begin (buffers kept): a new stream on the same object.
static int cstream_reset(bzx_cstream *s, int level)
{
    bzx_ctx *ctx = s->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_h2d));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_d2h));
    HIP_TRY(ctx, hipMemsetAsync(s->d_phase, 0, 4 * sizeof(uint64_t), ctx->stream));
    s->level = level;
    s->k = 0;
    s->carry_len = s->carry_start = 0;
    s->bits = 32;
    s->crc_comb = 0;
    s->nblk_total = 0;
    s->st = {};
    s->pend = false;
    s->coll_issued = false;
    s->finished = false;
    return BZX_OK;
}

extern "C" int bzx_cstream_feed(bzx_cstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap,
                                size_t *produced)
{
    if (!s || !s->ctx || !out || !produced || (len && !raw) || len > s->max_chunk || cap < 16) return BZX_E_PARAM;
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (s->finished) return BZX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->k == 0) {
        memset(out, 0, cap < 64 ? cap : 64);
        out[0] = 'B'; out[1] = 'Z'; out[2] = 'h'; out[3] = (uint8_t)('0' + s->level);
    }
    s->out = out;
    s->cap = cap;
    const uint32_t slot = s->k & 1u;
    const size_t total = s->carry_len + len;
    if (total > s->in_cap) {                     // (cannot happen with the provisioning above; never write past d_in)
        ctx->err = "chunked stream: withheld bytes + chunk exceed the device input buffer";
        return BZX_E_STATE;
    }
    // the device buffer of this slot was last read by chunk k-2; its kernels are long done when k-1's results were
    // collected, but the copy stream does not know that: make it wait
    if (s->k >= 2) HIP_TRY(ctx, hipStreamWaitEvent(s->s_h2d, s->ev_done[slot], 0));
    if (len) {
        HIP_TRY(ctx, hipMemcpyAsync(s->d_in[slot] + s->carry_len, raw, len, hipMemcpyHostToDevice, s->s_h2d));
    }
    HIP_TRY(ctx, hipEventRecord(s->ev_h2d[slot], s->s_h2d));
    if (s->carry_len)     // the withheld block's raw bytes move to the front of this chunk (after the kernels that read them)
        HIP_TRY(ctx, hipMemcpyAsync(s->d_in[slot], s->d_in[slot ^ 1u] + s->carry_start, s->carry_len, hipMemcpyDeviceToDevice,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s->ev_h2d[slot], 0));
    uint32_t nblk = 0, use = 0;
    uint64_t last_start = 0;
    int rc = BZX_OK;
    if (total) {
        ctx->B.blk_first = 0;
        ctx->B.blk_step = 1;
        rc = split_on_device(ctx, s->d_in[slot], total, s->level, &nblk, 0, 1, &last_start);     // (synchronises)
        if (rc) return rc;
        use = final ? nblk : nblk - 1;
        if (use > s->blk_cap) {
            ctx->err = "chunked stream: more blocks in a chunk than provisioned";
            return BZX_E_HIP;
        }
    }
    // the previous chunk was laid out before this chunk's split ran: its sizes are on the host now
    if (!total) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // Chunk k's stages go into the queue FIRST; then the copy-back of chunk k-1 is issued on its own stream and awaited:
    // it runs beside the compression of chunk k (with a pageable destination the runtime stages the copy and blocks the
    // host while it lasts -- the device has its work by then).
    if (use) {
        if ((rc = run_stages(ctx, use, STG_ALL, -1, s->d_out[slot], s->out_cap, s->d_phase))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(s->h_info[slot], s->d_phase, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(s->h_blk[slot], ctx->B.blk, (size_t)use * sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(s->ev_done[slot], ctx->stream));
    if ((rc = cstream_collect(s))) return rc;
    if ((rc = cstream_collect_finish(s))) return rc;
    if (use) {
        s->pend = true;
        s->pend_slot = slot;
        s->pend_nblk = use;
    }
    if (!final && total) {
        s->carry_start = (size_t)last_start;
        s->carry_len = total - (size_t)last_start;
    } else {
        s->carry_len = 0;
        s->carry_start = 0;
    }
    s->k++;
    if (final) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = cstream_collect(s))) return rc;
        if ((rc = cstream_collect_finish(s))) return rc;
        collect_stage_times(ctx);
        const uint64_t end = s->bits;
        const size_t need = (size_t)((end + 80 + 7) >> 3);
        if (need > cap) {
            ctx->err = "output buffer too small for the compressed stream";
            s->need_hint = need;
            return BZX_E_OUTBUF;
        }
        stream_write_footer(out, end, need, s->crc_comb);
        *produced = need;
        s->finished = true;
        ctx->stats.nblk = (uint32_t)s->nblk_total;
        ctx->stats_batch = false;
        ctx->stats.n_periodic = s->st.n_periodic;
        ctx->stats.rle1_bytes = s->st.rle1_bytes;
        ctx->stats.mtf_symbols = s->st.mtf_symbols;
        ctx->stats.raw_bytes = s->st.raw_bytes + len;
        ctx->stats.out_bits = (uint64_t)need * 8;
        return BZX_OK;
    }
    s->st.raw_bytes += len;
    // bytes that can no longer change: everything before the word the next chunk starts in
    *produced = (size_t)(s->bits >> 5) * 4;
    return BZX_OK;
}

// Host buffer -> host buffer: the chunked stream compressor over the whole input (H2D of chunk k+1, compression of
// chunk k and D2H of chunk k-1 overlap; no device allocation per call: the stream object is kept in the context).
// Pinned caller buffers (hipHostMalloc / hipHostRegister / bzx_host_alloc) make the copies truly asynchronous.
extern "C" int bzx_compress_buffer(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, uint8_t *out, size_t cap,
                                   size_t *out_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !out || !out_len || !level_ok(level) || (len && !raw) || cap < 16) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // chunk: 16 MiB doubling up to 128 MiB, then one block per compute unit (256 x 900,000 B on MI355X): the kernels that
    // give a block one workgroup then run whole rounds (299 blocks of a 256 MiB chunk were 1.17 rounds, paid as two)
    size_t chunk = (size_t)16 << 20;
    while (chunk < len && chunk < ((size_t)128 << 20)) chunk <<= 1;
    if (chunk < len) chunk = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 900000u;
    int rc;
    if (ctx->cs && ctx->cs->max_chunk < chunk) {
        bzx_cstream_end(ctx->cs);
        ctx->cs = nullptr;
    }
    if (!ctx->cs) {
        if ((rc = bzx_cstream_begin(ctx, level, chunk, &ctx->cs))) return rc;
    } else if ((rc = cstream_reset(ctx->cs, level))) {
        return rc;
    }
    chunk = ctx->cs->max_chunk;
    hipEvent_t e0 = ctx->ev[5], e1 = ctx->ev[7];
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    size_t off = 0, produced = 0;
    do {
        const size_t n = len - off < chunk ? len - off : chunk;
        const int fin = off + n == len;
        if ((rc = bzx_cstream_feed(ctx->cs, raw + off, n, fin, out, cap, &produced))) {
            if (rc == BZX_E_OUTBUF) *out_len = ctx->cs->need_hint;      // (a lower bound when chunks remain)
            return rc;
        }
        off += n;
    } while (off < len);
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&ctx->stats.ms_total, e0, e1);
    ctx->stats.raw_bytes = len;
    *out_len = produced;
    return BZX_OK;
}
