// bzx_cstream.hip -- chunked stream compressor (include/bzx.h: bzx_cstream_*), bzx_compress_buffer on top of it, and
// what it shares with the multi-device compressor of bzx_mdev.hip (bzx_host.h): buffer sizes, per-device resources
// (ChunkLane), the host's accounting of the stream (ChunkAcct: header, placement of a chunk, boundary word, CRC fold,
// footer) and the chunk rule of the one-shot calls.
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
// and footer (+ combined CRC, crc.rs:25-27) are written by the host.  A feed call validates chunk k-1 after chunk k's
// stages are in the queue: an error leaves the device phase ahead of the accounting, so it is sticky.
#include <string.h>
#include <new>
#include "bzx_host.h"

struct bzx_cstream {
    bzx_ctx *ctx = nullptr;
    ChunkCaps c = {};
    ChunkLane L;
    ChunkAcct a;
    size_t carry_len = 0, carry_start = 0;  // raw bytes of the withheld block inside d_in[(k-1)&1]
    bool pend = false;                      // a chunk's output still sits in d_out[pend_slot]
    uint32_t pend_slot = 0, pend_nblk = 0;
    bool counted = false;                   // the caller's object (bzx_cstream_begin), counted in ctx->n_cstreams
};

// A block covers at most nblockMAX RLE1 bytes = nblockMAX / 5 runs of 255: the withheld raw tail never exceeds this.
static size_t cstream_max_carry(int level) { return ((size_t)100000 * level / 5 + 2) * 255 + 4096; }

// Sized for EVERY level: the one-shot calls keep their stream object and start the next stream on it at whatever level
// their caller asks for -- the withheld raw tail is longest at level 9, the blocks of a chunk are most numerous at
// level 1.
ChunkCaps chunk_caps(size_t max_chunk)
{
    ChunkCaps c;
    if (max_chunk == 0) max_chunk = (size_t)256 << 20;
    c.max_chunk = (max_chunk + 15) & ~(size_t)15;
    c.in_cap = c.max_chunk + cstream_max_carry(9) + 256;
    c.out_cap = (c.in_cap + c.in_cap / 50 + 65536) & ~(size_t)255;       // RLE1 +25 % never survives coding: 2 % + slack
    c.out_cap += c.in_cap / 4;
    c.blk_cap = (uint32_t)((c.in_cap + c.in_cap / 4) / ((size_t)100000 * 1 - 19) + 4);
    return c;
}

// beyond 128 MiB one block per compute unit (256 x 900,000 B on MI355X): the kernels that give a block one workgroup
// then run whole rounds (299 blocks of a 256 MiB chunk were 1.17 rounds, paid as two)
size_t buffer_chunk(size_t len, int n_cu, size_t chunk_min)
{
    size_t chunk = chunk_min;
    while (chunk < len && chunk < ((size_t)128 << 20)) chunk <<= 1;
    if (chunk < len) chunk = (size_t)(n_cu > 0 ? n_cu : 256) * 900000u;
    return chunk;
}

bool ChunkLane::alloc(size_t in_cap, size_t out_cap, uint32_t blk_cap)
{
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++) {
        ok = d_in[i].reserve(in_cap) && d_out[i].reserve(out_cap) &&
             hipEventCreateWithFlags(&ev_h2d[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ev_done[i], hipEventDisableTiming) == hipSuccess &&
             h_info[i].reserve(4 * sizeof(uint64_t)) && h_blk[i].reserve((size_t)blk_cap * sizeof(BzxBlock));
    }
    device_bytes = 2 * in_cap + 2 * out_cap + 4 * sizeof(uint64_t);
    pinned_bytes = 2 * (4 * sizeof(uint64_t) + (size_t)blk_cap * sizeof(BzxBlock)) + 16;
    return ok && hipEventCreateWithFlags(&ev_d2h, hipEventDisableTiming) == hipSuccess &&
           d_phase.reserve(4 * sizeof(uint64_t)) && h_w0.reserve(16) &&
           hipStreamCreateWithFlags(&s_h2d, hipStreamNonBlocking) == hipSuccess &&
           hipStreamCreateWithFlags(&s_d2h, hipStreamNonBlocking) == hipSuccess;
}

void ChunkLane::free()
{
    if (s_h2d) (void)hipStreamSynchronize(s_h2d);
    if (s_d2h) (void)hipStreamSynchronize(s_d2h);
    for (int i = 0; i < 2; i++) {              // (here, with the lane's device current: not left to the destructor)
        d_in[i].reset();
        d_out[i].reset();
        h_info[i].reset();
        h_blk[i].reset();
        if (ev_h2d[i]) (void)hipEventDestroy(ev_h2d[i]);
        if (ev_done[i]) (void)hipEventDestroy(ev_done[i]);
    }
    d_phase.reset();
    h_w0.reset();
    if (ev_d2h) (void)hipEventDestroy(ev_d2h);
    if (s_h2d) (void)hipStreamDestroy(s_h2d);
    if (s_d2h) (void)hipStreamDestroy(s_d2h);
}

void ChunkAcct::begin_output(uint8_t *out_, size_t cap_)
{
    if (k == 0) {
        memset(out_, 0, cap_ < 64 ? cap_ : 64);
        out_[0] = 'B'; out_[1] = 'Z'; out_[2] = 'h'; out_[3] = (uint8_t)('0' + level);
    }
    out = out_;
    cap = cap_;
}

// A pure function of the accounting (but for need_hint): the chunk starts at the bit the stream has reached.
int ChunkAcct::place_chunk(uint64_t cbits, ChunkPlace *p, std::string &err)
{
    p->phase = bits & 31u;
    p->nwords = (p->phase + cbits + 31) >> 5;
    p->off = (size_t)(bits >> 5) * 4;
    if (p->off + p->nwords * 4 > cap) {
        err = "output buffer too small for the compressed stream";
        need_hint = p->off + (size_t)((p->phase + cbits + 80 + 7) >> 3);
        return BZX_E_OUTBUF;
    }
    return BZX_OK;
}

// The first word is shared with the predecessor (or with nothing: then the bytes there are still zero).
void ChunkAcct::merge_first_word(const ChunkPlace &p, const uint32_t *h_w0)
{
    if (!p.nwords) return;
    uint8_t w[4];
    memcpy(w, h_w0, 4);
    if (p.phase == 0) memcpy(out + p.off, w, 4);
    else for (int i = 0; i < 4; i++) out[p.off + i] |= w[i];
}

int index_append(std::vector<bzx_index_entry> &idx, const BzxBlock *h_blk, uint32_t nblk, int level, uint64_t *bit,
                 uint64_t *raw_off)
{
    try {
        idx.reserve(idx.size() + nblk);
    } catch (const std::bad_alloc &) {
        return BZX_E_NOMEM;
    }
    for (uint32_t b = 0; b < nblk; b++) {
        bzx_index_entry e;
        memset(&e, 0, sizeof(e));
        e.bit = *bit;
        e.out_off = *raw_off;
        e.out_len = h_blk[b].raw_len;
        e.crc = h_blk[b].crc;
        e.img_bits = (uint32_t)h_blk[b].bits;
        e.level = (uint8_t)level;
        idx.push_back(e);
        *bit += h_blk[b].bits;
        *raw_off += h_blk[b].raw_len;
    }
    return BZX_OK;
}

// (the withheld last block of a non-final chunk is not among h_blk: its entry comes with the chunk that finishes it)
int ChunkAcct::account_chunk(const BzxBlock *h_blk, uint32_t nblk, uint64_t cbits, std::string &err)
{
    if (keep) {
        uint64_t bit = bits;
        if (index_append(idx, h_blk, nblk, level, &bit, &raw_off)) {
            err = "out of host memory for the block index";
            return BZX_E_NOMEM;
        }
    }
    fold_blocks(st, h_blk, 0, nblk, 1);
    for (uint32_t b = 0; b < nblk; b++) crc_comb = crc_fold(crc_comb, h_blk[b].crc);
    nblk_total += nblk;
    bits += cbits;
    return BZX_OK;
}

int ChunkAcct::get_index(const bzx_index_entry **entries, bzx_index_info *info) const
{
    if (!keep || sticky) return BZX_E_STATE;
    *entries = idx.data();
    memset(info, 0, sizeof(*info));
    info->nblk = idx.size();
    info->out_bytes = raw_off;
    info->in_bytes = finished ? stream_bytes : 0;
    info->nstreams = finished ? 1 : 0;
    return BZX_OK;
}

// Footer of a stream whose last block ends at bit `end`: magic, combined CRC (crc.rs:25-27), zero padding to a byte
// (bitwriter.rs:103-114,158-172); need = (end + 80 + 7) / 8 bytes of out are the stream.
static void stream_write_footer(uint8_t *out, uint64_t end, size_t need, uint32_t crc_comb)
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

int ChunkAcct::finish(size_t len, size_t *produced, std::string &err)
{
    const size_t need = (size_t)((bits + 80 + 7) >> 3);
    if (need > cap) {
        err = "output buffer too small for the compressed stream";
        need_hint = need;
        return BZX_E_OUTBUF;
    }
    stream_write_footer(out, bits, need, crc_comb);
    *produced = need;
    finished = true;
    stream_bytes = need;
    st.nblk = (uint32_t)nblk_total;
    st.raw_bytes += len;
    st.out_bits = (uint64_t)need * 8;
    return BZX_OK;
}

extern "C" void bzx_cstream_end(bzx_cstream *s)
{
    if (!s) return;
    if (s->ctx && s->counted) {
        std::unique_lock<std::recursive_mutex> api_lock_(s->ctx->api_mu);
        s->ctx->n_cstreams--;
    }
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    if (s->ctx) (void)hipStreamSynchronize(s->ctx->stream);
    s->L.free();
    delete s;
}

// The stream object of bzx_cstream_begin, and the one bzx_compress_buffer keeps in the context (the lock is held).
static int cstream_make(bzx_ctx *ctx, int level, size_t max_chunk, bzx_cstream **out)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bzx_cstream *s = new (std::nothrow) bzx_cstream();
    if (!s) return BZX_E_NOMEM;
    s->ctx = ctx;
    s->a.reset(level, ctx->keep_index);
    s->c = chunk_caps(max_chunk);
    if (!s->L.alloc(s->c.in_cap, s->c.out_cap, s->c.blk_cap) ||
        hipMemsetAsync(s->L.d_phase, 0, 4 * sizeof(uint64_t), ctx->stream) != hipSuccess) {
        ctx->err = "bzx_cstream_begin: device or pinned allocation failed";
        bzx_cstream_end(s);
        return BZX_E_NOMEM;
    }
    *out = s;
    return BZX_OK;
}

extern "C" int bzx_cstream_begin(bzx_ctx *ctx, int level, size_t max_chunk, bzx_cstream **out)
{
    if (!ctx || !out || !level_ok(level)) return BZX_E_PARAM;
    *out = nullptr;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    const int rc = cstream_make(ctx, level, max_chunk, out);
    if (rc == BZX_OK) {
        (*out)->counted = true;
        ctx->n_cstreams++;
    }
    return rc;
}

extern "C" int bzx_cstream_get_index(const bzx_cstream *s, const bzx_index_entry **entries, bzx_index_info *info)
{
    if (!s || !s->ctx || !entries || !info) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(s->ctx->api_mu);
    return s->a.get_index(entries, info);
}

extern "C" int bzx_ctx_keep_index(bzx_ctx *ctx, int on)
{
    if (!ctx) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    if (ctx->n_cstreams) {
        ctx->err = "bzx_ctx_keep_index: a bzx_cstream is open on this context: call bzx_cstream_end first";
        return BZX_E_STATE;
    }
    ctx->keep_index = on != 0;
    ctx->cidx_ok = ctx->bidx_ok = false;
    return BZX_OK;
}

extern "C" int bzx_compress_get_index(const bzx_ctx *ctx, const bzx_index_entry **entries, bzx_index_info *info)
{
    if (!ctx || !entries || !info) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(const_cast<bzx_ctx *>(ctx)->api_mu);
    if (!ctx->keep_index || !ctx->cidx_ok) return BZX_E_STATE;
    *entries = ctx->cidx.data();
    *info = ctx->cidx_info;
    return BZX_OK;
}

// Brings the output of the chunk parked in d_out[pend_slot] to the caller's buffer on the copy-back stream, merges the
// word it shares with its predecessor and folds its block CRCs.  The chunk's layout has completed when this is called,
// and it is called AFTER the next chunk's stages have been enqueued: the copy-back of chunk k-1 runs beside the
// compression of chunk k.
static int cstream_collect(bzx_cstream *s)
{
    bzx_ctx *ctx = s->ctx;
    if (!s->pend) return BZX_OK;
    ChunkLane &L = s->L;
    const uint32_t slot = s->pend_slot;
    // h_info = {phase the NEXT chunk starts with, bits of this chunk}; this chunk started at the phase the host
    // accounting says
    const uint64_t cbits = L.h_info[slot][1];
    if (L.h_info[slot][0] != (((s->a.bits & 31u) + cbits) & 31u)) {
        ctx->err = "chunked stream: bit phase out of step";
        return BZX_E_STATE;
    }
    ChunkPlace p;
    int rc = s->a.place_chunk(cbits, &p, ctx->err);
    if (rc) return rc;
    if (p.nwords * 4 > s->c.out_cap) {
        ctx->err = "chunk output larger than its device buffer";
        return BZX_E_HIP;
    }
    HIP_TRY(ctx, hipStreamWaitEvent(L.s_d2h, L.ev_done[slot], 0));
    if (p.nwords) {
        HIP_TRY(ctx, hipMemcpyAsync(L.h_w0, L.d_out[slot], 4, hipMemcpyDeviceToHost, L.s_d2h));
        if (p.nwords > 1)
            HIP_TRY(ctx, hipMemcpyAsync(s->a.out + p.off + 4, L.d_out[slot] + 1, (p.nwords - 1) * 4, hipMemcpyDeviceToHost, L.s_d2h));
    }
    HIP_TRY(ctx, hipEventRecord(L.ev_d2h, L.s_d2h));
    HIP_TRY(ctx, hipEventSynchronize(L.ev_d2h));
    s->a.merge_first_word(p, L.h_w0);
    // (bzx_get_block_info: the stream's descriptors in order, as far as the context's descriptor table reaches)
    for (uint32_t b = 0; b < s->pend_nblk && ctx->h_blk && s->a.nblk_total + b < ctx->cap_blocks; b++)
        ctx->h_blk[s->a.nblk_total + b] = L.h_blk[slot][b];
    const uint32_t nblk = s->pend_nblk;
    s->pend = false;
    return s->a.account_chunk(L.h_blk[slot], nblk, cbits, ctx->err);
}

// Back to the state after bzx_cstream_begin (buffers kept): a new stream on the same object.
static int cstream_reset(bzx_cstream *s, int level)
{
    bzx_ctx *ctx = s->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(s->L.s_h2d));
    HIP_TRY(ctx, hipStreamSynchronize(s->L.s_d2h));
    HIP_TRY(ctx, hipMemsetAsync(s->L.d_phase, 0, 4 * sizeof(uint64_t), ctx->stream));
    s->a.reset(level, ctx->keep_index);
    s->carry_len = s->carry_start = 0;
    s->pend = false;
    return BZX_OK;
}

static int cstream_feed(bzx_cstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap, size_t *produced)
{
    bzx_ctx *ctx = s->ctx;
    ChunkLane &L = s->L;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s->a.begin_output(out, cap);
    const uint32_t slot = s->a.k & 1u;
    const size_t total = s->carry_len + len;
    if (total > s->c.in_cap) {                     // (cannot happen with the provisioning above; never write past d_in)
        ctx->err = "chunked stream: withheld bytes + chunk exceed the device input buffer";
        return BZX_E_STATE;
    }
    // the device buffer of this slot was last read by chunk k-2; its kernels are long done when k-1's results were
    // collected, but the copy stream does not know that: make it wait
    if (s->a.k >= 2) HIP_TRY(ctx, hipStreamWaitEvent(L.s_h2d, L.ev_done[slot], 0));
    if (len) HIP_TRY(ctx, hipMemcpyAsync(L.d_in[slot] + s->carry_len, raw, len, hipMemcpyHostToDevice, L.s_h2d));
    HIP_TRY(ctx, hipEventRecord(L.ev_h2d[slot], L.s_h2d));
    if (s->carry_len)     // the withheld block's raw bytes move to the front of this chunk (after the kernels that read them)
        HIP_TRY(ctx, hipMemcpyAsync(L.d_in[slot], L.d_in[slot ^ 1u] + s->carry_start, s->carry_len, hipMemcpyDeviceToDevice,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, L.ev_h2d[slot], 0));
    uint32_t nblk = 0, use = 0;
    uint64_t last_start = 0;
    int rc = BZX_OK;
    if (total) {
        ctx->B.blk_first = 0;
        ctx->B.blk_step = 1;
        rc = split_on_device(ctx, L.d_in[slot], total, s->a.level, &nblk, 0, 1, &last_start);     // (synchronises)
        if (rc) return rc;
        use = final ? nblk : nblk - 1;
        if (use > s->c.blk_cap) {
            ctx->err = "chunked stream: more blocks in a chunk than provisioned";
            return BZX_E_HIP;
        }
    }
    // the previous chunk was laid out before this chunk's split ran: its sizes are on the host now
    if (!total) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // Chunk k's stages go into the queue FIRST; then the copy-back of chunk k-1 is issued on its own stream and awaited:
    // it runs beside the compression of chunk k (with a pageable destination the runtime stages the copy and blocks the
    // host while it lasts -- the device has its work by then).  An error of that chunk k-1 is found with the device
    // phase already moved on: the caller makes it sticky.
    if (use) {
        if ((rc = run_stages(ctx, use, STG_ALL, -1, L.d_out[slot], s->c.out_cap, L.d_phase))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(L.h_info[slot], L.d_phase, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(L.h_blk[slot], ctx->B.blk, (size_t)use * sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(L.ev_done[slot], ctx->stream));
    if ((rc = cstream_collect(s))) return rc;
    if (use) {
        s->pend = true;
        s->pend_slot = slot;
        s->pend_nblk = use;
    }
    if (!final && total) {
        s->carry_start = (size_t)last_start;
        s->carry_len = total - (size_t)last_start;
    } else {
        s->carry_len = s->carry_start = 0;
    }
    s->a.k++;
    if (!final) {
        s->a.st.raw_bytes += len;
        // bytes that can no longer change: everything before the word the next chunk starts in
        *produced = (size_t)(s->a.bits >> 5) * 4;
        return BZX_OK;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = cstream_collect(s))) return rc;
    collect_stage_times(ctx);
    if ((rc = s->a.finish(len, produced, ctx->err))) return rc;
    ctx->stats_batch = false;
    ctx->stats.nblk = s->a.st.nblk;
    ctx->stats.n_periodic = s->a.st.n_periodic;
    ctx->stats.rle1_bytes = s->a.st.rle1_bytes;
    ctx->stats.mtf_symbols = s->a.st.mtf_symbols;
    ctx->stats.raw_bytes = s->a.st.raw_bytes;
    ctx->stats.out_bits = s->a.st.out_bits;
    return BZX_OK;
}

extern "C" int bzx_cstream_feed(bzx_cstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap,
                                size_t *produced)
{
    if (!s || !s->ctx || !out || !produced || (len && !raw) || len > s->c.max_chunk || cap < 16) return BZX_E_PARAM;
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (s->a.finished) return BZX_E_STATE;
    if (s->a.sticky) return s->a.sticky;
    const int rc = cstream_feed(s, raw, len, final, out, cap, produced);
    if (rc) s->a.sticky = rc;
    return rc;
}

// Host buffer -> host buffer: the chunked stream compressor over the whole input (H2D of chunk k+1, compression of
// chunk k and D2H of chunk k-1 overlap; no device allocation per call: the stream object is kept in the context).
// Pinned caller buffers (hipHostMalloc / hipHostRegister / bzx_host_alloc) make the copies truly asynchronous.
extern "C" int bzx_compress_buffer(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, uint8_t *out, size_t cap,
                                   size_t *out_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (ctx) ctx->cidx_ok = false;
    if (!ctx || !out || !out_len || !level_ok(level) || (len && !raw) || cap < 16) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t chunk = buffer_chunk(len, ctx->n_cu, (size_t)16 << 20);      // (the emulator's smaller floor is bzx_mcompress_buffer's alone)
    int rc;
    if (ctx->cs && ctx->cs->c.max_chunk < chunk) {
        bzx_cstream_end(ctx->cs);
        ctx->cs = nullptr;
    }
    if (!ctx->cs) {
        if ((rc = cstream_make(ctx, level, chunk, &ctx->cs))) return rc;
    } else if ((rc = cstream_reset(ctx->cs, level))) {
        return rc;
    }
    chunk = ctx->cs->c.max_chunk;
    hipEvent_t e0 = ctx->ev[5], e1 = ctx->ev[7];
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    size_t off = 0, produced = 0;
    do {
        const size_t n = len - off < chunk ? len - off : chunk;
        const int fin = off + n == len;
        if ((rc = bzx_cstream_feed(ctx->cs, raw + off, n, fin, out, cap, &produced))) {
            if (rc == BZX_E_OUTBUF) *out_len = ctx->cs->a.need_hint;      // (a lower bound when chunks remain)
            return rc;
        }
        off += n;
    } while (off < len);
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&ctx->stats.ms_total, e0, e1);
    ctx->stats.raw_bytes = len;
    *out_len = produced;
    if (ctx->keep_index) {                      // the stream's entries move to the context (no copy; the stream object
        const bzx_index_entry *e;               // clears what it gets back when the next call starts it anew)
        if (ctx->cs->a.get_index(&e, &ctx->cidx_info) == BZX_OK) {
            ctx->cidx.swap(ctx->cs->a.idx);
            ctx->cidx_ok = true;
        }
    }
    return BZX_OK;
}
