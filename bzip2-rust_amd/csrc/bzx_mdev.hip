// bzx_mdev.hip -- one process, several devices, one .bz2 (include/bzx.h: bzx_mctx_*, bzx_mstream_*,
// bzx_mcompress_buffer) and the kernel that shifts a finished chunk to its bit phase.
//
// The scheme is that of bzx_cstream.hip, chunk by chunk: split "withheld raw tail + new bytes", compress all blocks but
// the last, make the chunk outputs bit-contiguous; the buffer sizes, the per-device resources (ChunkLane) and the host's
// accounting of the stream (ChunkAcct) are the ones defined there (bzx_host.h).  There the two things one chunk hands
// to the next stay on the device (the tail: a device-to-device copy; the bit phase: d_phase, read by
// bzx_layout_kernel); here chunk k runs on entry k mod ndev, so both go through the host:
//   needs                               from                                   known after
//   raw bytes of the withheld block     host tail buffer (refilled from the     split of chunk k-1 (it ends in a host
//                                       caller's bytes)                         synchronisation)
//   bit position of its first block     32 + bits of all earlier chunks         Huffman stage of chunk k-1
//   folded combined CRC, block count    host                                    descriptors of chunk k-1 on the host
// The splits form a short serial chain; BWT, MTF, Huffman AND emit of chunk k wait for nothing of chunk k-1: a chunk is
// laid out and emitted at bit phase 0 into a buffer of its own, and shifted to its real phase (bzx_shift_bits_kernel,
// on the entry's copy-back stream) once the host knows it.  One host thread issues everything.
#include <string.h>
#include <new>
#include "bzx_host.h"
#include "bzx_wg.h"

// ---- the shift kernel ------------------------------------------------------------------------------------------
// out = in shifted right by p bits (0..31) in byte-stream bit order (most significant bit of byte 0 first): with
// W[i] the big-endian value of word i, out word i = (W[i-1] << (32 - p)) | (W[i] >> p).  A lane moves one 16-byte
// vector per step; the word before its vector is the last word of the lane before it (one DPP move), lane 0 of a wave
// loads it.  Both buffers hold nvec whole vectors; the input is zero behind its last used word, so the vector that
// holds the extra word at the end needs no special case.  Streaming: no LDS, no reuse.
#define SH_NT 256

__device__ __forceinline__ uint32_t sh_funnel(uint32_t hi, uint32_t lo, uint32_t p)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> p);
}

__global__ __launch_bounds__(SH_NT) void bzx_shift_bits_kernel(const uint4 *__restrict__ in, uint32_t nvec, uint32_t p,
                                                               uint4 *__restrict__ out)
{
    const uint32_t lane = bzx_lane();
    const uint32_t stride = gridDim.x * SH_NT;
    // (the loop bound is the same for all lanes of a wave: every lane takes part in the cross-lane move)
    for (uint32_t base = blockIdx.x * SH_NT + (threadIdx.x & ~63u); base < nvec; base += stride) {
        const uint32_t t = base + lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t < nvec) v = in[t];
        const uint32_t w0 = __builtin_bswap32(v.x), w1 = __builtin_bswap32(v.y), w2 = __builtin_bswap32(v.z),
                       w3 = __builtin_bswap32(v.w);
        uint32_t prev = bzx_lane_prev(w3);
        if (lane == 0 && t > 0 && t < nvec) prev = __builtin_bswap32(((const uint32_t *)in)[(size_t)t * 4 - 1]);
        if (t < nvec)
            out[t] = make_uint4(__builtin_bswap32(sh_funnel(prev, w0, p)), __builtin_bswap32(sh_funnel(w0, w1, p)),
                                __builtin_bswap32(sh_funnel(w1, w2, p)), __builtin_bswap32(sh_funnel(w2, w3, p)));
    }
}

static inline uint32_t shift_vecs(uint32_t n_words) { return (n_words + 1 + 3) / 4; }

// n_words input words -> n_words + 1 output words; both buffers hold shift_vecs(n_words) * 16 bytes, 16-byte aligned.
void bzx_launch_shift_bits(const uint32_t *d_in, uint32_t n_words, uint32_t p, uint32_t *d_out, uint32_t n_cu,
                           hipStream_t stream)
{
    const uint32_t nvec = shift_vecs(n_words);
    uint32_t grid = (nvec + SH_NT - 1) / SH_NT;
    const uint32_t gmax = (n_cu ? n_cu : 256u) * 8u;
    if (grid > gmax) grid = gmax;
    hipLaunchKernelGGL(bzx_shift_bits_kernel, dim3(grid), dim3(SH_NT), 0, stream, (const uint4 *)d_in, nvec, p, (uint4 *)d_out);
}

extern "C" int bzx_stage_shift_bits(bzx_ctx *ctx, const uint8_t *in, size_t nbytes, uint32_t p, uint8_t *out)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !out || (nbytes && !in) || p > 31 || nbytes > 0x7fffffffu) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n_words = (uint32_t)((nbytes + 3) / 4);
    const size_t bytes = (size_t)shift_vecs(n_words) * 16;
    DevMem<uint32_t> d_a, d_b;               // (freed on return, behind the synchronisation below)
    if (!d_a.reserve(bytes) || !d_b.reserve(bytes)) {
        ctx->err = "bzx_stage_shift_bits: device allocation failed";
        return BZX_E_NOMEM;
    }
    hipError_t e = hipMemsetAsync(d_a, 0, bytes, ctx->stream);
    if (e == hipSuccess && nbytes) e = hipMemcpyAsync(d_a, in, nbytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        bzx_launch_shift_bits(d_a, n_words, p, d_b, (uint32_t)ctx->n_cu, ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_b, ((size_t)n_words + 1) * 4, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    HIP_TRY(ctx, e);
    HIP_TRY(ctx, e2);
    return BZX_OK;
}

// ---- the multi-device context and its chunked stream -----------------------------------------------------------
struct bzx_mctx {
    uint32_t ndev = 0;
    int device[BZX_MAX_DEVICES];
    bzx_ctx *ctx[BZX_MAX_DEVICES];
    std::recursive_mutex mu;
    std::string err;
    bzx_mstream *open = nullptr;     // the caller's open stream (bzx_mstream_begin .. _end)
    bzx_mstream *cs = nullptr;       // stream object kept for bzx_mcompress_buffer
    bzx_stats stats;
    bzx_mdev_info info;
    bool keep_index = false;         // bzx_mctx_keep_index
    bool cidx_ok = false;            // cidx / cidx_info describe the last bzx_mcompress_buffer call
    std::vector<bzx_index_entry> cidx;
    bzx_index_info cidx_info = {};
};

struct MEntry {
    ChunkLane L;                                  // d_out: the chunk at bit phase 0; d_phase: zeroed before every chunk
    DevMem<uint32_t> d_shift;                     // ... shifted to its phase in the stream
    uint32_t pend_nblk[2] = {0, 0};
    bool timed = false;                           // the stage events of the context belong to a chunk not yet accounted for
};

struct bzx_mstream {
    bzx_mctx *m = nullptr;
    ChunkCaps c = {};                        // (out_cap rounded up to whole vectors of the shift kernel)
    ChunkAcct a;
    MEntry ent[BZX_MAX_DEVICES];
    PinMem<uint8_t> h_tail;                  // raw bytes of the withheld block
    size_t tail_cap = 0, tail_len = 0;
    uint32_t k_coll = 0;                     // chunks collected (in order; a.k: chunks fed)
};

static std::string entry_name(const bzx_mctx *m, uint32_t e)
{
    return "devices[" + std::to_string(e) + "] (device " + std::to_string(m->device[e]) + "): ";
}

#define M_TRY(m, e, expr)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (m)->err = entry_name(m, e) + #expr + ": " + hipGetErrorString(e_);                 \
            return BZX_E_HIP;                                                                   \
        }                                                                                       \
    } while (0)

// an error of the entry's private context, reported under the entry's name
static int ctx_failed(bzx_mctx *m, uint32_t e, int rc)
{
    m->err = entry_name(m, e) + m->ctx[e]->err;
    return rc;
}

extern "C" const char *bzx_mctx_last_error(const bzx_mctx *m) { return m ? m->err.c_str() : ""; }

extern "C" void bzx_mctx_destroy(bzx_mctx *m)
{
    if (!m) return;
    if (m->cs) bzx_mstream_end(m->cs);
    if (m->open) bzx_mstream_end(m->open);
    for (uint32_t e = 0; e < m->ndev; e++)
        if (m->ctx[e]) bzx_ctx_destroy(m->ctx[e]);
    delete m;
}

extern "C" int bzx_mctx_create(const int *devices, uint32_t ndev, uint32_t max_blocks, bzx_mctx **out)
{
    if (!out) return BZX_E_PARAM;
    *out = nullptr;
    if (!devices || ndev == 0 || ndev > BZX_MAX_DEVICES) return BZX_E_PARAM;
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return BZX_E_NODEVICE;
    for (uint32_t e = 0; e < ndev; e++)
        if (devices[e] < 0 || devices[e] >= have) return BZX_E_NODEVICE;
    bzx_mctx *m = new (std::nothrow) bzx_mctx();
    if (!m) return BZX_E_NOMEM;
    memset(&m->stats, 0, sizeof(m->stats));
    memset(&m->info, 0, sizeof(m->info));
    memset(m->ctx, 0, sizeof(m->ctx));
    for (uint32_t e = 0; e < ndev; e++) {
        m->device[e] = devices[e];
        const int rc = bzx_ctx_create(devices[e], max_blocks, &m->ctx[e]);
        if (rc) {
            bzx_mctx_destroy(m);
            return rc;
        }
        m->ndev = e + 1;
    }
    m->info.ndev = ndev;
    for (uint32_t e = 0; e < ndev; e++) m->info.dev[e].device = devices[e];
    *out = m;
    return BZX_OK;
}

extern "C" int bzx_mctx_get_stats(const bzx_mctx *m, bzx_stats *out)
{
    if (!m || !out) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> lock_(const_cast<bzx_mctx *>(m)->mu);
    *out = m->stats;
    return BZX_OK;
}

extern "C" int bzx_mctx_get_info(const bzx_mctx *m, bzx_mdev_info *out)
{
    if (!m || !out) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> lock_(const_cast<bzx_mctx *>(m)->mu);
    *out = m->info;
    return BZX_OK;
}

// Waits for everything the stream has in flight and frees it (the lock is held, or nobody else knows the object).
static void mstream_free(bzx_mstream *s)
{
    bzx_mctx *m = s->m;
    for (uint32_t e = 0; e < m->ndev; e++) {
        MEntry &E = s->ent[e];
        (void)hipSetDevice(m->device[e]);
        (void)hipStreamSynchronize(m->ctx[e]->stream);
        E.L.free();
        E.d_shift.reset();                   // (with its device current; `delete` frees the tail buffer)
    }
    delete s;
}

extern "C" void bzx_mstream_end(bzx_mstream *s)
{
    if (!s || !s->m) return;
    bzx_mctx *m = s->m;
    std::unique_lock<std::recursive_mutex> lock_(m->mu);
    if (m->open == s) m->open = nullptr;
    if (m->cs == s) m->cs = nullptr;
    mstream_free(s);
}

// The figures of a stream that starts now.
static void mstream_reset_counts(bzx_mstream *s, int level)
{
    bzx_mctx *m = s->m;
    s->a.reset(level, m->keep_index);
    s->k_coll = 0;
    s->tail_len = 0;
    m->info.chunks = m->info.shifted = 0;
    m->info.nblk = 0;
    for (uint32_t e = 0; e < m->ndev; e++) {
        s->ent[e].pend_nblk[0] = s->ent[e].pend_nblk[1] = 0;
        s->ent[e].timed = false;
        m->info.dev[e].chunks = 0;
        m->info.dev[e].blocks = 0;
        m->info.dev[e].ms_device = 0.f;
    }
}

static int mstream_make(bzx_mctx *m, int level, size_t max_chunk, bzx_mstream **out)
{
    bzx_mstream *s = new (std::nothrow) bzx_mstream();
    if (!s) return BZX_E_NOMEM;
    s->m = m;
    s->c = chunk_caps(max_chunk);
    s->c.out_cap = (s->c.out_cap + 255) & ~(size_t)255;      // the shift kernel moves whole 16-byte vectors
    s->tail_cap = s->c.in_cap - s->c.max_chunk;               // the longest withheld tail + slack
    // Read by every entry's device: asked for as portable explicitly (as bzx_host_alloc does for the callers' buffers).
    // The runtime's header calls the default flag "the same definition" as the portable one, but that is a comment, not
    // a promise, and a machine with one device cannot show the difference.
    bool ok = s->h_tail.reserve(s->tail_cap, BZX_HOST_PORTABLE);
    uint32_t bad = 0;
    for (uint32_t e = 0; e < m->ndev && ok; e++) {
        MEntry &E = s->ent[e];
        bad = e;
        ok = hipSetDevice(m->device[e]) == hipSuccess && E.L.alloc(s->c.in_cap, s->c.out_cap, s->c.blk_cap) &&
             E.d_shift.reserve(s->c.out_cap);
        m->info.dev[e].device_bytes = ok ? E.L.device_bytes + s->c.out_cap : 0;
        m->info.dev[e].pinned_bytes = ok ? E.L.pinned_bytes + (e == 0 ? s->tail_cap : 0) : 0;      // (the one tail buffer is counted with entry 0)
    }
    if (!ok) {
        m->err = entry_name(m, bad) + "bzx_mstream_begin: device or page-locked allocation failed";
        mstream_free(s);
        return BZX_E_NOMEM;
    }
    mstream_reset_counts(s, level);
    *out = s;
    return BZX_OK;
}

extern "C" int bzx_mstream_begin(bzx_mctx *m, int level, size_t max_chunk, bzx_mstream **out)
{
    if (!m || !out || !level_ok(level)) return BZX_E_PARAM;
    *out = nullptr;
    std::unique_lock<std::recursive_mutex> lock_(m->mu);
    if (m->open) {
        m->err = "a bzx_mstream is open on this bzx_mctx: call bzx_mstream_end first";
        return BZX_E_STATE;
    }
    const int rc = mstream_make(m, level, max_chunk, out);
    if (rc == BZX_OK) m->open = *out;
    return rc;
}

// Accounts for the stage events of the entry's last chunk (complete: its stream was synchronised behind them).
static void entry_times(bzx_mstream *s, uint32_t e)
{
    bzx_mctx *m = s->m;
    MEntry &E = s->ent[e];
    if (!E.timed) return;
    E.timed = false;
    bzx_ctx *ctx = m->ctx[e];
    float ms[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ctx->ev[i], ctx->ev[i + 1]);
    s->a.st.ms_bwt += ms[0];
    s->a.st.ms_mtf += ms[1];
    s->a.st.ms_huffman += ms[2];
    s->a.st.ms_emit += ms[3];
    m->info.dev[e].ms_device += ms[0] + ms[1] + ms[2] + ms[3];
}

// Brings chunk j (the oldest one not collected) to the caller's buffer: waits for its stages, shifts it to its bit
// phase if that is not 0, copies it back, merges the word it shares with its predecessor -- whose copy-back has
// completed, since chunks are collected one after the other -- and folds its block CRCs.
static int mstream_collect(bzx_mstream *s, uint32_t j)
{
    bzx_mctx *m = s->m;
    const uint32_t e = j % m->ndev, slot = (j / m->ndev) & 1u;
    MEntry &E = s->ent[e];
    ChunkLane &L = E.L;
    const uint32_t nblk = E.pend_nblk[slot];
    E.pend_nblk[slot] = 0;
    if (!nblk) return BZX_OK;
    M_TRY(m, e, hipSetDevice(m->device[e]));
    M_TRY(m, e, hipEventSynchronize(L.ev_done[slot]));
    const uint64_t cbits = L.h_info[slot][1];
    if (L.h_info[slot][0] != (cbits & 31u)) {
        m->err = entry_name(m, e) + "chunk laid out at a bit phase other than 0";
        return BZX_E_STATE;
    }
    ChunkPlace p;
    int rc = s->a.place_chunk(cbits, &p, m->err);
    if (rc) return rc;
    const uint64_t n_in = (cbits + 31) >> 5;
    if ((uint64_t)shift_vecs((uint32_t)n_in) * 16 > s->c.out_cap || n_in > 0x7ffffff0u) {
        m->err = entry_name(m, e) + "chunk output larger than its device buffer";
        return BZX_E_HIP;
    }
    const uint32_t *src = L.d_out[slot];
    M_TRY(m, e, hipStreamWaitEvent(L.s_d2h, L.ev_done[slot], 0));
    if (p.phase) {
        bzx_launch_shift_bits(L.d_out[slot], (uint32_t)n_in, (uint32_t)p.phase, E.d_shift, (uint32_t)m->ctx[e]->n_cu, L.s_d2h);
        M_TRY(m, e, hipGetLastError());
        src = E.d_shift;
        m->info.shifted++;
    }
    M_TRY(m, e, hipMemcpyAsync(L.h_w0, src, 4, hipMemcpyDeviceToHost, L.s_d2h));
    if (p.nwords > 1) M_TRY(m, e, hipMemcpyAsync(s->a.out + p.off + 4, src + 1, (p.nwords - 1) * 4, hipMemcpyDeviceToHost, L.s_d2h));
    M_TRY(m, e, hipEventRecord(L.ev_d2h, L.s_d2h));
    M_TRY(m, e, hipEventSynchronize(L.ev_d2h));
    s->a.merge_first_word(p, L.h_w0);
    if ((rc = s->a.account_chunk(L.h_blk[slot], nblk, cbits, m->err))) return rc;
    m->info.nblk = s->a.nblk_total;
    return BZX_OK;
}

static int mstream_feed(bzx_mstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap, size_t *produced)
{
    bzx_mctx *m = s->m;
    const uint32_t N = m->ndev, k = s->a.k, e = k % N, slot = (k / N) & 1u;
    MEntry &E = s->ent[e];
    ChunkLane &L = E.L;
    bzx_ctx *ctx = m->ctx[e];
    s->a.begin_output(out, cap);
    const size_t total = s->tail_len + len;
    if (total > s->c.in_cap) {                   // (cannot happen with the provisioning of begin; never write past d_in)
        m->err = "withheld bytes + chunk exceed the device input buffer";
        return BZX_E_STATE;
    }
    M_TRY(m, e, hipSetDevice(m->device[e]));
    // the buffers of this slot were last used by chunk k - 2 ndev: collected by now, but the copy stream does not know
    if (k >= 2 * N) M_TRY(m, e, hipStreamWaitEvent(L.s_h2d, L.ev_done[slot], 0));
    if (s->tail_len) M_TRY(m, e, hipMemcpyAsync(L.d_in[slot], s->h_tail, s->tail_len, hipMemcpyHostToDevice, L.s_h2d));
    if (len) M_TRY(m, e, hipMemcpyAsync(L.d_in[slot] + s->tail_len, raw, len, hipMemcpyHostToDevice, L.s_h2d));
    M_TRY(m, e, hipEventRecord(L.ev_h2d[slot], L.s_h2d));
    M_TRY(m, e, hipStreamWaitEvent(ctx->stream, L.ev_h2d[slot], 0));
    uint32_t nblk = 0, use = 0;
    uint64_t last_start = 0;
    int rc = BZX_OK;
    if (total) {
        ctx->B.blk_first = 0;
        ctx->B.blk_step = 1;
        // (synchronises the entry's stream: its chunk k - ndev is complete and both copies above have been read)
        if ((rc = split_on_device(ctx, L.d_in[slot], total, s->a.level, &nblk, 0, 1, &last_start))) return ctx_failed(m, e, rc);
        use = final ? nblk : nblk - 1;
        if (use > s->c.blk_cap) {
            m->err = entry_name(m, e) + "more blocks in a chunk than provisioned";
            return BZX_E_HIP;
        }
    } else {
        M_TRY(m, e, hipStreamSynchronize(ctx->stream));
    }
    entry_times(s, e);
    // the tail of the next chunk: the raw bytes from the start of this chunk's last block, kept on the host
    if (!final && total) {
        const size_t ls = (size_t)last_start, keep = total - ls;
        if (ls > total || keep > s->tail_cap) {
            m->err = "withheld block longer than the tail buffer";
            return BZX_E_STATE;
        }
        if (ls >= s->tail_len) {
            memcpy(s->h_tail, raw + (ls - s->tail_len), keep);
        } else {
            memmove(s->h_tail, s->h_tail + ls, s->tail_len - ls);
            if (len) memcpy(s->h_tail + (s->tail_len - ls), raw, len);
        }
        s->tail_len = keep;
    } else {
        s->tail_len = 0;
    }
    if (use) {
        M_TRY(m, e, hipMemsetAsync(L.d_phase, 0, 4 * sizeof(uint64_t), ctx->stream));
        if ((rc = run_stages(ctx, use, STG_ALL, -1, L.d_out[slot], s->c.out_cap, L.d_phase))) return ctx_failed(m, e, rc);
        M_TRY(m, e, hipMemcpyAsync(L.h_info[slot], L.d_phase, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        M_TRY(m, e, hipMemcpyAsync(L.h_blk[slot], ctx->B.blk, (size_t)use * sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
        E.timed = true;
        m->info.dev[e].chunks++;
        m->info.dev[e].blocks += use;
    }
    M_TRY(m, e, hipEventRecord(L.ev_done[slot], ctx->stream));
    E.pend_nblk[slot] = use;
    s->a.k = k + 1;
    m->info.chunks = s->a.k;
    // Chunk k's stages are in the queue; now collect, in order, what is known to be complete: chunk k - ndev, the one
    // the split above waited for.  Its copy-back runs beside the compression of the chunks after it.
    while (s->k_coll + N <= k)
        if ((rc = mstream_collect(s, s->k_coll++))) return rc;
    if (!final) {
        s->a.st.raw_bytes += len;
        *produced = (size_t)(s->a.bits >> 5) * 4;
        return BZX_OK;
    }
    while (s->k_coll <= k)
        if ((rc = mstream_collect(s, s->k_coll++))) return rc;
    float ms_max = 0.f;
    for (uint32_t i = 0; i < N; i++) {
        if (s->ent[i].timed) M_TRY(m, i, hipSetDevice(m->device[i]));
        entry_times(s, i);
        if (m->info.dev[i].ms_device > ms_max) ms_max = m->info.dev[i].ms_device;
    }
    if ((rc = s->a.finish(len, produced, m->err))) return rc;
    s->a.st.ms_total = ms_max;
    m->stats = s->a.st;
    return BZX_OK;
}

extern "C" int bzx_mstream_feed(bzx_mstream *s, const uint8_t *raw, size_t len, int final, uint8_t *out, size_t cap,
                                size_t *produced)
{
    if (!s || !s->m || !out || !produced || (len && !raw) || len > s->c.max_chunk || cap < 16) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> lock_(s->m->mu);
    if (s->a.finished) return BZX_E_STATE;
    if (s->a.sticky) return s->a.sticky;
    const int rc = mstream_feed(s, raw, len, final, out, cap, produced);
    if (rc) s->a.sticky = rc;
    return rc;
}

// Host buffer -> host buffer over all entries: a loop over feed (the chunk rule is stated in include/bzx.h).
extern "C" int bzx_mcompress_buffer(bzx_mctx *m, const uint8_t *raw, size_t len, int level, uint8_t *out, size_t cap,
                                    size_t *out_len)
{
    if (!m || !out || !out_len || !level_ok(level) || (len && !raw) || cap < 16) {
        if (m) {
            std::unique_lock<std::recursive_mutex> lock_(m->mu);
            m->cidx_ok = false;
        }
        return BZX_E_PARAM;
    }
    std::unique_lock<std::recursive_mutex> lock_(m->mu);
    m->cidx_ok = false;
    if (m->open) {
        m->err = "a bzx_mstream is open on this bzx_mctx: call bzx_mstream_end first";
        return BZX_E_STATE;
    }
    int n_cu = m->ctx[0]->n_cu;
    for (uint32_t e = 1; e < m->ndev; e++)
        if (m->ctx[e]->n_cu < n_cu) n_cu = m->ctx[e]->n_cu;
    const size_t chunk = buffer_chunk((len + m->ndev - 1) / m->ndev, n_cu, BZX_MBUF_CHUNK_MIN);
    int rc;
    if (m->cs && m->cs->c.max_chunk < chunk) bzx_mstream_end(m->cs);      // (clears m->cs)
    if (!m->cs) {
        if ((rc = mstream_make(m, level, chunk, &m->cs))) return rc;
    } else {
        // back to the state after begin (buffers kept); nothing of the last stream is in flight after its final feed,
        // but it may have ended in an error
        for (uint32_t e = 0; e < m->ndev; e++) {
            M_TRY(m, e, hipSetDevice(m->device[e]));
            M_TRY(m, e, hipStreamSynchronize(m->ctx[e]->stream));
            M_TRY(m, e, hipStreamSynchronize(m->cs->ent[e].L.s_h2d));
            M_TRY(m, e, hipStreamSynchronize(m->cs->ent[e].L.s_d2h));
        }
        mstream_reset_counts(m->cs, level);
    }
    bzx_mstream *s = m->cs;      // (may be sized for a larger chunk by an earlier call: the chunk stays the rule's)
    size_t off = 0, produced = 0;
    do {
        const size_t n = len - off < chunk ? len - off : chunk;
        const int fin = off + n == len;
        if ((rc = bzx_mstream_feed(s, raw + off, n, fin, out, cap, &produced))) {
            if (rc == BZX_E_OUTBUF) *out_len = s->a.need_hint;      // (a lower bound when chunks remain)
            return rc;
        }
        off += n;
    } while (off < len);
    *out_len = produced;
    if (m->keep_index) {                         // the stream's entries move to the bzx_mctx (bzx_compress_buffer likewise)
        const bzx_index_entry *e;
        if (s->a.get_index(&e, &m->cidx_info) == BZX_OK) {
            m->cidx.swap(s->a.idx);
            m->cidx_ok = true;
        }
    }
    return BZX_OK;
}

extern "C" int bzx_mctx_keep_index(bzx_mctx *m, int on)
{
    if (!m) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> lock_(m->mu);
    if (m->open) {
        m->err = "bzx_mctx_keep_index: a bzx_mstream is open on this bzx_mctx: call bzx_mstream_end first";
        return BZX_E_STATE;
    }
    for (uint32_t e = 0; e < m->ndev; e++) {
        const int rc = bzx_ctx_keep_index(m->ctx[e], on);
        if (rc) return ctx_failed(m, e, rc);
    }
    m->keep_index = on != 0;
    m->cidx_ok = false;
    return BZX_OK;
}

extern "C" int bzx_mctx_get_index(const bzx_mctx *m, const bzx_index_entry **entries, bzx_index_info *info)
{
    if (!m || !entries || !info) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> lock_(const_cast<bzx_mctx *>(m)->mu);
    if (!m->keep_index || !m->cidx_ok) return BZX_E_STATE;
    *entries = m->cidx.data();
    *info = m->cidx_info;
    return BZX_OK;
}

extern "C" int bzx_mstream_get_index(const bzx_mstream *s, const bzx_index_entry **entries, bzx_index_info *info)
{
    if (!s || !s->m || !entries || !info) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> lock_(s->m->mu);
    return s->a.get_index(entries, info);
}
