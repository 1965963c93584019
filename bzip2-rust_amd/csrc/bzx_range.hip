// bzx_range.hip -- random access on gfx950 (include/bzx.h: bzx_index_span, bzx_decompress_range_*, bzx_stage_ibwt):
// bytes [off, off + want) of what a .bz2 decodes to, from a block index (bzx_index_*, bzx_dstream.hip) and the input
// bytes of the covering blocks alone.
//
// No magic scan and no chain walk: the covering entries become BzxDcSrc triples directly.  Per round of at most R
// blocks (R = the context's slabs):
//   decode        bzx_dc_decode_kernel through the triples
//   inverse BWT   the many-lane walk (bzx_launch_dc_ibwt_wide): a range touches one to three blocks, which have nothing
//                 to hide a one-lane pointer chase behind
//   check         bzx_rg_check_kernel: is the block magic where the entry says, and is the expanded length the
//                 entry's?  A block that fails is neither expanded nor summed (its destination is sized by the entry)
//   expand, CRC   blocks wholly inside the range at their final place in the output, the at most two edge blocks of
//                 the range into staging areas of their own
//   [sync]        descriptors, CRCs and flags; the host holds every block against its entry, then the slices of the
//                 edge blocks are copied from their staging areas
// One host synchronisation per round; nothing leaves through _buffer before every block of the range has passed.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bzx_host.h"

#define RG_EDGE_BYTES ((size_t)(BZX_MAX_N / 5 * 259 + 16))      // an expanded block: 259/5 x 900,000, rounded up
#define RG_NO_MAGIC 1u
#define RG_LENGTH 2u

// One lane per block, behind the inverse BWT.
__global__ __launch_bounds__(64) void bzx_rg_check_kernel(BzxBatch B, const BzxDcSrc *__restrict__ src,
                                                         const uint32_t *__restrict__ want_len, uint32_t *__restrict__ flag)
{
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B.nblk) return;
    const BzxDcSrc s = src[b];
    uint64_t v = 0;
    for (uint32_t i = 0; i < 7; i++) v = (v << 8) | (s.bit / 8 + i < s.nbytes ? s.z[s.bit / 8 + i] : 0u);
    uint32_t f = 0;
    if (((v >> (8 - (s.bit & 7u))) & 0xFFFFFFFFFFFFull) != DC_MAGIC_BLOCK) f |= RG_NO_MAGIC;
    else if (!B.blk[b].status && B.blk[b].pack_word != want_len[b]) f |= RG_LENGTH;
    flag[b] = f;
    if (f) B.blk[b].status |= DC_SKIP;
}

static uint64_t rg_total(const bzx_index_entry *e, uint64_t n) { return n ? e[n - 1].out_off + e[n - 1].out_len : 0; }

extern "C" int bzx_index_span(const bzx_index_entry *e, uint64_t n, uint64_t off, uint64_t want, uint64_t *first,
                              uint64_t *count, uint64_t *byte_lo, uint64_t *byte_hi)
{
    if ((n && !e) || !first || !count || !byte_lo || !byte_hi) return BZX_E_PARAM;
    *first = *count = *byte_lo = *byte_hi = 0;
    const uint64_t total = rg_total(e, n);
    if (want == 0 || off >= total) return BZX_OK;
    const uint64_t end = want < total - off ? off + want : total;
    // first entry that ends behind off, last entry that starts before end (blocks are never empty)
    const bzx_index_entry *a = std::upper_bound(e, e + n, off, [](uint64_t v, const bzx_index_entry &x) {
        return v < x.out_off + x.out_len;
    });
    const bzx_index_entry *z = std::lower_bound(e, e + n, end, [](const bzx_index_entry &x, uint64_t v) {
        return x.out_off < v;
    });
    if (a >= z || a->out_off > off) return BZX_E_PARAM;          // (entries that are not in output order)
    *first = (uint64_t)(a - e);
    *count = (uint64_t)(z - a);
    *byte_lo = a->bit / 8;
    *byte_hi = (z[-1].bit + z[-1].img_bits + 7) / 8 + 8;
    return BZX_OK;
}

// Round tables: device [src R][dst R][want_len R][got R][flag R], pinned [got R][flag R]; behind them on the device the
// two edge staging areas.
struct RgTables {
    BzxDcSrc *d_src;
    BzxDcDst *d_dst;
    uint32_t *d_len, *d_got, *d_flag, *h_got, *h_flag;
    uint8_t *edge[2];
};

static size_t rg_al(size_t x) { return (x + 255) & ~(size_t)255; }

static int rg_tables(bzx_ctx *ctx, uint32_t R, RgTables *t)
{
    if (R > ctx->range_slabs) {
        if (ctx->range_ws) (void)hipFree(ctx->range_ws);
        if (ctx->range_pin) (void)hipHostFree(ctx->range_pin);
        ctx->range_ws = ctx->range_pin = nullptr;
        ctx->range_slabs = 0;
        const size_t dev = rg_al(R * sizeof(BzxDcSrc)) + rg_al(R * sizeof(BzxDcDst)) + 3 * rg_al((size_t)R * 4) + 2 * rg_al(RG_EDGE_BYTES);
        if (hipMalloc(&ctx->range_ws, dev) != hipSuccess || hipHostMalloc(&ctx->range_pin, 2 * rg_al((size_t)R * 4), 0) != hipSuccess) {
            if (ctx->range_ws) (void)hipFree(ctx->range_ws);
            ctx->range_ws = nullptr;
            ctx->err = "range read: device or pinned allocation failed";
            return BZX_E_NOMEM;
        }
        ctx->range_slabs = R;
    }
    R = ctx->range_slabs;
    uint8_t *q = (uint8_t *)ctx->range_ws;
    t->d_src = (BzxDcSrc *)q;
    q += rg_al(R * sizeof(BzxDcSrc));
    t->d_dst = (BzxDcDst *)q;
    q += rg_al(R * sizeof(BzxDcDst));
    t->d_len = (uint32_t *)q;
    q += rg_al((size_t)R * 4);
    t->d_got = (uint32_t *)q;                  // (got and flag lie side by side: one copy brings both)
    q += rg_al((size_t)R * 4);
    t->d_flag = (uint32_t *)q;
    q += rg_al((size_t)R * 4);
    t->edge[0] = q;
    t->edge[1] = q + rg_al(RG_EDGE_BYTES);
    t->h_got = (uint32_t *)ctx->range_pin;
    t->h_flag = (uint32_t *)((uint8_t *)ctx->range_pin + rg_al((size_t)R * 4));
    return BZX_OK;
}

// The _buffer form's device buffer k of at least `bytes` bytes: kept by the context, grown when a call needs more.
static int rg_io(bzx_ctx *ctx, int k, size_t bytes, void **p)
{
    if (bytes > ctx->range_io_bytes[k]) {
        if (ctx->range_io[k]) (void)hipFree(ctx->range_io[k]);
        ctx->range_io[k] = nullptr;
        ctx->range_io_bytes[k] = 0;
        const size_t want = std::max<size_t>(bytes, (size_t)4 << 20);      // (a 900k block's span and a few MB of output)
        if (hipMalloc(&ctx->range_io[k], want) != hipSuccess) {
            ctx->err = k ? "range read: hipMalloc(output) failed" : "range read: hipMalloc(span) failed";
            return BZX_E_NOMEM;
        }
        ctx->range_io_bytes[k] = want;
    }
    *p = ctx->range_io[k];
    return BZX_OK;
}

static int rg_refuse(bzx_ctx *ctx, const std::string &why)
{
    ctx->err = why;
    return BZX_E_DATA;
}

// Entries e[first, first + count) cover output bytes [lo, hi); d_z[0, zlen) holds input bytes [zbase, zbase + zlen).
// d_out receives [lo, hi).
static int range_run(bzx_ctx *ctx, const uint8_t *d_z, size_t zlen, uint64_t zbase, const bzx_index_entry *e, uint64_t first,
                     uint64_t count, uint64_t lo, uint64_t hi, uint8_t *d_out)
{
    hipStream_t st = ctx->stream;
    int rc = ensure_blocks(ctx, 1);              // (a context holds 16 slabs at least from bzx_ctx_create on: nothing grows)
    if (rc) return rc;
    const uint32_t R = ctx->cap_slabs;
    RgTables t;
    if ((rc = rg_tables(ctx, R, &t))) return rc;
    BzxBatch &B = ctx->B;
    B.blk_first = 0;
    B.blk_step = 1;
    std::vector<BzxDcSrc> src(R);
    std::vector<BzxDcDst> dst(R);
    std::vector<uint32_t> len(R);
    struct Edge { uint64_t k; uint32_t area; };
    uint32_t areas = 0;
    for (uint64_t k0 = first; k0 < first + count; k0 += R) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(R, first + count - k0);
        std::vector<Edge> edges;
        uint32_t n_hint = 0;                                 // an image is at most 5/4 of what it expands to
        for (uint32_t j = 0; j < nb; j++) {
            const bzx_index_entry &x = e[k0 + j];
            n_hint = std::max<uint32_t>(n_hint, (uint32_t)std::min<uint64_t>(BZX_MAX_N, (uint64_t)x.out_len * 5 / 4 + 8));
            src[j] = BzxDcSrc{d_z, zlen, x.bit - zbase * 8};
            len[j] = x.out_len;
            if (x.out_len > RG_EDGE_BYTES - 16) return rg_refuse(ctx, "index does not match the input: an entry's out_len exceeds a block");
            if (x.out_off >= lo && x.out_off + x.out_len <= hi) {
                dst[j] = BzxDcDst{d_out + (x.out_off - lo), x.out_len};
            } else {                                         // an edge of the range: at most two in all
                if (areas >= 2) {
                    ctx->err = "range read: more than two edge blocks";
                    return BZX_E_STATE;
                }
                edges.push_back(Edge{k0 + j, areas});
                dst[j] = BzxDcDst{t.edge[areas++], x.out_len};
            }
        }
        B.nblk = nb;
        HIP_TRY(ctx, hipMemcpyAsync(t.d_src, src.data(), nb * sizeof(BzxDcSrc), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(t.d_dst, dst.data(), nb * sizeof(BzxDcDst), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(t.d_len, len.data(), nb * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(t.d_got, 0, (size_t)((uint8_t *)(t.d_flag + nb) - (uint8_t *)t.d_got), st));
        bzx_launch_dc_decode(B, t.d_src, st);
        bzx_launch_dc_ibwt_wide(B, ctx->d_in, n_hint, st);
        hipLaunchKernelGGL(bzx_rg_check_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, B, t.d_src, t.d_len, t.d_flag);
        bzx_launch_dc_expand(B, ctx->d_in, t.d_dst, st);
        bzx_launch_dc_crc(B, t.d_dst, t.d_got, (uint32_t)ctx->n_cu, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, B.blk, nb * sizeof(BzxBlock), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(t.h_got, t.d_got, nb * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(t.h_flag, t.d_flag, nb * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));              // the round's one synchronisation
        for (uint32_t j = 0; j < nb; j++) {
            const bzx_index_entry &x = e[k0 + j];
            const BzxBlock &d = ctx->h_blk[j];
            const std::string blk = " (block " + std::to_string(k0 + j) + ")";
            if (t.h_flag[j] & RG_NO_MAGIC)
                return rg_refuse(ctx, "index does not match the input: no block magic at bit " + std::to_string(x.bit) + blk);
            const uint32_t status = d.status & ~DC_SKIP;
            if (status & BZX_ST_DC_RANDOMISED) return rg_refuse(ctx, dc_why_text(DC_WHY_RANDOMISED));
            if (status) return rg_refuse(ctx, dc_why_text(DC_WHY_DAMAGED) + blk);
            if (d.crc != x.crc) return rg_refuse(ctx, "index does not match the input: another stored CRC" + blk);
            if (d.n > 100000u * x.level) return rg_refuse(ctx, "index does not match the input: the block is longer than its level allows" + blk);
            if ((uint32_t)(d.bits - d.out_bit) != x.img_bits)
                return rg_refuse(ctx, "index does not match the input: another block size" + blk);
            if (t.h_flag[j] & RG_LENGTH) return rg_refuse(ctx, "index does not match the input: another decoded length" + blk);
            if (t.h_got[j] != d.crc) return rg_refuse(ctx, dc_why_text(DC_WHY_BLOCK_CRC, (uint32_t)(k0 + j)));
        }
        for (const Edge &g : edges) {                        // verified: the slices of the edge blocks
            const bzx_index_entry &x = e[g.k];
            const uint64_t a = std::max<uint64_t>(x.out_off, lo), z = std::min<uint64_t>(x.out_off + x.out_len, hi);
            HIP_TRY(ctx, hipMemcpyAsync(d_out + (a - lo), t.edge[g.area] + (a - x.out_off), z - a, hipMemcpyDeviceToDevice, st));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->stats_batch = true;
    ctx->stats.nblk = (uint32_t)count;
    ctx->stats.raw_bytes = hi - lo;
    return BZX_OK;
}

// Argument checks and the span of both forms.  *count == 0: nothing to do.
static int range_args(bzx_ctx *ctx, size_t len, uint64_t base, const bzx_index_entry *e, uint64_t n, uint64_t off, uint64_t want,
                      uint64_t *first, uint64_t *count, uint64_t *lo, uint64_t *hi)
{
    uint64_t byte_lo = 0, byte_hi = 0;
    if (bzx_index_span(e, n, off, want, first, count, &byte_lo, &byte_hi)) {
        ctx->err = "range read: the index entries are not in order";
        return BZX_E_PARAM;
    }
    if (!*count) return BZX_OK;
    if (base > byte_lo || base + len < byte_hi) {
        ctx->err = "range read: the input bytes given do not cover bytes [" + std::to_string(byte_lo) + ", " +
                   std::to_string(byte_hi) + ") of the file (bzx_index_span)";
        return BZX_E_PARAM;
    }
    *lo = off;
    *hi = std::min<uint64_t>(rg_total(e, n), off + std::min<uint64_t>(want, ~0ull - off));
    // the touched entries tile [their first byte, their last byte): out_off is the running sum of out_len
    uint64_t at = e[*first].out_off;
    for (uint64_t k = *first; k < *first + *count; k++) {
        if (e[k].out_off != at || e[k].out_len == 0)
            return rg_refuse(ctx, "index does not match the input: out_off is not the running sum of out_len (block " +
                                      std::to_string(k) + ")");
        at += e[k].out_len;
    }
    if (at < *hi) return rg_refuse(ctx, "index does not match the input: the entries do not cover the range");
    return BZX_OK;
}

extern "C" int bzx_decompress_range_device(bzx_ctx *ctx, const void *d_bz2, size_t len, uint64_t base, const bzx_index_entry *e,
                                           uint64_t n, uint64_t off, uint64_t want, void *d_out, size_t *got)
{
    auto api_lock_ = ctx_lock(ctx);
    if (got) *got = 0;
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !got || (n && !e)) return BZX_E_PARAM;
    uint64_t first = 0, count = 0, lo = 0, hi = 0;
    int rc = range_args(ctx, len, base, e, n, off, want, &first, &count, &lo, &hi);
    if (rc || !count) return rc;
    if (!d_bz2 || !d_out) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    try {
        rc = range_run(ctx, (const uint8_t *)d_bz2, len, base, e, first, count, lo, hi, (uint8_t *)d_out);
    } catch (const std::bad_alloc &) {                       // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (rc) (void)hipStreamSynchronize(ctx->stream);         // nothing of a failed call is left in flight
    else *got = (size_t)(hi - lo);
    return rc;
}

extern "C" int bzx_decompress_range_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint64_t base, const bzx_index_entry *e,
                                           uint64_t n, uint64_t off, uint64_t want, uint8_t *out, size_t *got)
{
    auto api_lock_ = ctx_lock(ctx);
    if (got) *got = 0;
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !got || (n && !e)) return BZX_E_PARAM;
    uint64_t first = 0, count = 0, lo = 0, hi = 0;
    int rc = range_args(ctx, len, base, e, n, off, want, &first, &count, &lo, &hi);
    if (rc || !count) return rc;
    if (!bz2 || !out) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the span alone travels to the device, one slice comes back
    const uint64_t byte_lo = e[first].bit / 8;
    const uint64_t byte_hi = (e[first + count - 1].bit + e[first + count - 1].img_bits + 7) / 8 + 8;
    // (two device buffers the context keeps and grows: no allocation, and no hipFree with its device-wide wait, on the
    // path of a small read)
    void *d_z = nullptr, *d_o = nullptr;
    if ((rc = rg_io(ctx, 0, (size_t)(byte_hi - byte_lo) + 64, &d_z)) || (rc = rg_io(ctx, 1, (size_t)(hi - lo) + 64, &d_o))) return rc;
    rc = hipMemcpyAsync(d_z, bz2 + (byte_lo - base), (size_t)(byte_hi - byte_lo), hipMemcpyHostToDevice, ctx->stream) == hipSuccess
             ? BZX_OK
             : BZX_E_HIP;
    try {
        if (!rc)
            rc = range_run(ctx, (const uint8_t *)d_z, (size_t)(byte_hi - byte_lo), byte_lo, e, first, count, lo, hi, (uint8_t *)d_o);
    } catch (const std::bad_alloc &) {                       // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (!rc && hipMemcpyAsync(out, d_o, (size_t)(hi - lo), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        ctx->err = "hipMemcpyAsync(range output) failed";
        rc = BZX_E_HIP;
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) {
        ctx->err = "hipStreamSynchronize(range output) failed";
        rc = BZX_E_HIP;
    }
    if (!rc) *got = (size_t)(hi - lo);
    return rc;
}

// ---- the inverse BWT alone, for the parity tests ------------------------------------------------------------------------
extern "C" int bzx_stage_ibwt(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, int wide, uint8_t *img_out,
                              uint8_t *raw_out, size_t raw_cap, uint64_t *raw_len, uint32_t *status)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !L || !img_out || !raw_len || !status || (raw_cap && !raw_out) || n == 0 || n > BZX_MAX_N || orig_ptr >= n)
        return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, 1);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    B.nblk = 1;
    B.blk_first = 0;
    B.blk_step = 1;
    // what the block decoder leaves: L, the number of earlier occurrences of each byte, the byte counts (scaffolding)
    std::vector<uint32_t> occ, freq;
    try {
        occ.resize(n);
        freq.assign(260, 0);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
    for (size_t i = 0; i < n; i++) occ[i] = freq[L[i]]++;
    BzxBlock d;
    memset(&d, 0, sizeof(d));
    d.n = (uint32_t)n;
    d.orig_ptr = orig_ptr;
    uint8_t *d_raw = nullptr;
    if (hipMalloc((void **)&d_raw, raw_cap + 64) != hipSuccess) {
        ctx->err = "bzx_stage_ibwt: hipMalloc(expansion) failed";
        return BZX_E_NOMEM;
    }
    const BzxDcDst dst{raw_cap ? d_raw : nullptr, raw_cap};
    BzxDcDst *d_dst = reinterpret_cast<BzxDcDst *>(B.selector);          // (a slab the inverse BWT does not touch)
    auto run = [&]() -> int {
        HIP_TRY(ctx, hipMemcpyAsync(B.bwt, L, n, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(B.rec_a, occ.data(), n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(B.freq, freq.data(), 260 * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(B.blk, &d, sizeof(d), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_dst, &dst, sizeof(dst), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_in, 0xEE, n, st));
        if (wide) bzx_launch_dc_ibwt_wide(B, ctx->d_in, (uint32_t)n, st);
        else bzx_launch_dc_ibwt(B, ctx->d_in, st);
        bzx_launch_dc_expand(B, ctx->d_in, d_dst, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, B.blk, sizeof(d), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(img_out, ctx->d_in, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        *status = ctx->h_blk[0].status;
        *raw_len = ctx->h_blk[0].pack_word;
        const size_t k = (size_t)std::min<uint64_t>(*raw_len, raw_cap);
        if (k && !*status) HIP_TRY(ctx, hipMemcpy(raw_out, d_raw, k, hipMemcpyDeviceToHost));
        return BZX_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_raw);
    return rc;
}

// The inverse BWT launchers alone under HIP events, for the probe: `copies` copies of one block side by side (slab 0 is
// filled from the host, the others from it on the device), `reps` launches, the best one's milliseconds.
extern "C" int bzx_stage_ibwt_time(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, int wide, uint32_t copies,
                                   uint32_t reps, float *ms_best)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !L || !ms_best || n == 0 || n > BZX_MAX_N || orig_ptr >= n || copies == 0 || reps == 0) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, copies);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    B.nblk = copies;
    B.blk_first = 0;
    B.blk_step = 1;
    std::vector<uint32_t> occ, freq;
    std::vector<BzxBlock> d;
    try {
        occ.resize(n);
        freq.assign(260, 0);
        d.resize(copies);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
    for (size_t i = 0; i < n; i++) occ[i] = freq[L[i]]++;
    memset(d.data(), 0, copies * sizeof(BzxBlock));
    for (uint32_t b = 0; b < copies; b++) {
        d[b].n = (uint32_t)n;
        d[b].orig_ptr = orig_ptr;
    }
    HIP_TRY(ctx, hipMemcpyAsync(B.bwt, L, n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(B.freq, freq.data(), 260 * 4, hipMemcpyHostToDevice, st));
    for (uint32_t b = 1; b < copies; b++) {
        HIP_TRY(ctx, hipMemcpyAsync(B.bwt + (size_t)b * BZX_BLK_STRIDE, B.bwt, n, hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(B.freq + (size_t)b * 260, B.freq, 260 * 4, hipMemcpyDeviceToDevice, st));
    }
    float best = 0.f;
    for (uint32_t r = 0; r < reps; r++) {
        // the pack kernel overwrites the occurrence counts: they are put back before every launch
        HIP_TRY(ctx, hipMemcpyAsync(B.rec_a, occ.data(), n * 4, hipMemcpyHostToDevice, st));
        for (uint32_t b = 1; b < copies; b++)
            HIP_TRY(ctx, hipMemcpyAsync(B.rec_a + (size_t)b * BZX_MAX_N, B.rec_a, n * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(B.blk, d.data(), copies * sizeof(BzxBlock), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipEventRecord(ctx->ev[5], st));
        if (wide) bzx_launch_dc_ibwt_wide(B, ctx->d_in, (uint32_t)n, st);
        else bzx_launch_dc_ibwt(B, ctx->d_in, st);
        HIP_TRY(ctx, hipEventRecord(ctx->ev[7], st));
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(st));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[7]));
        if (r == 0 || ms < best) best = ms;
    }
    *ms_best = best;
    return BZX_OK;
}
