// bzx_range.hip -- random access on gfx950 (include/bzx.h: bzx_index_span, bzx_decompress_range_*, bzx_stage_ibwt; many
// ranges in one call: bzx_index_spans, bzx_decompress_ranges_*, bzx_stage_gather, further down):
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
//   expand, CRC   a block that one range alone touches and wholly contains at its final place in the output, every
//                 other block (the at most two edge blocks of a range; a block that several ranges share) into the pool
//   [sync]        descriptors, CRCs and flags; the host holds every block against its entry, then one launch of the
//                 gather kernel moves the wanted slices of the verified pool blocks
// One host synchronisation per round; nothing leaves through _buffer before every block of the range has passed.
// One core (ranges_plan, ranges_exec, ranges_call) serves every entry point: the single call is count = 1 over one piece.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bzx_host.h"

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
    uint64_t other;
    rg_block_bytes(*a, byte_lo, &other);
    rg_block_bytes(z[-1], &other, byte_hi);
    return BZX_OK;
}

// Round tables: device [src R][dst R][want_len R][got R][flag R], pinned [got R][flag R]; behind them on the device the
// pool.
// (RgTables: bzx_host.h -- the record reads of bzx_records.hip run their rounds through the same tables)
int rg_tables(bzx_ctx *ctx, uint32_t R, RgTables *t)
{
    if (R < ctx->range_slabs) R = ctx->range_slabs;          // (the tables are laid out for the blocks they hold)
    const bool ok = carved(ctx->range_ws, 256, [&](Carver &c) {
        t->d_src = c.take<BzxDcSrc>(R);
        t->d_dst = c.take<BzxDcDst>(R);
        t->d_len = c.take<uint32_t>(R);
        t->d_got = c.take<uint32_t>(R);                      // (got and flag lie side by side: one memset clears both)
        t->d_flag = c.take<uint32_t>(R);
        t->pool = c.take<uint8_t>(RG_POOL_BYTES);
    }) && carved(ctx->range_pin, 256, [&](Carver &c) {
        t->h_got = c.take<uint32_t>(R);
        t->h_flag = c.take<uint32_t>(R);
    });
    if (!ok) {
        ctx->range_ws.reset();
        ctx->range_pin.reset();
        ctx->range_slabs = 0;
        ctx->err = "range read: device or pinned allocation failed";
        return BZX_E_NOMEM;
    }
    ctx->range_slabs = R;
    return BZX_OK;
}

// The _buffer form's device buffer k of at least `bytes` bytes: kept by the context, grown when a call needs more.
static int rg_io(bzx_ctx *ctx, int k, size_t bytes, void **p)
{
    // (at least 4 MiB: a 900k block's span and a few MB of output)
    if (!ctx->range_io[k].reserve(std::max<size_t>(bytes, (size_t)4 << 20))) {
        ctx->err = k ? "range read: hipMalloc(output) failed" : "range read: hipMalloc(span) failed";
        return BZX_E_NOMEM;
    }
    *p = ctx->range_io[k];
    return BZX_OK;
}

// The _buffer forms' upload: the pieces with held[j] set go, back to back, into the span buffer the context keeps;
// d_pc[j]: where piece j lies on the device (untouched for the others).  Enqueued on the context's stream.
int rg_upload(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const uint8_t *held, const uint8_t **d_pc)
{
    size_t bytes = 0;
    for (uint32_t j = 0; j < npc; j++) bytes += held[j] ? (size_t)pc[j].len : 0;
    void *d_z = nullptr;
    const int rc = rg_io(ctx, 0, bytes + 64, &d_z);
    if (rc) return rc;
    size_t at = 0;
    for (uint32_t j = 0; j < npc; j++) {
        if (!held[j]) continue;
        d_pc[j] = (const uint8_t *)d_z + at;
        HIP_TRY(ctx, hipMemcpyAsync((uint8_t *)d_z + at, pc[j].p, (size_t)pc[j].len, hipMemcpyHostToDevice, ctx->stream));
        at += (size_t)pc[j].len;
    }
    return BZX_OK;
}

static int rg_refuse(bzx_ctx *ctx, const std::string &why)
{
    ctx->err = why;
    return BZX_E_DATA;
}

// A decoded block held against its entry: BZX_OK, or BZX_E_DATA and the text.  k: the entry's number.
int rg_verdict(bzx_ctx *ctx, const bzx_index_entry &x, uint64_t k, const BzxBlock &d, uint32_t flag, uint32_t got)
{
    const std::string blk = " (block " + std::to_string(k) + ")";
    if (flag & RG_NO_MAGIC)
        return rg_refuse(ctx, "index does not match the input: no block magic at bit " + std::to_string(x.bit) + blk);
    const uint32_t status = d.status & ~DC_SKIP;
    if (status & BZX_ST_DC_RANDOMISED) return rg_refuse(ctx, dc_why_text(DC_WHY_RANDOMISED));
    if (status) return rg_refuse(ctx, dc_why_text(DC_WHY_DAMAGED) + blk);
    if (d.crc != x.crc) return rg_refuse(ctx, "index does not match the input: another stored CRC" + blk);
    if (d.n > 100000u * x.level) return rg_refuse(ctx, "index does not match the input: the block is longer than its level allows" + blk);
    if ((uint32_t)(d.bits - d.out_bit) != x.img_bits)
        return rg_refuse(ctx, "index does not match the input: another block size" + blk);
    if (flag & RG_LENGTH) return rg_refuse(ctx, "index does not match the input: another decoded length" + blk);
    if (got != d.crc) return rg_refuse(ctx, dc_why_text(DC_WHY_BLOCK_CRC, (uint32_t)k));
    return BZX_OK;
}

// One round on the device: nb blocks through decode, inverse BWT, check, expand and CRC; descriptors (ctx->h_blk), CRCs
// and flags (t.h_got, t.h_flag) are on the host when it returns.  The round's one synchronisation.
int rg_round(bzx_ctx *ctx, const RgTables &t, uint32_t nb, const BzxDcSrc *src, const BzxDcDst *dst, const uint32_t *len,
                    uint32_t n_hint)
{
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    B.nblk = nb;
    B.blk_first = 0;
    B.blk_step = 1;
    HIP_TRY(ctx, hipMemcpyAsync(t.d_src, src, nb * sizeof(BzxDcSrc), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(t.d_dst, dst, nb * sizeof(BzxDcDst), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(t.d_len, len, nb * 4, hipMemcpyHostToDevice, st));
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
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return BZX_OK;
}

// The touched entries tile [their first byte, their last byte): out_off is the running sum of out_len.
static int rg_tiles(bzx_ctx *ctx, const bzx_index_entry *e, uint64_t first, uint64_t count, uint64_t hi)
{
    uint64_t at = e[first].out_off;
    for (uint64_t k = first; k < first + count; k++) {
        if (e[k].out_off != at || e[k].out_len == 0)
            return rg_refuse(ctx, "index does not match the input: out_off is not the running sum of out_len (block " +
                                      std::to_string(k) + ")");
        at += e[k].out_len;
    }
    if (at < hi) return rg_refuse(ctx, "index does not match the input: the entries do not cover the range");
    return BZX_OK;
}

// ---- the core: any number of ranges in one call (bzx_index_spans, bzx_decompress_range_*, _ranges_*, bzx_stage_gather) ----
// The host plans the whole call from the index: every range is clipped and given its place in the packed output, the
// distinct touched blocks are listed in ascending order with the slices the ranges want of them, and rounds of at most R
// blocks go through rg_round.  A block that one range alone touches and wholly contains expands at its final place; every
// other block expands into the pool (behind the round tables in range_ws, 256-byte aligned offsets), and after the
// round's verdicts ONE launch of the gather kernel moves the slices of its verified pool blocks.
#define RG_PIECE ((uint64_t)64 << 10)          // bytes one workgroup of the gather kernel moves at most
#define RG_NT 256

struct RgSlice {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t len;
};

// One workgroup per table entry of at most RG_PIECE bytes; source and destination have any alignment, independently.
// Head bytes up to the first 16-byte boundary of dst, then one 16-byte store per lane and step, then the byte tail.  A
// source that is 16-byte aligned behind the head is read in 16-byte loads; any other in aligned dwords (the four or five
// that hold the lane's 16 bytes: never a byte outside the aligned dwords that hold the slice) put in place by a funnel
// shift.  The alignment is the same for every lane of the workgroup, so the branch is uniform.
__global__ __launch_bounds__(RG_NT) void bzx_rg_gather_kernel(const RgSlice *__restrict__ tab)
{
    const RgSlice s = tab[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const uint32_t len = (uint32_t)s.len;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)s.dst & 15u)) & 15u);
    if (head > len) head = len;
    if (t < head) s.dst[t] = s.src[t];
    const uint8_t *src = s.src + head;
    uint8_t *dst = s.dst + head;
    const uint32_t nvec = (len - head) / 16;
    const uint32_t k = (uint32_t)((uintptr_t)src & 3u);
    if (((uintptr_t)src & 15u) == 0) {
        for (uint32_t v = t; v < nvec; v += RG_NT) ((uint4 *)dst)[v] = ((const uint4 *)src)[v];
    } else {
        const uint32_t *w = (const uint32_t *)(src - k);
        const uint32_t sh = k * 8;
        for (uint32_t v = t; v < nvec; v += RG_NT) {
            const uint32_t *q = w + (size_t)v * 4;
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
            const uint32_t w4 = k ? q[4] : 0u;               // (k == 0: the fifth dword holds nothing of this vector)
            ((uint4 *)dst)[v] = make_uint4((uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh),
                                           (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh), (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh));
        }
    }
    const uint32_t done = nvec * 16, tail = len - head - done;
    if (t < tail) dst[done + t] = src[done + t];
}

// A slice as table entries of at most RG_PIECE bytes.
static void rg_cut(std::vector<RgSlice> &v, const uint8_t *src, uint8_t *dst, uint64_t len)
{
    for (uint64_t at = 0; at < len; at += RG_PIECE) v.push_back(RgSlice{src + at, dst + at, std::min<uint64_t>(RG_PIECE, len - at)});
}

// The table to the device (the context keeps it and grows it on demand) and one launch over it.
static int rg_gather(bzx_ctx *ctx, const std::vector<RgSlice> &v)
{
    if (v.empty()) return BZX_OK;
    // (grown to 1.5 times what the call needs, at least 4096 entries)
    if (v.size() * sizeof(RgSlice) > ctx->range_sl.bytes() &&
        !ctx->range_sl.reserve(std::max<size_t>(v.size() + v.size() / 2, 4096) * sizeof(RgSlice))) {
        ctx->err = "range read: hipMalloc(slice table) failed";
        return BZX_E_NOMEM;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->range_sl, v.data(), v.size() * sizeof(RgSlice), hipMemcpyHostToDevice, ctx->stream));
    const size_t GMAX = (size_t)1 << 30;                     // (a grid holds 2^31 - 1 workgroups)
    for (size_t at = 0; at < v.size(); at += GMAX)
        hipLaunchKernelGGL(bzx_rg_gather_kernel, dim3((uint32_t)std::min(GMAX, v.size() - at)), dim3(RG_NT), 0, ctx->stream,
                           ctx->range_sl.get<const RgSlice>() + at);
    HIP_TRY(ctx, hipGetLastError());
    return BZX_OK;
}

extern "C" int bzx_index_spans(const bzx_index_entry *e, uint64_t n, uint32_t count, const uint64_t *offs, const uint64_t *wants,
                               uint64_t *bases, uint64_t *lens, uint32_t cap_pieces, uint32_t *npieces)
{
    if (!npieces || (n && !e) || (count && (!offs || !wants)) || (cap_pieces && (!bases || !lens))) return BZX_E_PARAM;
    *npieces = 0;
    try {
        std::vector<std::pair<uint64_t, uint64_t>> iv;      // entries [first, end) of every range that touches any
        for (uint32_t i = 0; i < count; i++) {
            uint64_t first = 0, c = 0, lo = 0, hi = 0;
            if (bzx_index_span(e, n, offs[i], wants[i], &first, &c, &lo, &hi)) return BZX_E_PARAM;
            if (c) iv.push_back({first, first + c});
        }
        std::sort(iv.begin(), iv.end());
        uint64_t np = 0, next_k = 0, cur_lo = 0, cur_hi = 0;
        bool open = false;
        auto flush = [&]() {
            if (open && np < cap_pieces) {
                bases[np] = cur_lo;
                lens[np] = cur_hi - cur_lo;
            }
            np += open;
        };
        for (const auto &v : iv) {
            for (uint64_t k = std::max(v.first, next_k); k < v.second; k++) {      // every distinct block once, ascending
                uint64_t lo, hi;
                rg_block_bytes(e[k], &lo, &hi);
                if (open && lo <= cur_hi) {                  // overlapping or adjacent
                    cur_hi = std::max(cur_hi, hi);
                } else {
                    flush();
                    open = true;
                    cur_lo = lo;
                    cur_hi = hi;
                }
            }
            next_k = std::max(next_k, v.second);
        }
        flush();
        *npieces = (uint32_t)std::min<uint64_t>(np, 0xFFFFFFFFu);
        return np > cap_pieces ? BZX_E_OUTBUF : BZX_OK;
    } catch (const std::bad_alloc &) {
        return BZX_E_NOMEM;
    }
}

struct RgUse {                                  // bytes [a, z) of a pool block go to range r
    uint32_t r, a, z;
};
struct RgBlk {
    uint64_t k;                                 // the entry
    uint32_t piece;                             // the piece that holds its input bytes
    int64_t sole;                               // the one range that touches and wholly contains it: it expands in place; -1: pool
    size_t u0, u1;                              // its uses (pool blocks)
    uint64_t pool_off;
};
struct RgPlan {
    std::vector<uint64_t> lo, hi, first, cnt;   // per range, clipped
    std::vector<uint8_t> bad;                   // per range: failed
    std::vector<RgBlk> blk;                     // the distinct touched blocks, ascending
    std::vector<RgUse> use;
    uint64_t need = 0;
    uint64_t fail_k = ~0ull;                    // the lowest failed range and the text of its failure
    std::string fail_text;
    void fail(uint32_t r, const std::string &text)
    {
        bad[r] = 1;
        if (r < fail_k) {
            fail_k = r;
            fail_text = text;
        }
    }
};

// The host plan.  A return value other than BZX_OK fails the whole call; what fails one range is noted in the plan.
static int ranges_plan(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, uint32_t count,
                       const uint64_t *offs, const uint64_t *wants, size_t cap, size_t *out_offs, size_t *gots, size_t *need,
                       RgPlan &P)
{
    for (uint32_t j = 0; j < npc; j++) {
        if ((pc[j].len && !pc[j].p) || pc[j].len > ~0ull - pc[j].base || (j && pc[j].base < pc[j - 1].base + pc[j - 1].len)) {
            ctx->err = "range read: the pieces of the input are not ascending and disjoint (piece " + std::to_string(j) + ")";
            return BZX_E_PARAM;
        }
    }
    const uint64_t total = rg_total(e, n);
    P.lo.resize(count);
    P.hi.resize(count);
    P.first.resize(count);
    P.cnt.resize(count);
    P.bad.assign(count, 0);
    uint64_t sum = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t blo = 0, bhi = 0;
        if (bzx_index_span(e, n, offs[i], wants[i], &P.first[i], &P.cnt[i], &blo, &bhi)) {
            ctx->err = "range read: the index entries are not in order";
            return BZX_E_PARAM;
        }
        P.lo[i] = P.hi[i] = offs[i];
        if (P.cnt[i]) P.hi[i] = std::min<uint64_t>(total, offs[i] + std::min<uint64_t>(wants[i], ~0ull - offs[i]));
        out_offs[i] = (size_t)sum;
        gots[i] = (size_t)(P.hi[i] - P.lo[i]);
        sum += P.hi[i] - P.lo[i];
    }
    P.need = sum;
    *need = (size_t)sum;
    if (sum > cap) {
        ctx->err = "range read: the output needs " + std::to_string(sum) + " bytes";
        return BZX_E_OUTBUF;
    }
    // what the single call refuses before it decodes anything, per range
    std::vector<uint32_t> ord;
    for (uint32_t i = 0; i < count; i++) {
        if (!P.cnt[i]) continue;
        int rc = rg_tiles(ctx, e, P.first[i], P.cnt[i], P.hi[i]);
        for (uint64_t k = P.first[i]; !rc && k < P.first[i] + P.cnt[i]; k++)
            if (e[k].out_len > RG_EDGE_BYTES - 16) rc = rg_refuse(ctx, "index does not match the input: an entry's out_len exceeds a block");
        if (rc) P.fail(i, ctx->err);
        else ord.push_back(i);
    }
    // the distinct touched blocks in ascending order, each with the ranges that touch it
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return P.first[a] != P.first[b] ? P.first[a] < P.first[b] : a < b; });
    std::vector<uint32_t> act;
    size_t nx = 0;
    uint64_t k = 0;
    while (nx < ord.size() || !act.empty()) {
        if (act.empty()) k = P.first[ord[nx]];
        while (nx < ord.size() && P.first[ord[nx]] == k) act.push_back(ord[nx++]);
        const bzx_index_entry &x = e[k];
        RgBlk b{k, 0, -1, P.use.size(), P.use.size(), 0};
        uint64_t blo, bhi;
        rg_block_bytes(x, &blo, &bhi);
        const bzx_piece *q = std::upper_bound(pc, pc + npc, blo, [](uint64_t v, const bzx_piece &y) { return v < y.base; });
        if (q == pc || bhi > q[-1].base + q[-1].len) {
            ctx->err = "range " + std::to_string(*std::min_element(act.begin(), act.end())) +
                       ": range read: the input bytes given do not cover bytes [" + std::to_string(blo) + ", " + std::to_string(bhi) +
                       ") of the file in one piece (bzx_index_spans)";
            return BZX_E_PARAM;
        }
        b.piece = (uint32_t)(q - 1 - pc);
        if (act.size() == 1 && x.out_off >= P.lo[act[0]] && x.out_off + x.out_len <= P.hi[act[0]]) {
            b.sole = act[0];
        } else {
            for (uint32_t r : act) {
                const uint64_t a = std::max<uint64_t>(x.out_off, P.lo[r]), z = std::min<uint64_t>(x.out_off + x.out_len, P.hi[r]);
                P.use.push_back(RgUse{r, (uint32_t)(a - x.out_off), (uint32_t)(z - x.out_off)});
            }
            b.u1 = P.use.size();
        }
        P.blk.push_back(b);
        k++;
        act.erase(std::remove_if(act.begin(), act.end(), [&](uint32_t r) { return P.first[r] + P.cnt[r] <= k; }), act.end());
    }
    return BZX_OK;
}

// The rounds.  d_pc[j]: where piece j lies on the device.
static int ranges_exec(bzx_ctx *ctx, RgPlan &P, const bzx_piece *pc, const uint8_t *const *d_pc, const bzx_index_entry *e,
                       uint8_t *d_out, const size_t *out_offs)
{
    int rc = ensure_blocks(ctx, 1);              // (a context holds 16 slabs at least from bzx_ctx_create on: nothing grows)
    if (rc) return rc;
    const uint32_t R = ctx->cap_slabs;
    RgTables t;
    if ((rc = rg_tables(ctx, R, &t))) return rc;
    uint8_t *pool = t.pool;
    std::vector<BzxDcSrc> src(R);
    std::vector<BzxDcDst> dst(R);
    std::vector<uint32_t> len(R);
    std::vector<RgSlice> sl;
    for (size_t i = 0; i < P.blk.size();) {
        uint32_t nb = 0, n_hint = 0;
        uint64_t used = 0;
        for (; i + nb < P.blk.size() && nb < R; nb++) {
            RgBlk &b = P.blk[i + nb];
            const bzx_index_entry &x = e[b.k];
            if (b.sole < 0) {                                // (out_len <= RG_EDGE_BYTES - 16: one block always fits)
                if (used + rg_al(x.out_len) > RG_POOL_BYTES) break;
                b.pool_off = used;
                used += rg_al(x.out_len);
                dst[nb] = BzxDcDst{pool + b.pool_off, x.out_len};
            } else {
                dst[nb] = BzxDcDst{d_out + out_offs[b.sole] + (x.out_off - P.lo[b.sole]), x.out_len};
            }
            n_hint = std::max<uint32_t>(n_hint, (uint32_t)std::min<uint64_t>(BZX_MAX_N, (uint64_t)x.out_len * 5 / 4 + 8));
            src[nb] = BzxDcSrc{d_pc[b.piece], pc[b.piece].len, x.bit - pc[b.piece].base * 8};
            len[nb] = x.out_len;
        }
        if ((rc = rg_round(ctx, t, nb, src.data(), dst.data(), len.data(), n_hint))) return rc;
        sl.clear();
        for (uint32_t j = 0; j < nb; j++) {
            const RgBlk &b = P.blk[i + j];
            const bzx_index_entry &x = e[b.k];
            if (rg_verdict(ctx, x, b.k, ctx->h_blk[j], t.h_flag[j], t.h_got[j])) {      // fails the ranges that touch it
                if (b.sole >= 0) P.fail((uint32_t)b.sole, ctx->err);
                for (size_t u = b.u0; u < b.u1; u++) P.fail(P.use[u].r, ctx->err);
            }
        }
        for (uint32_t j = 0; j < nb; j++) {                  // the slices of the verified pool blocks
            const RgBlk &b = P.blk[i + j];
            for (size_t u = b.u0; u < b.u1; u++) {
                const RgUse &g = P.use[u];
                if (P.bad[g.r]) continue;
                rg_cut(sl, pool + b.pool_off + g.a, d_out + out_offs[g.r] + (e[b.k].out_off + g.a - P.lo[g.r]), g.z - g.a);
            }
        }
        if ((rc = rg_gather(ctx, sl))) return rc;
        i += nb;
        // every range has failed: nothing is left to deliver, statuses and texts are final
        if (std::find(P.bad.begin(), P.bad.end(), 0) == P.bad.end()) break;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BZX_OK;
}

// Both forms.  host: pieces[].p and out are host pointers.  BZX_E_DATA: the statuses are set range by range, *fail_k is
// the lowest failed range and ctx->err the text of its failure as it stands (the batched entry names the range in front).
static int ranges_call(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, uint32_t count,
                       const uint64_t *offs, const uint64_t *wants, uint8_t *out, size_t cap, size_t *out_offs, size_t *gots,
                       int *status, size_t *need, bool host, uint64_t *fail_k)
{
    RgPlan P;
    int rc = ranges_plan(ctx, pc, npc, e, n, count, offs, wants, cap, out_offs, gots, need, P);
    if (rc) return rc;
    if (!P.blk.empty()) {
        if (!out) {
            ctx->err = "range read: no output buffer";
            return BZX_E_PARAM;
        }
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<const uint8_t *> d_pc(npc, nullptr);
        uint8_t *d_out = out;
        if (host) {                                          // the pieces that hold a touched block, back to back
            std::vector<uint8_t> held(npc, 0);
            for (const RgBlk &b : P.blk) held[b.piece] = 1;
            void *d_o = nullptr;
            if ((rc = rg_upload(ctx, pc, npc, held.data(), d_pc.data())) || (rc = rg_io(ctx, 1, (size_t)P.need + 64, &d_o))) return rc;
            d_out = (uint8_t *)d_o;
        } else {
            for (uint32_t j = 0; j < npc; j++) d_pc[j] = (const uint8_t *)pc[j].p;
        }
        if ((rc = ranges_exec(ctx, P, pc, d_pc.data(), e, d_out, out_offs))) return rc;
        if (host) {                                          // maximal runs of consecutive good ranges: one copy each
            for (uint32_t i = 0; i < count;) {
                if (P.bad[i]) {
                    i++;
                    continue;
                }
                uint32_t j = i;
                while (j < count && !P.bad[j]) j++;
                const size_t a = out_offs[i], z = out_offs[j - 1] + gots[j - 1];
                if (z > a) HIP_TRY(ctx, hipMemcpyAsync(out + a, d_out + a, z - a, hipMemcpyDeviceToHost, ctx->stream));
                i = j;
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    uint64_t raw = 0;
    for (uint32_t i = 0; i < count; i++) {
        status[i] = P.bad[i] ? BZX_E_DATA : BZX_OK;
        if (P.bad[i]) gots[i] = 0;
        raw += gots[i];
    }
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->stats_batch = true;
    ctx->stats.nblk = (uint32_t)P.blk.size();
    ctx->stats.raw_bytes = raw;
    if (P.fail_k != ~0ull) {
        ctx->err = P.fail_text;
        *fail_k = P.fail_k;
        return BZX_E_DATA;
    }
    return BZX_OK;
}

// ... with nothing unwinding across the C ABI and nothing of a failed call left in flight.
static int ranges_core(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, uint32_t count,
                       const uint64_t *offs, const uint64_t *wants, void *out, size_t cap, size_t *out_offs, size_t *gots,
                       int *status, size_t *need, bool host, uint64_t *fail_k)
{
    int rc;
    try {
        rc = ranges_call(ctx, pc, npc, e, n, count, offs, wants, (uint8_t *)out, cap, out_offs, gots, status, need, host, fail_k);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (rc && rc != BZX_E_DATA) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

static int ranges_entry(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, uint32_t count,
                        const uint64_t *offs, const uint64_t *wants, void *out, size_t cap, size_t *out_offs, size_t *gots,
                        int *status, size_t *need, bool host)
{
    auto api_lock_ = ctx_lock(ctx);
    if (need) *need = 0;
    int rc = BZX_OK;
    bool whole = true;                           // rc fails the whole call: it goes into every status
    if (!ctx) {
        rc = BZX_E_PARAM;
    } else if (ctx->ds) {
        rc = refuse_streaming(ctx);
    } else if (count == 0) {
        return BZX_OK;
    } else if (!offs || !wants || !out_offs || !gots || !status || !need || (n && !e) || (npc && !pc)) {
        ctx->err = "range read: a NULL array";
        rc = BZX_E_PARAM;
    } else {
        uint64_t fail_k = 0;
        rc = ranges_core(ctx, pc, npc, e, n, count, offs, wants, out, cap, out_offs, gots, status, need, host, &fail_k);
        whole = rc != BZX_OK && rc != BZX_E_DATA;            // (BZX_E_DATA: the statuses are set, range by range)
        if (rc == BZX_E_DATA) ctx->err = "range " + std::to_string(fail_k) + ": " + ctx->err;
    }
    if (rc && whole) {
        for (uint32_t i = 0; i < count; i++) {
            if (status) status[i] = rc;
            if (gots) gots[i] = 0;
        }
    }
    return rc;
}

extern "C" int bzx_decompress_ranges_device(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                            uint64_t n, uint32_t count, const uint64_t *offs, const uint64_t *wants, void *d_out,
                                            size_t cap, size_t *out_offs, size_t *gots, int *status, size_t *need)
{
    return ranges_entry(ctx, pieces, npieces, e, n, count, offs, wants, d_out, cap, out_offs, gots, status, need, false);
}

extern "C" int bzx_decompress_ranges_buffer(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                            uint64_t n, uint32_t count, const uint64_t *offs, const uint64_t *wants, uint8_t *out,
                                            size_t cap, size_t *out_offs, size_t *gots, int *status, size_t *need)
{
    return ranges_entry(ctx, pieces, npieces, e, n, count, offs, wants, out, cap, out_offs, gots, status, need, true);
}

// The single call, both forms: count = 1 of the core over one piece.  host: bz2 and out are host pointers, and the span
// alone is the piece (it alone is uploaded, one slice comes back).  A touched entry whose bytes leave the piece (a corrupt
// index: the first and the last one lie inside the span by construction) would read zeros there: it is refused here with
// the text of a missing magic, before the core runs -- so if a lower-numbered block fails too, for another reason, this
// entry's text is the one reported.
static int range_entry(bzx_ctx *ctx, const void *bz2, size_t len, uint64_t base, const bzx_index_entry *e, uint64_t n, uint64_t off,
                       uint64_t want, void *out, size_t *got, bool host)
{
    auto api_lock_ = ctx_lock(ctx);
    if (got) *got = 0;
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !got || (n && !e)) return BZX_E_PARAM;
    uint64_t first = 0, count = 0, byte_lo = 0, byte_hi = 0;
    if (bzx_index_span(e, n, off, want, &first, &count, &byte_lo, &byte_hi)) {
        ctx->err = "range read: the index entries are not in order";
        return BZX_E_PARAM;
    }
    if (!count) return BZX_OK;
    if (base > byte_lo || base + len < byte_hi) {
        ctx->err = "range read: the input bytes given do not cover bytes [" + std::to_string(byte_lo) + ", " +
                   std::to_string(byte_hi) + ") of the file (bzx_index_span)";
        return BZX_E_PARAM;
    }
    if (!bz2 || !out) return BZX_E_PARAM;
    const bzx_piece pc = host ? bzx_piece{(const uint8_t *)bz2 + (byte_lo - base), byte_lo, byte_hi - byte_lo} : bzx_piece{bz2, base, len};
    for (uint64_t k = first; k < first + count; k++) {
        uint64_t lo, hi;
        rg_block_bytes(e[k], &lo, &hi);
        if (lo < pc.base || hi > pc.base + pc.len)
            return rg_refuse(ctx, "index does not match the input: no block magic at bit " + std::to_string(e[k].bit) + " (block " +
                                      std::to_string(k) + ")");
    }
    size_t out_off = 0, need = 0;
    int status = 0;
    uint64_t fail_k = 0;
    const int rc = ranges_core(ctx, &pc, 1, e, n, 1, &off, &want, out, ~(size_t)0, &out_off, got, &status, &need, host, &fail_k);
    if (rc) *got = 0;
    return rc;
}

extern "C" int bzx_decompress_range_device(bzx_ctx *ctx, const void *d_bz2, size_t len, uint64_t base, const bzx_index_entry *e,
                                           uint64_t n, uint64_t off, uint64_t want, void *d_out, size_t *got)
{
    return range_entry(ctx, d_bz2, len, base, e, n, off, want, d_out, got, false);
}

extern "C" int bzx_decompress_range_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint64_t base, const bzx_index_entry *e,
                                           uint64_t n, uint64_t off, uint64_t want, uint8_t *out, size_t *got)
{
    return range_entry(ctx, bz2, len, base, e, n, off, want, out, got, true);
}

// ---- the gather kernel alone, for the parity tests and the probe ----------------------------------------------------------
static int stage_gather(bzx_ctx *ctx, const uint8_t *src, size_t src_len, uint32_t nslices, const uint64_t *src_offs,
                        const uint64_t *dst_offs, const uint64_t *lens, uint8_t *out, size_t out_len, uint32_t reps, float *ms_best)
{
    if (!ctx || (nslices && (!src_offs || !dst_offs || !lens)) || (src_len && !src) || (out_len && !out)) return BZX_E_PARAM;
    for (uint32_t i = 0; i < nslices; i++) {
        if (src_offs[i] > src_len || lens[i] > src_len - src_offs[i] || dst_offs[i] > out_len || lens[i] > out_len - dst_offs[i]) {
            ctx->err = "bzx_stage_gather: slice " + std::to_string(i) + " leaves a buffer";
            return BZX_E_PARAM;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (both buffers start at a 256-byte boundary, so that an offset's low bits are the address's; the source is read in
    // aligned dwords: room for the one that holds its last byte)
    DevMem<> d_a, d_b;                           // (freed on return: every path below ends behind a synchronisation)
    if (!d_a.reserve(src_len + 512) || !d_b.reserve(out_len + 512)) {
        ctx->err = "bzx_stage_gather: device allocation failed";
        return BZX_E_NOMEM;
    }
    uint8_t *a = (uint8_t *)rg_al((size_t)(uintptr_t)d_a.get()), *b = (uint8_t *)rg_al((size_t)(uintptr_t)d_b.get());
    auto run = [&]() -> int {
        std::vector<RgSlice> sl;
        for (uint32_t i = 0; i < nslices; i++) rg_cut(sl, a + src_offs[i], b + dst_offs[i], lens[i]);
        if (src_len) HIP_TRY(ctx, hipMemcpyAsync(a, src, src_len, hipMemcpyHostToDevice, ctx->stream));
        if (out_len) HIP_TRY(ctx, hipMemcpyAsync(b, out, out_len, hipMemcpyHostToDevice, ctx->stream));
        float best = 0.f;
        for (uint32_t r = 0; r < reps; r++) {
            if (ms_best) HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
            const int rc = rg_gather(ctx, sl);
            if (rc) return rc;
            if (ms_best) {
                float ms = 0.f;
                HIP_TRY(ctx, hipEventRecord(ctx->ev[7], ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[7]));
                if (r == 0 || ms < best) best = ms;
            }
        }
        if (ms_best) *ms_best = best;
        if (out_len) HIP_TRY(ctx, hipMemcpyAsync(out, b, out_len, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return BZX_OK;
    };
    int rc = BZX_OK;
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

extern "C" int bzx_stage_gather(bzx_ctx *ctx, const uint8_t *src, size_t src_len, uint32_t nslices, const uint64_t *src_offs,
                                const uint64_t *dst_offs, const uint64_t *lens, uint8_t *out, size_t out_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    return stage_gather(ctx, src, src_len, nslices, src_offs, dst_offs, lens, out, out_len, 1, nullptr);
}

// ... under HIP events, for the probe: the best of `reps` launches in milliseconds.
extern "C" int bzx_stage_gather_time(bzx_ctx *ctx, const uint8_t *src, size_t src_len, uint32_t nslices, const uint64_t *src_offs,
                                     const uint64_t *dst_offs, const uint64_t *lens, uint8_t *out, size_t out_len, uint32_t reps,
                                     float *ms_best)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ms_best || reps == 0) return BZX_E_PARAM;
    return stage_gather(ctx, src, src_len, nslices, src_offs, dst_offs, lens, out, out_len, reps, ms_best);
}

// ---- the inverse BWT alone, for the parity tests and the probe ----------------------------------------------------------
// What the block decoder leaves, for `copies` copies of one block side by side (scaffolding): L and the byte counts in
// every slab (slab 0 from the host, the others from it on the device); the number of earlier occurrences of each byte and
// the descriptors stay in `in` for ibwt_arm.
struct IbwtIn {
    std::vector<uint32_t> occ, freq;
    std::vector<BzxBlock> d;
};

static int ibwt_load(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, uint32_t copies, IbwtIn &in)
{
    const int rc = ensure_blocks(ctx, copies);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    B.nblk = copies;
    B.blk_first = 0;
    B.blk_step = 1;
    try {
        in.occ.resize(n);
        in.freq.assign(260, 0);
        in.d.resize(copies);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
    for (size_t i = 0; i < n; i++) in.occ[i] = in.freq[L[i]]++;
    memset(in.d.data(), 0, copies * sizeof(BzxBlock));
    for (uint32_t b = 0; b < copies; b++) {
        in.d[b].n = (uint32_t)n;
        in.d[b].orig_ptr = orig_ptr;
    }
    HIP_TRY(ctx, hipMemcpyAsync(B.bwt, L, n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(B.freq, in.freq.data(), 260 * 4, hipMemcpyHostToDevice, st));
    for (uint32_t b = 1; b < copies; b++) {
        HIP_TRY(ctx, hipMemcpyAsync(B.bwt + (size_t)b * BZX_BLK_STRIDE, B.bwt, n, hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(B.freq + (size_t)b * 260, B.freq, 260 * 4, hipMemcpyDeviceToDevice, st));
    }
    return BZX_OK;
}

// The pack kernel overwrites the occurrence counts: they and the descriptors are put in place before every launch.
static int ibwt_arm(bzx_ctx *ctx, const IbwtIn &in)
{
    hipStream_t st = ctx->stream;
    const BzxBatch &B = ctx->B;
    const size_t n = in.occ.size();
    HIP_TRY(ctx, hipMemcpyAsync(B.rec_a, in.occ.data(), n * 4, hipMemcpyHostToDevice, st));
    for (uint32_t b = 1; b < B.nblk; b++)
        HIP_TRY(ctx, hipMemcpyAsync(B.rec_a + (size_t)b * BZX_MAX_N, B.rec_a, n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(B.blk, in.d.data(), B.nblk * sizeof(BzxBlock), hipMemcpyHostToDevice, st));
    return BZX_OK;
}

extern "C" int bzx_stage_ibwt(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, int wide, uint8_t *img_out,
                              uint8_t *raw_out, size_t raw_cap, uint64_t *raw_len, uint32_t *status)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !L || !img_out || !raw_len || !status || (raw_cap && !raw_out) || n == 0 || n > BZX_MAX_N || orig_ptr >= n)
        return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    DevMem<> d_raw;                              // (freed on return, behind the synchronisation below)
    if (!d_raw.reserve(raw_cap + 64)) {
        ctx->err = "bzx_stage_ibwt: hipMalloc(expansion) failed";
        return BZX_E_NOMEM;
    }
    const BzxDcDst dst{raw_cap ? d_raw.get() : nullptr, raw_cap};
    IbwtIn in;
    auto run = [&]() -> int {
        int rc;
        if ((rc = ibwt_load(ctx, L, n, orig_ptr, 1, in)) || (rc = ibwt_arm(ctx, in))) return rc;
        BzxDcDst *d_dst = reinterpret_cast<BzxDcDst *>(B.selector);      // (a slab the inverse BWT does not touch)
        HIP_TRY(ctx, hipMemcpyAsync(d_dst, &dst, sizeof(dst), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_in, 0xEE, n, st));
        if (wide) bzx_launch_dc_ibwt_wide(B, ctx->d_in, (uint32_t)n, st);
        else bzx_launch_dc_ibwt(B, ctx->d_in, st);
        bzx_launch_dc_expand(B, ctx->d_in, d_dst, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, B.blk, sizeof(BzxBlock), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(img_out, ctx->d_in, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        *status = ctx->h_blk[0].status;
        *raw_len = ctx->h_blk[0].pack_word;
        const size_t k = (size_t)std::min<uint64_t>(*raw_len, raw_cap);
        if (k && !*status) HIP_TRY(ctx, hipMemcpy(raw_out, d_raw, k, hipMemcpyDeviceToHost));
        return BZX_OK;
    };
    int rc;
    try {
        rc = run();
    } catch (const std::bad_alloc &) {             // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    (void)hipStreamSynchronize(st);
    return rc;
}

// The inverse BWT launchers alone under HIP events, for the probe: `copies` copies of one block side by side, `reps`
// launches, the best one's milliseconds.
extern "C" int bzx_stage_ibwt_time(bzx_ctx *ctx, const uint8_t *L, size_t n, uint32_t orig_ptr, int wide, uint32_t copies,
                                   uint32_t reps, float *ms_best)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !L || !ms_best || n == 0 || n > BZX_MAX_N || orig_ptr >= n || copies == 0 || reps == 0) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    try {
        IbwtIn in;
        int rc = ibwt_load(ctx, L, n, orig_ptr, copies, in);
        if (rc) return rc;
        hipStream_t st = ctx->stream;
        const BzxBatch &B = ctx->B;
        float best = 0.f;
        for (uint32_t r = 0; r < reps; r++) {
            if ((rc = ibwt_arm(ctx, in))) return rc;
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
    } catch (const std::bad_alloc &) {             // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
}
