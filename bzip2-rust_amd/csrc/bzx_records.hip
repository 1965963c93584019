// bzx_records.hip -- records (lines) of a .bz2 on gfx950 (include/bzx.h: bzx_records_*, bzx_decompress_records_*,
// bzx_stage_rec_*): "records [a, a + c) of what this .bz2 decodes to", a record being what one delimiter byte ends.
//
// The record table of an index says how many delimiters lie before every block; it comes from the index pass
// (bzx_index_count_records, bzx_dstream.hip, through bzx_launch_rec_count below) or from the raw bytes of a stream this
// library compressed (bzx_records_count_*).  With it the host names the block that holds a record boundary
// (bzx_records_span) and the file bytes a read needs (bzx_records_pieces); the device
//   count    bzx_rec_count_kernel: the delimiters of every segment of a table, one workgroup per segment
//   select   bzx_rec_select_kernel: the position of the j-th delimiter of a segment and the segment's count, one
//            workgroup per query
// Both cut a segment the same way (rec_cut): the head bytes up to the first 16-byte boundary, the body in 16-byte
// loads, the tail bytes.  The body is cut into tiles of 64 loads (1 KiB, one load per lane of a wave) and every wave of
// the workgroup takes a contiguous share of whole tiles; head and tail are a ballot of wave 0.  The sections -- head,
// the waves' shares, tail -- leave their counts in LDS (wave sums, no atomics); select then finds the section that holds
// delimiter j, and the one wave that owns it walks its share again, tile by tile, with a wave scan per tile.
// A byte is compared exactly: see rec_match.
//
// Locate (bzx_records_locate_*) decodes every distinct touched block once through the round of the range reads
// (rg_round, rg_verdict: bzx_range.hip) into the staging pool, then answers the round's queries with one launch of the
// select kernel: two host synchronisations per round, none per query.  A records read is one locate call over the
// 2 x count boundaries and one call of the many-ranges core over the byte ranges found.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bzx_host.h"
#include "bzx_wg.h"

#define REC_NT 512
#define REC_NW (REC_NT / 64)
#define REC_NSEC (REC_NW + 2)                    // sections of a segment: head, one share per wave, tail
#define REC_NONE 0xFFFFFFFFu

// One bit (bit 7) per byte of w that equals the byte repeated in rep.  Exact: the carry of the low seven bits never
// leaves its byte (0x7f + 0x7f < 0x100), so a byte's verdict does not depend on its neighbours, as it does in the
// usual (x - 0x01010101) & ~x & 0x80808080.
__device__ __forceinline__ uint32_t rec_match(uint32_t w, uint32_t rep)
{
    const uint32_t x = w ^ rep;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

__device__ __forceinline__ uint32_t rec_count16(const uint4 v, uint32_t rep)
{
    return (uint32_t)(__popc(rec_match(v.x, rep)) + __popc(rec_match(v.y, rep)) + __popc(rec_match(v.z, rep)) +
                      __popc(rec_match(v.w, rep)));
}

struct RecCut {
    uint32_t head, nvec, tail;     // bytes before the first 16-byte boundary, 16-byte loads, bytes behind them
    uint32_t share;                // loads of a wave's share: whole tiles of 64
};

__device__ __forceinline__ RecCut rec_cut(const uint8_t *p, uint32_t len)
{
    RecCut c;
    c.head = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u;
    if (c.head > len) c.head = len;
    c.nvec = (len - c.head) / 16;
    c.tail = len - c.head - c.nvec * 16;
    const uint32_t ntile = (c.nvec + 63) / 64;
    c.share = (ntile + REC_NW - 1) / REC_NW * 64;
    return c;
}

// The delimiters of every section into s_tot[REC_NSEC]; a barrier stands behind the last write.
__device__ __forceinline__ void rec_sections(const uint8_t *__restrict__ p, const RecCut &c, uint32_t delim, uint32_t rep,
                                             uint32_t *s_tot)
{
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(p + c.head);
    const uint32_t v0 = wave * c.share;
    const uint32_t v1 = v0 + c.share < c.nvec ? v0 + c.share : c.nvec;
    uint32_t acc = 0;
    for (uint32_t v = v0 + lane; v < v1; v += 64) acc += rec_count16(body[v], rep);
    const uint32_t incl = bzx_wave_incl_sum(acc);
    if (lane == 63) s_tot[1 + wave] = incl;
    if (wave == 0) {
        const uint8_t *__restrict__ tl = p + c.head + (size_t)c.nvec * 16;
        const unsigned long long mh = __ballot(lane < c.head && p[lane] == delim);
        const unsigned long long mt = __ballot(lane < c.tail && tl[lane] == delim);
        if (lane == 0) {
            s_tot[0] = (uint32_t)__popcll(mh);
            s_tot[REC_NW + 1] = (uint32_t)__popcll(mt);
        }
    }
    __syncthreads();
}

// ---- count: one workgroup per segment, the grid rule of bzx_dc_crc_kernel --------------------------------------------------
__global__ __launch_bounds__(REC_NT) void bzx_rec_count_kernel(const BzxBlock *__restrict__ blk, const BzxDcDst *__restrict__ seg,
                                                               uint32_t nseg, uint32_t delim, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_tot[REC_NSEC];
    const uint32_t rep = delim * 0x01010101u;
    for (uint32_t b = blockIdx.x; b < nseg; b += gridDim.x) {
        if ((blk && blk[b].status) || !seg[b].p) continue;   // (uniform over the workgroup)
        uint64_t len = seg[b].cap;
        if (blk && blk[b].pack_word < len) len = blk[b].pack_word;
        const uint8_t *p = seg[b].p;
        const RecCut c = rec_cut(p, (uint32_t)len);
        rec_sections(p, c, delim, rep, s_tot);
        if (threadIdx.x == 0) {
            uint32_t total = 0;
            for (uint32_t i = 0; i < REC_NSEC; i++) total += s_tot[i];
            counts[b] = total;
        }
        __syncthreads();                                     // (s_tot is written again for the next segment)
    }
}

void bzx_launch_rec_count(const BzxBlock *blk, const BzxDcDst *seg, uint32_t nseg, uint32_t delim, uint32_t *counts,
                          uint32_t n_cu, hipStream_t stream)
{
    if (!nseg) return;
    hipLaunchKernelGGL(bzx_rec_count_kernel, dim3(nseg < n_cu ? nseg : n_cu), dim3(REC_NT), 0, stream, blk, seg, nseg, delim,
                       counts);
}

// ---- select: one workgroup per query ---------------------------------------------------------------------------------------
struct RecQuery {
    const uint8_t *p;              // the segment
    uint32_t len;
    uint32_t j;                    // which delimiter, counted from 1
};
struct RecAnswer {
    uint32_t pos;                  // of delimiter j in the segment; REC_NONE: j is 0 or above cnt
    uint32_t cnt;                  // delimiters of the segment
};

// Delimiter k (1..popcount) of a lane's 16 bytes: its byte number.
__device__ __forceinline__ uint32_t rec_pick16(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t k)
{
    uint32_t at = 0;
    const uint32_t c0 = (uint32_t)__popc(m0), c1 = (uint32_t)__popc(m1), c2 = (uint32_t)__popc(m2);
    uint32_t m = m0;
    if (k > c0) {
        k -= c0;
        m = m1;
        at = 4;
        if (k > c1) {
            k -= c1;
            m = m2;
            at = 8;
            if (k > c2) {
                k -= c2;
                m = m3;
                at = 12;
            }
        }
    }
    // m has bits 7, 15, 23, 31 only: the k-th set one
    uint32_t b = 0;
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) {
        const uint32_t hit = (m >> (8 * b + 7)) & 1u;
        if (hit && k == 1) break;
        k -= hit;
        b++;
    }
    return at + b;
}

__global__ __launch_bounds__(REC_NT) void bzx_rec_select_kernel(const RecQuery *__restrict__ q, uint32_t delim,
                                                                RecAnswer *__restrict__ out)
{
    __shared__ uint32_t s_tot[REC_NSEC];
    const RecQuery Q = q[blockIdx.x];
    const uint32_t rep = delim * 0x01010101u;
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    const uint8_t *__restrict__ p = Q.p;
    const RecCut c = rec_cut(p, Q.len);
    rec_sections(p, c, delim, rep, s_tot);
    uint32_t total = 0, sec = REC_NSEC, before = 0;
    for (uint32_t i = 0; i < REC_NSEC; i++) {
        const uint32_t t = s_tot[i];
        if (sec == REC_NSEC && Q.j > total && Q.j - total <= t) {
            sec = i;
            before = total;
        }
        total += t;
    }
    if (threadIdx.x == 0) {
        out[blockIdx.x].cnt = total;
        if (sec == REC_NSEC) out[blockIdx.x].pos = REC_NONE;
    }
    if (sec == REC_NSEC) return;                             // (uniform: j is 0 or above the count)
    uint32_t rem = Q.j - before;                             // 1 .. the section's count
    if (sec == 0 || sec == REC_NW + 1) {                     // head or tail: wave 0, one byte per lane
        if (wave != 0) return;
        const uint32_t base = sec == 0 ? 0u : c.head + c.nvec * 16, nb = sec == 0 ? c.head : c.tail;
        const bool hit = lane < nb && p[base + lane] == delim;
        const unsigned long long m = __ballot(hit);
        if (hit && (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) == rem - 1) out[blockIdx.x].pos = base + lane;
        return;
    }
    if (wave != sec - 1) return;                             // the wave that owns the share walks it again
    const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(p + c.head);
    const uint32_t v0 = wave * c.share;
    const uint32_t v1 = v0 + c.share < c.nvec ? v0 + c.share : c.nvec;
    for (uint32_t vb = v0; vb < v1; vb += 64) {              // (uniform over the wave)
        const uint32_t v = vb + lane;
        uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
        if (v < v1) {
            const uint4 x = body[v];
            m0 = rec_match(x.x, rep);
            m1 = rec_match(x.y, rep);
            m2 = rec_match(x.z, rep);
            m3 = rec_match(x.w, rep);
        }
        const uint32_t mine = (uint32_t)(__popc(m0) + __popc(m1) + __popc(m2) + __popc(m3));
        const uint32_t incl = bzx_wave_incl_sum(mine);
        const uint32_t tile = __shfl(incl, 63);
        if (rem <= tile) {
            if (incl >= rem && incl - mine < rem)            // the one lane whose 16 bytes hold it
                out[blockIdx.x].pos = c.head + v * 16 + rec_pick16(m0, m1, m2, m3, rem - (incl - mine));
            return;
        }
        rem -= tile;
    }
}

// ---- host: tables and planners (no context, no device) ---------------------------------------------------------------------
// rec_before[0, n]: starts at 0 and never descends.
static bool rec_table_ok(const uint64_t *rb, uint64_t n)
{
    if (!rb || rb[0] != 0) return false;
    for (uint64_t k = 0; k < n; k++)
        if (rb[k + 1] < rb[k]) return false;
    return true;
}

// The entry that holds delimiter r (the smallest k with rec_before[k + 1] >= r) and which of its delimiters it is; the
// table has been checked.
static void rec_span(const uint64_t *rb, uint64_t n, uint64_t r, uint64_t *entry, uint64_t *j)
{
    if (r == 0) {
        *entry = 0;
        *j = 0;
    } else if (r > rb[n]) {
        *entry = n;
        *j = 0;
    } else {
        const uint64_t k = (uint64_t)(std::lower_bound(rb + 1, rb + n + 1, r) - (rb + 1));
        *entry = k;
        *j = r - rb[k];
    }
}

extern "C" int bzx_records_span(const uint64_t *rec_before, uint64_t n, uint64_t r, uint64_t *entry, uint64_t *j)
{
    if (!entry || !j || !rec_table_ok(rec_before, n)) return BZX_E_PARAM;
    rec_span(rec_before, n, r, entry, j);
    return BZX_OK;
}

static uint64_t rec_add(uint64_t a, uint64_t b) { return b > ~0ull - a ? ~0ull : a + b; }

// The entries [*first, *end) that locating and reading records [lo, lo + cnt) touch: from the entry that holds delimiter
// lo (entry 0 for lo == 0) to the one that holds delimiter lo + cnt, clipped to the index; none for a range that starts
// behind the last delimiter's record or that is [0, 0).
static void rec_touched(const uint64_t *rb, uint64_t n, uint64_t lo, uint64_t cnt, uint64_t *first, uint64_t *end)
{
    *first = *end = 0;
    const uint64_t hi = rec_add(lo, cnt);
    uint64_t a = 0, b = 0, j = 0;
    if (lo) rec_span(rb, n, lo, &a, &j);
    if (a >= n || hi == 0) return;
    rec_span(rb, n, hi, &b, &j);
    *first = a;
    *end = std::min<uint64_t>(b, n - 1) + 1;
}

extern "C" int bzx_records_pieces(const bzx_index_entry *e, uint64_t n, const uint64_t *rec_before, uint32_t count,
                                  const uint64_t *rec_los, const uint64_t *rec_cnts, uint64_t *bases, uint64_t *lens,
                                  uint32_t cap_pieces, uint32_t *npieces)
{
    if (!npieces || (n && !e) || (count && (!rec_los || !rec_cnts)) || (cap_pieces && (!bases || !lens)) ||
        !rec_table_ok(rec_before, n))
        return BZX_E_PARAM;
    *npieces = 0;
    try {
        std::vector<std::pair<uint64_t, uint64_t>> iv;
        for (uint32_t i = 0; i < count; i++) {
            uint64_t a, z;
            rec_touched(rec_before, n, rec_los[i], rec_cnts[i], &a, &z);
            if (z > a) iv.push_back({a, z});
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

// ---- the table from the raw side ---------------------------------------------------------------------------------------------
static int rec_count_raw(bzx_ctx *ctx, const uint8_t *raw, size_t len, int delim, const bzx_index_entry *e, uint64_t n,
                         uint64_t *rec_before, bool host)
{
    if (!ctx || !rec_before || (n && !e) || (len && !raw) || delim < 0 || delim > 255) return BZX_E_PARAM;
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (e[k].out_off != at) {
            ctx->err = "bzx_records_count: out_off is not the running sum of out_len (block " + std::to_string(k) + ")";
            return BZX_E_PARAM;
        }
        at += e[k].out_len;
    }
    if (at != len) {
        ctx->err = "bzx_records_count: the entries do not end at len";
        return BZX_E_PARAM;
    }
    rec_before[0] = 0;
    if (!n) return BZX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t STEP = (uint64_t)1 << 20;                 // segments per launch
    const size_t m = (size_t)std::min<uint64_t>(n, STEP);
    DevMem<> d_raw, d_tab;                       // (freed on return: every path below ends behind a synchronisation)
    if ((host && !d_raw.reserve(len + 64)) || !d_tab.reserve(m * (sizeof(BzxDcDst) + 4))) {
        ctx->err = "bzx_records_count: device allocation failed";
        return BZX_E_NOMEM;
    }
    auto run = [&]() -> int {
        const uint8_t *d = raw;
        if (host) {
            HIP_TRY(ctx, hipMemcpyAsync(d_raw.get(), raw, len, hipMemcpyHostToDevice, st));
            d = d_raw.get();
        }
        std::vector<BzxDcDst> seg(m);
        std::vector<uint32_t> cnt(m);
        BzxDcDst *d_seg = d_tab.get<BzxDcDst>();
        uint32_t *d_cnt = reinterpret_cast<uint32_t *>(d_seg + m);
        for (uint64_t k0 = 0; k0 < n; k0 += STEP) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(STEP, n - k0);
            for (uint32_t i = 0; i < nb; i++) seg[i] = BzxDcDst{const_cast<uint8_t *>(d) + e[k0 + i].out_off, e[k0 + i].out_len};
            HIP_TRY(ctx, hipMemcpyAsync(d_seg, seg.data(), nb * sizeof(BzxDcDst), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, nb * 4, st));
            bzx_launch_rec_count(nullptr, d_seg, nb, (uint32_t)delim, d_cnt, (uint32_t)ctx->n_cu, st);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_cnt, nb * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            for (uint32_t i = 0; i < nb; i++) rec_before[k0 + i + 1] = rec_before[k0 + i] + cnt[i];
        }
        return BZX_OK;
    };
    int rc;
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    (void)hipStreamSynchronize(st);
    return rc;
}

extern "C" int bzx_records_count_device(bzx_ctx *ctx, const void *d_raw, size_t len, int delim, const bzx_index_entry *e,
                                        uint64_t n, uint64_t *rec_before)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    return rec_count_raw(ctx, (const uint8_t *)d_raw, len, delim, e, n, rec_before, false);
}

extern "C" int bzx_records_count_buffer(bzx_ctx *ctx, const uint8_t *raw, size_t len, int delim, const bzx_index_entry *e,
                                        uint64_t n, uint64_t *rec_before)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    return rec_count_raw(ctx, raw, len, delim, e, n, rec_before, true);
}

// ---- locate ----------------------------------------------------------------------------------------------------------------
struct RecBlk {
    uint64_t k;                    // the entry
    uint32_t piece;                // the piece that holds its input bytes
    size_t q0, q1;                 // its queries: ord[q0, q1)
    uint64_t pool_off;
};

// What fails single queries is noted in status[] and `why` (the text of the lowest failed one); a return value other
// than BZX_OK fails the whole call.
static int locate_call(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n,
                       const uint64_t *rb, int delim, uint32_t count, const uint64_t *recs, uint64_t *byte_offs, int *status,
                       bool host, uint64_t *fail_k, std::vector<std::string> *texts)
{
    if (!rec_table_ok(rb, n)) {
        ctx->err = "record read: the record table does not start at 0 or descends";
        return BZX_E_PARAM;
    }
    for (uint32_t j = 0; j < npc; j++) {
        if ((pc[j].len && !pc[j].p) || pc[j].len > ~0ull - pc[j].base || (j && pc[j].base < pc[j - 1].base + pc[j - 1].len)) {
            ctx->err = "record read: the pieces of the input are not ascending and disjoint (piece " + std::to_string(j) + ")";
            return BZX_E_PARAM;
        }
    }
    const uint64_t total = n ? e[n - 1].out_off + e[n - 1].out_len : 0;
    std::vector<uint64_t> qk(count), qj(count);
    std::vector<uint32_t> ord;
    std::string why;
    *fail_k = ~0ull;
    auto fail = [&](uint32_t i, const std::string &text) {
        status[i] = BZX_E_DATA;
        byte_offs[i] = 0;
        if (texts) (*texts)[i] = text;
        if (i < *fail_k) {
            *fail_k = i;
            why = text;
        }
    };
    for (uint32_t i = 0; i < count; i++) {
        status[i] = BZX_OK;
        rec_span(rb, n, recs[i], &qk[i], &qj[i]);
        if (qj[i] == 0) byte_offs[i] = recs[i] ? total : 0;
        else ord.push_back(i);
    }
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return qk[a] != qk[b] ? qk[a] < qk[b] : a < b; });
    std::vector<RecBlk> blk;
    for (size_t q = 0; q < ord.size();) {
        const uint64_t k = qk[ord[q]];
        size_t q1 = q;
        while (q1 < ord.size() && qk[ord[q1]] == k) q1++;
        const bzx_index_entry &x = e[k];
        if (x.out_len == 0 || x.out_len > RG_EDGE_BYTES - 16) {
            for (size_t u = q; u < q1; u++)
                fail(ord[u], "index does not match the input: an entry's out_len is 0 or exceeds a block (block " + std::to_string(k) + ")");
        } else {
            uint64_t blo, bhi;
            rg_block_bytes(x, &blo, &bhi);
            const bzx_piece *w = std::upper_bound(pc, pc + npc, blo, [](uint64_t v, const bzx_piece &y) { return v < y.base; });
            if (w == pc || bhi > w[-1].base + w[-1].len) {
                ctx->err = "query " + std::to_string(ord[q]) + ": record read: the input bytes given do not cover bytes [" +
                           std::to_string(blo) + ", " + std::to_string(bhi) + ") of the file in one piece (bzx_records_pieces)";
                return BZX_E_PARAM;
            }
            blk.push_back(RecBlk{k, (uint32_t)(w - 1 - pc), q, q1, 0});
        }
        q = q1;
    }
    if (!blk.empty()) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        std::vector<const uint8_t *> d_pc(npc, nullptr);
        int rc;
        if (host) {
            std::vector<uint8_t> held(npc, 0);
            for (const RecBlk &b : blk) held[b.piece] = 1;
            if ((rc = rg_upload(ctx, pc, npc, held.data(), d_pc.data()))) return rc;
        } else {
            for (uint32_t j = 0; j < npc; j++) d_pc[j] = (const uint8_t *)pc[j].p;
        }
        if ((rc = ensure_blocks(ctx, 1))) return rc;
        const uint32_t R = ctx->cap_slabs;
        RgTables t;
        if ((rc = rg_tables(ctx, R, &t))) return rc;
        std::vector<BzxDcSrc> src(R);
        std::vector<BzxDcDst> dst(R);
        std::vector<uint32_t> len(R);
        std::vector<uint32_t> who;                           // the round's queries, as the device answers them
        for (size_t i = 0; i < blk.size();) {
            uint32_t nb = 0, n_hint = 0;
            uint64_t used = 0;
            size_t nq = 0;
            for (; i + nb < blk.size() && nb < R; nb++) {
                RecBlk &b = blk[i + nb];
                const bzx_index_entry &x = e[b.k];
                if (used + rg_al(x.out_len) > RG_POOL_BYTES) break;      // (one block always fits)
                b.pool_off = used;
                used += rg_al(x.out_len);
                dst[nb] = BzxDcDst{t.pool + b.pool_off, x.out_len};
                n_hint = std::max<uint32_t>(n_hint, (uint32_t)std::min<uint64_t>(BZX_MAX_N, (uint64_t)x.out_len * 5 / 4 + 8));
                src[nb] = BzxDcSrc{d_pc[b.piece], pc[b.piece].len, x.bit - pc[b.piece].base * 8};
                len[nb] = x.out_len;
                nq += b.q1 - b.q0;
            }
            if ((rc = rg_round(ctx, t, nb, src.data(), dst.data(), len.data(), n_hint))) return rc;      // synchronisation 1
            RecQuery *h_q = nullptr;
            RecAnswer *h_a = nullptr;
            RecQuery *d_q = nullptr;
            RecAnswer *d_a = nullptr;
            const bool ok = carved(ctx->rec_ws, 256, [&](Carver &c) {
                d_q = c.take<RecQuery>(std::max<size_t>(nq, 4096));
                d_a = c.take<RecAnswer>(std::max<size_t>(nq, 4096));
            }) && carved(ctx->rec_pin, 256, [&](Carver &c) {
                h_q = c.take<RecQuery>(std::max<size_t>(nq, 4096));
                h_a = c.take<RecAnswer>(std::max<size_t>(nq, 4096));
            });
            if (!ok) {
                ctx->rec_ws.reset();
                ctx->rec_pin.reset();
                ctx->err = "record read: device or pinned allocation failed";
                return BZX_E_NOMEM;
            }
            who.clear();
            for (uint32_t j = 0; j < nb; j++) {
                const RecBlk &b = blk[i + j];
                const bzx_index_entry &x = e[b.k];
                if (rg_verdict(ctx, x, b.k, ctx->h_blk[j], t.h_flag[j], t.h_got[j])) {      // fails the queries that touch it
                    for (size_t u = b.q0; u < b.q1; u++) fail(ord[u], ctx->err);
                    continue;
                }
                for (size_t u = b.q0; u < b.q1; u++) {
                    h_q[who.size()] = RecQuery{t.pool + b.pool_off, x.out_len, (uint32_t)qj[ord[u]]};
                    who.push_back(ord[u]);
                }
            }
            if (!who.empty()) {
                const uint32_t m = (uint32_t)who.size();
                HIP_TRY(ctx, hipMemcpyAsync(d_q, h_q, m * sizeof(RecQuery), hipMemcpyHostToDevice, st));
                const uint32_t GMAX = 1u << 30;                                             // (a grid holds 2^31 - 1 workgroups)
                for (uint32_t g = 0; g < m; g += GMAX)
                    hipLaunchKernelGGL(bzx_rec_select_kernel, dim3(std::min(GMAX, m - g)), dim3(REC_NT), 0, st, d_q + g,
                                       (uint32_t)delim, d_a + g);
                HIP_TRY(ctx, hipGetLastError());
                HIP_TRY(ctx, hipMemcpyAsync(h_a, d_a, m * sizeof(RecAnswer), hipMemcpyDeviceToHost, st));
                HIP_TRY(ctx, hipStreamSynchronize(st));                                     // synchronisation 2
                for (uint32_t u = 0; u < m; u++) {
                    const uint32_t qi = who[u];
                    const uint64_t k = qk[qi], says = rb[k + 1] - rb[k];
                    if (h_a[u].cnt != says || h_a[u].pos >= e[k].out_len)
                        fail(qi, "record table does not match the input: block " + std::to_string(k) + " holds " +
                                     std::to_string(h_a[u].cnt) + " delimiters, the table says " + std::to_string(says));
                    else byte_offs[qi] = e[k].out_off + h_a[u].pos + 1;
                }
            }
            i += nb;
        }
    }
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->stats_batch = true;
    ctx->stats.nblk = (uint32_t)blk.size();
    if (*fail_k != ~0ull) {
        ctx->err = why;
        return BZX_E_DATA;
    }
    return BZX_OK;
}

// ... with nothing unwinding across the C ABI and nothing of a failed call left in flight.
static int locate_core(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, const uint64_t *rb,
                       int delim, uint32_t count, const uint64_t *recs, uint64_t *byte_offs, int *status, bool host,
                       uint64_t *fail_k, std::vector<std::string> *texts)
{
    int rc;
    try {
        rc = locate_call(ctx, pc, npc, e, n, rb, delim, count, recs, byte_offs, status, host, fail_k, texts);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (rc && rc != BZX_E_DATA) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

static int locate_entry(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, const uint64_t *rb,
                        int delim, uint32_t count, const uint64_t *recs, uint64_t *byte_offs, int *status, bool host)
{
    auto api_lock_ = ctx_lock(ctx);
    int rc = BZX_OK;
    bool whole = true;                           // rc fails the whole call: it goes into every status
    if (!ctx) {
        rc = BZX_E_PARAM;
    } else if (ctx->ds) {
        rc = refuse_streaming(ctx);
    } else if (count == 0) {
        return BZX_OK;
    } else if (!recs || !byte_offs || !status || !rb || (n && !e) || (npc && !pc) || delim < 0 || delim > 255) {
        ctx->err = "record read: a NULL array or a delimiter outside 0..255";
        rc = BZX_E_PARAM;
    } else {
        uint64_t fail_k = 0;
        rc = locate_core(ctx, pc, npc, e, n, rb, delim, count, recs, byte_offs, status, host, &fail_k, nullptr);
        whole = rc != BZX_OK && rc != BZX_E_DATA;            // (BZX_E_DATA: the statuses are set, query by query)
        if (rc == BZX_E_DATA) ctx->err = "query " + std::to_string(fail_k) + ": " + ctx->err;
    }
    if (rc && whole) {
        for (uint32_t i = 0; i < count; i++) {
            if (status) status[i] = rc;
            if (byte_offs) byte_offs[i] = 0;
        }
    }
    return rc;
}

extern "C" int bzx_records_locate_device(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                         uint64_t n, const uint64_t *rec_before, int delim, uint32_t count,
                                         const uint64_t *recs, uint64_t *byte_offs, int *status)
{
    return locate_entry(ctx, pieces, npieces, e, n, rec_before, delim, count, recs, byte_offs, status, false);
}

extern "C" int bzx_records_locate_buffer(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                         uint64_t n, const uint64_t *rec_before, int delim, uint32_t count,
                                         const uint64_t *recs, uint64_t *byte_offs, int *status)
{
    return locate_entry(ctx, pieces, npieces, e, n, rec_before, delim, count, recs, byte_offs, status, true);
}

// ---- read: one locate call over the 2 x count boundaries, one call of the many-ranges core -----------------------------------
static int records_read(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, const uint64_t *rb,
                        int delim, uint32_t count, const uint64_t *los, const uint64_t *cnts, void *out, size_t cap,
                        size_t *out_offs, size_t *gots, int *status, size_t *need, bool host)
{
    std::vector<uint64_t> recs((size_t)count * 2), at((size_t)count * 2), offs(count), wants(count);
    std::vector<int> st((size_t)count * 2);
    std::vector<std::string> texts((size_t)count * 2);
    for (uint32_t i = 0; i < count; i++) {
        recs[2 * (size_t)i] = los[i];
        recs[2 * (size_t)i + 1] = rec_add(los[i], cnts[i]);
    }
    uint64_t fail_q = 0;
    int rc = locate_core(ctx, pc, npc, e, n, rb, delim, count * 2, recs.data(), at.data(), st.data(), host, &fail_q, &texts);
    if (rc && rc != BZX_E_DATA) return rc;
    for (uint32_t i = 0; i < count; i++) {
        const bool bad = st[2 * (size_t)i] || st[2 * (size_t)i + 1];
        offs[i] = bad ? 0 : at[2 * (size_t)i];
        wants[i] = bad ? 0 : at[2 * (size_t)i + 1] - at[2 * (size_t)i];
    }
    rc = host ? bzx_decompress_ranges_buffer(ctx, pc, npc, e, n, count, offs.data(), wants.data(), (uint8_t *)out, cap, out_offs,
                                             gots, status, need)
              : bzx_decompress_ranges_device(ctx, pc, npc, e, n, count, offs.data(), wants.data(), out, cap, out_offs, gots,
                                             status, need);
    if (rc && rc != BZX_E_DATA) return rc;
    const std::string ranges_text = ctx->err;
    int first_rc = BZX_OK;
    for (uint32_t i = 0; i < count; i++) {
        const std::string &t0 = texts[2 * (size_t)i], &t1 = texts[2 * (size_t)i + 1];
        if (st[2 * (size_t)i] || st[2 * (size_t)i + 1]) {
            status[i] = BZX_E_DATA;
            gots[i] = 0;
            if (!first_rc) ctx->err = "range " + std::to_string(i) + ": " + (st[2 * (size_t)i] ? t0 : t1);
        } else if (status[i] && !first_rc) {
            ctx->err = ranges_text;                          // (the ranges call names its lowest failing range: this one)
        }
        if (status[i] && !first_rc) first_rc = status[i];
    }
    return first_rc;
}

static int records_entry(bzx_ctx *ctx, const bzx_piece *pc, uint32_t npc, const bzx_index_entry *e, uint64_t n, const uint64_t *rb,
                         int delim, uint32_t count, const uint64_t *los, const uint64_t *cnts, void *out, size_t cap,
                         size_t *out_offs, size_t *gots, int *status, size_t *need, bool host)
{
    auto api_lock_ = ctx_lock(ctx);
    if (need) *need = 0;
    int rc = BZX_OK;
    if (!ctx) {
        rc = BZX_E_PARAM;
    } else if (ctx->ds) {
        rc = refuse_streaming(ctx);
    } else if (count == 0) {
        return BZX_OK;
    } else if (!los || !cnts || !out_offs || !gots || !status || !need || !rb || (n && !e) || (npc && !pc) || delim < 0 ||
               delim > 255 || count > 0x7FFFFFFFu) {
        ctx->err = "record read: a NULL array, a delimiter outside 0..255 or more than 2^31 - 1 ranges";
        rc = BZX_E_PARAM;
    } else {
        try {
            rc = records_read(ctx, pc, npc, e, n, rb, delim, count, los, cnts, out, cap, out_offs, gots, status, need, host);
        } catch (const std::bad_alloc &) {
            ctx->err = "out of host memory";
            rc = BZX_E_NOMEM;
        }
    }
    if (rc && rc != BZX_E_DATA) {
        for (uint32_t i = 0; i < count; i++) {
            if (status) status[i] = rc;
            if (gots) gots[i] = 0;
        }
    }
    return rc;
}

extern "C" int bzx_decompress_records_device(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                             uint64_t n, const uint64_t *rec_before, int delim, uint32_t count,
                                             const uint64_t *rec_los, const uint64_t *rec_cnts, void *d_out, size_t cap,
                                             size_t *out_offs, size_t *gots, int *status, size_t *need)
{
    return records_entry(ctx, pieces, npieces, e, n, rec_before, delim, count, rec_los, rec_cnts, d_out, cap, out_offs, gots,
                         status, need, false);
}

extern "C" int bzx_decompress_records_buffer(bzx_ctx *ctx, const bzx_piece *pieces, uint32_t npieces, const bzx_index_entry *e,
                                             uint64_t n, const uint64_t *rec_before, int delim, uint32_t count,
                                             const uint64_t *rec_los, const uint64_t *rec_cnts, uint8_t *out, size_t cap,
                                             size_t *out_offs, size_t *gots, int *status, size_t *need)
{
    return records_entry(ctx, pieces, npieces, e, n, rec_before, delim, count, rec_los, rec_cnts, out, cap, out_offs, gots,
                         status, need, true);
}

// ---- the two kernels alone, for the parity tests (host pointers) -----------------------------------------------------------
// The device copy of buf starts on a 256-byte boundary, so seg_offs[i] mod 16 is the alignment the kernel sees.
static int stage_rec(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                     const uint64_t *seg_lens, const uint32_t *js, int delim, uint32_t *pos_out, uint32_t *cnt_out)
{
    if (!ctx || (len && !buf) || (nseg && (!seg_offs || !seg_lens || !cnt_out)) || delim < 0 || delim > 255) return BZX_E_PARAM;
    for (uint32_t i = 0; i < nseg; i++) {
        if (seg_offs[i] > len || seg_lens[i] > len - seg_offs[i] || seg_lens[i] > 0xFFFFFFFFull) {
            ctx->err = "bzx_stage_rec: segment " + std::to_string(i) + " leaves the buffer";
            return BZX_E_PARAM;
        }
    }
    if (!nseg) return BZX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevMem<> d_buf, d_tab;                       // (freed on return: every path below ends behind a synchronisation)
    if (!d_buf.reserve(len + 512) || !d_tab.reserve((size_t)nseg * (16 + 8))) {
        ctx->err = "bzx_stage_rec: device allocation failed";
        return BZX_E_NOMEM;
    }
    uint8_t *d = (uint8_t *)rg_al((size_t)(uintptr_t)d_buf.get());
    auto run = [&]() -> int {
        if (len) HIP_TRY(ctx, hipMemcpyAsync(d, buf, len, hipMemcpyHostToDevice, st));
        if (js) {
            std::vector<RecQuery> q(nseg);
            std::vector<RecAnswer> a(nseg);
            for (uint32_t i = 0; i < nseg; i++) q[i] = RecQuery{d + seg_offs[i], (uint32_t)seg_lens[i], js[i]};
            RecQuery *d_q = d_tab.get<RecQuery>();
            RecAnswer *d_a = reinterpret_cast<RecAnswer *>(d_q + nseg);
            HIP_TRY(ctx, hipMemcpyAsync(d_q, q.data(), nseg * sizeof(RecQuery), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(d_a, 0xEE, nseg * sizeof(RecAnswer), st));
            hipLaunchKernelGGL(bzx_rec_select_kernel, dim3(nseg), dim3(REC_NT), 0, st, d_q, (uint32_t)delim, d_a);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(a.data(), d_a, nseg * sizeof(RecAnswer), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            for (uint32_t i = 0; i < nseg; i++) {
                pos_out[i] = a[i].pos;
                cnt_out[i] = a[i].cnt;
            }
        } else {
            std::vector<BzxDcDst> seg(nseg);
            for (uint32_t i = 0; i < nseg; i++) seg[i] = BzxDcDst{d + seg_offs[i], seg_lens[i]};
            BzxDcDst *d_seg = d_tab.get<BzxDcDst>();
            uint32_t *d_cnt = reinterpret_cast<uint32_t *>(d_seg + nseg);
            HIP_TRY(ctx, hipMemcpyAsync(d_seg, seg.data(), nseg * sizeof(BzxDcDst), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0xEE, (size_t)nseg * 4, st));
            bzx_launch_rec_count(nullptr, d_seg, nseg, (uint32_t)delim, d_cnt, (uint32_t)ctx->n_cu, st);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(cnt_out, d_cnt, (size_t)nseg * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        return BZX_OK;
    };
    int rc;
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    (void)hipStreamSynchronize(st);
    return rc;
}

extern "C" int bzx_stage_rec_count(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                                   const uint64_t *seg_lens, int delim, uint32_t *counts_out)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    return stage_rec(ctx, buf, len, nseg, seg_offs, seg_lens, nullptr, delim, nullptr, counts_out);
}

extern "C" int bzx_stage_rec_select(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nq, const uint64_t *seg_offs,
                                    const uint64_t *seg_lens, const uint32_t *js, int delim, uint32_t *pos_out,
                                    uint32_t *cnt_out)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (nq && (!js || !pos_out)) return BZX_E_PARAM;
    return stage_rec(ctx, buf, len, nq, seg_offs, seg_lens, js, delim, pos_out, cnt_out);
}
