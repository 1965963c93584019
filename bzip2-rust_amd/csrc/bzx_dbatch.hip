// bzx_dbatch.hip -- the host decoder on gfx950: many .bz2 inputs (each one stream or several concatenated) in one
// call (bzx_decompress_batch_*); the one-shot calls (bzx_decompress_device / _buffer) are its count = 1.
//
// The kernels that decode one block (bzx_decomp.hip: decode, inverse BWT, expand, CRC) work over any set of blocks;
// what a batch needs around them is segmented:
//   scan, once per call   every input gets scan tiles of its own (tile -> input map), so no read window crosses an
//                         input's end.  A candidate is (input, bit, kind); an end-of-stream candidate also carries
//                         the stored combined CRC and the level of a "BZh1..9" header at the next byte boundary with
//                         14 bytes left (0: none), so the host follows the streams of an input without reading device
//                         memory.  Thread 0 of an input's first tile checks its first four bytes.  The table's size
//                         comes from the call; an overflow (chance matches only) rescans with the exact size.
//   per device round      (whole inputs, at most R block candidates)
//     decode              every block candidate of the round, through its own (input pointer, length, start bit),
//                         with the 900000 limit; the host refuses n > 100000 * level of the block's stream
//     [sync 1]            the host walks each input's chain from bit 32: blocks, end-of-stream, footer, the next
//                         stream.  Candidates off the chain (chance matches of the magic in compressed data) and the
//                         blocks of refused inputs get a nonzero status: the later kernels skip them
//     inverse BWT         unchanged (bzx_launch_dc_ibwt); the walk leaves each block's expanded size in pack_word
//     layout              one workgroup: per input, an exclusive scan of its chain blocks' sizes -> every block's
//                         destination; an input whose total exceeds its cap (or whose walk failed) is flagged and
//                         neither expanded nor checked
//     expand, CRC         bzx_dc_expand_kernel and bzx_dc_crc_kernel through BzxDcDst
//     [sync 2]            one copy of CRCs, sizes and flags; the host checks block and combined CRCs
// Host synchronisations: one after the scan (two after a table overflow), two per round, none per input or stream.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bzx_host.h"
#include "bzx_wg.h"

#define DB_TILE 1024               // scan tile: 256 lanes x 4 byte offsets
#define DB_NT 1024                 // layout kernel (one workgroup)

struct DbIn {                      // one input of the call (scan)
    const uint8_t *z;
    uint64_t len;
    uint64_t tile0;
};

struct DbCand {                    // a magic found by the scan
    uint64_t pos;                  // bit << 5 | next header level << 1 | end-of-stream
    uint32_t input;
    uint32_t crc;                  // end-of-stream: the stored combined CRC (0 when the input ends first)
};

struct DbIo {                      // one input of a round (layout)
    uint8_t *out;                  // device output (null: placed in the round's staging area, the _buffer form)
    uint64_t cap;
    uint32_t c0, nc;               // its chain blocks: chain[c0, c0 + nc) (round block numbers)
    uint32_t live;                 // 0: refused already, nothing to lay out
    uint32_t flag;                 // out: 0 ok, 1 a block failed the inverse BWT, 2 total > cap
    uint64_t total;                // out: decoded bytes
    uint64_t at;                   // out: offset in the staging area
};

// ---- scan ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bzx_db_scan_kernel(const DbIn *__restrict__ in, const uint32_t *__restrict__ tile_in,
                                                          uint64_t ntiles, DbCand *__restrict__ cand,
                                                          uint32_t *__restrict__ n_cand, uint32_t cap,
                                                          uint32_t *__restrict__ level)
{
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile_in[tile];
        const DbIn s = in[i];
        const uint8_t *__restrict__ z = s.z;
        if (tile == s.tile0 && threadIdx.x == 0) level[i] = s.len >= 14 ? bzx_bzh_level(z) : 0u;
        const uint64_t byte0 = (tile - s.tile0) * DB_TILE + (uint64_t)threadIdx.x * 4;
        if (byte0 >= s.len) continue;
        bzx_dc_scan_word(z, s.len, byte0, [&](uint64_t bit, bool eos, uint64_t x, uint64_t y) {
            if (bit < 32) return;                           // (the stream header)
            DbCand c;
            c.input = i;
            c.crc = 0;
            uint32_t next = 0;
            if (eos) {
                if (bit + 80 <= s.len * 8) c.crc = (uint32_t)(((x & 0xFFFFull) << 16) | (y >> 48));
                const uint64_t at = (bit + 80 + 7) / 8;
                if (at + 14 <= s.len) next = bzx_bzh_level(z + at);
            }
            c.pos = (bit << 5) | (next << 1) | (eos ? 1u : 0u);
            const uint32_t k = atomicAdd(n_cand, 1u);
            if (k < cap) cand[k] = c;
        });
    }
}

// ---- layout of a round: per input, its chain blocks' destinations (one workgroup) ---------------------------------
__global__ __launch_bounds__(DB_NT) void bzx_db_layout_kernel(BzxBatch B, DbIo *__restrict__ io, uint32_t nio,
                                                              const uint32_t *__restrict__ chain, uint8_t *staging,
                                                              BzxDcDst *__restrict__ dst, uint64_t *__restrict__ end)
{
    __shared__ uint64_t wsum[DB_NT / 64];
    const uint32_t tid = threadIdx.x, lane = bzx_lane(), wave = bzx_wave();
    uint64_t carry = 0;
    for (uint32_t r0 = 0; r0 < nio; r0 += DB_NT) {
        const uint32_t r = r0 + tid;
        DbIo d;
        uint64_t total = 0;
        uint32_t flag = 0;
        if (r < nio) {
            d = io[r];
            for (uint32_t j = 0; j < d.nc; j++) {
                const BzxBlock &k = B.blk[chain[d.c0 + j]];
                if (k.status) flag = 1;
                total += k.pack_word;
            }
            if (!flag && total > d.cap) flag = 2;
        }
        const uint64_t size = (r < nio && d.live && !flag) ? total : 0;
        // exclusive scan of the sizes over the workgroup (the staging offsets of the _buffer form)
        const uint64_t x = bzx_wave_incl_sum64(size);
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint64_t pre = 0, tot = 0;
        for (uint32_t w = 0; w < DB_NT / 64; w++) {
            if (w < wave) pre += wsum[w];
            tot += wsum[w];
        }
        __syncthreads();
        const uint64_t at = carry + pre + x - size;
        carry += tot;
        if (r < nio) {
            io[r].flag = flag;
            io[r].total = total;
            io[r].at = at;
            uint8_t *out = staging ? staging + at : d.out;
            uint64_t off = 0;
            for (uint32_t j = 0; j < d.nc; j++) {
                const uint32_t b = chain[d.c0 + j];
                dst[b] = flag ? BzxDcDst{nullptr, 0} : BzxDcDst{out + off, total - off};
                off += B.blk[b].pack_word;
            }
        }
    }
    if (tid == 0) end[0] = carry;
}

// ---- host side ------------------------------------------------------------------------------------------------
// The tables of a call are carved out of ctx->dbatch_ws and ctx->dbatch_pin[0], both grown on demand: first the scan's,
// then -- the scan's are dead by then -- the rounds'.  Every table starts on a 16-byte boundary.
template <typename M, typename F> static int db_tables(bzx_ctx *ctx, M &mem, const char *what, F &&layout)
{
    if (carved(mem, 16, layout)) return BZX_OK;
    ctx->err = std::string(what) + "(batch decompression tables) failed";
    return BZX_E_NOMEM;
}

static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// Largest expansion of an RLE1 image of n bytes: every 5 bytes (4 equal and a count) become at most 259.
static uint64_t db_expand_bound(uint64_t n) { return n / 5 * 259 + n % 5; }

// The verdicts of one call of the core.  reason[i]: why input i failed.
struct DbResult {
    std::vector<std::string> reason;
    uint32_t nblk = 0;
    uint64_t raw_bytes = 0;
};

// The batch on device inputs.  d_outs null (the _buffer form): each round's outputs are packed into a device staging
// area and copied, one copy per round, into the pinned bounce buffer; then into h_outs[i] on the host.
// one_stream (bzx_decompress_device): an input whose first stream is followed by another is refused, once that first
// stream has passed every check of its own.
static int dbatch_run(bzx_ctx *ctx, uint32_t count, const void *const *d_srcs, const size_t *src_lens,
                      void *const *d_outs, uint8_t *const *h_outs, const size_t *caps, size_t *out_lens, int *status,
                      DbResult &res, bool one_stream = false)
{
    hipStream_t st = ctx->stream;
    res.reason.assign(count, std::string());
    // ---- scan tables
    std::vector<DbIn> in(count);
    uint64_t ntiles = 0, total_len = 0;
    for (uint32_t i = 0; i < count; i++) {
        in[i].z = (const uint8_t *)d_srcs[i];
        in[i].len = src_lens[i];
        in[i].tile0 = ntiles;
        ntiles += src_lens[i] ? (src_lens[i] + DB_TILE - 1) / DB_TILE : 0;
        total_len += src_lens[i];
        out_lens[i] = 0;
        status[i] = BZX_OK;
    }
    std::vector<uint32_t> tile_in(ntiles);
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t t1 = i + 1 < count ? in[i + 1].tile0 : ntiles;
        for (uint64_t t = in[i].tile0; t < t1; t++) tile_in[t] = i;
    }
    uint64_t cap_cand = (uint64_t)count * 4 + total_len / 2048 + 1024;
    uint32_t ncand = 0;
    std::vector<uint32_t> level(count, 0);
    DbCand *h_cand = nullptr;
    for (int pass = 0;; pass++) {
        if (cap_cand > 0xffffffffu) cap_cand = 0xffffffffu;
        DbIn *d_in = nullptr;
        DbCand *d_cand = nullptr;
        uint32_t *d_tile_in = nullptr, *d_level = nullptr, *d_ncand = nullptr, *h_level = nullptr, *h_ncand = nullptr;
        int rc = db_tables(ctx, ctx->dbatch_ws, "hipMalloc", [&](Carver &c) {
            d_in = c.take<DbIn>(count);
            d_tile_in = c.take<uint32_t>(ntiles);
            d_cand = c.take<DbCand>(cap_cand);
            d_level = c.take<uint32_t>(count);
            d_ncand = c.take<uint32_t>(4);
        });
        if (rc) return rc;
        rc = db_tables(ctx, ctx->dbatch_pin[0], "hipHostMalloc", [&](Carver &c) {
            h_cand = c.take<DbCand>(cap_cand);
            h_level = c.take<uint32_t>(count);
            h_ncand = c.take<uint32_t>(4);
        });
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_in, in.data(), count * sizeof(DbIn), hipMemcpyHostToDevice, st));
        if (ntiles) HIP_TRY(ctx, hipMemcpyAsync(d_tile_in, tile_in.data(), ntiles * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(d_level, 0, (size_t)count * 4, st));
        HIP_TRY(ctx, hipMemsetAsync(d_ncand, 0, 4, st));
        if (ntiles) {
            const uint64_t g = (uint64_t)ctx->n_cu * 8;
            hipLaunchKernelGGL(bzx_db_scan_kernel, dim3((uint32_t)(ntiles < g ? ntiles : g)), dim3(256), 0, st, d_in,
                               d_tile_in, ntiles, d_cand, d_ncand, (uint32_t)cap_cand, d_level);
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemcpyAsync(h_ncand, d_ncand, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(h_level, d_level, (size_t)count * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(h_cand, d_cand, cap_cand * sizeof(DbCand), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));              // the call's one synchronisation (two after an overflow)
        ncand = *h_ncand;
        memcpy(level.data(), h_level, (size_t)count * 4);
        if (ncand <= cap_cand) break;
        if (pass) {
            ctx->err = "batch decompression: the magic scan found more candidates on its second pass";
            return BZX_E_HIP;
        }
        cap_cand = ncand;
    }
    std::vector<DbCand> cand(h_cand, h_cand + ncand);
    std::sort(cand.begin(), cand.end(), [](const DbCand &a, const DbCand &b) {
        return a.input != b.input ? a.input < b.input : a.pos < b.pos;
    });
    // per input: its candidates [c_first[i], c_first[i + 1]) and its block candidates
    std::vector<uint32_t> c_first(count + 1, 0), nblkc(count, 0);
    for (const DbCand &c : cand) {
        c_first[c.input + 1]++;
        if (!(c.pos & 1u)) nblkc[c.input]++;
    }
    for (uint32_t i = 0; i < count; i++) c_first[i + 1] += c_first[i];
    uint32_t R = ctx->cap_slabs;
    for (uint32_t i = 0; i < count; i++) {
        if (!level[i]) {
            status[i] = BZX_E_DATA;
            res.reason[i] = dc_why_text(src_lens[i] < 14 ? DC_WHY_SHORT : DC_WHY_NO_HEADER);
            nblkc[i] = 0;
        }
        if (nblkc[i] > R) R = nblkc[i];
    }
    int rc = ensure_blocks(ctx, R);
    if (rc) return rc;
    // ---- round tables: device [src R][dst R][got R][chain R][io count][end], pinned [io count][got R][end]
    BzxDcSrc *d_src = nullptr;
    BzxDcDst *d_dst = nullptr;
    uint32_t *d_got = nullptr, *d_chain = nullptr, *h_got = nullptr;
    DbIo *d_io = nullptr, *h_io = nullptr;
    uint64_t *d_end = nullptr, *h_end = nullptr;
    rc = db_tables(ctx, ctx->dbatch_ws, "hipMalloc", [&](Carver &c) {
        d_src = c.take<BzxDcSrc>(R);
        d_dst = c.take<BzxDcDst>(R);
        d_got = c.take<uint32_t>(R);
        d_chain = c.take<uint32_t>(R);
        d_io = c.take<DbIo>(count);
        d_end = c.take<uint64_t>(2);
    });
    if (rc) return rc;
    rc = db_tables(ctx, ctx->dbatch_pin[0], "hipHostMalloc", [&](Carver &c) {
        h_io = c.take<DbIo>(count);
        h_got = c.take<uint32_t>(R);
        h_end = c.take<uint64_t>(2);
    });
    if (rc) return rc;

    BzxBatch &B = ctx->B;
    B.blk_first = 0;
    B.blk_step = 1;
    DevMem<> stg;                                // _buffer form: the round's outputs, packed
    struct Pending {                             // _buffer form: outputs of the last round, in the bounce buffer
        uint32_t i;
        uint64_t at, n;
    };
    std::vector<Pending> pending;
    auto drain = [&]() {                         // after a synchronisation: the bounce buffer holds them
        for (const Pending &p : pending) memcpy(h_outs[p.i], ctx->dbatch_pin[1] + p.at, p.n);
        pending.clear();
    };
    std::vector<BzxDcSrc> src;
    std::vector<uint32_t> blk_in, chain;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> streams;   // per round input: (chain blocks, stored CRC)
    for (uint32_t i0 = 0; i0 < count && !rc;) {
        uint32_t i1 = i0, nb = 0;
        while (i1 < count && nb + nblkc[i1] <= R) nb += nblkc[i1++];
        const uint32_t nio = i1 - i0;
        // block candidates of the round, in input order
        src.clear();
        blk_in.clear();
        std::vector<uint32_t> b_first(nio + 1, 0);
        for (uint32_t i = i0; i < i1; i++) {
            b_first[i - i0] = (uint32_t)src.size();
            if (status[i]) continue;
            for (uint32_t c = c_first[i]; c < c_first[i + 1]; c++)
                if (!(cand[c].pos & 1u)) {
                    src.push_back(BzxDcSrc{in[i].z, in[i].len, cand[c].pos >> 5});
                    blk_in.push_back(i);
                }
        }
        b_first[nio] = (uint32_t)src.size();
        B.nblk = nb;
        if (nb) {
            HIP_TRY(ctx, hipMemcpyAsync(d_src, src.data(), nb * sizeof(BzxDcSrc), hipMemcpyHostToDevice, st));
            bzx_launch_dc_decode(B, d_src, st);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, B.blk, nb * sizeof(BzxBlock), hipMemcpyDeviceToHost, st));
        }
        if (nb || !pending.empty()) HIP_TRY(ctx, hipStreamSynchronize(st));   // round synchronisation 1: descriptors
        drain();
        // ---- chain walk of every input of the round
        std::vector<uint8_t> on_chain(nb, 0), follows(nio, 0);
        chain.clear();
        streams.assign(nio, {});
        uint64_t staging_need = 0;
        for (uint32_t r = 0; r < nio; r++) {
            const uint32_t i = i0 + r;
            DbIo &io = h_io[r];
            io.out = d_outs ? (uint8_t *)d_outs[i] : nullptr;
            io.cap = caps[i];
            io.c0 = (uint32_t)chain.size();
            io.nc = 0;
            io.live = 0;
            if (status[i]) continue;
            const uint32_t cb0 = b_first[r];
            // candidates of input i sorted by pos; block candidate k of the input is round block cb0 + k
            std::vector<uint32_t> blk_of(c_first[i + 1] - c_first[i]);
            for (uint32_t c = c_first[i], k = 0; c < c_first[i + 1]; c++)
                blk_of[c - c_first[i]] = (cand[c].pos & 1u) ? 0xffffffffu : cb0 + k++;
            auto find = [&](uint64_t bit) -> int64_t {
                const DbCand *lo = cand.data() + c_first[i], *hi = cand.data() + c_first[i + 1];
                const DbCand *p = std::lower_bound(lo, hi, bit << 5, [](const DbCand &a, uint64_t v) { return a.pos < v; });
                return (p < hi && (p->pos >> 5) == bit) ? p - lo : -1;
            };
            uint64_t end_bit = 32;
            uint32_t lvl = level[i], s_first = (uint32_t)chain.size();
            uint32_t why = DC_OK;
            uint64_t bound = 0;
            for (;;) {
                const int64_t k = find(end_bit);
                if (k < 0) {
                    why = DC_WHY_NO_EOS;
                    break;
                }
                const DbCand &c = cand[c_first[i] + k];
                if (!(c.pos & 1u)) {
                    const uint32_t b = blk_of[k];
                    const BzxBlock &d = ctx->h_blk[b];
                    if (d.status & BZX_ST_DC_RANDOMISED) {
                        why = DC_WHY_RANDOMISED;
                        break;
                    }
                    if (d.status || d.n > 100000u * lvl) {
                        why = DC_WHY_DAMAGED;
                        break;
                    }
                    chain.push_back(b);
                    on_chain[b] = 1;
                    bound += db_expand_bound(d.n);
                    end_bit = d.bits;
                    continue;
                }
                if ((end_bit + 80 + 7) / 8 > in[i].len) {
                    why = DC_WHY_TRUNC_EOS;
                    break;
                }
                streams[r].push_back({(uint32_t)chain.size() - s_first, c.crc});
                s_first = (uint32_t)chain.size();
                const uint32_t next = (uint32_t)(c.pos >> 1) & 15u;
                follows[r] = one_stream && next;
                if (!next || one_stream) break;
                end_bit = 8 * ((end_bit + 80 + 7) / 8) + 32;
                lvl = next;
            }
            if (why) {
                status[i] = BZX_E_DATA;
                res.reason[i] = dc_why_text(why);
                for (uint32_t b = io.c0; b < chain.size(); b++) on_chain[chain[b]] = 0;
                chain.resize(io.c0);
                streams[r].clear();
                continue;
            }
            io.nc = (uint32_t)chain.size() - io.c0;
            io.live = 1;
            staging_need += al16(std::min<uint64_t>(caps[i], bound));
        }
        for (uint32_t b = 0; b < nb; b++)
            if (!on_chain[b]) ctx->h_blk[b].status |= DC_SKIP;
        if (!d_outs && !stg.reserve(staging_need)) {
            ctx->err = "hipMalloc(batch output staging) failed";
            return BZX_E_NOMEM;
        }
        // ---- inverse BWT, layout, expansion and CRCs of the chain blocks; no synchronisation in between
        if (nb) {
            HIP_TRY(ctx, hipMemcpyAsync(B.blk, ctx->h_blk, nb * sizeof(BzxBlock), hipMemcpyHostToDevice, st));
            if (!chain.empty())
                HIP_TRY(ctx, hipMemcpyAsync(d_chain, chain.data(), chain.size() * 4, hipMemcpyHostToDevice, st));
            bzx_launch_dc_ibwt(B, ctx->d_in, st);
        }
        HIP_TRY(ctx, hipMemcpyAsync(d_io, h_io, nio * sizeof(DbIo), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(bzx_db_layout_kernel, dim3(1), dim3(DB_NT), 0, st, B, d_io, nio, d_chain,
                           d_outs ? nullptr : stg.get(), d_dst, d_end);
        if (nb) {
            bzx_launch_dc_expand(B, ctx->d_in, d_dst, st);
            bzx_launch_dc_crc(B, d_dst, d_got, (uint32_t)ctx->n_cu, st);
            HIP_TRY(ctx, hipMemcpyAsync(h_got, d_got, nb * 4, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(h_io, d_io, nio * sizeof(DbIo), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(h_end, d_end, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));              // round synchronisation 2: CRCs, sizes and flags
        // ---- verdicts
        for (uint32_t r = 0; r < nio; r++) {
            const uint32_t i = i0 + r;
            const DbIo &io = h_io[r];
            if (status[i] || !io.live) continue;
            if (io.flag == 1) {
                status[i] = BZX_E_DATA;
                res.reason[i] = dc_why_text(DC_WHY_IBWT);
                continue;
            }
            if (io.flag == 2) {
                status[i] = BZX_E_OUTBUF;
                out_lens[i] = (size_t)io.total;
                res.reason[i] = dc_why_text(DC_WHY_OUTBUF);
                continue;
            }
            uint32_t why = DC_OK, bad_blk = 0;                 // (bad_blk: the block's number within its input)
            uint32_t k = io.c0;
            for (const auto &s : streams[r]) {
                uint32_t comb = 0;
                for (uint32_t j = 0; j < s.first; j++, k++) {
                    const uint32_t b = chain[k];
                    if (!why && h_got[b] != ctx->h_blk[b].crc) {
                        why = DC_WHY_BLOCK_CRC;
                        bad_blk = k - io.c0;
                    }
                    comb = crc_fold(comb, ctx->h_blk[b].crc);      // stored CRCs
                }
                if (!why && comb != s.second) why = DC_WHY_COMBINED_CRC;
            }
            if (!why && follows[r]) why = DC_WHY_STREAM_FOLLOWS;
            if (why) {
                status[i] = BZX_E_DATA;
                res.reason[i] = dc_why_text(why, bad_blk);
                continue;
            }
            out_lens[i] = (size_t)io.total;
            res.nblk += io.nc;
            res.raw_bytes += io.total;
            if (!d_outs && io.total) pending.push_back(Pending{i, io.at, io.total});
        }
        if (!d_outs && *h_end) {                             // the round's outputs, one copy into the bounce buffer
            if (!ctx->dbatch_pin[1].reserve(*h_end)) {
                ctx->err = "hipHostMalloc(batch decompression tables) failed";
                rc = BZX_E_NOMEM;
                break;
            }
            if (hipMemcpyAsync(ctx->dbatch_pin[1], stg, *h_end, hipMemcpyDeviceToHost, st) != hipSuccess) {
                ctx->err = "hipMemcpyAsync(batch output) failed";
                rc = BZX_E_HIP;
                break;
            }
        }
        i0 = i1;
    }
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = BZX_E_HIP;
    if (!rc) drain();
    return rc;
}

// Argument checks shared by both forms.
static int dbatch_args(bzx_ctx *ctx, const char *fn, uint32_t count, const void *srcs, const size_t *src_lens,
                       const void *const *outs, const size_t *caps, const size_t *out_lens, const int *status, bool device)
{
    if (!srcs || !src_lens || !outs || !caps || !out_lens || !status) {
        ctx->err = std::string(fn) + ": NULL array";
        return BZX_E_PARAM;
    }
    const void *const *s = (const void *const *)srcs;
    for (uint32_t i = 0; i < count; i++) {
        if (src_lens[i] && !s[i]) {
            ctx->err = std::string(fn) + ": input " + std::to_string(i) + ": NULL pointer with a non-zero length";
            return BZX_E_PARAM;
        }
        if (caps[i] && !outs[i]) {
            ctx->err = std::string(fn) + ": input " + std::to_string(i) + ": NULL output with a non-zero cap";
            return BZX_E_PARAM;
        }
        if (device && ((uintptr_t)outs[i] & 15u)) {
            ctx->err = std::string(fn) + ": input " + std::to_string(i) + ": d_outs[" + std::to_string(i) +
                       "] must be 16-byte aligned";
            return BZX_E_PARAM;
        }
    }
    return BZX_OK;
}

// Return value of a call: the lowest failing input's status, named in bzx_last_error; a call-wide error sets every
// status to itself.
static int dbatch_finish(bzx_ctx *ctx, const char *fn, int rc, uint32_t count, int *status, const DbResult &res)
{
    if (rc) {
        if (status)
            for (uint32_t i = 0; i < count; i++) status[i] = rc;
        (void)hipStreamSynchronize(ctx->stream);             // nothing of a failed call is left in flight
        return rc;
    }
    for (uint32_t i = 0; i < count; i++)
        if (status[i]) {
            ctx->err = std::string(fn) + ": input " + std::to_string(i) + ": " + res.reason[i];
            return status[i];
        }
    return BZX_OK;
}

static void dbatch_stats(bzx_ctx *ctx, const DbResult &res, float ms)
{
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->stats_batch = true;
    ctx->stats.nblk = res.nblk;
    ctx->stats.raw_bytes = res.raw_bytes;
    ctx->stats.ms_total = ms;
}

extern "C" int bzx_decompress_batch_device(bzx_ctx *ctx, uint32_t count, const void *const *d_srcs, const size_t *src_lens,
                                           void *const *d_outs, const size_t *caps, size_t *out_lens, int *status)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx) return BZX_E_PARAM;
    if (count == 0) return BZX_OK;
    const char *fn = "bzx_decompress_batch_device";
    DbResult res;
    int rc = dbatch_args(ctx, fn, count, d_srcs, src_lens, d_outs, caps, out_lens, status, true);
    if (!rc && hipSetDevice(ctx->device) != hipSuccess) {
        ctx->err = "hipSetDevice failed";
        rc = BZX_E_HIP;
    }
    if (!rc) {
        (void)hipEventRecord(ctx->ev[5], ctx->stream);
        try {
            rc = dbatch_run(ctx, count, d_srcs, src_lens, d_outs, nullptr, caps, out_lens, status, res);
        } catch (const std::bad_alloc &) {             // (nothing may unwind across the C ABI)
            ctx->err = "out of host memory";
            rc = BZX_E_NOMEM;
        }
        if (!rc) {
            float ms = 0.f;
            (void)hipEventRecord(ctx->ev[7], ctx->stream);
            (void)hipEventSynchronize(ctx->ev[7]);
            (void)hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[7]);
            dbatch_stats(ctx, res, ms);
        }
    }
    return dbatch_finish(ctx, fn, rc, count, status, res);
}

#define DB_GROUP_BYTES (256ull << 20)    // _buffer form: compressed bytes staged on the device at once

extern "C" int bzx_decompress_batch_buffer(bzx_ctx *ctx, uint32_t count, const uint8_t *const *srcs, const size_t *src_lens,
                                           uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx) return BZX_E_PARAM;
    if (count == 0) return BZX_OK;
    const char *fn = "bzx_decompress_batch_buffer";
    DbResult all;
    int rc = dbatch_args(ctx, fn, count, srcs, src_lens, (const void *const *)outs, caps, out_lens, status, false);
    if (!rc && hipSetDevice(ctx->device) != hipSuccess) {
        ctx->err = "hipSetDevice failed";
        rc = BZX_E_HIP;
    }
    DevMem<> d_in;                               // the staged inputs of a group (freed on return, behind the synchronisations)
    if (!rc) {
        (void)hipEventRecord(ctx->ev[5], ctx->stream);
        try {
            all.reason.assign(count, std::string());
            // groups of whole inputs with at most DB_GROUP_BYTES compressed bytes (or one larger input), staged and run
            for (uint32_t g0 = 0; g0 < count && !rc;) {
                uint32_t g1 = g0;
                size_t staged = 0;
                while (g1 < count && (g1 == g0 || staged + al16(src_lens[g1]) <= DB_GROUP_BYTES)) staged += al16(src_lens[g1++]);
                if (!d_in.reserve(staged)) {
                    ctx->err = "hipMalloc(batch inputs) failed";
                    rc = BZX_E_NOMEM;
                    break;
                }
                std::vector<const void *> d_srcs(g1 - g0, nullptr);
                size_t at = 0;
                for (uint32_t i = g0; i < g1 && !rc; i++) {
                    d_srcs[i - g0] = d_in + at;
                    if (src_lens[i] &&
                        hipMemcpyAsync(d_in + at, srcs[i], src_lens[i], hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
                        ctx->err = "hipMemcpyAsync(batch input) failed";
                        rc = BZX_E_HIP;
                    }
                    at += al16(src_lens[i]);
                }
                DbResult res;
                if (!rc)
                    rc = dbatch_run(ctx, g1 - g0, d_srcs.data(), src_lens + g0, nullptr, outs + g0, caps + g0, out_lens + g0,
                                    status + g0, res);
                if (!rc) {
                    for (uint32_t i = g0; i < g1; i++) all.reason[i] = res.reason[i - g0];
                    all.nblk += res.nblk;
                    all.raw_bytes += res.raw_bytes;
                }
                g0 = g1;
            }
        } catch (const std::bad_alloc &) {             // (nothing may unwind across the C ABI)
            ctx->err = "out of host memory";
            rc = BZX_E_NOMEM;
        }
        (void)hipStreamSynchronize(ctx->stream);
        if (!rc) {
            float ms = 0.f;
            (void)hipEventRecord(ctx->ev[7], ctx->stream);
            (void)hipEventSynchronize(ctx->ev[7]);
            (void)hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[7]);
            dbatch_stats(ctx, all, ms);
        }
    }
    return dbatch_finish(ctx, fn, rc, count, status, all);
}

// ---- the one-shot calls: one input through the core; its status is the return value, its reason the error text ------
static int dbatch_one(bzx_ctx *ctx, const void *d_bz2, size_t len, void *d_out, size_t cap, size_t *out_len, bool one_stream)
{
    DbResult res;
    int status = BZX_OK, rc;
    try {
        rc = dbatch_run(ctx, 1, &d_bz2, &len, &d_out, nullptr, &cap, out_len, &status, res, one_stream);
    } catch (const std::bad_alloc &) {                 // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);             // nothing of a failed call is left in flight
        return rc;
    }
    if (status) {
        ctx->err = res.reason[0];
        return status;
    }
    ctx->stats.nblk = res.nblk;                              // (the other fields stay: the last compression's)
    ctx->stats.raw_bytes = res.raw_bytes;
    ctx->stats_batch = true;                                 // the pinned descriptors are candidates, not blocks
    return BZX_OK;
}

// Device buffer -> device buffer: ONE stream (the reference's decompress() also stops at the first footer,
// decompress.rs:81-95).  Bytes behind the footer that are not another stream are ignored, as bzip2 does ("trailing
// garbage"); a concatenated .bz2 (pbzip2 output, cat a.bz2 b.bz2) is refused here rather than decoded in part --
// bzx_decompress_buffer decodes every stream of it.
extern "C" int bzx_decompress_device(bzx_ctx *ctx, const void *d_bz2, size_t len, void *d_out, size_t cap, size_t *out_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !d_bz2 || !out_len || (cap && !d_out) || ((uintptr_t)d_out & 15u)) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dbatch_one(ctx, d_bz2, len, d_out, cap, out_len, true);
}

// Host buffer -> host buffer, every stream of the input: upload, one core call into a device output of cap bytes, copy
// back what was decoded.
extern "C" int bzx_decompress_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint8_t *out, size_t cap, size_t *out_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !bz2 || !out_len || (cap && !out)) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out_len = 0;
    DevMem<> d_z, d_o;                           // (freed on return, behind the synchronisation below)
    if (!d_z.reserve(len + 64) || !d_o.reserve(cap + 64)) {
        ctx->err = "bzx_decompress_buffer: device allocation failed";
        return BZX_E_NOMEM;
    }
    int rc = hipMemcpyAsync(d_z, bz2, len, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? BZX_OK : BZX_E_HIP;
    if (!rc) rc = dbatch_one(ctx, d_z, len, d_o, cap, out_len, false);
    if (!rc && *out_len && hipMemcpy(out, d_o, *out_len, hipMemcpyDeviceToHost) != hipSuccess) rc = BZX_E_HIP;
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}
