// bzx_batch.hip -- batched compression on gfx950: many independent inputs, one .bz2 stream each.
//
// The stage kernels (BWT, MTF, Huffman, emit) already work over any set of blocks; what a batch needs around them is
// the split, the layout and the framing of MANY inputs at once:
//   split analysis, once per call over all inputs (kernels A, B, C of bzx_rle1.hip, segmented):
//     every input starts on a fresh 8 KiB tile and a tile knows its input (tile_seg); A and B load a tile through its
//     input's pointer at local positions, so the byte before an input's first byte is "none" and is never read.
//     Run starts are kept as tile0 * 8192 + local position + 1: each input's first byte starts a run, so the global
//     max-scan carries nothing across inputs; the RLE1 offsets are a global sum-scan minus the input's base.
//     C: one workgroup per input walks its chain of boundaries (bzx_split_chain) into slots of its own.
//   per device round (whole inputs, at most R blocks; batch_run below):
//     describe  block descriptors and block -> input map of the round (one wave per input)
//     scatter   the RLE1'd bytes of every block into its slab (plain tiles are copied; no block is read in place,
//               there is no single raw base)
//     crc       CRC-32/BZIP2 of every block's raw range, through its input's pointer
//     (run_stages: BWT .. Huffman, unchanged)
//     layout    per stream: out_bit = 8 * off + 32 + exclusive scan of the block sizes inside the stream; stream
//               length (32 + bits + 80 + 7) / 8; off = running offset + exclusive scan of the lengths rounded up to 4
//     (emit, unchanged: streams start on 32-bit words, so no word is shared by two streams)
//     frame     one wave per stream: "BZh<level>", footer magic, combined CRC over the stream's blocks (0 without blocks)
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include "bzx_host.h"
#include "bzx_rle1.h"

#define BT_NT 1024        // layout kernel (one workgroup)
#define BX_NT 256         // index kernel: entries per workgroup
#define BX_WORDS 5        // 64-bit words of a bzx_index_entry
static_assert(sizeof(bzx_index_entry) == BX_WORDS * 8 && (BX_NT * BX_WORDS) % 2 == 0, "index entries: whole 16-byte vectors per workgroup");

__device__ __forceinline__ uint64_t bt_carry(const BzxBatchWs &ws, const BzxSeg &s, uint64_t tile)
{
    const uint64_t v = ws.tile_rs[tile], base = s.tile0 * RL_TILE;
    return v > base ? v - base : 0;
}

// ---- A: last run start per tile, in the call's position numbering
__global__ __launch_bounds__(RL_NT) void bzx_bt_runstart_kernel(BzxBatchWs ws)
{
    __shared__ uint64_t scratch[RL_NT / 64];
    for (uint64_t tile = blockIdx.x; tile < ws.ntiles; tile += gridDim.x) {
        const BzxSeg s = ws.seg[ws.tile_seg[tile]];
        bool any4;
        const uint64_t tot = bzx_tile_runstart(s.raw, s.len, tile - s.tile0, scratch, any4);
        if (threadIdx.x == 0) {
            ws.tile_rs[tile] = tot ? tot + s.tile0 * RL_TILE : 0;
            ws.tile_np[tile] = any4 ? 1 : 0;     // provisional: 0 = plain for sure, B skips the tile
            ws.tile_off[tile] = RL_TILE;
        }
    }
}

// ---- B: emitted bytes of the tiles that may hold a run position k >= 3 (256 tiles per step, flags read coalesced)
__global__ __launch_bounds__(RL_NT) void bzx_bt_count_kernel(BzxBatchWs ws)
{
    __shared__ uint64_t s64[RL_NT / 64];
    __shared__ uint32_t s32[RL_NT / 64];
    __shared__ uint32_t s_list[RL_NT];
    __shared__ uint32_t s_cnt;
    for (uint64_t base = (uint64_t)blockIdx.x * RL_NT; base < ws.ntiles; base += (uint64_t)gridDim.x * RL_NT) {
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        {
            const uint64_t tile = base + threadIdx.x;
            if (tile < ws.ntiles && ws.tile_np[tile]) s_list[atomicAdd(&s_cnt, 1u)] = threadIdx.x;
        }
        __syncthreads();
        const uint32_t nlist = s_cnt;
        for (uint32_t k = 0; k < nlist; k++) {
            const uint64_t tile = base + s_list[k];
            const BzxSeg s = ws.seg[ws.tile_seg[tile]];
            TileInfo ti;
            tile_analyse(s.raw, s.len, tile - s.tile0, bt_carry(ws, s, tile), s64, s32, ti);
            const bool np = __syncthreads_or(ti.any_long);
            if (threadIdx.x == 0) {
                ws.tile_off[tile] = ti.f_total;
                ws.tile_np[tile] = np ? 1 : 0;
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// ---- C: block boundaries, one workgroup per input
__global__ __launch_bounds__(RL_NT) void bzx_bt_boundaries_kernel(BzxBatchWs ws, uint32_t nmax)
{
    __shared__ BzxChainLds lds;
    for (uint32_t i = blockIdx.x; i < ws.count; i += gridDim.x) {
        const BzxSeg s = ws.seg[i];
        BzxChainIO io;
        io.tile_rs = ws.tile_rs + s.tile0;
        io.tile_off = ws.tile_off + s.tile0;
        io.tile_np = ws.tile_np + s.tile0;
        io.rs_base = s.tile0 * RL_TILE;
        io.f_base = ws.tile_off[s.tile0];
        io.blk_raw = ws.blk_raw + s.slot0;
        io.blk_f = ws.blk_f + s.slot0;
        io.blk_plain = ws.blk_plain + s.slot0;
        io.max_blocks = s.nslot - 1;
        const uint32_t nb = bzx_split_chain(s.raw, s.len, (s.len + RL_TILE - 1) / RL_TILE, nmax, io, lds);
        if (threadIdx.x == 0) ws.seg_nblk[i] = nb;     // 0xffffffff: more blocks than slots (the host refuses the call)
        __syncthreads();
    }
}

// ---- describe: descriptors of the round's blocks [0, nb) (inputs [i0, i1), whose first block is rb0), one wave per input
__global__ __launch_bounds__(256) void bzx_bt_describe_kernel(BzxBatchWs ws, uint32_t i0, uint32_t i1, uint32_t rb0,
                                                              BzxBlock *__restrict__ blk)
{
    const uint32_t i = i0 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= i1) return;
    const uint32_t n = ws.seg_nblk[i], b0 = ws.seg_blk[i] - rb0, slot0 = ws.seg[i].slot0;
    for (uint32_t j = lane; j < n; j += 64) {
        const uint32_t b = b0 + j;
        ws.blk_seg[b] = i;
        blk[b].in_off = (uint64_t)b * BZX_BLK_STRIDE;
        blk[b].n = (uint32_t)(ws.blk_f[slot0 + j + 1] - ws.blk_f[slot0 + j]);
        blk[b].status = 0;
    }
}

// ---- D: scatter the emitted bytes of tiles [t0, t1) (the tiles of the round's inputs) into the block slabs
__global__ __launch_bounds__(RL_NT) void bzx_bt_scatter_kernel(BzxBatchWs ws, uint64_t t0, uint64_t t1, uint32_t rb0,
                                                               uint8_t *__restrict__ slabs)
{
    __shared__ uint64_t s64[RL_NT / 64];
    __shared__ uint32_t s32[RL_NT / 64];
    for (uint64_t tile = t0 + blockIdx.x; tile < t1; tile += gridDim.x) {
        const uint32_t si = ws.tile_seg[tile];
        const BzxSeg s = ws.seg[si];
        const uint64_t lt = tile - s.tile0;
        TileInfo ti;
        if (ws.tile_np[tile + 1] == ws.tile_np[tile]) {
            // no run position k >= 3 in the tile: every byte is emitted once
            tile_load(s.raw, s.len, lt, ti.t);
            ti.e_bits = 0x5555555555555555ull;
            ti.f_excl = threadIdx.x * RL_BYTES;
        } else {
            tile_analyse(s.raw, s.len, lt, bt_carry(ws, s, tile), s64, s32, ti);
        }
        if (ti.t.nvalid) {
            const uint64_t *braw = ws.blk_raw + s.slot0, *bf = ws.blk_f + s.slot0;
            const uint32_t nb = ws.seg_nblk[si], b0 = ws.seg_blk[si] - rb0;
            // block of my first byte: last block of the input with braw <= p0
            uint32_t lo = 0, hi = nb;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (braw[mid] <= ti.t.p0) lo = mid; else hi = mid;
            }
            uint32_t kb = lo;
            uint64_t next_raw = braw[kb + 1];
            uint64_t f0 = bf[kb];
            uint8_t *dst = slabs + (size_t)(b0 + kb) * BZX_BLK_STRIDE;
            uint64_t f = ws.tile_off[tile] - ws.tile_off[s.tile0] + ti.f_excl;
            for (int i = 0; i < RL_BYTES; i++) {
                if ((uint32_t)i < ti.t.nvalid) {
                    const uint64_t p = ti.t.p0 + i;
                    if (p >= next_raw) {
                        kb++;
                        next_raw = braw[kb + 1];
                        f0 = bf[kb];
                        dst = slabs + (size_t)(b0 + kb) * BZX_BLK_STRIDE;
                    }
                    const uint32_t e = (uint32_t)(ti.e_bits >> (2 * i)) & 3u;
                    if (e) {
                        const uint32_t c = tile_byte(ti.t, i);
                        dst[f - f0] = (uint8_t)c;
                        if (e == 2) {
                            // 4th byte of a piece: count the rest of the piece (<= 251 more equal bytes)
                            uint64_t q = p + 1;
                            uint32_t extra = 0;
                            while (q < s.len && extra < 251 && s.raw[q] == c) {
                                q++;
                                extra++;
                            }
                            dst[f - f0 + 1] = (uint8_t)extra;
                        }
                        f += e;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- E: CRC of every block of the round, through its input's pointer
__global__ __launch_bounds__(CRC_NT) void bzx_bt_crc_kernel(BzxBatchWs ws, uint32_t nb, uint32_t rb0,
                                                            BzxBlock *__restrict__ blk)
{
    __shared__ BzxCrcLds lds;
    const uint32_t my_weight = bzx_crc_setup(lds);
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint32_t si = ws.blk_seg[b];
        const BzxSeg s = ws.seg[si];
        const uint32_t j = s.slot0 + (b + rb0 - ws.seg_blk[si]);
        const uint32_t crc = bzx_crc_range(s.raw, ws.blk_raw[j], ws.blk_raw[j + 1], lds, my_weight);
        if (threadIdx.x == 0) blk[b].crc = crc;
    }
}

// Exclusive sum over the BT_NT lanes of the workgroup; total of all lanes in `total`.
__device__ __forceinline__ uint64_t bt_excl_sum64(uint64_t v, uint64_t *wsum, uint64_t &total)
{
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    uint64_t x = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
    for (uint32_t w = 0; w < BT_NT / 64; w++) {
        if (w < wave) pre += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    total = tot;
    return pre + x - v;
}

// ---- layout of the round's streams (inputs [i0, i1), blocks [0, nb)), the first at byte `base` of the output
__global__ __launch_bounds__(BT_NT) void bzx_bt_layout_kernel(BzxBatchWs ws, uint32_t i0, uint32_t i1, uint32_t rb0,
                                                              uint32_t nb, BzxBlock *__restrict__ blk, uint64_t base)
{
    __shared__ uint64_t wsum[BT_NT / 64];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0, tot;
    for (uint32_t b0 = 0; b0 < nb; b0 += BT_NT) {
        const uint32_t b = b0 + tid;
        const uint64_t ex = bt_excl_sum64(b < nb ? blk[b].bits : 0, wsum, tot);
        if (b < nb) ws.pre[b] = carry + ex;
        carry += tot;
    }
    if (tid == 0) ws.pre[nb] = carry;
    __syncthreads();
    carry = base;
    for (uint32_t k0 = i0; k0 < i1; k0 += BT_NT) {
        const uint32_t i = k0 + tid;
        uint64_t len = 0;
        if (i < i1) {
            const uint32_t first = ws.seg_blk[i] - rb0;
            len = (32 + (ws.pre[first + ws.seg_nblk[i]] - ws.pre[first]) + 80 + 7) >> 3;
        }
        const uint64_t ex = bt_excl_sum64((len + 3) & ~3ull, wsum, tot);
        if (i < i1) {
            ws.s_off[i] = carry + ex;
            ws.s_len[i] = len;
        }
        carry += tot;
    }
    if (tid == 0) ws.round_end[0] = carry;
    __syncthreads();
    for (uint32_t b = tid; b < nb; b += BT_NT) {
        const uint32_t si = ws.blk_seg[b];
        blk[b].out_bit = 8 * ws.s_off[si] + 32 + ws.pre[b] - ws.pre[ws.seg_blk[si] - rb0];
    }
}

// ---- index entries of the round's blocks [0, nb) (bzx_ctx_keep_index), after the layout: one lane per block builds the
// 40-byte entry in registers -- bit and out_off count from the start of the block's own stream and input -- and the
// workgroup's 256 entries, contiguous in ws.idx, leave through LDS as whole 16-byte vectors, lane after lane.
__global__ __launch_bounds__(BX_NT) void bzx_bt_index_kernel(BzxBatchWs ws, uint32_t rb0, uint32_t nb,
                                                             const BzxBlock *__restrict__ blk, uint32_t level)
{
    __shared__ __attribute__((aligned(16))) uint64_t s_w[BX_NT * BX_WORDS];
    const uint32_t tid = threadIdx.x, b0 = blockIdx.x * BX_NT, b = b0 + tid;
    if (b < nb) {
        const uint32_t si = ws.blk_seg[b], first = ws.seg_blk[si] - rb0;
        const uint64_t *braw = ws.blk_raw + ws.seg[si].slot0 + (b - first);
        const uint64_t off = braw[0];
        uint64_t *w = s_w + tid * BX_WORDS;
        w[0] = 32 + ws.pre[b] - ws.pre[first];                                       // bit
        w[1] = off;                                                                  // out_off
        w[2] = (uint64_t)(uint32_t)(braw[1] - off) | ((uint64_t)blk[b].crc << 32);   // out_len, crc
        w[3] = (uint64_t)(uint32_t)blk[b].bits;                                      // img_bits, stream = 0
        w[4] = (uint64_t)(level & 0xffu);                                            // level, reserved = 0
    }
    __syncthreads();
    const uint32_t cnt = nb - b0 < BX_NT ? nb - b0 : BX_NT, nw = cnt * BX_WORDS;     // words this workgroup owns
    uint64_t *dst = ws.idx + (size_t)b0 * BX_WORDS;                                  // (16-byte aligned: b0 * 40 is)
    for (uint32_t v = tid; v < nw / 2; v += BX_NT)
        reinterpret_cast<uint4 *>(dst)[v] = reinterpret_cast<const uint4 *>(s_w)[v];
    if ((nw & 1u) && tid == 0) dst[nw - 1] = s_w[nw - 1];
}

// OR the low nbits (1..32) of val into the big-endian bit buffer at bit pos (nothing else writes these words now)
__device__ __forceinline__ void bt_or_bits(uint32_t *out, uint64_t pos, uint32_t nbits, uint32_t val)
{
    const uint32_t sh = (uint32_t)(pos & 31u);
    const uint64_t v = (uint64_t)val << (64 - nbits - sh);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (hi) out[pos >> 5] |= __builtin_bswap32(hi);
    if (lo) out[(pos >> 5) + 1] |= __builtin_bswap32(lo);
}

// ---- framing of the round's streams, one wave per stream; after the emit kernel
__global__ __launch_bounds__(256) void bzx_bt_frame_kernel(BzxBatchWs ws, uint32_t i0, uint32_t i1, uint32_t rb0,
                                                           const BzxBlock *__restrict__ blk, uint32_t *out, int level)
{
    const uint32_t i = i0 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= i1) return;
    // combined CRC (crc.rs:25-27): c = rotl(c, 1) ^ crc_b over the stream's blocks, i.e. XOR_j rotl(crc_j, (n-1-j) mod 32)
    const uint32_t n = ws.seg_nblk[i], b0 = ws.seg_blk[i] - rb0;
    uint32_t x = 0;
    for (uint32_t j = lane; j < n; j += 64) {
        const uint32_t c = blk[b0 + j].crc, r = (n - 1u - j) & 31u;
        x ^= r ? ((c << r) | (c >> (32u - r))) : c;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x ^= __shfl_xor(x, d);
    if (lane == 0) {
        const uint64_t off = ws.s_off[i];
        const uint64_t end = 8 * off + 32 + (ws.pre[b0 + n] - ws.pre[b0]);
        out[off >> 2] = __builtin_bswap32(0x425A6830u + (uint32_t)level);        // "BZh<level>"
        bt_or_bits(out, end, 24, 0x177245u);
        bt_or_bits(out, end + 24, 24, 0x385090u);
        bt_or_bits(out, end + 48, 32, x);
    }
}

// ---- host side (on the context's stream)
static uint32_t bt_grid(uint64_t items, uint32_t ncu, uint32_t per_cu)
{
    const uint64_t g = (uint64_t)ncu * per_cu;
    return (uint32_t)(items < g ? (items ? items : 1) : g);
}

// Kernels A, B, C over every input of the call; writes ws.seg_nblk.
static void bzx_batch_launch_split(const BzxBatchWs &ws, int level, uint32_t ncu, hipStream_t st)
{
    const uint32_t grid = bt_grid(ws.ntiles, ncu, 8);
    hipLaunchKernelGGL(bzx_bt_runstart_kernel, dim3(grid), dim3(RL_NT), 0, st, ws);
    bzx_split_scan(st, ws.tile_rs, ws.ntiles, 1, ws.segtot);
    hipLaunchKernelGGL(bzx_bt_count_kernel, dim3(bt_grid((ws.ntiles + RL_NT - 1) / RL_NT, ncu, 8)), dim3(RL_NT), 0, st, ws);
    bzx_split_scan(st, ws.tile_off, ws.ntiles, 0, ws.segtot);
    bzx_split_scan(st, ws.tile_np, ws.ntiles, 0, ws.segtot);
    hipLaunchKernelGGL(bzx_bt_boundaries_kernel, dim3(bt_grid(ws.count, ncu, 4)), dim3(RL_NT), 0, st, ws,
                       100000u * (uint32_t)level - 19u);
}

// One round, before the stage kernels: descriptors, slabs and CRCs of blocks [0, nb) (inputs [i0, i1), tiles [t0, t1)).
static void bzx_batch_launch_round(const BzxBatchWs &ws, uint32_t i0, uint32_t i1, uint64_t t0, uint64_t t1,
                                   uint32_t rb0, uint32_t nb, uint8_t *slabs, BzxBlock *blk, uint32_t ncu, hipStream_t st)
{
    if (nb == 0) return;
    hipLaunchKernelGGL(bzx_bt_describe_kernel, dim3((i1 - i0 + 3) / 4), dim3(256), 0, st, ws, i0, i1, rb0, blk);
    hipLaunchKernelGGL(bzx_bt_scatter_kernel, dim3(bt_grid(t1 - t0, ncu, 8)), dim3(RL_NT), 0, st, ws, t0, t1, rb0, slabs);
    hipLaunchKernelGGL(bzx_bt_crc_kernel, dim3(bt_grid(nb, ncu, 1)), dim3(CRC_NT), 0, st, ws, nb, rb0, blk);
}

static void bzx_batch_launch_layout(const BzxBatchWs &ws, uint32_t i0, uint32_t i1, uint32_t rb0, uint32_t nb,
                                    BzxBlock *blk, uint64_t base, hipStream_t st)
{
    hipLaunchKernelGGL(bzx_bt_layout_kernel, dim3(1), dim3(BT_NT), 0, st, ws, i0, i1, rb0, nb, blk, base);
}

static void bzx_batch_launch_index(const BzxBatchWs &ws, uint32_t rb0, uint32_t nb, const BzxBlock *blk, int level,
                                   hipStream_t st)
{
    hipLaunchKernelGGL(bzx_bt_index_kernel, dim3((nb + BX_NT - 1) / BX_NT), dim3(BX_NT), 0, st, ws, rb0, nb, blk,
                       (uint32_t)level);
}

static void bzx_batch_launch_frame(const BzxBatchWs &ws, uint32_t i0, uint32_t i1, uint32_t rb0, const BzxBlock *blk,
                                   void *d_out, int level, hipStream_t st)
{
    hipLaunchKernelGGL(bzx_bt_frame_kernel, dim3((i1 - i0 + 3) / 4), dim3(256), 0, st, ws, i0, i1, rb0, blk,
                       (uint32_t *)d_out, level);
}

// ---- batched compression: count independent inputs -> count independent .bz2 streams (include/bzx.h)
static size_t round_up4(size_t x) { return (x + 3) & ~(size_t)3; }

extern "C" size_t bzx_compress_batch_bound(uint32_t count, const size_t *lens)
{
    size_t sum = 0;
    for (uint32_t i = 0; lens && i < count; i++) sum += round_up4(lens[i] + lens[i] / 50 + 4096);
    return sum;
}

// Carves the device tables of a batch call out of ctx->batch_ws (grown on demand).
static int batch_ws_alloc(bzx_ctx *ctx, uint32_t count, uint64_t ntiles, uint64_t nslots, uint32_t max_round, bool keep,
                          BzxBatchWs *ws)
{
    const bool ok = carved(ctx->batch_ws, 8, [&](Carver &c) {
        auto take = [&](size_t nwords) { return c.take<uint64_t>(nwords); };
        ws->idx = keep ? take((size_t)max_round * BX_WORDS + 2) : nullptr;      // (first: on the 16 bytes of the allocation)
        ws->seg = (BzxSeg *)take((size_t)count * (sizeof(BzxSeg) / 8));
        ws->tile_seg = (uint32_t *)take((ntiles + 8) / 2);
        ws->tile_rs = take(ntiles + 2);
        ws->tile_off = take(ntiles + 2);
        ws->tile_np = take(ntiles + 2);
        ws->blk_raw = take(nslots + 2);
        ws->blk_f = take(nslots + 2);
        ws->blk_plain = (uint32_t *)take((nslots + 8) / 2);
        ws->seg_nblk = (uint32_t *)take(((size_t)count + 2) / 2);
        ws->seg_blk = (uint32_t *)take(((size_t)count + 2) / 2);
        ws->blk_seg = (uint32_t *)take(((size_t)max_round + 8) / 2);
        ws->pre = take((size_t)max_round + 2);
        ws->s_off = take((size_t)count + 2);
        ws->s_len = take((size_t)count + 2);
        ws->round_end = take(2);
        ws->segtot = take(bzx_split_scan_words(ntiles));
        take(16 + 1);        // slack nobody uses: 16 words, and the one an odd count leaves between seg_nblk and seg_blk
    });
    if (!ok) {
        ctx->err = "hipMalloc(batch tables) failed";
        return BZX_E_NOMEM;
    }
    ws->ntiles = ntiles;
    ws->count = count;
    return BZX_OK;
}

// Argument checks shared by both forms; device: the inputs and the output are device pointers (alignment checked).
static int batch_args(bzx_ctx *ctx, const char *fn, uint32_t count, const void *const *raws, const size_t *lens,
                      const void *out, size_t *out_offs, size_t *out_lens, bool device)
{
    if (!raws || !lens || !out || !out_offs || !out_lens) {
        ctx->err = std::string(fn) + ": NULL array or output pointer";
        return BZX_E_PARAM;
    }
    if (device && ((uintptr_t)out & 3u)) {
        ctx->err = std::string(fn) + ": d_out must be 4-byte aligned";
        return BZX_E_PARAM;
    }
    for (uint32_t i = 0; i < count; i++) {
        if (lens[i] && !raws[i]) {
            ctx->err = std::string(fn) + ": input " + std::to_string(i) + ": NULL pointer with a non-zero length";
            return BZX_E_PARAM;
        }
        if (device && lens[i] && ((uintptr_t)raws[i] & 15u)) {
            ctx->err = std::string(fn) + ": input " + std::to_string(i) + ": d_raws[" + std::to_string(i) +
                       "] must be 16-byte aligned";
            return BZX_E_PARAM;
        }
    }
    return BZX_OK;
}

// Adds the figures of the BWT, MTF and Huffman stages of a run (collect_stage_times) to an accumulator.
static void add_stage_figures(bzx_stats &acc, const bzx_stats &run)
{
    acc.ms_bwt += run.ms_bwt;
    acc.ms_mtf += run.ms_mtf;
    acc.ms_huffman += run.ms_huffman;
    acc.ms_bwt_split += run.ms_bwt_split;
    acc.ms_bwt_sort += run.ms_bwt_sort;
    acc.ms_bwt_general += run.ms_bwt_general;
    acc.ms_bwt_rank += run.ms_bwt_rank;
    acc.bwt_launches += run.bwt_launches;
    acc.n_redo += run.n_redo;
    acc.n_buckets += run.n_buckets;
    acc.n_open_buckets += run.n_open_buckets;
    acc.n_open_left += run.n_open_left;
    acc.n_resume_left += run.n_resume_left;
    acc.n_from_scratch += run.n_from_scratch;
    acc.n_unsorted += run.n_unsorted;
}

// The batch on device buffers: split analysis of all inputs, then rounds of whole inputs (at most R blocks each).
static int batch_run(bzx_ctx *ctx, uint32_t count, const void *const *d_raws, const size_t *lens, int level, void *d_out,
                     size_t cap, size_t *out_offs, size_t *out_lens)
{
    hipStream_t st = ctx->stream;
    const bool keep = ctx->keep_index;
    const uint64_t nmax = (uint64_t)100000 * level - 19;
    std::vector<BzxSeg> seg(count);
    uint64_t ntiles = 0, nslots = 0;
    uint32_t max_bound = 0;
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t len = lens[i];
        const uint64_t bound = (len + len / 4) / nmax + 2;
        if (bound > 0x7fffffffu) return BZX_E_PARAM;
        seg[i].raw = (const uint8_t *)d_raws[i];
        seg[i].len = len;
        seg[i].tile0 = ntiles;
        seg[i].slot0 = (uint32_t)nslots;
        seg[i].nslot = (uint32_t)bound + 1;
        ntiles += (len + 8191) / 8192;
        nslots += bound + 1;
        if (nslots > 0x7fffffffu) {
            ctx->err = "bzx_compress_batch: too many inputs in one call";
            return BZX_E_PARAM;
        }
        if (bound > max_bound) max_bound = (uint32_t)bound;
    }
    const uint32_t max_round = ctx->cap_slabs > max_bound ? ctx->cap_slabs : max_bound;
    std::vector<uint32_t> tile_seg(ntiles);
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t t1 = i + 1 < count ? seg[i + 1].tile0 : ntiles;
        for (uint64_t t = seg[i].tile0; t < t1; t++) tile_seg[t] = i;
    }
    BzxBatchWs ws;
    int rc = batch_ws_alloc(ctx, count, ntiles, nslots, max_round, keep, &ws);
    if (rc) return rc;
    bzx_stats &stt = ctx->stats;
    memset(&stt, 0, sizeof(stt));
    ctx->stats_batch = true;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[5], st));
    HIP_TRY(ctx, hipMemcpyAsync(ws.seg, seg.data(), count * sizeof(BzxSeg), hipMemcpyHostToDevice, st));
    if (ntiles) HIP_TRY(ctx, hipMemcpyAsync(ws.tile_seg, tile_seg.data(), ntiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    bzx_batch_launch_split(ws, level, (uint32_t)ctx->n_cu, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[6], st));
    std::vector<uint32_t> nblk(count), first(count);
    HIP_TRY(ctx, hipMemcpyAsync(nblk.data(), ws.seg_nblk, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&stt.ms_split, ctx->ev[5], ctx->ev[6]);
    // block numbering of the call; rounds of whole inputs with at most R blocks
    uint32_t R = ctx->cap_slabs, total = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (nblk[i] >= seg[i].nslot || (lens[i] && nblk[i] == 0)) {
            ctx->err = "device block splitter produced an impossible block count (input " + std::to_string(i) + ")";
            return BZX_E_HIP;
        }
        first[i] = total;
        total += nblk[i];
        if (nblk[i] > R) R = nblk[i];
    }
    if ((rc = ensure_blocks(ctx, R))) return rc;
    if (keep) {                                 // 40 bytes per block of the call, and where each stream's entries start
        ctx->bidx.resize(total);
        ctx->bidx_first.resize((size_t)count + 1);
        for (uint32_t i = 0; i < count; i++) ctx->bidx_first[i] = first[i];
        ctx->bidx_first[count] = total;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ws.seg_blk, first.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    BzxBatch &B = ctx->B;
    B.in = ctx->d_in;
    B.raw = nullptr;                   // every block of a batch is in the slabs
    B.blk_first = 0;
    B.blk_step = 1;
    B.packed = 0;
    B.out = (uint32_t *)d_out;
    const size_t cap4 = cap & ~(size_t)3;
    uint64_t base = 0;
    bool emit_pending = false;
    std::vector<BzxBlock> hb;
    for (uint32_t i0 = 0; i0 < count;) {
        uint32_t i1 = i0, nb = 0;
        while (i1 < count && nb + nblk[i1] <= R) nb += nblk[i1++];
        const uint32_t rb0 = first[i0];
        const uint64_t t0 = seg[i0].tile0, t1 = i1 < count ? seg[i1].tile0 : ntiles;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_bt[0], st));
        bzx_batch_launch_round(ws, i0, i1, t0, t1, rb0, nb, ctx->d_in, B.blk, (uint32_t)ctx->n_cu, st);
        if (nb && (rc = run_stages(ctx, nb, STG_BWT | STG_MTF | STG_HUF))) return rc;
        bzx_batch_launch_layout(ws, i0, i1, rb0, nb, B.blk, base, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(out_offs + i0, ws.s_off + i0, (i1 - i0) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_lens + i0, ws.s_len + i0, (i1 - i0) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars, ws.round_end, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (nb) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, B.blk, nb * sizeof(BzxBlock), hipMemcpyDeviceToHost, st));
        if (keep && nb) {                                    // the round's entries, in input order behind those before
            bzx_batch_launch_index(ws, rb0, nb, B.blk, level, st);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(ctx->bidx.data() + rb0, ws.idx, (size_t)nb * sizeof(bzx_index_entry),
                                        hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));             // the round's one host synchronisation
        const uint64_t end = ctx->h_scalars[0];
        if (emit_pending) {                                  // emit time of the previous round
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ctx->ev_bt[1], ctx->ev_bt[2]);
            stt.ms_emit += ms;
            emit_pending = false;
        }
        if (nb) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ctx->ev_bt[0], ctx->ev[0]);
            const bzx_stats before = stt;
            collect_stage_times(ctx);                        // this round's figures, summed over the rounds
            add_stage_figures(stt, before);
            stt.ms_split = before.ms_split + ms;
            stt.ms_emit = before.ms_emit;
        }
        if (end > cap4) {
            ctx->err = "output buffer too small for the batch (input " + std::to_string(i0) + " onwards does not fit; "
                       "bzx_compress_batch_bound always fits)";
            return BZX_E_OUTBUF;
        }
        fold_blocks(stt, ctx->h_blk, 0, nb, 1);
        for (uint32_t i = i0; i < i1; i++) {
            stt.raw_bytes += lens[i];
            stt.out_bits += (uint64_t)out_lens[i] * 8;
        }
        stt.nblk += nb;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_bt[1], st));
        HIP_TRY(ctx, hipMemsetAsync((uint8_t *)d_out + base, 0, end - base, st));
        B.nblk = nb;
        if (nb) bzx_launch_emit(B, (uint32_t)ctx->n_cu, st);
        bzx_batch_launch_frame(ws, i0, i1, rb0, B.blk, d_out, level, st);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_bt[2], st));
        HIP_TRY(ctx, hipGetLastError());
        emit_pending = true;
        base = end;
        i0 = i1;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[7], st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (emit_pending) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ctx->ev_bt[1], ctx->ev_bt[2]);
        stt.ms_emit += ms;
    }
    (void)hipEventElapsedTime(&stt.ms_total, ctx->ev[5], ctx->ev[7]);
    ctx->bidx_ok = keep;
    return BZX_OK;
}

// count == 0: nothing is written; a kept index has no entry and first[] = {0}.
static int batch_empty(bzx_ctx *ctx)
{
    if (!ctx->keep_index) return BZX_OK;
    try {
        ctx->bidx.clear();
        ctx->bidx_first.assign(1, 0);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
    ctx->bidx_ok = true;
    return BZX_OK;
}

extern "C" int bzx_compress_batch_get_index(const bzx_ctx *ctx, const bzx_index_entry **entries, const uint64_t **first,
                                            uint32_t *count)
{
    if (!ctx || !entries || !first || !count) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(const_cast<bzx_ctx *>(ctx)->api_mu);
    if (!ctx->keep_index || !ctx->bidx_ok) return BZX_E_STATE;
    *entries = ctx->bidx.data();
    *first = ctx->bidx_first.data();
    *count = (uint32_t)(ctx->bidx_first.size() - 1);
    return BZX_OK;
}

extern "C" int bzx_compress_batch_device(bzx_ctx *ctx, uint32_t count, const void *const *d_raws, const size_t *lens,
                                         int level, void *d_out, size_t cap, size_t *out_offs, size_t *out_lens)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx) return BZX_E_PARAM;
    ctx->bidx_ok = false;
    if (!level_ok(level)) {
        ctx->err = "bzx_compress_batch_device: level must be 1..9";
        return BZX_E_PARAM;
    }
    if (count == 0) return batch_empty(ctx);
    int rc = batch_args(ctx, "bzx_compress_batch_device", count, d_raws, lens, d_out, out_offs, out_lens, true);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    try {
        rc = batch_run(ctx, count, d_raws, lens, level, d_out, cap, out_offs, out_lens);
    } catch (const std::bad_alloc &) {             // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (rc) (void)hipStreamSynchronize(ctx->stream);     // nothing of a failed call is left in flight
    return rc;
}

static int batch_buffer(bzx_ctx *ctx, uint32_t count, const uint8_t *const *raws, const size_t *lens, int level,
                        uint8_t *out, size_t cap, size_t *out_offs, size_t *out_lens);

// Host buffers: the inputs are staged to the device (each on a 16-byte boundary of one allocation), the streams come
// back in one copy.  Both device buffers live for the call only.
extern "C" int bzx_compress_batch_buffer(bzx_ctx *ctx, uint32_t count, const uint8_t *const *raws, const size_t *lens,
                                         int level, uint8_t *out, size_t cap, size_t *out_offs, size_t *out_lens)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx) return BZX_E_PARAM;
    ctx->bidx_ok = false;
    if (!level_ok(level)) {
        ctx->err = "bzx_compress_batch_buffer: level must be 1..9";
        return BZX_E_PARAM;
    }
    if (count == 0) return batch_empty(ctx);
    int rc = batch_args(ctx, "bzx_compress_batch_buffer", count, (const void *const *)raws, lens, out, out_offs, out_lens,
                        false);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    try {
        return batch_buffer(ctx, count, raws, lens, level, out, cap, out_offs, out_lens);
    } catch (const std::bad_alloc &) {             // (nothing may unwind across the C ABI)
        (void)hipStreamSynchronize(ctx->stream);
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
}

static int batch_buffer(bzx_ctx *ctx, uint32_t count, const uint8_t *const *raws, const size_t *lens, int level,
                        uint8_t *out, size_t cap, size_t *out_offs, size_t *out_lens)
{
    int rc = BZX_OK;
    std::vector<size_t> at(count);
    size_t staged = 0;
    for (uint32_t i = 0; i < count; i++) {
        at[i] = staged;
        staged += (lens[i] + 15) & ~(size_t)15;
    }
    std::vector<const void *> d_raws(count, nullptr);
    const size_t bound = bzx_compress_batch_bound(count, lens);
    const size_t dcap = (cap < bound ? cap : bound) & ~(size_t)3;
    DevMem<> d_in, d_out;                    // (freed on return, behind the synchronisation below)
    if (!d_in.reserve(staged ? staged : 16)) {
        ctx->err = "hipMalloc(batch inputs) failed";
        return BZX_E_NOMEM;
    }
    if (!d_out.reserve(dcap ? dcap : 4)) {
        ctx->err = "hipMalloc(batch output) failed";
        return BZX_E_NOMEM;
    }
    for (uint32_t i = 0; !rc && i < count; i++) {
        if (!lens[i]) continue;
        d_raws[i] = d_in + at[i];
        if (hipMemcpyAsync(d_in + at[i], raws[i], lens[i], hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            ctx->err = "hipMemcpyAsync(batch input) failed";
            rc = BZX_E_HIP;
        }
    }
    try {
        if (!rc) rc = batch_run(ctx, count, d_raws.data(), lens, level, d_out, dcap, out_offs, out_lens);
    } catch (const std::bad_alloc &) {             // (caught here: the buffers must outlive what is in flight)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    if (!rc) {
        const size_t end = out_offs[count - 1] + round_up4(out_lens[count - 1]);
        if (hipMemcpyAsync(out, d_out, end, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
            ctx->err = "hipMemcpyAsync(batch output) failed";
            rc = BZX_E_HIP;
            ctx->bidx_ok = false;
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}
