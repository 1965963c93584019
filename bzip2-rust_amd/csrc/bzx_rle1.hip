// bzx_rle1.hip -- RLE1, block splitting and block CRCs of a whole raw buffer on gfx950.
//
// Contract (reference src/tools/rle1.rs:33-263 RLE1Block + src/tools/crc.rs:15-22 do_crc):
// raw stream -> blocks of RLE1'd bytes (runs of 4..255 equal bytes -> 4 bytes + count) of at
// most 100000*level-19(+4+5) bytes, each with the CRC-32/BZIP2 of the raw bytes it covers.
// The split rule is libbz2's: the raw stream is cut into PIECES (maximal runs,
// cut every 255 bytes); a block is a whole number of pieces and ends with the first piece that
// brings its RLE1 length to >= nblockMAX; the pending run moves to the next block whole.
//
// The reference does this byte-serially under a lock (compress.rs:125-128).  Here:
//   A  per 8 KiB tile: last run start                      -> scan S1 (tile run-start carry-in)
//   B  per tile: RLE1 bytes emitted by the tile            -> scan S2 (tile RLE1 offsets F)
//      position p with k = (p - runstart(p)) mod 255 emits  k<3: 1 byte, k==3: 2 bytes (the 4th
//      copy + the count), k>3: nothing -- purely local once the run start is known.
//   C  block boundaries: a short serial chain over blocks (one workgroup): smallest position x
//      with F(x) >= F(start)+nblockMAX by search over the tile offsets and one tile scan, then
//      the end of the piece containing x.
//   D  per tile: scatter the emitted bytes into the block slabs (count byte = piece length - 4
//      by a <= 251 byte look-ahead)
//   E  per block: CRC of its raw range: per-lane table CRC of a chunk from a zero register,
//      combined with x^(8*len) mod P multiplications (GF(2) polynomial arithmetic).
#include <hip/hip_runtime.h>
#include <string.h>
#include "bzx_host.h"
#include "bzx_rle1.h"

// ---- A: last run start per tile (bzx_tile_runstart in bzx_rle1.h)
__global__ __launch_bounds__(RL_NT) void bzx_rl_runstart_kernel(const uint8_t *__restrict__ raw, uint64_t len,
                                                                uint64_t t_lo, uint64_t ntiles, BzxSplitWs ws)
{
    // tiles [t_lo, ntiles): all of them, or one rank's share of a sharded analysis (bzx_shard_scan_runs)
    __shared__ uint64_t scratch[RL_NT / 64];
    for (uint64_t tile = t_lo + blockIdx.x; tile < ntiles; tile += gridDim.x) {
        bool any4;
        const uint64_t tot = bzx_tile_runstart(raw, len, tile, scratch, any4);
        if (threadIdx.x == 0) {
            ws.tile_rs[tile] = tot;
            ws.tile_np[tile] = any4 ? 1 : 0;     // provisional: 0 = plain for sure, B skips the tile
            ws.tile_off[tile] = RL_TILE;
        }
    }
}

// ---- S1 / S2: single-workgroup exclusive scans over the tile summaries
__global__ __launch_bounds__(1024) void bzx_rl_scan_kernel(uint64_t *v_all, uint64_t n_all, int is_max, uint64_t seg,
                                                           uint64_t *tot_out)
{
    // Workgroup g: v_all[g seg .. min(n_all, (g+1) seg)) -> exclusive scan in place; tot_out[g] = its total.
    // (One workgroup with seg >= n_all and tot_out = v_all + n_all scans a whole array.)  8 consecutive elements
    // per lane, the next iteration's elements already in flight; one barrier per iteration (wave totals
    // double-buffered, every lane keeps the running carry itself).
    const uint64_t lo_ = (uint64_t)blockIdx.x * seg;
    if (lo_ >= n_all && blockIdx.x) return;
    uint64_t *v = v_all + lo_;
    const uint64_t n = lo_ >= n_all ? 0 : (n_all - lo_ < seg ? n_all - lo_ : seg);
    __shared__ uint64_t wsum[2][16];
    const uint32_t tid = threadIdx.x, lane = bzx_lane(), wave = bzx_wave();
    constexpr int E = 8;
    uint64_t carry = 0;
    uint64_t nx[E];
#pragma unroll
    for (int j = 0; j < E; j++) nx[j] = (uint64_t)tid * E + j < n ? v[(uint64_t)tid * E + j] : 0ull;
    int buf = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 1024 * E, buf ^= 1) {
        const uint64_t ib = i0 + (uint64_t)tid * E;
        uint64_t a[E];
#pragma unroll
        for (int j = 0; j < E; j++) {
            a[j] = nx[j];
            const uint64_t in = ib + 1024 * E + j;
            nx[j] = in < n ? v[in] : 0ull;
        }
        uint64_t mine = 0;                 // combination of my E elements
#pragma unroll
        for (int j = 0; j < E; j++) mine = is_max ? (a[j] > mine ? a[j] : mine) : mine + a[j];
        uint64_t x = mine;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d);
            if (lane >= d) x = is_max ? (y > x ? y : x) : x + y;
        }
        uint64_t ex = __shfl_up(x, 1);
        if (lane == 0) ex = 0;
        if (lane == 63) wsum[buf][wave] = x;
        __syncthreads();
        uint64_t pre = 0, tot = 0;
        for (uint32_t w = 0; w < 16; w++) {
            const uint64_t s = wsum[buf][w];
            if (is_max) {
                if (w < wave && s > pre) pre = s;
                if (s > tot) tot = s;
            } else {
                if (w < wave) pre += s;
                tot += s;
            }
        }
        uint64_t r;
        if (is_max) {
            r = ex > pre ? ex : pre;
            if (carry > r) r = carry;
        } else {
            r = carry + pre + ex;
        }
#pragma unroll
        for (int j = 0; j < E; j++) {
            if (ib + j < n) v[ib + j] = r;
            r = is_max ? (a[j] > r ? a[j] : r) : r + a[j];
        }
        carry = is_max ? (tot > carry ? tot : carry) : carry + tot;
    }
    if (tid == 0) tot_out[blockIdx.x] = carry;
}

// second level of a segmented scan: element i of segment g gets the scanned segment total off[g] combined in
__global__ __launch_bounds__(1024) void bzx_rl_scan_add_kernel(uint64_t *v, uint64_t n, int is_max, uint64_t seg,
                                                               const uint64_t *off, uint64_t nseg)
{
    const uint64_t o = off[blockIdx.x];
    const uint64_t lo = (uint64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 1024) {
        const uint64_t x = v[i];
        v[i] = is_max ? (x > o ? x : o) : x + o;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) v[n] = off[nseg];
}

#ifndef SCAN_SEG
#define SCAN_SEG 8192        // the emulator build uses a tiny segment so that small inputs take the two-level path
#endif
// v[0..n) -> exclusive scan in place, v[n] = total.  segtot: scratch of n / SCAN_SEG + 2 words.
static void launch_scan(hipStream_t st, uint64_t *v, uint64_t n, int is_max, uint64_t *segtot)
{
    if (n <= 2 * SCAN_SEG) {
        hipLaunchKernelGGL(bzx_rl_scan_kernel, dim3(1), dim3(1024), 0, st, v, n, is_max, n ? n : 1, v + n);
        return;
    }
    const uint64_t nseg = (n + SCAN_SEG - 1) / SCAN_SEG;
    hipLaunchKernelGGL(bzx_rl_scan_kernel, dim3((uint32_t)nseg), dim3(1024), 0, st, v, n, is_max, (uint64_t)SCAN_SEG, segtot);
    hipLaunchKernelGGL(bzx_rl_scan_kernel, dim3(1), dim3(1024), 0, st, segtot, nseg, is_max, nseg, segtot + nseg);
    hipLaunchKernelGGL(bzx_rl_scan_add_kernel, dim3((uint32_t)nseg), dim3(1024), 0, st, v, n, is_max, (uint64_t)SCAN_SEG,
                       segtot, nseg);
}

// ---- B: emitted bytes per tile
__global__ __launch_bounds__(RL_NT) void bzx_rl_count_kernel(const uint8_t *__restrict__ raw, uint64_t len,
                                                             uint64_t t_lo, uint64_t ntiles, BzxSplitWs ws)
{
    __shared__ uint64_t s64[RL_NT / 64];
    __shared__ uint32_t s32[RL_NT / 64];
    // kernel A flagged the tiles that may hold a run position k >= 3; only those are analysed here.  A workgroup
    // takes 256 tiles at a time (one flag per lane, coalesced) and walks the flagged ones.
    __shared__ uint32_t s_list[RL_NT];
    __shared__ uint32_t s_cnt;
    for (uint64_t base = t_lo + (uint64_t)blockIdx.x * RL_NT; base < ntiles; base += (uint64_t)gridDim.x * RL_NT) {
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        {
            const uint64_t tile = base + threadIdx.x;
            if (tile < ntiles && !(tile > 0 && (tile + 1) * RL_TILE <= len && ws.tile_np[tile] == 0))
                s_list[atomicAdd(&s_cnt, 1u)] = threadIdx.x;
        }
        __syncthreads();
        const uint32_t nlist = s_cnt;
        for (uint32_t k = 0; k < nlist; k++) {
            const uint64_t tile = base + s_list[k];
            TileInfo ti;
            tile_analyse(raw, len, tile, ws.tile_rs[tile], s64, s32, ti);
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

// ---- C: block boundaries (single workgroup, serial over blocks; bzx_split_chain in bzx_rle1.h)
__global__ __launch_bounds__(RL_NT) void bzx_rl_boundaries_kernel(const uint8_t *__restrict__ raw, uint64_t len,
                                                                  uint64_t ntiles, uint32_t nmax, BzxSplitWs ws)
{
    __shared__ BzxChainLds lds;
    BzxChainIO io;
    io.tile_rs = ws.tile_rs;
    io.tile_off = ws.tile_off;
    io.tile_np = ws.tile_np;
    io.rs_base = 0;
    io.f_base = 0;
    io.blk_raw = ws.blk_raw;
    io.blk_f = ws.blk_f;
    io.blk_plain = ws.blk_plain;
    io.max_blocks = ws.max_blocks;
    const uint32_t nb = bzx_split_chain(raw, len, ntiles, nmax, io, lds);
    if (threadIdx.x == 0) ws.nblk[0] = nb;   // 0xffffffff: more blocks than max_blocks (error marker)
}


// ---- D: scatter the emitted bytes into the block slabs + fill the block descriptors' in_off / n
// own_first/own_step: only blocks b = own_first (mod own_step) are materialised (round-robin sharding over GPUs).
__global__ __launch_bounds__(RL_NT) void bzx_rl_scatter_kernel(const uint8_t *__restrict__ raw, uint64_t len,
                                                               uint64_t ntiles, BzxSplitWs ws, uint8_t *__restrict__ slabs,
                                                               BzxBlock *__restrict__ blk, uint32_t own_first,
                                                               uint32_t own_step)
{
    __shared__ uint64_t s64[RL_NT / 64];
    __shared__ uint32_t s32[RL_NT / 64];
    const uint32_t nblk = ws.nblk[0];
    const bool all_plain = ws.tile_np[ntiles] == 0;      // no run position k >= 3 anywhere: every block is zero-copy
    for (uint64_t tile = blockIdx.x; tile < ntiles && !all_plain; tile += gridDim.x) {
        {
            // skip tiles that lie entirely in blocks of other ranks or in zero-copy blocks (uniform decision)
            const uint64_t pa = tile * RL_TILE;
            const uint64_t pb = (pa + RL_TILE < len ? pa + RL_TILE : len) - 1;
            uint32_t lo = 0, hi = nblk;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ws.blk_raw[mid] <= pa) lo = mid; else hi = mid;
            }
            const uint32_t ka = lo;
            const uint32_t kb2 = (ka + 1 < nblk && ws.blk_raw[ka + 1] <= pb) ? ka + 1 : ka;
            const bool need_a = (ka % own_step) == own_first && !ws.blk_plain[ka];
            const bool need_b = (kb2 % own_step) == own_first && !ws.blk_plain[kb2];
            if (!need_a && !need_b) continue;
        }
        TileInfo ti;
        tile_analyse(raw, len, tile, ws.tile_rs[tile], s64, s32, ti);
        if (ti.t.nvalid) {
            // block of my first byte: last block with blk_raw <= p0
            uint32_t lo = 0, hi = nblk;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ws.blk_raw[mid] <= ti.t.p0) lo = mid; else hi = mid;
            }
            uint32_t kb = lo;
            uint64_t next_raw = ws.blk_raw[kb + 1];
            uint64_t f0 = ws.blk_f[kb];
            uint8_t *dst = slabs + (size_t)(kb / own_step) * BZX_BLK_STRIDE;      // (slab of an owned block: its local index)
            uint64_t f = ws.tile_off[tile] + ti.f_excl;
            for (int i = 0; i < RL_BYTES; i++) {
                if ((uint32_t)i < ti.t.nvalid) {
                    const uint64_t p = ti.t.p0 + i;
                    if (p >= next_raw) {
                        kb++;
                        next_raw = ws.blk_raw[kb + 1];
                        f0 = ws.blk_f[kb];
                        dst = slabs + (size_t)(kb / own_step) * BZX_BLK_STRIDE;
                    }
                    const uint32_t e = (uint32_t)(ti.e_bits >> (2 * i)) & 3u;
                    if (e && ((kb % own_step) != own_first || ws.blk_plain[kb])) {
                        f += e;
                    } else if (e) {
                        const uint32_t c = tile_byte(ti.t, i);
                        dst[f - f0] = (uint8_t)c;
                        if (e == 2) {
                            // 4th byte of a piece: count the rest of the piece (<= 251 more equal bytes)
                            uint64_t q = p + 1;
                            uint32_t extra = 0;
                            while (q < len && extra < 251 && raw[q] == c) {
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
    for (uint32_t b = blockIdx.x * RL_NT + threadIdx.x; b < nblk; b += gridDim.x * RL_NT) {
        blk[b].in_off = (ws.blk_plain[b] || all_plain) ? (BZX_IN_RAW | ws.blk_raw[b]) : (uint64_t)(b / own_step) * BZX_BLK_STRIDE;
        blk[b].n = (uint32_t)(ws.blk_f[b + 1] - ws.blk_f[b]);
        blk[b].raw_len = (uint32_t)(ws.blk_raw[b + 1] - ws.blk_raw[b]);
        blk[b].status = 0;
    }
}

// ---- E: CRC-32/BZIP2 of every block's raw range, one workgroup per block (bzx_crc_range in bzx_rle1.h)
__global__ __launch_bounds__(CRC_NT) void bzx_rl_crc_kernel(const uint8_t *__restrict__ raw, BzxSplitWs ws,
                                                            BzxBlock *__restrict__ blk, uint32_t own_first,
                                                            uint32_t own_step)
{
    __shared__ BzxCrcLds lds;
    const uint32_t my_weight = bzx_crc_setup(lds);
    const uint32_t nblk = ws.nblk[0];
    for (uint32_t b = own_first + blockIdx.x * own_step; b < nblk; b += gridDim.x * own_step) {
        const uint32_t crc = bzx_crc_range(raw, ws.blk_raw[b], ws.blk_raw[b + 1], lds, my_weight);
        if (threadIdx.x == 0) blk[b].crc = crc;
    }
}


// ---- host orchestration

// Scratch of the splitter: the three tile arrays (in the context's scratch, or -- sharded analysis -- in the caller's
// array `tiles` of 3 x tile_stride words, which the ranks all-gather), the block arrays and the scans' segment totals.
static int split_ws(bzx_ctx *ctx, size_t len, uint32_t max_blocks, uint64_t *tiles, size_t tile_stride, BzxSplitWs *ws_out,
                    uint64_t **segtot_out)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE;
    const uint64_t nsegw = ntiles / SCAN_SEG + 4;                         // scratch of the two-level scans
    const size_t own_tiles = tiles ? 0 : 3 * (ntiles + 2);
    const size_t bytes = (own_tiles + 3 * ((size_t)max_blocks + 2) + nsegw + 8) * sizeof(uint64_t) + 64;
    void *p = nullptr;
    int rc = bzx_ctx_split_scratch(ctx, bytes, &p);
    if (rc) return rc;
    BzxSplitWs ws;
    uint64_t *q = (uint64_t *)p;
    if (tiles) {
        ws.tile_rs = tiles;
        ws.tile_off = tiles + tile_stride;
        ws.tile_np = tiles + 2 * tile_stride;
    } else {
        ws.tile_rs = q;
        ws.tile_off = ws.tile_rs + (ntiles + 2);
        ws.tile_np = ws.tile_off + (ntiles + 2);
        q = ws.tile_np + (ntiles + 2);
    }
    ws.blk_raw = q;
    ws.blk_f = ws.blk_raw + (max_blocks + 2);
    ws.blk_plain = (uint32_t *)(ws.blk_f + (max_blocks + 2));
    ws.nblk = (uint32_t *)((uint64_t *)ws.blk_plain + (max_blocks + 2));
    *segtot_out = (uint64_t *)ws.nblk + 8;
    ws.max_blocks = max_blocks;
    *ws_out = ws;
    return 0;
}

static uint32_t tile_grid(bzx_ctx *ctx, uint64_t ntiles)
{
    const uint64_t g = (uint64_t)ctx->n_cu * 8;
    return (uint32_t)(ntiles < g ? (ntiles ? ntiles : 1) : g);
}

// Launches A..C; writes the block count to ws.nblk (device).  max_blocks bounds the descriptor arrays.
int bzx_split_launch_boundaries(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, int level, uint32_t max_blocks,
                                BzxSplitWs *ws_out)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE;
    BzxSplitWs ws;
    uint64_t *segtot = nullptr;
    int rc = split_ws(ctx, len, max_blocks, nullptr, 0, &ws, &segtot);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint32_t grid = tile_grid(ctx, ntiles);
    const uint32_t nmax = 100000u * (uint32_t)level - 19u;
    hipLaunchKernelGGL(bzx_rl_runstart_kernel, dim3(grid), dim3(RL_NT), 0, st, d_raw, (uint64_t)len, (uint64_t)0, ntiles, ws);
    launch_scan(st, ws.tile_rs, ntiles, 1, segtot);
    hipLaunchKernelGGL(bzx_rl_count_kernel, dim3(grid), dim3(RL_NT), 0, st, d_raw, (uint64_t)len, (uint64_t)0, ntiles, ws);
    launch_scan(st, ws.tile_off, ntiles, 0, segtot);
    launch_scan(st, ws.tile_np, ntiles, 0, segtot);
    hipLaunchKernelGGL(bzx_rl_boundaries_kernel, dim3(1), dim3(RL_NT), 0, st, d_raw, (uint64_t)len, ntiles, nmax, ws);
    *ws_out = ws;
    return 0;
}

// ---- the same analysis with the per-byte scans (kernels A and B) on one rank's share of the tiles.
// Tile arrays: the caller's `tiles`, 3 arrays of `stride` = per_rank * world words; rank r owns the entries
// [r * per_rank, (r + 1) * per_rank) of each and all-gathers them between the steps (the library has no collective).
uint64_t bzx_split_tiles_per_rank(size_t len, uint32_t world)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE;
    return (ntiles + 2 + world - 1) / world;
}

// step 1: kernel A on this rank's tiles (all three arrays get their provisional entries)
int bzx_split_shard_runs(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, uint32_t rank, uint32_t world, uint64_t *tiles)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE, per = bzx_split_tiles_per_rank(len, world);
    const uint64_t lo = (uint64_t)rank * per < ntiles ? (uint64_t)rank * per : ntiles;
    const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
    BzxSplitWs ws;
    uint64_t *segtot = nullptr;
    int rc = split_ws(ctx, len, 2, tiles, per * world, &ws, &segtot);
    if (rc) return rc;
    if (hi > lo)
        hipLaunchKernelGGL(bzx_rl_runstart_kernel, dim3(tile_grid(ctx, hi - lo)), dim3(RL_NT), 0, ctx->stream, d_raw,
                           (uint64_t)len, lo, hi, ws);
    return 0;
}

// step 2 (array 0 gathered): carry-in scan over ALL tiles (every rank the same, 8 B per 8 KiB of input), kernel B on
// this rank's tiles
int bzx_split_shard_counts(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, uint32_t rank, uint32_t world, uint64_t *tiles)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE, per = bzx_split_tiles_per_rank(len, world);
    const uint64_t lo = (uint64_t)rank * per < ntiles ? (uint64_t)rank * per : ntiles;
    const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
    BzxSplitWs ws;
    uint64_t *segtot = nullptr;
    int rc = split_ws(ctx, len, 2, tiles, per * world, &ws, &segtot);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    launch_scan(st, ws.tile_rs, ntiles, 1, segtot);
    if (hi > lo)
        hipLaunchKernelGGL(bzx_rl_count_kernel, dim3(tile_grid(ctx, (hi - lo + RL_NT - 1) / RL_NT)), dim3(RL_NT), 0, st, d_raw,
                           (uint64_t)len, lo, hi, ws);
    return 0;
}

// step 3 (arrays 1 and 2 gathered): offsets and the serial chain of block boundaries, on every rank
int bzx_split_shard_boundaries(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, int level, uint32_t max_blocks, uint32_t world,
                               uint64_t *tiles, BzxSplitWs *ws_out)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE, per = bzx_split_tiles_per_rank(len, world);
    BzxSplitWs ws;
    uint64_t *segtot = nullptr;
    int rc = split_ws(ctx, len, max_blocks, tiles, per * world, &ws, &segtot);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint32_t nmax = 100000u * (uint32_t)level - 19u;
    launch_scan(st, ws.tile_off, ntiles, 0, segtot);
    launch_scan(st, ws.tile_np, ntiles, 0, segtot);
    hipLaunchKernelGGL(bzx_rl_boundaries_kernel, dim3(1), dim3(RL_NT), 0, st, d_raw, (uint64_t)len, ntiles, nmax, ws);
    *ws_out = ws;
    return 0;
}

// Launches D and E for nblk blocks (ws.nblk on the device already holds nblk).
void bzx_split_launch_scatter(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, const BzxSplitWs &ws, uint32_t nblk,
                              uint8_t *d_slabs, BzxBlock *d_blk, uint32_t own_first, uint32_t own_step)
{
    const uint64_t ntiles = (len + RL_TILE - 1) / RL_TILE;
    hipStream_t st = ctx->stream;
    const uint32_t grid = (uint32_t)(ntiles < (uint64_t)ctx->n_cu * 8 ? ntiles : (uint64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(bzx_rl_scatter_kernel, dim3(grid), dim3(RL_NT), 0, st, d_raw, (uint64_t)len, ntiles, ws, d_slabs, d_blk, own_first, own_step);
    const uint32_t mine = nblk > own_first ? (nblk - own_first + own_step - 1) / own_step : 0;
    const uint32_t cgrid = mine < (uint32_t)ctx->n_cu ? (mine ? mine : 1) : (uint32_t)ctx->n_cu;
    hipLaunchKernelGGL(bzx_rl_crc_kernel, dim3(cgrid), dim3(CRC_NT), 0, st, d_raw, ws, d_blk, own_first, own_step);
}

// CRC-32/BZIP2 of nblk consecutive byte ranges [bounds[b], bounds[b+1]) of d_raw into blk[b].crc (the decompressor
// checks its output with the compressor's kernel).  d_nblk: device word holding nblk.
void bzx_launch_block_crcs(bzx_ctx *ctx, const uint8_t *d_raw, const uint64_t *d_bounds, uint32_t *d_nblk, BzxBlock *d_blk,
                           uint32_t nblk)
{
    BzxSplitWs ws;
    memset(&ws, 0, sizeof(ws));
    ws.blk_raw = const_cast<uint64_t *>(d_bounds);
    ws.nblk = d_nblk;
    const uint32_t cgrid = nblk < (uint32_t)ctx->n_cu ? (nblk ? nblk : 1) : (uint32_t)ctx->n_cu;
    hipLaunchKernelGGL(bzx_rl_crc_kernel, dim3(cgrid), dim3(CRC_NT), 0, ctx->stream, d_raw, ws, d_blk, 0u, 1u);
}

// The tile scans for the batched splitter (bzx_batch.hip): v[0..n) -> exclusive scan in place, v[n] = total; segtot:
// bzx_split_scan_words(n) words of scratch.
void bzx_split_scan(hipStream_t st, uint64_t *v, uint64_t n, int is_max, uint64_t *segtot)
{
    launch_scan(st, v, n, is_max, segtot);
}
uint64_t bzx_split_scan_words(uint64_t n) { return n / SCAN_SEG + 4; }
