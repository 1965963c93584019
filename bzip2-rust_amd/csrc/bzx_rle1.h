// bzx_rle1.h -- device pieces of the RLE1 / block splitter shared by the one-input splitter (bzx_rle1.hip) and the
// batched one (bzx_batch.hip): tile loads and emission analysis, the chain of block boundaries of one input, and the
// CRC-32/BZIP2 of a raw byte range.  See bzx_rle1.hip for the split rule and the kernel sequence.
#pragma once
#include <hip/hip_runtime.h>
#include "bzx_device.h"
#include "bzx_wg.h"

#define RL_NT 256
#define RL_BYTES 32
#define RL_TILE (RL_NT * RL_BYTES)   // 8192

// Per-lane view of 32 consecutive raw bytes of a tile.
struct TileLane {
    uint32_t w[8];         // the bytes
    uint64_t p0;           // raw position of byte 0
    uint32_t nvalid;       // bytes inside the input
    uint32_t prev;         // byte before p0 (256 if p0 == 0)
};

__device__ __forceinline__ void tile_load(const uint8_t *__restrict__ raw, uint64_t len, uint64_t tile, TileLane &t)
{
    t.p0 = tile * RL_TILE + (uint64_t)threadIdx.x * RL_BYTES;
    t.nvalid = t.p0 >= len ? 0u : (len - t.p0 < RL_BYTES ? (uint32_t)(len - t.p0) : (uint32_t)RL_BYTES);
#pragma unroll
    for (int i = 0; i < 8; i++) t.w[i] = 0;
    if (t.nvalid == RL_BYTES) {
        const uint4 a = *reinterpret_cast<const uint4 *>(raw + t.p0);
        const uint4 b = *reinterpret_cast<const uint4 *>(raw + t.p0 + 16);
        t.w[0] = a.x; t.w[1] = a.y; t.w[2] = a.z; t.w[3] = a.w;
        t.w[4] = b.x; t.w[5] = b.y; t.w[6] = b.z; t.w[7] = b.w;
    } else {
        for (uint32_t i = 0; i < t.nvalid; i++) t.w[i >> 2] |= (uint32_t)raw[t.p0 + i] << (8 * (i & 3));
    }
    t.prev = (t.p0 == 0 || t.nvalid == 0) ? 256u : raw[t.p0 - 1];
}

__device__ __forceinline__ uint32_t tile_byte(const TileLane &t, int i) { return (t.w[i >> 2] >> (8 * (i & 3))) & 255u; }

// last run start (+1) among my bytes, 0 if none
__device__ __forceinline__ uint64_t lane_last_rs(const TileLane &t)
{
    uint64_t rs = 0;
    uint32_t prev = t.prev;
#pragma unroll
    for (int i = 0; i < RL_BYTES; i++) {
        const uint32_t c = tile_byte(t, i);
        if ((uint32_t)i < t.nvalid && c != prev) rs = t.p0 + i + 1;
        prev = c;
    }
    return rs;
}

// Block-wide exclusive max scan of 64-bit values (0 = identity).  scratch: RL_NT/64 words.
__device__ __forceinline__ uint64_t block_excl_max64(uint64_t v, uint64_t *scratch, uint64_t &total)
{
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    uint64_t x = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d);
        if (lane >= d && y > x) x = y;
    }
    uint64_t ex = __shfl_up(x, 1);
    if (lane == 0) ex = 0;
    if (lane == 63) scratch[wave] = x;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
    for (uint32_t i = 0; i < RL_NT / 64; i++) {
        const uint64_t s = scratch[i];
        if (i < wave && s > pre) pre = s;
        if (s > tot) tot = s;
    }
    __syncthreads();
    total = tot;
    return ex > pre ? ex : pre;
}

// Emission analysis of my 32 bytes: e[i] in {0,1,2} packed 2 bits each; returns my emitted byte count.
// rs_in = run start (+1) carried into the tile (0 = none, only possible at p == 0).
__device__ __forceinline__ uint32_t lane_emission(const TileLane &t, uint64_t rs_in_plus1, uint64_t &e_bits,
                                                  uint32_t &k_first, bool &any_long)
{
    any_long = false;
    // run start for my first byte: either inside earlier lanes of the tile / earlier tiles (rs_in) or my own byte
    uint32_t k = 0;
    if (t.nvalid) {
        const uint64_t rs = rs_in_plus1 ? rs_in_plus1 - 1 : 0;   // p0 == 0 has rs_in == 0 and starts a run itself
        k = (uint32_t)((t.p0 - rs) % 255u);
    }
    uint32_t prev = t.prev, cnt = 0;
    uint64_t bits = 0;
    k_first = k;
#pragma unroll
    for (int i = 0; i < RL_BYTES; i++) {
        const uint32_t c = tile_byte(t, i);
        if ((uint32_t)i < t.nvalid) {
            if (c != prev) k = 0;
            if (i == 0) k_first = k;
            const uint32_t e = k < 3 ? 1u : (k == 3 ? 2u : 0u);
            if (k >= 3) any_long = true;
            bits |= (uint64_t)e << (2 * i);
            cnt += e;
            k = (k + 1 == 255) ? 0 : k + 1;
        }
        prev = c;
    }
    e_bits = bits;
    return cnt;
}

// Shared tile analysis: every lane gets its bytes, emission bits and F (RLE1 offset, tile relative) of its first byte.
struct TileInfo {
    TileLane t;
    uint64_t e_bits;
    uint32_t k_first;
    uint32_t f_excl;     // emitted bytes of the tile before my first byte
    uint32_t f_total;    // emitted bytes of the whole tile
    bool any_long;       // my bytes contain a run position with k >= 3 (RLE1 is not the identity here)
};

// carry = run start (+1) carried into the tile (the scanned tile_rs entry, in the positions of `raw`)
__device__ __forceinline__ void tile_analyse(const uint8_t *__restrict__ raw, uint64_t len, uint64_t tile,
                                             uint64_t carry, uint64_t *scratch64, uint32_t *scratch32, TileInfo &ti)
{
    tile_load(raw, len, tile, ti.t);
    uint64_t tot;
    const uint64_t rs_prev = block_excl_max64(lane_last_rs(ti.t), scratch64, tot);
    const uint64_t rs_in = rs_prev ? rs_prev : carry;
    const uint32_t cnt = lane_emission(ti.t, rs_in, ti.e_bits, ti.k_first, ti.any_long);
    ti.f_excl = bzx_block_excl_sum<RL_NT>(cnt, scratch32, ti.f_total);
}

// end of the piece that contains position x (x < len): first piece start after x
static __device__ uint64_t piece_end(const uint8_t *__restrict__ raw, uint64_t len, uint64_t x, uint32_t k_at_x)
{
    const uint8_t c = raw[x];
    uint64_t q = x + 1;
    uint32_t k = k_at_x + 1;
    while (q < len && k < 255 && raw[q] == c) {
        q++;
        k++;
    }
    return q;
}

__device__ __forceinline__ uint32_t gf_mulmod(uint32_t a, uint32_t b)
{
    // a(x) * b(x) mod P(x), P = x^32 + 0x04C11DB7, bit 31 = x^31
    uint32_t r = 0;
    for (int i = 31; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x80000000u) ? 0x04C11DB7u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^(8*nbytes) mod P
static __device__ uint32_t gf_xpow8(uint64_t nbytes)
{
    uint32_t result = 1u;            // the polynomial "1"
    uint32_t sq = 0x100u;            // x^8
    while (nbytes) {
        if (nbytes & 1ull) result = gf_mulmod(result, sq);
        sq = gf_mulmod(sq, sq);
        nbytes >>= 1;
    }
    return result;
}

#define CRC_NT 1024
#define CRC_SUB 64                         // bytes per lane per tile
#define CRC_TILE (CRC_NT * CRC_SUB)        // 64 KiB
#define CRC_PITCH 72                       // LDS row pitch of a lane's 64 bytes (8-byte aligned, spreads banks)

// Kernel A on one tile: last run start (+1) inside the tile (0 = none), in the positions of `raw`; any4 = the tile may
// hold a run position k >= 3 (decided exactly by kernel B).  scratch: RL_NT/64 words.
__device__ __forceinline__ uint64_t bzx_tile_runstart(const uint8_t *__restrict__ raw, uint64_t len, uint64_t tile,
                                                      uint64_t *scratch, bool &any4)
{
    TileLane t;
    bool run4 = true;                   // "this tile may hold a run position k >= 3": decided exactly by kernel B
    if (tile > 0 && (tile + 1) * RL_TILE <= len) {
        // Full inner tile: one load serves the run starts and a cheap test for B: a tile in which no four
        // consecutive equal bytes end (looking 3 bytes back into the previous tile) has no run position
        // k >= 3, so RLE1 copies it.
        t.p0 = tile * RL_TILE + (uint64_t)threadIdx.x * RL_BYTES;
        t.nvalid = RL_BYTES;
        uint32_t w0;
        __builtin_memcpy(&w0, raw + t.p0 - 4, 4);
        const uint4 a = *reinterpret_cast<const uint4 *>(raw + t.p0);
        const uint4 b = *reinterpret_cast<const uint4 *>(raw + t.p0 + 16);
        t.w[0] = a.x; t.w[1] = a.y; t.w[2] = a.z; t.w[3] = a.w;
        t.w[4] = b.x; t.w[5] = b.y; t.w[6] = b.z; t.w[7] = b.w;
        t.prev = w0 >> 24;
        uint64_t m = 0;                      // bit i: byte i of the 36 (from p0 - 4) equals byte i+1
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const uint32_t cur = i ? t.w[i - 1] : w0;
            const uint32_t nxt = i < 8 ? t.w[i] : ~t.w[7];
            const uint32_t z = cur ^ ((cur >> 8) | (nxt << 24));
            const uint32_t f = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu) >> 7;   // 0x01 in exactly the zero bytes
            m |= (uint64_t)((f * 0x01020408u) >> 24 & 0xFu) << (4 * i);
        }
        m >>= 1;                             // pairs starting at byte p0-3 and later
        run4 = (m & (m >> 1) & (m >> 2)) != 0;
    } else {
        tile_load(raw, len, tile, t);
    }
    uint64_t tot;
    (void)block_excl_max64(lane_last_rs(t), scratch, tot);
    any4 = __syncthreads_or(run4);
    return tot;
}

// ---- C: the chain of block boundaries of ONE input (one workgroup, serial over its blocks)
#define BND_J 64                       // blocks per batch of the fast path
#define BND_W (4 * BND_J + 16)         // window bytes per predicted boundary (drift <= 4 per block), multiple of 16

// The input's view of the tile and block arrays.  A batch keeps many inputs in one set of arrays: the pointers start at
// the input's first tile / first block slot, and the scanned tile values are those of the whole batch, so the input's
// own values are the scanned ones minus rs_base (run starts, 0 = none stays 0) and f_base (RLE1 offsets).
struct BzxChainIO {
    const uint64_t *tile_rs, *tile_off, *tile_np;    // [ntiles + 1] after the scans
    uint64_t rs_base, f_base;
    uint64_t *blk_raw, *blk_f;                       // [max_blocks + 1] raw start / F of every block; [nblk] = len / F(len)
    uint32_t *blk_plain;                             // [max_blocks + 1]
    uint32_t max_blocks;
};

struct BzxChainLds {
    uint64_t s64[RL_NT / 64];
    uint32_t s32[RL_NT / 64];
    uint64_t x;        // candidate position
    uint32_t k;        // k at the candidate
    uint64_t next, fnext;
    // windows of raw bytes around the next BND_J predicted boundaries (see the batched fast path below)
    __attribute__((aligned(16))) uint8_t win[BND_J][BND_W];
};

__device__ __forceinline__ uint64_t chain_carry(const BzxChainIO &io, uint64_t tile)
{
    const uint64_t v = io.tile_rs[tile];
    return v > io.rs_base ? v - io.rs_base : 0;
}

// Returns the number of blocks, or 0xffffffff when they do not fit max_blocks.
__device__ __forceinline__ uint32_t bzx_split_chain(const uint8_t *__restrict__ raw, uint64_t len, uint64_t ntiles,
                                                    uint32_t nmax, const BzxChainIO &io, BzxChainLds &lds)
{
    const uint32_t tid = threadIdx.x;
    uint64_t start = 0, f_start = 0;
    uint32_t nb = 0;
    const uint64_t f_len = io.tile_off[ntiles] - io.f_base;
    while (start < len && nb < io.max_blocks) {
        // ---- batched fast path: when no tile that the next J blocks can touch has a run position k >= 3, RLE1 is
        // the identity on all of them and block j ends within 4 bytes of start + (j+1) nmax + (0..4j).  The raw
        // bytes around all J predicted boundaries are fetched in one round trip into LDS, then the serial chain
        // (every lane runs it redundantly, lane 0 stores) costs LDS latency per block instead of HBM latency.
        {
            uint32_t J = BND_J;
            const uint64_t room = len > start + BND_W + 16 ? (len - start - BND_W - 16) / nmax : 0;   // blocks that end well before len
            if (room < J + 1) J = room > 1 ? (uint32_t)room - 1 : 0;
            if (nb + J > io.max_blocks) J = io.max_blocks - nb;
            if (J >= 2) {
                const uint64_t last = start + (uint64_t)(J + 1) * nmax + 4 * J + 8;
                uint64_t t1 = last / RL_TILE + 2;
                if (t1 > ntiles) t1 = ntiles;
                if (io.tile_np[t1] != io.tile_np[start / RL_TILE]) J = 0;
            }
            if (J >= 2) {
                for (uint32_t i = tid; i < J * (BND_W / 16); i += RL_NT) {
                    const uint32_t j = i / (BND_W / 16), c = i % (BND_W / 16);
                    uint4 v;
                    __builtin_memcpy(&v, raw + start + (uint64_t)(j + 1) * nmax - 4 + 16 * c, 16);
                    *reinterpret_cast<uint4 *>(&lds.win[j][16 * c]) = v;
                }
                __syncthreads();
                const uint64_t start0 = start;
                for (uint32_t j = 0; j < J; j++) {
                    if (tid == 0) {
                        io.blk_raw[nb] = start;
                        io.blk_f[nb] = f_start;
                        io.blk_plain[nb] = 1;
                    }
                    nb++;
                    const uint64_t x = start + nmax;
                    const uint8_t *w = &lds.win[j][(uint32_t)(start - (start0 + (uint64_t)j * nmax))];   // bytes x-4 .. x+3
                    uint32_t k = 0;
                    while (k < 3 && w[3 - k] == w[4]) k++;
                    uint64_t q = x;
                    if (k) {
                        q = x + 1;
                        uint32_t kk = k + 1;
                        while (kk < 4 && q < x + 4 && w[4 + (q - x)] == w[4]) {
                            q++;
                            kk++;
                        }
                    }
                    f_start += q - start;
                    start = q;
                }
                __syncthreads();
                continue;
            }
        }
        if (tid == 0) {
            io.blk_raw[nb] = start;
            io.blk_f[nb] = f_start;
            io.blk_plain[nb] = 0;
        }
        nb++;
        const uint64_t target = f_start + nmax;
        if (f_len < target) {
            // last block: plain if no tile from here to the end has a run position k >= 3
            if (tid == 0 && io.tile_np[ntiles] == io.tile_np[start / RL_TILE]) io.blk_plain[nb - 1] = 1;
            start = len;
            f_start = f_len;
            break;
        }
        // ---- fast path: RLE1 is the identity on every tile this block can touch (no run position k >= 3),
        // so F(x) - F(start) = x - start and the boundary is the end of the piece around start + nmax.
        {
            const uint64_t x = start + nmax;
            const uint64_t t0 = start / RL_TILE;
            uint64_t t1 = x / RL_TILE + 2;
            if (t1 > ntiles) t1 = ntiles;
            if (x + 4 < len && x >= 4 && io.tile_np[t1] == io.tile_np[t0]) {
                uint8_t w[8];
                __builtin_memcpy(w, raw + x - 4, 8);        // bytes x-4 .. x+3
                // k(x) = equal bytes immediately before x (runs are <= 3 long here)
                uint32_t k = 0;
                while (k < 3 && w[3 - k] == w[4]) k++;
                uint64_t q = x;
                if (k) {
                    q = x + 1;
                    uint32_t kk = k + 1;
                    while (kk < 4 && q < x + 4 && w[4 + (q - x)] == w[4]) {
                        q++;
                        kk++;
                    }
                }
                if (tid == 0) io.blk_plain[nb - 1] = 1;
                start = q;
                f_start = f_start + (q - (x - nmax));
                continue;
            }
        }
        // largest tile with F(tile start) < target   (tile_off is non-decreasing; tile_off[0] = 0 < target)
        uint64_t lo = 0, hi = ntiles;   // invariant: tile_off[lo] < target; hi = first tile with tile_off >= target or ntiles
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (io.tile_off[mid] - io.f_base < target) lo = mid; else hi = mid;
        }
        const uint64_t tile = lo;
        TileInfo ti;
        tile_analyse(raw, len, tile, chain_carry(io, tile), lds.s64, lds.s32, ti);
        // smallest x with F(x) >= target inside this tile, or the start of the next tile
        if (tid == 0) {
            lds.x = (tile + 1) * RL_TILE < len ? (tile + 1) * RL_TILE : len;
            lds.k = 0xffffffffu;
        }
        __syncthreads();
        {
            const uint64_t f0 = io.tile_off[tile] - io.f_base + ti.f_excl;
            uint64_t f = f0;
            uint32_t k = ti.k_first;
            uint32_t prev = ti.t.prev;
            bool found = false;
            uint64_t fx = 0;
            uint32_t kx = 0;
            for (int i = 0; i < RL_BYTES; i++) {
                if ((uint32_t)i < ti.t.nvalid) {
                    const uint32_t c = tile_byte(ti.t, i);
                    if (i > 0) k = (c != prev) ? 0u : (k + 1 == 255 ? 0u : k + 1);
                    if (!found && f >= target) {
                        found = true;
                        fx = ti.t.p0 + i;
                        kx = k;
                    }
                    f += (ti.e_bits >> (2 * i)) & 3u;
                    prev = c;
                }
            }
            // lanes are ordered by position: the first lane that found one owns the minimum
            const uint64_t any = __ballot(found);
            if (any && (int)bzx_lane() == __ffsll((unsigned long long)any) - 1) {
                // lowest wave wins: atomicMin on position
                atomicMin((unsigned long long *)&lds.x, (unsigned long long)fx);
            }
            __syncthreads();
            if (found && fx == lds.x) lds.k = kx;
            __syncthreads();
        }
        if (tid == 0) {
            uint64_t x = lds.x, q;
            if (x >= len) {
                q = len;
            } else if (lds.k == 0xffffffffu) {
                // x is the first byte of the next tile: its k is not known here; derive it from its run start
                uint64_t rs1 = chain_carry(io, tile + 1);        // run start (+1) carried into that tile
                const bool newrun = raw[x] != raw[x - 1];
                uint32_t k = newrun ? 0u : (uint32_t)((x - (rs1 ? rs1 - 1 : 0)) % 255u);
                q = (k == 0) ? x : piece_end(raw, len, x, k);
            } else {
                q = (lds.k == 0) ? x : piece_end(raw, len, x, lds.k);
            }
            lds.next = q;
        }
        __syncthreads();
        const uint64_t q = lds.next;
        // F(q): emitted bytes before q
        if (q >= len) {
            if (tid == 0) lds.fnext = f_len;
        } else {
            const uint64_t qt = q / RL_TILE;
            TileInfo tq;
            tile_analyse(raw, len, qt, chain_carry(io, qt), lds.s64, lds.s32, tq);
            uint64_t f = io.tile_off[qt] - io.f_base + tq.f_excl;
            for (int i = 0; i < RL_BYTES; i++) {
                if (tq.t.p0 + i == q) lds.fnext = f;
                f += (tq.e_bits >> (2 * i)) & 3u;
            }
        }
        __syncthreads();
        start = q;
        f_start = lds.fnext;
        __syncthreads();
    }
    if (tid == 0) {
        io.blk_raw[nb] = len;
        io.blk_f[nb] = f_len;
    }
    return (start < len) ? 0xffffffffu : nb;
}

// ---- E: CRC-32/BZIP2 of a raw byte range, one workgroup of CRC_NT lanes.  The range is walked in 64 KiB tiles that
// END at its end (the first tile is padded with virtual leading zero bytes, which do not change a zero-initialised CRC
// register): coalesced 16-byte loads -> LDS -> every lane runs slicing-by-8 over its own 64 contiguous bytes.  A lane
// keeps one running register across tiles (Horner step: R = R * x^(8*65536) + r, the multiplication by table), so the
// GF(2) combination of the 1024 lanes happens once per range: D = sum_t R_t * x^(8*64*(1023-t)), and
// crc = ~(0xffffffff * x^(8*total) + D).
struct BzxCrcLds {
    uint32_t tab[8][256];       // slicing-by-8: register after byte v followed by k zero bytes
    uint32_t tabx[4][256];      // (v << 8k) * x^(8*65536) mod P
    __attribute__((aligned(16))) uint8_t buf[CRC_NT * CRC_PITCH];
    uint32_t red[CRC_NT / 64];
};

// Fills the tables; returns this lane's weight x^(8*64*(1023-t)).  Ends with a barrier.
__device__ __forceinline__ uint32_t bzx_crc_setup(BzxCrcLds &l)
{
    const uint32_t tid = threadIdx.x;
    if (tid < 256) {
        uint32_t c = tid << 24;
        for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
        l.tab[0][tid] = c;
    }
    __syncthreads();
    for (int k = 1; k < 8; k++) {
        if (tid < 256) {
            const uint32_t p = l.tab[k - 1][tid];
            l.tab[k][tid] = (p << 8) ^ l.tab[0][p >> 24];
        }
        __syncthreads();
    }
    {
        const uint32_t xt = gf_xpow8(CRC_TILE);
        l.tabx[tid >> 8][tid & 255u] = gf_mulmod((tid & 255u) << (8 * (tid >> 8)), xt);
    }
    const uint32_t my_weight = gf_xpow8((uint64_t)CRC_SUB * (CRC_NT - 1 - tid));
    __syncthreads();
    return my_weight;
}

// CRC of raw[lo, hi); the result is valid in thread 0.
__device__ __forceinline__ uint32_t bzx_crc_range(const uint8_t *__restrict__ raw, uint64_t lo, uint64_t hi, BzxCrcLds &l,
                                                  uint32_t my_weight)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t total = hi - lo;
    const uint64_t ntile = (total + CRC_TILE - 1) / CRC_TILE;
    uint32_t R = 0;
    // piece e of lane t in a tile = bytes [(e*1024 + t)*16, +16) of the tile; tile k starts at hi - (ntile-k)*64K
    uint4 nx[4];
    auto load_piece = [&](int64_t p) -> uint4 {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p >= (int64_t)lo) {
            __builtin_memcpy(&v, raw + p, 16);
        } else if (p + 16 > (int64_t)lo) {
            uint8_t tmp[16];
            for (int j = 0; j < 16; j++) tmp[j] = (p + j >= (int64_t)lo) ? raw[p + j] : (uint8_t)0;
            __builtin_memcpy(&v, tmp, 16);
        }
        return v;
    };
    int64_t t0 = (int64_t)hi - (int64_t)(ntile * CRC_TILE);
#pragma unroll
    for (int e = 0; e < 4; e++) nx[e] = ntile ? load_piece(t0 + (int64_t)(e * CRC_NT + tid) * 16) : make_uint4(0, 0, 0, 0);
    for (uint64_t k = 0; k < ntile; k++) {
        uint4 cur[4];
#pragma unroll
        for (int e = 0; e < 4; e++) cur[e] = nx[e];
        t0 += CRC_TILE;
        if (k + 1 < ntile) {
#pragma unroll
            for (int e = 0; e < 4; e++) nx[e] = load_piece(t0 + (int64_t)(e * CRC_NT + tid) * 16);
        }
        __syncthreads();                       // previous tile fully consumed
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t o = (uint32_t)(e * CRC_NT + tid) * 16;              // byte offset inside the tile
            uint64_t *dst = reinterpret_cast<uint64_t *>(l.buf + (o / CRC_SUB) * CRC_PITCH + (o % CRC_SUB));
            dst[0] = (uint64_t)cur[e].x | ((uint64_t)cur[e].y << 32);
            dst[1] = (uint64_t)cur[e].z | ((uint64_t)cur[e].w << 32);
        }
        __syncthreads();
        const uint64_t *src = reinterpret_cast<const uint64_t *>(l.buf + tid * CRC_PITCH);
        uint32_t r = 0;
#pragma unroll
        for (int q = 0; q < CRC_SUB / 8; q++) {
            const uint64_t w = src[q];
            const uint32_t w0 = __builtin_bswap32((uint32_t)w) ^ r, w1 = __builtin_bswap32((uint32_t)(w >> 32));
            r = l.tab[7][w0 >> 24] ^ l.tab[6][(w0 >> 16) & 255u] ^ l.tab[5][(w0 >> 8) & 255u] ^ l.tab[4][w0 & 255u] ^
                l.tab[3][w1 >> 24] ^ l.tab[2][(w1 >> 16) & 255u] ^ l.tab[1][(w1 >> 8) & 255u] ^ l.tab[0][w1 & 255u];
        }
        R = l.tabx[3][R >> 24] ^ l.tabx[2][(R >> 16) & 255u] ^ l.tabx[1][(R >> 8) & 255u] ^ l.tabx[0][R & 255u] ^ r;
    }
    // D = xor over lanes of R_t * weight_t
    uint32_t d = gf_mulmod(R, my_weight);
#pragma unroll
    for (int s2 = 32; s2 > 0; s2 >>= 1) d ^= __shfl_xor(d, s2);
    __syncthreads();
    if (lane == 0) l.red[wave] = d;
    __syncthreads();
    uint32_t crc = 0;
    if (tid == 0) {
        uint32_t D = 0;
        for (uint32_t i = 0; i < CRC_NT / 64; i++) D ^= l.red[i];
        crc = ~(gf_mulmod(0xffffffffu, gf_xpow8(total)) ^ D);
    }
    return crc;
}
