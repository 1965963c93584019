// bzx_emit.hip -- bit emission of a block image, stream layout and stream framing on gfx950.
//
// Contract: the bits huf_encode writes after table optimisation (reference
// src/huffman_coding/huffman.rs:209-466) behind the block header compress_block writes
// (src/compression/compress_block.rs:34-48), MSB first like BitPacker
// (src/bitstream/bitpacker.rs:43-84); then what BitWriter does on the host in the reference
// (src/bitstream/bitwriter.rs:67-132): blocks appended bit-granularly, "BZh<level>" in front,
// footer magic + combined CRC (src/tools/crc.rs:25-27) behind.
//
// Every variable-length item gets its bit offset from an exclusive scan of item sizes, so all
// items are written independently: one lane per 50-symbol group for the payload, one lane per
// selector chunk, one lane per coding table.  A lane packs its bits in a 64-bit register into
// whole 32-bit words; only the first and last word of a lane's range can be shared with a
// neighbour and are merged with atomicOr into zeroed memory.  Selectors and tables go straight
// to the output.  The payload is cut into tiles of BZX_EMIT_TILE groups whose start offsets the
// Huffman stage leaves (BzxBatch.tbits), so a block's tiles are work items of their own: a
// tile is packed in LDS and leaves as consecutive words from consecutive lanes.  Because a
// block's out_bit is its final position in the stream (scan over block sizes,
// bzx_layout_kernel), no host-side or second-pass bit shifting is needed: the .bz2 is complete
// in HBM.
#include <hip/hip_runtime.h>
#include "bzx_host.h"
#include "bzx_wg.h"

#define EMIT_NT 512
#define EMIT_NW (EMIT_NT / 64)

#ifndef EMIT_TPI
// Tiles per work item.  Measured on the 1,194-block batch: 1 and 2 are slower, 4, 8 and 36 (the
// whole block) the same within the spread; 4 is the smallest of those, so that a lone block spreads the widest.
#define EMIT_TPI 4
#endif
#define EMIT_SLOTS ((BZX_MAX_TILES + EMIT_TPI - 1) / EMIT_TPI)      // item slots per block (a small block leaves most empty)
static_assert(EMIT_NT == BZX_EMIT_TILE, "one lane per group of a tile");
// The staging area takes the largest tile there is (every group fifty 17-bit codes) at any bit phase and any alignment
// of its first output word: no tile goes another way.
#define EMIT_STAGE_BITS (EMIT_NT * BZX_G_SIZE * 17u)
#define EMIT_STAGE_WORDS ((EMIT_STAGE_BITS / 32u + 2u + 3u + 3u) & ~3u)

// MSB-first bit writer of one lane over a zeroed word array.  GLOBAL: the output buffer, words big-endian; otherwise the
// LDS staging area, words in register order (swapped when the tile is copied out).
template <bool GLOBAL> struct BitWT {
    uint32_t *out;
    uint64_t wi;      // next 32-bit word index
    uint64_t acc;
    uint32_t nacc;    // bits held in acc (< 32 between calls)
    bool first;
    __device__ __forceinline__ void init(uint32_t *o, uint64_t bitpos)
    {
        out = o;
        wi = bitpos >> 5;
        nacc = (uint32_t)(bitpos & 31u);   // leading bits belong to the predecessor: zeros here, OR-merged
        acc = 0;
        first = true;
    }
    __device__ __forceinline__ void flush_word(uint32_t w)
    {
        const uint32_t be = GLOBAL ? __builtin_bswap32(w) : w;
        if (first) {
            if (be) atomicOr(&out[wi], be);
            first = false;
        } else {
            out[wi] = be;
        }
        wi++;
    }
    __device__ __forceinline__ void put(uint32_t nbits, uint32_t val)
    {
        if (nbits == 0) return;
        acc = (acc << nbits) | (uint64_t)val;
        nacc += nbits;
        if (nacc >= 32) {
            nacc -= 32;
            flush_word((uint32_t)(acc >> nacc));
            acc &= (1ull << nacc) - 1ull;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (nacc > 0) {
            const uint32_t w = (uint32_t)(acc << (32 - nacc));
            const uint32_t be = GLOBAL ? __builtin_bswap32(w) : w;
            if (be) atomicOr(&out[wi], be);
        }
    }
};
typedef BitWT<true> BitW;

__shared__ uint8_t e_len[6][BZX_MAX_ALPHA + 2];
__shared__ uint32_t e_cl[6][BZX_MAX_ALPHA + 2];     // code | length << 24: one lookup per payload symbol
// one tile of payload bits, packed by the lanes at tile-relative bit offsets and copied out by the whole workgroup;
// all zero between tiles (the copy clears what it reads)
__shared__ __attribute__((aligned(16))) uint32_t e_stage[EMIT_STAGE_WORDS];
__shared__ uint32_t e_tabbits[8];
__shared__ uint32_t e_scratch[2 * EMIT_NW];
__shared__ uint32_t e_bcast[4];

#define EMIT_STAMP(slot)                                                      \
    do {                                                                      \
        if (B.dbg && tid == 0) {                                              \
            const unsigned long long now_ = wall_clock64();                   \
            atomicAdd(&B.dbg[slot], now_ - t_last);                           \
            t_last = now_;                                                    \
        }                                                                     \
    } while (0)

// What a lane needs of tile t: its group's fifty symbols (two per word; the slab is longer than any block's symbols, so
// a short last group reads past n_mtf -- such symbols are never coded), the group's size and table, and the tile's
// place in the payload.  All of it is in flight together; nothing here waits.
__device__ __forceinline__ void emit_load_tile(const uint16_t *__restrict__ V, const uint16_t *__restrict__ GB,
                                               const uint8_t *__restrict__ SEL, const uint32_t *__restrict__ TB, uint32_t t,
                                               uint32_t n_sel, uint32_t (&vw)[BZX_G_SIZE / 2], uint32_t &gb, uint32_t &sel,
                                               uint32_t &tb)
{
    const uint32_t g = t * EMIT_NT + threadIdx.x;
    tb = TB[t];
    gb = 0;
    sel = 0;
#pragma unroll
    for (uint32_t k = 0; k < BZX_G_SIZE / 2; k++) vw[k] = 0;
    if (g < n_sel) {
        const uint32_t *__restrict__ vp = reinterpret_cast<const uint32_t *>(V + (size_t)g * BZX_G_SIZE);
#pragma unroll
        for (uint32_t k = 0; k < BZX_G_SIZE / 2; k++) vw[k] = vp[k];
        gb = GB[g];
        sel = SEL[g];
    }
}

// Work item: EMIT_TPI consecutive tiles of one block (item slot s of block j is item j * EMIT_SLOTS + s, empty slots
// are skipped by the lane that fetches), so that the tiles of a batch are dealt evenly over the resident workgroups
// and one block alone still spreads over the chip.  The item with a block's first tile also writes sections (a)-(c).
__global__ __launch_bounds__(EMIT_NT) void bzx_emit_kernel(BzxBatch B)
{
    const uint32_t tid = threadIdx.x, lane = bzx_lane(), wave = bzx_wave();
    unsigned long long t_last = 0;
    const uint32_t n_items = B.nblk * EMIT_SLOTS;
    uint4 *stage4 = reinterpret_cast<uint4 *>(e_stage);
    for (uint32_t i = tid; i < EMIT_STAGE_WORDS / 4; i += EMIT_NT) stage4[i] = make_uint4(0u, 0u, 0u, 0u);

    for (;;) {
        if (tid == 0) {
            uint32_t id;
            for (;;) {
                id = atomicAdd(&B.counters[3], 1u);
                if (id >= n_items || id % EMIT_SLOTS == 0) break;
                const uint32_t bb = B.blk_first + (id / EMIT_SLOTS) * B.blk_step;
                if ((id % EMIT_SLOTS) * (EMIT_TPI * EMIT_NT) < B.blk[bb].n_selectors) break;
            }
            e_bcast[0] = id;
        }
        __syncthreads();
        const uint32_t id = bzx_uni(e_bcast[0]);
        __syncthreads();
        if (id >= n_items) break;
        const uint32_t slot = id % EMIT_SLOTS;
        const uint32_t b = B.blk_first + (id / EMIT_SLOTS) * B.blk_step;

        if (B.dbg && tid == 0) t_last = wall_clock64();
        const BzxBlock d = B.blk[b];
        const uint32_t alpha = d.n_in_use + 2, n_mtf = d.n_mtf, n_sel = d.n_selectors, n_groups = d.n_groups;
        const uint16_t *__restrict__ V = B.mtfv + BZX_SLAB(B, b) * BZX_BLK_STRIDE;
        const uint8_t *__restrict__ SEL = B.selector + BZX_SLAB(B, b) * BZX_SEL_STRIDE;
        const uint8_t *__restrict__ SELM = B.selector_mtf + BZX_SLAB(B, b) * BZX_SEL_STRIDE;
        const uint16_t *__restrict__ GB = B.gbits + BZX_SLAB(B, b) * BZX_SEL_STRIDE;
        const uint32_t *__restrict__ TB = B.tbits + BZX_SLAB(B, b) * BZX_TILE_STRIDE;
        uint32_t *out = B.out;

        // final stream position, or (sharded runs) the same bit phase inside this rank's packed buffer
        const uint64_t ob = B.packed ? d.pack_word * 32 + (d.out_bit & 31u) : d.out_bit;
        const uint64_t o_map = ob + 105;
        const uint64_t o_ng = o_map + d.sec_bits[3];
        const uint64_t o_sel = o_ng + 18;
        const uint64_t o_tab = o_sel + d.sec_bits[0];
        const uint64_t o_pay = o_tab + d.sec_bits[1];

        // the item's tiles; the first one's loads leave before anything waits
        const uint32_t n_tiles = (n_sel + EMIT_NT - 1) / EMIT_NT;
        const uint32_t t0 = slot * EMIT_TPI, t1 = t0 + EMIT_TPI < n_tiles ? t0 + EMIT_TPI : n_tiles;
        for (uint32_t i = tid; i < 6 * 260; i += EMIT_NT) {
            const uint32_t t = i / 260, v = i % 260;
            if (v < BZX_MAX_ALPHA + 2) {
                const uint8_t l = B.len[BZX_SLAB(B, b) * 6 * 260 + i];
                if (slot == 0) e_len[t][v] = l;
                e_cl[t][v] = B.code[BZX_SLAB(B, b) * 6 * 260 + i] | ((uint32_t)l << 24);
            }
        }
        uint32_t vn[BZX_G_SIZE / 2], gbn, seln, tbn;
        emit_load_tile(V, GB, SEL, TB, t0, n_sel, vn, gbn, seln, tbn);
        bzx_lds_barrier();

        if (slot == 0) {
            // ---- (a) block header, symbol map, nGroups, nSelectors (compress_block.rs:34-48, huffman.rs:209-224)
            if (tid == 0) {
                BitW w;
                w.init(out, ob);
                w.put(24, 0x314159u);
                w.put(24, 0x265359u);
                w.put(32, d.crc);
                w.put(1, 0);
                w.put(24, d.orig_ptr);
                uint32_t l1 = 0, words[16];
                for (uint32_t i = 0; i < 16; i++) {
                    uint32_t wv = 0;
                    for (uint32_t j = 0; j < 16; j++)
                        if (B.in_use[BZX_SLAB(B, b) * 256 + i * 16 + j]) wv |= 0x8000u >> j;
                    words[i] = wv;
                    if (wv) l1 |= 0x8000u >> i;
                }
                w.put(16, l1);
                for (uint32_t i = 0; i < 16; i++)
                    if (words[i]) w.put(16, words[i]);
                w.put(3, n_groups);
                w.put(15, n_sel);
                w.finish();
            }

            EMIT_STAMP(48);
            // ---- (b) selectors, unary (huffman.rs:237-292)
            {
                const uint32_t per = (n_sel + EMIT_NT - 1) / EMIT_NT;
                const uint32_t lo = tid * per < n_sel ? tid * per : n_sel;
                const uint32_t hi = lo + per < n_sel ? lo + per : n_sel;
                uint32_t my_bits = 0;
                for (uint32_t i = lo; i < hi; i++) my_bits += SELM[i] + 1u;
                uint32_t tot;
                const uint32_t ex = bzx_block_excl_sum_lds<EMIT_NT>(my_bits, e_scratch, tot);
                if (hi > lo) {
                    BitW w;
                    w.init(out, o_sel + ex);
                    for (uint32_t i = lo; i < hi; i++) {
                        const uint32_t j = SELM[i];
                        w.put(j + 1, ((1u << j) - 1u) << 1);
                    }
                    w.finish();
                }
            }

            EMIT_STAMP(49);
            // ---- (c) coding tables, delta coded (huffman.rs:391-438), one lane per table
            if (lane == 0 && wave < n_groups) {
                uint32_t bits = 5;
                int32_t curr = e_len[wave][0];
                for (uint32_t i = 0; i < alpha; i++) {
                    const int32_t l = e_len[wave][i];
                    bits += 2u * (uint32_t)(l > curr ? l - curr : curr - l) + 1u;
                    curr = l;
                }
                e_tabbits[wave] = bits;
            }
            bzx_lds_barrier();
            if (lane == 0 && wave < n_groups) {
                uint64_t pos = o_tab;
                for (uint32_t t = 0; t < wave; t++) pos += e_tabbits[t];
                BitW w;
                w.init(out, pos);
                int32_t curr = e_len[wave][0];
                w.put(5, (uint32_t)curr);
                for (uint32_t i = 0; i < alpha; i++) {
                    const int32_t l = e_len[wave][i];
                    while (curr < l) {
                        w.put(2, 2);
                        curr++;
                    }
                    while (curr > l) {
                        w.put(2, 3);
                        curr--;
                    }
                    w.put(1, 0);
                }
                w.finish();
            }
            EMIT_STAMP(50);
        }

        // ---- (d) payload (huffman.rs:452-466): one lane per group.  A group's place in its tile comes from a scan of the
        // tile's group sizes, the tile's place in the payload from the Huffman stage (TB).  The lanes pack into the
        // staging area; the workgroup then copies the tile's words out, consecutive lanes consecutive words, 16 bytes
        // each where all four words are the tile's alone.  Only the first and the last word of a tile can be shared
        // (with the next tile, the section in front or the next block): those are merged with atomicOr into the zeroed
        // output.  The next tile's loads are in flight meanwhile.
        for (uint32_t t = t0; t < t1; t++) {
            uint32_t vw[BZX_G_SIZE / 2];
#pragma unroll
            for (uint32_t k = 0; k < BZX_G_SIZE / 2; k++) vw[k] = vn[k];
            const uint32_t gb = gbn, sel = seln;
            const uint64_t start = o_pay + bzx_uni(tbn);
            if (t + 1 < t1) emit_load_tile(V, GB, SEL, TB, t + 1, n_sel, vn, gbn, seln, tbn);

            uint32_t tot;
            const uint32_t ex = bzx_block_excl_sum_lds<EMIT_NT>(gb, e_scratch, tot);
            const uint64_t wbase = start >> 5;
            const uint32_t phase = (uint32_t)(start & 31u);
            // the tile's first word sits at staging word `off`, so that 16-byte pieces line up in LDS and in the output
            const uint32_t off = (uint32_t)((uintptr_t)(out + wbase) >> 2) & 3u;
            const uint32_t g = t * EMIT_NT + tid;
            if (g < n_sel) {
                const uint32_t gs = g * BZX_G_SIZE;
                const uint32_t cnt = (n_mtf - gs < BZX_G_SIZE) ? n_mtf - gs : BZX_G_SIZE;
                const uint32_t *__restrict__ cl = e_cl[sel];
                BitWT<false> w;
                w.init(e_stage, off * 32u + phase + ex);
#pragma unroll
                for (uint32_t k = 0; k < BZX_G_SIZE / 2; k++) {
                    const uint32_t c0 = 2 * k < cnt ? cl[vw[k] & 0xffffu] : 0u;
                    const uint32_t c1 = 2 * k + 1 < cnt ? cl[vw[k] >> 16] : 0u;
                    w.put(c0 >> 24, c0 & 0xffffffu);
                    w.put(c1 >> 24, c1 & 0xffffffu);
                }
                w.finish();
            }
            bzx_lds_barrier();
            const uint32_t end = off + ((phase + tot + 31u) >> 5);          // staging words [off, end) are the tile's
            uint32_t *gbase = out + wbase - off;                            // 16-byte aligned
            for (uint32_t i0 = 4 * tid; i0 < end; i0 += 4 * EMIT_NT) {
                const uint4 v = stage4[i0 / 4];
                stage4[i0 / 4] = make_uint4(0u, 0u, 0u, 0u);
                const uint32_t x[4] = {__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z),
                                       __builtin_bswap32(v.w)};
                if (i0 > off && i0 + 4 < end) {
                    *reinterpret_cast<uint4 *>(gbase + i0) = make_uint4(x[0], x[1], x[2], x[3]);
                } else {
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++) {
                        const uint32_t i = i0 + c;
                        if (i < off || i >= end) continue;
                        if (i == off || i + 1 == end) {
                            if (x[c]) atomicOr(gbase + i, x[c]);
                        } else {
                            gbase[i] = x[c];
                        }
                    }
                }
            }
            bzx_lds_barrier();
        }
        EMIT_STAMP(51);
    }
}

extern "C" void bzx_emit_geometry(uint32_t *tile_groups, uint32_t *tiles_per_item, uint32_t *staging_bits)
{
    if (tile_groups) *tile_groups = EMIT_NT;
    if (tiles_per_item) *tiles_per_item = EMIT_TPI;
    if (staging_bits) *staging_bits = (EMIT_STAGE_WORDS - 4u) * 32u;
}

// out_bit of every block: first_bit + exclusive scan of block sizes (stream mode, stride_bits == 0)
// or b * stride_bits (per-block mode).  total[0] = first_bit + sum of sizes.
// phase (optional, chunked streams): the first bit comes from phase[0] on the device (bit phase 0..31 left by the
// previous chunk of the stream); afterwards phase[0] = phase of the next chunk, phase[1] = bits of this one.
__global__ __launch_bounds__(EMIT_NT) void bzx_layout_kernel(BzxBatch B, uint64_t first_bit, uint64_t stride_bits,
                                                            uint64_t *total, uint64_t *phase)
{
    __shared__ uint64_t l_wsum[EMIT_NW];
    __shared__ uint64_t l_carry;
    const uint32_t tid = threadIdx.x, lane = bzx_lane(), wave = bzx_wave();
    if (phase) first_bit = phase[0];
    if (tid == 0) l_carry = first_bit;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < B.nblk; b0 += EMIT_NT) {
        const uint32_t b = b0 + tid;
        const uint64_t v = b < B.nblk ? B.blk[b].bits : 0ull;
        uint64_t x = v;
        for (uint32_t dd = 1; dd < 64; dd <<= 1) {
            const uint64_t y = __shfl_up(x, dd);
            if (lane >= dd) x += y;
        }
        if (lane == 63) l_wsum[wave] = x;
        const uint64_t carry = l_carry;
        __syncthreads();
        uint64_t pre = 0, tot = 0;
        for (uint32_t i = 0; i < EMIT_NW; i++) {
            if (i < wave) pre += l_wsum[i];
            tot += l_wsum[i];
        }
        if (b < B.nblk) B.blk[b].out_bit = stride_bits ? (uint64_t)b * stride_bits : carry + pre + x - v;
        __syncthreads();
        if (tid == 0) l_carry = carry + tot;
        __syncthreads();
    }
    if (tid == 0) {
        total[0] = l_carry;
        if (phase) {
            phase[1] = l_carry - first_bit;
            phase[0] = l_carry & 31u;
        }
    }
}

// "BZh<level>" at bit 0, footer magic + combined CRC behind the last block; out_bytes[0] = stream length.
__global__ __launch_bounds__(256) void bzx_stream_frame_kernel(BzxBatch B, int level, const uint64_t *total,
                                                               uint64_t *out_bytes)
{
    // combined CRC (crc.rs:25-27): c = rotl(c, 1) ^ crc_b over the blocks in order.  Rotation is linear over
    // XOR, so c = XOR_b rotl(crc_b, (nblk - 1 - b) mod 32): one pass over the descriptors by the whole workgroup.
    __shared__ uint32_t part[4];
    if (blockIdx.x != 0) return;
    uint32_t x = 0;
    for (uint32_t b = threadIdx.x; b < B.nblk; b += blockDim.x) {
        const uint32_t c = B.blk[b].crc, r = (B.nblk - 1u - b) & 31u;
        x ^= r ? ((c << r) | (c >> (32u - r))) : c;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x ^= __shfl_xor(x, d);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t combined = part[0] ^ part[1] ^ part[2] ^ part[3];
    BitW w;
    w.init(B.out, 0);
    w.put(8, 'B');
    w.put(8, 'Z');
    w.put(8, 'h');
    w.put(8, (uint32_t)('0' + level));
    w.finish();
    const uint64_t end = total[0];
    w.init(B.out, end);
    w.put(24, 0x177245u);
    w.put(24, 0x385090u);
    w.put(32, combined);
    w.finish();
    out_bytes[0] = (end + 80 + 7) >> 3;
}

// Sharded runs (round-robin blocks over GPUs): export my blocks' sizes / import everybody's sizes.
__global__ void bzx_bits_export_kernel(BzxBatch B, long long *bits)
{
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < B.nblk; j += gridDim.x * blockDim.x) {
        const uint32_t b = B.blk_first + j * B.blk_step;
        bits[b] = (long long)(B.blk[b].bits | ((uint64_t)B.blk[b].crc << 32));   // size (< 2^32 bits) and CRC of my block
    }
}
__global__ void bzx_bits_import_kernel(BzxBatch B, const long long *bits)
{
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B.nblk; b += gridDim.x * blockDim.x)
    {
        B.blk[b].bits = (uint64_t)bits[b] & 0xffffffffull;
        B.blk[b].crc = (uint32_t)((uint64_t)bits[b] >> 32);
    }
}
// Packed layout of one rank's blocks (b = first + j*step): every image starts on a word boundary of the packed
// buffer with the bit phase it has in the final stream, so merging is a word-wise OR.  total[0] = words used.
__global__ __launch_bounds__(EMIT_NT) void bzx_pack_layout_kernel(BzxBatch B, uint32_t first, uint32_t step,
                                                                 uint32_t nown, uint64_t *total)
{
    __shared__ uint64_t l_wsum[EMIT_NW];
    __shared__ uint64_t l_carry;
    const uint32_t tid = threadIdx.x, lane = bzx_lane(), wave = bzx_wave();
    if (tid == 0) l_carry = 0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < nown; j0 += EMIT_NT) {
        const uint32_t j = j0 + tid;
        const uint32_t b = first + j * step;
        const uint64_t v = j < nown ? (((B.blk[b].out_bit & 31u) + B.blk[b].bits + 31u) >> 5) : 0ull;
        uint64_t x = v;
        for (uint32_t dd = 1; dd < 64; dd <<= 1) {
            const uint64_t y = __shfl_up(x, dd);
            if (lane >= dd) x += y;
        }
        if (lane == 63) l_wsum[wave] = x;
        const uint64_t carry = l_carry;
        __syncthreads();
        uint64_t pre = 0, tot = 0;
        for (uint32_t i = 0; i < EMIT_NW; i++) {
            if (i < wave) pre += l_wsum[i];
            tot += l_wsum[i];
        }
        if (j < nown) B.blk[b].pack_word = carry + pre + x - v;
        __syncthreads();
        if (tid == 0) l_carry = carry + tot;
        __syncthreads();
    }
    if (tid == 0) total[0] = l_carry;
}

// Largest packed buffer of any rank, in words (every rank knows every block's size and position after the exchange
// of sizes, so the common length of the gather needs no further collective and no extra host round trip).
__global__ __launch_bounds__(EMIT_NT) void bzx_pack_max_kernel(BzxBatch B, uint32_t world, uint64_t *out)
{
    __shared__ unsigned long long sums[64];
    const uint32_t tid = threadIdx.x;
    if (tid < 64) sums[tid] = 0;
    __syncthreads();
    for (uint32_t b = tid; b < B.nblk; b += EMIT_NT)
        atomicAdd(&sums[b % world], (unsigned long long)(((B.blk[b].out_bit & 31u) + B.blk[b].bits + 31u) >> 5));
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = 0;
        for (uint32_t r = 0; r < world && r < 64; r++) m = sums[r] > m ? sums[r] : m;
        out[0] = m;
    }
}

// Merge one rank's packed buffer into the final stream: interior words are owned by one block, the first and
// last word of an image may be shared with its neighbours and are OR-ed into the zeroed buffer.
__global__ __launch_bounds__(256) void bzx_unpack_kernel(BzxBatch B, const uint32_t *__restrict__ packed, uint32_t first,
                                                        uint32_t step, uint32_t nown)
{
    for (uint32_t j = blockIdx.x; j < nown; j += gridDim.x) {
        const BzxBlock d = B.blk[first + j * step];
        const uint64_t nw = ((d.out_bit & 31u) + d.bits + 31u) >> 5;
        const uint32_t *src = packed + d.pack_word;
        uint32_t *dst = B.out + (d.out_bit >> 5);
        for (uint64_t w = threadIdx.x; w < nw; w += blockDim.x) {
            const uint32_t v = src[w];
            if (w == 0 || w + 1 == nw) {
                if (v) atomicOr(&dst[w], v);
            } else {
                dst[w] = v;
            }
        }
    }
}

// Sharded assembly writes every interior word of a block image with a plain store; only the words that are merged
// with atomicOr need to start from zero: the first and last word of every image, the header word and the first
// and last word of the footer.  (Zeroing the whole stream instead costs a pass over gigabytes at N = 8.)
__global__ __launch_bounds__(256) void bzx_zero_edges_kernel(BzxBatch B, const uint64_t *total)
{
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B.nblk; b += gridDim.x * blockDim.x) {
        const uint64_t ob = B.blk[b].out_bit, nb = B.blk[b].bits;
        B.out[ob >> 5] = 0;
        if (nb) B.out[(ob + nb - 1) >> 5] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t end = total[0];
        B.out[0] = 0;
        for (uint64_t w = end >> 5; w <= (end + 79) >> 5; w++) B.out[w] = 0;
    }
}

void bzx_launch_zero_edges(const BzxBatch &B, const uint64_t *d_total, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_zero_edges_kernel, dim3(64), dim3(256), 0, stream, B, d_total);
}

void bzx_launch_pack_layout(const BzxBatch &B, uint32_t first, uint32_t step, uint32_t nown, uint64_t *d_total,
                            hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_pack_layout_kernel, dim3(1), dim3(EMIT_NT), 0, stream, B, first, step, nown, d_total);
}
void bzx_launch_pack_max(const BzxBatch &B, uint32_t world, uint64_t *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_pack_max_kernel, dim3(1), dim3(EMIT_NT), 0, stream, B, world, d_out);
}
void bzx_launch_unpack(const BzxBatch &B, const uint32_t *packed, uint32_t first, uint32_t step, uint32_t nown,
                       uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_unpack_kernel, dim3(grid), dim3(256), 0, stream, B, packed, first, step, nown);
}

void bzx_launch_bits_export(const BzxBatch &B, long long *bits, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_bits_export_kernel, dim3(64), dim3(256), 0, stream, B, bits);
}
void bzx_launch_bits_import(const BzxBatch &B, const long long *bits, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_bits_import_kernel, dim3(64), dim3(256), 0, stream, B, bits);
}

void bzx_launch_emit(const BzxBatch &B, uint32_t n_cu, hipStream_t stream)
{
    // two workgroups fit a compute unit (62 KB of LDS each); fewer when the batch has fewer item slots than that
    const uint64_t slots = (uint64_t)B.nblk * EMIT_SLOTS;
    const uint32_t grid = slots < 2ull * n_cu ? (uint32_t)slots : 2u * n_cu;
    hipLaunchKernelGGL(bzx_emit_kernel, dim3(grid), dim3(EMIT_NT), 0, stream, B);
}

void bzx_launch_layout(const BzxBatch &B, uint64_t first_bit, uint64_t stride_bits, uint64_t *d_total_bits,
                       hipStream_t stream, uint64_t *d_phase)
{
    hipLaunchKernelGGL(bzx_layout_kernel, dim3(1), dim3(EMIT_NT), 0, stream, B, first_bit, stride_bits, d_total_bits,
                       d_phase);
}

void bzx_launch_stream_frame(const BzxBatch &B, int level, const uint64_t *d_total_bits, uint64_t *d_out_bytes,
                             hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_stream_frame_kernel, dim3(1), dim3(256), 0, stream, B, level, d_total_bits, d_out_bytes);
}
