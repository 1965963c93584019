// bzx_decomp.hip -- bzip2 decompression on gfx950 (round-trip verification on the device).
//
// Contract (reference src/compression/decompress.rs:38-404; bwt_decode bwt_sort.rs:91-130; rle2_mtf_decode_fast
// rle2_mtf.rs:191-287; rle1_decode rle1.rs:267-316; decode_sym_map symbol_map.rs:20-42): .bz2 stream -> raw bytes,
// every block CRC and the combined CRC checked.  The reference decodes one block after the other on one thread; here
// the blocks of a stream are decoded side by side:
//   scan      every bit offset is tested for the 48-bit block magic / end-of-stream magic (blocks start at arbitrary
//             bits): bzx_dc_scan_word (bzx_dc.h) inside the scan kernels of bzx_dbatch.hip and bzx_dstream.hip, which
//             also order the candidates and walk the chain of blocks; a candidate that does not continue the chain
//             is a chance match inside compressed data and is skipped (DC_SKIP)
//   decode    one wave per block: header, symbol map, selectors, code lengths (decompress.rs:98-260), then the
//             Huffman / MTF / RUNA-RUNB loop (decompress.rs:293-358).  The bit reader and the Huffman tables are
//             wave-uniform; the 256-entry MTF list lives in four registers per lane and a move-to-front is a few
//             cross-lane shifts for any rank; decoded bytes (and, for the inverse BWT, the number of earlier
//             occurrences of the same byte) leave through 64-entry coalesced stores
//   ibwt      T[C[L[i]] + occ[i]] = i is a plain scatter (the decoder already counted occ), then ONE pointer walk
//             per block, 64 blocks per wave (bwt_sort.rs:91-130); the walk also measures the RLE1 expansion and
//             leaves a checkpoint every 4096 bytes
//   expand    RLE1 runs are expanded from the checkpoints in parallel (rle1.rs:267-316) at the block's final
//             offset; block CRCs with bzx_crc_range (bzx_rle1.h) over the output
// Integer/byte work, latency-bound (a serial bit stream and a serial pointer chase per block); all blocks of a
// round are in flight at once.  This file holds the kernels and their launchers; every block is read through its
// BzxDcSrc and written through its BzxDcDst, so one set of kernels serves the one-shot calls, the batch and the stream.
#include <hip/hip_runtime.h>
#include "bzx_host.h"
#include "bzx_rle1.h"
#include "bzx_wg.h"

#define DC_CK_SHIFT 12             // a checkpoint every 4096 bytes of the RLE1 image
#define DC_CK_STRIDE 224           // checkpoints per block slab (900000 / 4096 + 1 = 220)

// ---- decode ---------------------------------------------------------------------------------------------------
// Wave-uniform bit reader over big-endian 32-bit words: every lane keeps one word of a 64-word window.
struct DcBits {
    const uint8_t *z;
    uint64_t nbytes;
    uint64_t win_word;      // index of the window's first 32-bit word
    uint32_t mine;          // my word of the window
    uint64_t pos;           // next bit
    __device__ __forceinline__ void load_window(uint64_t w0)
    {
        win_word = w0;
        const uint64_t b = (w0 + bzx_lane()) * 4;
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) v = (v << 8) | (b + i < nbytes ? z[b + i] : 0u);
        mine = v;
    }
    __device__ __forceinline__ void init(const uint8_t *z_, uint64_t nbytes_, uint64_t bit)
    {
        z = z_;
        nbytes = nbytes_;
        pos = bit;
        load_window(bit >> 5);
    }
    // the next n (<= 32) bits, not consumed
    __device__ __forceinline__ uint32_t peek(uint32_t n)
    {
        uint64_t w = pos >> 5;
        if (w + 1 >= win_word + 64) load_window(w);          // both words inside the window
        const uint32_t k = (uint32_t)(w - win_word);
        const uint64_t a = __shfl(mine, (int)k), b = __shfl(mine, (int)(k + 1));
        const uint64_t x = (a << 32) | b;
        return (uint32_t)((x << (pos & 31u)) >> (64u - n));
    }
    __device__ __forceinline__ uint32_t get(uint32_t n)
    {
        const uint32_t v = peek(n);
        pos += n;
        return v;
    }
    __device__ __forceinline__ bool past_end() const { return pos > nbytes * 8; }
};

__shared__ int32_t d_limit[6][24];
__shared__ int32_t d_base[6][24];
__shared__ uint16_t d_perm[6][260];
__shared__ uint8_t d_len[6][260];
__shared__ uint32_t d_minlen[6];
__shared__ uint32_t d_count[256];      // occurrences of every byte so far (unzftab)
__shared__ uint8_t d_seq2byte[256];

// hbCreateDecodeTables of libbz2 / huf_decode_map (decompress.rs:426-486) for table t.
__device__ static void dc_make_tables(uint32_t t, uint32_t alpha)
{
    uint32_t minl = 32, maxl = 0;
    for (uint32_t i = 0; i < alpha; i++) {
        const uint32_t l = d_len[t][i];
        maxl = l > maxl ? l : maxl;
        minl = l < minl ? l : minl;
    }
    uint32_t pp = 0;
    for (uint32_t l = minl; l <= maxl; l++)
        for (uint32_t j = 0; j < alpha; j++)
            if (d_len[t][j] == l) d_perm[t][pp++] = (uint16_t)j;
    for (uint32_t i = 0; i < 24; i++) {
        d_base[t][i] = 0;
        d_limit[t][i] = 0;
    }
    for (uint32_t i = 0; i < alpha; i++) d_base[t][d_len[t][i] + 1]++;
    for (uint32_t i = 1; i < 23; i++) d_base[t][i] += d_base[t][i - 1];
    int32_t vec = 0;
    for (uint32_t l = minl; l <= maxl; l++) {
        vec += d_base[t][l + 1] - d_base[t][l];
        d_limit[t][l] = vec - 1;
        vec <<= 1;
    }
    for (uint32_t l = minl + 1; l <= maxl; l++) d_base[t][l] = ((d_limit[t][l - 1] + 1) << 1) - d_base[t][l];
    d_minlen[t] = minl;
}

// One wave per block.  Block j starts (its magic) at bit src[j].bit of src[j].z[0, src[j].nbytes).  Outputs: L bytes
// (B.bwt slab), occ ranks (u32, B.rec_a slab), byte counts (B.freq slab), descriptor: n (at most BZX_MAX_N; the host
// holds it against 100000 * level of the block's stream), crc (stored), orig_ptr, bits = bit after the block's last
// symbol, status (DC_ERR_* on malformed data).
__global__ __launch_bounds__(64) void bzx_dc_decode_kernel(BzxBatch B, const BzxDcSrc *__restrict__ src)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b >= B.nblk) return;
    BzxBlock &D = B.blk[b];
    uint8_t *__restrict__ L = B.bwt + (size_t)b * BZX_BLK_STRIDE;
    uint32_t *__restrict__ OCC = reinterpret_cast<uint32_t *>(B.rec_a + (size_t)b * BZX_MAX_N);
    uint8_t *__restrict__ SEL = B.selector + (size_t)b * BZX_SEL_STRIDE;
    const uint64_t start = src[b].bit;
    DcBits br;
    br.init(src[b].z, src[b].nbytes, start + 48);
    uint32_t err = 0;
    const uint32_t crc = br.get(32);
    const uint32_t randomised = br.get(1);
    const uint32_t orig = br.get(24);
    // never written by bzip2 >= 0.9.5 nor by the reference (compress_block.rs:41); de-randomising is not implemented
    if (randomised) err |= BZX_ST_DC_RANDOMISED;
    // symbol map (symbol_map.rs:20-42)
    const uint32_t l1 = br.get(16);
    uint32_t n_in_use = 0;
    for (uint32_t i = 0; i < 16; i++) {
        if ((l1 >> (15 - i)) & 1u) {
            const uint32_t w = br.get(16);
            for (uint32_t j = 0; j < 16; j++)
                if ((w >> (15 - j)) & 1u) {
                    if (lane == 0) d_seq2byte[n_in_use] = (uint8_t)(i * 16 + j);
                    n_in_use++;
                }
        }
    }
    const uint32_t alpha = n_in_use + 2;
    const uint32_t n_groups = br.get(3);
    const uint32_t n_sel = br.get(15);
    // any count the 15-bit field holds; only the first BZX_MAX_SEL are kept (libbz2 >= 1.0.8 and decompress.rs ignore
    // the rest: no block has more than ceil(900001 / 50) groups)
    if (n_in_use == 0 || n_groups < 2 || n_groups > 6 || n_sel < 1) err |= DC_ERR_HEADER;
    const uint32_t n_sel_kept = n_sel < BZX_MAX_SEL ? n_sel : BZX_MAX_SEL;
    if (!err) {
        // selectors: unary MTF indices (decompress.rs:159-203)
        uint32_t pos[6] = {0, 1, 2, 3, 4, 5};
        for (uint32_t i = 0; i < n_sel && !err; i++) {
            uint32_t j = 0;
            while (br.get(1)) {
                j++;
                if (j >= n_groups || br.past_end()) {
                    err |= DC_ERR_HEADER;
                    break;
                }
            }
            if (err) break;
            const uint32_t v = pos[j];
            for (uint32_t k = j; k > 0; k--) pos[k] = pos[k - 1];
            pos[0] = v;
            if (lane == 0 && i < BZX_MAX_SEL) SEL[i] = (uint8_t)v;
        }
        // code lengths, delta coded (decompress.rs:216-260)
        for (uint32_t t = 0; t < n_groups && !err; t++) {
            int32_t cur = (int32_t)br.get(5);
            for (uint32_t i = 0; i < alpha; i++) {
                for (;;) {
                    if (cur < 1 || cur > 20 || br.past_end()) {
                        err |= DC_ERR_HEADER;
                        break;
                    }
                    if (!br.get(1)) break;
                    cur += br.get(1) ? -1 : 1;
                }
                if (err) break;
                if (lane == 0) d_len[t][i] = (uint8_t)cur;
            }
        }
    }
    __syncthreads();
    if (!err && lane < n_groups) dc_make_tables(lane, alpha);
    for (uint32_t i = lane; i < 256; i += 64) d_count[i] = 0;
    __syncthreads();

    // ---- Huffman + MTF + RUNA/RUNB (decompress.rs:293-358, rle2_mtf.rs:191-287)
    uint32_t v0 = lane, v1 = lane + 64, v2 = lane + 128, v3 = lane + 192;      // MTF list: position p = lane + 64*slot
    uint32_t n = 0;                           // bytes decoded
    uint32_t pend_b = 0, pend_o = 0;          // my slot of the 64-entry output stage
    uint32_t run = 0, run_w = 1;              // pending zero run (bijective base 2)
    const uint32_t eob = n_in_use + 1;
    uint32_t g = 0, g_left = 0, tsel = 0;
    auto emit = [&](uint32_t byte, uint32_t count) {
        // `count` copies of `byte` at L[n ..]; occ = d_count[byte] ..; all lanes take part (wave-uniform arguments)
        const uint32_t c0 = d_count[byte];
        __syncthreads();
        if (lane == 0) d_count[byte] = c0 + count;
        uint32_t done = 0;
        while (done < count) {
            const uint32_t fill = n & 63u;
            const uint32_t k = count - done < 64u - fill ? count - done : 64u - fill;
            if (lane >= fill && lane < fill + k) {
                pend_b = byte;
                pend_o = c0 + done + (lane - fill);
            }
            n += k;
            done += k;
            if ((n & 63u) == 0) {
                L[n - 64 + lane] = (uint8_t)pend_b;
                OCC[n - 64 + lane] = pend_o;
            }
        }
    };
    while (!err) {
        if (g_left == 0) {
            if (g >= n_sel_kept) {
                err |= DC_ERR_DATA;
                break;
            }
            tsel = SEL[g++];
            g_left = 50;
        }
        g_left--;
        // canonical code: shortest length whose limit admits the prefix
        const uint32_t v20 = br.peek(20);
        uint32_t zn = d_minlen[tsel];
        int32_t zvec = (int32_t)(v20 >> (20 - zn));
        while (zn <= 20 && zvec > d_limit[tsel][zn]) {
            zn++;
            zvec = (int32_t)(v20 >> (20 - zn));
        }
        const int32_t idx = zvec - d_base[tsel][zn];
        if (zn > 20 || idx < 0 || idx >= (int32_t)alpha || br.past_end()) {
            err |= DC_ERR_DATA;
            break;
        }
        br.pos += zn;
        const uint32_t sym = d_perm[tsel][idx];
        if (sym <= 1) {                       // RUNA / RUNB
            run += (sym + 1) * run_w;
            run_w <<= 1;
            if (run > BZX_MAX_N) {
                err |= DC_ERR_DATA;
                break;
            }
            continue;
        }
        if (run) {
            if (n + run > BZX_MAX_N) {
                err |= DC_ERR_DATA;
                break;
            }
            emit(d_seq2byte[__shfl(v0, 0)], run);
            run = 0;
            run_w = 1;
        }
        if (sym == eob) break;
        if (n + 1 > BZX_MAX_N) {
            err |= DC_ERR_DATA;
            break;
        }
        // move the entry at position r = sym - 1 (>= 1) to the front: new[p] = p == 0 ? x : p <= r ? old[p-1] : old[p]
        // with p = lane + 64 * slot; old[p-1] comes from the lane below, or from lane 63 of the slot before
        const uint32_t r = sym - 1;
        const uint32_t sr = r >> 6, lr = r & 63u;
        const uint32_t o0 = v0, o1 = v1, o2 = v2, o3 = v3;
        const uint32_t src = sr == 0 ? o0 : sr == 1 ? o1 : sr == 2 ? o2 : o3;
        const uint32_t x = __shfl(src, (int)lr);
        {
            const uint32_t up = __shfl_up(o0, 1);
            v0 = lane == 0 ? x : (lane <= r ? up : o0);
        }
        if (r >= 64) {                                   // (text rarely gets here: ranks are small)
            const uint32_t up = __shfl_up(o1, 1), c = __shfl(o0, 63);
            v1 = lane + 64 <= r ? (lane == 0 ? c : up) : o1;
        }
        if (r >= 128) {
            const uint32_t up = __shfl_up(o2, 1), c = __shfl(o1, 63);
            v2 = lane + 128 <= r ? (lane == 0 ? c : up) : o2;
        }
        if (r >= 192) {
            const uint32_t up = __shfl_up(o3, 1), c = __shfl(o2, 63);
            v3 = lane + 192 <= r ? (lane == 0 ? c : up) : o3;
        }
        emit(d_seq2byte[x], 1);
    }
    // flush the partial stage
    if ((n & 63u) && lane < (n & 63u)) {
        L[(n & ~63u) + lane] = (uint8_t)pend_b;
        OCC[(n & ~63u) + lane] = pend_o;
    }
    __syncthreads();
    for (uint32_t i = lane; i < 256; i += 64) B.freq[(size_t)b * 260 + i] = d_count[i];
    if (lane == 0) {
        if (!err && (n == 0 || orig >= n)) err |= DC_ERR_DATA;
        D.n = n;
        D.crc = crc;
        D.orig_ptr = orig;
        D.out_bit = start;
        D.bits = br.pos;
        D.status = err;
        D.n_in_use = n_in_use;
    }
}

// ---- inverse BWT (bwt_sort.rs:91-130) ---------------------------------------------------------------------------
// grid (tiles, blocks): TT[C[L[i]] + occ[i]] = i, C = exclusive prefix of the byte counts.
__global__ __launch_bounds__(256) void bzx_dc_scatter_kernel(BzxBatch B)
{
    __shared__ uint32_t c_start[256];
    __shared__ uint32_t c_scan[4];
    const uint32_t b = blockIdx.y, tid = threadIdx.x;
    if (B.blk[b].status) return;
    const uint32_t n = B.blk[b].n;
    {
        const uint32_t v = B.freq[(size_t)b * 260 + tid];
        const uint32_t incl = bzx_wave_incl_sum(v);
        if (bzx_lane() == 63) c_scan[bzx_wave()] = incl;
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t w = 0; w < bzx_wave(); w++) pre += c_scan[w];
        c_start[tid] = pre + incl - v;
    }
    __syncthreads();
    const uint8_t *__restrict__ L = B.bwt + (size_t)b * BZX_BLK_STRIDE;
    const uint32_t *__restrict__ OCC = reinterpret_cast<const uint32_t *>(B.rec_a + (size_t)b * BZX_MAX_N);
    uint32_t *__restrict__ TT = reinterpret_cast<uint32_t *>(B.rec_b + (size_t)b * BZX_MAX_N);
    for (uint32_t i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        const uint32_t j = c_start[L[i]] + OCC[i];
        if (j < n) TT[j] = i;
    }
}

// tt[j] = TT[j] << 8 | L[j]: one word per step of the walk (overwrites the occ array, no longer needed)
__global__ __launch_bounds__(256) void bzx_dc_pack_kernel(BzxBatch B)
{
    const uint32_t b = blockIdx.y;
    if (B.blk[b].status) return;
    const uint32_t n = B.blk[b].n;
    const uint8_t *__restrict__ L = B.bwt + (size_t)b * BZX_BLK_STRIDE;
    const uint32_t *__restrict__ TT = reinterpret_cast<const uint32_t *>(B.rec_b + (size_t)b * BZX_MAX_N);
    uint32_t *__restrict__ W = reinterpret_cast<uint32_t *>(B.rec_a + (size_t)b * BZX_MAX_N);
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) W[j] = (TT[j] << 8) | L[j];
}

struct DcCheck {
    uint32_t out_pos;       // expanded bytes before this image position
    uint32_t state;         // last byte | equal-run length so far (0..4) << 8
};

// One LANE per block: the pointer walk (a serial chain of dependent loads: ~n memory latencies per block, all blocks
// of the stream in flight).  Writes the RLE1 image, its expanded length and a checkpoint every 4096 image bytes.
__global__ __launch_bounds__(64) void bzx_dc_walk_kernel(BzxBatch B, uint8_t *__restrict__ img_slabs)
{
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B.nblk || B.blk[b].status) return;
    const uint32_t n = B.blk[b].n;
    const uint32_t *__restrict__ W = reinterpret_cast<const uint32_t *>(B.rec_a + (size_t)b * BZX_MAX_N);
    uint8_t *__restrict__ IMG = img_slabs + (size_t)b * BZX_BLK_STRIDE;
    DcCheck *__restrict__ CK = reinterpret_cast<DcCheck *>(B.gbits + (size_t)b * BZX_SEL_STRIDE);
    uint32_t tpos = W[B.blk[b].orig_ptr] >> 8;
    uint32_t last = 256, cnt = 0;
    uint64_t out = 0;
    for (uint32_t k = 0; k < n; k++) {
        if ((k & ((1u << DC_CK_SHIFT) - 1u)) == 0) {
            DcCheck c;
            c.out_pos = (uint32_t)out;
            c.state = (last & 0x1FFu) | (cnt << 9);
            CK[k >> DC_CK_SHIFT] = c;
        }
        if (tpos >= n) {                       // corrupt permutation: stop (the CRC check reports the block)
            B.blk[b].status = DC_ERR_DATA;
            break;
        }
        const uint32_t e = W[tpos];
        const uint32_t ch = e & 255u;
        tpos = e >> 8;
        IMG[k] = (uint8_t)ch;
        // RLE1 (rle1.rs:267-316): after four equal bytes the next one is a repeat count; then a fresh run starts
        if (cnt == 4) {
            out += ch;
            cnt = 0;
            last = 256;
        } else {
            cnt = ch == last ? cnt + 1 : 1;
            last = ch;
            out++;
        }
    }
    // four equal bytes end the block: libbz2 reads their count byte past the block's end and refuses the stream
    if (cnt == 4) B.blk[b].status = DC_ERR_DATA;
    B.blk[b].pack_word = out;                  // expanded length
}

// ---- the many-lane walk: one WORKGROUP per block (range reads: one to three blocks, nothing to hide the chase behind) --
// Leaves what bzx_dc_walk_kernel leaves -- IMG[0, n), the checkpoints, pack_word, the status -- for ANY L: the scatter
// makes T a permutation whatever L is, but one with several cycles when L is no BWT (or the BWT of u^k), and the
// one-lane walk then goes round the cycle of its start for n steps.
//   splitters   the walk's start p0 and every position that is a multiple of DW_STRIDE (a test on the position: no
//               marks).  The segments between splitters partition the cycles that hold one, so all walks together
//               take at most n steps, and each ends: a splitter's own cycle leads back to it.
//   phase A     a lane walks from a splitter to the next one it meets and records how many steps that took and which
//               splitter it met; lanes take splitters from an LDS counter until none is left.  The loop body is ONE
//               step: a lane that arrives takes its next splitter inside the same loop, so the lanes of a wave do not
//               wait for the longest segment among them.
//   phase B     one lane follows the splitters from the start until it is back there (at most n / DW_STRIDE + 2 LDS
//               reads) and turns the lengths into offsets; c, their sum, is the length of the start's cycle.
//   phase C     the lanes walk the segments of that cycle again and store their bytes at their offsets; then
//               IMG[i] = IMG[i mod c] for the rest.
// The RLE1 checkpoints are a pass of their own over IMG (bzx_dc_ckpt_kernel).
#define DW_NT 1024
#define DW_STRIDE 64u
#define DW_MAX_S ((BZX_MAX_N + DW_STRIDE - 1) / DW_STRIDE + 1)
#define DW_ON_CHAIN 0x80000000u

__global__ __launch_bounds__(DW_NT) void bzx_dc_wide_walk_kernel(BzxBatch B, uint8_t *__restrict__ img_slabs)
{
    __shared__ uint32_t s_len[DW_MAX_S];       // A: steps to the next splitter; B: DW_ON_CHAIN | offset of the segment
    __shared__ uint16_t s_nxt[DW_MAX_S];       // A: the splitter met
    __shared__ uint32_t s_fetch[2];            // work counters of phases A and C
    __shared__ uint32_t s_bad, s_cyc;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (B.blk[b].status) return;               // (uniform over the workgroup)
    const uint32_t n = B.blk[b].n;
    const uint32_t *__restrict__ W = reinterpret_cast<const uint32_t *>(B.rec_a + (size_t)b * BZX_MAX_N);
    uint8_t *IMG = img_slabs + (size_t)b * BZX_BLK_STRIDE;
    const uint32_t orig = B.blk[b].orig_ptr;
    const uint32_t p0 = orig < n ? W[orig] >> 8 : n;
    const uint32_t nsplit = (n + DW_STRIDE - 1) / DW_STRIDE + 1;       // splitter 0: p0; 1 + q: position q * DW_STRIDE
    if (tid == 0) {
        s_fetch[0] = 0;
        s_fetch[1] = 0;
        s_bad = p0 >= n ? 1u : 0u;
        s_cyc = 0;
    }
    __syncthreads();
    volatile uint32_t *bad = &s_bad;
    auto pos_of = [&](uint32_t s) { return s ? (s - 1u) * DW_STRIDE : p0; };
    auto id_of = [&](uint32_t pos) { return pos == p0 ? 0u : 1u + pos / DW_STRIDE; };
    auto is_split = [&](uint32_t pos) { return pos == p0 || (pos & (DW_STRIDE - 1u)) == 0; };
    // ---- A
    {
        uint32_t s = 0, pos = 0, len = 0;
        auto next = [&]() {                    // my next splitter; false: none left
            for (;;) {
                s = atomicAdd(&s_fetch[0], 1u);
                if (s >= nsplit || *bad) return false;
                pos = pos_of(s);
                len = 0;
                if (s && pos == p0) {          // the start is a multiple of the stride too: it is splitter 0
                    s_len[s] = 0;
                    s_nxt[s] = 0;
                    continue;
                }
                return true;
            }
        };
        bool live = next();
        while (live) {
            pos = W[pos] >> 8;
            len++;
            if (pos >= n || len > n) {         // no permutation (cannot follow from a decoded block): the block is refused
                *bad = 1;
                break;
            }
            if (is_split(pos)) {
                s_len[s] = len;
                s_nxt[s] = (uint16_t)id_of(pos);
                live = next();
            }
        }
    }
    __syncthreads();
    // ---- B
    if (tid == 0 && !*bad) {
        uint32_t s = 0, off = 0, steps = 0;
        do {
            const uint32_t len = s_len[s];
            if ((len & DW_ON_CHAIN) || off + len > n) {
                *bad = 1;
                break;
            }
            s_len[s] = DW_ON_CHAIN | off;
            off += len;
            s = s_nxt[s];
        } while (s != 0 && ++steps < nsplit);
        s_cyc = off;
    }
    __syncthreads();
    if (*bad) {
        if (tid == 0) {
            B.blk[b].status = DC_ERR_DATA;
            B.blk[b].pack_word = 0;
        }
        return;
    }
    // ---- C
    {
        uint32_t pos = 0, off = 0;
        auto next = [&]() {
            for (;;) {
                const uint32_t s = atomicAdd(&s_fetch[1], 1u);
                if (s >= nsplit) return false;
                const uint32_t v = s_len[s];
                if (!(v & DW_ON_CHAIN)) continue;          // a splitter of another cycle
                off = v & ~DW_ON_CHAIN;
                pos = pos_of(s);
                return true;
            }
        };
        bool live = next();
        while (live) {
            const uint32_t e = W[pos];
            if (off < n) IMG[off] = (uint8_t)e;
            off++;
            pos = e >> 8;
            if (is_split(pos)) live = next();
        }
    }
    __syncthreads();                           // the cycle's bytes are stored (and visible to this workgroup)
    const uint32_t c = s_cyc;
    for (uint32_t i = c + tid; i < n; i += DW_NT) IMG[i] = IMG[i % c];
}

__device__ __forceinline__ void dc_rle1_step(uint32_t ch, uint32_t &last, uint32_t &cnt, uint32_t &out)
{
    if (cnt == 4) {
        out += ch;
        cnt = 0;
        last = 256;
    } else {
        cnt = ch == last ? cnt + 1 : 1;
        last = ch;
        out++;
    }
}

// The RLE1 state machine over IMG[k0, k1), 16 bytes per load where the address allows it.
__device__ static void dc_rle1_run(const uint8_t *__restrict__ IMG, uint32_t k0, uint32_t k1, uint32_t &last, uint32_t &cnt,
                                   uint32_t &out)
{
    uint32_t k = k0;
    while (k < k1 && ((uintptr_t)(IMG + k) & 15u)) dc_rle1_step(IMG[k++], last, cnt, out);
    for (; k + 16 <= k1; k += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(IMG + k);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) dc_rle1_step((w[i >> 2] >> ((i & 3u) * 8u)) & 255u, last, cnt, out);
    }
    while (k < k1) dc_rle1_step(IMG[k++], last, cnt, out);
}

// One workgroup per block, one lane per 4096-byte segment of the image: the checkpoints, the expanded length and the
// "ends in four equal bytes" status, from IMG alone.  The RLE1 state at a segment's start depends on the bytes before
// it, but not on many of them: after three bytes a != b != c the state is (last = c, run = 1) whatever came before
// (c is no count byte, since a != b; if b was one, a run starts afresh at c; if not, c differs from it).  A lane looks
// for such a place in the segment before its own and runs the state machine from there.  Where the segment before has
// none -- stretches of one byte -- the state is carried over from the segment before that, one lane going through the
// segments in order.
__global__ __launch_bounds__(256) void bzx_dc_ckpt_kernel(BzxBatch B, const uint8_t *__restrict__ img_slabs)
{
    __shared__ uint32_t s_state[256];
    __shared__ uint32_t s_scan[4];
    const uint32_t b = blockIdx.x, g = threadIdx.x;
    if (B.blk[b].status) return;               // (uniform over the workgroup)
    const uint32_t n = B.blk[b].n;
    const uint32_t seg_len = 1u << DC_CK_SHIFT;
    const uint32_t nseg = (n + seg_len - 1) >> DC_CK_SHIFT;            // <= 220
    const uint8_t *__restrict__ IMG = img_slabs + (size_t)b * BZX_BLK_STRIDE;
    DcCheck *__restrict__ CK = reinterpret_cast<DcCheck *>(B.gbits + (size_t)b * BZX_SEL_STRIDE);
    const uint32_t k0 = g << DC_CK_SHIFT;
    const uint32_t unknown = 0xFFFFFFFFu;
    uint32_t st = unknown;
    if (g == 0) st = 256u;
    else if (g < nseg) {
        for (uint32_t j = k0; j >= k0 - seg_len + 3; j--) {
            const uint32_t x = IMG[j - 3], y = IMG[j - 2], z = IMG[j - 1];
            if (x != y && y != z) {
                uint32_t last = z, cnt = 1, out = 0;
                dc_rle1_run(IMG, j, k0, last, cnt, out);
                st = last | (cnt << 9);
                break;
            }
        }
    }
    s_state[g] = st;
    __syncthreads();
    if (g == 0) {
        for (uint32_t q = 1; q < nseg; q++)
            if (s_state[q] == unknown) {
                uint32_t last = s_state[q - 1] & 0x1FFu, cnt = s_state[q - 1] >> 9, out = 0;
                dc_rle1_run(IMG, (q - 1) << DC_CK_SHIFT, q << DC_CK_SHIFT, last, cnt, out);
                s_state[q] = last | (cnt << 9);
            }
    }
    __syncthreads();
    uint32_t last = 256, cnt = 0, out = 0;
    if (g < nseg) {
        st = s_state[g];
        last = st & 0x1FFu;
        cnt = st >> 9;
        dc_rle1_run(IMG, k0, k0 + seg_len < n ? k0 + seg_len : n, last, cnt, out);
    }
    uint32_t total = 0;
    const uint32_t before = bzx_block_excl_sum<256>(out, s_scan, total);
    if (g < nseg) {
        DcCheck c;
        c.out_pos = before;
        c.state = st;
        CK[g] = c;
    }
    if (g == nseg - 1) {
        // four equal bytes end the block: libbz2 reads their count byte past the block's end and refuses the stream
        if (cnt == 4) B.blk[b].status = DC_ERR_DATA;
        B.blk[b].pack_word = total;
    }
}

// grid (segments, blocks): expands one 4096-byte segment of the RLE1 image from its checkpoint to dst[b].p (at most
// dst[b].cap bytes from there; a null dst[b].p: the block is not written).
__global__ __launch_bounds__(64) void bzx_dc_expand_kernel(BzxBatch B, const uint8_t *__restrict__ img_slabs,
                                                          const BzxDcDst *__restrict__ dst)
{
    const uint32_t b = blockIdx.y;
    if (B.blk[b].status) return;
    uint8_t *__restrict__ out = dst[b].p;
    const uint64_t cap = dst[b].cap;
    if (!out) return;
    const uint32_t n = B.blk[b].n;
    const uint32_t seg = blockIdx.x * 64 + threadIdx.x;
    const uint32_t k0 = seg << DC_CK_SHIFT;
    if (k0 >= n) return;
    const uint32_t k1 = k0 + (1u << DC_CK_SHIFT) < n ? k0 + (1u << DC_CK_SHIFT) : n;
    const uint8_t *__restrict__ IMG = img_slabs + (size_t)b * BZX_BLK_STRIDE;
    const DcCheck c = reinterpret_cast<const DcCheck *>(B.gbits + (size_t)b * BZX_SEL_STRIDE)[seg];
    uint64_t o = c.out_pos;
    uint32_t last = c.state & 0x1FFu, cnt = c.state >> 9;
    for (uint32_t k = k0; k < k1; k++) {
        const uint32_t ch = IMG[k];
        if (cnt == 4) {
            for (uint32_t r = 0; r < ch; r++)
                if (o + r < cap) out[o + r] = (uint8_t)last;
            o += ch;
            cnt = 0;
            last = 256;
        } else {
            cnt = ch == last ? cnt + 1 : 1;
            last = ch;
            if (o < cap) out[o] = (uint8_t)ch;
            o++;
        }
    }
}

// ---- CRC-32/BZIP2 of every block the expansion placed (bzx_crc_range, bzx_rle1.h) -----------------------------------
__global__ __launch_bounds__(CRC_NT) void bzx_dc_crc_kernel(BzxBatch B, const BzxDcDst *__restrict__ dst,
                                                            uint32_t *__restrict__ got)
{
    __shared__ BzxCrcLds lds;
    const uint32_t my_weight = bzx_crc_setup(lds);
    for (uint32_t b = blockIdx.x; b < B.nblk; b += gridDim.x) {
        if (B.blk[b].status || !dst[b].p) continue;          // (uniform over the workgroup)
        const uint32_t crc = bzx_crc_range(dst[b].p, 0, B.blk[b].pack_word, lds, my_weight);
        if (threadIdx.x == 0) got[b] = crc;
    }
}

void bzx_launch_dc_decode(const BzxBatch &B, const BzxDcSrc *src, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_dc_decode_kernel, dim3(B.nblk), dim3(64), 0, stream, B, src);
}
void bzx_launch_dc_ibwt(const BzxBatch &B, uint8_t *img_slabs, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_dc_scatter_kernel, dim3(32, B.nblk), dim3(256), 0, stream, B);
    hipLaunchKernelGGL(bzx_dc_pack_kernel, dim3(32, B.nblk), dim3(256), 0, stream, B);
    hipLaunchKernelGGL(bzx_dc_walk_kernel, dim3((B.nblk + 63) / 64), dim3(64), 0, stream, B, img_slabs);
}
// The same contract with the many-lane walk: one workgroup per block (range reads: bzx_range.hip).  n_hint: about the
// length of the longest block; it sizes the grids of the two grid-stride kernels and nothing else.
void bzx_launch_dc_ibwt_wide(const BzxBatch &B, uint8_t *img_slabs, uint32_t n_hint, hipStream_t stream)
{
    const uint32_t tiles = n_hint >= 32 * 256 ? 32u : n_hint / 256 + 1;
    hipLaunchKernelGGL(bzx_dc_scatter_kernel, dim3(tiles, B.nblk), dim3(256), 0, stream, B);
    hipLaunchKernelGGL(bzx_dc_pack_kernel, dim3(tiles, B.nblk), dim3(256), 0, stream, B);
    hipLaunchKernelGGL(bzx_dc_wide_walk_kernel, dim3(B.nblk), dim3(DW_NT), 0, stream, B, img_slabs);
    hipLaunchKernelGGL(bzx_dc_ckpt_kernel, dim3(B.nblk), dim3(256), 0, stream, B, img_slabs);
}
void bzx_launch_dc_expand(const BzxBatch &B, const uint8_t *img_slabs, const BzxDcDst *dst, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_dc_expand_kernel, dim3((DC_CK_STRIDE + 63) / 64, B.nblk), dim3(64), 0, stream, B, img_slabs, dst);
}
void bzx_launch_dc_crc(const BzxBatch &B, const BzxDcDst *dst, uint32_t *got, uint32_t n_cu, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_dc_crc_kernel, dim3(B.nblk < n_cu ? B.nblk : n_cu), dim3(CRC_NT), 0, stream, B, dst, got);
}
