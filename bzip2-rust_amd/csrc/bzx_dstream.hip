// bzx_dstream.hip -- streaming decompression on gfx950 (include/bzx.h: bzx_dstream_*): the .bz2 arrives in pieces, the
// decoded bytes leave in pieces, device memory is fixed at bzx_dstream_begin.  The counterpart of bzx_cstream.hip.
//
// The kernels that decode a block (bzx_decomp.hip: decode, inverse BWT, expand) take per-block sources and
// destinations; this file adds the state between calls, the windowing and the device-side pieces that let a window be
// processed without the whole stream in view.
//   window                the undecoded tail of the window before (the carry) + the bytes accepted since, contiguous in
//                         one of two device input buffers: the accepted bytes go to the buffer that is not being
//                         decoded, behind a gap of DS_CARRY_MAX bytes that the carry is copied into when the buffers
//                         change roles.  Positions are bits from the start of the whole input, so the chain position
//                         survives the change of window.
//   scan, per window      every bit offset of [chain position, end) is tested for the block / end-of-stream magic; no
//                         stream header is expected at the start (a window usually starts inside a stream).  The
//                         candidates come back to the host once, are sorted there and go back to the device.  A full
//                         table halves the scanned range and scans again (the rest is scanned when the chain gets
//                         there): no limit on candidates per stream.                          [1 synchronisation]
//   round, <= R blocks    decode the next R block candidates from the chain position on (bzx_dc_decode_kernel through
//                         BzxDcSrc), then bzx_ds_chain_kernel: one wave walks the sorted candidates from the carried
//                         chain bit, marks chance matches of the magic with the skip status, tells a block that runs
//                         off the end of the window (withheld while more input may come; damage at `final` or when
//                         DS_BLOCK_BOUND bytes did not end it) from a damaged one, recognises end-of-stream, checks the
//                         stored combined CRC at its bit phase against the folded stored block CRCs, and follows a
//                         "BZh<level>" at the next byte boundary into the next stream.  Inverse BWT unchanged.
//   pass, <= 48 MiB       bzx_ds_layout_kernel: a wave-level scan of the expanded sizes gives the next chain blocks of
//                         the round their places in a staging area and cuts after the last block that fits (a block
//                         expands to at most 46.62 MB: every pass places at least one); blocks that did not fit stay
//                         decoded in their slabs for the next pass.  Expand (bzx_dc_expand_kernel through BzxDcDst),
//                         block CRCs (bzx_dc_crc_kernel), bzx_ds_verdict_kernel compares them with the stored ones and
//                         leaves ONE fixed-size record for the host.                          [1 synchronisation]
//                         The first pass of a round is enqueued behind its decode/chain/inverse BWT without a
//                         synchronisation in between: a round whose output fits one staging area costs one.
//   overlap               three HIP streams: accepted bytes travel to the device beside the kernels of the window
//                         before; the verified bytes of a pass travel to page-locked memory beside the kernels of the
//                         next pass (two staging areas); the host copies from there into the caller's buffer.
// Only verified bytes leave the device: the copy-back of a pass is sized by the record's verified byte count.
// Two more modes run on the same windows, scans and rounds: the index (bzx_index_*: nothing is copied back) and salvage
// (bzx_salvage_*: the walk goes on behind a block that does not verify; its kernels and passes are further down).
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bzx_host.h"
#include "bzx_wg.h"

#define DS_BLOCK_BOUND 2400000ull            // bytes: no legal block image is longer (18,002 x 50 x 20 bits + tables)
#define DS_CARRY_MAX (DS_BLOCK_BOUND + 4096) // gap in front of the accepted bytes: room for the longest carry
#define DS_STAGE_BYTES ((size_t)48 << 20)    // output staging area: at least one expanded block (46.62 MB)
#define DS_MIN_CHUNK ((size_t)16)               // (the carry has its own room: a small chunk only costs launches)
#define DS_DEF_CHUNK ((size_t)128 << 20)

enum { DS_STOP_GO = 0, DS_STOP_NOMAGIC, DS_STOP_WITHHELD, DS_STOP_END, DS_STOP_ERROR };

struct DsRec {                     // what the host reads of a pass (device -> page-locked host), fixed size
    uint64_t chain_bit;            // chain: where it stands after the round (bit of the whole input)
    uint64_t bytes;                // layout: bytes placed in the staging area by this pass
    uint64_t good_bytes;           // verdict: ... of which lie before the first block whose CRC did not match
    uint32_t nchain;               // chain: chain blocks of the round (slab numbers in d_chain, stream order)
    uint32_t streams;              // chain: streams finished in the round
    uint32_t comb;                 // chain: running combined CRC of the open stream
    uint32_t level;                // chain: level of the open stream
    uint32_t stop;                 // chain: DS_STOP_*
    uint32_t err;                  // chain: DcWhy behind the last chain block (stop == DS_STOP_ERROR)
    uint32_t pass_j0;              // layout: first chain block of this pass
    uint32_t placed;               // layout: chain blocks placed so far (this pass included)
    uint32_t lay_err;              // layout: the next chain block failed its inverse BWT
    uint32_t good;                 // verdict: blocks of this pass before the first CRC mismatch
};

// ---- scan: block / end-of-stream magics of window bytes [from, to), as bits of the whole input ---------------------
__global__ __launch_bounds__(256) void bzx_ds_scan_kernel(const uint8_t *__restrict__ z, uint64_t wlen, uint64_t from,
                                                          uint64_t to, uint64_t base_bit, uint64_t *__restrict__ found,
                                                          uint32_t *__restrict__ n_found, uint32_t cap)
{
    const uint64_t nwords = (to - from + 3) / 4;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * blockDim.x) {
        bzx_dc_scan_word(z, wlen, from + w * 4, [&](uint64_t bit, bool eos, uint64_t, uint64_t) {
            if (bit >= to * 8) return;
            const uint32_t k = atomicAdd(n_found, 1u);
            if (k < cap) found[k] = ((base_bit + bit) << 1) | (eos ? 1u : 0u);
        });
    }
}

__device__ __forceinline__ uint32_t ds_byte(const uint8_t *__restrict__ z, uint64_t wlen, uint64_t i)
{
    return i < wlen ? z[i] : 0u;
}

// ---- chain and framing of a round: one wave ----------------------------------------------------------------------
// cand[c0, c1): the round's candidates, sorted ((bit of the whole input) << 1 | end-of-stream); block candidate number
// k of them was decoded into slab k (B.blk[k]: status, n, stored CRC, bits = window bit behind its last symbol).
// Walks the chain from chain_bit; 64 candidates are loaded side by side, the walk over them is shuffles only.
__global__ __launch_bounds__(64) void bzx_ds_chain_kernel(BzxBatch B, const uint8_t *__restrict__ z, uint64_t wlen,
                                                         uint64_t base_bit, uint32_t final,
                                                         const uint64_t *__restrict__ cand, uint32_t c0, uint32_t c1,
                                                         uint64_t chain_bit, uint32_t comb, uint32_t level,
                                                         uint32_t *__restrict__ chain, DsRec *__restrict__ rec,
                                                         uint32_t *__restrict__ meta)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t wbits = wlen * 8;
    uint64_t at_bit = chain_bit;
    uint32_t nch = 0, streams = 0, stop = DS_STOP_GO, err = 0, nblk_before = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t k = base + lane;
        const bool valid = k < c1;
        const uint64_t pos = valid ? cand[k] : ~0ull;
        const bool isblk = valid && !(pos & 1u);
        const unsigned long long blks = __ballot(isblk);
        const uint32_t slab = nblk_before + (uint32_t)__popcll(blks & ((1ull << lane) - 1ull));
        uint32_t st = 0, n = 0, crc = 0;
        uint64_t endw = 0;
        if (isblk) {
            const BzxBlock &d = B.blk[slab];
            st = d.status;
            n = d.n;
            crc = d.crc;
            endw = d.bits;
        }
        bool mine_on_chain = false;
        const uint32_t cnt = c1 - base < 64u ? c1 - base : 64u;
        for (uint32_t i = 0; i < cnt && stop == DS_STOP_GO; i++) {        // (everything below is wave-uniform)
            const uint64_t p = __shfl(pos, (int)i);
            const uint64_t bit = p >> 1;
            if (bit < at_bit) continue;                                   // a chance match inside a chain block
            if (bit > at_bit) {
                stop = DS_STOP_NOMAGIC;
                break;
            }
            const uint64_t rel = bit - base_bit;
            if (!(p & 1u)) {
                const uint32_t st_i = __shfl(st, (int)i), n_i = __shfl(n, (int)i), crc_i = __shfl(crc, (int)i);
                const uint32_t slab_i = __shfl(slab, (int)i);
                const uint64_t end_i = __shfl(endw, (int)i);
                // the reader went past the window's end (it reads zeros there), or stopped on an error within reach of it
                const bool ran_off = end_i > wbits || (st_i && end_i + 64 > wbits);
                if (ran_off && !final && wbits - rel < DS_BLOCK_BOUND * 8) {
                    stop = DS_STOP_WITHHELD;
                    break;
                }
                if (st_i & BZX_ST_DC_RANDOMISED) {
                    stop = DS_STOP_ERROR;
                    err = DC_WHY_RANDOMISED;
                    break;
                }
                if (st_i || ran_off || n_i > 100000u * level) {
                    stop = DS_STOP_ERROR;
                    err = DC_WHY_DAMAGED;
                    break;
                }
                if (lane == i) mine_on_chain = true;
                if (lane == 0) chain[nch] = slab_i;
                if (lane == 0 && meta) meta[nch] = level | (streams << 4);      // (the index: bzx_ds_index_kernel)
                nch++;
                comb = crc_fold(comb, crc_i);                             // stored CRCs
                at_bit = base_bit + end_i;
            } else {
                const uint64_t after = (rel + 80 + 7) / 8;                // first byte behind the footer
                if (!final && after + 14 > wlen) {                        // is it a stream header?  not known yet
                    stop = DS_STOP_WITHHELD;
                    break;
                }
                if (rel + 80 > wbits) {
                    stop = DS_STOP_ERROR;
                    err = DC_WHY_TRUNC_EOS;
                    break;
                }
                const uint64_t fb = (rel + 48) >> 3;
                uint64_t fv = 0;
                for (uint32_t q = 0; q < 5; q++) fv = (fv << 8) | ds_byte(z, wlen, fb + q);
                const uint32_t stored = (uint32_t)((fv << ((rel + 48) & 7u)) >> 8);
                if (stored != comb) {
                    stop = DS_STOP_ERROR;
                    err = DC_WHY_COMBINED_CRC;
                    break;
                }
                streams++;
                comb = 0;
                const uint32_t next = after + 14 <= wlen ? bzx_bzh_level(z + after) : 0u;
                if (next) {
                    level = next;
                    at_bit = base_bit + after * 8 + 32;
                } else {
                    at_bit = base_bit + after * 8;
                    stop = DS_STOP_END;
                }
            }
        }
        if (isblk && !mine_on_chain) B.blk[slab].status = st | DC_SKIP;
        nblk_before += (uint32_t)__popcll(blks);
    }
    if (lane == 0) {
        DsRec r;
        r.chain_bit = at_bit;
        r.bytes = 0;
        r.good_bytes = 0;
        r.nchain = nch;
        r.streams = streams;
        r.comb = comb;
        r.level = level;
        r.stop = stop;
        r.err = err;
        r.pass_j0 = 0;
        r.placed = 0;
        r.lay_err = 0;
        r.good = 0;
        *rec = r;
    }
}

// ---- layout of a pass: one wave ------------------------------------------------------------------------------------
// Chain blocks rec->placed .. of the round get their places in the staging area, in stream order, until one does not
// fit or failed its inverse BWT; every other block of the round gets no place (the expansion skips it).
__global__ __launch_bounds__(64) void bzx_ds_layout_kernel(BzxBatch B, const uint32_t *__restrict__ chain,
                                                          uint8_t *stage, uint64_t stage_cap,
                                                          BzxDcDst *__restrict__ dst, DsRec *__restrict__ rec)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t nch = rec->nchain, j0 = rec->placed;
    for (uint32_t b = lane; b < B.nblk; b += 64) dst[b] = BzxDcDst{nullptr, 0};
    __syncthreads();                                   // the places below are written after every "no place"
    uint64_t off = 0;
    uint32_t placed = j0, lay_err = 0;
    bool stop = false;
    for (uint32_t base = j0; base < nch && !stop; base += 64) {
        const uint32_t j = base + lane;
        const bool valid = j < nch;
        const uint32_t b = valid ? chain[j] : 0u;
        const uint64_t size = valid ? B.blk[b].pack_word : 0ull;
        const uint32_t bad = (valid && B.blk[b].status) ? 1u : 0u;
        const uint64_t x = bzx_wave_incl_sum64(size);  // inclusive scan of the expanded sizes over the wave
        const bool fits = valid && !bad && off + x <= stage_cap;
        const unsigned long long nf = __ballot(valid && !fits);
        const uint32_t cnt = nch - base < 64u ? nch - base : 64u;
        const uint32_t first = nf ? (uint32_t)__ffsll(nf) - 1u : 64u;
        const uint32_t take = first < cnt ? first : cnt;
        if (lane < take) dst[b] = BzxDcDst{stage + off + (x - size), size};
        const uint64_t gx = __shfl(x, (int)(take ? take - 1u : 0u));
        const uint32_t bad_next = __shfl(bad, (int)(take < 64u ? take : 0u));
        if (take) off += gx;
        placed += take;
        if (take < cnt) {
            stop = true;
            lay_err = bad_next;
        }
    }
    if (lane == 0) {
        rec->pass_j0 = j0;
        rec->placed = placed;
        rec->bytes = off;
        rec->lay_err = lay_err;
    }
}

// ---- verdict of a pass: computed against stored block CRCs, one wave -------------------------------------------------
__global__ __launch_bounds__(64) void bzx_ds_verdict_kernel(BzxBatch B, const uint32_t *__restrict__ chain,
                                                           const BzxDcDst *__restrict__ dst,
                                                           const uint32_t *__restrict__ got, const uint8_t *stage,
                                                           DsRec *__restrict__ rec)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t j0 = rec->pass_j0, j1 = rec->placed;
    uint32_t good = j1 - j0;
    uint64_t good_bytes = rec->bytes;
    for (uint32_t base = j0; base < j1; base += 64) {
        const uint32_t j = base + lane;
        const bool valid = j < j1;
        const uint32_t b = valid ? chain[j] : 0u;
        const bool bad = valid && got[b] != B.blk[b].crc;
        const unsigned long long m = __ballot(bad);
        if (m) {
            const uint32_t f = base + (uint32_t)__ffsll(m) - 1u;
            good = f - j0;
            good_bytes = (uint64_t)(dst[chain[f]].p - stage);
            break;
        }
    }
    if (lane == 0) {
        rec->good = good;
        rec->good_bytes = good_bytes;
    }
}

// ---- the index: what an entry needs of the chain blocks a pass placed, next to the pass's record ----------------------
struct DsIxRec {
    uint64_t bit;                  // the block's magic, bit of the whole input
    uint32_t out_len, crc;         // expanded length, stored CRC
    uint32_t img_bits;             // from the magic to the bit behind the last symbol
    uint32_t meta;                 // level | streams finished in the round before the block << 4
};

__global__ __launch_bounds__(64) void bzx_ds_index_kernel(BzxBatch B, const uint32_t *__restrict__ chain,
                                                         const uint32_t *__restrict__ meta, uint64_t base_bit,
                                                         const DsRec *__restrict__ rec, DsIxRec *__restrict__ out,
                                                         const uint32_t *__restrict__ rec_cnt, uint32_t *__restrict__ cnt_out)
{
    const uint32_t j0 = rec->pass_j0, j1 = rec->placed;
    for (uint32_t j = j0 + threadIdx.x; j < j1; j += 64) {
        const BzxBlock &d = B.blk[chain[j]];
        if (rec_cnt) cnt_out[j - j0] = rec_cnt[chain[j]];    // (bzx_index_count_records: the block's delimiters)
        DsIxRec r;
        r.bit = base_bit + d.out_bit;
        r.out_len = (uint32_t)d.pack_word;
        r.crc = d.crc;
        r.img_bits = (uint32_t)(d.bits - d.out_bit);
        r.meta = meta[j];
        out[j - j0] = r;
    }
}

// ---- salvage (bzx_salvage_*): the walk that goes on after a break ---------------------------------------------------------
// The rule is in include/bzx.h.  A round decodes its block candidates as every mode does; then
//   bzx_sv_trial_kernel    sorts them into classes: a candidate that decoded is a TRIAL and goes, in input order, into the
//                          list the layout places (d_chain); the others (structure, randomised, withheld) get the skip
//                          status.  No candidate is dropped by position here: whether it lies inside an accepted block is
//                          known behind the CRCs only.  The price: trials behind a withheld candidate, or inside a block
//                          the walk then accepts, go through inverse BWT, expansion and CRC for nothing, and the former
//                          are decoded again with the next window.  That is nothing on a clean input and multiplies the
//                          work on heavy damage fed in small windows; cutting the list at the first withheld candidate
//                          would need a class "not looked at yet" and a round that ends early, and is not built.
//   inverse BWT            unchanged; a trial it refuses keeps a status and gets no place (bzx_sv_layout_kernel skips it,
//                          where bzx_ds_layout_kernel ends the pass)
//   per pass               layout, expansion, CRCs as in the index mode, then bzx_sv_verdict_kernel (a verdict per placed
//                          trial) and bzx_sv_walk_kernel: one lane takes the walk's state (DsSvState, a kernel argument;
//                          the host keeps it between passes and windows and never looks into the window) over the round's
//                          candidates up to the first trial that has no verdict yet, and leaves entries, closed gaps and
//                          the new state in tables of fixed size that travel back with the record.   [1 synchronisation]
// st.P is the bit behind the last accepted block or footer (where a gap opens), st.S the first bit not examined yet
// (where the next window's carry starts): S runs ahead of P over failed candidates and over input that holds no magic,
// so the carry stays below DS_CARRY_MAX however long the damage is.  Both keep the last 47 bits of a window, in which a
// magic may straddle into the next.
enum { SV_EOS = 0, SV_TRIAL, SV_WITHHOLD, SV_FAIL_STRUCTURE, SV_FAIL_RANDOMISED };     // DsSvCand.cls
enum { SV_PENDING = 0, SV_GOOD, SV_BAD_CRC, SV_BAD_IBWT };                             // verdict of a trial

struct DsSvCand {                  // one candidate of the round
    uint32_t slab;                 // host: slab of a block candidate
    uint32_t cls;                  // trial kernel: SV_*
    uint32_t trial;                // trial kernel: its place in the trial list (cls == SV_TRIAL)
    uint32_t pad_;
};

struct DsSvEnt {                   // an accepted block, as the host appends it
    uint64_t bit, out_off;
    uint32_t out_len, crc, img_bits, stream, level, pad_;
};

struct DsSvState {
    uint64_t P, S;                 // see above (bits of the whole input)
    uint64_t out_off;              // bytes of the entries so far
    bzx_gap gap;                   // the open gap (gap_open), bit_hi not yet known
    uint32_t gap_open;
    uint32_t level;
    uint32_t between;              // behind a footer that no header followed
    uint32_t clean;                // the stream's header was read and no gap was opened or recorded since
    uint32_t comb;                 // fold of the stream's entry CRCs
    uint32_t streams;              // end-of-stream markers passed
    uint32_t k;                    // candidates of the round the walk is through (between the passes of a round)
    uint32_t pad_;
};

struct DsSvRec {                   // what the host reads of a salvage pass
    DsSvState st;                  // walk
    uint64_t bytes;                // layout: bytes placed in the staging area
    uint32_t ntrial;               // trial kernel: trials of the round
    uint32_t pass_j0, placed;      // layout: first trial of this pass, trials placed or skipped so far
    uint32_t nent, ngap;           // walk: entries and closed gaps of this pass
    uint32_t stop;                 // walk: DS_STOP_GO or DS_STOP_WITHHELD
    uint32_t round_done;           // walk: through all candidates of the round (or withheld)
    uint32_t pad_;
};

// cand[c0, c1): the round's candidates; svc[k - c0].slab: where block candidate k was decoded.
__global__ __launch_bounds__(64) void bzx_sv_trial_kernel(BzxBatch B, uint64_t wlen, uint64_t base_bit, uint32_t final,
                                                         const uint64_t *__restrict__ cand, uint32_t c0, uint32_t c1,
                                                         DsSvCand *__restrict__ svc, uint32_t *__restrict__ trials,
                                                         uint32_t *__restrict__ verdict, DsSvRec *__restrict__ rec)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t wbits = wlen * 8;
    uint32_t nt = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t k = base + lane;
        const bool valid = k < c1;
        const uint64_t pos = valid ? cand[k] : 1ull;
        uint32_t cls = SV_EOS, slab = 0;
        if (valid && !(pos & 1u)) {
            slab = svc[k - c0].slab;
            const uint32_t st = B.blk[slab].status;
            const uint64_t end = B.blk[slab].bits, rel = (pos >> 1) - base_bit;
            // the reader went past the window's end (it reads zeros there), or stopped on an error within reach of it
            const bool ran_off = end > wbits || (st && end + 64 > wbits);
            if (ran_off && !final && wbits - rel < DS_BLOCK_BOUND * 8) cls = SV_WITHHOLD;
            else if (st & BZX_ST_DC_RANDOMISED) cls = SV_FAIL_RANDOMISED;
            else if (st || ran_off) cls = SV_FAIL_STRUCTURE;
            else cls = SV_TRIAL;
            if (cls != SV_TRIAL) B.blk[slab].status = st | DC_SKIP;
        }
        const unsigned long long m = __ballot(cls == SV_TRIAL);
        const uint32_t t = nt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (cls == SV_TRIAL) {
            trials[t] = slab;
            verdict[t] = SV_PENDING;
        }
        if (valid) {
            svc[k - c0].cls = cls;
            svc[k - c0].trial = t;
        }
        nt += (uint32_t)__popcll(m);
    }
    if (lane == 0) {
        rec->ntrial = nt;
        rec->pass_j0 = 0;
        rec->placed = 0;
        rec->bytes = 0;
    }
}

// bzx_ds_layout_kernel over the trial list, except that a trial the inverse BWT refused takes no room and does not end
// the pass.
__global__ __launch_bounds__(64) void bzx_sv_layout_kernel(BzxBatch B, const uint32_t *__restrict__ trials, uint8_t *stage,
                                                          uint64_t stage_cap, BzxDcDst *__restrict__ dst,
                                                          DsSvRec *__restrict__ rec)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t nt = rec->ntrial, j0 = rec->placed;
    for (uint32_t b = lane; b < B.nblk; b += 64) dst[b] = BzxDcDst{nullptr, 0};
    __syncthreads();                                   // the places below are written after every "no place"
    uint64_t off = 0;
    uint32_t placed = j0;
    bool stop = false;
    for (uint32_t base = j0; base < nt && !stop; base += 64) {
        const uint32_t j = base + lane;
        const bool valid = j < nt;
        const uint32_t b = valid ? trials[j] : 0u;
        const bool bad = valid && B.blk[b].status;
        const uint64_t size = valid && !bad ? B.blk[b].pack_word : 0ull;
        const uint64_t x = bzx_wave_incl_sum64(size);
        const bool fits = valid && off + x <= stage_cap;
        const unsigned long long nf = __ballot(valid && !fits);
        const uint32_t cnt = nt - base < 64u ? nt - base : 64u;
        const uint32_t first = nf ? (uint32_t)__ffsll(nf) - 1u : 64u;
        const uint32_t take = first < cnt ? first : cnt;
        if (lane < take && !bad) dst[b] = BzxDcDst{stage + off + (x - size), size};
        const uint64_t gx = __shfl(x, (int)(take ? take - 1u : 0u));
        if (take) off += gx;
        placed += take;
        if (take < cnt) stop = true;
    }
    if (lane == 0) {
        rec->pass_j0 = j0;
        rec->placed = placed;
        rec->bytes = off;
    }
}

__global__ __launch_bounds__(64) void bzx_sv_verdict_kernel(BzxBatch B, const uint32_t *__restrict__ trials,
                                                           const uint32_t *__restrict__ got, uint32_t *__restrict__ verdict,
                                                           const DsSvRec *__restrict__ rec)
{
    const uint32_t j1 = rec->placed;
    for (uint32_t j = rec->pass_j0 + threadIdx.x; j < j1; j += 64) {
        const uint32_t b = trials[j];
        verdict[j] = B.blk[b].status ? SV_BAD_IBWT : got[b] == B.blk[b].crc ? SV_GOOD : SV_BAD_CRC;
    }
}

// ent[R], gaps[2 R]: a round has at most R block candidates and R end-of-stream candidates (the host cuts it so), and a
// candidate closes or records at most one gap (a marker records COMBINED_CRC only where it had no other gap to settle).
__global__ __launch_bounds__(64) void bzx_sv_walk_kernel(BzxBatch B, const uint8_t *__restrict__ z, uint64_t wlen,
                                                        uint64_t base_bit, uint32_t final,
                                                        const uint64_t *__restrict__ cand, uint32_t c0, uint32_t c1,
                                                        const DsSvCand *__restrict__ svc,
                                                        const uint32_t *__restrict__ verdict, DsSvState st,
                                                        DsSvEnt *__restrict__ ent, bzx_gap *__restrict__ gaps,
                                                        DsSvRec *__restrict__ rec)
{
    if (threadIdx.x) return;
    const uint64_t wbits = wlen * 8;
    const uint32_t placed = rec->placed;
    uint32_t nent = 0, ngap = 0, stop = DS_STOP_GO;
    // an accepted block or a marker at bit b: the open gap closes there, or what lies between P and b is one
    auto settle = [&](uint64_t b) {
        if (st.gap_open) {
            st.gap.bit_hi = b;
            gaps[ngap++] = st.gap;
            st.gap_open = 0;
        } else if (b > st.P) {
            gaps[ngap++] = bzx_gap{st.P, b, st.out_off, 0u, BZX_GAP_NO_MAGIC | (st.between ? BZX_GAP_HEADER : 0u)};
            st.clean = 0;
        }
    };
    uint32_t k = st.k;
    for (; c0 + k < c1; k++) {
        const uint64_t pos = cand[c0 + k];
        const uint64_t bit = pos >> 1, rel = bit - base_bit;
        if (bit < st.S) continue;                                         // inside an accepted block or a footer
        if (pos & 1u) {
            const uint64_t after = (rel + 80 + 7) / 8;                    // first byte behind the footer
            if (!final && after + 14 > wlen) {                            // is it a stream header?  not known yet
                st.S = bit;
                stop = DS_STOP_WITHHELD;
                break;
            }
            if (rel + 80 > wbits) continue;                               // cut off by the end of the input: not there
            settle(bit);
            if (st.clean) {
                const uint64_t fb = (rel + 48) >> 3;
                uint64_t fv = 0;
                for (uint32_t q = 0; q < 5; q++) fv = (fv << 8) | ds_byte(z, wlen, fb + q);
                const uint32_t stored = (uint32_t)((fv << ((rel + 48) & 7u)) >> 8);
                if (stored != st.comb) gaps[ngap++] = bzx_gap{bit, bit, st.out_off, 0u, BZX_GAP_COMBINED_CRC};
            }
            st.streams++;
            st.comb = 0;
            const uint32_t next = after + 14 <= wlen ? bzx_bzh_level(z + after) : 0u;
            st.level = next ? next : 9u;
            st.between = next ? 0u : 1u;
            st.clean = next ? 1u : 0u;
            st.P = st.S = base_bit + after * 8 + (next ? 32u : 0u);
            continue;
        }
        const DsSvCand c = svc[k];
        if (c.cls == SV_WITHHOLD) {                                       // more input may complete it
            st.S = bit;
            stop = DS_STOP_WITHHELD;
            break;
        }
        uint32_t why = c.cls == SV_FAIL_RANDOMISED ? BZX_GAP_RANDOMISED : BZX_GAP_STRUCTURE;
        if (c.cls == SV_TRIAL) {
            if (c.trial >= placed) break;                                 // its verdict comes with a later pass
            const uint32_t v = verdict[c.trial];
            const BzxBlock &d = B.blk[c.slab];
            if (v == SV_GOOD && d.n <= 100000u * st.level) {
                settle(bit);
                DsSvEnt e;
                e.bit = bit;
                e.out_off = st.out_off;
                e.out_len = (uint32_t)d.pack_word;
                e.crc = d.crc;
                e.img_bits = (uint32_t)(d.bits - d.out_bit);
                e.stream = st.streams;
                e.level = st.level;
                e.pad_ = 0;
                ent[nent++] = e;
                st.out_off += e.out_len;
                st.comb = crc_fold(st.comb, d.crc);
                st.between = 0;
                st.P = st.S = bit + e.img_bits;
                continue;
            }
            why = v == SV_BAD_CRC && d.n <= 100000u * st.level ? BZX_GAP_BLOCK_CRC : BZX_GAP_STRUCTURE;
        }
        if (!st.gap_open) {
            st.gap = bzx_gap{st.P, 0, st.out_off, 0u, st.between ? BZX_GAP_HEADER : 0u};
            st.gap_open = 1;
            st.clean = 0;
        }
        st.gap.why |= why;
        st.gap.candidates++;
        st.S = bit + 1;
    }
    const uint32_t round_done = (c0 + k >= c1 || stop != DS_STOP_GO) ? 1u : 0u;
    st.k = round_done ? 0u : k;
    rec->st = st;
    rec->nent = nent;
    rec->ngap = ngap;
    rec->stop = stop;
    rec->round_done = round_done;
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct bzx_index {
    bzx_dstream *s = nullptr;
    std::vector<bzx_index_entry> entries;
    std::vector<bzx_gap> gaps;                             // (salvage)
    std::vector<uint64_t> rec;                             // (bzx_index_count_records) delimiters before every entry, and T
    std::vector<uint64_t> hits;                            // (bzx_index_find) the first max_hits hits, ascending
    uint64_t hit_total = 0;                                // ... and how many there are
    std::vector<uint64_t> lines;                           // (bzx_index_find_lines) lines[i] = delimiters of D before hits[i]
    bool fed = false;                                      // bzx_index_feed has been called
};

struct DsSlot {                    // an output staging area: the verified bytes of one pass
    uint64_t bytes = 0, off = 0;   // bytes of the pass, bytes of them delivered
    bool arrived = false;          // its copy-back has been awaited
};

enum DsMode { DS_STREAM, DS_INDEX, DS_SALVAGE };         // set once, in ds_begin

struct bzx_dstream {
    bzx_ctx *ctx = nullptr;
    DsMode mode = DS_STREAM;
    size_t max_chunk = 0, in_cap = 0;
    uint32_t cap_cand = 0, R = 0;
    DevMem<uint8_t> d_in[2], d_stage[2];
    PinMem<uint8_t> h_stage[2];
    DevMem<uint64_t> d_cand;
    PinMem<uint64_t> h_cand;                               // h_cand[cap_cand]: the window's candidates, sorted
    DevMem<uint32_t> d_ncand;
    PinMem<uint32_t> h_ncand;
    DevMem<BzxDcSrc> d_src;
    PinMem<BzxDcSrc> h_src;
    DevMem<BzxDcDst> d_dst;
    DevMem<uint32_t> d_chain, d_got;
    DevMem<DsRec> d_rec;
    PinMem<DsRec> h_rec;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_h2d = nullptr, ev_carry = nullptr, ev_d2h[2] = {nullptr, nullptr};
    // input
    uint32_t acc = 0;                  // the input buffer that accepts bytes (the other one holds the window)
    size_t acc_fill = 0;
    uint8_t head[4] = {0, 0, 0, 0};    // first bytes of the input (stream header)
    bool final_seen = false;
    // window
    bool have_win = false, wfinal = false, need_more = false, need_scan = false;
    uint8_t *wptr = nullptr;
    uint64_t wlen = 0, wbase = 0;      // its length, and the offset of its first byte in the whole input
    uint64_t scan_to = 0;              // window bytes [.., scan_to) have been scanned
    uint32_t ncand = 0, ci = 0;        // candidates, and the first one no round has taken
    // chain
    bool started = false;
    uint64_t chain_bit = 0;
    uint32_t comb = 0, level = 0;
    // round
    bool rd_active = false;            // the slabs hold chain blocks that have not been placed yet
    uint32_t rd_nb = 0, rd_c0 = 0, rd_c1 = 0;      // its blocks (slabs), its candidates [rd_c0, rd_c1)
    DsRec rd = {};                     // the chain part of the round's record (DS_STREAM, DS_INDEX)
    // output: passes in flight or being delivered, oldest first
    DsSlot slot[2];
    uint32_t q_head = 0, q_n = 0;
    // verdict
    bool finished = false, done = false;
    int pend_rc = 0, err_rc = 0;       // an error waits behind the verified bytes still to be delivered / is raised
    std::string pend_text, err_text;
    bzx_dstream_info info = {};
    float ms = 0.f;
    // DS_INDEX (bzx_index_*): nothing is copied back or handed out; the placed blocks' figures come with the record
    bzx_index *ix = nullptr;           // where entries and gaps go (DS_INDEX, DS_SALVAGE)
    DevMem<uint32_t> d_meta;
    DevMem<DsIxRec> d_ix;
    PinMem<DsIxRec> h_ix;
    // ... with bzx_index_count_records: one count per slab, and behind the nb records of a pass's copy its nb counts
    int rec_delim = -1;
    DevMem<uint32_t> d_rcnt;
    // ... with bzx_index_find: a BzxFindOut in front of the pass's records in d_ix / h_ix (find_off bytes of both), the
    // sections' counts, one emit window, and the last m - 1 verified bytes, in which the next pass's straddling hits start
    bool find_on = false;
    size_t find_off = 0;
    BzxFindPat find_pat = {};
    uint64_t find_max = 0;
    uint32_t find_inline = 0;          // room of the pass's inline emit
    DevMem<uint32_t> d_fsec, d_fwin;
    PinMem<uint32_t> h_fwin;
    std::vector<uint8_t> find_carry;
    // ... with bzx_index_find_lines: a BzxFindLines behind the BzxFindOut (find_off covers both), the sections' delimiter
    // counts, a second emit window, and the delimiters of the passes digested so far
    int lines_delim = -1;
    uint64_t dbase = 0;
    DevMem<uint32_t> d_dsec, d_lwin;
    PinMem<uint32_t> h_lwin;
    // DS_SALVAGE (bzx_salvage_*): the index mode's memory, with the tables of the salvage kernels in place of d_meta / d_ix
    DsSvState sv = {};                 // the walk's state between passes and windows
    DevMem<DsSvCand> d_svc;
    PinMem<DsSvCand> h_svc;
    DevMem<uint32_t> d_verdict;
    DevMem<DsSvEnt> d_ent;
    PinMem<DsSvEnt> h_ent;
    DevMem<bzx_gap> d_gap;
    PinMem<bzx_gap> h_gap;
    DevMem<DsSvRec> d_svrec;
    PinMem<DsSvRec> h_svrec;
};

extern "C" void bzx_dstream_end(bzx_dstream *s)
{
    if (!s) return;
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_;
    if (ctx) {
        api_lock_ = std::unique_lock<std::recursive_mutex>(ctx->api_mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (s->s_h2d) (void)hipStreamSynchronize(s->s_h2d);
    if (s->s_d2h) (void)hipStreamSynchronize(s->s_d2h);
    // (the device is current and the three streams are idle: `delete` below frees every buffer the stream owns)
    for (int i = 0; i < 2; i++)
        if (s->ev_d2h[i]) (void)hipEventDestroy(s->ev_d2h[i]);
    if (s->ev_h2d) (void)hipEventDestroy(s->ev_h2d);
    if (s->ev_carry) (void)hipEventDestroy(s->ev_carry);
    if (s->s_h2d) (void)hipStreamDestroy(s->s_h2d);
    if (s->s_d2h) (void)hipStreamDestroy(s->s_d2h);
    if (ctx && ctx->ds == s) ctx->ds = nullptr;
    delete s;
}

// DS_INDEX, DS_SALVAGE: the stream of a bzx_index -- one output staging area, none on the host, and the mode's tables.
static int ds_begin(bzx_ctx *ctx, size_t max_chunk, DsMode mode, bzx_dstream **out)
{
    const bool index = mode != DS_STREAM;
    if (!ctx || !out) return BZX_E_PARAM;
    *out = nullptr;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (max_chunk == 0) max_chunk = DS_DEF_CHUNK;
    if (max_chunk < DS_MIN_CHUNK) max_chunk = DS_MIN_CHUNK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, ctx->cap_slabs ? ctx->cap_slabs : 16);
    if (rc) return rc;
    bzx_dstream *s = new (std::nothrow) bzx_dstream();
    if (!s) return BZX_E_NOMEM;
    s->ctx = ctx;
    s->mode = mode;
    s->max_chunk = max_chunk;
    s->R = ctx->cap_slabs;
    s->in_cap = DS_CARRY_MAX + max_chunk + 64;
    s->cap_cand = (uint32_t)std::min<size_t>(s->in_cap / 256 + 1024, 0x7fffffffu);
    const size_t R = s->R;
    uint64_t dev = 0, pin = 0;
    auto dmal = [&](auto &m, size_t n) {
        dev += n;
        return m.reserve(n);
    };
    auto hmal = [&](auto &m, size_t n) {
        pin += n;
        return m.reserve(n);
    };
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++)
        ok = dmal(s->d_in[i], s->in_cap) && (index && i ? true : dmal(s->d_stage[i], DS_STAGE_BYTES)) &&
             (index || hmal(s->h_stage[i], DS_STAGE_BYTES)) &&
             hipEventCreateWithFlags(&s->ev_d2h[i], hipEventDisableTiming) == hipSuccess;
    if (mode == DS_SALVAGE)                                  // (zeroed as d_ix below)
        ok = ok && dmal(s->d_svc, 2 * R * sizeof(DsSvCand)) && hmal(s->h_svc, 2 * R * sizeof(DsSvCand)) &&
             dmal(s->d_verdict, R * 4) && dmal(s->d_ent, R * sizeof(DsSvEnt)) && hmal(s->h_ent, R * sizeof(DsSvEnt)) &&
             dmal(s->d_gap, 2 * R * sizeof(bzx_gap)) && hmal(s->h_gap, 2 * R * sizeof(bzx_gap)) &&
             dmal(s->d_svrec, sizeof(DsSvRec)) && hmal(s->h_svrec, sizeof(DsSvRec)) &&
             hipMemset(s->d_ent, 0, R * sizeof(DsSvEnt)) == hipSuccess &&
             hipMemset(s->d_gap, 0, 2 * R * sizeof(bzx_gap)) == hipSuccess;
    else if (index)                                          // (zeroed: a pass copies the whole R-entry table back and
        ok = ok && dmal(s->d_meta, R * 4) &&       // writes the entries of the blocks it placed only)
             dmal(s->d_ix, R * sizeof(DsIxRec)) && hmal(s->h_ix, R * sizeof(DsIxRec)) &&
             hipMemset(s->d_ix, 0, R * sizeof(DsIxRec)) == hipSuccess;
    ok = ok && dmal(s->d_cand, (size_t)s->cap_cand * 8) && hmal(s->h_cand, (size_t)s->cap_cand * 8) &&
         dmal(s->d_ncand, 64) && hmal(s->h_ncand, 64) && dmal(s->d_src, R * sizeof(BzxDcSrc)) &&
         hmal(s->h_src, R * sizeof(BzxDcSrc)) && dmal(s->d_dst, R * sizeof(BzxDcDst)) &&
         dmal(s->d_chain, R * 4) && dmal(s->d_got, R * 4) && dmal(s->d_rec, sizeof(DsRec)) &&
         hmal(s->h_rec, sizeof(DsRec)) && hipEventCreateWithFlags(&s->ev_h2d, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&s->ev_carry, hipEventDisableTiming) == hipSuccess &&
         hipStreamCreateWithFlags(&s->s_h2d, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&s->s_d2h, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        s->ctx = nullptr;                      // (the lock is held here)
        bzx_dstream_end(s);
        ctx->err = "bzx_dstream_begin: device or pinned allocation failed";
        return BZX_E_NOMEM;
    }
    s->info.slabs = s->R;
    s->info.device_bytes = dev;
    s->info.pinned_bytes = pin;
    ctx->ds = s;
    *out = s;
    return BZX_OK;
}

extern "C" int bzx_dstream_begin(bzx_ctx *ctx, size_t max_chunk, bzx_dstream **out)
{
    return ds_begin(ctx, max_chunk, DS_STREAM, out);
}

extern "C" int bzx_dstream_get_info(const bzx_dstream *s, bzx_dstream_info *out)
{
    if (!s || !out || !s->ctx) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(s->ctx->api_mu);
    *out = s->info;
    out->slabs = s->ctx->cap_slabs;
    return BZX_OK;
}

static void ds_fail(bzx_dstream *s, const std::string &why)
{
    s->pend_rc = BZX_E_DATA;
    s->pend_text = why;
    s->rd_active = false;
}

// Scans the window from the chain position on; a full table halves the range and scans again.
static int ds_scan(bzx_dstream *s)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t from = s->chain_bit / 8 - s->wbase;
    uint64_t to = s->wlen;
    for (;;) {
        HIP_TRY(ctx, hipMemsetAsync(s->d_ncand, 0, 4, st));
        if (to > from) {
            const uint64_t nwords = (to - from + 3) / 4, g = (uint64_t)ctx->n_cu * 8;
            const uint64_t need = (nwords + 255) / 256;
            hipLaunchKernelGGL(bzx_ds_scan_kernel, dim3((uint32_t)(need < g ? need : g)), dim3(256), 0, st, s->wptr, s->wlen,
                               from, to, s->wbase * 8, s->d_cand.get(), s->d_ncand.get(), s->cap_cand);
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemcpyAsync(s->h_ncand, s->d_ncand, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(s->h_cand, s->d_cand, (size_t)s->cap_cand * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));              // the scan's synchronisation
        s->info.scans++;
        if (*s->h_ncand <= s->cap_cand) break;
        to = from + (to - from) / 2;                         // (cap_cand >= 1024 magics of 6 bytes: ends above 6 KiB)
    }
    s->ncand = *s->h_ncand;
    std::sort(s->h_cand.get(), s->h_cand + s->ncand);
    if (s->ncand) HIP_TRY(ctx, hipMemcpyAsync(s->d_cand, s->h_cand, (size_t)s->ncand * 8, hipMemcpyHostToDevice, st));
    s->scan_to = to;
    s->ci = 0;
    s->need_scan = false;
    return BZX_OK;
}

// The chain found no magic where it stands (or the candidates are used up).
static void ds_no_magic(bzx_dstream *s, bool used_up)
{
    const uint64_t rel = s->chain_bit - s->wbase * 8;
    if (used_up && s->scan_to < s->wlen && rel >= s->scan_to * 8) {
        s->need_scan = true;                                 // the rest of a window whose scan was cut short
        return;
    }
    if (rel + 48 > s->wlen * 8 && !s->wfinal) s->need_more = true;
    else ds_fail(s, dc_why_text(DC_WHY_NO_EOS));
}

static void ds_round_complete(bzx_dstream *s)
{
    const DsRec &r = s->rd;
    s->rd_active = false;
    s->chain_bit = r.chain_bit;
    s->comb = r.comb;
    s->level = r.level;
    s->info.nstreams += r.streams;
    switch (r.stop) {
    case DS_STOP_GO:
        break;
    case DS_STOP_NOMAGIC:
        ds_no_magic(s, false);
        break;
    case DS_STOP_WITHHELD:
        s->need_more = true;
        break;
    case DS_STOP_END:
        s->finished = true;
        break;
    default:
        ds_fail(s, dc_why_text(r.err));
    }
}

// Salvage: the candidates of the window are used up: the rest of a window whose scan was cut short, the next window, or -- behind
// the last byte of the input -- the end of the walk.
static void sv_used_up(bzx_dstream *s)
{
    DsSvState &v = s->sv;
    if (s->scan_to < s->wlen) {                              // (the scan finds every magic that starts before scan_to)
        v.S = std::max(v.S, (s->wbase + s->scan_to) * 8);
        s->chain_bit = v.S;
        s->need_scan = true;
        return;
    }
    const uint64_t end = (s->wbase + s->wlen) * 8;
    if (!s->wfinal) {                                        // a magic may start in the last 47 bits
        if (end >= 47) v.S = std::max(v.S, end - 47);
        s->chain_bit = v.S;
        s->need_more = true;
        return;
    }
    if (v.gap_open) {
        v.gap.bit_hi = end;
        if (!v.between) v.gap.why |= BZX_GAP_TRUNCATED;
        s->ix->gaps.push_back(v.gap);
        v.gap_open = 0;
    } else if (!v.between) {
        s->ix->gaps.push_back(bzx_gap{v.P, end, v.out_off, 0u, BZX_GAP_TRUNCATED});
    }
    s->finished = true;
}

// ---- what a mode contributes to a pass: its kernels, its copies back, the digest of its record ------------------------
static bzx_index_entry ds_entry(uint64_t bit, uint64_t out_off, uint32_t out_len, uint32_t crc, uint32_t img_bits,
                                uint32_t stream, uint32_t level)
{
    bzx_index_entry e;
    memset(&e, 0, sizeof(e));
    e.bit = bit;
    e.out_off = out_off;
    e.out_len = out_len;
    e.crc = crc;
    e.img_bits = img_bits;
    e.stream = stream;
    e.level = (uint8_t)level;
    return e;
}

// Behind the decode of a new round: the chain walk from the carried bit, or (salvage) every candidate into its class.
static void ds_launch_chain(bzx_dstream *s)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t final = s->wfinal ? 1u : 0u;
    if (s->mode == DS_SALVAGE)
        hipLaunchKernelGGL(bzx_sv_trial_kernel, dim3(1), dim3(64), 0, st, ctx->B, s->wlen, s->wbase * 8, final, s->d_cand.get(),
                           s->rd_c0, s->rd_c1, s->d_svc.get(), s->d_chain.get(), s->d_verdict.get(), s->d_svrec.get());
    else
        hipLaunchKernelGGL(bzx_ds_chain_kernel, dim3(1), dim3(64), 0, st, ctx->B, s->wptr, s->wlen, s->wbase * 8, final,
                           s->d_cand.get(), s->rd_c0, s->rd_c1, s->chain_bit, s->comb, s->level, s->d_chain.get(), s->d_rec.get(),
                           s->d_meta.get());
}

static void ds_launch_layout(bzx_dstream *s, uint32_t q)
{
    bzx_ctx *ctx = s->ctx;
    if (s->mode == DS_SALVAGE)
        hipLaunchKernelGGL(bzx_sv_layout_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->B, s->d_chain.get(), s->d_stage[0].get(),
                           (uint64_t)DS_STAGE_BYTES, s->d_dst.get(), s->d_svrec.get());
    else
        hipLaunchKernelGGL(bzx_ds_layout_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->B, s->d_chain.get(), s->d_stage[q].get(),
                           (uint64_t)DS_STAGE_BYTES, s->d_dst.get(), s->d_rec.get());
}

static void ds_launch_find(bzx_dstream *s, uint32_t q);     // (bzx_index_find: below)

// Behind the CRCs of the nb blocks a pass may place: the verdict, then what the mode leaves for the host next to its
// record -- the index's entries, or the salvage walk over the round's candidates (which runs without a block too).
static int ds_launch_verdict(bzx_dstream *s, uint32_t q, uint32_t nb)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    if (s->mode == DS_SALVAGE) {
        if (nb)
            hipLaunchKernelGGL(bzx_sv_verdict_kernel, dim3(1), dim3(64), 0, st, B, s->d_chain.get(), s->d_got.get(), s->d_verdict.get(),
                               s->d_svrec.get());
        hipLaunchKernelGGL(bzx_sv_walk_kernel, dim3(1), dim3(64), 0, st, B, s->wptr, s->wlen, s->wbase * 8, s->wfinal ? 1u : 0u,
                           s->d_cand.get(), s->rd_c0, s->rd_c1, s->d_svc.get(), s->d_verdict.get(), s->sv, s->d_ent.get(), s->d_gap.get(),
                           s->d_svrec.get());
        return BZX_OK;
    }
    if (!nb) return BZX_OK;
    hipLaunchKernelGGL(bzx_ds_verdict_kernel, dim3(1), dim3(64), 0, st, B, s->d_chain.get(), s->d_dst.get(), s->d_got.get(), s->d_stage[q].get(),
                       s->d_rec.get());
    if (s->mode == DS_INDEX) {
        const bool counting = s->rec_delim >= 0;
        DsIxRec *tab = reinterpret_cast<DsIxRec *>(s->d_ix.get<uint8_t>() + s->find_off);
        hipLaunchKernelGGL(bzx_ds_index_kernel, dim3(1), dim3(64), 0, st, B, s->d_chain.get(), s->d_meta.get(), s->wbase * 8, s->d_rec.get(),
                           tab, (const uint32_t *)s->d_rcnt.get(), counting ? reinterpret_cast<uint32_t *>(tab + nb) : nullptr);
        if (s->find_on) ds_launch_find(s, q);
        // (the round's share of the table; the pass wrote its first placed - pass_j0 entries, the host reads
        // r.good <= that many, the rest is what bzx_index_begin zeroed or an earlier pass left)
        HIP_TRY(ctx, hipMemcpyAsync(s->h_ix, s->d_ix, s->find_off + nb * (sizeof(DsIxRec) + (counting ? 4 : 0)), hipMemcpyDeviceToHost, st));
    }
    return BZX_OK;
}

// bzx_index_find, behind the verdict of a pass: count, scan and the emit of the first hits over the verified bytes of the
// staging area (rec->good_bytes, read on the device), all next to the pass's index records.
static void ds_launch_find(bzx_dstream *s, uint32_t q)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    BzxFindOut *fo = s->d_ix.get<BzxFindOut>();
    const uint64_t *len = &s->d_rec.get()->good_bytes;
    const uint8_t *stage = s->d_stage[q].get();
    const uint32_t grid = bzx_find_grid(DS_STAGE_BYTES, (uint32_t)ctx->n_cu);
    const uint64_t have = s->ix->hits.size();
    s->find_inline = (uint32_t)std::min<uint64_t>(FIND_INLINE_HITS, s->find_max > have ? s->find_max - have : 0);
    if (s->lines_delim >= 0) {                               // the lines forms in place of the plain ones
        BzxFindLines *fl = reinterpret_cast<BzxFindLines *>(fo + 1);
        const uint32_t delim = (uint32_t)s->lines_delim;
        bzx_launch_find_count_lines(stage, len, s->find_pat, delim, s->d_fsec.get(), s->d_dsec.get(), grid, st);
        bzx_launch_find_scan_lines(stage, len, s->find_pat.m, s->d_fsec.get(), s->d_dsec.get(), nullptr, &fo->count, &fl->dcount, fo, st);
        bzx_launch_find_emit_lines(stage, len, s->find_pat, delim, s->d_fsec.get(), s->d_dsec.get(), nullptr, &fo->count, 0,
                                   s->find_inline, fo->hits, fl->lines, grid, st);
        return;
    }
    bzx_launch_find_count(stage, len, s->find_pat, s->d_fsec.get(), grid, st);
    bzx_launch_find_scan(stage, len, s->find_pat.m, s->d_fsec.get(), nullptr, &fo->count, fo, st);
    bzx_launch_find_emit(stage, len, s->find_pat, s->d_fsec.get(), nullptr, &fo->count, 0, s->find_inline, fo->hits, grid, st);
}

// ... and behind the pass's synchronisation: the hits that straddle into the pass (found here, in the carried bytes and
// the pass's first ones: both parts are shorter than the pattern, so every match there straddles), then the pass's own
// -- the inline ones, and while the list has room the rest in windows of FIND_WINDOW_HITS, one emit launch, one copy and
// one synchronisation each (the staging bytes and the sections' sums stay until the next pass).  base: the decoded
// bytes before the pass.
// With lines on every hit comes with its line: a device hit's is dbase (the delimiters of the passes before this one)
// plus what the emit kernel left; a straddling hit's is dbase minus the delimiters in the carry at or behind its start.
static int ds_find_digest(bzx_dstream *s, uint32_t q, uint64_t base)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    bzx_index *ix = s->ix;
    const BzxFindOut &fo = *s->h_ix.get<BzxFindOut>();
    const uint32_t m = s->find_pat.m;
    const uint8_t *pat = reinterpret_cast<const uint8_t *>(s->find_pat.w);
    std::vector<uint8_t> &c = s->find_carry;
    const size_t nc = c.size();
    const bool lines = s->lines_delim >= 0;
    const BzxFindLines *fl = lines ? reinterpret_cast<const BzxFindLines *>(&fo + 1) : nullptr;
    c.insert(c.end(), fo.head, fo.head + fo.nedge);
    for (size_t i = 0; i < nc && i + m <= c.size(); i++) {
        if (memcmp(c.data() + i, pat, m)) continue;
        ix->hit_total++;
        if (ix->hits.size() >= s->find_max) continue;
        ix->hits.push_back(base - nc + i);
        if (lines) ix->lines.push_back(s->dbase - (uint64_t)std::count(c.begin() + i, c.begin() + nc, (uint8_t)s->lines_delim));
    }
    if (fo.nedge == m - 1) c.assign(fo.tail, fo.tail + fo.nedge);       // (a shorter pass extends the carry)
    else if (c.size() > m - 1) c.erase(c.begin(), c.end() - (m - 1));
    ix->hit_total += fo.count;
    uint64_t skip = std::min<uint64_t>(fo.count, s->find_inline);
    for (uint64_t i = 0; i < skip && ix->hits.size() < s->find_max; i++) {
        ix->hits.push_back(base + fo.hits[i]);
        if (lines) ix->lines.push_back(s->dbase + fl->lines[i]);
    }
    const uint32_t grid = bzx_find_grid(DS_STAGE_BYTES, (uint32_t)ctx->n_cu);
    while (skip < fo.count && ix->hits.size() < s->find_max) {
        const uint32_t cap = (uint32_t)std::min<uint64_t>(FIND_WINDOW_HITS, std::min<uint64_t>(fo.count - skip, s->find_max - ix->hits.size()));
        if (lines)
            bzx_launch_find_emit_lines(s->d_stage[q].get(), &s->d_rec.get()->good_bytes, s->find_pat, (uint32_t)s->lines_delim,
                                       s->d_fsec.get(), s->d_dsec.get(), nullptr, &s->d_ix.get<BzxFindOut>()->count, skip, cap,
                                       s->d_fwin.get(), s->d_lwin.get(), grid, st);
        else
            bzx_launch_find_emit(s->d_stage[q].get(), &s->d_rec.get()->good_bytes, s->find_pat, s->d_fsec.get(), nullptr,
                                 &s->d_ix.get<BzxFindOut>()->count, skip, cap, s->d_fwin.get(), grid, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(s->h_fwin, s->d_fwin, (size_t)cap * 4, hipMemcpyDeviceToHost, st));
        if (lines) HIP_TRY(ctx, hipMemcpyAsync(s->h_lwin, s->d_lwin, (size_t)cap * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));              // a window's synchronisation
        for (uint32_t i = 0; i < cap; i++) ix->hits.push_back(base + s->h_fwin[i]);
        for (uint32_t i = 0; lines && i < cap; i++) ix->lines.push_back(s->dbase + s->h_lwin[i]);
        skip += cap;
    }
    if (lines) s->dbase += fl->dcount;
    return BZX_OK;
}

static int ds_copy_record(bzx_dstream *s)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    if (s->mode != DS_SALVAGE) {
        HIP_TRY(ctx, hipMemcpyAsync(s->h_rec, s->d_rec, sizeof(DsRec), hipMemcpyDeviceToHost, st));
        return BZX_OK;
    }
    // (tables of fixed size: the host reads the first nent / ngap of them, the rest is what begin zeroed or a pass left)
    HIP_TRY(ctx, hipMemcpyAsync(s->h_ent, s->d_ent, (size_t)s->R * sizeof(DsSvEnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(s->h_gap, s->d_gap, (size_t)2 * s->R * sizeof(bzx_gap), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(s->h_svrec, s->d_svrec, sizeof(DsSvRec), hipMemcpyDeviceToHost, st));
    return BZX_OK;
}

// Salvage: the walk's entries and closed gaps are appended; its state says where the round and the window stand.
static int sv_digest(bzx_dstream *s)
{
    const DsSvRec &r = *s->h_svrec;
    for (uint32_t j = 0; j < r.nent; j++) {
        const DsSvEnt &x = s->h_ent[j];
        s->ix->entries.push_back(ds_entry(x.bit, x.out_off, x.out_len, x.crc, x.img_bits, x.stream, x.level));
    }
    s->ix->gaps.insert(s->ix->gaps.end(), s->h_gap.get(), s->h_gap.get() + r.ngap);
    s->sv = r.st;
    s->chain_bit = r.st.S;
    s->info.nblk += r.nent;
    s->info.out_bytes = r.st.out_off;
    s->info.nstreams = r.st.streams;
    s->rd_active = !r.round_done;
    if (r.round_done && r.stop == DS_STOP_WITHHELD) s->need_more = true;
    return BZX_OK;
}

// Stream and index: the verified blocks become entries, or their bytes start the way out of staging area `q`; the first
// block that did not verify ends the stream, the last placed block of the chain ends the round.
static int ds_digest(bzx_dstream *s, uint32_t q, bool fresh)
{
    bzx_ctx *ctx = s->ctx;
    const DsRec r = *s->h_rec;
    if (fresh) {
        s->rd = r;
        s->rd_active = true;
    }
    if (s->mode == DS_INDEX) {                               // their bytes stay
        const DsIxRec *tab = reinterpret_cast<const DsIxRec *>(s->h_ix.get<uint8_t>() + s->find_off);
        const uint32_t *cnt = reinterpret_cast<const uint32_t *>(tab + s->rd_nb);                // (counting: behind the records)
        const uint64_t pass_base = s->info.out_bytes;
        for (uint32_t j = 0; j < r.good; j++) {
            const DsIxRec &x = tab[j];
            if (s->rec_delim >= 0) s->ix->rec.push_back(s->ix->rec.back() + cnt[j]);
            s->ix->entries.push_back(ds_entry(x.bit, s->info.out_bytes, x.out_len, x.crc, x.img_bits,
                                              s->info.nstreams + (x.meta >> 4), x.meta & 15u));
            s->info.out_bytes += x.out_len;
        }
        if (s->find_on && s->rd_nb) {                        // (a round without a block copies nothing back)
            const int rc = ds_find_digest(s, q, pass_base);
            if (rc) return rc;
        }
    } else if (r.good_bytes) {                               // the verified bytes travel beside the next pass
        HIP_TRY(ctx, hipMemcpyAsync(s->h_stage[q], s->d_stage[q], r.good_bytes, hipMemcpyDeviceToHost, s->s_d2h));
        HIP_TRY(ctx, hipEventRecord(s->ev_d2h[q], s->s_d2h));
        s->slot[q].bytes = r.good_bytes;
        s->slot[q].off = 0;
        s->slot[q].arrived = false;
        s->q_n++;
    }
    const uint32_t first_blk = s->info.nblk;
    s->info.nblk += r.good;
    if (r.good < r.placed - r.pass_j0) ds_fail(s, dc_why_text(DC_WHY_BLOCK_CRC, first_blk + r.good));
    else if (r.placed < r.nchain && r.lay_err) ds_fail(s, dc_why_text(DC_WHY_IBWT));
    else if (r.placed >= r.nchain) ds_round_complete(s);
    return BZX_OK;
}

// One pass, in every mode: a new round (scan if the window needs one, decode of the next candidates, chain, inverse BWT)
// when no decoded block waits in the slabs, then layout, expansion, CRCs and verdict into the staging area `q`, the
// record, ONE synchronisation, and the host's digest of the record (which starts the copy-back of the verified bytes on
// its own stream).  A round takes at most R block candidates; salvage, whose kernels look at the end-of-stream
// candidates too, cuts it at R of those as well and tells the device which slab decodes which candidate.
static int ds_pass(bzx_dstream *s, uint32_t q)
{
    bzx_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    BzxBatch &B = ctx->B;
    const bool sv = s->mode == DS_SALVAGE, fresh = !s->rd_active;
    if (fresh) {
        if (s->need_scan) {
            const int rc = ds_scan(s);
            if (rc) return rc;
        }
        while (s->ci < s->ncand && (s->h_cand[s->ci] >> 1) < s->chain_bit) s->ci++;
        if (s->ci == s->ncand) {
            if (sv) sv_used_up(s);
            else ds_no_magic(s, true);
            return BZX_OK;
        }
        const uint32_t c0 = s->ci;
        uint32_t c1 = c0, nb = 0, ne = 0;
        for (; c1 < s->ncand; c1++) {
            if (s->h_cand[c1] & 1u) {
                if (sv && ne == s->R) break;
                ne++;
                continue;
            }
            if (nb == s->R) break;
            if (sv) s->h_svc[c1 - c0].slab = nb;
            s->h_src[nb++] = BzxDcSrc{s->wptr, s->wlen, (s->h_cand[c1] >> 1) - s->wbase * 8};
        }
        s->ci = c1;
        s->rd_c0 = c0;
        s->rd_c1 = c1;
        s->rd_nb = nb;
        s->sv.k = 0;                                         // (salvage: the walk stands before the round's first candidate)
    }
    const uint32_t nb = s->rd_nb, c0 = s->rd_c0, c1 = s->rd_c1;
    B.nblk = nb;
    B.blk_first = 0;
    B.blk_step = 1;
    (void)hipEventRecord(ctx->ev[5], st);
    if (fresh) {
        if (nb) {
            HIP_TRY(ctx, hipMemcpyAsync(s->d_src, s->h_src, nb * sizeof(BzxDcSrc), hipMemcpyHostToDevice, st));
            if (sv) HIP_TRY(ctx, hipMemcpyAsync(s->d_svc, s->h_svc, (c1 - c0) * sizeof(DsSvCand), hipMemcpyHostToDevice, st));
            bzx_launch_dc_decode(B, s->d_src, st);
        }
        ds_launch_chain(s);
        if (nb) bzx_launch_dc_ibwt(B, ctx->d_in, st);
    }
    if (nb) {
        ds_launch_layout(s, q);
        bzx_launch_dc_expand(B, ctx->d_in, s->d_dst, st);
        bzx_launch_dc_crc(B, s->d_dst, s->d_got, (uint32_t)ctx->n_cu, st);
        if (s->rec_delim >= 0)
            bzx_launch_rec_count(B.blk, s->d_dst, nb, (uint32_t)s->rec_delim, s->d_rcnt, (uint32_t)ctx->n_cu, st);
    }
    int rc = ds_launch_verdict(s, q, nb);
    if (rc) return rc;
    HIP_TRY(ctx, hipGetLastError());
    rc = ds_copy_record(s);
    if (rc) return rc;
    (void)hipEventRecord(ctx->ev[7], st);
    HIP_TRY(ctx, hipStreamSynchronize(st));                  // the pass's one synchronisation
    s->info.rounds++;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[7]) == hipSuccess) s->ms += ms;
    return sv ? sv_digest(s) : ds_digest(s, q, fresh);
}

// The first window is there: the stream's header, and where the chain (or the salvage walk: include/bzx.h) starts.
static void ds_start(bzx_dstream *s)
{
    s->started = true;
    if (s->mode == DS_SALVAGE) {
        s->sv = DsSvState{};
        s->sv.level = s->info.in_bytes >= 4 ? bzx_bzh_level(s->head) : 0u;
        if (s->sv.level) {
            s->sv.P = s->sv.S = 32;
            s->sv.clean = 1;
        } else {
            s->sv.level = 9;
            s->sv.gap = bzx_gap{0, 0, 0, 0u, BZX_GAP_HEADER};
            s->sv.gap_open = 1;
        }
        s->chain_bit = s->sv.S;
    } else if (s->wlen < 14) {
        ds_fail(s, dc_why_text(DC_WHY_SHORT));
    } else if (!(s->level = bzx_bzh_level(s->head))) {
        ds_fail(s, dc_why_text(DC_WHY_NO_HEADER));
    } else {
        s->chain_bit = 32;
        s->comb = 0;
    }
}

// The accepted bytes become the window: the carry of the window before moves in front of them.
static int ds_promote(bzx_dstream *s)
{
    bzx_ctx *ctx = s->ctx;
    const uint32_t a = s->acc;
    uint64_t carry_off = 0, carry_len = 0;
    if (s->have_win) {
        carry_off = s->chain_bit / 8 - s->wbase;
        carry_len = s->wlen - carry_off;
        if (carry_len > DS_CARRY_MAX) {                      // (cannot happen: a withheld block is shorter)
            ctx->err = "bzx_dstream: the withheld tail exceeds its reserve";
            return BZX_E_STATE;
        }
    }
    uint8_t *np = s->d_in[a] + DS_CARRY_MAX - carry_len;
    if (carry_len)
        HIP_TRY(ctx, hipMemcpyAsync(np, s->wptr + carry_off, carry_len, hipMemcpyDeviceToDevice, ctx->stream));
    // later accepted bytes land in the buffer the carry is read from: behind that copy
    HIP_TRY(ctx, hipEventRecord(s->ev_carry, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(s->s_h2d, s->ev_carry, 0));
    HIP_TRY(ctx, hipEventRecord(s->ev_h2d, s->s_h2d));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s->ev_h2d, 0));
    s->wbase += carry_off;
    s->wptr = np;
    s->wlen = carry_len + s->acc_fill;
    s->wfinal = s->final_seen;
    s->have_win = true;
    s->need_more = false;
    s->need_scan = true;
    s->acc = a ^ 1u;
    s->acc_fill = 0;
    s->info.windows++;
    if (!s->started) ds_start(s);
    return BZX_OK;
}

static int ds_feed(bzx_dstream *s, const uint8_t *bz2, size_t len, int final, size_t *consumed, uint8_t *out, size_t cap,
                   size_t *produced, int *done, bool *copied)
{
    bzx_ctx *ctx = s->ctx;
    for (;;) {
        // ---- accept input (after the end of the last stream, or behind an error: swallowed)
        if (s->finished || s->pend_rc) {
            s->info.in_bytes += len - *consumed;
            *consumed = len;
        } else if (*consumed < len && s->acc_fill < s->max_chunk) {
            const size_t k = std::min(len - *consumed, s->max_chunk - s->acc_fill);
            for (size_t i = 0; i < k && s->info.in_bytes + i < 4; i++) s->head[s->info.in_bytes + i] = bz2[*consumed + i];
            HIP_TRY(ctx, hipMemcpyAsync(s->d_in[s->acc] + DS_CARRY_MAX + s->acc_fill, bz2 + *consumed, k, hipMemcpyHostToDevice,
                                        s->s_h2d));
            *copied = true;
            s->acc_fill += k;
            s->info.in_bytes += k;
            *consumed += k;
        }
        if (final && *consumed == len) s->final_seen = true;
        // ---- everything verified has been delivered: the verdict
        if (s->q_n == 0 && s->pend_rc) {
            if (*produced) return BZX_OK;                    // (the bytes of this call count: the error is the next call's)
            s->err_rc = s->pend_rc;
            s->err_text = s->pend_text;
            ctx->err = s->err_text;
            return s->err_rc;
        }
        if (s->q_n == 0 && s->finished) {
            s->done = true;
            *done = 1;
            memset(&ctx->stats, 0, sizeof(ctx->stats));
            ctx->stats_batch = true;
            ctx->stats.nblk = s->info.nblk;
            ctx->stats.raw_bytes = s->info.out_bytes;
            ctx->stats.ms_total = s->ms;
            return BZX_OK;
        }
        const bool live = !s->pend_rc && !s->finished;
        // ---- a pass, when there is something to decode or place and a staging area is free
        if (live && (s->rd_active || (s->have_win && !s->need_more)) && s->q_n < 2) {
            const uint32_t q = (s->q_head + s->q_n) & 1u;
            const int rc = ds_pass(s, q);
            if (rc) return rc;
            continue;
        }
        // ---- the window is used up: the next one, when it is full or nothing follows
        if (live && !s->rd_active && (!s->have_win || s->need_more) &&
            (s->acc_fill == s->max_chunk || (s->final_seen && !(s->have_win && s->wfinal)))) {
            const int rc = ds_promote(s);
            if (rc) return rc;
            continue;
        }
        // ---- deliver
        if (s->q_n && *produced < cap) {
            DsSlot &sl = s->slot[s->q_head];
            if (!sl.arrived) {
                HIP_TRY(ctx, hipEventSynchronize(s->ev_d2h[s->q_head]));
                sl.arrived = true;
            }
            const size_t k = (size_t)std::min<uint64_t>(cap - *produced, sl.bytes - sl.off);
            memcpy(out + *produced, s->h_stage[s->q_head] + sl.off, k);
            sl.off += k;
            *produced += k;
            s->info.out_bytes += k;
            if (sl.off == sl.bytes) {
                s->q_head ^= 1u;
                s->q_n--;
            }
            continue;
        }
        return BZX_OK;                                       // buffered, or the caller's room is used up
    }
}

// The feed call of every mode (the callers have checked their arguments): the lock, a latched error again, ds_feed, and
// the wait that lets the caller reuse its input buffer.
static int ds_feed_call(bzx_dstream *s, const uint8_t *bz2, size_t len, int final, size_t *consumed, uint8_t *out, size_t cap,
                        size_t *produced, int *done)
{
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    *consumed = 0;
    *produced = 0;
    *done = 0;
    if (s->err_rc) {
        ctx->err = s->err_text;
        return s->err_rc;
    }
    if (s->done && s->mode == DS_STREAM) {
        ctx->err = "bzx_dstream_feed: the stream is done";
        return BZX_E_STATE;
    }
    if (s->done) {                                           // bytes behind the last stream: counted, not looked at
        s->info.in_bytes += len;
        *consumed = len;
        *done = 1;
        return BZX_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool copied = false;
    int rc;
    try {
        rc = ds_feed(s, bz2, len, final, consumed, out, cap, produced, done, &copied);
    } catch (const std::bad_alloc &) {                       // (nothing may unwind across the C ABI)
        ctx->err = "out of host memory";
        rc = BZX_E_NOMEM;
    }
    // the accepted bytes have left the caller's buffer when the call returns (it may be page-locked and reused)
    if (copied && hipStreamSynchronize(s->s_h2d) != hipSuccess && !rc) {
        ctx->err = "hipStreamSynchronize(input copy) failed";
        rc = BZX_E_HIP;
    }
    if (rc && !s->err_rc) {                                  // a runtime error ends the stream too
        s->err_rc = rc;
        s->err_text = ctx->err;
    }
    return rc;
}

extern "C" int bzx_dstream_feed(bzx_dstream *s, const uint8_t *bz2, size_t len, int final, size_t *consumed, uint8_t *out,
                                size_t cap, size_t *produced, int *done)
{
    if (!s || !s->ctx || !consumed || !produced || !done || (len && !bz2) || (cap && !out)) return BZX_E_PARAM;
    return ds_feed_call(s, bz2, len, final, consumed, out, cap, produced, done);
}

// ---- bzx_index_*, bzx_salvage_*: the same machine with nothing handed out -----------------------------------------------
extern "C" void bzx_index_end(bzx_index *ix)
{
    if (!ix) return;
    if (ix->s) {
        ix->s->ix = nullptr;
        bzx_dstream_end(ix->s);
    }
    delete ix;
}

static int ix_begin(bzx_ctx *ctx, size_t max_chunk, DsMode mode, bzx_index **out)
{
    if (!ctx || !out) return BZX_E_PARAM;
    *out = nullptr;
    bzx_index *ix = new (std::nothrow) bzx_index();
    if (!ix) return BZX_E_NOMEM;
    const int rc = ds_begin(ctx, max_chunk, mode, &ix->s);
    if (rc) {
        delete ix;
        return rc;
    }
    ix->s->ix = ix;
    *out = ix;
    return BZX_OK;
}

extern "C" int bzx_index_begin(bzx_ctx *ctx, size_t max_chunk, bzx_index **out)
{
    return ix_begin(ctx, max_chunk, DS_INDEX, out);
}

extern "C" int bzx_salvage_begin(bzx_ctx *ctx, size_t max_chunk, bzx_index **out)
{
    return ix_begin(ctx, max_chunk, DS_SALVAGE, out);
}

extern "C" int bzx_index_feed(bzx_index *ix, const uint8_t *bz2, size_t len, int final, size_t *consumed, int *done)
{
    if (!ix || !ix->s || !ix->s->ctx || !consumed || !done || (len && !bz2)) return BZX_E_PARAM;
    size_t produced = 0;
    ix->fed = true;
    return ds_feed_call(ix->s, bz2, len, final, consumed, nullptr, 0, &produced, done);
}

// Counting switched on: the pass gains bzx_rec_count_kernel behind the CRCs and one word per block in its copy; the
// tables grow here, between begin and the first feed, so that an index without counting allocates what it always did.
extern "C" int bzx_index_count_records(bzx_index *ix, int delim)
{
    if (!ix || !ix->s || !ix->s->ctx) return BZX_E_PARAM;
    bzx_dstream *s = ix->s;
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    if (s->mode != DS_INDEX) {
        ctx->err = "bzx_index_count_records: not on a salvage index (its entries come from the device walk)";
        return BZX_E_STATE;
    }
    if (ix->fed) {
        ctx->err = "bzx_index_count_records: call it before the first bzx_index_feed";
        return BZX_E_STATE;
    }
    if (delim < 0 || delim > 255) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t R = s->R, before_ix = s->d_ix.bytes(), before_pin = s->h_ix.bytes();
    try {
        ix->rec.assign(1, 0);
    } catch (const std::bad_alloc &) {
        return BZX_E_NOMEM;
    }
    const size_t tab = s->find_off + R * (sizeof(DsIxRec) + 4);
    if (!s->d_rcnt.reserve(R * 4) || !s->d_ix.reserve(tab) || !s->h_ix.reserve(tab) ||
        hipMemset(s->d_ix, 0, tab) != hipSuccess || hipMemset(s->d_rcnt, 0, R * 4) != hipSuccess) {
        ctx->err = "bzx_index_count_records: device or pinned allocation failed";
        return BZX_E_NOMEM;
    }
    if (s->rec_delim < 0) {
        s->info.device_bytes += R * 4 + s->d_ix.bytes() - before_ix;
        s->info.pinned_bytes += s->h_ix.bytes() - before_pin;
    }
    s->rec_delim = delim;
    return BZX_OK;
}

extern "C" int bzx_index_get_records(const bzx_index *ix, const uint64_t **rec_before, uint64_t *n)
{
    if (!ix || !ix->s || !ix->s->ctx || !rec_before || !n) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ix->s->ctx->api_mu);
    if (ix->s->rec_delim < 0) {
        ix->s->ctx->err = "bzx_index_get_records: counting was not switched on (bzx_index_count_records)";
        return BZX_E_STATE;
    }
    *rec_before = ix->rec.data();
    *n = ix->entries.size();
    return BZX_OK;
}

// Find switched on: the pass gains the three kernels of bzx_find.hip behind its verdict and a BzxFindOut in front of the
// records in the copy that brings its entries back; everything the device side needs is allocated here, between begin
// and the first feed, so that an index without find allocates what it always did.
static_assert(sizeof(BzxFindOut) % 8 == 0, "the index records behind it hold 64-bit values");
extern "C" int bzx_index_find(bzx_index *ix, const uint8_t *pat, size_t m, uint64_t max_hits)
{
    if (!ix || !ix->s || !ix->s->ctx) return BZX_E_PARAM;
    bzx_dstream *s = ix->s;
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    if (s->mode != DS_INDEX) {
        ctx->err = "bzx_index_find: not on a salvage index (its entries come from the device walk)";
        return BZX_E_STATE;
    }
    if (ix->fed) {
        ctx->err = "bzx_index_find: call it before the first bzx_index_feed";
        return BZX_E_STATE;
    }
    BzxFindPat fp;
    if (!bzx_find_pattern(pat, m, &fp)) {
        ctx->err = "bzx_index_find: the pattern is NULL, empty or longer than BZX_FIND_MAX_PATTERN bytes";
        return BZX_E_PARAM;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t R = s->R, before_dev = s->d_ix.bytes() + s->d_fsec.bytes() + s->d_fwin.bytes(),
                 before_pin = s->h_ix.bytes() + s->h_fwin.bytes();
    const size_t off = sizeof(BzxFindOut) + (s->lines_delim >= 0 ? sizeof(BzxFindLines) : 0);   // (lines stay on)
    const size_t tab = off + R * (sizeof(DsIxRec) + (s->rec_delim >= 0 ? 4 : 0));
    try {
        ix->hits.clear();
        ix->lines.clear();
        s->find_carry.clear();
        s->find_carry.reserve(2 * BZX_FIND_MAX_PATTERN);
    } catch (const std::bad_alloc &) {
        return BZX_E_NOMEM;
    }
    if (!s->d_fsec.reserve(bzx_find_sections(DS_STAGE_BYTES) * 4) || !s->d_fwin.reserve((size_t)FIND_WINDOW_HITS * 4) ||
        !s->h_fwin.reserve((size_t)FIND_WINDOW_HITS * 4) || !s->d_ix.reserve(tab) || !s->h_ix.reserve(tab) ||
        hipMemset(s->d_ix, 0, tab) != hipSuccess) {
        ctx->err = "bzx_index_find: device or pinned allocation failed";
        return BZX_E_NOMEM;
    }
    s->info.device_bytes += s->d_ix.bytes() + s->d_fsec.bytes() + s->d_fwin.bytes() - before_dev;
    s->info.pinned_bytes += s->h_ix.bytes() + s->h_fwin.bytes() - before_pin;
    s->find_on = true;
    s->find_off = off;
    s->dbase = 0;
    s->find_pat = fp;
    s->find_max = max_hits;
    ix->hit_total = 0;
    return BZX_OK;
}

extern "C" int bzx_index_get_hits(const bzx_index *ix, const uint64_t **hits, uint64_t *nlisted, uint64_t *total)
{
    if (!ix || !ix->s || !ix->s->ctx || !hits || !nlisted || !total) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ix->s->ctx->api_mu);
    if (!ix->s->find_on) {
        ix->s->ctx->err = "bzx_index_get_hits: find was not switched on (bzx_index_find)";
        return BZX_E_STATE;
    }
    *hits = ix->hits.data();
    *nlisted = ix->hits.size();
    *total = ix->hit_total;
    return BZX_OK;
}

// Lines switched on: the pass launches the lines forms of the three kernels in place of the plain ones and its copy
// grows by a BzxFindLines behind the BzxFindOut; what that takes is allocated here, so that a find without lines
// allocates, launches and copies what it always did.
static_assert(sizeof(BzxFindLines) % 8 == 0, "the index records behind it hold 64-bit values");
extern "C" int bzx_index_find_lines(bzx_index *ix, int delim)
{
    if (!ix || !ix->s || !ix->s->ctx) return BZX_E_PARAM;
    bzx_dstream *s = ix->s;
    bzx_ctx *ctx = s->ctx;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    if (s->mode != DS_INDEX) {
        ctx->err = "bzx_index_find_lines: not on a salvage index (its entries come from the device walk)";
        return BZX_E_STATE;
    }
    if (ix->fed) {
        ctx->err = "bzx_index_find_lines: call it before the first bzx_index_feed";
        return BZX_E_STATE;
    }
    if (!s->find_on) {
        ctx->err = "bzx_index_find_lines: call it after bzx_index_find";
        return BZX_E_STATE;
    }
    if (delim < 0 || delim > 255) {
        ctx->err = "bzx_index_find_lines: the delimiter is one byte value, 0..255";
        return BZX_E_PARAM;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t R = s->R, before_dev = s->d_ix.bytes() + s->d_dsec.bytes() + s->d_lwin.bytes(),
                 before_pin = s->h_ix.bytes() + s->h_lwin.bytes();
    const size_t off = sizeof(BzxFindOut) + sizeof(BzxFindLines);
    const size_t tab = off + R * (sizeof(DsIxRec) + (s->rec_delim >= 0 ? 4 : 0));
    ix->lines.clear();
    if (!s->d_dsec.reserve(bzx_find_sections(DS_STAGE_BYTES) * 4) || !s->d_lwin.reserve((size_t)FIND_WINDOW_HITS * 4) ||
        !s->h_lwin.reserve((size_t)FIND_WINDOW_HITS * 4) || !s->d_ix.reserve(tab) || !s->h_ix.reserve(tab) ||
        hipMemset(s->d_ix, 0, tab) != hipSuccess) {
        ctx->err = "bzx_index_find_lines: device or pinned allocation failed";
        return BZX_E_NOMEM;
    }
    s->info.device_bytes += s->d_ix.bytes() + s->d_dsec.bytes() + s->d_lwin.bytes() - before_dev;
    s->info.pinned_bytes += s->h_ix.bytes() + s->h_lwin.bytes() - before_pin;
    s->find_off = off;
    s->lines_delim = delim;
    s->dbase = 0;
    return BZX_OK;
}

extern "C" int bzx_index_get_hit_lines(const bzx_index *ix, const uint64_t **lines, uint64_t *nlisted)
{
    if (!ix || !ix->s || !ix->s->ctx || !lines || !nlisted) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ix->s->ctx->api_mu);
    if (ix->s->lines_delim < 0) {
        ix->s->ctx->err = "bzx_index_get_hit_lines: lines were not switched on (bzx_index_find_lines)";
        return BZX_E_STATE;
    }
    *lines = ix->lines.data();
    *nlisted = ix->lines.size();
    return BZX_OK;
}

extern "C" int bzx_index_get(const bzx_index *ix, const bzx_index_entry **entries, bzx_index_info *info)
{
    if (!ix || !ix->s || !ix->s->ctx || !entries || !info) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ix->s->ctx->api_mu);
    *entries = ix->entries.data();
    memset(info, 0, sizeof(*info));
    info->in_bytes = ix->s->info.in_bytes;
    info->out_bytes = ix->s->info.out_bytes;
    info->nblk = ix->entries.size();
    info->nstreams = ix->s->info.nstreams;
    return BZX_OK;
}

extern "C" int bzx_index_get_gaps(const bzx_index *ix, const bzx_gap **gaps, uint64_t *ngaps)
{
    if (!ix || !ix->s || !ix->s->ctx || !gaps || !ngaps) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ix->s->ctx->api_mu);
    *gaps = ix->gaps.data();
    *ngaps = ix->gaps.size();
    return BZX_OK;
}

// ---- the calls over a whole buffer ----------------------------------------------------------------------------------------
// Begin, a loop over feed, the lists and `info`, end.  The lists leave the handle by swap, so nothing is allocated behind
// the feed loop.  A run that failed hands nothing out, except in the index mode: there the entries and `info` describe
// the verified prefix, and the feed's code and text are the call's.
static int ix_build(bzx_ctx *ctx, DsMode mode, const uint8_t *bz2, size_t len, std::vector<bzx_index_entry> &entries,
                    bzx_index_info *info, std::vector<bzx_gap> &gaps, int delim = -1, std::vector<uint64_t> *rec = nullptr,
                    const uint8_t *pat = nullptr, size_t m = 0, uint64_t max_hits = 0, std::vector<uint64_t> *hits = nullptr,
                    uint64_t *hit_total = nullptr)
{
    bzx_index *ix = nullptr;
    int rc = ix_begin(ctx, std::min<size_t>(std::max<size_t>(len, DS_MIN_CHUNK), (size_t)64 << 20), mode, &ix);
    if (rc) return rc;
    if ((rec && (rc = bzx_index_count_records(ix, delim))) || (hits && (rc = bzx_index_find(ix, pat, m, max_hits)))) {
        const std::string why = ctx->err;
        bzx_index_end(ix);
        ctx->err = why;
        return rc;
    }
    size_t pos = 0;
    int done = 0;
    while (!rc && !(done && pos == len)) {
        size_t used = 0;
        rc = bzx_index_feed(ix, bz2 + pos, len - pos, 1, &used, &done);
        pos += used;
        if (!rc && !used && !done) {                         // (a final feed consumes or finishes)
            ctx->err = mode == DS_INDEX ? "bzx_index_build_buffer: the feed loop made no progress"
                                        : "bzx_salvage: the feed loop made no progress";
            rc = BZX_E_STATE;
        }
    }
    const std::string why = ctx->err;
    const bzx_index_entry *e = nullptr;
    if ((!rc || mode == DS_INDEX) && bzx_index_get(ix, &e, info) == BZX_OK) {
        entries.swap(ix->entries);
        gaps.swap(ix->gaps);
        if (rec) rec->swap(ix->rec);
        if (hits) {
            hits->swap(ix->hits);
            *hit_total = ix->hit_total;
        }
    }
    bzx_index_end(ix);
    if (rc) ctx->err = why;
    return rc;
}

// The first min(size, cap) elements of a list go out; a list that did not fit turns a call that succeeded so far (rc)
// into BZX_E_OUTBUF with `text`.
template <typename T>
static int ix_copy_out(bzx_ctx *ctx, int rc, const std::vector<T> &v, T *out, uint64_t cap, const char *text)
{
    const uint64_t k = std::min<uint64_t>(v.size(), cap);
    if (k) memcpy(out, v.data(), (size_t)k * sizeof(T));
    if (rc || v.size() <= cap) return rc;
    ctx->err = text;
    return BZX_E_OUTBUF;
}

extern "C" int bzx_index_build_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, bzx_index_entry *entries,
                                      uint64_t cap_entries, bzx_index_info *info)
{
    if (!ctx || !info || (len && !bz2) || (cap_entries && !entries)) return BZX_E_PARAM;
    memset(info, 0, sizeof(*info));
    std::vector<bzx_index_entry> e;
    std::vector<bzx_gap> g;
    const int rc = ix_build(ctx, DS_INDEX, bz2, len, e, info, g);
    return ix_copy_out(ctx, rc, e, entries, cap_entries, "bzx_index_build_buffer: more blocks than cap_entries");
}

extern "C" int bzx_index_build_records_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, int delim, bzx_index_entry *entries,
                                              uint64_t cap_entries, bzx_index_info *info, uint64_t *rec_before)
{
    if (!ctx || !info || !rec_before || (len && !bz2) || (cap_entries && !entries) || delim < 0 || delim > 255) return BZX_E_PARAM;
    memset(info, 0, sizeof(*info));
    rec_before[0] = 0;
    std::vector<bzx_index_entry> e;
    std::vector<bzx_gap> g;
    std::vector<uint64_t> r;
    const int rc = ix_build(ctx, DS_INDEX, bz2, len, e, info, g, delim, &r);
    // (the table of the entries that go out: one value more than they are)
    const size_t k = (size_t)std::min<uint64_t>(e.size(), cap_entries);
    if (r.size() > k) memcpy(rec_before, r.data(), (k + 1) * sizeof(uint64_t));
    return ix_copy_out(ctx, rc, e, entries, cap_entries, "bzx_index_build_records_buffer: more blocks than cap_entries");
}

extern "C" int bzx_find_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, const uint8_t *pat, size_t m, uint64_t *hits,
                               uint64_t cap_hits, uint64_t *nlisted, uint64_t *total, bzx_index_entry *entries,
                               uint64_t cap_entries, bzx_index_info *info)
{
    BzxFindPat fp;
    if (!ctx || !nlisted || !total || !info || (len && !bz2) || (cap_hits && !hits) || (cap_entries && !entries) ||
        !bzx_find_pattern(pat, m, &fp))
        return BZX_E_PARAM;
    memset(info, 0, sizeof(*info));
    *nlisted = *total = 0;
    std::vector<bzx_index_entry> e;
    std::vector<bzx_gap> g;
    std::vector<uint64_t> h;
    const int rc = ix_build(ctx, DS_INDEX, bz2, len, e, info, g, -1, nullptr, pat, m, cap_hits, &h, total);
    *nlisted = h.size();
    if (!h.empty()) memcpy(hits, h.data(), h.size() * sizeof(uint64_t));
    if (!entries && !cap_entries) return rc;                 // (the index is not wanted)
    return ix_copy_out(ctx, rc, e, entries, cap_entries, "bzx_find_buffer: more blocks than cap_entries");
}

extern "C" int bzx_salvage_build_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, bzx_index_entry *entries,
                                        uint64_t cap_entries, bzx_index_info *info, bzx_gap *gaps, uint64_t cap_gaps,
                                        uint64_t *ngaps)
{
    if (!ctx || !info || !ngaps || (len && !bz2) || (cap_entries && !entries) || (cap_gaps && !gaps)) return BZX_E_PARAM;
    memset(info, 0, sizeof(*info));
    *ngaps = 0;
    std::vector<bzx_index_entry> e;
    std::vector<bzx_gap> g;
    const int rc = ix_build(ctx, DS_SALVAGE, bz2, len, e, info, g);
    if (rc) return rc;
    *ngaps = g.size();
    const int rc_gaps = ix_copy_out(ctx, 0, g, gaps, cap_gaps, "bzx_salvage: more gaps than cap_gaps");
    const int rc_ent = ix_copy_out(ctx, 0, e, entries, cap_entries, "bzx_salvage_build_buffer: more blocks than cap_entries");
    return rc_ent ? rc_ent : rc_gaps;                        // (both did not fit: the entries' text)
}

extern "C" int bzx_salvage_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, uint8_t *out, size_t cap, size_t *out_len,
                                  bzx_gap *gaps, uint64_t cap_gaps, uint64_t *ngaps)
{
    if (!ctx || !out_len || !ngaps || (len && !bz2) || (cap && !out) || (cap_gaps && !gaps)) return BZX_E_PARAM;
    *out_len = 0;
    *ngaps = 0;
    std::vector<bzx_index_entry> e;
    std::vector<bzx_gap> g;
    bzx_index_info info;
    memset(&info, 0, sizeof(info));
    int rc = ix_build(ctx, DS_SALVAGE, bz2, len, e, &info, g);
    if (rc) return rc;
    *ngaps = g.size();
    const int rc_gaps = ix_copy_out(ctx, 0, g, gaps, cap_gaps, "bzx_salvage: more gaps than cap_gaps");
    *out_len = (size_t)info.out_bytes;
    const uint64_t want = std::min<uint64_t>(info.out_bytes, cap);
    if (want) {
        // The range reader asks for 8 bytes behind a block's image (bzx_index_span); the last blocks of a truncated input
        // may not have them.  Those are read in a second call, over a copy of the input's tail with 8 zero bytes appended.
        uint64_t k = e.size();
        while (k > 0 && (e[k - 1].bit + e[k - 1].img_bits + 7) / 8 + 8 > len) k--;
        const uint64_t head = k < e.size() ? std::min<uint64_t>(e[k].out_off, want) : want;
        size_t got = 0;
        if (head) rc = bzx_decompress_range_buffer(ctx, bz2, len, 0, e.data(), e.size(), 0, head, out, &got);
        if (!rc && want > head) {
            const uint64_t base = e[k].bit / 8;
            std::vector<uint8_t> tail;
            try {
                tail.assign(bz2 + base, bz2 + len);
                tail.resize(tail.size() + 8, 0);
            } catch (const std::bad_alloc &) {
                ctx->err = "out of host memory";
                return BZX_E_NOMEM;
            }
            rc = bzx_decompress_range_buffer(ctx, tail.data(), tail.size(), base, e.data(), e.size(), head, want - head, out + head,
                                             &got);
        }
        if (rc) return rc;
    }
    if (info.out_bytes > cap) {
        ctx->err = "bzx_salvage_buffer: the salvaged data needs " + std::to_string(info.out_bytes) + " bytes";
        return BZX_E_OUTBUF;
    }
    return rc_gaps;
}
