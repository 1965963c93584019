// bzx_find.hip -- the positions of a byte pattern in a run of device bytes on gfx950 (include/bzx.h: bzx_index_find,
// bzx_find_geometry, bzx_stage_find; the index pass launches these kernels behind its verdict: bzx_dstream.hip).
//
// The rule: pat[0, m) with 1 <= m <= 256 bytes of any value; a hit of the run [p, p + L) is a start position s with
// s + m <= L and p[s, s + m) == pat, overlapping ones included.  L is read on the device (in the index pass it is the
// verified byte count the verdict kernel left), and no byte at or behind p + L is ever read: what lies there -- the next
// pass's blocks, a neighbouring segment -- cannot make a hit and cannot fault.
//
// The cut.  Start positions are cut on the 16-byte boundaries of the ADDRESS: with a = p mod 16 the frame byte f = a + s,
// a chunk is 16 frame bytes (one lane's load), a step is 64 chunks (1 KiB, one load per lane of a wave), a section is 4
// steps (FIND_SEC_BYTES, what one wave walks), a tile is 4 sections (FIND_TILE_BYTES, one workgroup of 256 lanes); the
// workgroups stride over the tiles.  A chunk that lies wholly inside the run is one 16-byte load; the chunk that holds
// the run's first bytes in front of a boundary (the head) and the one that holds its last bytes behind one (the tail)
// are read byte by byte, with zeros in place of what is not the run's.  A lane also reads the four bytes behind its
// chunk, the same way.
//
// The match, per lane and chunk, is a 16-bit mask of start positions:
//   first byte   rec_match's carry-free test (bzx_records.hip) of the four words against pat[0]: exact, and for m == 1
//                the whole answer
//   prefix       for the candidates: the word at each of the 16 byte phases (bzx_alignbyte over the lane's five words)
//                against the first min(m, 4) pattern bytes, under a mask for m < 4
//   rest         for m > 4 and where the prefix matched: bytes 4 .. m - 1 from memory against the pattern in LDS, to the
//                first difference.  All-equal data with an all-equal pattern runs every one of these to its end: correct,
//                and slow (DESIGN.md 5k has the figure).
//   validity     s >= 0 and s + m <= L, so the zeros that stand for bytes outside the run never take part in a hit
//
// Three kernels, no atomics and no sort:
//   count   every wave leaves the hits of its section in sec[] (a wave sum, one store)
//   scan    one workgroup turns sec[] into its exclusive sum and leaves *after = *before + the run's count; for the
//           index pass it also copies the run's first and last min(m - 1, L) bytes next to the count (the host finds
//           the hits that straddle two passes in them)
//   emit    every wave whose section's numbers meet [skip, skip + cap) walks it again; a wave scan per step gives every
//           lane the number of its first hit, and hit k goes to out[k - skip].  The list is ascending by construction.
//
// The lines forms (bzx_index_find_lines, bzx_stage_find_lines): the same three kernels with the delimiters of the run
// counted in the same walk, so that every hit comes with line(hit) = the delimiters of the run in front of its first
// byte.  The test is find_match against bzx_rep4(delim) on the four words the lane holds anyway, under a validity mask
// for 0 <= s < L (a zero that stands for a byte outside the run never counts, also for delim == 0).
//   count   also leaves the delimiters of every section in dsec[]; these sections cover the WHOLE run, frame bytes
//           [a, a + L): ceil((a + L) / FIND_SEC_BYTES) of them, one more than nsec where the last m - 1 bytes open a
//           section of their own, and all there are when L < m
//   scan    also turns dsec[] into its exclusive sum and leaves the run's delimiter total
//   emit    a second wave scan per step, over the popcounts of the lanes' delimiter masks: hit k at bit j of a chunk
//           writes lines_out[k - skip] = dsec[s] + the delimiters of the section's earlier steps + those of the lower
//           lanes + popc(dmask & ((1 << j) - 1)), a 32-bit count relative to the run
// The plain forms keep their kernels and their launches; find_mask16<false> is the code they always ran.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bzx_host.h"
#include "bzx_wg.h"

#define FIND_NT 256
#define FIND_STEPS (FIND_SEC_BYTES / 1024u)

// rec_match of bzx_records.hip: one bit (bit 7) per byte of w that equals the byte repeated in rep, without a carry
// between bytes.
__device__ __forceinline__ uint32_t find_match(uint32_t w, uint32_t rep)
{
    const uint32_t x = w ^ rep;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// bits 7, 15, 23, 31 -> bits 0 .. 3
__device__ __forceinline__ uint32_t find_bits4(uint32_t mm)
{
    return ((mm >> 7) & 1u) | ((mm >> 14) & 2u) | ((mm >> 21) & 4u) | ((mm >> 28) & 8u);
}

struct FindRun {
    const uint8_t *p;
    int64_t len;                   // L
    uint32_t a;                    // p mod 16
    uint32_t nsec;                 // sections that hold a start position of a hit (0 when L < m)
    uint32_t m, pm, pmask, pat0, rep;
};

__device__ __forceinline__ FindRun find_run(const uint8_t *p, uint64_t len, uint32_t m, const uint32_t *s_pat)
{
    FindRun R;
    R.p = p;
    R.len = (int64_t)len;
    R.a = (uint32_t)((uintptr_t)p & 15u);
    R.nsec = len >= m ? (uint32_t)((R.a + (len - m + 1) + FIND_SEC_BYTES - 1) / FIND_SEC_BYTES) : 0u;
    R.m = m;
    R.pm = m < 4u ? m : 4u;
    R.pmask = R.pm == 4u ? 0xFFFFFFFFu : (1u << (8u * R.pm)) - 1u;
    R.pat0 = s_pat[0] & R.pmask;
    R.rep = bzx_rep4(s_pat[0]);
    return R;
}

// Byte s of the run, 0 outside it.
__device__ __forceinline__ uint32_t find_byte(const FindRun &R, int64_t s)
{
    return s >= 0 && s < R.len ? (uint32_t)R.p[s] : 0u;
}

__device__ __forceinline__ uint32_t find_word_bytes(const FindRun &R, int64_t s)
{
    return find_byte(R, s) | (find_byte(R, s + 1) << 8) | (find_byte(R, s + 2) << 16) | (find_byte(R, s + 3) << 24);
}

// The 16-bit mask of the hits that start in chunk c (frame bytes [16 c, 16 c + 16)); *lo = the position of its first byte.
// LINES: also *dmask_out = the 16-bit mask of the chunk's bytes that lie in the run and equal the byte repeated in drep.
template <bool LINES>
__device__ __forceinline__ uint32_t find_mask16(const FindRun &R, const uint8_t *s_pat8, uint32_t c, int64_t *lo_out,
                                                uint32_t drep = 0u, uint32_t *dmask_out = nullptr)
{
    const int64_t lo = (int64_t)c * 16 - R.a;
    *lo_out = lo;
    const int64_t last = R.len - (int64_t)R.m - lo;          // the last valid start, relative to lo
    if constexpr (LINES) {                                   // (a chunk without a valid start can still hold delimiters)
        *dmask_out = 0u;
        if (lo >= R.len || lo + 16 <= 0) return 0u;
    } else {
        if (last < 0 || lo + 16 <= 0) return 0u;
    }
    uint32_t valid = 0xFFFFu;
    if (lo < 0) valid &= 0xFFFFu << (uint32_t)(-lo);
    if (LINES && last < 0) valid = 0u;
    else if (last < 15) valid &= 0xFFFFu >> (uint32_t)(15 - last);
    uint32_t w0, w1, w2, w3, w4;
    if (lo >= 0 && lo + 16 <= R.len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(R.p + lo);
        w0 = v.x;
        w1 = v.y;
        w2 = v.z;
        w3 = v.w;
    } else {                                                 // head or tail: byte by byte
        w0 = find_word_bytes(R, lo);
        w1 = find_word_bytes(R, lo + 4);
        w2 = find_word_bytes(R, lo + 8);
        w3 = find_word_bytes(R, lo + 12);
    }
    if constexpr (LINES) {
        const int64_t dlast = R.len - 1 - lo;                // the run's last byte, relative to lo (>= 0 here)
        uint32_t dvalid = 0xFFFFu;
        if (lo < 0) dvalid &= 0xFFFFu << (uint32_t)(-lo);
        if (dlast < 15) dvalid &= 0xFFFFu >> (uint32_t)(15 - dlast);
        *dmask_out = (find_bits4(find_match(w0, drep)) | (find_bits4(find_match(w1, drep)) << 4) |
                      (find_bits4(find_match(w2, drep)) << 8) | (find_bits4(find_match(w3, drep)) << 12)) & dvalid;
    }
    uint32_t hit = find_bits4(find_match(w0, R.rep)) | (find_bits4(find_match(w1, R.rep)) << 4) |
                   (find_bits4(find_match(w2, R.rep)) << 8) | (find_bits4(find_match(w3, R.rep)) << 12);
    hit &= valid;
    if (R.m == 1u || hit == 0u) return hit;
    if (lo + 16 >= 0 && lo + 20 <= R.len) w4 = *reinterpret_cast<const uint32_t *>(R.p + lo + 16);
    else w4 = find_word_bytes(R, lo + 16);
    uint32_t pre = 0;
#define FIND_PHASE(J, HI, LO)                                                                         \
    pre |= (((bzx_alignbyte(HI, LO, (J) & 3u) ^ R.pat0) & R.pmask) == 0u ? 1u : 0u) << (J);
    FIND_PHASE(0, w1, w0) FIND_PHASE(1, w1, w0) FIND_PHASE(2, w1, w0) FIND_PHASE(3, w1, w0)
    FIND_PHASE(4, w2, w1) FIND_PHASE(5, w2, w1) FIND_PHASE(6, w2, w1) FIND_PHASE(7, w2, w1)
    FIND_PHASE(8, w3, w2) FIND_PHASE(9, w3, w2) FIND_PHASE(10, w3, w2) FIND_PHASE(11, w3, w2)
    FIND_PHASE(12, w4, w3) FIND_PHASE(13, w4, w3) FIND_PHASE(14, w4, w3) FIND_PHASE(15, w4, w3)
#undef FIND_PHASE
    hit &= pre;
    if (R.m <= 4u) return hit;
    uint32_t out = 0;
    for (uint32_t left = hit; left; left &= left - 1u) {     // the rest, where the prefix matched
        const uint32_t j = (uint32_t)__ffs(left) - 1u;
        const uint8_t *q = R.p + lo + j;                     // (valid: q[0, m) lies inside the run)
        uint32_t i = 4;
        while (i < R.m && q[i] == s_pat8[i]) i++;
        if (i == R.m) out |= 1u << j;
    }
    return out;
}

__device__ __forceinline__ void find_stage_pattern(const BzxFindPat &pat, uint32_t *s_pat)
{
    if (threadIdx.x < BZX_FIND_MAX_PATTERN / 4) s_pat[threadIdx.x] = pat.w[threadIdx.x];
    __syncthreads();
}

// ---- count -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIND_NT) void bzx_find_count_kernel(const uint8_t *__restrict__ p, const uint64_t *__restrict__ len,
                                                                 BzxFindPat pat, uint32_t *__restrict__ sec)
{
    __shared__ uint32_t s_pat[BZX_FIND_MAX_PATTERN / 4];
    find_stage_pattern(pat, s_pat);
    const FindRun R = find_run(p, *len, pat.m, s_pat);
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    for (uint32_t t = blockIdx.x; t * 4u < R.nsec; t += gridDim.x) {
        const uint32_t s = t * 4u + wave;
        if (s >= R.nsec) continue;                           // (uniform over the wave)
        uint32_t acc = 0;
        for (uint32_t step = 0; step < FIND_STEPS; step++) {
            int64_t lo;
            acc += (uint32_t)__popc(find_mask16<false>(R, reinterpret_cast<const uint8_t *>(s_pat), (s * FIND_STEPS + step) * 64u + lane, &lo));
        }
        const uint32_t incl = bzx_wave_incl_sum(acc);
        if (lane == 63) sec[s] = incl;
    }
}

// ---- scan: one workgroup -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIND_NT) void bzx_find_scan_kernel(const uint8_t *__restrict__ p, const uint64_t *__restrict__ len,
                                                                uint32_t m, uint32_t *__restrict__ sec,
                                                                const uint64_t *__restrict__ before, uint64_t *__restrict__ after,
                                                                BzxFindOut *__restrict__ edges)
{
    __shared__ uint32_t s_scr[FIND_NT / 64];
    const uint64_t L = *len;
    const uint32_t a = (uint32_t)((uintptr_t)p & 15u);
    const uint32_t nsec = L >= m ? (uint32_t)((a + (L - m + 1) + FIND_SEC_BYTES - 1) / FIND_SEC_BYTES) : 0u;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nsec; base += FIND_NT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nsec ? sec[i] : 0u;
        uint32_t total;
        const uint32_t excl = bzx_block_excl_sum<FIND_NT>(v, s_scr, total);
        if (i < nsec) sec[i] = (uint32_t)carry + excl;      // (a run is shorter than 2^32 bytes, and so is its count)
        carry += total;
    }
    if (threadIdx.x == 0) *after = (before ? *before : 0ull) + carry;
    if (edges) {
        const uint32_t nb = (uint32_t)(L < m - 1u ? L : m - 1u);     // (at most 255: one lane each)
        if (threadIdx.x < nb) {
            edges->head[threadIdx.x] = p[threadIdx.x];
            edges->tail[threadIdx.x] = p[L - nb + threadIdx.x];
        }
        if (threadIdx.x == 0) {
            edges->nedge = nb;
            edges->pad_ = 0;
        }
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIND_NT) void bzx_find_emit_kernel(const uint8_t *__restrict__ p, const uint64_t *__restrict__ len,
                                                                BzxFindPat pat, const uint32_t *__restrict__ sec,
                                                                const uint64_t *__restrict__ before,
                                                                const uint64_t *__restrict__ after, uint64_t skip, uint32_t cap,
                                                                uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_pat[BZX_FIND_MAX_PATTERN / 4];
    find_stage_pattern(pat, s_pat);
    const FindRun R = find_run(p, *len, pat.m, s_pat);
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    const uint64_t k0 = before ? *before : 0ull, k1 = *after;
    for (uint32_t t = blockIdx.x; t * 4u < R.nsec; t += gridDim.x) {
        const uint32_t s = t * 4u + wave;
        if (s >= R.nsec) continue;                           // (uniform over the wave, as is everything up to the walk)
        uint64_t k = k0 + sec[s];
        const uint64_t kend = s + 1u < R.nsec ? k0 + sec[s + 1u] : k1;
        if (k == kend || kend <= skip || (k >= skip && k - skip >= cap)) continue;
        for (uint32_t step = 0; step < FIND_STEPS; step++) {
            int64_t lo;
            uint32_t mask = find_mask16<false>(R, reinterpret_cast<const uint8_t *>(s_pat), (s * FIND_STEPS + step) * 64u + lane, &lo);
            const uint32_t mine = (uint32_t)__popc(mask);
            const uint32_t incl = bzx_wave_incl_sum(mine);
            const uint32_t tot = bzx_bcast63(incl);
            uint64_t kk = k + (incl - mine);
            for (; mask; mask &= mask - 1u, kk++)
                if (kk >= skip && kk - skip < cap) out[kk - skip] = (uint32_t)(lo + ((uint32_t)__ffs(mask) - 1u));
            k += tot;
        }
    }
}

// ---- the lines forms ---------------------------------------------------------------------------------------------------------
// Sections of the delimiter counts: the whole run, frame bytes [a, a + L).
__device__ __forceinline__ uint32_t find_dsections(uint32_t a, uint64_t len)
{
    return (uint32_t)((a + len + FIND_SEC_BYTES - 1) / FIND_SEC_BYTES);
}

__global__ __launch_bounds__(FIND_NT) void bzx_find_count_lines_kernel(const uint8_t *__restrict__ p, const uint64_t *__restrict__ len,
                                                                       BzxFindPat pat, uint32_t delim, uint32_t *__restrict__ sec,
                                                                       uint32_t *__restrict__ dsec)
{
    __shared__ uint32_t s_pat[BZX_FIND_MAX_PATTERN / 4];
    find_stage_pattern(pat, s_pat);
    const FindRun R = find_run(p, *len, pat.m, s_pat);
    const uint32_t ndsec = find_dsections(R.a, (uint64_t)R.len), drep = bzx_rep4(delim);
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    for (uint32_t t = blockIdx.x; t * 4u < ndsec; t += gridDim.x) {
        const uint32_t s = t * 4u + wave;
        if (s >= ndsec) continue;                            // (uniform over the wave)
        uint32_t acc = 0, dacc = 0;
        for (uint32_t step = 0; step < FIND_STEPS; step++) {
            int64_t lo;
            uint32_t dmask;
            acc += (uint32_t)__popc(find_mask16<true>(R, reinterpret_cast<const uint8_t *>(s_pat), (s * FIND_STEPS + step) * 64u + lane,
                                                      &lo, drep, &dmask));
            dacc += (uint32_t)__popc(dmask);
        }
        const uint32_t incl = bzx_wave_incl_sum(acc), dincl = bzx_wave_incl_sum(dacc);
        if (lane == 63) {
            if (s < R.nsec) sec[s] = incl;
            dsec[s] = dincl;
        }
    }
}

// One workgroup: the plain scan, then the same over dsec[]; *dafter = the run's delimiters.
__global__ __launch_bounds__(FIND_NT) void bzx_find_scan_lines_kernel(const uint8_t *__restrict__ p, const uint64_t *__restrict__ len,
                                                                      uint32_t m, uint32_t *__restrict__ sec, uint32_t *__restrict__ dsec,
                                                                      const uint64_t *__restrict__ before, uint64_t *__restrict__ after,
                                                                      uint64_t *__restrict__ dafter, BzxFindOut *__restrict__ edges)
{
    __shared__ uint32_t s_scr[FIND_NT / 64];
    const uint64_t L = *len;
    const uint32_t a = (uint32_t)((uintptr_t)p & 15u);
    const uint32_t nsec = L >= m ? (uint32_t)((a + (L - m + 1) + FIND_SEC_BYTES - 1) / FIND_SEC_BYTES) : 0u;
    const uint32_t ndsec = find_dsections(a, L);
    uint64_t carry = 0, dcarry = 0;
    for (uint32_t base = 0; base < ndsec; base += FIND_NT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nsec ? sec[i] : 0u, dv = i < ndsec ? dsec[i] : 0u;
        uint32_t total, dtotal;
        const uint32_t excl = bzx_block_excl_sum<FIND_NT>(v, s_scr, total);
        const uint32_t dexcl = bzx_block_excl_sum<FIND_NT>(dv, s_scr, dtotal);
        if (i < nsec) sec[i] = (uint32_t)carry + excl;      // (a run is shorter than 2^32 bytes, and so are its counts)
        if (i < ndsec) dsec[i] = (uint32_t)dcarry + dexcl;
        carry += total;
        dcarry += dtotal;
    }
    if (threadIdx.x == 0) {
        *after = (before ? *before : 0ull) + carry;
        *dafter = dcarry;
    }
    if (edges) {
        const uint32_t nb = (uint32_t)(L < m - 1u ? L : m - 1u);     // (at most 255: one lane each)
        if (threadIdx.x < nb) {
            edges->head[threadIdx.x] = p[threadIdx.x];
            edges->tail[threadIdx.x] = p[L - nb + threadIdx.x];
        }
        if (threadIdx.x == 0) {
            edges->nedge = nb;
            edges->pad_ = 0;
        }
    }
}

__global__ __launch_bounds__(FIND_NT) void bzx_find_emit_lines_kernel(const uint8_t *__restrict__ p, const uint64_t *__restrict__ len,
                                                                      BzxFindPat pat, uint32_t delim, const uint32_t *__restrict__ sec,
                                                                      const uint32_t *__restrict__ dsec,
                                                                      const uint64_t *__restrict__ before,
                                                                      const uint64_t *__restrict__ after, uint64_t skip, uint32_t cap,
                                                                      uint32_t *__restrict__ out, uint32_t *__restrict__ lines_out)
{
    __shared__ uint32_t s_pat[BZX_FIND_MAX_PATTERN / 4];
    find_stage_pattern(pat, s_pat);
    const FindRun R = find_run(p, *len, pat.m, s_pat);
    const uint32_t drep = bzx_rep4(delim);
    const uint32_t lane = bzx_lane(), wave = bzx_wave();
    const uint64_t k0 = before ? *before : 0ull, k1 = *after;
    for (uint32_t t = blockIdx.x; t * 4u < R.nsec; t += gridDim.x) {
        const uint32_t s = t * 4u + wave;
        if (s >= R.nsec) continue;                           // (uniform over the wave, as is everything up to the walk)
        uint64_t k = k0 + sec[s];
        const uint64_t kend = s + 1u < R.nsec ? k0 + sec[s + 1u] : k1;
        if (k == kend || kend <= skip || (k >= skip && k - skip >= cap)) continue;
        uint32_t d = dsec[s];                                // the run's delimiters in front of the section, then of the step
        for (uint32_t step = 0; step < FIND_STEPS; step++) {
            int64_t lo;
            uint32_t dmask;
            uint32_t mask = find_mask16<true>(R, reinterpret_cast<const uint8_t *>(s_pat), (s * FIND_STEPS + step) * 64u + lane, &lo,
                                              drep, &dmask);
            const uint32_t mine = (uint32_t)__popc(mask), dmine = (uint32_t)__popc(dmask);
            const uint32_t incl = bzx_wave_incl_sum(mine), dincl = bzx_wave_incl_sum(dmine);
            const uint32_t tot = bzx_bcast63(incl), dtot = bzx_bcast63(dincl);
            const uint32_t dd = d + (dincl - dmine);         // ... in front of the lane's chunk
            uint64_t kk = k + (incl - mine);
            for (; mask; mask &= mask - 1u, kk++)
                if (kk >= skip && kk - skip < cap) {
                    const uint32_t j = (uint32_t)__ffs(mask) - 1u;
                    out[kk - skip] = (uint32_t)(lo + j);
                    lines_out[kk - skip] = dd + (uint32_t)__popc(dmask & ((1u << j) - 1u));
                }
            k += tot;
            d += dtot;
        }
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------------
// Workgroups for a run of at most `len` bytes: one per tile, up to eight per compute unit.
uint32_t bzx_find_grid(uint64_t len, uint32_t n_cu)
{
    const uint64_t ntile = (len + 15 + FIND_TILE_BYTES - 1) / FIND_TILE_BYTES, g = (uint64_t)n_cu * 8;
    return (uint32_t)std::max<uint64_t>(1, std::min(ntile, g));
}

void bzx_launch_find_count(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, uint32_t *sec, uint32_t grid,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_find_count_kernel, dim3(grid), dim3(FIND_NT), 0, stream, p, len, pat, sec);
}

void bzx_launch_find_scan(const uint8_t *p, const uint64_t *len, uint32_t m, uint32_t *sec, const uint64_t *before,
                          uint64_t *after, BzxFindOut *edges, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_find_scan_kernel, dim3(1), dim3(FIND_NT), 0, stream, p, len, m, sec, before, after, edges);
}

void bzx_launch_find_emit(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, const uint32_t *sec,
                          const uint64_t *before, const uint64_t *after, uint64_t skip, uint32_t cap, uint32_t *out,
                          uint32_t grid, hipStream_t stream)
{
    if (!cap) return;
    hipLaunchKernelGGL(bzx_find_emit_kernel, dim3(grid), dim3(FIND_NT), 0, stream, p, len, pat, sec, before, after, skip, cap, out);
}

void bzx_launch_find_count_lines(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, uint32_t delim, uint32_t *sec,
                                 uint32_t *dsec, uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_find_count_lines_kernel, dim3(grid), dim3(FIND_NT), 0, stream, p, len, pat, delim, sec, dsec);
}

void bzx_launch_find_scan_lines(const uint8_t *p, const uint64_t *len, uint32_t m, uint32_t *sec, uint32_t *dsec,
                                const uint64_t *before, uint64_t *after, uint64_t *dafter, BzxFindOut *edges, hipStream_t stream)
{
    hipLaunchKernelGGL(bzx_find_scan_lines_kernel, dim3(1), dim3(FIND_NT), 0, stream, p, len, m, sec, dsec, before, after, dafter, edges);
}

void bzx_launch_find_emit_lines(const uint8_t *p, const uint64_t *len, const BzxFindPat &pat, uint32_t delim, const uint32_t *sec,
                                const uint32_t *dsec, const uint64_t *before, const uint64_t *after, uint64_t skip, uint32_t cap,
                                uint32_t *out, uint32_t *lines_out, uint32_t grid, hipStream_t stream)
{
    if (!cap) return;
    hipLaunchKernelGGL(bzx_find_emit_lines_kernel, dim3(grid), dim3(FIND_NT), 0, stream, p, len, pat, delim, sec, dsec, before, after,
                       skip, cap, out, lines_out);
}

extern "C" void bzx_find_geometry(uint32_t *tile_bytes, uint32_t *inline_hits, uint32_t *window_hits)
{
    if (tile_bytes) *tile_bytes = FIND_TILE_BYTES;
    if (inline_hits) *inline_hits = FIND_INLINE_HITS;
    if (window_hits) *window_hits = FIND_WINDOW_HITS;
}

// ---- the kernels alone, for the parity tests (host pointers) -----------------------------------------------------------------
// Segment i is a run of its own; d_run[i] = the hits of the segments before it, so the numbering of the emit kernel runs
// through all segments.  Everything is enqueued without a synchronisation in between.  delim >= 0: the lines forms;
// d_dtot[i] = the delimiters of segment i, and a hit's line counts those of its own segment only.
static int stage_find(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                      const uint64_t *seg_lens, const BzxFindPat &pat, uint64_t skip, uint32_t cap, uint32_t *counts_out,
                      uint64_t *hits_out, uint32_t *nwritten, int delim = -1, uint32_t *dcounts_out = nullptr,
                      uint64_t *lines_out = nullptr)
{
    const bool lines = delim >= 0;
    uint64_t longest = 0;
    for (uint32_t i = 0; i < nseg; i++) {
        if (seg_offs[i] > len || seg_lens[i] > len - seg_offs[i] || seg_lens[i] > 0xFFFFFFFFull) {
            ctx->err = std::string(lines ? "bzx_stage_find_lines" : "bzx_stage_find") + ": segment " + std::to_string(i) + " leaves the buffer";
            return BZX_E_PARAM;
        }
        longest = std::max(longest, seg_lens[i]);
    }
    *nwritten = 0;
    if (!nseg) return BZX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevMem<> d_buf, d_tab;                       // (freed on return: every path below ends behind a synchronisation)
    uint64_t *d_len = nullptr, *d_run = nullptr, *d_dtot = nullptr;
    uint32_t *d_sec = nullptr, *d_out = nullptr, *d_dsec = nullptr, *d_lout = nullptr;
    const bool ok = d_buf.reserve(len + 512) && carved(d_tab, 256, [&](Carver &c) {
        d_len = c.take<uint64_t>(nseg);
        d_run = c.take<uint64_t>((size_t)nseg + 1);
        d_sec = c.take<uint32_t>(bzx_find_sections(longest));
        d_out = c.take<uint32_t>(std::max<uint32_t>(cap, 1));
        if (lines) {
            d_dtot = c.take<uint64_t>(nseg);
            d_dsec = c.take<uint32_t>(bzx_find_sections(longest));
            d_lout = c.take<uint32_t>(std::max<uint32_t>(cap, 1));
        }
    });
    if (!ok) {
        ctx->err = "bzx_stage_find: device allocation failed";
        return BZX_E_NOMEM;
    }
    uint8_t *d = (uint8_t *)rg_al((size_t)(uintptr_t)d_buf.get());
    auto run = [&]() -> int {
        std::vector<uint64_t> total((size_t)nseg + 1);
        std::vector<uint32_t> got(cap), lgot(lines ? cap : 0);
        std::vector<uint64_t> dtot(lines ? nseg : 0);
        if (len) HIP_TRY(ctx, hipMemcpyAsync(d, buf, len, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_len, seg_lens, (size_t)nseg * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(d_run, 0, 8, st));
        if (cap) HIP_TRY(ctx, hipMemsetAsync(d_out, 0xEE, (size_t)cap * 4, st));
        if (cap && lines) HIP_TRY(ctx, hipMemsetAsync(d_lout, 0xEE, (size_t)cap * 4, st));
        for (uint32_t i = 0; i < nseg; i++) {
            const uint32_t grid = bzx_find_grid(seg_lens[i], (uint32_t)ctx->n_cu);
            if (lines) {
                bzx_launch_find_count_lines(d + seg_offs[i], d_len + i, pat, (uint32_t)delim, d_sec, d_dsec, grid, st);
                bzx_launch_find_scan_lines(d + seg_offs[i], d_len + i, pat.m, d_sec, d_dsec, d_run + i, d_run + i + 1, d_dtot + i,
                                           nullptr, st);
                bzx_launch_find_emit_lines(d + seg_offs[i], d_len + i, pat, (uint32_t)delim, d_sec, d_dsec, d_run + i, d_run + i + 1,
                                           skip, cap, d_out, d_lout, grid, st);
                continue;
            }
            bzx_launch_find_count(d + seg_offs[i], d_len + i, pat, d_sec, grid, st);
            bzx_launch_find_scan(d + seg_offs[i], d_len + i, pat.m, d_sec, d_run + i, d_run + i + 1, nullptr, st);
            bzx_launch_find_emit(d + seg_offs[i], d_len + i, pat, d_sec, d_run + i, d_run + i + 1, skip, cap, d_out, grid, st);
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(total.data(), d_run, ((size_t)nseg + 1) * 8, hipMemcpyDeviceToHost, st));
        if (cap) HIP_TRY(ctx, hipMemcpyAsync(got.data(), d_out, (size_t)cap * 4, hipMemcpyDeviceToHost, st));
        if (lines) HIP_TRY(ctx, hipMemcpyAsync(dtot.data(), d_dtot, (size_t)nseg * 8, hipMemcpyDeviceToHost, st));
        if (cap && lines) HIP_TRY(ctx, hipMemcpyAsync(lgot.data(), d_lout, (size_t)cap * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < nseg; i++) counts_out[i] = (uint32_t)(total[i + 1] - total[i]);
        for (uint32_t i = 0; lines && i < nseg; i++) dcounts_out[i] = (uint32_t)dtot[i];
        const uint64_t all = total[nseg];
        const uint32_t n = (uint32_t)(all > skip ? std::min<uint64_t>(all - skip, cap) : 0);
        for (uint32_t i = 0; i < n; i++) hits_out[i] = got[i];
        for (uint32_t i = 0; lines && i < n; i++) lines_out[i] = lgot[i];
        *nwritten = n;
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

// The pattern as the kernels take it; false: NULL, m == 0 or m > BZX_FIND_MAX_PATTERN.
bool bzx_find_pattern(const uint8_t *pat, size_t m, BzxFindPat *out)
{
    if (!pat || m == 0 || m > BZX_FIND_MAX_PATTERN) return false;
    memset(out, 0, sizeof(*out));
    memcpy(out->w, pat, m);
    out->m = (uint32_t)m;
    return true;
}

extern "C" int bzx_stage_find(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                              const uint64_t *seg_lens, const uint8_t *pat, size_t m, uint64_t skip, uint32_t cap,
                              uint32_t *counts_out, uint64_t *hits_out, uint32_t *nwritten)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    BzxFindPat fp;
    if (!ctx || !nwritten || (len && !buf) || (nseg && (!seg_offs || !seg_lens || !counts_out)) || (cap && !hits_out) ||
        !bzx_find_pattern(pat, m, &fp))
        return BZX_E_PARAM;
    return stage_find(ctx, buf, len, nseg, seg_offs, seg_lens, fp, skip, cap, counts_out, hits_out, nwritten);
}

extern "C" int bzx_stage_find_lines(bzx_ctx *ctx, const uint8_t *buf, size_t len, uint32_t nseg, const uint64_t *seg_offs,
                                    const uint64_t *seg_lens, const uint8_t *pat, size_t m, int delim, uint64_t skip, uint32_t cap,
                                    uint32_t *counts_out, uint32_t *dcounts_out, uint64_t *hits_out, uint64_t *lines_out,
                                    uint32_t *nwritten)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    BzxFindPat fp;
    if (!ctx || !nwritten || (len && !buf) || (nseg && (!seg_offs || !seg_lens || !counts_out || !dcounts_out)) ||
        (cap && (!hits_out || !lines_out)) || delim < 0 || delim > 255 || !bzx_find_pattern(pat, m, &fp))
        return BZX_E_PARAM;
    return stage_find(ctx, buf, len, nseg, seg_offs, seg_lens, fp, skip, cap, counts_out, hits_out, nwritten, delim, dcounts_out,
                      lines_out);
}
