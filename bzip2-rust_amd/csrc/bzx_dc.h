// bzx_dc.h -- what the decoders (bzx_dbatch.hip: one-shot and batch; bzx_dstream.hip) share besides the block kernels
// of bzx_decomp.hip: the stream-header test, the magic scan of one word, and the reasons an input is refused.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "bzx_device.h"

// Level 1..9 of the stream header "BZh1".."BZh9" at p[0..4), 0: none.
__host__ __device__ inline uint32_t bzx_bzh_level(const uint8_t *p)
{
    return (p[0] == 'B' && p[1] == 'Z' && p[2] == 'h' && p[3] >= '1' && p[3] <= '9') ? (uint32_t)(p[3] - '0') : 0u;
}

// Tests the 32 bit offsets of the 4-byte word at z[byte0] for the block / end-of-stream magic (blocks start at any
// bit); nothing at or past z + len is read, and a magic that does not end inside z[0, len) is no hit.  Every hit goes
// to hit(bit, is_eos, x, y): bit = its offset in z, x = the 64 bits from there on (the magic and the 16 bits behind
// it), y = the bits behind x, left-aligned (64 - bit % 32 of them, then zeros).
template <class F>
__device__ __forceinline__ void bzx_dc_scan_word(const uint8_t *__restrict__ z, uint64_t len, uint64_t byte0, F &&hit)
{
    uint64_t hi = 0, lo = 0;                            // bytes byte0 .. byte0+15, big-endian
#pragma unroll
    for (int i = 0; i < 8; i++) hi = (hi << 8) | (byte0 + i < len ? z[byte0 + i] : 0u);
#pragma unroll
    for (int i = 8; i < 16; i++) lo = (lo << 8) | (byte0 + i < len ? z[byte0 + i] : 0u);
#pragma unroll
    for (uint32_t s = 0; s < 32; s++) {
        const uint64_t x = s ? (hi << s) | (lo >> (64 - s)) : hi;
        const uint64_t v = x >> 16;
        const uint64_t bit = byte0 * 8 + s;
        if ((v == DC_MAGIC_BLOCK || v == DC_MAGIC_EOS) && bit + 48 <= len * 8) hit(bit, v == DC_MAGIC_EOS, x, lo << s);
    }
}

// Why an input is refused.  The same damage is named in the same words by the one-shot calls, the batch and the stream.
enum DcWhy : uint32_t {
    DC_OK = 0,
    DC_WHY_SHORT,
    DC_WHY_NO_HEADER,
    DC_WHY_NO_EOS,
    DC_WHY_RANDOMISED,
    DC_WHY_DAMAGED,
    DC_WHY_TRUNC_EOS,
    DC_WHY_IBWT,
    DC_WHY_OUTBUF,
    DC_WHY_BLOCK_CRC,          // (followed by the number of the block within its input)
    DC_WHY_COMBINED_CRC,
    DC_WHY_STREAM_FOLLOWS,
};

inline std::string dc_why_text(uint32_t why, uint32_t block = 0)
{
    static const char *const text[] = {
        "",
        "shorter than the smallest bzip2 stream",
        "no BZh1..BZh9 header",
        "blocks do not end at an end-of-stream marker",
        "randomised block (written by bzip2 0.9.0 or older): not supported",
        "damaged block in the bzip2 stream",
        "truncated after the end-of-stream marker",
        "damaged block in the bzip2 stream (inverse BWT)",
        "output buffer too small for the decompressed data",
        "block CRC mismatch in block ",
        "combined CRC mismatch",
        "another bzip2 stream follows the first (concatenated .bz2): bzx_decompress_buffer decodes all of them",
    };
    return why == DC_WHY_BLOCK_CRC ? text[why] + std::to_string(block) : std::string(text[why]);
}
