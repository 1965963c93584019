// bzx_api.hip -- C ABI (include/bzx.h): the context, the stage runner, the stage and per-block entry points,
// bzx_compress_device, the split entry points and sharding.  Batches, decompression and the chunked stream compressor
// have their host side next to their kernels (bzx_batch.hip, bzx_decomp.hip, bzx_cstream.hip).
//
// Host side of the boundary described in include/bzx.h.  Mirrors the reference's driver
// (src/compression/compress.rs:40-136) but batch-shaped: every stage kernel runs once over
// all blocks of the batch, one workgroup per block, on one HIP stream; HIP events around
// each stage feed bzx_stats.  No CPU implementation of any stage exists here.
#include <string.h>
#include <chrono>
#include <new>
#include "bzx_host.h"
#include "bzx_wg.h"

extern "C" const char *bzx_version(void) { return "bzx 0.1 (gfx950)"; }

extern "C" const char *bzx_strerror(int code)
{
    switch (code) {
    case BZX_OK: return "ok";
    case BZX_E_NODEVICE: return "no HIP device";
    case BZX_E_PARAM: return "bad parameter";
    case BZX_E_NOMEM: return "out of memory";
    case BZX_E_OUTBUF: return "output buffer too small";
    case BZX_E_HIP: return "HIP runtime error";
    case BZX_E_STATE: return "bad call sequence";
    case BZX_E_DATA: return "damaged or invalid bzip2 data";
    default: return "unknown error";
    }
}

extern "C" const char *bzx_last_error(const bzx_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

template <typename T> static int dev_alloc(bzx_ctx *ctx, std::vector<DevMem<>> &owner, T **p, size_t count)
{
    DevMem<> m;
    if (!m.reserve(count * sizeof(T))) {
        ctx->err = std::string("hipMalloc: ") + hipGetErrorString(hipGetLastError());
        return BZX_E_NOMEM;
    }
    *p = m.get<T>();
    owner.push_back(std::move(m));
    return BZX_OK;
}

// Block descriptors for `nblk` blocks (global block numbers) and per-block slabs for `nslab` of them (the blocks
// this context owns: all of them, or every world-th one of a sharded run -- BZX_SLAB in bzx_device.h).
int ensure_blocks(bzx_ctx *ctx, uint32_t nblk, uint32_t nslab)
{
    if (nslab == 0 || nslab > nblk) nslab = nblk;
    BzxBatch &B = ctx->B;
    int rc;
    if (nblk > ctx->cap_blocks) {
        ctx->descs.clear();
        ctx->cap_blocks = 0;
        const uint32_t cap = nblk < 16 ? 16 : nblk;
        if ((rc = dev_alloc(ctx, ctx->descs, &B.blk, cap))) return rc;
        if ((rc = dev_alloc(ctx, ctx->descs, &B.plist, (size_t)cap))) return rc;
        if ((rc = dev_alloc(ctx, ctx->descs, &B.redo_list, (size_t)cap))) return rc;
        if ((rc = dev_alloc(ctx, ctx->descs, &B.resume_list, (size_t)cap))) return rc;
        if (!ctx->h_blk.reserve((size_t)cap * sizeof(BzxBlock))) {
            ctx->err = "hipHostMalloc(block descriptors) failed";
            return BZX_E_NOMEM;
        }
        ctx->cap_blocks = cap;
    }
    if (nslab <= ctx->cap_slabs) return BZX_OK;
    ctx->slabs.clear();
    ctx->cap_slabs = 0;
    const uint32_t cap = nslab < 16 ? 16 : nslab;
    if ((rc = dev_alloc(ctx, ctx->slabs, &ctx->d_in, (size_t)cap * BZX_BLK_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.bwt, (size_t)cap * BZX_BLK_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.rank, (size_t)cap * BZX_BLK_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.mtfv, (size_t)cap * BZX_BLK_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.freq, (size_t)cap * 260))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.in_use, (size_t)cap * 256))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.len, (size_t)cap * 6 * 260))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.code, (size_t)cap * 6 * 260))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.selector, (size_t)cap * BZX_SEL_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.selector_mtf, (size_t)cap * BZX_SEL_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.gbits, (size_t)cap * BZX_SEL_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.tbits, (size_t)cap * BZX_TILE_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.pk, (size_t)cap * BZX_PK_STRIDE))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.rec_a, (size_t)cap * BZX_MAX_N))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.rec_b, (size_t)cap * BZX_MAX_N))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.bk_list, (size_t)cap * BZX_BK_PER_BLOCK))) return rc;
    B.bk_cap = cap * BZX_BK_PER_BLOCK;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.rk_list, (size_t)B.bk_cap * 2))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.deep_list, (size_t)cap * BZX_DEEP_PER_BLOCK * 4 * 3))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slabs, &B.isa2, (size_t)cap * 2 * BZX_MAX_N))) return rc;
    B.rk_blocks = cap;
    // MTF stage: positions of the run heads, 4 B each and one more.  They live in the block's record slab (8 B per
    // rotation, dead once the BWT of the block is done).
    B.hpos = reinterpret_cast<uint32_t *>(B.rec_a);
    B.hpos_stride = 2 * BZX_MAX_N;
    if ((rc = dev_alloc(ctx, ctx->slabs, &ctx->d_outbuf, (size_t)cap * (BZX_OUT_STRIDE / 4)))) return rc;
    ctx->cap_slabs = cap;
    return BZX_OK;
}

static int ensure_slots(bzx_ctx *ctx, uint32_t n_slots)
{
    if (n_slots <= ctx->n_slots) return BZX_OK;
    ctx->slot_allocs.clear();
    ctx->n_slots = 0;
    std::vector<BzxSortWs> h(n_slots);
    int rc;
    // one slab per array kind, carved per slot (a few large allocations instead of thousands)
    uint64_t *u = nullptr;
    uint32_t *w = nullptr;
    if ((rc = dev_alloc(ctx, ctx->slot_allocs, &u, (size_t)n_slots * 2 * BZX_MAX_N))) return rc;
    if ((rc = dev_alloc(ctx, ctx->slot_allocs, &w, (size_t)n_slots * 4 * BZX_MAX_N))) return rc;
    for (uint32_t i = 0; i < n_slots; i++) {
        h[i].u0 = u + (size_t)i * 2 * BZX_MAX_N;
        h[i].u1 = h[i].u0 + BZX_MAX_N;
        h[i].s0 = w + (size_t)i * 4 * BZX_MAX_N;
        h[i].s1 = h[i].s0 + BZX_MAX_N;
        h[i].isa = h[i].s1 + BZX_MAX_N;
        h[i].sa = h[i].isa + BZX_MAX_N;
    }
    if ((rc = dev_alloc(ctx, ctx->slot_allocs, &ctx->B.sort_ws, (size_t)n_slots))) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->B.sort_ws, h.data(), n_slots * sizeof(BzxSortWs), hipMemcpyHostToDevice));
    ctx->n_slots = n_slots;
    ctx->B.n_slots = n_slots;
    return BZX_OK;
}

extern "C" int bzx_ctx_create(int device, uint32_t max_blocks, bzx_ctx **out)
{
    if (!out) return BZX_E_PARAM;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BZX_E_NODEVICE;
    if (hipSetDevice(device) != hipSuccess) return BZX_E_NODEVICE;
    bzx_ctx *ctx = new (std::nothrow) bzx_ctx();
    if (!ctx) return BZX_E_NOMEM;
    memset(&ctx->B, 0, sizeof(ctx->B));
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        delete ctx;
        return BZX_E_NODEVICE;
    }
    ctx->n_cu = prop.multiProcessorCount;
    if (hipStreamCreate(&ctx->stream) != hipSuccess) {
        delete ctx;
        return BZX_E_NODEVICE;
    }
    ctx->own_stream = true;
    for (int i = 0; i < 8; i++) (void)hipEventCreate(&ctx->ev[i]);
    // A stream of another priority gets a hardware queue of its own; with the default priority HIP may map it onto
    // the queue of the caller's stream (it does once RCCL has created its streams), which would serialise the
    // early general-sorter launch behind the bucket sort instead of running it beside it.
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&ctx->aux, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
        hipEventCreate(&ctx->ev_join) != hipSuccess || hipEventCreate(&ctx->ev_b1) != hipSuccess ||
        hipEventCreate(&ctx->ev_b2) != hipSuccess || hipEventCreate(&ctx->ev_b3) != hipSuccess ||
        hipEventCreate(&ctx->ev_b4) != hipSuccess || hipEventCreate(&ctx->ev_bt[0]) != hipSuccess ||
        hipEventCreate(&ctx->ev_bt[1]) != hipSuccess || hipEventCreate(&ctx->ev_bt[2]) != hipSuccess) {
        bzx_ctx_destroy(ctx);
        return BZX_E_HIP;
    }
    bool ok = ctx->d_counters.reserve(BZX_N_COUNTERS * sizeof(uint32_t)) && ctx->d_scalars.reserve(8 * sizeof(uint64_t)) &&
              ctx->h_scalars.reserve(8 * sizeof(uint64_t)) && ctx->h_counters.reserve(64 * sizeof(uint32_t));
    if (!ok || ensure_blocks(ctx, max_blocks ? max_blocks : 16) != BZX_OK) {
        bzx_ctx_destroy(ctx);
        return BZX_E_NOMEM;
    }
    *out = ctx;
    return BZX_OK;
}

extern "C" void bzx_ctx_destroy(bzx_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->cs) {
        bzx_cstream_end(ctx->cs);
        ctx->cs = nullptr;
    }
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
    // (the device is current and both streams are idle: `delete` below frees every buffer the context owns)
    if (ctx->ev_b1) (void)hipEventDestroy(ctx->ev_b1);
    if (ctx->ev_b2) (void)hipEventDestroy(ctx->ev_b2);
    if (ctx->ev_b3) (void)hipEventDestroy(ctx->ev_b3);
    if (ctx->ev_b4) (void)hipEventDestroy(ctx->ev_b4);
    for (int i = 0; i < 3; i++)
        if (ctx->ev_bt[i]) (void)hipEventDestroy(ctx->ev_bt[i]);
    for (int i = 0; i < 8; i++) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int bzx_ctx_set_stream(bzx_ctx *ctx, void *hip_stream)
{
    if (!ctx) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(ctx->api_mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    return BZX_OK;
}

extern "C" int bzx_get_stats(const bzx_ctx *ctx, bzx_stats *out)
{
    if (!ctx || !out) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(const_cast<bzx_ctx *>(ctx)->api_mu);
    *out = ctx->stats;
    return BZX_OK;
}

static void block_info_of(const BzxBlock &d, bzx_block_info *out)
{
    out->n = d.n;
    out->crc = d.crc;
    out->orig_ptr = d.orig_ptr;
    out->periodic = (d.status & BZX_ST_PERIODIC) ? 1u : 0u;
    out->n_in_use = d.n_in_use;
    out->n_mtf = d.n_mtf;
    out->n_tables = d.n_groups;
    out->n_selectors = d.n_selectors;
    out->bits_selectors = d.sec_bits[0];
    out->bits_tables = d.sec_bits[1];
    out->bits_payload = d.sec_bits[2];
    out->bits_symbol_map = d.sec_bits[3];
    out->bits = d.bits;
}

extern "C" int bzx_get_block_info(const bzx_ctx *ctx, uint32_t block, bzx_block_info *out)
{
    if (!ctx || !out) return BZX_E_PARAM;
    std::unique_lock<std::recursive_mutex> api_lock_(const_cast<bzx_ctx *>(ctx)->api_mu);
    if (ctx->stats_batch) return BZX_E_STATE;
    if (!ctx->h_blk || block >= ctx->stats.nblk || block >= ctx->cap_blocks) return BZX_E_PARAM;
    block_info_of(ctx->h_blk[block], out);
    return BZX_OK;
}



// Runs the stage kernels over blocks [0,nblk) whose descriptors (in_off,n,crc) are already on the device.
// STG_EMIT: out_level == 0 -> every block image byte-aligned in its own slab of ctx->d_outbuf;
//           out_level 1..9 -> one .bz2 stream in d_stream_out (cap bytes, device memory).
//           out_level -1   -> one CHUNK of a stream (bzx_cstream_*): the block images back to back in d_stream_out,
//                             starting at the bit phase d_phase[0] (kept on the device from chunk to chunk); no header,
//                             no footer, no host synchronisation
int run_stages(bzx_ctx *ctx, uint32_t nblk, int stages, int out_level, void *d_stream_out, size_t stream_cap,
               uint64_t *d_phase)
{
    BzxBatch &B = ctx->B;
    B.nblk = nblk;
    B.counters = ctx->d_counters;
    if (B.blk_step == 0) B.blk_step = 1;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, BZX_N_COUNTERS * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    ctx->bsort_used = false;
    if ((stages & STG_BWT) && nblk) {
        // bucket sorter: split every block into LDS-sized buckets, sort the buckets (any workgroup, any block), then
        // the general sorter takes the blocks that were handed over (deep repeats, periodic blocks); usually none
        const uint32_t ncu = (uint32_t)ctx->n_cu;
        uint32_t per_cu = bzx_bwt_max_blocks_per_cu();
        int rc = ensure_slots(ctx, ncu * per_cu);
        if (rc) return rc;
        // this launch's share of the bucket work lists: eight lists of items / 8 (cap_slabs >= 16, so at least 4096 each);
        // ALL of it is zeroed, so an item the split kernel reserved but did not write is an empty one
        const size_t cap_all = (size_t)ctx->cap_slabs * BZX_BK_PER_BLOCK;
        const size_t want = (size_t)(nblk < 16 ? 16 : nblk) * BZX_BK_PER_BLOCK;       // (a lone repetitive block emits thousands of one-bucket splits)
        const size_t items = (want < cap_all ? want : cap_all) & ~(size_t)7;
        B.bk_cap = (uint32_t)items;
        // few blocks: their buckets are dealt over all eight lists, so that every compute unit gets work; many: a list
        // holds whole blocks (one L2 per block)
        B.bk_affine = nblk >= 64 ? 1u : 0u;
        HIP_TRY(ctx, hipMemsetAsync(B.bk_list, 0, items * sizeof(BzxBucket), ctx->stream));
        // the two lists of oversized bins (deeper split levels): zeroed, an item reserved but not written is an empty one
        const size_t deep_all = (size_t)ctx->cap_slabs * BZX_DEEP_PER_BLOCK;
        B.deep_cap = (uint32_t)((size_t)nblk * BZX_DEEP_PER_BLOCK < deep_all ? (size_t)nblk * BZX_DEEP_PER_BLOCK : deep_all);
        HIP_TRY(ctx, hipMemsetAsync(B.deep_list, 0, (size_t)B.deep_cap * 2 * 16, ctx->stream));
        bzx_launch_bsplit(B, nblk < ncu ? nblk : ncu, ncu, ctx->stream);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_b1, ctx->stream));
        // Blocks the split kernel refused (oversized bins beyond its depth / split limits: a handful in real data)
        // are sorted from scratch by the general sorter, one workgroup each, 10-60 ms: started right away on the
        // high-priority side stream, in sort slots of their own, beside the bucket sort of everything else.
        const bool early = ctx->n_slots >= 64;
        const uint32_t n_early = 32;
        B.rk_slot0 = 0;
        B.rk_blocks = ctx->cap_slabs;                               // every block in resume state gets its two rank arrays
#ifdef BZX_STRESS_FEW_RANK_ARRAYS                                   // (stress builds: only eight blocks get rank arrays)
        B.rk_blocks = 8;
#endif
        B.slot_base = 0;
        B.redo_once = 0;
        if (early) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_b1, 0));
            BzxBatch Be = B;
            Be.redo = 1;
            Be.ctr_bwt = BZX_CTR_REDO_FETCH;
            Be.redo_once = 1;
            bzx_launch_bwt(Be, n_early, ctx->aux);
            HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
        }
        B.bsort_mode = 0;
        bzx_launch_bsort(B, bzx_bsort_blocks_per_cu() * ncu, ctx->stream);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_b2, ctx->stream));
        ctx->bsort_used = true;
        // the blocks in which a bucket gave up (deep repeats): the fill pass writes the order of their finished
        // buckets and enters their ranks into the block's two rank arrays, the regrouping pass turns oversized groups
        // into ordinary items, prefix-tripling rank rounds over the open buckets finish the leftover groups -- any
        // workgroup on any bucket, each launch exits at once when nothing is open.  Then the general sorter takes what is
        // left: refused blocks beyond the early launch's 32, and resume blocks still open after the rank rounds (periodic
        // blocks, oversized groups the regrouping pass could not dissolve and the groups that read their coarse ranks,
        // stress builds: blocks without rank arrays).
        BzxBatch Bf = B;
        Bf.bsort_mode = 1;
        bzx_launch_bsort(Bf, bzx_bsort_blocks_per_cu() * ncu, ctx->stream);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_b3, ctx->stream));
        bzx_launch_bgiant(B, ncu, ctx->stream);                      // (a no-op launch unless the split left an oversized group)
        bzx_launch_brank(B, bzx_bsort_blocks_per_cu() * ncu, ctx->stream);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_b4, ctx->stream));
        if (early) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        BzxBatch Br = B;
        Br.redo = 1;
        Br.ctr_bwt = BZX_CTR_REDO_FETCH;
        bzx_launch_bwt(Br, grid_for(ctx, nblk, per_cu), ctx->stream);
        Br.redo = 2;
        Br.ctr_bwt = BZX_CTR_RESUME_FETCH;
        bzx_launch_bwt(Br, grid_for(ctx, nblk, per_cu), ctx->stream);
        bzx_launch_periodic(B, ctx->n_slots < 64 ? ctx->n_slots : 64, ctx->stream);
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    if ((stages & STG_MTF) && nblk) bzx_launch_mtf(B, grid_for(ctx, nblk, 1), ctx->stream);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    if ((stages & STG_HUF) && nblk) bzx_launch_huffman(B, grid_for(ctx, nblk, 3), ctx->stream);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    if (stages & STG_EMIT) {
        if (out_level < 0) {
            B.out = (uint32_t *)d_stream_out;
            bzx_launch_layout(B, 0, 0, ctx->d_scalars, ctx->stream, d_phase);
            HIP_TRY(ctx, hipMemsetAsync(d_stream_out, 0, stream_cap, ctx->stream));
            if (nblk) bzx_launch_emit(B, (uint32_t)ctx->n_cu, ctx->stream);
        } else if (out_level == 0) {
            B.out = ctx->d_outbuf;
            bzx_launch_layout(B, 0, (uint64_t)BZX_OUT_STRIDE * 8, ctx->d_scalars, ctx->stream);
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_outbuf, 0, (size_t)nblk * BZX_OUT_STRIDE, ctx->stream));
            if (nblk) bzx_launch_emit(B, (uint32_t)ctx->n_cu, ctx->stream);
        } else {
            // sizes are known after the Huffman stage: lay the stream out, check it fits, then emit
            B.out = (uint32_t *)d_stream_out;
            bzx_launch_layout(B, 32, 0, ctx->d_scalars, ctx->stream);
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, sizeof(uint64_t), hipMemcpyDeviceToHost,
                                        ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            const uint64_t out_bytes = (ctx->h_scalars[0] + 80 + 7) >> 3;
            const uint64_t need = (out_bytes + 3) & ~3ull;
            ctx->h_scalars[1] = out_bytes;
            if (need > stream_cap) {
                ctx->err = "output buffer too small for the compressed stream";
                return BZX_E_OUTBUF;
            }
            HIP_TRY(ctx, hipMemsetAsync(d_stream_out, 0, need, ctx->stream));
            if (nblk) bzx_launch_emit(B, (uint32_t)ctx->n_cu, ctx->stream);
            bzx_launch_stream_frame(B, out_level, ctx->d_scalars, ctx->d_scalars + 1, ctx->stream);
        }
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    return BZX_OK;
}

int bzx_ctx_split_scratch(bzx_ctx *ctx, size_t bytes, void **p)
{
    if (!ctx->split_ws.reserve(bytes)) {
        ctx->err = "hipMalloc(split scratch) failed";
        return BZX_E_NOMEM;
    }
    *p = ctx->split_ws;
    return BZX_OK;
}

void collect_stage_times(bzx_ctx *ctx)
{
    float ms[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ctx->ev[i], ctx->ev[i + 1]);
    ctx->stats.ms_bwt = ms[0];
    ctx->stats.n_redo = 0;
    ctx->stats.n_buckets = 0;
    ctx->stats.ms_bwt_split = ctx->stats.ms_bwt_sort = ctx->stats.ms_bwt_general = ctx->stats.ms_bwt_rank = 0.f;
    ctx->stats.n_open_buckets = ctx->stats.n_open_left = ctx->stats.n_resume_left = ctx->stats.n_from_scratch = ctx->stats.n_unsorted = 0;
    if (ctx->bsort_used) {
        ctx->stats.n_redo = ctx->h_counters[BZX_CTR_REDO] + ctx->h_counters[BZX_CTR_RESUME];
        ctx->stats.n_buckets = 0;
        for (int x = 0; x < 8; x++) ctx->stats.n_buckets += ctx->h_counters[BZX_CTR_BK_LIST0 + x];
        (void)hipEventElapsedTime(&ctx->stats.ms_bwt_split, ctx->ev[0], ctx->ev_b1);
        (void)hipEventElapsedTime(&ctx->stats.ms_bwt_sort, ctx->ev_b1, ctx->ev_b2);
        (void)hipEventElapsedTime(&ctx->stats.ms_bwt_general, ctx->ev_b2, ctx->ev[1]);
        (void)hipEventElapsedTime(&ctx->stats.ms_bwt_rank, ctx->ev_b3, ctx->ev_b4);
        ctx->stats.n_open_buckets = ctx->h_counters[BZX_CTR_RK_ITEMS];
        ctx->stats.n_open_left = ctx->h_counters[BZX_CTR_RK_OPEN];
        ctx->stats.n_resume_left = ctx->h_counters[BZX_CTR_RESUME_LEFT];
        ctx->stats.n_from_scratch = ctx->h_counters[BZX_CTR_REDO];
        ctx->stats.n_unsorted = ctx->h_counters[BZX_CTR_STAT0 + 15];

    }
    ctx->stats.bwt_launches = 1;
    ctx->stats.ms_mtf = ms[1];
    ctx->stats.ms_huffman = ms[2];
    ctx->stats.ms_emit = ms[3];
}

// Adds the periodic flags, RLE1 bytes and MTF symbols of the descriptors blk[first], blk[first + step], ... below end.
void fold_blocks(bzx_stats &st, const BzxBlock *blk, uint32_t first, uint32_t end, uint32_t step)
{
    for (uint32_t b = first; b < end; b += step) {
        st.n_periodic += (blk[b].status & BZX_ST_PERIODIC) ? 1 : 0;
        st.rle1_bytes += blk[b].n;
        st.mtf_symbols += blk[b].n_mtf;
    }
}

static int check_blk_args(const uint8_t *p, size_t n)
{
    if (!p || n == 0 || n > BZX_MAX_BLOCK) return BZX_E_PARAM;
    return BZX_OK;
}

extern "C" int bzx_stage_bwt(bzx_ctx *ctx, const uint8_t *blk, size_t n, uint8_t *bwt_out, uint32_t *orig_ptr,
                             uint32_t *status)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !bwt_out || !orig_ptr || check_blk_args(blk, n)) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, 1);
    if (rc) return rc;
    memset(&ctx->h_blk[0], 0, sizeof(BzxBlock));
    ctx->h_blk[0].in_off = 0;
    ctx->h_blk[0].n = (uint32_t)n;
    ctx->B.in = ctx->d_in;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_in, blk, n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.blk, ctx->h_blk, sizeof(BzxBlock), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_stages(ctx, 1, STG_BWT))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(bwt_out, ctx->B.bwt, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, ctx->B.blk, sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *orig_ptr = ctx->h_blk[0].orig_ptr;
    if (status) *status = ctx->h_blk[0].status & BZX_ST_PERIODIC;
    return BZX_OK;
}

#ifdef BZX_DIAG
// Debug/bench helper (not part of include/bzx.h): replicate one block `reps` times as a batch, run the
// given stages, return the HIP-event time of each stage in ms[4] (bwt, mtf, huffman, emit).
extern "C" int bzx_dbg_time_stages(bzx_ctx *ctx, const uint8_t *blk, size_t n, uint32_t reps, int stages, float ms[4])
{
    auto api_lock_ = ctx_lock(ctx);
    if (!ctx || check_blk_args(blk, n) || reps == 0) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, reps);
    if (rc) return rc;
    ctx->B.in = ctx->d_in;
    for (uint32_t b = 0; b < reps; b++) {
        memset(&ctx->h_blk[b], 0, sizeof(BzxBlock));
        ctx->h_blk[b].in_off = (uint64_t)b * BZX_BLK_STRIDE;
        ctx->h_blk[b].n = (uint32_t)n;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_in + (size_t)b * BZX_BLK_STRIDE, blk, n, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.blk, ctx->h_blk, reps * sizeof(BzxBlock), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_stages(ctx, reps, stages))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; i++) {
        ms[i] = 0.f;
        (void)hipEventElapsedTime(&ms[i], ctx->ev[i], ctx->ev[i + 1]);
    }
    return BZX_OK;
}
#endif   // BZX_DIAG

extern "C" int bzx_stage_mtf(bzx_ctx *ctx, const uint8_t *bwt, size_t n, uint16_t *mtfv_out, uint32_t *n_mtf,
                             uint32_t freq_out[258], uint8_t in_use_out[256])
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !mtfv_out || !n_mtf || !freq_out || !in_use_out || check_blk_args(bwt, n)) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, 1);
    if (rc) return rc;
    memset(&ctx->h_blk[0], 0, sizeof(BzxBlock));
    ctx->h_blk[0].n = (uint32_t)n;
    ctx->B.in = ctx->d_in;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.bwt, bwt, n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.blk, ctx->h_blk, sizeof(BzxBlock), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_stages(ctx, 1, STG_MTF))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, ctx->B.blk, sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t m = ctx->h_blk[0].n_mtf;
    if (m == 0 || m > n + 1) {
        ctx->err = "device MTF produced an impossible symbol count";
        return BZX_E_HIP;
    }
    *n_mtf = m;
    HIP_TRY(ctx, hipMemcpy(mtfv_out, ctx->B.mtfv, (size_t)m * 2, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(freq_out, ctx->B.freq, 258 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(in_use_out, ctx->B.in_use, 256, hipMemcpyDeviceToHost));
    return BZX_OK;
}

extern "C" int bzx_stage_huffman(bzx_ctx *ctx, const uint16_t *mtfv, uint32_t n_mtf, const uint32_t freq[258],
                                 uint32_t alpha_size, uint32_t *n_groups, uint32_t *n_selectors, uint8_t *selectors,
                                 uint8_t len_out[6][258], uint32_t code_out[6][258])
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !mtfv || !freq || !n_groups || !n_selectors || !selectors || !len_out || !code_out) return BZX_E_PARAM;
    if (n_mtf == 0 || n_mtf > BZX_MAX_BLOCK + 1 || alpha_size < 3 || alpha_size > BZX_MAX_ALPHA) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, 1);
    if (rc) return rc;
    memset(&ctx->h_blk[0], 0, sizeof(BzxBlock));
    ctx->h_blk[0].n = n_mtf - 1;
    ctx->h_blk[0].n_mtf = n_mtf;
    ctx->h_blk[0].n_in_use = alpha_size - 2;
    uint32_t f260[260];
    memset(f260, 0, sizeof(f260));
    memcpy(f260, freq, 258 * sizeof(uint32_t));
    HIP_TRY(ctx, hipMemcpy(ctx->B.mtfv, mtfv, (size_t)n_mtf * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->B.freq, f260, sizeof(f260), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(ctx->B.in_use, 0, 256));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.blk, ctx->h_blk, sizeof(BzxBlock), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_stages(ctx, 1, STG_HUF))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, ctx->B.blk, sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_groups = ctx->h_blk[0].n_groups;
    *n_selectors = ctx->h_blk[0].n_selectors;
    if (*n_selectors > BZX_MAX_SEL) {
        ctx->err = "device Huffman stage produced an impossible selector count";
        return BZX_E_HIP;
    }
    HIP_TRY(ctx, hipMemcpy(selectors, ctx->B.selector, *n_selectors, hipMemcpyDeviceToHost));
    static thread_local uint8_t hl[6 * 260];
    static thread_local uint32_t hc[6 * 260];
    HIP_TRY(ctx, hipMemcpy(hl, ctx->B.len, sizeof(hl), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(hc, ctx->B.code, sizeof(hc), hipMemcpyDeviceToHost));
    for (int t = 0; t < 6; t++)
        for (int v = 0; v < 258; v++) {
            len_out[t][v] = hl[t * 260 + v];
            code_out[t][v] = hc[t * 260 + v];
        }
    return BZX_OK;
}

// Huffman stage, then emit stage, of one block whose descriptor and symbol slabs the host fills (the MTF stage's part
// of the descriptor: n, n_mtf, n_in_use; the BWT's orig_ptr; the splitter's crc).  The emit stage runs only once the
// Huffman stage's size of the image is known to fit the block's output slab.
extern "C" int bzx_stage_encode(bzx_ctx *ctx, const uint16_t *mtfv, uint32_t n_mtf, const uint32_t freq[258],
                                const uint8_t in_use[256], uint32_t orig_ptr, uint32_t crc, uint8_t *out, size_t cap,
                                size_t *out_len, uint8_t *pad_bits, uint8_t *selector_mtf, bzx_block_info *info)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !mtfv || !freq || !in_use || !out || !out_len || !pad_bits || !selector_mtf || !info) return BZX_E_PARAM;
    uint32_t alpha_size = 2;
    uint8_t iu[256];
    for (int i = 0; i < 256; i++) alpha_size += (iu[i] = in_use[i] ? 1 : 0);
    if (n_mtf == 0 || n_mtf > BZX_MAX_BLOCK + 1 || alpha_size < 3 || alpha_size > BZX_MAX_ALPHA || orig_ptr > 0xffffffu)
        return BZX_E_PARAM;
    for (uint32_t i = 0; i < n_mtf; i++)
        if (mtfv[i] >= alpha_size) {
            ctx->err = "bzx_stage_encode: symbol outside the alphabet";
            return BZX_E_PARAM;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, 1);
    if (rc) return rc;
    memset(&ctx->h_blk[0], 0, sizeof(BzxBlock));
    ctx->h_blk[0].n = n_mtf - 1;
    ctx->h_blk[0].n_mtf = n_mtf;
    ctx->h_blk[0].n_in_use = alpha_size - 2;
    ctx->h_blk[0].orig_ptr = orig_ptr;
    ctx->h_blk[0].crc = crc;
    uint32_t f260[260];
    memset(f260, 0, sizeof(f260));
    memcpy(f260, freq, 258 * sizeof(uint32_t));
    HIP_TRY(ctx, hipMemcpy(ctx->B.mtfv, mtfv, (size_t)n_mtf * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->B.freq, f260, sizeof(f260), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->B.in_use, iu, 256, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.blk, ctx->h_blk, sizeof(BzxBlock), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_stages(ctx, 1, STG_HUF))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, ctx->B.blk, sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const BzxBlock &d = ctx->h_blk[0];
    if (d.n_selectors != (n_mtf + BZX_G_SIZE - 1) / BZX_G_SIZE || d.n_groups < 2 || d.n_groups > 6) {
        ctx->err = "device Huffman stage produced an impossible selector or table count";
        return BZX_E_HIP;
    }
    const uint64_t sum = 105ull + d.sec_bits[3] + 18 + d.sec_bits[0] + d.sec_bits[1] + d.sec_bits[2];
    if (d.bits != sum || d.bits > (uint64_t)BZX_OUT_STRIDE * 8) {
        ctx->err = d.bits != sum ? "device Huffman stage produced section sizes that do not add up"
                                 : "bzx_stage_encode: the image of this symbol stream is larger than a block's output slab";
        return d.bits != sum ? BZX_E_HIP : BZX_E_PARAM;
    }
    if ((rc = run_stages(ctx, 1, STG_EMIT, 0))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    block_info_of(d, info);
    HIP_TRY(ctx, hipMemcpy(selector_mtf, ctx->B.selector_mtf, d.n_selectors, hipMemcpyDeviceToHost));
    const size_t bytes = (size_t)((d.bits + 7) >> 3);
    *out_len = bytes;
    if (bytes > cap) return BZX_E_OUTBUF;
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_outbuf, bytes, hipMemcpyDeviceToHost));
    *pad_bits = (uint8_t)((8 - (d.bits & 7)) & 7);
    return BZX_OK;
}

// The block figures of a run over blocks [0, nblk) of ctx->h_blk.
static void fill_stats_from_blocks(bzx_ctx *ctx, uint32_t nblk, uint64_t raw_bytes)
{
    bzx_stats &st = ctx->stats;
    st.nblk = nblk;
    ctx->stats_batch = false;
    st.n_periodic = 0;
    st.raw_bytes = raw_bytes;
    st.rle1_bytes = 0;
    st.mtf_symbols = 0;
    fold_blocks(st, ctx->h_blk, 0, nblk, 1);
}

extern "C" int bzx_compress_blocks(bzx_ctx *ctx, uint32_t nblk, const uint8_t *const *blks, const size_t *ns,
                                   const uint32_t *crcs, uint8_t *const *outs, const size_t *caps, size_t *out_lens,
                                   uint8_t *pads)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !blks || !ns || !crcs || !outs || !caps || !out_lens || !pads) return BZX_E_PARAM;
    if (nblk == 0) return BZX_OK;
    for (uint32_t b = 0; b < nblk; b++)
        if (check_blk_args(blks[b], ns[b]) || !outs[b]) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_blocks(ctx, nblk);
    if (rc) return rc;
    ctx->B.in = ctx->d_in;
    for (uint32_t b = 0; b < nblk; b++) {
        memset(&ctx->h_blk[b], 0, sizeof(BzxBlock));
        ctx->h_blk[b].in_off = (uint64_t)b * BZX_BLK_STRIDE;
        ctx->h_blk[b].n = (uint32_t)ns[b];
        ctx->h_blk[b].crc = crcs[b];
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_in + (size_t)b * BZX_BLK_STRIDE, blks[b], ns[b], hipMemcpyHostToDevice,
                                    ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->B.blk, ctx->h_blk, nblk * sizeof(BzxBlock), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_stages(ctx, nblk, STG_ALL, 0))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, ctx->B.blk, nblk * sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    collect_stage_times(ctx);
    fill_stats_from_blocks(ctx, nblk, 0);
    bzx_stats &st = ctx->stats;
    st.out_bits = 0;
    st.ms_split = 0;
    int ret = BZX_OK;
    for (uint32_t b = 0; b < nblk; b++) {
        const BzxBlock &d = ctx->h_blk[b];
        const size_t bytes = (size_t)((d.bits + 7) >> 3);
        st.out_bits += d.bits;
        if (bytes > BZX_OUT_STRIDE) {
            // cannot happen: an image is at most n * 17/8 + tables, and the emit kernel clips at the slab end
            ctx->err = "block image larger than its device slab";
            (void)hipStreamSynchronize(ctx->stream);       // copies into earlier callers' buffers are in flight
            return BZX_E_HIP;
        }
        if (bytes > caps[b]) {
            ret = BZX_E_OUTBUF;
            out_lens[b] = bytes;
            continue;
        }
        if (hipMemcpyAsync(outs[b], (const uint8_t *)ctx->d_outbuf + (size_t)b * BZX_OUT_STRIDE, bytes, hipMemcpyDeviceToHost,
                           ctx->stream) != hipSuccess) {
            ctx->err = "hipMemcpyAsync(block image) failed";
            (void)hipStreamSynchronize(ctx->stream);       // earlier copies into caller buffers are in flight
            return BZX_E_HIP;
        }
        out_lens[b] = bytes;
        pads[b] = (uint8_t)((8 - (d.bits & 7)) & 7);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    st.ms_total = st.ms_bwt + st.ms_mtf + st.ms_huffman + st.ms_emit;
    return ret;
}

// compress_block.rs:24.  Thread-safe: the reference calls compress_block from every rayon worker at once
// (compress.rs:125-132).  The first caller becomes the batch leader, waits a moment for the others, runs all pending
// blocks as ONE device batch and hands the results back; callers that arrive meanwhile form the next batch.
extern "C" int bzx_compress_block(bzx_ctx *ctx, const uint8_t *blk, size_t n, uint32_t crc, uint8_t *out, size_t cap,
                                  size_t *out_len, uint8_t *pad_bits)
{
    if (!ctx || !out || !out_len || !pad_bits || check_blk_args(blk, n)) return BZX_E_PARAM;
    BlockReq rq;
    rq.blk = blk;
    rq.n = n;
    rq.crc = crc;
    rq.out = out;
    rq.cap = cap;
    std::unique_lock<std::mutex> lk(ctx->bq_mu);
    try {
        ctx->bq_pending.push_back(&rq);
    } catch (const std::bad_alloc &) {
        return BZX_E_NOMEM;                      // (nothing may unwind across the C ABI)
    }
    while (!rq.done) {
        if (ctx->bq_leader) {
            ctx->bq_cv.wait(lk);
            continue;
        }
        ctx->bq_leader = true;
        ctx->bq_cv.wait_for(lk, std::chrono::microseconds(300));          // collection window (lock released)
        std::vector<BlockReq *> batch;
        batch.swap(ctx->bq_pending);                                      // (swap does not allocate)
        lk.unlock();
        const uint32_t nb = (uint32_t)batch.size();
        int rc = BZX_OK;
        std::vector<size_t> lens;
        try {
            std::vector<const uint8_t *> blks(nb);
            std::vector<size_t> ns(nb), caps(nb);
            std::vector<uint32_t> crcs(nb);
            std::vector<uint8_t *> outs(nb);
            std::vector<uint8_t> pads(nb, 0);
            lens.assign(nb, 0);
            for (uint32_t i = 0; i < nb; i++) {
                blks[i] = batch[i]->blk;
                ns[i] = batch[i]->n;
                crcs[i] = batch[i]->crc;
                outs[i] = batch[i]->out;
                caps[i] = batch[i]->cap;
            }
            rc = nb ? bzx_compress_blocks(ctx, nb, blks.data(), ns.data(), crcs.data(), outs.data(), caps.data(),
                                          lens.data(), pads.data())
                    : BZX_OK;
            for (uint32_t i = 0; i < nb; i++) batch[i]->pad = pads[i];
        } catch (const std::bad_alloc &) {
            rc = BZX_E_NOMEM;                    // every request of the batch fails; nobody is left waiting
        }
        lk.lock();
        for (uint32_t i = 0; i < nb; i++) {
            BlockReq *q = batch[i];
            q->out_len = i < lens.size() ? lens[i] : 0;
            // a block whose image did not fit reports that; its neighbours in the batch are fine
            q->rc = rc == BZX_E_OUTBUF ? (q->out_len > q->cap ? BZX_E_OUTBUF : BZX_OK) : rc;
            q->done = true;
        }
        ctx->bq_leader = false;
        ctx->bq_cv.notify_all();
    }
    *out_len = rq.out_len;
    *pad_bits = rq.pad;
    return rq.rc;
}


// Device split: raw (device) -> block slabs + descriptors (n, crc, in_off).  Returns the block count.
int split_on_device(bzx_ctx *ctx, const uint8_t *d_raw, size_t len, int level, uint32_t *nblk_out, uint32_t own_first,
                    uint32_t own_step, uint64_t *last_raw_start, uint64_t *gathered_tiles)
{
    *nblk_out = 0;
    if (len == 0) return BZX_OK;
    const size_t nmax = (size_t)100000 * level - 19;
    const size_t max_blocks_sz = (len + len / 4) / nmax + 2;
    if (max_blocks_sz > 0x7fffffffu) return BZX_E_PARAM;
    const uint32_t max_blocks = (uint32_t)max_blocks_sz;
    int rc = ensure_blocks(ctx, max_blocks, (max_blocks + own_step - 1) / own_step + 1);
    if (rc) return rc;
    BzxSplitWs ws;
    // (gathered_tiles: the per-byte scans were done rank by rank, bzx_shard_scan_*; only the chain of boundaries is left)
    if (gathered_tiles) rc = bzx_split_shard_boundaries(ctx, d_raw, len, level, max_blocks, own_step, gathered_tiles, &ws);
    else rc = bzx_split_launch_boundaries(ctx, d_raw, len, level, max_blocks, &ws);
    if (rc) return rc;
    uint32_t *h_n = (uint32_t *)(ctx->h_scalars + 4);
    HIP_TRY(ctx, hipMemcpyAsync(h_n, ws.nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t nblk = *h_n;
    if (nblk == 0 || nblk > max_blocks) {
        ctx->err = "device block splitter produced an impossible block count";
        return BZX_E_HIP;
    }
    if (last_raw_start) {
        // raw position where the last block starts: a chunked caller restarts the split there (the splitter's state
        // is clean at a block start: a block is a whole number of run pieces, bzx_rle1.hip)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars + 5, ws.blk_raw + (nblk - 1), sizeof(uint64_t), hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *last_raw_start = ctx->h_scalars[5];
    }
    bzx_split_launch_scatter(ctx, d_raw, len, ws, nblk, ctx->d_in, ctx->B.blk, own_first, own_step);
    HIP_TRY(ctx, hipGetLastError());
    ctx->B.in = ctx->d_in;
    ctx->B.raw = d_raw;
    *nblk_out = nblk;
    return BZX_OK;
}

extern "C" int bzx_compress_device(bzx_ctx *ctx, const void *d_raw, size_t len, int level, void *d_out, size_t cap,
                                   size_t *out_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (ctx) ctx->cidx_ok = false;
    if (!ctx || !d_out || !out_len || !level_ok(level) || (len && !d_raw)) return BZX_E_PARAM;
    if (((uintptr_t)d_raw & 15u) || ((uintptr_t)d_out & 3u) || cap < 16) {
        ctx->err = "bzx_compress_device: d_raw must be 16-byte aligned, d_out 4-byte aligned, cap >= 16";
        return BZX_E_PARAM;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
    uint32_t nblk = 0;
    int rc = split_on_device(ctx, (const uint8_t *)d_raw, len, level, &nblk);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[6], ctx->stream));
    if ((rc = run_stages(ctx, nblk, STG_ALL, level, d_out, cap & ~(size_t)3))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[7], ctx->stream));
    if (nblk) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, ctx->B.blk, nblk * sizeof(BzxBlock), hipMemcpyDeviceToHost,
                                          ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out_len = (size_t)ctx->h_scalars[1];
    collect_stage_times(ctx);
    fill_stats_from_blocks(ctx, nblk, len);
    ctx->stats.out_bits = (uint64_t)*out_len * 8;
    (void)hipEventElapsedTime(&ctx->stats.ms_split, ctx->ev[5], ctx->ev[6]);
    (void)hipEventElapsedTime(&ctx->stats.ms_total, ctx->ev[5], ctx->ev[7]);
    if (ctx->keep_index) {                      // the descriptors are on the host already: the index costs no device work
        uint64_t bit = 32, raw_off = 0;
        ctx->cidx.clear();
        if (index_append(ctx->cidx, ctx->h_blk, nblk, level, &bit, &raw_off)) {
            ctx->err = "out of host memory for the block index";
            return BZX_E_NOMEM;
        }
        memset(&ctx->cidx_info, 0, sizeof(ctx->cidx_info));
        ctx->cidx_info.in_bytes = *out_len;
        ctx->cidx_info.out_bytes = raw_off;
        ctx->cidx_info.nblk = nblk;
        ctx->cidx_info.nstreams = 1;
        ctx->cidx_ok = true;
    }
    return BZX_OK;
}

// Host bytes pre[0..npre) followed by raw[0..len) are copied to the device and split there; the first blocks -- all of
// them if final, else all but the last -- come back into blocks_out, ns and crcs, and their count into *nblk_out.
// last_start (optional): raw position where the last block starts.
static int split_to_host(bzx_ctx *ctx, const uint8_t *pre, size_t npre, const uint8_t *raw, size_t len, int level,
                         bool final, uint8_t *blocks_out, uint32_t nblk_cap, uint32_t *ns, uint32_t *crcs,
                         uint32_t *nblk_out, uint64_t *last_start)
{
    const size_t total = npre + len;
    if (total == 0) return BZX_OK;
    DevMem<> d_raw;                          // (freed on return, behind the synchronisation below)
    if (!d_raw.reserve(total)) {
        ctx->err = "hipMalloc(split input) failed";
        return BZX_E_NOMEM;
    }
    int rc = BZX_OK;
    uint32_t nblk = 0, use = 0;
    if (npre && hipMemcpyAsync(d_raw, pre, npre, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = BZX_E_HIP;
    if (!rc && len && hipMemcpyAsync(d_raw + npre, raw, len, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = BZX_E_HIP;
    if (!rc) rc = split_on_device(ctx, d_raw, total, level, &nblk, 0, 1, last_start);
    if (!rc) {
        use = final ? nblk : nblk - 1;
        if (use > nblk_cap) rc = BZX_E_OUTBUF;
    }
    if (!rc && use) {
        if (hipMemcpyAsync(ctx->h_blk, ctx->B.blk, use * sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = BZX_E_HIP;
    }
    for (uint32_t b = 0; !rc && b < use; b++) {
        ns[b] = ctx->h_blk[b].n;
        crcs[b] = ctx->h_blk[b].crc;
        if (ns[b] == 0 || ns[b] > BZX_MAX_BLOCK) {
            ctx->err = "device block splitter produced an impossible block length";
            rc = BZX_E_HIP;
            break;
        }
        const uint64_t off = ctx->h_blk[b].in_off;
        const uint8_t *src = (off & BZX_IN_RAW) ? d_raw + (off & ~BZX_IN_RAW) : ctx->d_in + off;
        if (hipMemcpy(blocks_out + (size_t)b * BZX_MAX_BLOCK, src, ns[b], hipMemcpyDeviceToHost) != hipSuccess)
            rc = BZX_E_HIP;
    }
    (void)hipStreamSynchronize(ctx->stream);
    if (!rc) *nblk_out = use;
    return rc;
}

extern "C" int bzx_split_rle1(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, uint8_t *blocks_out,
                              uint32_t nblk_cap, uint32_t *ns, uint32_t *crcs, uint32_t *nblk_out)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !blocks_out || !ns || !crcs || !nblk_out || !level_ok(level) || (len && !raw)) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *nblk_out = 0;
    return split_to_host(ctx, nullptr, 0, raw, len, level, true, blocks_out, nblk_cap, ns, crcs, nblk_out, nullptr);
}

// ---- multi-GPU sharding: block i belongs to rank i mod world; no collective in here.
// The caller all-reduces (sum) d_bits between the two calls and sums the partial streams afterwards
// (torch.distributed / RCCL; see bench.py).  Declared in include/bzx.h.
static int shard_prepare(bzx_ctx *ctx, const void *d_raw, size_t len, int level, uint32_t rank, uint32_t world,
                         uint32_t *nblk_total, long long *d_bits, size_t bits_cap, uint64_t *gathered_tiles)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !nblk_total || !d_bits || !level_ok(level) || world == 0 || rank >= world || (len && !d_raw)) return BZX_E_PARAM;
    if ((uintptr_t)d_raw & 15u) {
        ctx->err = "bzx_shard_prepare: d_raw must be 16-byte aligned";
        return BZX_E_PARAM;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!gathered_tiles) HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));     // (else: bzx_shard_scan_runs did)
    uint32_t nblk = 0;
    ctx->B.blk_first = 0;
    ctx->B.blk_step = 1;
    int rc = split_on_device(ctx, (const uint8_t *)d_raw, len, level, &nblk, rank, world, nullptr, gathered_tiles);
    if (rc) return rc;
    if (nblk > bits_cap) return BZX_E_OUTBUF;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[6], ctx->stream));
    const uint32_t mine = nblk > rank ? (nblk - rank + world - 1) / world : 0;
    ctx->B.blk_first = rank;
    ctx->B.blk_step = world;
    rc = run_stages(ctx, mine, STG_BWT | STG_MTF | STG_HUF);
    if (!rc && mine) bzx_launch_bits_export(ctx->B, d_bits, ctx->stream);
    ctx->B.blk_first = 0;
    ctx->B.blk_step = 1;
    if (rc) return rc;
    ctx->shard_total = nblk;
    ctx->shard_rank = rank;
    ctx->shard_world = world;
    ctx->shard_level = level;
    ctx->shard_packed_max = 0;
    ctx->shard_len = len;
    *nblk_total = nblk;
    return BZX_OK;
}

extern "C" int bzx_shard_prepare(bzx_ctx *ctx, const void *d_raw, size_t len, int level, uint32_t rank, uint32_t world,
                                 uint32_t *nblk_total, long long *d_bits, size_t bits_cap)
{
    return shard_prepare(ctx, d_raw, len, level, rank, world, nblk_total, d_bits, bits_cap, nullptr);
}

// ---- sharded split analysis: the two per-byte passes of the block splitter run on 1/world of the
// input per rank; what the ranks exchange is 24 bytes per 8 KiB tile (the caller's all-gathers).  include/bzx.h.
static int shard_scan_args(bzx_ctx *ctx, const void *d_raw, size_t len, uint32_t rank, uint32_t world, long long *d_tiles)
{
    if (!ctx || !d_tiles || world == 0 || rank >= world || !len || !d_raw) return BZX_E_PARAM;
    if ((uintptr_t)d_raw & 15u) {
        ctx->err = "bzx_shard_scan_*: d_raw must be 16-byte aligned";
        return BZX_E_PARAM;
    }
    return BZX_OK;
}

extern "C" size_t bzx_shard_scan_entries(size_t len, uint32_t world)
{
    return world ? (size_t)bzx_split_tiles_per_rank(len, world) : 0;
}

extern "C" int bzx_shard_scan_runs(bzx_ctx *ctx, const void *d_raw, size_t len, uint32_t rank, uint32_t world, long long *d_tiles)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    int rc = shard_scan_args(ctx, d_raw, len, rank, world, d_tiles);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
    rc = bzx_split_shard_runs(ctx, (const uint8_t *)d_raw, len, rank, world, (uint64_t *)d_tiles);
    HIP_TRY(ctx, hipGetLastError());
    return rc;
}

extern "C" int bzx_shard_scan_counts(bzx_ctx *ctx, const void *d_raw, size_t len, uint32_t rank, uint32_t world, long long *d_tiles)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    int rc = shard_scan_args(ctx, d_raw, len, rank, world, d_tiles);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = bzx_split_shard_counts(ctx, (const uint8_t *)d_raw, len, rank, world, (uint64_t *)d_tiles);
    HIP_TRY(ctx, hipGetLastError());
    return rc;
}

extern "C" int bzx_shard_prepare_scanned(bzx_ctx *ctx, const void *d_raw, size_t len, int level, uint32_t rank, uint32_t world,
                                         long long *d_tiles, uint32_t *nblk_total, long long *d_bits, size_t bits_cap)
{
    if (!d_tiles || !len) return BZX_E_PARAM;
    return shard_prepare(ctx, d_raw, len, level, rank, world, nblk_total, d_bits, bits_cap, (uint64_t *)d_tiles);
}

extern "C" int bzx_ctx_sync(bzx_ctx *ctx)
{
    auto api_lock_ = ctx_lock(ctx);
    if (!ctx) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BZX_OK;
}

static uint32_t shard_count(uint32_t nblk, uint32_t rank, uint32_t world)
{
    return nblk > rank ? (nblk - rank + world - 1) / world : 0;
}

extern "C" int bzx_shard_packed_max(bzx_ctx *ctx, size_t *max_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !max_len) return BZX_E_PARAM;
    if (ctx->shard_level == 0 || ctx->shard_packed_max == 0) return BZX_E_STATE;
    *max_len = (size_t)ctx->shard_packed_max;
    return BZX_OK;
}

extern "C" int bzx_shard_emit_packed(bzx_ctx *ctx, const long long *d_bits_all, void *d_packed, size_t cap,
                                     size_t *packed_len, size_t *stream_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !d_bits_all || !d_packed || !packed_len || !stream_len || ((uintptr_t)d_packed & 3u)) return BZX_E_PARAM;
    if (ctx->shard_level == 0) return BZX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BzxBatch &B = ctx->B;
    const uint32_t nblk = ctx->shard_total, rank = ctx->shard_rank, world = ctx->shard_world;
    const uint32_t mine = shard_count(nblk, rank, world);
    B.nblk = nblk;
    B.blk_first = 0;
    B.blk_step = 1;
    B.packed = 0;
    if (nblk) bzx_launch_bits_import(B, d_bits_all, ctx->stream);
    bzx_launch_layout(B, 32, 0, ctx->d_scalars, ctx->stream);                              // final positions of ALL blocks
    bzx_launch_pack_layout(B, rank, world, mine, ctx->d_scalars + 2, ctx->stream);         // my packed positions
    if (world <= 64) bzx_launch_pack_max(B, world, ctx->d_scalars + 3, ctx->stream);       // ... and the longest of any rank
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->shard_packed_max = world <= 64 ? ctx->h_scalars[3] * 4 : 0;
    const uint64_t out_bytes = (ctx->h_scalars[0] + 80 + 7) >> 3;
    const uint64_t need = ctx->h_scalars[2] * 4;
    if (need > cap) {
        ctx->err = "packed buffer too small for this rank's blocks";
        return BZX_E_OUTBUF;
    }
    HIP_TRY(ctx, hipMemsetAsync(d_packed, 0, need, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 64 * sizeof(uint32_t), ctx->stream));
    B.out = (uint32_t *)d_packed;
    B.nblk = mine;
    B.blk_first = rank;
    B.blk_step = world;
    B.packed = 1;
    if (mine) bzx_launch_emit(B, (uint32_t)ctx->n_cu, ctx->stream);
    B.packed = 0;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[7], ctx->stream));
    if (nblk) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_blk, B.blk, nblk * sizeof(BzxBlock), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    B.nblk = nblk;
    B.blk_first = 0;
    B.blk_step = 1;
    *packed_len = (size_t)need;
    *stream_len = (size_t)out_bytes;
    // stats over my blocks
    bzx_stats &st = ctx->stats;
    collect_stage_times(ctx);
    st.nblk = mine;
    ctx->stats_batch = false;
    st.n_periodic = 0;
    st.raw_bytes = ctx->shard_len / world;
    st.rle1_bytes = 0;
    st.mtf_symbols = 0;
    fold_blocks(st, ctx->h_blk, rank, nblk, world);
    st.out_bits = out_bytes * 8;
    (void)hipEventElapsedTime(&st.ms_split, ctx->ev[5], ctx->ev[6]);
    (void)hipEventElapsedTime(&st.ms_total, ctx->ev[5], ctx->ev[7]);
    return BZX_OK;
}

extern "C" int bzx_shard_assemble_begin(bzx_ctx *ctx, void *d_out, size_t cap, size_t *stream_len)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !d_out || ((uintptr_t)d_out & 3u)) return BZX_E_PARAM;
    if (ctx->shard_level == 0) return BZX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BzxBatch &B = ctx->B;
    B.nblk = ctx->shard_total;
    B.blk_first = 0;
    B.blk_step = 1;
    B.out = (uint32_t *)d_out;
    const uint64_t out_bytes = (ctx->h_scalars[0] + 80 + 7) >> 3;      // total bits from bzx_shard_emit_packed
    const uint64_t need = (out_bytes + 3) & ~3ull;
    if (need > (cap & ~(size_t)3)) {
        ctx->err = "output buffer too small for the compressed stream";
        return BZX_E_OUTBUF;
    }
    bzx_launch_zero_edges(B, ctx->d_scalars, ctx->stream);       // only the words that are OR-merged, not the whole stream
    bzx_launch_stream_frame(B, ctx->shard_level, ctx->d_scalars, ctx->d_scalars + 1, ctx->stream);
    if (stream_len) *stream_len = (size_t)out_bytes;
    return BZX_OK;
}

extern "C" int bzx_shard_assemble_rank(bzx_ctx *ctx, const void *d_packed_r, uint32_t r, void *d_out)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !d_packed_r || !d_out || ((uintptr_t)d_packed_r & 3u) || r >= ctx->shard_world) return BZX_E_PARAM;
    if (ctx->shard_level == 0) return BZX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BzxBatch &B = ctx->B;
    const uint32_t nblk = ctx->shard_total, world = ctx->shard_world;
    const uint32_t nown = shard_count(nblk, r, world);
    B.nblk = nblk;
    B.out = (uint32_t *)d_out;
    if (nown == 0) return BZX_OK;
    bzx_launch_pack_layout(B, r, world, nown, ctx->d_scalars + 3, ctx->stream);            // rank r's packed positions
    bzx_launch_unpack(B, (const uint32_t *)d_packed_r, r, world, nown, grid_for(ctx, nown, 4), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return BZX_OK;
}

// RLE1Block::new(source, block_size) + Iterator::next (rle1.rs:49-85,245-263) for a source that arrives in pieces:
// every call returns the blocks that are complete with the bytes seen so far; the last, unfinished block is withheld
// (its raw bytes are kept in the context) and comes out of a later call, or of the call with final != 0.
extern "C" int bzx_split_rle1_chunk(bzx_ctx *ctx, const uint8_t *raw, size_t len, int level, int final, uint8_t *blocks_out,
                                    uint32_t nblk_cap, uint32_t *ns, uint32_t *crcs, uint32_t *nblk_out)
{
    auto api_lock_ = ctx_lock(ctx);
    BZX_REFUSE_WHILE_STREAMING(ctx);
    if (!ctx || !blocks_out || !ns || !crcs || !nblk_out || !level_ok(level) || (len && !raw)) return BZX_E_PARAM;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *nblk_out = 0;
    std::vector<uint8_t> &carry = ctx->split_carry;
    const size_t total = carry.size() + len;
    uint32_t use = 0;
    uint64_t last_start = 0;
    int rc = split_to_host(ctx, carry.data(), carry.size(), raw, len, level, final, blocks_out, nblk_cap, ns, crcs, &use,
                           &last_start);
    if (rc) return rc;
    // the withheld block's raw bytes: [last_start, total) of (carry | raw)
    std::vector<uint8_t> next;
    if (!final) {
        const size_t ls = (size_t)last_start, cs = carry.size();
        try {
            next.reserve(total - ls);
            if (ls < cs) next.insert(next.end(), carry.begin() + ls, carry.end());
            const size_t from = ls > cs ? ls - cs : 0;
            if (len > from) next.insert(next.end(), raw + from, raw + len);
        } catch (const std::bad_alloc &) {
            return BZX_E_NOMEM;
        }
    }
    carry.swap(next);
    *nblk_out = use;
    return BZX_OK;
}

// Page-locked host memory for the callers' buffers (copies from/to pageable memory are staged by the runtime and
// cannot overlap the kernels).
extern "C" void *bzx_host_alloc(size_t bytes)
{
    void *p = nullptr;
    // portable: bzx_mstream_* copies from one such buffer to every device of the process
    return hipHostMalloc(&p, bytes ? bytes : 1, BZX_HOST_PORTABLE) == hipSuccess ? p : nullptr;
}
extern "C" void bzx_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}


#ifdef BZX_DIAG
// Diagnostic build only (libbzx_diag.so, -DBZX_DIAG; never in libbzx.so): phase timers of the sort kernels.
// Debug helper (not in include/bzx.h): enable/read the BWT kernel's phase timers (100 MHz wall-clock ticks summed over blocks).
extern "C" int bzx_dbg_set_stop(bzx_ctx *ctx, uint32_t k)
{
    if (!ctx) return BZX_E_PARAM;
    ctx->B.dbg_stop = k;
    return BZX_OK;
}

extern "C" int bzx_dbg_phase_timers(bzx_ctx *ctx, int enable, unsigned long long out[128])
{
    if (!ctx) return BZX_E_PARAM;
    if (enable && !ctx->d_dbg) {
        if (!ctx->d_dbg.reserve(128 * sizeof(unsigned long long))) return BZX_E_NOMEM;
    }
    if (out && ctx->d_dbg) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(out, ctx->d_dbg, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    if (ctx->d_dbg) HIP_TRY(ctx, hipMemset(ctx->d_dbg, 0, 128 * sizeof(unsigned long long)));
    ctx->B.dbg = enable ? ctx->d_dbg.get() : nullptr;
    return BZX_OK;
}

// Debug helper: per-block microseconds spent in the BWT kernel during the last run with phase timers enabled.
extern "C" int bzx_dbg_block_times(bzx_ctx *ctx, uint32_t nblk, uint32_t *us_out, uint32_t *n_out, uint32_t *inuse_out)
{
    if (!ctx || !us_out || nblk > ctx->cap_blocks) return BZX_E_PARAM;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->h_blk, ctx->B.blk, nblk * sizeof(BzxBlock), hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < nblk; b++) {
        us_out[b] = ctx->h_blk[b].pad_[1];
        if (n_out) n_out[b] = ctx->h_blk[b].n;
        if (inuse_out) inuse_out[b] = ctx->h_blk[b].n_in_use;
    }
    return BZX_OK;
}
#endif   // BZX_DIAG
