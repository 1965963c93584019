// bzx_grep.hip -- the records of a .bz2 that hold a byte pattern (include/bzx.h: bzx_grep_buffer), on top of the public
// index interface: ONE index pass with the record table (bzx_index_count_records), find (bzx_index_find) and the hits'
// line numbers (bzx_index_find_lines) switched on, then ONE call of bzx_decompress_records_buffer over the index and the
// table that pass left, with one range {line, 1} per distinct line.  The blocks that hold a matching record are decoded
// twice -- by the pass and by the record read -- the trade of bzx_salvage_buffer and bzx_decompress_records_*.
#include <string.h>
#include <algorithm>
#include <new>
#include <string>
#include <vector>
#include "bzx_host.h"

struct GrepIx {                      // the open index, closed on every way out
    bzx_index *ix = nullptr;
    ~GrepIx() { end(); }
    void end()
    {
        if (ix) bzx_index_end(ix);
        ix = nullptr;
    }
};

static int grep_run(bzx_ctx *ctx, const uint8_t *bz2, size_t len, const uint8_t *pat, size_t m, int delim, uint64_t max_hits,
                    uint64_t *recs, uint64_t cap_recs, uint64_t *nrecs, uint8_t *out, size_t cap, size_t *out_offs, size_t *lens,
                    size_t *need, uint64_t *total_hits, int *truncated)
{
    GrepIx g;
    int rc = bzx_index_begin(ctx, std::min<size_t>(std::max<size_t>(len, 16), (size_t)64 << 20), &g.ix);
    if (rc) return rc;
    bzx_index *ix = g.ix;
    if ((rc = bzx_index_count_records(ix, delim)) || (rc = bzx_index_find(ix, pat, m, max_hits)) ||
        (rc = bzx_index_find_lines(ix, delim))) {
        const std::string why = ctx->err;
        g.end();
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
            ctx->err = "bzx_grep_buffer: the feed loop made no progress";
            rc = BZX_E_STATE;
        }
    }
    const std::string why = ctx->err;                        // (BZX_E_DATA: the verified prefix is still searched and read)
    std::vector<bzx_index_entry> e;
    std::vector<uint64_t> rb, want;
    const int pass_rc = rc;
    if (!rc || rc == BZX_E_DATA) {
        const bzx_index_entry *ep = nullptr;
        const uint64_t *tp = nullptr, *hp = nullptr, *lp = nullptr;
        bzx_index_info info;
        uint64_t n = 0, nh = 0, nl = 0;
        int rc2;
        if ((rc2 = bzx_index_get(ix, &ep, &info)) || (rc2 = bzx_index_get_records(ix, &tp, &n)) ||
            (rc2 = bzx_index_get_hits(ix, &hp, &nh, total_hits)) || (rc2 = bzx_index_get_hit_lines(ix, &lp, &nl))) {
            g.end();
            return rc2;
        }
        e.assign(ep, ep + n);
        rb.assign(tp, tp + n + 1);
        want.assign(lp, lp + nl);                            // (non-descending: the distinct values are the runs' first)
        want.erase(std::unique(want.begin(), want.end()), want.end());
        *truncated = *total_hits > nh ? 1 : 0;
    }
    g.end();
    if (pass_rc && pass_rc != BZX_E_DATA) {
        ctx->err = why;
        return pass_rc;
    }
    *nrecs = want.size();
    if (want.size() > cap_recs) {
        ctx->err = "bzx_grep_buffer: " + std::to_string(want.size()) + " matching records, cap_recs is " + std::to_string(cap_recs);
        return BZX_E_OUTBUF;
    }
    if (want.size() > 0x7FFFFFFFull) {
        ctx->err = "bzx_grep_buffer: more than 2^31 - 1 matching records in one call (lower max_hits)";
        return BZX_E_PARAM;
    }
    if (!want.empty()) {
        memcpy(recs, want.data(), want.size() * sizeof(uint64_t));
        const std::vector<uint64_t> ones(want.size(), 1);
        std::vector<int> status(want.size());
        const bzx_piece whole = {bz2, 0, len};
        rc = bzx_decompress_records_buffer(ctx, &whole, 1, e.data(), e.size(), rb.data(), delim, (uint32_t)want.size(), recs,
                                           ones.data(), out, cap, out_offs, lens, status.data(), need);
        if (rc) return rc;
    }
    if (pass_rc) ctx->err = why;
    return pass_rc;
}

extern "C" int bzx_grep_buffer(bzx_ctx *ctx, const uint8_t *bz2, size_t len, const uint8_t *pat, size_t m, int delim,
                               uint64_t max_hits, uint64_t *recs, uint64_t cap_recs, uint64_t *nrecs, uint8_t *out, size_t cap,
                               size_t *out_offs, size_t *lens, size_t *need, uint64_t *total_hits, int *truncated)
{
    BzxFindPat fp;
    if (!ctx || !nrecs || !need || !total_hits || !truncated || (len && !bz2) || (cap_recs && (!recs || !out_offs || !lens)) ||
        (cap && !out) || delim < 0 || delim > 255 || !bzx_find_pattern(pat, m, &fp))
        return BZX_E_PARAM;
    *nrecs = 0;
    *need = 0;
    *total_hits = 0;
    *truncated = 0;
    if (memchr(pat, delim, m)) {
        ctx->err = "bzx_grep_buffer: the pattern contains the delimiter (no record holds it)";
        return BZX_E_PARAM;
    }
    try {
        return grep_run(ctx, bz2, len, pat, m, delim, max_hits, recs, cap_recs, nrecs, out, cap, out_offs, lens, need, total_hits,
                        truncated);
    } catch (const std::bad_alloc &) {
        ctx->err = "out of host memory";
        return BZX_E_NOMEM;
    }
}
