// bzx -- thin command line over libbzx.so, mirroring the reference's CLI (src/tools/cli.rs:113-303, src/main.rs:16-38)
// and C bzip2's conventions: -z / -d / -t, -1..-9, -c, -k, -f, -q, -v.  SURVEY.md 8f N4.  Host glue only: every byte of
// compression and decompression work happens on the device behind include/bzx.h; without a HIP device the tool fails.
// Compression streams the input through bzx_cstream_feed in chunks (files larger than device memory are fine and the
// output is written while the next chunk is compressed); decompression of one file, of a file above the batch limit and
// of standard input streams through bzx_dstream_feed the same way (no size guess, bounded memory).  Compressing two or more
// named files (without -v), the regular files of at most 16 MiB are read and compressed together, one
// bzx_compress_batch_buffer call per batch of up to 256 MiB, each into its own .bz2; -d and -t do the same through
// bzx_decompress_batch_buffer (a file it does not accept is decoded again on its own, for the one-file path's message).
// --devices LIST (HIP ordinals, comma-separated, repeats allowed): the chunked compression path deals its chunks over
// these devices through bzx_mstream_feed, one process, host-side assembly; the bytes are the same.
// --index FILE.bz2 ... writes FILE.bz2.bzxi, the block index of bzx_index_* (layout: include/bzx.h); -dc --range OFF:LEN
// FILE.bz2 reads that index and only the bytes of the file that bzx_index_span names, and writes decoded bytes
// [OFF, OFF + LEN) to standard output through bzx_decompress_range_buffer.  Without an index that matches the file it
// refuses: there is no silent full decode behind --range.  -dc --ranges LIST FILE.bz2 does the same for a list of OFF:LEN
// lines in one bzx_decompress_ranges_buffer call: it reads the byte intervals of the file that bzx_index_spans names and
// writes the ranges in list order, back to back; when any range fails, nothing is written.
// --with-index FILE ... (compression) writes FILE.bz2 and FILE.bz2.bzxi in one pass: the library keeps the index while it
// compresses (bzx_ctx_keep_index / bzx_mctx_keep_index), on the chunked path, with --devices and on the batched path; the
// index is written after its .bz2 closed cleanly, in the format --index writes.
// --recover FILE.bz2 ... (the counterpart of bzip2recover) writes FILE.recovered, or standard output with -c: every intact
// block of a damaged file.  A salvage index (bzx_salvage_begin, fed as --index feeds) says which blocks verify and where the
// gaps are; the data then comes from bzx_decompress_range_buffer over that index in pieces of at most 256 MiB of output,
// reading only the bytes of the file each piece needs.  One line per gap goes to standard error.  The input stays.  With
// --index it also writes FILE.bz2.bzxi (the gaps are not stored): -dc --range then reads the damaged file.  Exit status
// 0: nothing was lost, 2: something was, 1: trouble.
// --index --lines FILE.bz2 ... also writes FILE.bz2.bzxr, the record table of bzx_index_count_records for the delimiter '\n'
// (little-endian: a 32-byte header -- "BZXR", version 1 (u32), delimiter (u32), zero (u32), nblk (u64), T (u64) -- and
// nblk + 1 u64 values); -dc --lines FIRST:COUNT FILE.bz2 reads .bzxi and .bzxr (and refuses when either is missing or they
// describe different block counts), reads only the bytes of the file that bzx_records_pieces names and writes lines
// [FIRST, FIRST + COUNT), numbered from 0, to standard output through bzx_decompress_records_buffer.
// --find STRING / --find-hex HEX FILE.bz2 ... prints where the byte string occurs in what every FILE decodes to: one decimal
// offset per line, FILE:OFFSET with several files, through bzx_index_find on the index pass (nothing decoded leaves the
// device); --count prints the total only; --max-hits N (default 1000000) bounds the list, and one line on standard error
// says how many more hits there were.  With --index, and with --index --lines, the same pass writes .bzxi and .bzxr.  Exit
// status as grep's: 0 a hit, 1 none, 2 an error or a damaged file (whose verified prefix is still searched and printed).
// --grep STRING / --grep-hex HEX FILE.bz2 ... prints the lines (delimiter '\n') of what every FILE decodes to that contain the
// byte string, FILE: in front with several files, N: in front with --line-number (N numbered from 0, the numbering of
// --lines FIRST:COUNT): one index pass with bzx_index_find, bzx_index_find_lines and the line table, then one
// bzx_decompress_records_buffer over the pieces of the file that hold a matching line.  --count prints the number of
// matching lines among the listed hits; --max-hits as for --find; with --index --lines the same pass writes .bzxi and
// .bzxr.  Exit status as grep's: 0 a line matched, 1 none, 2 an error or a damaged file.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <new>
#include <string>
#include <vector>
#include "../include/bzx.h"

enum Mode { ZIP, UNZIP, TEST };
struct Opts {
    Mode mode = ZIP;
    int level = 9;
    bool to_stdout = false, keep = false, force = false;
    int verbose = 0;
    bool quiet = false;
    std::vector<std::string> files;
    std::vector<int> devices;          // --devices: entries of a bzx_mctx for the chunked compression path
    bool index = false, range = false; // --index; --range OFF:LEN
    bool recover = false;              // --recover
    bool mode_set = false;             // -z, -d or -t was given
    bool with_index = false;           // --with-index: FILE.bz2.bzxi beside FILE.bz2, from the compressor
    uint64_t range_off = 0, range_len = 0;
    std::string ranges;                // --ranges LIST
    bool lines = false, lines_range = false;       // --lines; --lines FIRST:COUNT
    uint64_t lines_first = 0, lines_count = 0;
    bool find = false, count = false;  // --find STRING or --find-hex HEX; --count
    std::string find_pat;
    uint64_t max_hits = 1000000;       // --max-hits N
    bool grep = false, line_number = false;        // --grep STRING or --grep-hex HEX (the pattern is find_pat); --line-number
};

static void help()
{
    puts("usage: bzx [flags] [files ...]\n"
         "  -z --compress     compress (default)        -d --decompress   decompress\n"
         "  -t --test         check integrity           -c --stdout       write to standard output\n"
         "  -k --keep         keep input files          -f --force        overwrite output files\n"
         "  -1 .. -9          block size 100k .. 900k   --fast = -1, --best = -9 (default)\n"
         "  -q --quiet        no warnings               -v --verbose      statistics (-vv more)\n"
         "  -s --small        accepted, ignored         -h --help  -V --version  -L --license\n"
         "  --devices LIST    compress one stream on several devices: ordinals, comma-separated, repeats allowed\n"
         "  --index           write FILE.bzxi, the block index of every FILE (a .bz2), for --range\n"
         "  --range OFF:LEN   with -dc: decoded bytes [OFF, OFF + LEN) of FILE to standard output, through FILE.bzxi\n"
         "  --ranges LIST     with -dc: the same for every OFF:LEN line of the text file LIST, in one call, back to back\n"
         "  --lines           with --index: also write FILE.bzxr, the table of lines per block\n"
         "  --lines FIRST:COUNT  with -dc: lines [FIRST, FIRST + COUNT) of FILE, numbered from 0, through FILE.bzxi and FILE.bzxr\n"
         "  --find STRING     print the offsets at which STRING occurs in what every FILE (a .bz2) decodes to, one per line\n"
         "  --find-hex HEX    the same for the bytes HEX names (1 to 256 of them), e.g. 0d0a00ff\n"
         "                    --count: the total only; --max-hits N: list at most N (default 1000000); with --index (and\n"
         "                    --lines) the same pass writes the index; exit status 0: a hit, 1: none, 2: error or damage\n"
         "  --grep STRING     print the lines of what every FILE (a .bz2) decodes to that contain STRING (--grep-hex HEX: bytes)\n"
         "                    --line-number: N: in front, N numbered from 0 as for --lines FIRST:COUNT, so -dc --lines N:1 reads\n"
         "                    that line; --count: the number of matching lines among the listed hits; --max-hits N as for\n"
         "                    --find; with --index --lines the same pass writes both tables; exit status 0: a line matched,\n"
         "                    1: none, 2: error or damage\n"
         "  --recover         write every intact block of a damaged FILE.bz2 to FILE.recovered (-c: standard output) and\n"
         "                    one line per gap to standard error; with --index also FILE.bz2.bzxi for --range;\n"
         "                    exit status 0: nothing lost, 2: data lost, 1: trouble\n"
         "  --with-index      compress FILE to FILE.bz2 and write FILE.bz2.bzxi in the same pass (not with -c or standard input)\n"
         "With no file, or when a file is -, reads standard input and writes standard output.");
}

static bool read_all(FILE *f, std::vector<uint8_t> &v)
{
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    return !ferror(f);
}

static int fail(const Opts &o, const char *what, const char *name, bzx_ctx *ctx, int rc)
{
    if (!o.quiet) fprintf(stderr, "bzx: %s: %s: %s%s%s\n", name, what, bzx_strerror(rc), ctx && bzx_last_error(ctx)[0] ? ": " : "",
                          ctx ? bzx_last_error(ctx) : "");
    return 1;
}

// input stream -> .bz2 on `out`, chunk by chunk
static int mfail(const Opts &o, const char *what, const char *name, bzx_mctx *m, int rc)
{
    if (!o.quiet) fprintf(stderr, "bzx: %s: %s: %s%s%s\n", name, what, bzx_strerror(rc), bzx_mctx_last_error(m)[0] ? ": " : "",
                          bzx_mctx_last_error(m));
    return 1;
}

// The index of one compressed file, copied out of the library before its stream object ends.
struct KeptIndex {
    std::vector<bzx_index_entry> e;
    bzx_index_info info;
};

// (mctx: with --devices the chunks go through bzx_mstream_feed, dealt over its entries, instead of bzx_cstream_feed;
// kept: with --with-index, receives the stream's index)
static int do_zip(const Opts &o, bzx_ctx *ctx, bzx_mctx *mctx, FILE *in, FILE *out, const char *name, KeptIndex *kept)
{
    const size_t CH = (size_t)64 << 20;
    bzx_cstream *cs = nullptr;
    bzx_mstream *ms = nullptr;
    int rc = mctx ? bzx_mstream_begin(mctx, o.level, CH, &ms) : bzx_cstream_begin(ctx, o.level, CH, &cs);
    if (rc) return mctx ? mfail(o, "cannot start", name, mctx, rc) : fail(o, "cannot start", name, ctx, rc);
    uint8_t *buf[2] = {(uint8_t *)bzx_host_alloc(CH), (uint8_t *)bzx_host_alloc(CH)};
    size_t cap = CH + CH / 50 + (1 << 20), total_in = 0, flushed = 0, produced = 0;
    uint8_t *obuf = (uint8_t *)malloc(cap);
    int ret = 0;
    if (!buf[0] || !buf[1] || !obuf) ret = fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
    size_t have = ret ? 0 : fread(buf[0], 1, CH, in);
    for (int k = 0; !ret; k++) {
        // read ahead to know whether this chunk is the last one
        const size_t next = have == CH ? fread(buf[(k + 1) & 1], 1, CH, in) : 0;
        const int fin = next == 0;
        // the whole stream must fit the output buffer the library writes into: grow it as the input grows
        const size_t need = total_in + have + (total_in + have) / 50 + (1 << 20);
        if (need > cap) {
            uint8_t *nb = (uint8_t *)realloc(obuf, need * 2);
            if (!nb) {
                ret = fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
                break;
            }
            memset(nb + cap, 0, need * 2 - cap);
            obuf = nb;
            cap = need * 2;
        }
        rc = mctx ? bzx_mstream_feed(ms, buf[k & 1], have, fin, obuf, cap, &produced)
                  : bzx_cstream_feed(cs, buf[k & 1], have, fin, obuf, cap, &produced);
        if (rc) {
            ret = mctx ? mfail(o, "compression failed", name, mctx, rc) : fail(o, "compression failed", name, ctx, rc);
            break;
        }
        total_in += have;
        if (produced > flushed) {
            if (fwrite(obuf + flushed, 1, produced - flushed, out) != produced - flushed) {
                ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
                break;
            }
            flushed = produced;
        }
        if (fin) break;
        have = next;
    }
    if (!ret && o.verbose && mctx) {
        bzx_stats st;
        bzx_mdev_info *mi = new (std::nothrow) bzx_mdev_info;
        bzx_mctx_get_stats(mctx, &st);
        fprintf(stderr, "  %s: %zu -> %zu bytes, %.3f:1, %u blocks (%u periodic)\n", name, total_in, produced,
                produced ? (double)total_in / (double)produced : 0.0, st.nblk, st.n_periodic);
        for (uint32_t e = 0; mi && bzx_mctx_get_info(mctx, mi) == BZX_OK && e < mi->ndev; e++)
            fprintf(stderr, "    devices[%u] = %d: %u chunks, %llu blocks, %.1f ms\n", e, mi->dev[e].device, mi->dev[e].chunks,
                    (unsigned long long)mi->dev[e].blocks, mi->dev[e].ms_device);
        delete mi;
    } else if (!ret && o.verbose) {
        bzx_stats st;
        bzx_get_stats(ctx, &st);
        fprintf(stderr, "  %s: %zu -> %zu bytes, %.3f:1, %u blocks (%u periodic)\n", name, total_in, produced,
                produced ? (double)total_in / (double)produced : 0.0, st.nblk, st.n_periodic);
        // -vv: one line per block, the figures the reference logs at -vvv (compress_block.rs:58-63, huffman.rs:176-181)
        bzx_block_info bi;
        for (uint32_t b = 0; o.verbose > 1 && b < st.nblk && bzx_get_block_info(ctx, b, &bi) == BZX_OK; b++)
            fprintf(stderr, "    block %u: crc = 0x%08x, %u in block, origPtr %u%s, %u values in use, %u mtf symbols, "
                            "%u coding tables, %u selectors; bits: map %u + selectors %u + tables %u + codes %u -> %llu\n",
                    b + 1, bi.crc, bi.n, bi.orig_ptr, bi.periodic ? " (periodic)" : "", bi.n_in_use, bi.n_mtf, bi.n_tables,
                    bi.n_selectors, bi.bits_symbol_map, bi.bits_selectors, bi.bits_tables, bi.bits_payload,
                    (unsigned long long)bi.bits);
    }
    if (!ret && kept) {
        const bzx_index_entry *e = nullptr;
        rc = mctx ? bzx_mstream_get_index(ms, &e, &kept->info) : bzx_cstream_get_index(cs, &e, &kept->info);
        if (rc) {
            ret = mctx ? mfail(o, "no index", name, mctx, rc) : fail(o, "no index", name, ctx, rc);
        } else {
            try {
                kept->e.assign(e, e + kept->info.nblk);
            } catch (const std::bad_alloc &) {
                ret = fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
            }
        }
    }
    if (mctx) bzx_mstream_end(ms);
    else bzx_cstream_end(cs);
    bzx_host_free(buf[0]);
    bzx_host_free(buf[1]);
    free(obuf);
    return ret;
}

// .bz2 on `in` (or, with in == nullptr, in `mem`) -> raw bytes on `out` (none for -t) through bzx_dstream_feed: read in
// chunks into page-locked memory, written as it is produced; no guess of the output size, one decode, device memory
// independent of the file.
static int do_unzip(const Opts &o, bzx_ctx *ctx, FILE *in, const std::vector<uint8_t> *mem, FILE *out, const char *name)
{
    const size_t CH = (size_t)64 << 20, OC = (size_t)64 << 20;
    const char *what = o.mode == TEST ? "integrity check failed" : "decompression failed";
    bzx_dstream *ds = nullptr;
    int rc = bzx_dstream_begin(ctx, CH, &ds);
    if (rc) return fail(o, "cannot start", name, ctx, rc);
    uint8_t *ibuf = in ? (uint8_t *)bzx_host_alloc(CH) : nullptr, *obuf = (uint8_t *)malloc(OC);
    const uint8_t *src = in ? ibuf : mem->data();
    int ret = 0, done = 0;
    if ((in && !ibuf) || !obuf) ret = fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
    size_t have = in ? 0 : mem->size(), off = 0, total_in = 0, total_out = 0;
    bool eof = !in;
    while (!ret && !done) {
        if (off == have && !eof) {
            have = fread(ibuf, 1, CH, in);
            off = 0;
            if (have < CH) {
                if (ferror(in)) {
                    ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
                    break;
                }
                eof = true;
            }
        }
        size_t used = 0, made = 0;
        rc = bzx_dstream_feed(ds, src + off, have - off, eof ? 1 : 0, &used, obuf, OC, &made, &done);
        if (rc) {
            ret = fail(o, what, name, ctx, rc);
            break;
        }
        off += used;
        total_in += used;
        total_out += made;
        if (made && out && fwrite(obuf, 1, made, out) != made) ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
    }
    if (!ret && o.verbose) fprintf(stderr, "  %s: %s, %zu -> %zu bytes\n", name, o.mode == TEST ? "ok" : "done", total_in, total_out);
    bzx_dstream_end(ds);
    if (ibuf) bzx_host_free(ibuf);
    free(obuf);
    return ret;
}

// ---- --index / --range ---------------------------------------------------------------------------------------------
static void put_le(uint8_t *p, uint64_t v, int n)
{
    for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}
static uint64_t get_le(const uint8_t *p, int n)
{
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
static const size_t BZXI_HEADER = 64, BZXI_ENTRY = 40;

// The stored form of an index (include/bzx.h) into oname; after a failure: a message, the partial file removed, 1.
static int write_bzxi(const Opts &o, const std::string &oname, const bzx_index_entry *e, const bzx_index_info &info)
{
    FILE *out = fopen(oname.c_str(), "wb");
    uint8_t head[BZXI_HEADER] = {'B', 'Z', 'X', 'I'}, rec[BZXI_ENTRY];
    put_le(head + 4, 1, 4);
    put_le(head + 8, info.in_bytes, 8);
    put_le(head + 16, info.out_bytes, 8);
    put_le(head + 24, info.nblk, 8);
    put_le(head + 32, info.nstreams, 4);
    bool ok = out && fwrite(head, 1, sizeof head, out) == sizeof head;
    for (uint64_t k = 0; ok && k < info.nblk; k++) {
        memset(rec, 0, sizeof rec);
        put_le(rec, e[k].bit, 8);
        put_le(rec + 8, e[k].out_off, 8);
        put_le(rec + 16, e[k].out_len, 4);
        put_le(rec + 20, e[k].crc, 4);
        put_le(rec + 24, e[k].img_bits, 4);
        put_le(rec + 28, e[k].stream, 4);
        rec[32] = e[k].level;
        ok = fwrite(rec, 1, sizeof rec, out) == sizeof rec;
    }
    if (out && fclose(out) != 0) ok = false;
    if (!ok) {
        if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", oname.c_str(), strerror(errno));
        unlink(oname.c_str());
        return 1;
    }
    if (o.verbose)
        fprintf(stderr, "  %s: %llu blocks in %u streams, %llu -> %llu bytes\n", oname.c_str(), (unsigned long long)info.nblk,
                info.nstreams, (unsigned long long)info.in_bytes, (unsigned long long)info.out_bytes);
    return 0;
}

// FILE.bz2 through bzx_index_feed, 64 MiB chunks in page-locked memory as -d reads them: the index (--index), or the
// salvage index (--recover).  -> 0 and the open index, or 1 after a message.
// find (--find): the pattern and the list size of bzx_index_find; then a file that does not verify leaves the index of
// its verified prefix open, after the message, and *damaged says so.
struct FindReq {
    const std::string *pat;
    uint64_t max_hits;
    bool damaged = false;
    int lines_delim = -1;              // (--grep) also bzx_index_find_lines
};
static int feed_index(const Opts &o, bzx_ctx *ctx, const std::string &f, bool salvage, bzx_index **out, int delim = -1,
                      FindReq *find = nullptr)
{
    *out = nullptr;
    const char *name = f.c_str();
    FILE *in = fopen(name, "rb");
    if (!in) {
        if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", name, strerror(errno));
        return 1;
    }
    const size_t CH = (size_t)64 << 20;
    bzx_index *ix = nullptr;
    int rc = salvage ? bzx_salvage_begin(ctx, CH, &ix) : bzx_index_begin(ctx, CH, &ix);
    if (!rc && delim >= 0 && (rc = bzx_index_count_records(ix, delim))) bzx_index_end(ix);
    if (!rc && find && (rc = bzx_index_find(ix, (const uint8_t *)find->pat->data(), find->pat->size(), find->max_hits)))
        bzx_index_end(ix);
    if (!rc && find && find->lines_delim >= 0 && (rc = bzx_index_find_lines(ix, find->lines_delim))) bzx_index_end(ix);
    if (rc) {
        fclose(in);
        return fail(o, "cannot start", name, ctx, rc);
    }
    uint8_t *ibuf = (uint8_t *)bzx_host_alloc(CH);
    int ret = ibuf ? 0 : fail(o, "out of memory", name, nullptr, BZX_E_NOMEM), done = 0;
    size_t have = 0, off = 0;
    bool eof = false;
    while (!ret && !(done && eof && off == have)) {
        if (off == have && !eof) {
            have = fread(ibuf, 1, CH, in);
            off = 0;
            if (have < CH) {
                if (ferror(in)) {
                    ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
                    break;
                }
                eof = true;
            }
        }
        size_t used = 0;
        rc = bzx_index_feed(ix, ibuf + off, have - off, eof ? 1 : 0, &used, &done);
        if (rc) {
            ret = fail(o, salvage ? "salvage failed" : "indexing failed", name, ctx, rc);
            if (rc == BZX_E_DATA && find) {
                find->damaged = true;
                ret = 0;
            }
            break;
        }
        off += used;
    }
    fclose(in);
    if (ibuf) bzx_host_free(ibuf);
    if (ret) bzx_index_end(ix);
    else *out = ix;
    return ret;
}

static const size_t BZXR_HEADER = 32;
static const int LINE_DELIM = '\n';

// The stored form of a record table into oname; after a failure: a message, the partial file removed, 1.
static int write_bzxr(const Opts &o, const std::string &oname, const uint64_t *rec_before, uint64_t nblk)
{
    FILE *out = fopen(oname.c_str(), "wb");
    uint8_t head[BZXR_HEADER] = {'B', 'Z', 'X', 'R'}, v[8];
    put_le(head + 4, 1, 4);
    put_le(head + 8, LINE_DELIM, 4);
    put_le(head + 16, nblk, 8);
    put_le(head + 24, rec_before[nblk], 8);
    bool ok = out && fwrite(head, 1, sizeof head, out) == sizeof head;
    for (uint64_t k = 0; ok && k <= nblk; k++) {
        put_le(v, rec_before[k], 8);
        ok = fwrite(v, 1, sizeof v, out) == sizeof v;
    }
    if (out && fclose(out) != 0) ok = false;
    if (!ok) {
        if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", oname.c_str(), strerror(errno));
        unlink(oname.c_str());
        return 1;
    }
    if (o.verbose)
        fprintf(stderr, "  %s: %llu lines end in %llu blocks\n", oname.c_str(), (unsigned long long)rec_before[nblk],
                (unsigned long long)nblk);
    return 0;
}

// FILE.bz2 -> FILE.bz2.bzxi, and with --lines FILE.bz2.bzxr
static int do_index(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    const char *name = f.c_str();
    bzx_index *ix = nullptr;
    if (feed_index(o, ctx, f, false, &ix, o.lines ? LINE_DELIM : -1)) return 1;
    const bzx_index_entry *e = nullptr;
    bzx_index_info info;
    const uint64_t *rb = nullptr;
    uint64_t nrb = 0;
    int ret = 0, rc;
    if ((rc = bzx_index_get(ix, &e, &info))) ret = fail(o, "indexing failed", name, ctx, rc);
    if (!ret && o.lines && (rc = bzx_index_get_records(ix, &rb, &nrb))) ret = fail(o, "indexing failed", name, ctx, rc);
    if (!ret) ret = write_bzxi(o, f + ".bzxi", e, info);
    if (!ret && o.lines) ret = write_bzxr(o, f + ".bzxr", rb, nrb);
    bzx_index_end(ix);
    return ret;
}

// --find: the hits of FILE.bz2 to standard output; with --index also what do_index writes, from the same pass (not for a
// damaged file).  -> 0: a hit, 1: none, 2: an error or a damaged file.
static int do_find(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    const char *name = f.c_str();
    const bool multi = o.files.size() > 1;
    bzx_index *ix = nullptr;
    FindReq req{&o.find_pat, o.count ? 0 : o.max_hits};
    if (feed_index(o, ctx, f, false, &ix, o.index && o.lines ? LINE_DELIM : -1, &req)) return 2;
    const bool damaged = req.damaged;
    const uint64_t *hits = nullptr, *rb = nullptr;
    uint64_t nlisted = 0, total = 0, nrb = 0;
    const bzx_index_entry *e = nullptr;
    bzx_index_info info;
    int rc, ret = 0;
    if ((rc = bzx_index_get_hits(ix, &hits, &nlisted, &total))) ret = fail(o, "find failed", name, ctx, rc);
    if (!ret && o.count) {
        if (multi) printf("%s:", name);
        printf("%llu\n", (unsigned long long)total);
    } else if (!ret) {
        for (uint64_t i = 0; i < nlisted; i++) {
            if (multi) printf("%s:", name);
            printf("%llu\n", (unsigned long long)hits[i]);
        }
        if (total > nlisted && !o.quiet)
            fprintf(stderr, "bzx: %s: %llu more hits not listed (--max-hits %llu)\n", name, (unsigned long long)(total - nlisted),
                    (unsigned long long)o.max_hits);
    }
    if (!ret && fflush(stdout) != 0) ret = fail(o, strerror(errno), "standard output", nullptr, BZX_OK);
    if (!ret && o.index && !damaged) {
        if ((rc = bzx_index_get(ix, &e, &info))) ret = fail(o, "indexing failed", name, ctx, rc);
        if (!ret && o.lines && (rc = bzx_index_get_records(ix, &rb, &nrb))) ret = fail(o, "indexing failed", name, ctx, rc);
        if (!ret) ret = write_bzxi(o, f + ".bzxi", e, info);
        if (!ret && o.lines) ret = write_bzxr(o, f + ".bzxr", rb, nrb);
    }
    bzx_index_end(ix);
    return ret || damaged ? 2 : total ? 0 : 1;
}

static int range_refuse(const Opts &o, const std::string &f, const char *why)
{
    if (!o.quiet) fprintf(stderr, "bzx: %s: --range: %s\n", f.c_str(), why);
    return 1;
}

// FILE.bz2.bzxi and FILE.bz2, with the refusals of --range and --ranges: no index, not an index, an index of another size.
// -> 0 and the entries, the open file and its size; 1 after a message.
static int load_index(const Opts &o, const std::string &f, std::vector<bzx_index_entry> &e, uint64_t *out_bytes, FILE **in,
                      uint64_t *file_size)
{
    const std::string iname = f + ".bzxi";
    FILE *xf = fopen(iname.c_str(), "rb");
    if (!xf) return range_refuse(o, f, ("no index " + iname + " (write it with bzx --index " + f + ")").c_str());
    std::vector<uint8_t> x;
    const bool xok = read_all(xf, x);
    fclose(xf);
    if (!xok || x.size() < BZXI_HEADER || memcmp(x.data(), "BZXI", 4) != 0 || get_le(x.data() + 4, 4) != 1)
        return range_refuse(o, f, ("not a bzx index of version 1: " + iname).c_str());
    const uint64_t in_bytes = get_le(x.data() + 8, 8), nblk = get_le(x.data() + 24, 8);
    *out_bytes = get_le(x.data() + 16, 8);
    if ((x.size() - BZXI_HEADER) / BZXI_ENTRY != nblk || (x.size() - BZXI_HEADER) % BZXI_ENTRY)
        return range_refuse(o, f, ("truncated index " + iname).c_str());
    *in = fopen(f.c_str(), "rb");
    struct stat sb;
    if (!*in || fstat(fileno(*in), &sb) != 0) {
        if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", f.c_str(), strerror(errno));
        if (*in) fclose(*in);
        *in = nullptr;
        return 1;
    }
    *file_size = (uint64_t)sb.st_size;
    int ret = 0;
    try {
        e.resize(nblk);
        for (uint64_t k = 0; k < nblk; k++) {
            const uint8_t *r = x.data() + BZXI_HEADER + k * BZXI_ENTRY;
            memset(&e[k], 0, sizeof(e[k]));
            e[k].bit = get_le(r, 8);
            e[k].out_off = get_le(r + 8, 8);
            e[k].out_len = (uint32_t)get_le(r + 16, 4);
            e[k].crc = (uint32_t)get_le(r + 20, 4);
            e[k].img_bits = (uint32_t)get_le(r + 24, 4);
            e[k].stream = (uint32_t)get_le(r + 28, 4);
            e[k].level = r[32];
        }
        const uint64_t total = nblk ? e[nblk - 1].out_off + e[nblk - 1].out_len : 0;
        if (*file_size != in_bytes || total != *out_bytes)
            ret = range_refuse(o, f, "the index does not match the file (another size): write it again with bzx --index");
    } catch (const std::bad_alloc &) {
        ret = fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
    }
    if (ret) {
        fclose(*in);
        *in = nullptr;
    }
    return ret;
}

// Decoded bytes [off, off + len) of FILE.bz2 to standard output, from FILE.bz2.bzxi and the span of the file alone.
static int do_range(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    std::vector<bzx_index_entry> e;
    uint64_t out_bytes = 0, file_size = 0;
    FILE *in = nullptr;
    if (load_index(o, f, e, &out_bytes, &in, &file_size)) return 1;
    const uint64_t nblk = e.size();
    int ret = 0;
    std::vector<uint8_t> span, out;
    uint64_t first = 0, count = 0, lo = 0, hi = 0;
    size_t got = 0;
    try {
        if (bzx_index_span(e.data(), nblk, o.range_off, o.range_len, &first, &count, &lo, &hi)) {
            ret = range_refuse(o, f, "the index does not match the file (entries out of order)");
        } else if (count) {
            // (a salvaged block at the end of a truncated file: the 8 bytes behind it that the reader asks for are zeros)
            const size_t in_file = (size_t)(std::min(hi, file_size) - std::min(lo, file_size));
            span.assign((size_t)(hi - lo), 0);
            out.resize((size_t)std::min<uint64_t>(o.range_len, out_bytes - o.range_off));
            if (fseeko(in, (off_t)lo, SEEK_SET) != 0 || fread(span.data(), 1, in_file, in) != in_file) {
                ret = fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK);
            } else {
                const int rc = bzx_decompress_range_buffer(ctx, span.data(), span.size(), lo, e.data(), nblk, o.range_off,
                                                           o.range_len, out.data(), &got);
                if (rc) ret = fail(o, "range read failed", f.c_str(), ctx, rc);
            }
        }
    } catch (const std::bad_alloc &) {
        ret = fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
    }
    fclose(in);
    if (!ret && got && fwrite(out.data(), 1, got, stdout) != got) ret = fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK);
    if (!ret && fflush(stdout) != 0) ret = 1;
    if (!ret && o.verbose) fprintf(stderr, "  %s: bytes [%llu, %llu) from %llu blocks, %zu bytes of the file read\n", f.c_str(),
                                   (unsigned long long)o.range_off, (unsigned long long)(o.range_off + got),
                                   (unsigned long long)count, span.size());
    return ret;
}

// ---- --recover ---------------------------------------------------------------------------------------------------------
static std::string gap_words(uint32_t why)
{
    static const struct { uint32_t bit; const char *text; } words[] = {
        {BZX_GAP_HEADER, "no stream header"},         {BZX_GAP_NO_MAGIC, "no block magic"},
        {BZX_GAP_STRUCTURE, "damaged block"},         {BZX_GAP_BLOCK_CRC, "block CRC mismatch"},
        {BZX_GAP_RANDOMISED, "randomised block"},     {BZX_GAP_TRUNCATED, "truncated"},
        {BZX_GAP_COMBINED_CRC, "combined CRC mismatch"}};
    std::string s;
    for (const auto &w : words)
        if (why & w.bit) s += (s.empty() ? "" : ", ") + std::string(w.text);
    return s;
}

static const uint64_t RECOVER_PIECE = (uint64_t)256 << 20;   // output bytes of one range read (a block more where one alone is larger)
static const uint64_t RECOVER_SPAN = (uint64_t)320 << 20;    // ... and the bytes of the file read for it: a piece ends before a long gap

// Every intact block of FILE.bz2 -> FILE.recovered.  -> 0: nothing lost, 2: gaps, 1: trouble (after a message).
static int do_recover(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    const char *name = f.c_str();
    // the output's name, checked as -d checks its own, before the salvage pass is paid for
    std::string oname;
    if (!o.to_stdout) {
        oname = (f.size() > 4 && f.compare(f.size() - 4, 4, ".bz2") == 0 ? f.substr(0, f.size() - 4) : f) + ".recovered";
        struct stat sb;
        if (!o.force && stat(oname.c_str(), &sb) == 0) {
            if (!o.quiet) fprintf(stderr, "bzx: %s already exists (use -f)\n", oname.c_str());
            return 1;
        }
    }
    bzx_index *ix = nullptr;
    if (feed_index(o, ctx, f, true, &ix)) return 1;
    const bzx_index_entry *e = nullptr;
    const bzx_gap *g = nullptr;
    bzx_index_info info;
    uint64_t ngaps = 0;
    int rc = bzx_index_get(ix, &e, &info);
    if (!rc) rc = bzx_index_get_gaps(ix, &g, &ngaps);
    if (rc) {
        bzx_index_end(ix);
        return fail(o, "salvage failed", name, ctx, rc);
    }
    std::vector<bzx_index_entry> ent;
    try {
        ent.assign(e, e + info.nblk);
    } catch (const std::bad_alloc &) {
        bzx_index_end(ix);
        return fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
    }
    if (!o.quiet)
        for (uint64_t k = 0; k < ngaps; k++)
            fprintf(stderr, "bzx: %s: gap at bits [%llu, %llu): %s; %u candidate block%s did not verify; at output offset %llu\n", name,
                    (unsigned long long)g[k].bit_lo, (unsigned long long)g[k].bit_hi, gap_words(g[k].why).c_str(), g[k].candidates,
                    g[k].candidates == 1 ? "" : "s", (unsigned long long)g[k].out_off);
    bzx_index_end(ix);                                       // (the range reads need the context)
    FILE *out = stdout;
    if (!o.to_stdout) {
        out = fopen(oname.c_str(), "wb");
        if (!out) {
            if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", oname.c_str(), strerror(errno));
            return 1;
        }
    }
    FILE *in = fopen(name, "rb");
    int ret = in ? 0 : fail(o, strerror(errno), name, nullptr, BZX_OK);
    std::vector<uint8_t> span, buf;
    const uint64_t n = ent.size();
    for (uint64_t k0 = 0; !ret && k0 < n;) {
        // entries [k0, k1): one piece
        const uint64_t lo = ent[k0].bit / 8;
        uint64_t k1 = k0, bytes = 0, hi = lo;
        while (k1 < n) {
            const uint64_t end = (ent[k1].bit + ent[k1].img_bits + 7) / 8 + 8;
            if (k1 > k0 && (bytes + ent[k1].out_len > RECOVER_PIECE || end - lo > RECOVER_SPAN)) break;
            bytes += ent[k1].out_len;
            hi = end;
            k1++;
        }
        try {
            const size_t in_file = (size_t)(std::min(hi, info.in_bytes) - lo);
            span.assign((size_t)(hi - lo), 0);               // (zeros behind the end of a truncated file)
            buf.resize((size_t)bytes);
            size_t got = 0;
            if (fseeko(in, (off_t)lo, SEEK_SET) != 0 || fread(span.data(), 1, in_file, in) != in_file)
                ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
            else if ((rc = bzx_decompress_range_buffer(ctx, span.data(), span.size(), lo, ent.data(), n, ent[k0].out_off, bytes, buf.data(),
                                                       &got)) ||
                     got != bytes)
                ret = fail(o, "reading the salvaged blocks failed", name, ctx, rc ? rc : BZX_E_DATA);
            else if (fwrite(buf.data(), 1, got, out) != got)
                ret = fail(o, strerror(errno), oname.empty() ? "(stdout)" : oname.c_str(), nullptr, BZX_OK);
        } catch (const std::bad_alloc &) {
            ret = fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
        }
        k0 = k1;
    }
    if (in) fclose(in);
    if (out != stdout) {
        if (fflush(out) != 0 || ferror(out) || fclose(out) != 0) {
            if (!ret && !o.quiet) fprintf(stderr, "bzx: %s: %s\n", oname.c_str(), strerror(errno));
            ret = 1;
        }
        if (ret) unlink(oname.c_str());
    } else if (fflush(out) != 0) {
        ret = 1;
    }
    if (!ret && o.index) ret = write_bzxi(o, f + ".bzxi", ent.data(), info);
    if (!ret && o.verbose)
        fprintf(stderr, "  %s: %llu blocks, %llu bytes salvaged, %llu gaps\n", name, (unsigned long long)info.nblk,
                (unsigned long long)info.out_bytes, (unsigned long long)ngaps);
    return ret ? 1 : ngaps ? 2 : 0;
}

// LIST: OFF:LEN lines; blank lines and # comments are skipped.  -> 0, or 1 after a message that names the line.
static int read_ranges(const Opts &o, std::vector<uint64_t> &offs, std::vector<uint64_t> &wants)
{
    FILE *lf = fopen(o.ranges.c_str(), "r");
    if (!lf) {
        fprintf(stderr, "bzx: %s: %s\n", o.ranges.c_str(), strerror(errno));
        return 1;
    }
    std::vector<uint8_t> raw;
    const bool ok = read_all(lf, raw);
    fclose(lf);
    if (!ok) {
        fprintf(stderr, "bzx: %s: %s\n", o.ranges.c_str(), strerror(errno));
        return 1;
    }
    const std::string all(raw.begin(), raw.end());
    size_t line = 0;
    for (size_t p = 0; p < all.size();) {
        const size_t q = all.find('\n', p) == std::string::npos ? all.size() : all.find('\n', p);
        std::string t = all.substr(p, q - p);
        p = q + 1;
        line++;
        if (t.find('#') != std::string::npos) t.erase(t.find('#'));
        const size_t a = t.find_first_not_of(" \t\r"), z = t.find_last_not_of(" \t\r");
        if (a == std::string::npos) continue;
        t = t.substr(a, z - a + 1);
        const size_t c = t.find(':');
        const std::string x = t.substr(0, c), y = c == std::string::npos ? "" : t.substr(c + 1);
        if (x.empty() || y.empty() || x.size() > 19 || y.size() > 19 || x.find_first_not_of("0123456789") != std::string::npos ||
            y.find_first_not_of("0123456789") != std::string::npos) {
            fprintf(stderr, "bzx: %s: line %zu: not OFF:LEN in bytes (got \"%s\")\n", o.ranges.c_str(), line, t.c_str());
            return 1;
        }
        offs.push_back(strtoull(x.c_str(), nullptr, 10));
        wants.push_back(strtoull(y.c_str(), nullptr, 10));
    }
    return 0;
}

// The ranges of LIST to standard output, in list order, back to back: one bzx_decompress_ranges_buffer call over the byte
// intervals of the file that bzx_index_spans names.
static int do_ranges(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    std::vector<uint64_t> offs, wants;
    try {
        if (read_ranges(o, offs, wants)) return 1;
    } catch (const std::bad_alloc &) {
        return fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
    }
    std::vector<bzx_index_entry> e;
    uint64_t out_bytes = 0, file_size = 0;
    FILE *in = nullptr;
    if (load_index(o, f, e, &out_bytes, &in, &file_size)) return 1;
    const uint64_t nblk = e.size();
    const uint32_t count = (uint32_t)offs.size();
    int ret = 0;
    size_t need = 0, read_bytes = 0;
    uint32_t np = 0;
    std::vector<uint8_t> out;
    try {
        if (offs.size() > 0xFFFFFFFFull) {
            ret = range_refuse(o, f, "too many ranges in the list");
        } else if (bzx_index_spans(e.data(), nblk, count, offs.data(), wants.data(), nullptr, nullptr, 0, &np) == BZX_E_PARAM) {
            ret = range_refuse(o, f, "the index does not match the file (entries out of order)");
        } else if (count) {
            std::vector<uint64_t> bases(np), lens(np);
            std::vector<std::vector<uint8_t>> held(np);
            std::vector<bzx_piece> pieces(np);
            std::vector<size_t> out_offs(count), gots(count);
            std::vector<int> status(count);
            if (np && bzx_index_spans(e.data(), nblk, count, offs.data(), wants.data(), bases.data(), lens.data(), np, &np))
                ret = fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
            for (uint32_t j = 0; !ret && j < np; j++) {
                if (bases[j] + lens[j] > file_size) {
                    ret = range_refuse(o, f, "the index does not match the file (a block ends behind it)");
                    break;
                }
                held[j].resize((size_t)lens[j]);
                if (fseeko(in, (off_t)bases[j], SEEK_SET) != 0 || fread(held[j].data(), 1, held[j].size(), in) != held[j].size())
                    ret = fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK);
                pieces[j] = bzx_piece{held[j].data(), bases[j], lens[j]};
                read_bytes += held[j].size();
            }
            for (uint32_t i = 0; i < count; i++)
                need += offs[i] < out_bytes ? (size_t)std::min<uint64_t>(wants[i], out_bytes - offs[i]) : 0;
            if (!ret) {
                out.resize(need ? need : 1);
                const int rc = bzx_decompress_ranges_buffer(ctx, pieces.data(), np, e.data(), nblk, count, offs.data(), wants.data(),
                                                            out.data(), need, out_offs.data(), gots.data(), status.data(), &need);
                if (rc) ret = fail(o, "range read failed", f.c_str(), ctx, rc);
            }
        }
    } catch (const std::bad_alloc &) {
        ret = fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
    }
    fclose(in);
    if (!ret && need && fwrite(out.data(), 1, need, stdout) != need) ret = fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK);
    if (!ret && fflush(stdout) != 0) ret = 1;
    if (!ret && o.verbose) {
        bzx_stats st;
        memset(&st, 0, sizeof st);
        if (count) bzx_get_stats(ctx, &st);
        fprintf(stderr, "  %s: %u ranges, %zu bytes from %u distinct blocks, %u pieces (%zu bytes) of the file read\n", f.c_str(), count,
                need, st.nblk, np, read_bytes);
    }
    return ret;
}

// Lines [first, first + count) of FILE.bz2 to standard output, from FILE.bz2.bzxi, FILE.bz2.bzxr and the byte intervals of
// the file that bzx_records_pieces names.
static int do_lines(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    std::vector<bzx_index_entry> e;
    uint64_t out_bytes = 0, file_size = 0;
    FILE *in = nullptr;
    if (load_index(o, f, e, &out_bytes, &in, &file_size)) return 1;
    const uint64_t nblk = e.size();
    int ret = 0;
    size_t need = 0, read_bytes = 0;
    uint32_t np = 0;
    std::vector<uint8_t> out;
    try {
        const std::string rname = f + ".bzxr";
        std::vector<uint8_t> x;
        std::vector<uint64_t> rb;
        FILE *rf = fopen(rname.c_str(), "rb");
        const bool rok = rf && read_all(rf, x);
        if (rf) fclose(rf);
        if (!rf) {
            ret = range_refuse(o, f, ("no record table " + rname + " (write it with bzx --index --lines " + f + ")").c_str());
        } else if (!rok || x.size() < BZXR_HEADER || memcmp(x.data(), "BZXR", 4) != 0 || get_le(x.data() + 4, 4) != 1 ||
                   get_le(x.data() + 8, 4) != (uint64_t)LINE_DELIM) {
            ret = range_refuse(o, f, ("not a bzx line table of version 1: " + rname).c_str());
        } else if (get_le(x.data() + 16, 8) != nblk || (x.size() - BZXR_HEADER) % 8 || (x.size() - BZXR_HEADER) / 8 != nblk + 1) {
            ret = range_refuse(o, f, "the record table and the index describe different block counts: write both again with bzx --index --lines");
        } else {
            rb.resize(nblk + 1);
            for (uint64_t k = 0; k <= nblk; k++) rb[k] = get_le(x.data() + BZXR_HEADER + 8 * k, 8);
            if (bzx_records_pieces(e.data(), nblk, rb.data(), 1, &o.lines_first, &o.lines_count, nullptr, nullptr, 0, &np) == BZX_E_PARAM)
                ret = range_refuse(o, f, "the record table is damaged (it descends)");
        }
        if (!ret) {
            std::vector<uint64_t> bases(np), lens(np);
            std::vector<std::vector<uint8_t>> held(np);
            std::vector<bzx_piece> pieces(np);
            if (np && bzx_records_pieces(e.data(), nblk, rb.data(), 1, &o.lines_first, &o.lines_count, bases.data(), lens.data(), np, &np))
                ret = fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
            for (uint32_t j = 0; !ret && j < np; j++) {
                if (bases[j] + lens[j] > file_size) {
                    ret = range_refuse(o, f, "the index does not match the file (a block ends behind it)");
                    break;
                }
                held[j].resize((size_t)lens[j]);
                if (fseeko(in, (off_t)bases[j], SEEK_SET) != 0 || fread(held[j].data(), 1, held[j].size(), in) != held[j].size())
                    ret = fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK);
                pieces[j] = bzx_piece{held[j].data(), bases[j], lens[j]};
                read_bytes += held[j].size();
            }
            // room: the decoded bytes of the blocks from the one that holds the first line's start to the one that holds
            // the last line's end
            uint64_t a = 0, z = 0, j = 0, room = 0;
            const uint64_t hi = o.lines_count > ~0ull - o.lines_first ? ~0ull : o.lines_first + o.lines_count;
            if (o.lines_first) bzx_records_span(rb.data(), nblk, o.lines_first, &a, &j);
            bzx_records_span(rb.data(), nblk, hi, &z, &j);
            if (a < nblk && hi) {
                z = std::min(z, nblk - 1);
                room = e[z].out_off + e[z].out_len - e[a].out_off;
            }
            if (!ret) {
                size_t out_off = 0, got = 0;
                int status = 0;
                out.resize(room ? (size_t)room : 1);
                const int rc = bzx_decompress_records_buffer(ctx, pieces.data(), np, e.data(), nblk, rb.data(), LINE_DELIM, 1,
                                                             &o.lines_first, &o.lines_count, out.data(), (size_t)room, &out_off, &got,
                                                             &status, &need);
                if (rc) ret = fail(o, "line read failed", f.c_str(), ctx, rc);
            }
        }
    } catch (const std::bad_alloc &) {
        ret = fail(o, "out of memory", f.c_str(), nullptr, BZX_E_NOMEM);
    }
    fclose(in);
    if (!ret && need && fwrite(out.data(), 1, need, stdout) != need) ret = fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK);
    if (!ret && fflush(stdout) != 0) ret = 1;
    if (!ret && o.verbose)
        fprintf(stderr, "  %s: lines [%llu, +%llu): %zu bytes, %u pieces (%zu bytes) of the file read\n", f.c_str(),
                (unsigned long long)o.lines_first, (unsigned long long)o.lines_count, need, np, read_bytes);
    return ret;
}

// --grep: the matching lines of FILE.bz2 to standard output.  One pass gives the hits' line numbers, the index and the
// line table; the lines then come through bzx_decompress_records_buffer from the pieces of the file that
// bzx_records_pieces names (blocks with a matching line are decoded a second time).  With --index --lines also what
// do_index writes, from the same pass (not for a damaged file).  -> 0: a line matched, 1: none, 2: an error or damage.
static int do_grep(const Opts &o, bzx_ctx *ctx, const std::string &f)
{
    const char *name = f.c_str();
    const bool multi = o.files.size() > 1;
    bzx_index *ix = nullptr;
    FindReq req{&o.find_pat, o.max_hits};
    req.lines_delim = LINE_DELIM;
    if (feed_index(o, ctx, f, false, &ix, LINE_DELIM, &req)) return 2;
    const bool damaged = req.damaged;
    int rc, ret = 0;
    uint64_t nmatch = 0;
    try {
        const uint64_t *hits = nullptr, *lines = nullptr, *rbp = nullptr;
        uint64_t nlisted = 0, total = 0, nl = 0, nblk = 0;
        const bzx_index_entry *ep = nullptr;
        bzx_index_info info;
        std::vector<bzx_index_entry> e;
        std::vector<uint64_t> rb, recs;
        if ((rc = bzx_index_get_hits(ix, &hits, &nlisted, &total)) || (rc = bzx_index_get_hit_lines(ix, &lines, &nl)) ||
            (rc = bzx_index_get(ix, &ep, &info)) || (rc = bzx_index_get_records(ix, &rbp, &nblk)))
            ret = fail(o, "grep failed", name, ctx, rc);
        if (!ret) {
            e.assign(ep, ep + nblk);
            rb.assign(rbp, rbp + nblk + 1);
            recs.assign(lines, lines + nl);                  // (non-descending)
            recs.erase(std::unique(recs.begin(), recs.end()), recs.end());
            nmatch = recs.size();
            if (o.index && !damaged) {
                ret = write_bzxi(o, f + ".bzxi", ep, info);
                if (!ret && o.lines) ret = write_bzxr(o, f + ".bzxr", rbp, nblk);
            }
        }
        bzx_index_end(ix);                                   // (the record read wants the context to itself)
        ix = nullptr;
        if (!ret && total > nlisted && !o.quiet)
            fprintf(stderr, "bzx: %s: %llu more hits not listed (--max-hits %llu): their lines are missing\n", name,
                    (unsigned long long)(total - nlisted), (unsigned long long)o.max_hits);
        if (!ret && o.count) {
            if (multi) printf("%s:", name);
            printf("%llu\n", (unsigned long long)nmatch);
        } else if (!ret && nmatch > 0x7FFFFFFFull) {
            if (!o.quiet) fprintf(stderr, "bzx: %s: more than 2^31 - 1 matching lines: lower --max-hits\n", name);
            ret = 1;
        } else if (!ret && nmatch) {
            const uint32_t count = (uint32_t)nmatch;
            const std::vector<uint64_t> ones(count, 1);
            std::vector<size_t> offs(count), gots(count);
            std::vector<int> status(count);
            uint32_t np = 0;
            bzx_records_pieces(e.data(), nblk, rb.data(), count, recs.data(), ones.data(), nullptr, nullptr, 0, &np);
            std::vector<uint64_t> bases(np), lens(np);
            std::vector<std::vector<uint8_t>> held(np);
            std::vector<bzx_piece> pieces(np);
            if (np && (rc = bzx_records_pieces(e.data(), nblk, rb.data(), count, recs.data(), ones.data(), bases.data(), lens.data(), np, &np)))
                ret = fail(o, "grep failed", name, nullptr, rc);
            FILE *in = ret ? nullptr : fopen(name, "rb");
            if (!ret && !in) ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
            for (uint32_t j = 0; !ret && j < np; j++) {      // (a piece may end up to 8 bytes behind the file)
                held[j].resize((size_t)lens[j]);
                if (fseeko(in, (off_t)bases[j], SEEK_SET) != 0) ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
                else if (fread(held[j].data(), 1, held[j].size(), in) != held[j].size() && ferror(in))
                    ret = fail(o, strerror(errno), name, nullptr, BZX_OK);
                pieces[j] = bzx_piece{held[j].data(), bases[j], lens[j]};
            }
            if (in) fclose(in);
            std::vector<uint8_t> out;
            size_t need = 0;
            for (int turn = 0; !ret && turn < 2; turn++) {   // room is known behind the locate step: at most one repeat
                out.resize(turn ? need : (size_t)std::min<uint64_t>(std::max<uint64_t>(info.out_bytes, 1), (uint64_t)64 << 20));
                rc = bzx_decompress_records_buffer(ctx, pieces.data(), np, e.data(), nblk, rb.data(), LINE_DELIM, count, recs.data(),
                                                   ones.data(), out.data(), out.size(), offs.data(), gots.data(), status.data(), &need);
                if (rc != BZX_E_OUTBUF || turn) break;
            }
            if (!ret && rc) ret = fail(o, "line read failed", name, ctx, rc);
            for (uint32_t i = 0; !ret && i < count; i++) {
                if (multi) printf("%s:", name);
                if (o.line_number) printf("%llu:", (unsigned long long)recs[i]);
                fwrite(out.data() + offs[i], 1, gots[i], stdout);
                if (!gots[i] || out[offs[i] + gots[i] - 1] != (uint8_t)LINE_DELIM) putchar(LINE_DELIM);     // (the unterminated last line)
            }
        }
    } catch (const std::bad_alloc &) {
        ret = fail(o, "out of memory", name, nullptr, BZX_E_NOMEM);
    }
    if (ix) bzx_index_end(ix);
    if (!ret && (fflush(stdout) != 0 || ferror(stdout))) ret = fail(o, strerror(errno), "standard output", nullptr, BZX_OK);
    return ret || damaged ? 2 : nmatch ? 0 : 1;
}

// The end of one file's work: output flushed and closed (or removed after a failure), input removed unless -k.
static int finish_file(const Opts &o, FILE *out, const std::string &oname, const std::string &f, int r)
{
    int wr = 0;                                  // the output is complete on disk only when flush and close succeed
    if (out && out != stdout) {
        if (fflush(out) != 0 || ferror(out)) wr = 1;
        if (fclose(out) != 0) wr = 1;
        if (wr && !r && !o.quiet) fprintf(stderr, "bzx: %s: %s\n", oname.c_str(), strerror(errno));
        if (r || wr) unlink(oname.c_str());      // never leave a partial output ...
        else if (!o.keep && f != "-") unlink(f.c_str());   // ... and never remove the input unless the output is whole
    } else if (out) {
        if (fflush(out) != 0 || ferror(out)) wr = 1;
    }
    return r | wr;
}

// Opens the output of input f (after the same checks, with the same messages, as C bzip2): 0, or 1 after a message.
static int open_output(const Opts &o, const std::string &f, bool std_in, FILE **out, std::string &oname)
{
    *out = nullptr;
    if (o.mode == TEST) return 0;
    if (std_in || o.to_stdout) {
        *out = stdout;
        return 0;
    }
    if (o.mode == ZIP) oname = f + ".bz2";
    else if (f.size() > 4 && f.compare(f.size() - 4, 4, ".bz2") == 0) oname = f.substr(0, f.size() - 4);
    else oname = f + ".out";
    struct stat sb;
    if (!o.force && stat(oname.c_str(), &sb) == 0) {
        if (!o.quiet) fprintf(stderr, "bzx: %s already exists (use -f)\n", oname.c_str());
        return 1;
    }
    *out = fopen(oname.c_str(), "wb");
    if (!*out) {
        if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", oname.c_str(), strerror(errno));
        return 1;
    }
    return 0;
}

// Small files waiting for one batched compression call, in argument order.
struct Pending {
    std::string name, oname;
    FILE *out;
    std::vector<uint8_t> data;
};
static const size_t BATCH_FILE_MAX = (size_t)16 << 20;     // larger files take the chunked path
static const size_t BATCH_BYTES = (size_t)256 << 20;       // input bytes per batch call
static const size_t BATCH_FILES = 512;                     // files per batch call (their outputs stay open until it)
static const uint32_t BATCH_SLABS = 320;                   // context slabs: a 256 MiB batch at -9 in one device round
static const uint32_t UNZIP_SLABS = 256;                   // ... of a streamed -d / -t: blocks per round (one per compute unit)

// -d / -t: the pending .bz2 files in one bzx_decompress_batch_buffer call.  A file whose status is not BZX_OK is
// decoded again on its own from memory through the stream path (do_unzip), which prints the one-file path's message
// and needs no guess of the output size.
static int flush_unzip_batch(const Opts &o, bzx_ctx *ctx, std::vector<Pending> &pend)
{
    const uint32_t n = (uint32_t)pend.size();
    std::vector<const uint8_t *> srcs(n);
    std::vector<uint8_t *> outs(n);
    std::vector<size_t> lens(n), caps(n), olens(n, 0);
    std::vector<int> status(n, BZX_E_NOMEM);
    std::vector<std::vector<uint8_t>> raw(n);
    int rc = BZX_OK;
    try {
        for (uint32_t i = 0; i < n; i++) {
            srcs[i] = pend[i].data.data();
            lens[i] = pend[i].data.size();
            caps[i] = lens[i] * 6 + (1 << 20);          // (a larger output: the stream path below)
            raw[i].resize(caps[i]);
            outs[i] = raw[i].data();
        }
    } catch (const std::bad_alloc &) {
        rc = BZX_E_NOMEM;
    }
    if (!rc) (void)bzx_decompress_batch_buffer(ctx, n, srcs.data(), lens.data(), outs.data(), caps.data(), olens.data(),
                                               status.data());
    int ret = 0;
    for (uint32_t i = 0; i < n; i++) {
        Pending &p = pend[i];
        int r = 0;
        if (status[i] != BZX_OK) {
            std::vector<uint8_t>().swap(raw[i]);
            r = do_unzip(o, ctx, nullptr, &p.data, p.out, p.name.c_str());
        } else if (p.out && fwrite(raw[i].data(), 1, olens[i], p.out) != olens[i]) {
            r = fail(o, strerror(errno), p.name.c_str(), nullptr, BZX_OK);
        }
        std::vector<uint8_t>().swap(raw[i]);
        ret |= finish_file(o, p.out, p.oname, p.name, r);
    }
    return ret;
}

static int flush_batch(const Opts &o, bzx_ctx *ctx, std::vector<Pending> &pend, size_t &pend_bytes)
{
    if (pend.empty()) return 0;
    if (o.mode != ZIP) {
        const int ret = flush_unzip_batch(o, ctx, pend);
        pend.clear();
        pend_bytes = 0;
        return ret;
    }
    const uint32_t n = (uint32_t)pend.size();
    std::vector<const uint8_t *> raws(n);
    std::vector<size_t> lens(n), offs(n, 0), olens(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        raws[i] = pend[i].data.data();
        lens[i] = pend[i].data.size();
    }
    const size_t cap = bzx_compress_batch_bound(n, lens.data());
    uint8_t *obuf = (uint8_t *)malloc(cap ? cap : 1);
    const int rc = obuf ? bzx_compress_batch_buffer(ctx, n, raws.data(), lens.data(), o.level, obuf, cap, offs.data(),
                                                    olens.data())
                        : BZX_E_NOMEM;
    // --with-index: stream i's slice of the call's index is the index of FILE.bz2 on its own
    const bzx_index_entry *ie = nullptr;
    const uint64_t *ifirst = nullptr;
    uint32_t icount = 0;
    int irc = BZX_OK;
    if (!rc && o.with_index) irc = bzx_compress_batch_get_index(ctx, &ie, &ifirst, &icount);
    if (!irc && o.with_index && !rc && icount != n) irc = BZX_E_STATE;
    int ret = 0;
    for (uint32_t i = 0; i < n; i++) {
        Pending &p = pend[i];
        int r = 0;
        if (rc) r = fail(o, "compression failed", p.name.c_str(), obuf ? ctx : nullptr, rc);
        else if (fwrite(obuf + offs[i], 1, olens[i], p.out) != olens[i]) r = fail(o, strerror(errno), p.name.c_str(), nullptr, BZX_OK);
        const int done = finish_file(o, p.out, p.oname, p.name, r);
        ret |= done;
        if (o.with_index && !done && irc) {
            ret |= fail(o, "no index", p.name.c_str(), ctx, irc);
        } else if (o.with_index && !done) {
            bzx_index_info info;
            memset(&info, 0, sizeof info);
            info.in_bytes = olens[i];
            info.out_bytes = lens[i];
            info.nblk = ifirst[i + 1] - ifirst[i];
            info.nstreams = 1;
            ret |= write_bzxi(o, p.oname + ".bzxi", ie + ifirst[i], info);
        }
    }
    free(obuf);
    pend.clear();
    pend_bytes = 0;
    return ret;
}

int main(int argc, char **argv)
{
    Opts o;
    int bad = 1;                                             // a usage error; 2, as grep's, when the command line asks for a find
    for (int i = 1; i < argc; i++)
        if (!strncmp(argv[i], "--find", 6) || !strcmp(argv[i], "--count") || !strncmp(argv[i], "--max-hits", 10) ||
            !strncmp(argv[i], "--grep", 6) || !strcmp(argv[i], "--line-number"))
            bad = 2;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-" || a[0] != '-') {
            o.files.push_back(a);
        } else if (a.rfind("--", 0) == 0) {
            if (a == "--help") { help(); return 0; }
            else if (a == "--version" || a == "--license") { printf("bzx, bzip2 block compression on MI355X; %s\n", bzx_version()); return 0; }
            else if (a == "--decompress") o.mode = UNZIP, o.mode_set = true;
            else if (a == "--compress") o.mode = ZIP, o.mode_set = true;
            else if (a == "--test") o.mode = TEST, o.mode_set = true;
            else if (a == "--stdout") o.to_stdout = true;
            else if (a == "--keep") o.keep = true;
            else if (a == "--force") o.force = true;
            else if (a == "--quiet") o.quiet = true;
            else if (a == "--verbose") o.verbose++;
            else if (a == "--small") {}
            else if (a == "--fast") o.level = 1;
            else if (a == "--best") o.level = 9;
            else if (a == "--index") o.index = true;
            else if (a == "--recover") o.recover = true;
            else if (a == "--with-index") o.with_index = true;
            else if (a == "--range" || a.rfind("--range=", 0) == 0) {
                const std::string v = a == "--range" ? (i + 1 < argc ? argv[++i] : "") : a.substr(8);
                const size_t c = v.find(':');
                const std::string x = v.substr(0, c), y = c == std::string::npos ? "" : v.substr(c + 1);
                if (x.empty() || y.empty() || x.size() > 19 || y.size() > 19 || x.find_first_not_of("0123456789") != std::string::npos ||
                    y.find_first_not_of("0123456789") != std::string::npos) {
                    fprintf(stderr, "bzx: --range takes OFF:LEN in bytes, e.g. 41000000000:65536 (got \"%s\")\n", v.c_str());
                    return bad;
                }
                o.range = true;
                o.range_off = strtoull(x.c_str(), nullptr, 10);
                o.range_len = strtoull(y.c_str(), nullptr, 10);
            }
            else if (a == "--lines") {                      // alone with --index; FIRST:COUNT behind it with -dc
                o.lines = true;
                const std::string v = i + 1 < argc ? argv[i + 1] : "";
                const size_t c = v.find(':');
                const std::string x = v.substr(0, c), y = c == std::string::npos ? "" : v.substr(c + 1);
                if (!x.empty() && !y.empty() && x.size() <= 19 && y.size() <= 19 && x.find_first_not_of("0123456789") == std::string::npos &&
                    y.find_first_not_of("0123456789") == std::string::npos) {
                    i++;
                    o.lines_range = true;
                    o.lines_first = strtoull(x.c_str(), nullptr, 10);
                    o.lines_count = strtoull(y.c_str(), nullptr, 10);
                }
            }
            else if (a == "--find" || a.rfind("--find=", 0) == 0) {
                if (a == "--find" && i + 1 >= argc) { fprintf(stderr, "bzx: --find takes a string\n"); return bad; }
                if (o.grep) { fprintf(stderr, "bzx: --grep does not go with --find\n"); return 2; }
                o.find = true;
                o.find_pat = a == "--find" ? argv[++i] : a.substr(7);
            }
            else if (a == "--find-hex" || a.rfind("--find-hex=", 0) == 0) {
                const std::string v = a == "--find-hex" ? (i + 1 < argc ? argv[++i] : "") : a.substr(11);
                if (v.empty() || v.size() % 2 || v.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos) {
                    fprintf(stderr, "bzx: --find-hex takes an even number of hex digits, e.g. 0d0a00ff (got \"%s\")\n", v.c_str());
                    return 2;
                }
                o.find = true;
                o.find_pat.clear();
                for (size_t k = 0; k < v.size(); k += 2) o.find_pat.push_back((char)strtoul(v.substr(k, 2).c_str(), nullptr, 16));
            }
            else if (a == "--grep" || a.rfind("--grep=", 0) == 0) {
                if (a == "--grep" && i + 1 >= argc) { fprintf(stderr, "bzx: --grep takes a string\n"); return bad; }
                if (o.find) { fprintf(stderr, "bzx: --grep does not go with --find\n"); return 2; }
                o.grep = true;
                o.find_pat = a == "--grep" ? argv[++i] : a.substr(7);
            }
            else if (a == "--grep-hex" || a.rfind("--grep-hex=", 0) == 0) {
                const std::string v = a == "--grep-hex" ? (i + 1 < argc ? argv[++i] : "") : a.substr(11);
                if (v.empty() || v.size() % 2 || v.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos) {
                    fprintf(stderr, "bzx: --grep-hex takes an even number of hex digits, e.g. 0d0a00ff (got \"%s\")\n", v.c_str());
                    return 2;
                }
                if (o.find) { fprintf(stderr, "bzx: --grep does not go with --find\n"); return 2; }
                o.grep = true;
                o.find_pat.clear();
                for (size_t k = 0; k < v.size(); k += 2) o.find_pat.push_back((char)strtoul(v.substr(k, 2).c_str(), nullptr, 16));
            }
            else if (a == "--line-number") o.line_number = true;
            else if (a == "--count") o.count = true;
            else if (a == "--max-hits" || a.rfind("--max-hits=", 0) == 0) {
                const std::string v = a == "--max-hits" ? (i + 1 < argc ? argv[++i] : "") : a.substr(11);
                if (v.empty() || v.size() > 19 || v.find_first_not_of("0123456789") != std::string::npos) {
                    fprintf(stderr, "bzx: --max-hits takes a number (got \"%s\")\n", v.c_str());
                    return 2;
                }
                o.max_hits = strtoull(v.c_str(), nullptr, 10);
            }
            else if (a == "--ranges" || a.rfind("--ranges=", 0) == 0) {
                o.ranges = a == "--ranges" ? (i + 1 < argc ? argv[++i] : "") : a.substr(9);
                if (o.ranges.empty()) { fprintf(stderr, "bzx: --ranges takes a file of OFF:LEN lines\n"); return bad; }
            }
            else if (a == "--devices" || a.rfind("--devices=", 0) == 0) {
                std::string list = a == "--devices" ? (i + 1 < argc ? argv[++i] : "") : a.substr(10);
                o.devices.clear();
                for (size_t p = 0; p <= list.size();) {
                    const size_t q = list.find(',', p) == std::string::npos ? list.size() : list.find(',', p);
                    const std::string t = list.substr(p, q - p);
                    if (t.empty() || t.size() > 4 || t.find_first_not_of("0123456789") != std::string::npos) {
                        fprintf(stderr, "bzx: --devices takes ordinals separated by commas, e.g. 0,1 (got \"%s\")\n", list.c_str());
                        return bad;
                    }
                    o.devices.push_back(atoi(t.c_str()));
                    p = q + 1;
                }
                if (o.devices.size() > BZX_MAX_DEVICES) {
                    fprintf(stderr, "bzx: --devices takes at most %d entries\n", BZX_MAX_DEVICES);
                    return bad;
                }
            }
            else { fprintf(stderr, "bzx: unexpected argument %s\n", a.c_str()); return bad; }
        } else {
            for (size_t k = 1; k < a.size(); k++) {
                const char c = a[k];
                if (c >= '1' && c <= '9') o.level = c - '0';
                else if (c == 'd') o.mode = UNZIP, o.mode_set = true;
                else if (c == 'z') o.mode = ZIP, o.mode_set = true;
                else if (c == 't') o.mode = TEST, o.mode_set = true;
                else if (c == 'c') o.to_stdout = true;
                else if (c == 'k') o.keep = true;
                else if (c == 'f') o.force = true;
                else if (c == 'q') o.quiet = true;
                else if (c == 'v') o.verbose++;
                else if (c == 's') {}
                else if (c == 'h') { help(); return 0; }
                else if (c == 'V' || c == 'L') { printf("bzx, bzip2 block compression on MI355X; %s\n", bzx_version()); return 0; }
                else { fprintf(stderr, "bzx: unexpected flag -%c\n", c); return bad; }
            }
        }
    }
    if (o.grep || o.line_number) {                           // (exit status 2 for every error, as grep's)
        const char *why = !o.grep ? "--line-number goes with --grep or --grep-hex"
                          : o.find ? "--grep does not go with --find"
                          : o.find_pat.empty() || o.find_pat.size() > BZX_FIND_MAX_PATTERN ? "--grep takes 1 to 256 bytes"
                          : o.find_pat.find((char)LINE_DELIM) != std::string::npos ? "--grep takes a pattern without a newline (no line holds one)"
                          : o.with_index || o.recover || o.range || !o.ranges.empty() || o.lines_range || o.mode_set || o.to_stdout
                              ? "--grep goes with --line-number, --count, --max-hits, --index, --index --lines, -q and -v only (not with "
                                "--find, --range, --ranges, --recover or --with-index)"
                          : o.lines && !o.index ? "--lines goes with --index"
                          : o.files.empty()     ? "--grep takes files"
                                                : nullptr;
        for (const std::string &f : o.files)
            if (!why && f == "-") why = "--grep needs a file that can be read again, not standard input";
        if (why) {
            fprintf(stderr, "bzx: %s\n", why);
            return 2;
        }
        bzx_ctx *ctx = nullptr;
        const int rc = bzx_ctx_create(0, UNZIP_SLABS, &ctx);
        if (rc) {
            fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
            return 2;
        }
        int worst = 1;
        for (const std::string &f : o.files) {
            const int r = do_grep(o, ctx, f);
            worst = r == 2 || worst == 2 ? 2 : r == 0 ? 0 : worst;
        }
        bzx_ctx_destroy(ctx);
        return worst;
    }
    if (o.find || o.count) {                                 // (exit status 2 for every error, as grep's)
        const char *why = !o.find ? "--count goes with --find, --find-hex, --grep or --grep-hex"
                          : o.find_pat.empty() || o.find_pat.size() > BZX_FIND_MAX_PATTERN ? "--find takes 1 to 256 bytes"
                          : o.with_index || o.recover || o.range || !o.ranges.empty() || o.lines_range || o.mode_set || o.to_stdout
                              ? "--find goes with --index, --index --lines, --count, --max-hits, -q and -v only"
                          : o.lines && !o.index ? "--lines goes with --index"
                          : o.files.empty()     ? "--find takes files"
                                                : nullptr;
        for (const std::string &f : o.files)
            if (!why && f == "-") why = "--find needs a file, not standard input";
        if (why) {
            fprintf(stderr, "bzx: %s\n", why);
            return 2;
        }
        bzx_ctx *ctx = nullptr;
        const int rc = bzx_ctx_create(0, UNZIP_SLABS, &ctx);
        if (rc) {
            fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
            return 2;
        }
        int worst = 1;
        for (const std::string &f : o.files) {
            const int r = do_find(o, ctx, f);
            worst = r == 2 || worst == 2 ? 2 : r == 0 ? 0 : worst;
        }
        bzx_ctx_destroy(ctx);
        return worst;
    }
    if (o.with_index) {
        const char *why = o.index || o.range || !o.ranges.empty() ? "--with-index does not go with --index, --range or --ranges"
                          : o.mode == UNZIP                        ? "--with-index goes with compression, not with -d"
                          : o.mode == TEST                         ? "--with-index goes with compression, not with -t"
                          : o.to_stdout ? "--with-index needs a FILE.bz2 to name the index after: not with -c"
                                        : nullptr;
        for (const std::string &f : o.files)
            if (!why && f == "-") why = "--with-index needs a FILE.bz2 to name the index after: not with standard input";
        if (!why && o.files.empty()) why = "--with-index needs a FILE.bz2 to name the index after: not with standard input";
        if (why) {
            fprintf(stderr, "bzx: %s\n", why);
            return 1;
        }
    }
    if (o.recover) {
        if (o.with_index || o.range || !o.ranges.empty() || o.mode_set) {
            fprintf(stderr, "bzx: --recover goes with --index, -c, -f, -q and -v only (not with -z, -d, -t, --range, --ranges or --with-index)\n");
            return 1;
        }
        if (o.files.empty()) { fprintf(stderr, "bzx: --recover takes files\n"); return 1; }
        for (const std::string &f : o.files)
            if (f == "-") { fprintf(stderr, "bzx: --recover needs a file that can be read again, not standard input\n"); return 1; }
        bzx_ctx *ctx = nullptr;
        const int rc = bzx_ctx_create(0, UNZIP_SLABS, &ctx);
        if (rc) {
            fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
            return 1;
        }
        int lost = 0, trouble = 0;
        for (const std::string &f : o.files) {
            const int r = do_recover(o, ctx, f);
            if (r == 1) trouble = 1;
            if (r == 2) lost = 2;
        }
        bzx_ctx_destroy(ctx);
        return trouble ? 1 : lost;
    }
    if (o.lines) {
        const char *why = o.with_index || o.recover || o.range || !o.ranges.empty()
                              ? "--lines does not go with --with-index, --recover, --range or --ranges"
                          : o.index && o.lines_range ? "--index --lines takes no FIRST:COUNT"
                          : !o.index && !o.lines_range ? "--lines goes with --index, or as -dc --lines FIRST:COUNT FILE.bz2"
                          : !o.index && (o.mode != UNZIP || !o.to_stdout) ? "--lines FIRST:COUNT goes with -dc"
                          : !o.index && (o.files.size() != 1 || o.files[0] == "-") ? "--lines FIRST:COUNT takes one file, not standard input"
                                                                                   : nullptr;
        if (why) {
            fprintf(stderr, "bzx: %s\n", why);
            return 1;
        }
        if (!o.index) {
            bzx_ctx *ctx = nullptr;
            const int rc = bzx_ctx_create(0, 0, &ctx);
            if (rc) {
                fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
                return 2;
            }
            const int ret = do_lines(o, ctx, o.files[0]);
            bzx_ctx_destroy(ctx);
            return ret;
        }
    }
    if (!o.ranges.empty()) {
        if (o.index || o.range) { fprintf(stderr, "bzx: --ranges does not go with --index or --range\n"); return 1; }
        if (o.mode != UNZIP || !o.to_stdout) { fprintf(stderr, "bzx: --ranges goes with -dc\n"); return 1; }
        if (o.files.size() != 1 || o.files[0] == "-") { fprintf(stderr, "bzx: --ranges takes one file, not standard input\n"); return 1; }
        bzx_ctx *ctx = nullptr;
        const int rc = bzx_ctx_create(0, 0, &ctx);
        if (rc) {
            fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
            return 2;
        }
        const int ret = do_ranges(o, ctx, o.files[0]);
        bzx_ctx_destroy(ctx);
        return ret;
    }
    if (o.index || o.range) {
        if (o.index && o.range) { fprintf(stderr, "bzx: --index and --range do not go together\n"); return 1; }
        if (o.range && (o.mode != UNZIP || !o.to_stdout)) { fprintf(stderr, "bzx: --range goes with -dc\n"); return 1; }
        if (o.files.empty() || (o.range && o.files.size() != 1)) {
            fprintf(stderr, o.range ? "bzx: --range takes one file\n" : "bzx: --index takes files\n");
            return 1;
        }
        for (const std::string &f : o.files)
            if (f == "-") { fprintf(stderr, "bzx: --index and --range need a file that can be read again, not standard input\n"); return 1; }
        bzx_ctx *ctx = nullptr;
        const int rc = bzx_ctx_create(0, o.index ? UNZIP_SLABS : 0, &ctx);
        if (rc) {
            fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
            return 2;
        }
        int ret = 0;
        for (const std::string &f : o.files) ret |= o.index ? do_index(o, ctx, f) : do_range(o, ctx, f);
        bzx_ctx_destroy(ctx);
        return ret;
    }
    if (o.files.empty()) o.files.push_back("-");
    // two or more named files, without -v: the small regular ones go through the batched entry points
    const bool batching = o.files.size() >= 2 && !o.verbose;
    bzx_ctx *ctx = nullptr;
    int rc = bzx_ctx_create(0, batching ? BATCH_SLABS : o.mode != ZIP ? UNZIP_SLABS : 0, &ctx);
    if (rc) {
        fprintf(stderr, "bzx: %s (the product has no CPU path)\n", bzx_strerror(rc));
        return 2;
    }
    bzx_mctx *mctx = nullptr;
    if (!o.devices.empty() && o.mode != ZIP) {
        if (o.verbose) fprintf(stderr, "bzx: --devices applies to compression only: ignored\n");
    } else if (!o.devices.empty()) {
        rc = bzx_mctx_create(o.devices.data(), (uint32_t)o.devices.size(), 0, &mctx);
        if (rc) {
            fprintf(stderr, "bzx: --devices: %s\n", bzx_strerror(rc));
            bzx_ctx_destroy(ctx);
            return 2;
        }
    }
    if (o.with_index && (rc = mctx ? bzx_mctx_keep_index(mctx, 1) : BZX_OK) == BZX_OK) rc = bzx_ctx_keep_index(ctx, 1);
    if (rc) {
        fprintf(stderr, "bzx: --with-index: %s\n", bzx_strerror(rc));
        bzx_mctx_destroy(mctx);
        bzx_ctx_destroy(ctx);
        return 2;
    }
    int ret = 0;
    std::vector<Pending> pend;
    size_t pend_bytes = 0;
    for (const std::string &f : o.files) {
        const bool std_in = f == "-";
        if (std_in && batching) ret |= flush_batch(o, ctx, pend, pend_bytes);
        FILE *in = std_in ? stdin : fopen(f.c_str(), "rb");
        if (!in) {
            if (!o.quiet) fprintf(stderr, "bzx: %s: %s\n", f.c_str(), strerror(errno));
            ret = 1;
            continue;
        }
        struct stat sb;
        const bool small = batching && !std_in && fstat(fileno(in), &sb) == 0 && S_ISREG(sb.st_mode) &&
                           (size_t)sb.st_size <= BATCH_FILE_MAX;
        if (batching && !small) {
            ret |= flush_batch(o, ctx, pend, pend_bytes);
        } else if (small && (pend_bytes + (size_t)sb.st_size > BATCH_BYTES || pend.size() >= BATCH_FILES)) {
            ret |= flush_batch(o, ctx, pend, pend_bytes);
        }
        std::string oname;
        FILE *out = nullptr;
        if (open_output(o, f, std_in, &out, oname)) {
            if (!std_in) fclose(in);
            ret = 1;
            continue;
        }
        if (small) {
            Pending p{f, oname, out, {}};
            p.data.reserve((size_t)sb.st_size);
            const bool ok = read_all(in, p.data);
            fclose(in);
            if (!ok) {
                ret |= finish_file(o, out, oname, f, fail(o, strerror(errno), f.c_str(), nullptr, BZX_OK));
                continue;
            }
            pend_bytes += p.data.size();
            pend.push_back(std::move(p));
            continue;
        }
        KeptIndex kept;
        const int r = o.mode == ZIP ? do_zip(o, ctx, mctx, in, out, f.c_str(), o.with_index ? &kept : nullptr)
                                    : do_unzip(o, ctx, in, nullptr, out, f.c_str());
        if (!std_in) fclose(in);
        const int done = finish_file(o, out, oname, f, r);
        ret |= done;
        // the index only beside a .bz2 that closed cleanly; a failure here leaves the .bz2 and costs the exit status
        if (o.with_index && !done) ret |= write_bzxi(o, oname + ".bzxi", kept.e.data(), kept.info);
    }
    ret |= flush_batch(o, ctx, pend, pend_bytes);
    bzx_mctx_destroy(mctx);
    bzx_ctx_destroy(ctx);
    return ret;
}
