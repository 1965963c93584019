"""A plain writer of the bzip2 format, for tests of the decompressor.

It writes the format and makes none of an encoder's choices: per block the caller may choose the Huffman tables and
their code lengths (start value of the delta coding included), the selector list (longer than the payload needs, or
given as raw MTF indices), the randomised bit, origPtr, the symbol map and the raw 3-bit nGroups and 15-bit
nSelectors fields.  Whatever is not chosen comes from the CPU oracle (oracle/, the checker of the compressor): its
BWT, MTF/RLE2 and Huffman stages.  Fed the oracle's choices, the writer reproduces oracle.compress_block and
bz2.compress byte for byte (tests/test_decode_shapes.py), which is what makes the unusual streams it writes
trustworthy.

Streams it can write that libbz2 never writes: 2..6 tables whatever the block size, any number of selectors up to
32767, code lengths up to 20, incomplete prefix codes, RLE1 images given directly (runs that end the block without a
count byte, count bytes above 251), blocks longer than the level allows, set randomised bits.
"""

import functools

BLOCK_MAGIC = 0x314159265359
EOS_MAGIC = 0x177245385090


class BitWriter:
    """MSB-first bit packer over a Python integer; whole bytes leave the accumulator as soon as there are eight."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, nbits, value):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc >> (self.n - 8 * k)).to_bytes(k, "big")
            self.n -= 8 * k
            self.acc &= (1 << self.n) - 1

    @property
    def bits(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        """The bytes written so far, the last one padded with zero bits."""
        pad = -self.n % 8
        tail = (self.acc << pad).to_bytes((self.n + pad) // 8, "big")
        return bytes(self.out) + tail


def stream_crc(block_crcs):
    c = 0
    for b in block_crcs:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ b
    return c


def rle1_decode(img):
    """The bytes an RLE1 image stands for: after four equal bytes the next byte is a repeat count (0..255)."""
    out = bytearray()
    last, cnt, i = None, 0, 0
    while i < len(img):
        ch = img[i]
        if cnt == 4:
            out += bytes([last]) * ch
            cnt, last = 0, None
        else:
            cnt = cnt + 1 if ch == last else 1
            last = ch
            out.append(ch)
        i += 1
    return bytes(out)


def canonical_codes(lens):
    """Code values of canonical prefix codes for the given lengths (shorter first, then by symbol), as libbz2
    assigns them; valid for incomplete codes too."""
    ok = [l for l in lens if 1 <= l <= 20]
    code = [0] * len(lens)
    if not ok:
        return code
    vec = 0
    for n in range(min(ok), max(ok) + 1):
        for i, l in enumerate(lens):
            if l == n:
                code[i] = vec
                vec += 1
        vec <<= 1
    return code


def selectors_to_mtf(sel):
    """Table indices -> the MTF indices the stream stores (unary coded)."""
    order = list(range(6))
    out = []
    for s in sel:
        j = order.index(s)
        out.append(j)
        order.insert(0, order.pop(j))
    return out


def lengths_with_max(alpha, maxlen, freq=None):
    """Code lengths for `alpha` symbols whose longest code is exactly `maxlen`.  Complete when alpha > maxlen (a chain
    1, 2, .., maxlen, maxlen whose shortest leaves are split until there are alpha of them), incomplete otherwise
    (1, 2, .., alpha - 1, maxlen).  The shortest codes go to the most frequent symbols when `freq` is given."""
    assert 2 <= alpha <= 258 and 2 <= maxlen <= 20
    if alpha <= maxlen:
        leaves = list(range(1, alpha)) + [maxlen]
    else:
        leaves = list(range(1, maxlen)) + [maxlen, maxlen]
        while len(leaves) < alpha:
            i = min((l, i) for i, l in enumerate(leaves) if l < maxlen)[1]
            leaves[i] += 1
            leaves.append(leaves[i])
    leaves.sort()
    rank = sorted(range(alpha), key=lambda s: -(freq[s] if freq else 0))
    lens = [0] * alpha
    for r, s in enumerate(rank):
        lens[s] = leaves[r]
    return lens


class Block:
    """One block: its RLE1 image and the choices the writer should make for it (None = the oracle's choice).

    image        the RLE1 image, the input of the BWT (any bytes: a count byte may be 0..255, a block may end inside
                 a run)
    crc          stored block CRC; default: CRC of the bytes the image stands for
    tables       code lengths per table, alpha entries each; lengths outside 1..20 are written as deltas that reach
                 them (the payload of such a stream is written with the lengths clamped)
    starts       5-bit start values of the first tables' delta coding; default: the table's first length
    selectors    table index of every selector; may run past the last group (the extra ones are written, and ignored
                 by a decoder); default: the oracle's, or table 0 for every group when `tables` is given
    selector_mtf raw MTF indices of the selectors, written as they are (overrides `selectors` in the header)
    n_groups     raw 3-bit field; default len(tables)
    n_selectors  raw 15-bit field; default the number of selectors written
    randomised   the randomised bit
    orig_ptr     24-bit origPtr; default the BWT's
    in_use       256 flags written as the symbol map; default: the bytes of the BWT
    """

    def __init__(self, image, crc=None, tables=None, starts=None, selectors=None, selector_mtf=None, n_groups=None,
                 n_selectors=None, randomised=0, orig_ptr=None, in_use=None):
        self.image = bytes(image)
        self.crc, self.tables, self.starts = crc, tables, starts
        self.selectors, self.selector_mtf = selectors, selector_mtf
        self.n_groups, self.n_selectors = n_groups, n_selectors
        self.randomised, self.orig_ptr, self.in_use = randomised, orig_ptr, in_use

    def raw(self):
        return rle1_decode(self.image)


@functools.lru_cache(maxsize=8)
def analyse(oracle, image):
    """The oracle's stages over an image: (L column, origPtr, mtfv incl. EOB, freq, in_use, n_in_use)."""
    L, orig = oracle.bwt(image)
    mtfv, freq, in_use, niu = oracle.mtf(L)
    return L, orig, mtfv, freq, in_use, niu


def write_block(bw, oracle, blk, fields=None):
    """Appends one block (magic to last payload bit) to BitWriter bw; returns the stored CRC.  `fields`, when given,
    gets the bit range [start, end) of every part of the block, keyed by name."""
    def mark(name, start):
        if fields is not None:
            fields.setdefault(name, []).append((start, bw.bits))

    img = blk.image
    L, orig, mtfv, freq, in_use, niu = analyse(oracle, img)
    alpha = niu + 2
    crc = blk.crc if blk.crc is not None else oracle.crc32(blk.raw())
    tables, sel = blk.tables, blk.selectors
    if tables is None:
        ng, osel, olens, _ = oracle.huff(mtfv, freq, alpha)
        tables = olens
        sel = osel if sel is None else sel
    elif sel is None:
        sel = [0] * ((len(mtfv) + 49) // 50)
    smtf = blk.selector_mtf if blk.selector_mtf is not None else selectors_to_mtf(sel)

    s = bw.bits
    bw.put(48, BLOCK_MAGIC)
    mark("magic", s)
    s = bw.bits
    bw.put(32, crc)
    mark("crc", s)
    s = bw.bits
    bw.put(1, blk.randomised)
    mark("randomised", s)
    s = bw.bits
    bw.put(24, orig if blk.orig_ptr is None else blk.orig_ptr)
    mark("orig_ptr", s)
    s = bw.bits
    use = blk.in_use if blk.in_use is not None else [b != 0 for b in in_use]
    l1 = 0
    for i in range(16):
        if any(use[i * 16:i * 16 + 16]):
            l1 |= 1 << (15 - i)
    bw.put(16, l1)
    for i in range(16):
        if l1 >> (15 - i) & 1:
            w = 0
            for j in range(16):
                if use[i * 16 + j]:
                    w |= 1 << (15 - j)
            bw.put(16, w)
    mark("symbol_map", s)
    s = bw.bits
    bw.put(3, len(tables) if blk.n_groups is None else blk.n_groups)
    mark("n_groups", s)
    s = bw.bits
    bw.put(15, len(smtf) if blk.n_selectors is None else blk.n_selectors)
    mark("n_selectors", s)
    s = bw.bits
    for j in smtf:
        bw.put(j + 1, ((1 << j) - 1) << 1)          # j ones, one zero
    mark("selectors", s)
    s = bw.bits
    for t, lens in enumerate(tables):
        cur = blk.starts[t] if blk.starts is not None and t < len(blk.starts) else lens[0]
        bw.put(5, cur)
        for target in lens:
            while cur < target:
                bw.put(2, 2)
                cur += 1
            while cur > target:
                bw.put(2, 3)
                cur -= 1
            bw.put(1, 0)
    mark("tables", s)
    s = bw.bits
    lens_ok = [[min(max(l, 1), 20) for l in lens] for lens in tables]
    codes = [canonical_codes(lens) for lens in lens_ok]
    put = bw.put
    for g in range((len(mtfv) + 49) // 50):
        t = sel[g] if g < len(sel) and sel[g] < len(tables) else 0
        ln, cd = lens_ok[t], codes[t]
        for v in mtfv[g * 50:g * 50 + 50]:
            put(ln[v], cd[v])
    mark("payload", s)
    return crc


def write_stream(oracle, blocks, level=9, combined_crc=None, fields=None):
    """One stream: 'BZh' + level digit, the blocks, the end-of-stream marker and the combined CRC (default: the one
    the blocks' CRCs give).  A `level` above 9 is written as that raw byte instead of a digit.  Returns the bytes."""
    bw = BitWriter()
    s = bw.bits
    bw.put(24, 0x425A68)
    bw.put(8, (0x30 + level) if level <= 9 else level)
    if fields is not None:
        fields.setdefault("stream_header", []).append((s, bw.bits))
    crcs = [write_block(bw, oracle, b, fields) for b in blocks]
    s = bw.bits
    bw.put(48, EOS_MAGIC)
    if fields is not None:
        fields.setdefault("eos", []).append((s, bw.bits))
    s = bw.bits
    bw.put(32, stream_crc(crcs) if combined_crc is None else combined_crc)
    if fields is not None:
        fields.setdefault("stream_crc", []).append((s, bw.bits))
    return bw.getvalue()


def block_bits(oracle, blk):
    """The block alone, as oracle.compress_block returns it: (bytes, pad bits of the last byte)."""
    bw = BitWriter()
    write_block(bw, oracle, blk)
    return bw.getvalue(), -bw.bits % 8
