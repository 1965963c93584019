"""Symbol streams for the Huffman and emit stage tests (test_huffman_edges.py, on the device and through the emulator):
streams no ordinary input produces.  A case is (mtfv, alpha): an array of uint16 symbols below alpha whose last one is
EOB (alpha - 1) and appears once.  freq_of() counts it, in_use_for() gives a symbol map with alpha - 2 bytes in use.
Every builder is deterministic (random.Random(seed) only).

retry_*       code lengths past 17 bits before libbz2's limiter halves the weights (certify() proves it)
fib25         a 17-bit code that needed no halving
heavy_groups  a group whose payload is 850 bits, fifty 17-bit codes (group_payloads() proves it)
thr_*         n_mtf at the table-count thresholds (2..6 tables), a small and a large alphabet
tile_*        selector counts around the 512-lane chunking of the selector MTF and the emitter's 512-group tiles,
              with the last group full, of one symbol and of 49; max_* the largest streams the ABI takes, max_flat
              the largest image (about 901 kB of the 921.6 kB a block's output slab holds)
empty_*       one symbol carries nearly everything: initial partitions without a symbol
uniform*      exactly uniform frequencies (ties in the heap), alphabets at the edges of the 64-lane loops
tie_groups_*  groups that cost the same under two tables: the first-minimum rule
"""
import random
from array import array

G = 50


def freq_of(mtfv):
    f = [0] * 258
    for s in mtfv:
        f[s] += 1
    return f


def in_use_for(alpha):
    """alpha - 2 byte values in use, spread over the sixteen words of the symbol map (37 is coprime to 256)."""
    m = bytearray(256)
    for i in range(alpha - 2):
        m[(i * 37) % 256] = 1
    return bytes(m)


def _finish(groups, alpha):
    out = array("H")
    for g in groups:
        out.extend(g)
    out.append(alpha - 1)
    return out, alpha


def retry_groups(alpha, n_b, seed):
    """Groups of two kinds, shuffled: kind A cut from a shuffled pool of symbols 0..18 with counts 2^s (filled up to
    whole groups with symbol 18), kind B uniform over the symbols 19..alpha-2.  EOB is a group of its own."""
    rnd = random.Random(seed)
    pool = [s for s in range(19) for _ in range(1 << s)]
    pool += [18] * (-len(pool) % G)
    rnd.shuffle(pool)
    groups = [pool[i:i + G] for i in range(0, len(pool), G)]
    rest = list(range(19, alpha - 1))
    groups += [rnd.choices(rest, k=G) for _ in range(n_b)]
    rnd.shuffle(groups)
    return _finish(groups, alpha)


def powers_of_two(seed):
    """19 symbols with counts 2^s, shuffled without grouping."""
    rnd = random.Random(seed)
    pool = [s for s in range(19) for _ in range(1 << s)]
    rnd.shuffle(pool)
    return _finish([pool], 20)


def fibonacci(k, seed):
    """k symbols with Fibonacci counts 1, 1, 2, 3, 5, ..., shuffled: the deepest tree a total allows."""
    rnd = random.Random(seed)
    a, b, pool = 1, 1, []
    for s in range(k):
        pool += [s] * a
        a, b = b, a + b
    rnd.shuffle(pool)
    return _finish([pool], k + 1)


def kinds(n_mtf, alpha, seed, n_kinds=7):
    """n_mtf symbols (EOB included) in 50-symbol groups of n_kinds kinds, each kind with symbols and geometric weights
    of its own, the kind changing every one to three groups: selectors that vary from group to group."""
    rnd = random.Random(seed)
    syms = list(range(alpha - 1))
    dist = []
    for _ in range(n_kinds):
        k = rnd.randint(1, min(len(syms), 24))
        sub = rnd.sample(syms, k)
        ratio = rnd.choice((0.5, 0.7, 0.9))
        dist.append((sub, [ratio ** i for i in range(k)]))
    out = array("H")
    body = n_mtf - 1
    while len(out) < body:
        sub, w = dist[rnd.randrange(n_kinds)]
        out.extend(rnd.choices(sub, w, k=G * rnd.randint(1, 3)))
    del out[body:]
    out.append(alpha - 1)
    return out, alpha


def dominant(n_mtf, alpha, dom, others, seed):
    """Symbol dom everywhere but for one occurrence of each of `others`, at seeded places."""
    rnd = random.Random(seed)
    body = [dom] * (n_mtf - 1)
    for pos, s in zip(rnd.sample(range(n_mtf - 1), len(others)), others):
        body[pos] = s
    return _finish([body], alpha)


def flat(n_mtf, alpha, seed):
    """Independent symbols, all equally likely: about eight bits each at alpha = 258, the largest image."""
    rnd = random.Random(seed)
    return _finish([rnd.choices(range(alpha - 1), k=n_mtf - 1)], alpha)


def uniform(alpha, times, seed):
    """Every symbol but EOB exactly `times` times, shuffled."""
    rnd = random.Random(seed)
    body = list(range(alpha - 1)) * times
    rnd.shuffle(body)
    return _finish([body], alpha)


def tie_groups(n_groups_of_stream, per_part, seed):
    """6 * per_part symbols of about equal frequency; every group holds 25 symbols of one range of per_part symbols and
    25 of another.  Where the initial partitions fall on those ranges (the counts are not exactly even, so this is
    approximate) a group costs the same under two tables in the first pass; nothing here proves a tie, the builder
    only makes them likely."""
    rnd = random.Random(seed)
    alpha = 6 * per_part + 1
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    groups = []
    for i in range(n_groups_of_stream):
        a, b = pairs[i % len(pairs)]
        g = [a * per_part + (i + j) % per_part for j in range(G // 2)] + [b * per_part + (i + j) % per_part for j in range(G // 2)]
        rnd.shuffle(g)
        groups.append(g)
    rnd.shuffle(groups)
    return _finish(groups, alpha)


def heavy_groups(scale, n_common, n_rare_groups, seed):
    """Six kinds of groups, each over n_common symbols of its own with counts scale * (1, 1, 2, 3, 5, ...), so that
    each of the six tables settles on one kind; every other symbol appears once, n_rare_groups groups hold 50 of them
    each.  Such a symbol weighs the least in every table and lies below the whole chain of the common ones: at
    scale 260 and nine common symbols at 16 or 17 bits, so a rare group's payload reaches 50 * 17 = 850 bits, all the
    10-bit group size field is made for."""
    rnd = random.Random(seed)
    fib, a, b = [], 1, 1
    for _ in range(n_common):
        fib.append(a * scale)
        a, b = b, a + b
    groups, common = [], set()
    for kind in range(6):
        syms = [kind * 43 + j for j in range(n_common)]
        common.update(syms)
        pool = [s for s, c in zip(syms, fib) for _ in range(c)]
        pool += [syms[-1]] * (-len(pool) % G)
        rnd.shuffle(pool)
        groups += [pool[i:i + G] for i in range(0, len(pool), G)]
    rare = [s for s in range(257) if s not in common]
    rnd.shuffle(rare)
    groups += [rare[i * G:(i + 1) * G] for i in range(n_rare_groups)]
    rnd.shuffle(groups)
    return _finish(groups, 258)


RETRY = {
    "retry_a21": lambda: retry_groups(21, 0, 1),
    "retry_a40": lambda: retry_groups(40, 200, 2),
    "retry_a258": lambda: retry_groups(258, 500, 3),
    "retry_pow2": lambda: powers_of_two(4),
}

LONG_NO_RETRY = {"fib25": lambda: fibonacci(25, 2)}
HEAVY = {"heavy_groups": lambda: heavy_groups(260, 9, 2, 1)}

THRESHOLDS = (1, 2, 49, 50, 51, 199, 200, 599, 600, 1199, 1200, 2399, 2400)
TILE_SELECTORS = (511, 512, 513, 1023, 1024, 1025)
MAX_N_MTF = 900001


def _others():
    c = {}
    for n in THRESHOLDS:
        for alpha in (4, 258):
            c[f"thr_{n}_a{alpha}"] = lambda n=n, alpha=alpha: kinds(n, alpha, 100 + n + alpha, 3)
    for ns in TILE_SELECTORS:
        for last in (G, 1, 49):                       # symbols in the last group
            n = (ns - 1) * G + last
            c[f"tile_{ns}_last{last}"] = lambda n=n, ns=ns: kinds(n, 90 if ns % 2 else 258, 200 + n)
    for n in (MAX_N_MTF - 2, MAX_N_MTF - 1, MAX_N_MTF):
        c[f"max_{n}"] = lambda n=n: kinds(n, 258, 300 + n, 9)
    c["max_flat"] = lambda: flat(MAX_N_MTF, 258, 16)
    c["empty_a3"] = lambda: dominant(2500, 3, 0, [1] * 5, 6)
    c["empty_a3_second"] = lambda: dominant(2500, 3, 1, [0] * 5, 7)
    c["empty_a258"] = lambda: dominant(3000, 258, 0, list(range(1, 257)), 8)
    c["empty_a258_mid"] = lambda: dominant(3000, 258, 130, [s for s in range(257) if s != 130], 9)
    c["empty_a258_three_used"] = lambda: dominant(2600, 258, 100, [7, 7, 200, 200, 200], 10)
    c["uniform_a258"] = lambda: uniform(258, 12, 11)
    for alpha in (3, 4, 64, 65, 128, 129, 257, 258):
        c[f"uniform_once_a{alpha}"] = lambda alpha=alpha: uniform(alpha, 1, 12 + alpha)
    for alpha in (3, 4, 64, 65, 128, 129, 257):
        c[f"uniform_a{alpha}"] = lambda alpha=alpha: uniform(alpha, 2500 // (alpha - 1) + 1, 13 + alpha)
    c["tie_groups_a37"] = lambda: tie_groups(600, 6, 14)
    c["tie_groups_a241"] = lambda: tie_groups(90, 40, 15)
    return c


CASES = {**RETRY, **LONG_NO_RETRY, **HEAVY, **_others()}


def max_depth_and_halvings(oracle, rfreq, alpha, limit=17):
    """Depth of libbz2's tree over rfreq without a limit, and the halvings of the weights that bring it to `limit`
    (bzo_make_code_lengths with the limit lifted, the halving done here)."""
    w = [max(f, 1) for f in rfreq[:alpha]]
    first = depth = max(oracle.make_code_lengths(w, alpha, 255))
    halvings = 0
    while depth > limit:
        w = [1 + x // 2 for x in w]
        halvings += 1
        depth = max(oracle.make_code_lengths(w, alpha, 255))
    return first, halvings


def final_tables(oracle, mtfv, alpha):
    """The oracle's final pass: [(frequencies of the table under the final selectors, its final lengths)]."""
    T = oracle.huff_full(mtfv, freq_of(mtfv), alpha)
    rfreq = [[0] * alpha for _ in range(T.n_groups)]
    for g in range(T.n_selectors):
        row = rfreq[T.selector[g]]
        for s in mtfv[g * G:(g + 1) * G]:
            row[s] += 1
    return [(rfreq[t], list(T.len[t][:alpha])) for t in range(T.n_groups)]


def certify(oracle, mtfv, alpha):
    """-> (most halvings any table of the final pass needed, longest final code, its unlimited depth)."""
    tabs = final_tables(oracle, mtfv, alpha)
    res = [max_depth_and_halvings(oracle, rf, alpha) for rf, _ in tabs]
    for (rf, lens), (_, h) in zip(tabs, res):
        # the oracle's own limiter agrees with the halving done here
        w = [max(f, 1) for f in rf]
        for _ in range(h):
            w = [1 + x // 2 for x in w]
        assert oracle.make_code_lengths(w, alpha, 255) == lens
    return max(h for _, h in res), max(max(lens) for _, lens in tabs), max(d for d, _ in res)


def group_payloads(oracle, mtfv, alpha):
    """Payload bits of every group under the oracle's final tables and selectors."""
    T = oracle.huff_full(mtfv, freq_of(mtfv), alpha)
    return [sum(T.len[T.selector[g]][s] for s in mtfv[g * G:(g + 1) * G]) for g in range(T.n_selectors)]
