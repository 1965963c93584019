"""Blocks for the bucket sorter's path tests (test_bsort_paths.py on the device, test_emu_bsort_paths.py through the
emulator): the same families at two scales.  Every builder is deterministic."""
import random


def letters(n, alphabet, seed):
    rnd = random.Random(seed)
    return bytes(rnd.choice(alphabet) for _ in range(n))


def writeout_lengths():
    """Every length 1..600 of one 3-letter text: bucket sizes of every residue mod 8, rotation 0 in every slot of a lane."""
    data = letters(600, b"abc", 11)
    return [data[:n] for n in range(1, 601)]


def long_runs(n, seed=5):
    """Two symbols, long stretches of one of them: the records of a bucket agree on whole 8-bit key digits."""
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += b"a" * rnd.randint(40, 200) + bytes(rnd.choice(b"ab") for _ in range(rnd.randint(1, 6))) + b"b"
    return bytes(out[:n])


def alphabet_block(n, k, seed=21):
    rnd = random.Random(seed + k)
    syms = rnd.sample(range(256), k)
    return bytes(rnd.choices(syms, [1.0 / (i + 1) for i in range(k)], k=n))


def with_phrase(text, length, copies, seed=7):
    """`copies` copies of one phrase of `length` symbols of the text's own alphabet (the symbol width stays), spread over
    the text, each between different neighbours."""
    rnd = random.Random(seed)
    syms = sorted(set(text))
    phrase = bytes(rnd.choice(syms) for _ in range(length))
    step = len(text) // copies
    parts = []
    for i in range(copies):
        parts += [text[i * step:(i + 1) * step if i + 1 < copies else len(text)], phrase]
    return b"".join(parts)


def with_copy(text, at, length):
    """A stretch of the text once more at its end: a repeat of `length` symbols."""
    return text + text[at:at + length] + b"!"
