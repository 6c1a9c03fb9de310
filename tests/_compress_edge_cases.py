"""The compressor's in-block edge cases, shared by the CPU file
that proves what they claim (tests/test_compress_edges_cpu.py) and the GPU file
that runs them through the three kernels (tests/test_gpu_compress_edges.py):
the extension ended at every place, literal runs and match lengths at the
token's and the extension's thresholds, blocks around the stored threshold, the
partial last window, the offset limit inside one block, small alphabets and the
emit kernel's alignments.  Seeded and deterministic.  Every family returns
[(name, record, its block's sequences or None)] and is built once.  Test
infrastructure only."""
import functools
import random

from _compress_cases import KiB, noise

A = noise(448, 11)  # seven windows of noise: every position of it is inserted
A1K = noise(1024, 11)  # sixteen; the first seven are A


def differing(data, byte):
    """data with its first byte made unequal to `byte`."""
    return bytes([data[0] ^ 1]) + data[1:] if data[0] == byte else data


def planted(lit, ml, seed=None):
    """Noise, a first repeat, `lit` bytes of noise, a repeat of exactly `ml`
    bytes from an inserted place, 20 bytes of noise -> (record, its sequences).
    The noise in front is A, or A1K where the match is longer than A holds."""
    base = A if 64 + ml < len(A) else A1K
    # (seeds under which no position of the run shares the source's hash)
    run = differing(noise(lit, 300 + lit if seed is None else seed), base[32])
    tail = differing(noise(20, 200 + ml), base[64 + ml])
    data = base + base[:32] + run + base[64:64 + ml] + tail
    at = len(base) + 32 + lit
    return data, [(len(base), len(base), 32), (lit, at - 64, ml), (20, 0, 0)]


def far_repeat(distance):
    """A 32-byte repeat whose only earlier copy lies `distance` back, at
    positions past 2^16 in a block of 256 KiB: zeros (one match: nothing inside
    it is inserted), 64 bytes of noise holding the source at 16, zeros again,
    the copy, 20 bytes of noise -> (record, where the copy begins)."""
    s = differing(noise(32, 31), 0)  # (a seed under which no later inserted position shares its hash)
    src = noise(16, 23) + s + noise(16, 24)
    tail = differing(noise(20, 22), src[48])
    return bytes(70000) + src + bytes(distance - 48) + s + tail, 70000 + 16 + distance


# ---------------------------------------------------------------- extension

MATCH_LENGTHS = [*range(4, 25), *range(250, 275), *range(505, 535)]  # steps 0, 1 and 2 of the extension


@functools.lru_cache(maxsize=None)
def extension_grid():
    """A match ended at every byte of a lane's dword in the extension's first
    three steps: by a mismatch (`mis`), and by the block's end, n - 5 (`end`)."""
    cases = []
    run = differing(noise(20, 320), A1K[32])
    for ml in MATCH_LENGTHS:
        tail = differing(noise(20, 200 + ml), A1K[64 + ml])
        cases.append((f"ext_mis_ml{ml}", A1K + A1K[:32] + run + A1K[64:64 + ml] + tail,
                      [(1024, 1024, 32), (20, 1012, ml), (20, 0, 0)]))
    for ml in MATCH_LENGTHS:
        if ml >= 7:  # a match that begins at n - 12 or before and ends at n - 5
            cases.append((f"ext_end_ml{ml}", A1K + A1K[64:64 + ml + 5], [(1024, 960, ml), (5, 0, 0)]))
    return cases


# ------------------------------------------------------------- length edges

# literal runs with a match of 40; 16,590 is the first whose 255s number 65, one
# more than the lanes.  The runs past 500 bytes carry seeds of their own, found
# by trying 1, 2, ...: ones under which none of the run's positions takes the
# table entry of the match's source.
LITERAL_RUNS = {14: None, 15: None, 16: None, 269: None, 270: None, 271: None, 524: 1, 525: 1, 526: 1,
                16589: 44, 16590: 44, 16591: 44, 16845: 44}
MATCH_EDGES = [18, 19, 20, 273, 274, 275, 528, 529, 530]  # after 20 literals


@functools.lru_cache(maxsize=None)
def length_edges():
    cases = [(f"lit{lit}", *planted(lit, 40, seed)) for lit, seed in LITERAL_RUNS.items()]
    return cases + [(f"ml{ml}", *planted(20, ml)) for ml in MATCH_EDGES]


# --------------------------------------------------------------- near bound

def near(n, at, length, src=0):
    """noise(n, 1000 + n) with the `length` bytes at `src` planted again at
    `at` and the byte after the copy made to differ: one match of exactly
    `length` -> (record, its sequences when nothing bounds the block)."""
    b = bytearray(noise(n, 1000 + n))
    b[at:at + length] = b[src:src + length]
    if b[at + length] == b[src + length]:
        b[at + length] ^= 1
    return bytes(b), [(at, at - src, length), (n - at - length, 0, 0)]


# The large blocks.  Late: the source cannot be the block's first bytes, whose
# table entry thousands of noise positions overwrite, so it lies 100 in front of
# the copy.  Early: (place, length) of a copy of the first bytes whose block
# comes out at exactly n - 1 and n (arithmetic: token, extensions, offset).
NEAR_LATE_SOURCE = 100
NEAR_EARLY = {8192: ((100, 39), (100, 38)), 65536: ((600, 263), (600, 262))}


@functools.lru_cache(maxsize=None)
def near_bound():
    """Blocks whose compressed form is a few bytes around their own length.
    `early` has the match at 100 (600 in the large blocks), `late` at
    n - 20 - L."""
    cases = []
    for n in (300, 600):
        for L in range(4, 14):
            cases.append((f"near_n{n}_early_L{L}", *near(n, 100, L)))
            cases.append((f"near_n{n}_late_L{L}", *near(n, n - 20 - L, L)))
    for n in (8192, 65536):
        for L in (4, 9, 13):
            at = n - 20 - L
            cases.append((f"near_n{n}_late_L{L}", *near(n, at, L, at - NEAR_LATE_SOURCE)))
        for at, L in NEAR_EARLY[n]:
            cases.append((f"near_n{n}_early_L{L}", *near(n, at, L)))
    return cases


# -------------------------------------------------------------- window tail

@functools.lru_cache(maxsize=None)
def window_tail():
    """A repeat of A's first k bytes at the record's end: it begins at n - k,
    so k = 11 stays literal and k >= 12 is a match of k - 5 bytes.  After 0..63
    bytes of noise the last window's length and the repeat's lane in it vary."""
    cases = []
    for pre in range(64):
        head = noise(pre, 500 + pre)
        for k in (11, 12, 13, 18, 19):
            rec = head + A + A[:k]
            want = [(len(rec), 0, 0)] if k < 12 else [(pre + len(A), len(A), k - 5), (5, 0, 0)]
            cases.append((f"tail_pre{pre}_k{k}", rec, want))
    return cases


# -------------------------------------------------------------- far repeats

@functools.lru_cache(maxsize=None)
def far_repeats():
    """The offset limit at positions past 2^17: one block of 256 KiB each; the
    tests also cut them into blocks of 64 KiB."""
    return [(f"far{d}", far_repeat(d)[0], None) for d in (65535, 65536)]


# ---------------------------------------------------------- small alphabets

def _symbols(r, a, n):
    return bytes(97 + r.randrange(a) for _ in range(n))


def copy_built(a, n, seed):
    """Random literals over `a` symbols interleaved with copies from earlier in
    the record: offsets 1..8 and 60..70, lengths 4..300."""
    r = random.Random(seed)
    out = bytearray(_symbols(r, a, 70))
    while len(out) < n:
        if r.random() < 0.4:
            out += _symbols(r, a, r.randint(1, 24))
        else:
            off = r.choice((1, 2, 3, 4, 5, 6, 7, 8, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70))
            for _ in range(r.randint(4, 300)):
                out.append(out[-off])
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def small_alphabets():
    """The fuzz: windows with many valid lanes, hashes shared inside an
    inserted prefix, offsets of 1..8.  The name carries alphabet, length, seed."""
    cases = []
    for a in (2, 3, 4, 16):
        for n in [*range(141), 500, 4096, 5000]:
            seed = 10000 * a + n
            cases.append((f"alpha{a}_len{n}_seed{seed}", _symbols(random.Random(seed), a, n), None))
    for a in (3, 4):
        for i in range(62):
            n, seed = 300 + 370 * i, 100 * a + i
            cases.append((f"copies{a}_len{n}_seed{seed}", copy_built(a, n, seed), None))
    return cases


# --------------------------------------------------------- alignment ladder

@functools.lru_cache(maxsize=None)
def alignment_ladder():
    """Noise of every length 0..100 (stored) and two-symbol records of every
    length 13..113 (compressed from 76 bytes on, where they shrink: the first
    window finds an empty table, so no match begins before position 64), in a
    seeded order: laid out in step, a frame's place mod 4 would follow from its
    length mod 8.  (The seed is one under which the few compressed blocks meet
    all 16 combinations; tests/test_compress_edges_cpu.py asserts it.)"""
    cases = [(f"ladder_noise{i}", noise(i, 700 + i), None) for i in range(101)]
    cases += [(f"ladder_two{13 + i}", _symbols(random.Random(800 + i), 2, 13 + i), None) for i in range(101)]
    random.Random(7).shuffle(cases)
    return cases


# ------------------------------------------------------------------ layouts

def laid_out(records, pad=3, shuffle=True):
    """The records at odd places of one input -- 1 + i % pad bytes in front of
    the i-th -- and the jobs in an order of their own -> (input, spans, the
    order: job j is record order[j])."""
    data, where = bytearray(), []
    for i, r in enumerate(records):
        data += b"\x55" * (1 + i % pad)
        where.append((len(data), len(r)))
        data += r
    order = list(range(len(records)))
    if shuffle:
        order = order[::-1]
        order = order[1::2] + order[0::2]
    return bytes(data), [where[i] for i in order], order


def in_block_cases(far_cut=True):
    """The list the plain, the dictionary and the decode tests share:
    (name, record) of every family about one block's inside."""
    cases = [*extension_grid(), *length_edges(), *near_bound(), *window_tail()]
    if far_cut:
        cases += far_repeats()  # with the default block: five blocks of 64 KiB
    return [(name, rec) for name, rec, _ in cases]


EDGE_DICT = noise(1000, 77)  # seeds the table and matches nothing the cases plan
B0 = noise(64 * KiB, 78)  # block 0 in front of a case that is block 1 of a linked record


@functools.lru_cache(maxsize=None)
def continuation_cases():
    """[(name, record of two blocks at 64 KiB, block 1's sequences)]: the
    extension grid thinned to every third length and the length edges under
    16,000 bytes, each behind 64 KiB of noise."""
    keep = {*range(4, 25, 3), *range(250, 275, 3), *range(505, 535, 3)}
    cases = [c for c in extension_grid() if int(c[0].split("ml")[1]) in keep]
    cases += [c for c in length_edges() if len(c[1]) < 16000]
    return [(name, B0 + rec, want) for name, rec, want in cases]
