"""What the CPU and GPU tests of the compressor's linked frames share
(DESIGN.md §21): the strict sequence parser with the frame's earlier output as
the decoded prefix, the crafted records at the boundary between a block and the
record in front of it, the rows of the recorded sizes and the mixed jobs.  Test
infrastructure only."""
from _compress_cases import BLOCK_LEN, id4_records, noise, pseudo_text
from _compress_dict_cases import _nz, parse_block_dict

B = 65536  # the block length of the crafted records, and the window

# the record lengths around one and two blocks of 64 KiB
LENGTHS = [B + 1, B + 12, B + 13, B + 14, B + 1024, 2 * B, 2 * B + 1]


def block_history(plain, i, block_len, dictionary=b""):
    """What lies in front of block i of a linked frame: the dictionary for
    block 0, the record's own last 65,536 bytes for every later block."""
    return bytes(dictionary) if i == 0 else plain[i * block_len - B:i * block_len]


def parse_block_linked(comp, plain, i, block_len, dictionary=b""):
    """_compress_dict_cases.parse_block_dict over block i of the record
    `plain`, the decoded prefix being the frame's earlier output: an offset
    never exceeds 65,535 and never reaches before the window."""
    at = i * block_len
    return parse_block_dict(comp, plain[at:at + block_len], block_history(plain, i, block_len, dictionary))


def rows_record():
    """400 rows of 48 noise bytes and 80 text bytes, the 51,200 bytes three
    times over: repeats that cross the 64 KiB boundaries."""
    nz, tx = noise(48 * 400, 3), pseudo_text(80 * 400, 3)
    return b"".join(nz[48 * i:48 * i + 48] + tx[80 * i:80 * i + 80] for i in range(400)) * 3


def size_rows():
    """[(name, record, block length)]: the rows of tests/golden/compress_linked_sizes.json;
    tests/golden/make_compress_linked_sizes.py builds the same records."""
    return [("text4x64k", pseudo_text(4 * B, 7), B), ("text16x64k", pseudo_text(16 * B, 11), B),
            ("text64k+1k", pseudo_text(B + 1024, 5), B), ("text300000_256k", pseudo_text(300000, 300001), 4 * B),
            ("rows3x51200", rows_record(), B)]


# What the statement gives on those rows, payload bytes.
RECORDED = [130176, 501667, 33943, 148973, 48059]


# ------------------------------------------------------------------ crafted
# Block 0 is zeros with planted noise and block 1 noise without a zero byte, as
# in _compress_dict_cases: every four bytes of a zero run share one table entry,
# so a planted string's entry is its own, and every case states block 1's
# sequences, so a collision shows.

def _b0(*planted):
    """65,536 bytes of zeros with (index from the end, bytes) planted: index k
    puts the string's first byte at position -k of block 1."""
    b = bytearray(B)
    for k, s in planted:
        b[B - k:B - k + len(s)] = s
    assert len(b) == B
    return bytes(b)


def crafted():
    """[(name, record of two blocks at 64 KiB, block 1's sequences)]"""
    cases = []
    S, tail = _nz(8, 41), _nz(20, 42)
    # the offset limit: 8 bytes 65,536 in front of their repeat stay literal
    # (position -65,536 is seeded and never valid), 65,535 in front they match;
    # at the block's first position and seven bytes into it
    cases.append(("distance65536", _b0((B, S)), S + tail, [(28, 0, 0)]))
    cases.append(("distance65535", _b0((B - 1, S)), S + tail, [(0, 65535, 8), (20, 0, 0)]))
    lead = _nz(7, 43)
    cases.append(("distance65536_at7", _b0((B - 7, S)), lead + S + tail, [(35, 0, 0)]))
    cases.append(("distance65535_at7", _b0((B - 8, S)), lead + S + tail, [(7, 65535, 8), (20, 0, 0)]))
    # a match that starts k bytes before the boundary and runs m bytes into the
    # block: k = 4 is the last seeded position, k = 4..11 put position 0 at
    # every place of the extension's first three dwords
    R0, fill = _nz(40, 44), _nz(30, 45)
    for k in (4, 5, 6, 7, 8, 9, 10, 11):
        for m in ((0, 1, 2, 3, 7, 40) if k >= 8 else (0, 1, 9, 40)):
            U = _nz(k, 46)
            rec = R0 + fill + U + R0[:m] + _nz(20, 47, first_not=R0[m] if m < 40 else fill[0])
            cases.append((f"cross_k{k}_m{m}", _b0((k, U)), rec, [(70, 70 + k, k + m), (20, 0, 0)]))
    # -3 .. -1 are not seeded: four bytes astride the boundary, the last three
    # of block 0 and the first of block 1, come again and are not found
    T3, first = _nz(3, 48), _nz(1, 49)
    body = first + _nz(30, 50, first_not=0) + T3 + first
    rec = body + _nz(20, 51, first_not=body[1])
    cases.append(("astride_not_seeded", _b0((3, T3)), rec, [(len(rec), 0, 0)]))
    # a candidate 6 bytes before the boundary, on a repeat of period 3: the
    # match runs from block 0 across position 0 into its own output, 300 bytes
    cases.append(("period3", _b0((60, b"abc" * 20)), b"abc" * 100 + _nz(20, 52, first_not=ord("a")),
                  [(0, 6, 300), (20, 0, 0)]))
    # the same string in the history and earlier in the block: the block's wins
    T = _nz(16, 53)
    a, gap = _nz(50, 54), _nz(33, 55, first_not=0)
    rec = a + T + gap + T + _nz(20, 56, first_not=gap[0])
    cases.append(("block_wins", _b0((56, T)), rec, [(50, 50 + 40 + 16, 16), (33, 16 + 33, 16), (20, 0, 0)]))
    # a last block of 13 bytes may hold one match (it starts at 0 or 1 and ends
    # at 8), one of 12 bytes is a literal run, and stored
    P = _nz(13, 57)
    cases.append(("last13", _b0((500, P[:8])), P, [(0, 500, 8), (5, 0, 0)]))
    cases.append(("last12", _b0((500, P[:8])), P[:12], [(12, 0, 0)]))
    return [(name, b0 + b1, want) for name, b0, b1, want in cases]


def stored_then_compressible():
    """Three blocks at 64 KiB: text, noise (stored), then the noise's last
    1,000 bytes again and text: block 2 reads what a stored block left.  (The
    table keeps the latest position per hash, 4,096 of the window's 65,533, so
    it is the near history that is found.)"""
    nz = noise(B, 61)
    return pseudo_text(B, 62) + nz + nz[-1000:] + pseudo_text(3000, 63)


def dict_only_record(d):
    """131,073 bytes whose second block begins with the dictionary's last 100
    bytes, which block 0 does not hold (second_block_from_dictionary's shape)."""
    text = pseudo_text(2 * B + 1, 8)
    rec = text[:B] + d[-100:] + text[B + 100:]
    assert d[-100:][:16] not in rec[:B]
    return rec


def linked_records():
    """[(name, record)]: every record of more than one 64 KiB block that the
    tests compress -- the lengths, the crafted ones, the stored block."""
    recs = [(f"text{n}", pseudo_text(n, n + 1)) for n in LENGTHS]
    recs += [(name, rec) for name, rec, _ in crafted()]
    recs.append(("stored_then_compressible", stored_then_compressible()))
    return recs


def mixed_jobs():
    """_compress_dict_cases.mixed_jobs extended by the linked records: every
    record laid out at an odd place of one input, the jobs in an order of their
    own, with jobs that overlap others and begin inside another's blocks ->
    (input, spans, the plaintext of every job)."""
    recs = [r for _, r in id4_records()] + [r for _, r in linked_records()]
    data, where = b"", []
    for i, r in enumerate(recs):
        data += b"\x55" * (1 + i % 3)  # no record starts aligned by accident
        where.append((len(data), len(r)))
        data += r
    order = list(range(len(recs)))[::-1]
    order = order[1::2] + order[0::2]  # out of order in in_off
    spans = [where[i] for i in order]
    big = max(where, key=lambda w: w[1])
    assert big[1] >= 2 * B + 1000
    spans += [(big[0] + 100, 70000), (big[0] + 3, 13), (big[0], big[1]), (big[0] + B - 7, B + 1000),
              (big[0] + 1, 2 * B)]
    return data, spans, [data[o:o + n] for o, n in spans]


assert BLOCK_LEN[4] == B
