"""What the CPU and GPU tests of the compressor with a dictionary share
(DESIGN.md §18): the text dictionary, a strict sequence parser that knows the
dictionary, and the crafted records at the edges of the rule -- the offset
limit across the boundary, matches that start in the dictionary and cross into
the record, the dictionary in front of every block.  Test infrastructure only."""
import struct

import _oracle as O
from _compress_cases import id4_records, noise, pseudo_text

DICT_TEXT = pseudo_text(100000, 7)  # its tails are the dictionaries of every length
DICT_LENGTHS = [1, 3, 4, 5, 63, 64, 65, 1000, 65535, 65536, 65537, 100000]


def text_dict(n):
    return DICT_TEXT[len(DICT_TEXT) - n:]


def parse_block_dict(comp, plain, dictionary):
    """_compress_cases.parse_block with the dictionary's used tail D as the
    decoded prefix: an offset reaches back to len(D) + start at most and never
    exceeds 65,535; the end rules are unchanged -> [(literals, offset, match
    length)], the last with offset 0 and match length 0."""
    D = bytes(dictionary)[-65536:] if dictionary else b""
    n, out, p, seqs = len(plain), bytearray(D), 0, []

    def ext(v):
        nonlocal p
        if v == 15:
            while True:
                b = comp[p]
                p += 1
                v += b
                if b != 255:
                    break
        return v

    while True:
        assert p < len(comp), "the block ends without a last sequence"
        tok = comp[p]
        p += 1
        lit = ext(tok >> 4)
        assert p + lit <= len(comp), "literals run past the block"
        out += comp[p:p + lit]
        p += lit
        if p == len(comp):
            assert tok & 15 == 0, "the last token names a match"
            seqs.append((lit, 0, 0))
            break
        off = comp[p] | (comp[p + 1] << 8)
        p += 2
        ml = ext(tok & 15) + 4
        start = len(out) - len(D)
        assert 1 <= off <= 65535 and off <= len(D) + start, f"offset {off} at {start}"
        assert start <= n - 12, f"a match starts at {start} of {n}: inside the last 12 bytes"
        assert start + ml <= n - 5, f"a match ends at {start + ml} of {n}: inside the last 5 bytes"
        for _ in range(ml):
            out.append(out[-off])
        seqs.append((lit, off, ml))
    assert bytes(out[len(D):]) == plain, "the block does not decode to the record"
    if n < 13:
        assert len(seqs) == 1, "a block under 13 bytes is one literal run"
    if len(seqs) > 1:
        assert seqs[-1][0] >= 5
    return seqs


# What the statement gives on the six rows of tests/golden/compress_dict_sizes.json,
# payload bytes; the 64 x 1 KiB total of the GPU test is the second.
RECORDED = [9006, 34707, 135539, 128417, 39305, 51280]


def dict_frame_blocks(frame):
    """_compress_cases.frame_blocks for a frame that may carry a dictionary id
    -> (flg, bd, content size or None, dictionary id or None, [(stored,
    payload, checksum or None)], content checksum or None, the header's
    length); asserts HC and that the frame ends where its bytes end."""
    assert frame[:4] == b"\x04\x22\x4d\x18"
    flg, bd = frame[4], frame[5]
    assert flg & 0xC2 == 0x40 and bd & 0x8F == 0, "version 01, no reserved bit"
    pos, size, did = 6, None, None
    if flg & 8:
        (size,) = struct.unpack_from("<Q", frame, pos)
        pos += 8
    if flg & 1:
        (did,) = struct.unpack_from("<I", frame, pos)
        pos += 4
    assert frame[pos] == (O.xxh32(frame[4:pos]) >> 8) & 0xFF, "HC covers FLG, BD, the size and the id"
    pos += 1
    hlen, blocks = pos, []
    while True:
        (w,) = struct.unpack_from("<I", frame, pos)
        pos += 4
        if w == 0:
            break
        n = w & 0x7FFFFFFF
        payload = frame[pos:pos + n]
        assert len(payload) == n
        pos += n
        ck = None
        if flg & 0x10:
            (ck,) = struct.unpack_from("<I", frame, pos)
            pos += 4
        blocks.append((bool(w >> 31), payload, ck))
    cck = None
    if flg & 4:
        (cck,) = struct.unpack_from("<I", frame, pos)
        pos += 4
    assert pos == len(frame)
    return flg, bd, size, did, blocks, cck, hlen


def reads_dictionary(seqs):
    """Whether a match of these sequences begins in front of the block."""
    at = 0
    for lit, off, ml in seqs:
        at += lit
        if off > at:
            return True
        at += ml
    return False


# ------------------------------------------------------------------ crafted
# Dictionaries of zeros with planted noise: every four bytes of a zero run
# share one table entry, so a planted string's entry is its own unless one of
# the few positions astride its ends collides -- the seeds below are ones under
# which none does, and every case states its sequences, so a collision shows.

def _nz(n, seed, first_not=None):
    """n bytes of noise without a zero byte, the first unequal to first_not."""
    b = bytearray(x or 1 for x in noise(n, seed))
    if n and first_not is not None and b[0] == first_not:
        b[0] = b[0] % 255 + 1
    return bytes(b)


def crafted():
    """[(name, dictionary, record, the first block's sequences)]"""
    cases = []
    # the offset limit across the boundary: 8 bytes unique to tail index 0 lie
    # 65,536 before record position 0, at tail index 1 they lie 65,535 before
    S = _nz(8, 41)
    tail = _nz(20, 42)
    cases.append(("distance65536", S + bytes(65536 - 8), S + tail, [(28, 0, 0)]))
    cases.append(("distance65535", b"\0" + S + bytes(65536 - 9), S + tail, [(0, 65535, 8), (20, 0, 0)]))
    # the same with 100,000 bytes: the tail begins 34,464 in
    cases.append(("distance65535_long", _nz(34464, 43) + b"\0" + S + bytes(65536 - 9), S + tail,
                  [(0, 65535, 8), (20, 0, 0)]))
    # a match that starts k bytes before D's end and runs m bytes into the
    # record: k = 8..11 are the four alignments of position 0 against the
    # extension's lanes (0, 1, 2 and 3 bytes of the dword astride on D's side);
    # m = 0 ends exactly at D's last byte
    R0 = _nz(40, 44)
    fill = _nz(30, 45)
    for k in (5, 6, 7, 8, 9, 10, 11, 64, 261, 262, 263):
        for m in ((0, 1, 2, 3, 7, 40) if k in (8, 9, 10, 11) else (0, 9)):
            U = _nz(k, 46)
            rec = R0 + fill + U + R0[:m] + _nz(20, 47, first_not=R0[m] if m < 40 else fill[0])
            cases.append((f"cross_k{k}_m{m}", bytes(1000) + U, rec, [(70, 70 + k, k + m), (20, 0, 0)]))
    # a candidate whose four bytes end 2 bytes before D's end (c = -6), on a
    # repeat of period 3: the match runs from D across position 0 into its own
    # output, 300 bytes, past one 256-byte step of the extension
    run = b"abc" * 100
    cases.append(("period3", bytes(500) + b"abc" * 20, run + _nz(20, 48, first_not=ord("a")),
                  [(0, 6, 300), (20, 0, 0)]))
    # the same hash in D and earlier in the block: the block's position wins
    T = _nz(16, 49)
    a, gap = _nz(50, 50), _nz(33, 51, first_not=0)
    rec = a + T + gap + T + _nz(20, 52, first_not=gap[0])
    cases.append(("block_wins", bytes(1000) + T + bytes(40), rec,
                  [(50, 50 + 40 + 16, 16), (33, 16 + 33, 16), (20, 0, 0)]))
    return cases


def second_block_from_dictionary():
    """(dictionary, record of 131,073 bytes): 64 KiB of text, then a second
    block that begins with the dictionary's last 100 bytes, then one byte."""
    d = text_dict(65536)
    text = pseudo_text(131073, 8)
    return d, text[:65536] + d[-100:] + text[65636:]


def mixed_jobs():
    """The shape of tests/test_gpu_compress.py's mixed_jobs: every record of the
    CPU lists laid out at odd places of one input, the jobs in an order of
    their own, with jobs that overlap others -> (input, spans, the plaintext
    of every job)."""
    recs = [r for _, r in id4_records()]
    data, where = b"", []
    for i, r in enumerate(recs):
        data += b"\x55" * (1 + i % 3)  # no record starts aligned by accident
        where.append((len(data), len(r)))
        data += r
    order = list(range(len(recs)))[::-1]
    order = order[1::2] + order[0::2]  # out of order in in_off
    spans = [where[i] for i in order]
    big = max(where, key=lambda w: w[1])
    spans += [(big[0] + 100, 70000), (big[0] + 3, 13), (big[0], big[1]), (big[0] + 65536 - 7, 65537)]
    return data, spans, [data[o:o + n] for o, n in spans]
