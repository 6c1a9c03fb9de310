"""What the compressor's CPU and GPU tests share: the seeded
pseudo-text, the record lists, a strict sequence parser and the frame
arithmetic restated.  Test infrastructure only."""
import random
import struct

KiB = 1024
MiB = 1 << 20
BLOCK_LEN = {4: 64 * KiB, 5: 256 * KiB, 6: 1 * MiB, 7: 4 * MiB}


def pseudo_text(n, seed):
    """n bytes of seeded pseudo-text: 600 made-up words drawn with a skew, with
    spaces, punctuation and line ends.  Integer arithmetic only (xorshift32), so
    every Python gives the same bytes; tests/golden/make_compress_sizes.py
    carries the same twelve lines."""
    s = [(seed * 2654435761 + 1) & 0xFFFFFFFF or 1]
    def r(k):
        x = s[0]; x ^= (x << 13) & 0xFFFFFFFF; x ^= x >> 17; x ^= (x << 5) & 0xFFFFFFFF; s[0] = x; return x % k
    abc = "etaoinshrdlucmfwypvbgkqjxz"
    vocab = ["".join(abc[min(r(26), r(26))] for _ in range(2 + r(9))) for _ in range(600)]
    out, size = [], 0
    while size < n:
        out.append(vocab[min(r(600), r(600), r(600))] + (" ", " ", " ", " ", ", ", ". ", "\n")[r(7)])
        size += len(out[-1])
    return "".join(out).encode()[:n]


def noise(n, seed):
    return random.Random(seed).randbytes(n)


# the record lengths of the round trip and of the device-equals-host test
LENGTHS_ID4 = [0, 1, 4, 12, 13, 14, 63, 64, 65, 65535, 65536, 65537, 131073]
LEN_ID5 = 300000


def record(n, kind="text"):
    return pseudo_text(n, n + 1) if kind == "text" else noise(n, n + 1) if kind == "noise" else bytes(n)


def id4_records():
    """[(name, bytes)]: text of every length, and noise and zeros of some."""
    recs = [(f"text{n}", record(n)) for n in LENGTHS_ID4]
    recs += [(f"noise{n}", record(n, "noise")) for n in (13, 65, 65537)]
    recs += [(f"zeros{n}", record(n, "zeros")) for n in (14, 65536, 131073)]
    return recs


def frame_bound(n, block_id=4, bck=False, cck=False, size=False):
    """The bound of include/lz4ada_hip.h, restated."""
    nb = -(-n // BLOCK_LEN[block_id or 4])
    return 7 + (8 if size else 0) + nb * (4 + (4 if bck else 0)) + n + 4 + (4 if cck else 0)


def frame_blocks(frame):
    """A strict walk of one modern frame -> (flg, bd, content size or None,
    [(stored, payload, checksum or None)], content checksum or None); asserts
    that the frame ends where its bytes end."""
    assert frame[:4] == b"\x04\x22\x4d\x18"
    flg, bd = frame[4], frame[5]
    assert flg & 0xC3 == 0x40 and bd & 0x8F == 0, "version 01, no dictionary id, no reserved bit"
    pos, size = 6, None
    if flg & 8:
        (size,) = struct.unpack_from("<Q", frame, pos)
        pos += 8
    pos += 1  # HC: checked by the decoders
    blocks = []
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
    return flg, bd, size, blocks, cck


def parse_block(comp, plain):
    """Walk every sequence of the compressed block `comp`, which must decode to
    `plain`, asserting the LZ4 end-of-block rules and the validity of every
    offset -> [(literals, offset, match length)], the last with offset 0 and
    match length 0.  Nothing is left to a lenient decoder."""
    n, out, p, seqs = len(plain), bytearray(), 0, []

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
        start = len(out)
        assert 1 <= off <= 65535 and off <= start, f"offset {off} at {start}"
        assert start <= n - 12, f"a match starts at {start} of {n}: inside the last 12 bytes"
        assert start + ml <= n - 5, f"a match ends at {start + ml} of {n}: inside the last 5 bytes"
        for _ in range(ml):
            out.append(out[-off])
        seqs.append((lit, off, ml))
    assert bytes(out) == plain, "the block does not decode to the record"
    if n < 13:
        assert len(seqs) == 1, "a block under 13 bytes is one literal run"
    if len(seqs) > 1:
        assert seqs[-1][0] >= 5
    return seqs
