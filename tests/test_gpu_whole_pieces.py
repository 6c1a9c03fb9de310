"""Pass 2's cut of literal runs and HBM-sourced matches into 16-byte pieces
(k_decode_idx, lz4ada_idx.hip decode_block): a run's own lane stores its
LAST piece with the exact-length store, the pieces before it are dealt over
the wave and stored as 16 whole bytes.  Blocks built here sequence by
sequence, deterministically (no generator of csrc/lz4gen.cpp), put every
run length around the piece sizes at ordinary places and around the LDS
output ring's end (every multiple of 8,192 output bytes), where a store
takes the wave-uniform fallback; the bytes are compared with the oracle's.

Overflow stretches (more than 64, and more than 128, dealt HBM pieces in one
batch: the borrowed-slot path and M's load-and-wait loop) are in the blocks
too.  No status or stamp hook tells Python which of those paths a batch
took -- the per-phase counters exist only in the diagnostic stamps build --
so the test checks their bytes, not that they ran: the stretches are sized
(4 to 6, and 8 to 12, matches of 300 bytes = 18 dealt pieces each, back to
back) so that a batch holding one whole has 72 to 108, or 144 to 216,
dealt pieces.

The linked frame puts quirk D1 matches of 17, 32 and 33 bytes (piece 0 of
such a match is a dealt piece, and the D1 bytes must land on top of it)
after literals and right after a match, once with enough long far matches
before them in the batch that the D1 match's dealt pieces are beyond the
64th (stored by M's loop in the linked planes' kernels)."""
import struct

import pytest

import _oracle as O
import lz4ada
import lz4frame
from test_gpu_linked import oracle, want_path
from test_gpu_parity import _run_variant_alone, oracle_blocks

pytestmark = pytest.mark.gpu

KiB = 1024
RING = 8192          # the LDS output ring: a store wraps at its multiples
BMAX = 256 * KiB
PREFIX = 66000       # output before the first case: every offset up to 65,535 is valid

LIT_LENS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255 + 15]
HBM_LENS = [4, 15, 16, 17, 31, 32, 33, 48, 49, 300]
HBM_OFFS = [4200, 65535, 8200, 12345, 4300, 40000, 8176, 30001]
# from 8,176 back a match is HBM-sourced wherever it lies in its batch (a
# batch holds at most 4,080 bytes, the threshold lies 4,096 + 16 before it);
# nearer ones are where their batch begins close enough before them
FAR_OFFS = [o for o in HBM_OFFS if o >= 8176]


def _ext(n):
    out = b""
    while n >= 255:
        out += b"\xff"
        n -= 255
    return out + bytes([n])


class Block:
    """One LZ4 block, sequence by sequence; literal bytes from a counter."""

    def __init__(self, salt):
        self.out, self.comp, self.i = bytearray(), bytearray(), salt

    def _lits(self, n):
        b = bytes((((self.i + j) * 2654435761) >> 11) & 0xff for j in range(n))
        self.i += n
        return b

    def seq(self, L, off, ml):
        lits = self._lits(L)
        assert ml >= 4 and 1 <= off <= min(len(self.out) + L, 65535), (L, off, ml, len(self.out))
        m = ml - 4
        self.comp += bytes([(min(L, 15) << 4) | min(m, 15)])
        if L >= 15:
            self.comp += _ext(L - 15)
        self.comp += lits + struct.pack("<H", off)
        if m >= 15:
            self.comp += _ext(m - 15)
        self.out += lits
        for _ in range(ml):
            self.out.append(self.out[-off])

    def fill(self, target):
        """Short literal runs and short near matches up to output position
        `target` exactly."""
        near = (1, 3, 8, 15, 16, 33, 200, 1500)
        assert target == len(self.out) or target - len(self.out) >= 8, (target, len(self.out))
        while target - len(self.out) >= 48:
            L = 4 + self.i % 13
            self.seq(L, min(near[self.i % 8], len(self.out) + L), 4 + self.i % 3)
        r = target - len(self.out)
        if r >= 24:
            self.seq(r - 16 - 4, 7, 4)
            r = 16
        if r:
            self.seq(r - 4, 5, 4)
        assert len(self.out) == target

    def at_ring_end(self, before, need):
        """Fill so that the next sequence starts `before` bytes ahead of the
        next multiple of RING that leaves room; False if the block is full."""
        b = (len(self.out) + before + 64 + RING - 1) // RING * RING
        if b + need + 64 > BMAX:
            return False
        self.fill(b - before)
        return True

    def finish(self, tail):
        lits = self._lits(tail)
        self.comp += bytes([min(tail, 15) << 4]) + (_ext(tail - 15) if tail >= 15 else b"") + lits
        self.out += lits
        assert len(self.out) <= BMAX
        return bytes(self.comp), bytes(self.out)


def _cuts(n):
    """Bytes of an n-byte run that lie before the ring's end: the run's
    edges, inside its first piece, at and inside its last piece (16 (K - 1)
    on), inside a middle piece."""
    last = 16 * ((n - 1) // 16)
    js = {0, n, 1, n - 1, last, last + 1}
    if last:
        js |= {8, last - 8}
    return sorted(j for j in js if 0 <= j <= n)


def _cases():
    """Every crafted sequence as (literals, offset, match length, bytes of
    the run before the ring's end or None for an ordinary place, whether the
    run is the match).  A literal case is followed by a 4-byte match."""
    cs, k = [], 0
    for L in LIT_LENS:
        cs.append((L, 5, 4, None, False))
        cs += [(L, 5, 4, j, False) for j in _cuts(L)]
    for ml in HBM_LENS:
        for j in [None, None] + _cuts(ml):
            offs = HBM_OFFS if j is None else FAR_OFFS  # at the ring's end: HBM-sourced for certain
            cs.append((3 * (k & 1), offs[k % len(offs)], ml, j, True))
            k += 1
    # overflow past 64 / 128 dealt pieces: far matches of 300 bytes back to
    # back, zero or two literals; each stretch once across the ring's end
    for g in (4, 5, 6, 8, 10, 12):
        for j in (None, 700):
            cs.append(("stretch", g, 300, j, True))
    return cs


def build_crafted():
    """(frame, decoded blocks): the cases laid out over 256 KiB independent
    blocks, final literal-only sequences of 1, 16 and 17 bytes in turn."""
    blocks, tails = [], [1, 16, 17]

    def new_block():
        b = Block(1000 * len(blocks) + 7)
        b.seq(40, 9, 4)
        b.fill(PREFIX)
        return b

    def close(b):
        c, r = b.finish(tails[len(blocks) % 3])
        blocks.append((c, r, False))

    b = new_block()
    for L, off, ml, j, is_match in _cases():
        n = (2 + ml) * off if L == "stretch" else L + ml
        while True:
            if j is None:
                ok = len(b.out) + 200 + n + 64 <= BMAX
                if ok:
                    b.fill(len(b.out) + 100 + len(blocks))
            else:
                ok = b.at_ring_end(j + (L if is_match and L != "stretch" else 0), n)
            if ok:
                break
            close(b)
            b = new_block()
        if L == "stretch":
            for i in range(off):
                b.seq(2 * (i & 1), 20000 + 37 * i, ml)
        else:
            b.seq(L, off, ml)
    b.fill(len(b.out) + 300)
    close(b)
    assert len(blocks) >= 3  # every final-sequence length occurs
    frame, _ = lz4frame.build_frame(blocks, BMAX, indep=True)
    return frame, [r for _, r, _ in blocks]


@pytest.fixture(scope="module")
def crafted():
    return build_crafted()


def test_crafted_layout(crafted):
    """The construction itself: blocks of 128 to 256 KiB whose cases lie
    where the docstring says (checked on the sequence list, no decode)."""
    frame, raws = crafted
    assert all(128 * KiB <= len(r) <= BMAX for r in raws[:-1]) and len(raws[-1]) <= BMAX
    lit_last, hbm_last = set(), set()
    for L, off, ml, j, is_match in _cases():
        if L == "stretch" or j is None:
            continue
        n = ml if is_match else L
        assert not is_match or 8176 <= off <= 65535
        if 16 * ((n - 1) // 16) < j < n:  # the last piece straddles the ring's end
            (hbm_last if is_match else lit_last).add(n)
    # (a 1-byte last piece cannot straddle: lengths 1, 17, 33 and 49 lie at
    # the ring's end with the piece on either side of it instead)
    assert lit_last == {L for L in LIT_LENS if (L - 1) % 16}
    assert hbm_last == {m for m in HBM_LENS if (m - 1) % 16}


@pytest.mark.parametrize("variant", ["idx1", "product"])
def test_crafted_blocks(crafted, variant):
    frame, raws = crafted
    ref = oracle_blocks(frame, len(raws))
    assert ref == raws  # the builder's own bytes are the reference's
    v = {"idx1": lz4ada.DECODE_IDX1_ALONE, "product": lz4ada.DECODE_IDX}[variant]
    descs, st, out = _run_variant_alone(frame, v)
    for i, r in enumerate(raws):
        assert st[i].code == 0, (i, st[i].code)  # k_decode_idx itself took every block
        o = descs[i].out_off
        assert st[i].out_len == len(r), i
        got = out[o:o + len(r)]
        if got != r:
            x = next(k for k in range(len(r)) if got[k] != r[k])
            pytest.fail(f"block {i}: first difference at output byte {x} (ring position {x % RING})")


def d1_linked_frame():
    """A full 64 KiB block (the round ends at 65,536), then a 64 KiB-class
    block of D1-range matches (offset 65,533: the reference reads what its
    last wild copy left, not history) of 17, 32 and 33 bytes: after 20
    literals, right after a short match, and -- after six far matches of
    300 bytes in the same batch, 108 dealt pieces -- after 20 literals
    again, so that the D1 match's own dealt pieces are beyond the 64th."""
    comp0, raw0 = lz4ada.gen_block(1, 1234, 65536)
    comp = bytearray()

    def seq(lits, off, ml):
        L, m = len(lits), ml - 4
        comp.extend(bytes([(min(L, 15) << 4) | min(m, 15)]) + (_ext(L - 15) if L >= 15 else b"") + lits +
                    struct.pack("<H", off) + (_ext(m - 15) if m >= 15 else b""))
        return L + ml

    pos = 0
    for ml in (17, 32, 33):
        pos += seq(bytes(range(65, 85)), 65533, ml)         # after literals
        pos += seq(bytes(range(97, 113)), 16, 4)            # 16 literals, a match inside the round
        pos += seq(b"", 65533, ml)                          # ... and D1 with no literals
        pos += seq(bytes(range(48, 60)), 30000, 8)
    for i in range(6):
        pos += seq(b"", 60000 + 11 * i, 300)
    pos += seq(bytes(range(65, 85)), 65533, 33)
    tail = b"vwxyz0123"
    comp += bytes([len(tail) << 4]) + tail
    assert pos + 33 < 65533  # every D1 read stays before the round
    blocks = [(comp0, raw0), (bytes(comp), b"\0" * (pos + len(tail)))]
    frame, _ = lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, indep=False)
    return frame, blocks


def plain_decode(hist, payload):
    """The block over contiguous history (the format's meaning, no quirk)."""
    out, i, n = bytearray(hist), 0, len(payload)
    while i < n:
        t = payload[i]
        i += 1
        L = t >> 4
        if L == 15:
            while True:
                L, i = L + payload[i], i + 1
                if payload[i - 1] != 255:
                    break
        out += payload[i:i + L]
        i += L
        if i >= n:
            break
        off, i, ml = payload[i] | (payload[i + 1] << 8), i + 2, (t & 15) + 4
        if ml == 19:
            while True:
                ml, i = ml + payload[i], i + 1
                if payload[i - 1] != 255:
                    break
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out[len(hist):])


def test_d1_whole_pieces_linked():
    frame, blocks = d1_linked_frame()
    st, ref, msg = oracle(frame)
    assert st == O.OK, msg
    assert len(ref) == 65536 + len(blocks[1][1])
    # the reference really diverges from contiguous history in every D1 match
    plain = plain_decode(ref[:65536], blocks[1][0])
    diff = [k for k in range(len(plain)) if plain[k] != ref[65536 + k]]
    assert len(diff) >= 7 and diff[-1] > 1800, diff
    out, _ = lz4ada.decode_frame(frame)
    assert out == ref
    assert lz4ada.last_path() == want_path(blocks, 64 * KiB)
    assert lz4ada.last_path() == lz4ada.PATH_LINKED  # emulated in the bulk pass, no exact path
