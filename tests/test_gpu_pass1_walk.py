"""Pass 1 of the index decoder (k_index; index_block<W> in
csrc/lz4ada_idx.hip, by one wave or two) on the shapes where a lane's first walk of a chunk can
go wrong: a sequence start at every bit of a record and at every boundary
(32-byte sub-segment, 256-byte segment, 16 KiB chunk), fields straddling a
boundary, the densest sub-segments next to the largest sequences the
branch-free parse accepts, output counts that saturate the records' 16-bit
field, rare shapes beside ordinary lanes, segments and chunks without a
start, literal bytes that read as tokens (so lead-in guesses miss and the
fixed-point loop re-walks), ragged sizes, payloads that end around the
half chunk where the second wave's lanes begin, and malformed data on the
converged chain.

Every well-formed block must be ACCEPTED (status 0, not DS_RETRY) by the
one-wave decoder, the two-launch split and the pipelined pair, each alone,
with the oracle's bytes: a pass 1 that silently declined would still give
right bytes through the retry decoder.  The pass-1 table itself
(lz4ada_index_table_debug), written by one wave per block and by two, must
equal a serial parse in Python.  Small
frames: blocks of at most ~100 KiB in 256 KiB slots."""
import random

import pytest

import _oracle as O
import lz4ada
import lz4frame
from _lz4build import encode
from test_gpu_parity import _run_variant_alone, oracle_blocks

pytestmark = pytest.mark.gpu

BMAX = 256 << 10  # in_len * 64 >= out_cap for every in_len >= 4096: the RLE rule never applies
SEG, CHUNK = 256, 16384


def _extlen(v):
    return 0 if v < 15 else (v - 15) // 255 + 1


class Blk:
    """Sequences for _lz4build.encode with the payload position in hand."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.seqs = []
        self.n = 0    # payload bytes so far
        self.out = 0  # decoded bytes so far

    def add(self, lits, off=None, ml=4):
        if isinstance(lits, int):
            lits = self.rng.randbytes(lits)
        self.out += len(lits)
        if off is None:
            off = self.rng.randint(1, min(self.out, 65535))
        assert 1 <= off <= self.out and ml >= 4
        self.seqs.append((lits, off, ml))
        self.n += 1 + _extlen(len(lits)) + len(lits) + 2 + _extlen(ml - 4)
        self.out += ml
        return self

    def three(self, count=1):
        """3-byte sequences: L = 0, ml = 4."""
        for _ in range(count):
            self.add(b"")
        return self

    def fill_to(self, T):
        """Ordinary short sequences (3..17 bytes, no length extension) up to
        payload position T exactly."""
        if not self.seqs:
            self.add(8, ml=self.rng.randint(4, 18))
        assert T == self.n or T >= self.n + 3, (T, self.n)
        while self.n < T:
            gap = T - self.n
            L = self.rng.choice([0, 0, 0, 0, 1, 1, 2, 3, 5, 9, 14])
            if gap - (3 + L) != 0 and gap - (3 + L) < 3:
                L = gap - 3 if gap - 3 <= 14 else 0
            self.add(L, ml=self.rng.randint(4, 18))
        assert self.n == T
        return self

    def done(self, tail=b"tail!"):
        return encode(self.seqs, tail)


def _sized(seed, n):
    """A block whose payload is exactly n bytes."""
    if n < 20:
        return encode([], b"x" * (n - 1))
    return Blk(seed).fill_to(n - 6).done(b"tail!")


HALF_SIZES = (CHUNK // 2 - 1, CHUNK // 2, CHUNK // 2 + 1, CHUNK + CHUNK // 2 + 1)


def _cases():
    c = {}
    # a 3-byte sequence's token at every bit of a record, and at the last /
    # first byte of a segment and of a chunk
    c["phase"] = [Blk(100 + T).fill_to(T).three(14).fill_to(T + 90).done()
                  for T in list(range(64, 96)) + [255, 256, 511, 512, CHUNK - 1, CHUNK]]
    # the token's e1 byte, the offset pair and the e2 byte across a segment
    # and the chunk boundary (near the chunk's end the 8-byte window test fails)
    st = []
    for B in (SEG, 2 * SEG, CHUNK, 2 * CHUNK):
        st.append(Blk(B + 1).fill_to(B - 1).add(20).fill_to(B + 120).done())          # e1 at B
        st.append(Blk(B + 2).fill_to(B - 4).add(2).fill_to(B + 120).done())           # offset pair B-1, B
        st.append(Blk(B + 3).fill_to(B - 3).add(b"", ml=30).fill_to(B + 120).done())  # e2 at B
        st.append(Blk(B + 4).fill_to(B - 5).add(15, ml=19).fill_to(B + 120).done())   # around B
    c["straddle"] = st
    # eleven 3-byte sequences in one sub-segment (starts 0, 3 .. 30), the
    # last of them or their neighbour the largest the branch-free parse
    # takes (L = 269, ml = 273): in an even and in an odd record
    dn = []
    for base in (320, 352, CHUNK - 64, CHUNK + 32):
        b = Blk(base).fill_to(base).three(10).add(269, ml=273)
        b.fill_to((b.n + 34) // 32 * 32).three(11).add(269, ml=273).add(269, ml=273)
        dn.append(b.fill_to(b.n + 100).done())
        b = Blk(base + 7).fill_to(base).add(269, ml=273).add(b"", ml=273).add(b"", ml=273)
        dn.append(b.fill_to(b.n + 100).done())
    c["dense"] = dn
    # counts at and over the 16-bit field: one sequence, and a sum over a
    # sub-segment's sequences that are each below it (payloads < 4 KiB)
    sat = [Blk(1).fill_to(300).add(300, off=7, ml=66000).fill_to(1100).done(),
           Blk(2).fill_to(300).add(2, off=1, ml=70000).three(5).done(),
           Blk(3).fill_to(5000).add(40, ml=65535 + 300).fill_to(6000).done()]
    for total in (65533, 65534, 65535, 65536, 65911):
        b = Blk(total).fill_to(512)
        for _ in range(7):
            b.add(b"", ml=273)
        sat.append(b.add(b"", ml=total - 7 * 273).fill_to(b.n + 200).done())
    c["saturate"] = sat
    # one-byte length extensions of 255 (L = 270.., ml = 274..), apart and in
    # one token, between ordinary sequences
    sl = []
    for seed, (L, ml) in enumerate([(270, 8), (3, 274), (270, 274), (525, 529), (780, 300), (14, 1000)]):
        b = Blk(500 + seed).fill_to(700 + 37 * seed)
        for _ in range(6):
            b.add(L, ml=ml).fill_to(b.n + 150 + seed)
        sl.append(b.fill_to(CHUNK + 500).done())
    c["slow"] = sl
    # literal runs that leave a segment, four segments and a whole chunk
    # without a sequence start
    c["empty"] = [Blk(700 + i).fill_to(900 + 13 * i).add(run).fill_to(900 + 13 * i + run + 2000).done()
                  for i, run in enumerate((300, 1100, 17 << 10))]
    # literal bytes that read as tokens with long lengths: lead-in guesses
    # land inside them and miss, so segments are re-walked; then ordinary data
    rw = []
    for seed, alpha in enumerate([bytes(range(0xF0, 0x100)), b"\x0f", bytes(range(0xF0, 0x100)) + b"\x0f\x0f\x0f\x0f",
                                  b"\xff\xf0\x1f\x0f\x00"]):
        b = Blk(900 + seed).fill_to(2000 + 5 * seed)
        for run in (3000, 700, 5000):
            b.add(bytes(b.rng.choice(alpha) for _ in range(run))).fill_to(b.n + 1500)
        rw.append(b.fill_to(2 * CHUNK + 3000).done())
    c["rewalk"] = rw
    c["sizes"] = [_sized(1000 + n, n) for n in (6, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 32773)]
    # two waves per block (128 lanes of 128 bytes; the second wave's begin at
    # CHUNK / 2): payloads in which it has no lane, exactly one lane, and one
    # lane in the second chunk; and a token-like literal run (the rewalk
    # recipe) over CHUNK / 2 - 400 .. CHUNK / 2 + 400, so the lead-in guess of
    # the second wave's lane 0 misses and it converges a second time
    hf = [_sized(2000 + n, n) for n in HALF_SIZES]
    b = Blk(990).fill_to(CHUNK // 2 - 410)
    lit0 = b.n + 1 + _extlen(830)  # the run's first literal byte
    assert lit0 <= CHUNK // 2 - 400 and lit0 + 830 > CHUNK // 2 + 400
    b.add(bytes(b.rng.choice(bytes(range(0xF0, 0x100))) for _ in range(830))).fill_to(b.n + 1500)
    hf.append(b.fill_to(CHUNK + 3000).done())
    c["half"] = hf
    return c


CASES = _cases()
VARIANTS = {"idx1": lz4ada.DECODE_IDX1_ALONE, "split": lz4ada.DECODE_IDX_SPLIT,
            "pp2": lz4ada.DECODE_PP2_ALONE, "product": lz4ada.DECODE_IDX}


@pytest.fixture(scope="module")
def frames():
    """name -> (frame, payloads, the oracle's blocks); built once."""
    res = {}
    for name, blocks in CASES.items():
        assert all(len(r) <= BMAX and len(c) < 4 * CHUNK for c, r in blocks), name
        frame, _ = lz4frame.build_frame([(c, r, False) for c, r in blocks], BMAX, indep=True)
        ref = oracle_blocks(frame, len(blocks))
        assert ref == [r for _, r in blocks], name  # the builder's bytes are the reference's
        res[name] = (frame, [c for c, _ in blocks], ref)
    return res


def test_sizes_are_the_issues():
    assert [len(c) for c, _ in CASES["sizes"]] == [6, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 32773]
    assert [len(c) for c, _ in CASES["half"][:4]] == [8191, 8192, 8193, 24577]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(CASES))
def test_accepted_and_exact(frames, name, variant):
    frame, _, ref = frames[name]
    descs, st, out = _run_variant_alone(frame, VARIANTS[variant])
    for i, r in enumerate(ref):
        assert st[i].code == 0, (name, i, st[i].code)
        assert st[i].out_len == len(r), (name, i)
        o = descs[i].out_off
        assert out[o:o + len(r)] == r, (name, i)


def model_records(c):
    """Serial parse: per 32-byte sub-segment, start bitmap | output bytes of
    the sequences starting there << 32 (a count >= 0xFFFF saturates the low
    16 bits and the high word holds it whole: the same number)."""
    n = len(c)
    bm = [0] * ((n + 31) // 32)
    cnt = [0] * len(bm)
    p = 0
    while p < n:
        s = p
        tk = c[p]
        p += 1
        L = tk >> 4
        if L == 15:
            while True:
                e = c[p]
                p += 1
                L += e
                if e != 255:
                    break
        p += L
        ml = 0
        if p < n:
            p += 2
            m = tk & 15
            if m == 15:
                while True:
                    e = c[p]
                    p += 1
                    m += e
                    if e != 255:
                        break
            ml = m + 4
        bm[s >> 5] |= 1 << (s & 31)
        cnt[s >> 5] += L + ml
    assert p == n
    return [b | (k << 32) for b, k in zip(bm, cnt)]


# (waves = 1 keeps the case's name as its id)
@pytest.mark.parametrize("name,waves", [(n, w) for w in (1, 2) for n in CASES],
                         ids=[n if w == 1 else n + "-waves2" for w in (1, 2) for n in CASES])
def test_table_equals_serial_parse(frames, name, waves):
    import torch
    frame, payloads, _ = frames[name]
    info, descs = lz4ada.frame_index(frame)
    nb = info.nblocks
    dev = torch.device("cuda:0")
    d_frame = torch.frombuffer(bytearray(frame), dtype=torch.uint8).to(dev)
    d_desc = torch.frombuffer(bytearray(bytes(descs)[:nb * 32]), dtype=torch.uint8).to(dev)
    d_st = torch.zeros(nb * 32, dtype=torch.uint8, device=dev)
    tab = lz4ada.index_table_debug(d_frame.data_ptr(), len(frame), d_desc.data_ptr(), nb,
                                   d_st.data_ptr(), torch.cuda.current_stream().cuda_stream, waves=waves)
    st = (lz4ada.BlockStatus * nb).from_buffer_copy(d_st.cpu().numpy().tobytes())
    for i, c in enumerate(payloads):
        assert st[i].code == 0, (name, waves, i, st[i].code)
        assert frame[descs[i].in_off:descs[i].in_off + descs[i].in_len] == c
        want = model_records(c)
        base = 64 * ((descs[i].in_off >> 8) + i)
        got = [int.from_bytes(tab[base + 8 * k:base + 8 * k + 8], "little") for k in range(len(want))]
        bad = [(k, hex(got[k]), hex(want[k])) for k in range(len(want)) if got[k] != want[k]]
        assert not bad, (name, waves, i, len(c), bad[:4])


# ---- malformed data on the converged chain

PLACES = {"first": 3 * SEG, "last": 3 * SEG + 253, "lane63": 63 * SEG + 100}
KINDS = ["off0", "short", "past", "ext255"]


def _malformed(kind, T):
    pre, _ = encode(Blk(T).fill_to(T).seqs)
    assert len(pre) == T
    if kind == "off0":  # a zero offset, ordinary sequences after it
        return pre + b"\x00\x00\x00" + b"\x00\x01\x00" * 20 + b"\x50tail!"
    if kind == "short":  # the block ends inside the offset pair
        return pre + b"\x10A\x01"
    if kind == "past":  # a literal run ending one byte past the block
        return pre + b"\x50tail"
    return pre + b"\xf0" + b"\xff" * 20  # a length extension still running at the block's end


@pytest.fixture(scope="module")
def good_block():
    return Blk(4242).fill_to(3000).done()


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("kind", KINDS)
def test_malformed_is_declined(good_block, kind, place):
    bad = _malformed(kind, PLACES[place])
    frame, _ = lz4frame.build_frame([good_block + (False,), (bad, b"", False)], BMAX, indep=True)
    for variant in ("idx1", "split", "pp2"):
        descs, st, out = _run_variant_alone(frame, VARIANTS[variant])
        assert st[0].code == 0 and out[:st[0].out_len] == good_block[1], (variant, st[0].code)
        assert st[1].code == lz4ada.DS_RETRY, (variant, st[1].code)
    descs, st, out = _run_variant_alone(frame, VARIANTS["product"])
    assert st[0].code == 0 and out[:st[0].out_len] == good_block[1]
    assert st[1].code not in (0, lz4ada.DS_RETRY, lz4ada.DS_SPARSE), st[1].code
    # the product: the oracle's status and bytes
    ost, ref, msg = O.unlz4ada(frame, out_cap=4 << 20)
    got, _, exc = lz4ada.decode_frame_partial(frame)
    assert ost != O.OK and exc is not None
    assert str(exc) == O.exception_information(ost, msg)
    assert got == ref
