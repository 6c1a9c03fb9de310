"""Test helper: the blocks of the exact-cap tests ("Why exact
caps are safe").  Every block is (payload, expected bytes, stored), independent
and decodable alone.  Decoded sizes are base + residue, the residues mod 256
around the 16-byte piece, the 32-byte ring piece and the slot rounding, the
bases the smallest at which a mechanism exists (one batch, the 4,080-byte
batch boundary, a 64 KiB block's last bytes, a 256 KiB block).  Built from the
generator, rand_block, Payload / encode; checked on the CPU by
test_exact_caps_fixtures_cpu.py.  Pure Python, test infrastructure only."""
import random
import struct

import lz4ada
from _lz4build import encode
from test_gpu_frames_sizes import Payload
from test_gpu_random_blocks import rand_block

RESIDUES = (0, 1, 15, 16, 17, 240, 241, 255)
SPARSE_RESIDUES = (0, 1, 16, 255)
BASES = (0, 3840, 65280)        # under 256; across the 4,080-byte batch; up to 65,535
BIG_BASE = 261888               # the generator kinds only, under a 4 MiB maximum
BMAX = 4 << 20
GEN = ("dense", "mixed", "rle", "literal", "chain")
ENDINGS = ("match_end", "match300_off1", "lit16_end", "lit1_end")


class Block:
    """One fixture block: cls (its class), name, payload, want (the expected
    bytes), stored."""

    def __init__(self, cls, name, payload, want, stored=False):
        self.cls, self.name, self.payload, self.want, self.stored = cls, name, payload, want, stored

    @property
    def size(self):
        return len(self.want)

    def __repr__(self):
        return f"<{self.cls}:{self.name} {len(self.payload)}->{self.size}>"


def round256(v):
    return (v + 255) & ~255


def magnitude(size):
    """The base a size belongs to (the empty block: None)."""
    if size == 0:
        return None
    for base in (BIG_BASE,) + BASES[::-1]:
        if base <= size < base + 256:
            return base
    return -1  # a sparse block: its size follows from its payload


def parse(payload):
    """The sequences of a well-formed block -> (list of dicts tok, L, lit,
    off_at, off, ml, out: the payload positions of the token, the literals and
    the offset field, and the output position where the match starts; the
    final literals' (payload position of their token, length) or None where
    the block ends after a match)."""
    seqs, p, o, n = [], 0, 0, len(payload)
    while p < n:
        tok = p
        t = payload[p]
        p += 1
        L = t >> 4
        if L == 15:
            while True:
                e = payload[p]
                p += 1
                L += e
                if e != 255:
                    break
        lit = p
        p += L
        o += L
        if p >= n:
            assert p == n and (t & 15) == 0
            return seqs, (tok, L)
        off_at = p
        off = payload[p] | payload[p + 1] << 8
        p += 2
        ml = (t & 15) + 4
        if ml == 19:
            while True:
                e = payload[p]
                p += 1
                ml += e
                if e != 255:
                    break
        seqs.append(dict(tok=tok, L=L, lit=lit, off_at=off_at, off=off, ml=ml, out=o))
        o += ml
    return seqs, None


def _prefix(rng, upto):
    """Sequences for encode() in rand_block's shapes that decode to at most
    `upto` bytes -> (seqs, decoded length)."""
    if upto < 5:
        return [], 0
    payload, _ = rand_block(rng, upto)
    seqs, at = [], 0
    for s in parse(payload)[0]:
        if s["out"] + s["ml"] > upto:
            break
        seqs.append((payload[s["lit"]:s["lit"] + s["L"]], s["off"], s["ml"]))
        at = s["out"] + s["ml"]
    return seqs, at


def rand_sized(seed, size):
    """A rand_block cut after its last sequence that ends below `size`, its
    final literals as long as it takes to decode to exactly `size` bytes."""
    rng = random.Random(seed)
    seqs, at = _prefix(rng, size - 1)
    return encode(seqs, rng.randbytes(size - at))


def crafted_ending(kind, seed, size):
    """A block of `size` bytes with the ending `kind`, or None where the size
    is too small to hold it."""
    rng = random.Random(seed)
    if kind == "match_end":  # the block ends after a match: no last literals
        if size < 5:
            return None
        seqs, at = _prefix(rng, size - 12)
        ml = min(size - at - 1, 9)
        return encode(seqs + [(rng.randbytes(size - at - ml), 3 if size - ml >= 3 else 1, ml)])
    if kind == "match300_off1":  # a last match of 300 bytes and more, offset 1, up to the size; no literals behind it
        if size < 302:
            return None
        ml = 300 + seed % 41
        seqs, at = _prefix(rng, size - ml - 1)
        return encode(seqs + [(rng.randbytes(size - ml - at), 1, ml)], b"")
    if kind == "lit16_end":  # the last literals: 16 to 31 bytes that end at the size
        if size < 16:
            return None
        fl = 16 + seed % 16
        if size < fl + 5:
            return encode([], rng.randbytes(size))
        seqs, at = _prefix(rng, size - fl - 5)
        return encode(seqs + [(rng.randbytes(1), 1, size - fl - at - 1)], rng.randbytes(fl))
    assert kind == "lit1_end"  # one last literal
    if size < 6:
        return encode([], rng.randbytes(size)) if size == 1 else None
    seqs, at = _prefix(rng, size - 6)
    return encode(seqs + [(rng.randbytes(1), 1, size - at - 2)], rng.randbytes(1))


def sparse_ratio(seed, residue):
    """DS_SPARSE by ratio, as rle_block builds it: 4,096 payload bytes and more
    that decode to over 64 times as many.  Residues 0 and 1 by the last match
    length (the block ends after it), the others by the final literals."""
    p = Payload(seed)
    for _ in range(18):  # 18: over 64 times the payload with 275 final literals too
        p.add(b"", 4 + 15 + 255 * 64 + 7)
    while p.n < 4096:
        p.add(p.rng.randbytes(14), 4)
    size = sum(len(l) + ml for l, _, ml in p.seqs)
    if residue in (0, 1):
        ml = 300 + (residue - size - 300) % 256
        comp, raw = encode(p.seqs + [(b"", 1, ml)])
    else:
        fl = 20 + (residue - size - 20) % 256
        comp, raw = encode(p.seqs, p.rng.randbytes(fl))
    assert len(raw) % 256 == residue
    return comp, raw


def sparse_density(seed, residue):
    """DS_SPARSE by density, as literal_block builds it: 65,536 payload bytes and
    more in a handful of sequences.  The residue by the final literals."""
    p = Payload(seed)
    for _ in range(4):
        p.add(p.rng.randbytes(15 + 255 * 64 + 11), 4)
    size = sum(len(l) + ml for l, _, ml in p.seqs)
    fl = 300 + (residue - size - 300) % 256
    comp, raw = encode(p.seqs, p.rng.randbytes(fl))
    assert len(raw) % 256 == residue
    return comp, raw


def cap_blocks():
    """The whole set, in a fixed order.  Classes: the generator kinds,
    "rand", "stored", the four ENDINGS, "sparse_ratio", "sparse_density",
    "empty".  The crafted endings take every residue under 256 and from 3,840
    where the ending fits; from 65,280 each ending takes two of the residues in
    turn, all eight between them: the set stays under 16 MiB."""
    out = []
    out.append(Block("empty", "one_zero_token", b"\x00", b""))
    out.append(Block("empty", "stored_0", b"", b"", True))
    seed = 0xCA9
    for base in BASES + (BIG_BASE,):
        for r in RESIDUES:
            size = base + r
            if size == 0:
                continue
            seed += 1
            for kind in GEN:
                comp, raw = lz4ada.gen_block(lz4ada.GEN_KINDS[kind], seed, size)
                out.append(Block(kind, f"{kind}_{size}", comp, raw))
            if base == BIG_BASE:
                continue
            out.append(Block("rand", f"rand_{size}", *rand_sized(seed, size)))
            raw = random.Random(seed).randbytes(size)
            out.append(Block("stored", f"stored_{size}", raw, raw, True))
            for k, kind in enumerate(ENDINGS):
                if base == BASES[-1] and RESIDUES.index(r) % 4 != k:
                    continue
                made = crafted_ending(kind, seed, size)
                if made is not None:
                    out.append(Block(kind, f"{kind}_{size}", *made))
    for r in SPARSE_RESIDUES:
        out.append(Block("sparse_ratio", f"sparse_ratio_r{r}", *sparse_ratio(40 + r, r)))
        out.append(Block("sparse_density", f"sparse_density_r{r}", *sparse_density(50 + r, r)))
    return out


# ------------------------------------------------------------ rewritten offsets

REWRITES = ("zero", "before_block", "max", "other")


class Rewritten:
    """A rand_block with 1 to 3 offset fields rewritten, the chain kept:
    payload, original (the unchanged payload), fields ((payload position of
    the offset field, the rewrite's kind, the new offset), ...)."""

    def __init__(self, name, payload, original, fields):
        self.name, self.payload, self.original, self.fields = name, payload, original, fields


def rewritten_blocks(count=40):
    """Seeded blocks of under 65,000 decoded bytes (no valid offset comes near
    65,529: quirk D1 stays out).  Even blocks get other valid offsets only,
    odd ones at least one offset the reference rejects (0, one byte before the
    block, 65,535)."""
    out = []
    for i in range(count):
        rng = random.Random(0x0FF5 + i)
        payload, raw = rand_block(rng, rng.choice([40, 700, 4095, 9000, 20000, 40000]))
        assert len(raw) < 65000
        seqs, _ = parse(payload)
        picks = rng.sample(seqs, min(len(seqs), 1 + i % 3))
        b = bytearray(payload)
        fields = []
        for k, s in enumerate(picks):
            kind = "other" if i % 2 == 0 else (REWRITES[(i // 2 + k) % 3] if k == 0 else rng.choice(REWRITES))
            if kind == "other":
                new = rng.choice([x for x in (1, 2, 15, 16, 17, s["out"], rng.randint(1, s["out"]))
                                  if x <= s["out"] and x != s["off"]] or [s["off"]])
            else:
                new = dict(zero=0, before_block=s["out"] + 1, max=65535)[kind]
            b[s["off_at"]:s["off_at"] + 2] = struct.pack("<H", new)
            fields.append((s["off_at"], kind, new))
        out.append(Rewritten(f"rewritten_{i}", bytes(b), payload, tuple(fields)))
    return out
