"""Pass 2's dealing of ring-sourced matches, two 16-byte units per piece.

`ring_pieces` (lz4ada_idx.hip) cuts every ring-sourced match of a batch into
pieces of two units -- 32 output bytes, or two steps of a period pattern -- and
deals them over the wave's lanes; a piece stores one whole 16-byte unit and one
exact-length unit, and waits for the lower pieces of its 64-piece chunk that
write into either unit's source.  The blocks here are crafted around that rule:
second units of every tail length, overlaps whose second read wraps the period,
patterns of every period, sources that straddle producers' pieces and units,
piece counts at the edges of one and two chunks, pieces across the output
ring's end, the block's end and a batch's unaligned start.

A model of the batch cut (test_gpu_dealt_overflow's) and of the piece rule
(`cut_pieces`, `run_batch`) decodes every dealt batch on the CPU the way the
kernel does -- step by step, each ready piece reading what the steps before it
left -- and `test_model_*` assert that each intended case occurs in a dealt
batch.  The GPU tests require the oracle's bytes and length for every block
from each variant and from the linked planes, and that no variant declines a
block."""
import random

import pytest

import _lz4build
from test_gpu_dealt_overflow import BMAX, OW, RING_LANE_MAX, batches, build_block, match_pieces

ORING = 8192
EDGES = list(range(62, 68)) + list(range(126, 131))
PLAIN_ML = [17, 31, 32, 33, 47, 48, 49, 64, 65]
WIDE_OFF = [16, 17, 23, 24, 31, 32, 33, 47]


def pattern_step(off):
    return off * (16 // off) if off <= 8 else off


def wide_ml(off):
    return [off + 1, 2 * off - 1, 2 * off + 1, 4 * off + 3]


def pattern_ml(off):
    stp = pattern_step(off)
    # (a match is at least 4 bytes: off + 1 is none for off 1 and 2; a pattern is longer than off)
    return sorted(m for m in {off + 1, 16, 17, stp + 15, stp + 16, stp + 17, 2 * stp + 1, 4 * stp + 3}
                  if m >= max(4, off + 1))


# ---- the piece rule -------------------------------------------------------

def pieces32(off, ml):
    return (match_pieces(off, ml) + 1) // 2 if ml else 0


def cut_pieces(mdst, off, ml):
    """A match's pieces: [(pd, [(dst, n, src, wraps)] per unit, (s_lo, s_hi))];
    a unit copies n bytes to dst from the period-`off` sequence at src (for an
    overlap: source byte i of the period [mdst - off, mdst), wrapping)."""
    pat = off < 16 and off < ml
    stp = pattern_step(off) if pat else 16
    wide = not pat and ml > off
    res = []
    for k in range(pieces32(off, ml)):
        base = 2 * k * stp
        left = ml - base
        assert left > 0
        two = left > 16
        units = [(mdst + base, 16 if two else left)]
        if two:
            units.append((mdst + base + stp, min(16, left - stp)))
        end = units[-1][0] + units[-1][1]
        if pat or wide:
            src = (mdst - off, mdst)
        else:
            src = (mdst - off + base, mdst - off + end - mdst)
        res.append((mdst + base, end, units, src))
    # the pieces cover the match exactly, in order
    assert res[0][0] == mdst and res[-1][1] == mdst + ml
    assert all(a[1] >= b[0] and a[0] < b[0] for a, b in zip(res, res[1:]))
    return res


def batch_ring(seqs, bt):
    """[(sequence, mdst, off, ml)] of a batch's ring-sourced matches, and
    whether ring_pieces deals them (one is longer than RING_LANE_MAX)."""
    o_batch, a, b = bt
    glo = o_batch - OW - 16
    pos = o_batch
    ring = []
    for s in range(a, b):
        L, off, ml = seqs[s]
        mdst = pos + L
        pos = mdst + ml
        if ml and mdst - off >= glo:
            ring.append((s, mdst, off, ml))
    return ring, any(m[3] > RING_LANE_MAX for m in ring)


def run_batch(buf, ring, note=None):
    """The dealing of one batch on `buf` (everything but the ring matches'
    output already in place): chunks of 64 pieces, each piece waiting for the
    lower pieces of its chunk whose output meets its source; every step's
    ready pieces read what the steps before left.  -> (pieces, store steps);
    note(sequence, piece index, piece, producers) sees every piece."""
    pcs = []
    for s, mdst, off, ml in ring:
        for k, p in enumerate(cut_pieces(mdst, off, ml)):
            pcs.append((s, k, off, mdst, p))
    steps = 0
    for c0 in range(0, len(pcs), 64):
        chunk = pcs[c0:c0 + 64]
        deps = []
        for i, (s, k, off, mdst, (pd, pe, units, (s_lo, s_hi))) in enumerate(chunk):
            d = [j for j in range(i) if chunk[j][4][0] < s_hi and chunk[j][4][1] > s_lo]
            deps.append(set(d))
            if note:
                note(s, k, chunk[i][4], [(chunk[j][0], chunk[j][1], chunk[j][4]) for j in d])
        done = set()
        while len(done) < len(chunk):
            ready = [i for i in range(len(chunk)) if i not in done and deps[i] <= done]
            assert ready
            lo = min(chunk[i][4][3][0] for i in ready)
            snap = bytes(buf[lo:chunk[-1][4][1]])
            for i in ready:
                s, k, off, mdst, (pd, pe, units, src) = chunk[i]
                for dst, n in units:
                    for x in range(n):
                        y = mdst - off + (dst + x - mdst) % off
                        buf[dst + x] = snap[y - lo]
            done.update(ready)
            steps += 1
    return len(pcs), steps


def model_block(raw, seqs, note=None):
    """The block decoded by the model: each dealt batch through run_batch, the
    rest taken as decoded.  -> [(pieces, steps, o_batch, ring)] per dealt batch."""
    buf = bytearray(raw)
    res = []
    for bt in batches([(L, ml) for L, _, ml in seqs]):
        if not bt:
            continue
        ring, dealt = batch_ring(seqs, bt)
        if not dealt:
            continue
        for s, mdst, off, ml in ring:
            buf[mdst:mdst + ml] = bytes(ml)  # not yet written
        n, st = run_batch(buf, ring, note)
        res.append((n, st, bt[0], ring))
    assert bytes(buf) == raw
    return res


# ---- blocks ---------------------------------------------------------------

class Builder:
    """Sequences appended one by one; offsets are given, or placed by kind."""

    def __init__(self, rng, filler=9 << 10):
        self.rng, self.seqs, self.pos, self.tags = rng, [], 0, {}
        while self.pos < filler:
            self.add(14, 14, 4)

    def add(self, L, off, ml, tag=None):
        assert 0 < off <= min(self.pos + L, 65535), (L, off, ml, self.pos)
        if tag is not None:
            self.tags[len(self.seqs)] = tag
        self.seqs.append((L, off, ml))
        self.pos += L + ml
        return len(self.seqs) - 1

    def far(self, L, ml, tag=None):
        """a source in the ring, well before the match's batch"""
        return self.add(L, self.rng.randint(ml + 600, 3000), ml, tag)

    def dealer(self):
        """a match over RING_LANE_MAX bytes, so that its batch is dealt"""
        self.far(self.rng.randint(0, 3), 40)

    def to(self, mdst, L_min=0):
        """plain short sequences until the next match can begin at mdst with
        L_min..L_min + 17 literal bytes; -> that L"""
        while mdst - self.pos > L_min + 17:
            self.add(14, 14, 4)
        assert mdst - self.pos >= L_min, (mdst, self.pos)
        return mdst - self.pos

    def finish(self, final=5):
        lits = [self.rng.randbytes(L) for L, _, _ in self.seqs]
        last = None if final is None else self.rng.randbytes(final)
        comp, raw = _lz4build.encode([(l, off, ml) for l, (_, off, ml) in zip(lits, self.seqs)], last)
        assert len(raw) <= BMAX
        seqs = list(self.seqs) + ([(final, 0, 0)] if final is not None else [])
        return comp, raw, seqs, self.tags


def form_blocks(rng):
    """Plain, wide and pattern matches of the listed lengths: right behind
    their source (near: it is this batch's output), and from far back."""
    res = []
    cases = [("plain", ml, None if d is None else ml + d) for ml in PLAIN_ML for d in (0, 7, None)]
    cases += [("wide", ml, off) for off in WIDE_OFF for ml in wide_ml(off)]
    cases += [("pat", ml, off) for off in range(1, 16) for ml in pattern_ml(off)]
    for rep in range(2):
        order = cases[:]
        rng.shuffle(order)
        for part in range(0, len(order), 90):
            b = Builder(rng)
            for i, (kind, ml, off) in enumerate(order[part:part + 90]):
                if i % 5 == 0:
                    b.dealer()
                L = rng.choice([0, 1, 2, 3, 5, 16, 21])
                if off is None:
                    b.far(L, ml, (kind, ml, "far"))
                else:
                    b.add(L, off, ml, (kind, ml, off))
            res.append(b.finish())
    return res


def dependency_block(rng):
    b = Builder(rng)
    # a 32-byte source across two of the producer's pieces (bytes 20..51 of its 64)
    b.dealer()
    b.far(2, 64, "P2")
    b.add(0, 44, 32, "straddle")
    # ... beginning inside the second unit of the producer's first piece
    b.far(3, 64, "Pu")
    b.add(0, 43, 10, "unit2")
    b.far(3, 64)
    b.add(0, 43, 33)  # ... and on into the producer's second piece
    # the last bytes of a pattern
    b.add(5, 3, 50, "Pp")
    b.add(0, 20, 20, "tail")
    # literals and the match before them: 10 + 12 bytes, as a copy and as an overlap
    b.far(1, 40, "Pl")
    b.add(10, 22, 22, "mixed")
    b.far(1, 40)
    b.add(10, 22, 40, "mixedw")
    # a chain: each match is the one before it, over again
    b.far(2, 40, "chain0")
    for i in range(7):
        b.add(0, 40, 40, "chain")
    b.far(1, 33)
    for i in range(6):
        b.add(i & 1, 33 + (i & 1), 33, "chain")
    return b.finish()


def wrap_blocks(rng):
    """Two-unit pieces around the output ring's end (every 8 KiB of output;
    the pipelined pair's window ends every 16 KiB): the first unit ending at
    it, the second across it, the first across it, and positions around."""
    res = []
    ds = [-16, -24, -8, -32, -31, -17, -15, -1, 0, -33, -25, -9, 16, -40]
    forms = [("far", None, 40), ("far", None, 64), ("wide", 23, 50), ("pat", 3, 40), ("pat", 11, 38),
             ("near", 40, 40)]
    for f, (kind, off, ml) in enumerate(forms):
        for half in range(2):
            b = Builder(rng, filler=0)
            for k in range(1, 8):
                d = ds[(7 * half + k - 1 + f) % len(ds)]
                L = b.to(ORING * k + d, L_min=1)
                if kind == "far":
                    b.add(L, rng.randint(700, 3000), ml, ("wrap", ORING * k + d))
                else:
                    b.add(L, off, ml, ("wrap", ORING * k + d))
            res.append(b.finish())
    return res


def end_blocks(rng):
    """The last match ends 12 bytes before the block's capacity: followed by
    the 12 literal bytes that fill it, and as the block's last byte."""
    res = []
    for final, ml, off in ((12, 40, None), (None, 40, None), (12, 50, 23), (None, 35, 3), (12, 64, None)):
        b = Builder(rng, filler=(48 << 10))
        b.dealer()
        L = b.to(BMAX - 12 - ml, L_min=1)
        if off is None:
            b.far(L, ml, "end")
        else:
            b.add(L, off, ml, "end")
        assert b.pos == BMAX - 12
        res.append(b.finish(final))
    return res


def start_blocks(rng):
    """Runs of 41- and 37-byte matches with no or few literals: batches begin
    at every residue of 16 with a two-unit piece."""
    res = []
    for ml, Ls in ((41, [0]), (37, [0, 1, 0, 2])):
        b = Builder(rng)
        i = 0
        while b.pos < BMAX - 200:
            b.far(Ls[i % len(Ls)], ml)
            i += 1
        res.append(b.finish())
    return res


def count_blocks(rng):
    """Ring piece counts around 64 and 128 per batch (build_block's runs of
    like sequences, swept): matches of up to 32 bytes are one piece, of 33 to
    64 two."""
    L03 = [0, 1, 2, 3]
    short = ("hbm", L03, [12, 16, 9, 14])
    one = ("far", L03, [16, 12, 17, 31])
    one2 = ("far", L03, [17, 32, 24, 20])
    two = ("far", L03, [33, 40, 48, 36])
    two1 = ("far", [0, 1], [33, 34])
    sp = []
    for i in range(14):   # around 64: about half the batch's sequences ring-sourced
        sp.append(([short, one], [0.42 + 0.01 * i], (32, two)))
    for i in range(8):    # ... two-piece matches among them
        sp.append(([short, one2, two], [0.30 + 0.01 * i, 0.08], None))
    for i in range(12):   # around 128: nearly every sequence, some with two pieces
        sp.append(([one, short, two1], [0.01 * i, 0.02 + 0.004 * i], (32, two)))
    for i in range(8):
        sp.append(([one, two1], [0.005 * i], (64, two)))
    res = []
    for s in sp:
        comp, raw, seqs = build_block(rng, *s)
        res.append((comp, raw, seqs, {}))
    return res


_built = {}


def groups():
    if not _built:
        rng = random.Random(0x32B17E5)
        _built.update(forms=form_blocks(rng), deps=[dependency_block(rng)], wrap=wrap_blocks(rng),
                      ends=end_blocks(rng), starts=start_blocks(rng), counts=count_blocks(rng))
    return _built


def blocks():
    g = groups()
    return [b for name in ("forms", "deps", "wrap", "ends", "starts", "counts") for b in g[name]]


# ---- the model's checks (CPU) ---------------------------------------------

def dealt_tags(group):
    """tag -> [(piece index, piece, producers)] over the group's dealt pieces"""
    seen = {}
    for comp, raw, seqs, tags in groups()[group]:
        def note(s, k, piece, prod):
            if s in tags:
                seen.setdefault(tags[s], []).append((k, piece, prod))
        model_block(raw, seqs, note)
    return seen


def test_model_forms_are_dealt():
    seen = dealt_tags("forms")
    for ml in PLAIN_ML:
        for o in (ml, ml + 7, "far"):
            assert ("plain", ml, o) in seen, (ml, o)
    # second units of 1, 15, 16 and 17 - 16 bytes, and a third piece
    tails = {p[2][1][1] for ml in PLAIN_ML for v in [seen[("plain", ml, "far")]] for _, p, _ in v if len(p[2]) == 2}
    assert {1, 15, 16} <= tails
    assert any(k == 2 for k, _, _ in seen[("plain", 65, "far")])
    wraps2 = 0
    for off in WIDE_OFF:
        for ml in wide_ml(off):
            assert ("wide", ml, off) in seen, (off, ml)
            for k, (pd, pe, units, src), _ in seen[("wide", ml, off)]:
                if len(units) == 2:
                    r2 = (units[1][0] - src[1]) % off
                    wraps2 += r2 + units[1][1] > off
    assert wraps2 >= 8  # second units whose read wraps the period
    for off in range(1, 16):
        for ml in pattern_ml(off):
            assert ("pat", ml, off) in seen, (off, ml)


def test_model_dependencies():
    seen = dealt_tags("deps")
    (k, piece, prod), = seen["straddle"]
    assert sorted((t, pk) for t, pk, _ in prod) == [(prod[0][0], 0), (prod[0][0], 1)]
    (k, piece, prod), = seen["unit2"]
    (_, pk, (ppd, ppe, punits, _)), = prod
    assert pk == 0 and len(punits) == 2 and punits[1][0] <= piece[3][0] < ppd + 32
    (k, piece, prod), = seen["tail"]
    assert prod and all(len(p[2][3]) == 2 and p[2][3][1] - p[2][3][0] == 3 for p in prod)  # the pattern's pieces
    assert max(p[2][1] for p in prod) == piece[0]                                          # ... to its end
    for tag in ("mixed", "mixedw"):
        k, piece, prod = seen[tag][0]
        assert prod and piece[3][1] - max(p[2][1] for p in prod) == 10  # 10 literal bytes after the producers
    # the chain: a batch whose steps number at least six
    comp, raw, seqs, tags = groups()["deps"][0]
    assert max(st for n, st, _, _ in model_block(raw, seqs)) >= 6
    assert len(seen["chain"]) >= 2 * 13 - 2


def test_model_piece_counts():
    seen = set()
    for comp, raw, seqs, tags in groups()["counts"]:
        seen |= {n for n, _, _, _ in model_block(raw, seqs)}
    assert not [c for c in EDGES if c not in seen], sorted(seen)


def test_model_wrap_end_and_start():
    seen = dealt_tags("wrap")
    at = {}
    for (_, pos), v in seen.items():
        for k, (pd, pe, units, src), _ in v:
            if len(units) == 2:
                for w in (ORING, 2 * ORING):
                    u0, u1 = units
                    at.setdefault(w, set())
                    if (u0[0] + 16) % w == 0:
                        at[w].add("first ends at it")
                    if u1[0] % w and u1[0] // w != (u1[0] + u1[1] - 1) // w:
                        at[w].add("second across")
                    if u0[0] % w and u0[0] // w != (u0[0] + 15) // w:
                        at[w].add("first across")
    for w in (ORING, 2 * ORING):
        assert at[w] == {"first ends at it", "second across", "first across"}, (w, at[w])
    assert all(len(raw) >= (24 << 10) for _, raw, _, _ in groups()["wrap"])
    ends = dealt_tags("ends")["end"]
    assert {p[1] for _, p, _ in ends} >= {BMAX - 12} and len(ends) >= 2 * len(groups()["ends"]) - 1
    for comp, raw, seqs, tags in groups()["ends"]:
        assert len(raw) in (BMAX, BMAX - 12)
    res = set()
    for comp, raw, seqs, tags in groups()["starts"]:
        for n, st, o_batch, ring in model_block(raw, seqs):
            if ring[0][3] > 16:
                res.add(o_batch % 16)
    assert len(res - {0}) >= 8, res


# ---- the decoders (GPU) ---------------------------------------------------

FRAME_BLOCKS = 32


@pytest.fixture(scope="module")
def frames():
    """The blocks in frames of FRAME_BLOCKS, with the oracle's output."""
    import lz4frame
    from test_gpu_parity import oracle_blocks
    bl = blocks()
    res = []
    for k in range(0, len(bl), FRAME_BLOCKS):
        part = bl[k:k + FRAME_BLOCKS]
        frame, _ = lz4frame.build_frame([(b[0], b[1], False) for b in part], BMAX, indep=True,
                                        block_cksum=bool((k // FRAME_BLOCKS) & 1))
        ref = oracle_blocks(frame, len(part))
        assert ref == [b[1] for b in part]  # the builder's own bytes are the reference's
        res.append((frame, ref))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["idx1", "pp2", "product"])
def test_ring_pieces32(frames, variant):
    import lz4ada
    from test_gpu_parity import _run_variant_alone
    v = {"idx1": lz4ada.DECODE_IDX1_ALONE, "pp2": lz4ada.DECODE_PP2_ALONE,
         "product": lz4ada.DECODE_IDX}[variant]
    bad = []
    for f, (frame, ref) in enumerate(frames):
        descs, st, out = _run_variant_alone(frame, v)
        for i, r in enumerate(ref):
            o = descs[i].out_off
            if st[i].code != 0 or st[i].out_len != len(r) or out[o:o + len(r)] != r:
                got = out[o:o + len(r)]
                j = next((x for x in range(len(r)) if got[x] != r[x]), -1)
                bad.append((f, i, st[i].code, st[i].out_len, len(r), j))
    assert not bad, bad  # (frame, block, status code, out_len, expected, first differing byte)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["forms", "deps", "wrap", "counts"])
def test_ring_pieces32_linked(group):
    """The same blocks as a linked frame: pass 2 runs in the linked planes'
    kernels (no block here reads the one before it; the frame says it may)."""
    import _oracle as O
    import lz4ada
    import lz4frame
    part = groups()[group][:12]
    frame, raw = lz4frame.build_frame([(b[0], b[1], False) for b in part], BMAX, indep=False)
    st, ref, msg = O.unlz4ada(frame, out_cap=len(raw) + (1 << 20))
    assert st == O.OK, msg
    assert ref == raw
    out, used = lz4ada.decode_frame(frame)
    assert used == len(frame) and len(out) == len(ref)
    assert out == ref, next(x for x in range(len(ref)) if out[x] != ref[x])
