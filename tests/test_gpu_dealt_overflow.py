"""Pass 2 of the index decoders at the edge of its piece dealings.

Pass 2 deals 16-byte pieces over the wave's 64 lanes three times per batch:
literal pieces, pieces of HBM-sourced matches beyond each match's first, and
pieces of ring-sourced matches.  A dealing of more than 64 (and of more than
128) pieces takes other code than one that fits, so the blocks here are
crafted to put the two match dealings right at those edges: runs of like
sequences whose shape fixes the pieces per batch, swept from block to block.

The batch cut works on 32-byte compressed sub-segments, so a block cannot pin
a count.  A small model of the cut (`batches`) gives each batch's counts, and
`test_model_covers_the_edges` (CPU) asserts that every count in 62..67 and
126..130 occurs for both dealings.  The GPU tests then require the oracle's
bytes and length for every block from each variant, and that no variant
declines a block: what is checked is the decoders' behaviour, whatever
mechanism deals the pieces."""
import random

import pytest

import _lz4build

OW = 4080        # a batch's output bytes at most (lz4ada_idx.hip)
MAXSEQ = 128     # ... and its sequences
SUB = 32         # compressed bytes per lane of a batch
RING_LANE_MAX = 32
BMAX = 64 << 10
FILLER = 9 << 10
EDGES = list(range(62, 68)) + list(range(126, 131))


def seq_size(L, ml):
    return 1 + (L >= 15) + L + 2 + (ml - 4 >= 15)  # (no length here needs a second extension byte)


def batches(shape):
    """The cut: `shape` is the block's [(L, ml)] (a last literal-only
    sequence as ml 0) -> [(o_batch, first sequence, one past the last)], or
    None for sub-segments that go to HBM directly (no dealing)."""
    pos, starts = 0, []
    for L, ml in shape:
        starts.append(pos)
        pos += seq_size(L, ml) if ml else 1 + (L >= 15) + L
    nsub = (pos + SUB - 1) // SUB
    per = [[] for _ in range(nsub)]
    for i, p in enumerate(starts):
        per[p // SUB].append(i)
    res, k0, o = [], 0, 0
    while k0 < nsub:
        nb = ns = m = 0
        first = None
        for k in range(k0, min(k0 + 64, nsub)):
            b = sum(shape[i][0] + shape[i][1] for i in per[k])
            if nb + b > OW or ns + len(per[k]) > MAXSEQ:
                break
            nb, ns, m = nb + b, ns + len(per[k]), m + 1
            if first is None and per[k]:
                first = per[k][0]
        if m == 0:  # oversized: 64 sub-segments straight to HBM
            o += sum(shape[i][0] + shape[i][1] for k in range(k0, min(k0 + 64, nsub)) for i in per[k])
            res.append(None)
            k0 += 64
            continue
        if first is not None:
            res.append((o, first, first + ns))
        o += nb
        k0 += m
    return res


def match_pieces(off, ml):
    if off < 16 and off < ml:
        stp = off * (16 // off) if off <= 8 else off
        return (ml + stp - 1) // stp
    return (ml + 15) // 16


def dealt(seqs, bt):
    """(HBM-sourced pieces beyond each match's first, ring-sourced pieces or
    None where every ring match keeps a lane of its own) of one batch."""
    o_batch, a, b = bt
    glo = o_batch - OW - 16
    pos = o_batch
    hbm = ring = 0
    longest = 0
    for L, off, ml in seqs[a:b]:
        mdst = pos + L
        pos = mdst + ml
        if ml == 0:
            continue
        if mdst - off < glo:
            hbm += max((ml + 15) // 16 - 1, 0)
        else:
            ring += match_pieces(off, ml)
            longest = max(longest, ml)
    return hbm, (ring if longest > RING_LANE_MAX else None)


def build_block(rng, types, fracs, every=None):
    """One block: FILLER bytes of plain short sequences, then sequences of
    types[0], with every 1/fracs[j]-th one of types[j + 1] instead (and each
    every[0]-th one of type every[1]), to BMAX.  A type is (kind, Ls, mls);
    the kind places the match's source once the cut is known.
    -> (payload, decoded, [(L, off, ml)])"""
    shape, kinds = [], []
    out = 0
    while out < FILLER:
        shape.append((14, 4))
        kinds.append("fill")
        out += 18
    i = 0
    while True:
        t = types[0]
        for j, f in enumerate(fracs):
            if int((i + 1) * f) > int(i * f):
                t = types[j + 1]
        if every and i % every[0] == every[0] - 1:
            t = every[1]
        kind, Ls, mls = t
        L, ml = Ls[i % len(Ls)], mls[(i // len(Ls)) % len(mls)]
        if out + L + ml > BMAX - 16:
            break
        shape.append((L, ml))
        kinds.append(kind)
        out += L + ml
        i += 1
    shape.append((5, 0))
    kinds.append("last")
    # the cut, then each match's source relative to its batch
    o_of = {}
    for bt in batches(shape):
        if bt:
            for s in range(bt[1], bt[2]):
                o_of[s] = bt[0]
    seqs, pos, prev = [], 0, 0
    for s, ((L, ml), kind) in enumerate(zip(shape, kinds)):
        mdst = pos + L
        o_batch = o_of.get(s, mdst)
        glo = o_batch - OW - 16
        if kind == "fill":
            off = 14
        elif kind == "last":
            off = 0
        elif kind == "hbm" and glo - 64 > 0:  # anywhere in the flushed output
            off = mdst - rng.randrange(0, glo - 64)
        elif kind == "own" and L > 0:         # in its own literals
            off = rng.randint(1, L)
        elif kind == "pat":                   # period pattern
            off = rng.randint(1, min(15, ml - 1))
        elif kind == "wide":                  # overlap with off >= 16
            off = rng.randint(16, ml - 1) if ml > 16 else 16
        elif kind == "next":                  # the previous match from its first byte on
            off = mdst - prev
        else:                                 # "far": in the ring, before the batch
            off = mdst - (o_batch - rng.randint(100, 3000))
        assert ml == 0 or 0 < off <= min(mdst, 65535), (kind, off, mdst)
        seqs.append((L, off, ml))
        prev = mdst
        pos = mdst + ml
    lits = [rng.randbytes(L) for L, _, _ in seqs]
    comp, raw = _lz4build.encode([(lit, off, ml) for lit, (_, off, ml) in zip(lits[:-1], seqs[:-1])], lits[-1])
    assert len(raw) <= BMAX
    return comp, raw, seqs


L03 = [0, 1, 2, 3]


def specs():
    """(types, fracs, every) per block, in groups (see the module docstring
    for what each is for)."""
    sp = []
    short = ("hbm", L03, [12, 16, 9, 14])
    hb1 = ("hbm", L03, [17, 24, 31, 20])   # one dealt piece
    hb2 = ("hbm", L03, [33, 40, 48, 36])   # two
    far0 = ("far", L03, [16, 12, 16, 15])
    far2 = ("far", L03, [17, 17, 24, 17])
    far3 = ("far", [1], [40])
    # HBM-sourced pieces around 64: 128 sequences, about half with a dealt piece
    for i in range(18):
        sp.append(([short, hb1], [0.42 + 0.01 * i], None))
    # ... around 128: nearly all with one, then a few with two
    for i in range(8):
        sp.append(([short, ("hbm", L03, [17, 18, 19, 20])], [0.93 + 0.01 * i], None))
    for i in range(8):
        sp.append(([("hbm", [0, 1], [17, 18, 19, 20]), ("hbm", [0], [33, 34])], [0.01 * i], None))
    # ring-sourced pieces around 64 (HBM-sourced short matches between: both
    # kinds in one round), one 40-byte match per 32 to deal them at all
    for i in range(18):
        sp.append(([short, far0], [0.38 + 0.01 * i], (32, far3)))
    for i in range(6):
        sp.append(([short, far2], [0.20 + 0.01 * i], (32, far3)))
    # ... around 128: lengths 16 and 17, and the overlap forms among them
    for i in range(14):
        sp.append(([far0, short, far2], [0.01 * i, 0.03], (32, far3)))
    for i in range(6):
        sp.append(([far0, far2, ("pat", L03, [17, 20]), ("wide", L03, [17, 24, 33])],
                   [0.01 * i, 0.02, 0.02], (32, far3)))
    # in their own literals
    for i in range(4):
        sp.append(([("own", [1, 2, 3, 7, 12], [16, 17, 24, 40]), far2], [0.1 * i], None))
    # a near match reading a far match's first 16 bytes and its remainder
    for i in range(4):
        sp.append(([("far", [0, 2], [17, 24, 33, 40]), ("next", [0, 1, 3], [17, 24, 33, 16])], [0.5],
                   (7 + i, hb1)))
    # HBM-sourced and far ring matches in one round, both dealings over 64
    for i in range(8):
        sp.append(([hb1, far2, hb2], [0.35 + 0.03 * i, 0.05], (32, far3)))
    # more pieces beyond 64 than lanes with an idle slot: nearly every
    # match HBM-sourced and over 32 bytes
    for i in range(4):
        sp.append(([hb2, far0], [0.02 * i], None))
    return sp


_built = {}


def blocks():
    if not _built:
        rng = random.Random(0xDEA17)
        _built["b"] = [build_block(rng, *s) for s in specs()]
    return _built["b"]


def test_model_covers_the_edges():
    seen_h, seen_r = set(), set()
    for comp, raw, seqs in blocks():
        for bt in batches([(L, ml) for L, _, ml in seqs]):
            if bt:
                h, r = dealt(seqs, bt)
                seen_h.add(h)
                seen_r.add(r)
    assert not [c for c in EDGES if c not in seen_h], sorted(seen_h)
    assert not [c for c in EDGES if c not in seen_r], sorted(x for x in seen_r if x is not None)
    assert max(seen_h) > 150  # the batch with more overflow than idle slots


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
        frame, _ = lz4frame.build_frame([(c, r, False) for c, r, _ in part], BMAX, indep=True,
                                        block_cksum=bool((k // FRAME_BLOCKS) & 1))
        ref = oracle_blocks(frame, len(part))
        assert ref == [r for _, r, _ in part]  # the builder's own bytes are the reference's
        res.append((frame, ref))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["idx1", "pp2", "product"])
def test_dealt_overflow(frames, variant):
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
