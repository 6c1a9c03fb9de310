"""Pass 2 of the index decoders where its wave-wide totals sit at their edges.

Pass 2 takes every wave-wide total and cut position from one lane of a
prefix sum: lane 63 for a total, lane m - 1 for a batch of m sub-segments,
lane 0 for a chunk's first piece.  The blocks here move m, the batch's
sequence count N and the piece totals of the three dealings (literal pieces,
pieces of HBM-sourced matches, pieces of ring-sourced matches) to their edges:

* sub-segment counts: a block of one sub-segment (m = 1), payloads of 2,033
  to 2,050 bytes (64 and 65 sub-segments, and, wherever the payload lies in
  its frame, one that ends a byte into a new 2 KiB input chunk);
* the limit that cuts the batch: 128 sequences (3-byte sequences); 4,080
  output bytes with the limit reached in lane 0 (m = 1) and in lane 63 (m =
  64, and m = 63 with a byte more); a first sub-segment that alone exceeds
  the limits (m = 0: 64 sub-segments straight to HBM), at the block's start
  and further on, ordinary batches after it;
* N = 1, 64, 65 and 128: one round, a second round of one sequence, two full;
* dealings whose round 0 holds no pieces and whose round 1 holds all, and the
  reverse, for each of the three dealings;
* a block whose last sequence sits in lane 63 of a full round (N = 64 and
  N = 128 in the block's last batch).

A batch is pinned by a separator: one sequence of exactly 32 payload bytes
(one sub-segment) and 4,080 output bytes.  It fills a batch alone, so what
follows it, up to the next separator, starts a batch at its first sequence.

`cut` is the cut model of test_gpu_dealt_overflow.py with exact sequence
sizes (the lengths here take more than one extension byte); `rounds` gives a
batch's piece totals per round as decode_block counts them.
`test_model_covers_the_cases` (CPU) asserts that each case above occurs in
the blocks built.  The GPU tests require the oracle's bytes and length for
every block from each variant, and that no variant declines a block."""
import random

import pytest

import _lz4build
from test_gpu_dealt_overflow import MAXSEQ, OW, RING_LANE_MAX, SUB, batches, match_pieces

BMAX = 64 << 10
G = (13, 4067, "pat")  # the separator: 32 payload bytes, OW output bytes


def ext(v):
    return 0 if v < 15 else 1 + (v - 15) // 255


def seq_size(L, ml):
    """Payload bytes of a sequence (ml 0: the literal-only last one)."""
    return 1 + ext(L) + L + (2 + ext(ml - 4) if ml else 0)


assert seq_size(G[0], G[1]) == SUB and G[0] + G[1] == OW


def cut(shape):
    """The batch cut of a block of [(L, ml)] -> (nsub, [batch]): a batch is
    a dict of k0, m (0: the 64 sub-segments from k0 go straight to HBM), its
    output start o and bytes, its sequences [a, b), and why it ended ("seq",
    "bytes", "lanes": 64 sub-segments, "end": of the block)."""
    pos, starts = 0, []
    for L, ml in shape:
        starts.append(pos)
        pos += seq_size(L, ml)
    nsub = (pos + SUB - 1) // SUB
    per = [[] for _ in range(nsub)]
    for i, p in enumerate(starts):
        per[p // SUB].append(i)
    res, k0, o, nxt = [], 0, 0, 0
    while k0 < nsub:
        nb = ns = m = 0
        why = "end"
        for k in range(k0, nsub):
            b = sum(shape[i][0] + shape[i][1] for i in per[k])
            if k == k0 + 64:
                why = "lanes"
            elif nb + b > OW:
                why = "bytes"
            elif ns + len(per[k]) > MAXSEQ:
                why = "seq"
            else:
                nb, ns, m = nb + b, ns + len(per[k]), m + 1
                continue
            break
        if m == 0:
            ns = sum(len(per[k]) for k in range(k0, min(k0 + 64, nsub)))
            nb = sum(shape[i][0] + shape[i][1] for i in range(nxt, nxt + ns))
        res.append({"k0": k0, "m": m, "o": o, "bytes": nb, "a": nxt, "b": nxt + ns, "why": why})
        o += nb
        nxt += ns
        k0 += m if m else 64
    return nsub, res


def rounds(seqs, bt):
    """Per round of 64 sequences of batch bt: (literal pieces beyond each
    run's first, pieces of HBM-sourced matches beyond each match's first,
    pieces of ring-sourced matches), and whether the ring pieces are dealt
    (a ring-sourced match over RING_LANE_MAX bytes in the batch)."""
    glo = bt["o"] - OW - 16
    pos = bt["o"]
    res, longest = [], 0
    for r0 in range(bt["a"], bt["b"], 64):
        lit = hbm = ring = 0
        for L, off, ml in seqs[r0:min(r0 + 64, bt["b"])]:
            mdst = pos + L
            pos = mdst + ml
            lit += (L - 1) >> 4 if L > 16 else 0
            if ml == 0:
                continue
            if mdst - off < glo:
                hbm += max((ml + 15) // 16 - 1, 0)
            else:
                ring += (match_pieces(off, ml) + 1) >> 1
                longest = max(longest, ml)
        res.append((lit, hbm, ring))
    return res, longest > RING_LANE_MAX


def build(rng, parts, final=5):
    """A block from [(L, ml, kind)]: the kind places each match's source once
    the cut is known (as test_gpu_dealt_overflow.build_block does); final:
    the last literal run (None: the block ends after a match).
    -> (payload, decoded, [(L, off, ml)])"""
    shape = [(L, ml) for L, ml, _ in parts] + ([(final, 0)] if final is not None else [])
    kinds = [k for _, _, k in parts] + (["last"] if final is not None else [])
    _, bts = cut(shape)
    o_of = {}
    for bt in bts:
        if bt["m"]:
            for s in range(bt["a"], bt["b"]):
                o_of[s] = bt["o"]
    seqs, pos = [], 0
    for s, ((L, ml), kind) in enumerate(zip(shape, kinds)):
        mdst = pos + L
        o_batch = o_of.get(s, mdst)
        glo = o_batch - OW - 16
        if kind == "last":
            off = 0
        elif kind == "hbm":      # anywhere in the flushed output
            assert glo - 64 > 0, (s, o_batch)
            off = mdst - rng.randrange(0, glo - 64)
        elif kind == "far":      # in the ring, before the batch
            assert o_batch >= 200, (s, o_batch)
            off = mdst - (o_batch - rng.randint(100, min(3000, o_batch)))
        elif kind == "pat":      # a period pattern out of its own literals
            off = rng.randint(1, min(15, L))
        else:                    # "own": in its own literals
            off = rng.randint(1, L)
        assert ml == 0 or 0 < off <= min(mdst, 65535), (kind, off, mdst)
        seqs.append((L, off, ml))
        pos = mdst + ml
    lits = [rng.randbytes(L) for L, _, _ in seqs]
    body = [(lit, off, ml) for lit, (_, off, ml) in zip(lits, seqs)]
    if final is not None:
        comp, raw = _lz4build.encode(body[:-1], lits[-1])
    else:
        comp, raw = _lz4build.encode(body)
    assert len(raw) <= BMAX and len(comp) == sum(seq_size(L, ml) for L, ml in shape)
    return comp, raw, seqs


def group(*runs, whole=True):
    """Runs of (count, L, [ml...], kind); whole: a whole number of
    sub-segments, as the sequences between two separators must be."""
    res = []
    for n, L, mls, kind in runs:
        res += [(L, mls[i % len(mls)], kind) for i in range(n)]
    assert not whole or sum(seq_size(L, ml) for L, ml, _ in res) % SUB == 0
    return res


def specs():
    """name -> (parts, final) of every block."""
    sp = {}
    # one sub-segment: m = 1, N = 2
    sp["one_sub"] = ([(1, 3000, "own")], 5)
    # 64 and 65 sub-segments, the payload's end swept over a chunk boundary
    for n in range(2033, 2051):
        parts = [(27, 4, "own")] * 64          # 31 payload bytes each
        last = n - 64 * 31 - 2                 # the last run's token and extension byte
        assert seq_size(last, 0) == n - 64 * seq_size(27, 4)
        sp["len%d" % n] = (parts, last)
    # the sequence limit, 3-byte sequences: 128 in 12 sub-segments, twice
    sp["seq3"] = ([G] + group((256, 0, [4, 9, 18, 16], "far")) + [G], 5)
    # N = 128 by the sequence limit with 8-byte sequences, N = 65 and N = 1
    # by the byte limit (the separators); HBM- and ring-sourced matches
    sp["n128_n65"] = ([G, G] + group((160, 5, [8, 18, 16], "far")) + [G] +
                      group((64, 13, [12, 18, 5], "hbm"), (1, 28, [9], "far")) + [G], 5)
    # the byte limit in lane 63: 64 sub-segments of OW bytes together (m = 64,
    # N = 64), then the same with a byte more (m = 63)
    full = group((48, 27, [37], "far"), (16, 27, [36], "own"))
    over = group((48, 27, [37], "far"), (15, 27, [36], "own"), (1, 27, [37], "pat"))
    assert sum(L + ml for L, ml, _ in full) == OW
    sp["bytes63"] = ([G] + full + [G] + over + [G], 5)
    # m = 0 at the block's start (a match of 5,000 bytes in sub-segment 0),
    # 64 sub-segments straight to HBM, ordinary batches after them
    sp["over_first"] = ([(13, 5000, "pat")] + [(5, 12, "own"), (5, 9, "pat")] * 200 + [(5, 18, "far")] * 60, 5)
    # ... and after ordinary batches (the oversized one on a sub-segment of
    # its own, so that a batch starts at it)
    sp["over_later"] = ([G] + group((128, 5, [11, 18], "far")) + [(9, 5000, "pat")] +
                        [(5, 12, "own"), (5, 9, "far")] * 200, 5)
    # dealings with all pieces in one round (N = 96: rounds of 64 and 32)
    a_hbm, a_far = (64, 5, [16], "hbm"), (64, 5, [8, 12], "far")
    sp["lit_01"] = ([G, G] + group(a_far, (32, 20, [8], "far")) + [G], 5)
    sp["lit_10"] = ([G, G] + group((64, 20, [8], "far"), (32, 5, [8, 12], "far")) + [G], 5)
    sp["hbm_01"] = ([G, G] + group(a_hbm, (32, 4, [24, 40], "hbm")) + [G], 5)
    sp["hbm_10"] = ([G, G] + group((64, 4, [24, 40], "hbm"), (32, 5, [16], "hbm")) + [G], 5)
    sp["ring_01"] = ([G, G] + group(a_hbm, (32, 4, [40, 24], "far")) + [G], 5)
    sp["ring_10"] = ([G, G] + group((64, 4, [40, 24], "far"), (32, 5, [16], "hbm")) + [G], 5)
    # the block's last sequence in lane 63 of a full round: 63 sequences and
    # the last literal run, 64 sequences and no run, 127 and the run
    sp["last63_run"] = ([G] + group((62, 13, [18, 7], "far"), (1, 12, [8], "own"), whole=False), 16)
    sp["last63_match"] = ([G] + group((64, 13, [18, 7], "far")), None)
    sp["last127_run"] = ([G] + group((126, 5, [18, 7], "far"), (1, 4, [8], "own"), whole=False), 8)
    return sp


_built = {}


def blocks():
    if not _built:
        rng = random.Random(0x63A1)
        _built["b"] = {name: build(rng, *s) for name, s in specs().items()}
    return _built["b"]


def model():
    """name -> (nsub, batches, [rounds(batch)]) of every block."""
    res = {}
    for name, (comp, raw, seqs) in blocks().items():
        nsub, bts = cut([(L, ml) for L, _, ml in seqs])
        assert nsub == (len(comp) + SUB - 1) // SUB and sum(bt["bytes"] for bt in bts) == len(raw)
        res[name] = (nsub, bts, [rounds(seqs, bt) if bt["m"] else None for bt in bts])
    return res


def test_cut_agrees_with_the_dealt_overflow_model():
    """Where the other file's model applies (no length with a second
    extension byte), the two cut alike."""
    n = 0
    for name, (comp, raw, seqs) in blocks().items():
        shape = [(L, ml) for L, _, ml in seqs]
        if all(L < 270 and ml < 274 for L, ml in shape[:-1]) and shape[-1][1] == 0 and shape[-1][0] < 270:
            # (the other model leaves out a batch that holds no sequence start)
            ours = [(bt["o"], bt["a"], bt["b"]) if bt["m"] else None for bt in cut(shape)[1]
                    if bt["b"] > bt["a"] or not bt["m"]]
            assert ours == batches(shape), name
            n += 1
    assert n >= 18


def test_model_covers_the_cases():
    M = model()
    N = lambda bt: bt["b"] - bt["a"]
    # sub-segment counts
    assert M["one_sub"][0] == 1 and [bt["m"] for bt in M["one_sub"][1]] == [1]
    assert {M["len%d" % n][0] for n in range(2033, 2049)} == {64}
    assert {M["len%d" % n][0] for n in (2049, 2050)} == {65}
    assert [bt["m"] for bt in M["len2048"][1]] == [64] and [bt["m"] for bt in M["len2049"][1]] == [64, 1]
    # the limit that cuts
    seq3 = [bt for bt in M["seq3"][1] if bt["why"] == "seq"]
    assert [(bt["m"], N(bt)) for bt in seq3] == [(12, 128)], seq3
    g = M["seq3"][1][0]
    assert (g["m"], N(g), g["bytes"], g["why"]) == (1, 1, OW, "bytes")  # lane 0
    b63 = M["bytes63"][1]
    assert (64, 64, OW, "lanes") in [(bt["m"], N(bt), bt["bytes"], bt["why"]) for bt in b63]  # lane 63
    assert (63, 63, "bytes") in [(bt["m"], N(bt), bt["why"]) for bt in b63]
    first = M["over_first"][1]
    assert first[0]["m"] == 0 and first[0]["k0"] == 0 and all(bt["m"] > 0 for bt in first[1:]) and len(first) > 2
    later = M["over_later"][1]
    i = [bt["m"] for bt in later].index(0)
    assert i >= 2 and len(later) > i + 2 and all(bt["m"] > 0 for bt in later[i + 1:])
    # sequence counts
    ns = {(N(bt), bt["why"]) for bt in M["n128_n65"][1]}
    assert {(128, "seq"), (65, "bytes"), (1, "bytes")} <= ns, ns
    assert 64 in [N(bt) for bt in b63]
    # dealings with every piece in one round
    for d, kind in enumerate(("lit", "hbm", "ring")):
        for name, want in ((kind + "_01", (False, True)), (kind + "_10", (True, False))):
            hit = [rr for rr in M[name][2] if rr and len(rr[0]) == 2 and
                   (rr[0][0][d] > 0, rr[0][1][d] > 0) == want and (kind != "ring" or rr[1])]
            assert hit, (name, M[name][2])
    # the block's last sequence in lane 63 of a full round
    for name, n in (("last63_run", 64), ("last63_match", 64), ("last127_run", 128)):
        bt = M[name][1][-1]
        assert N(bt) == n and bt["b"] == len(blocks()[name][2]), (name, bt)


FRAME_BLOCKS = 20


@pytest.fixture(scope="module")
def frames():
    """The blocks in frames of FRAME_BLOCKS, with the oracle's output."""
    import lz4frame
    from test_gpu_parity import oracle_blocks
    bl = list(blocks().items())
    res = []
    for k in range(0, len(bl), FRAME_BLOCKS):
        part = bl[k:k + FRAME_BLOCKS]
        frame, _ = lz4frame.build_frame([(c, r, False) for _, (c, r, _) in part], BMAX, indep=True,
                                        block_cksum=bool((k // FRAME_BLOCKS) & 1))
        ref = oracle_blocks(frame, len(part))
        assert ref == [r for _, (_, r, _) in part]  # the builder's own bytes are the reference's
        res.append(([name for name, _ in part], frame, ref))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["idx1", "pp2", "product"])
def test_uniform_reads(frames, variant):
    import lz4ada
    from test_gpu_parity import _run_variant_alone
    v = {"idx1": lz4ada.DECODE_IDX1_ALONE, "pp2": lz4ada.DECODE_PP2_ALONE,
         "product": lz4ada.DECODE_IDX}[variant]
    bad = []
    for names, frame, ref in frames:
        descs, st, out = _run_variant_alone(frame, v)
        for i, r in enumerate(ref):
            o = descs[i].out_off
            if st[i].code != 0 or st[i].out_len != len(r) or out[o:o + len(r)] != r:
                got = out[o:o + len(r)]
                j = next((x for x in range(len(r)) if got[x] != r[x]), -1)
                bad.append((names[i], st[i].code, st[i].out_len, len(r), j))
    assert not bad, bad  # (block, status code, out_len, expected, first differing byte)
