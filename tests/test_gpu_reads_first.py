"""Pass 2 with the LDS reads of a store step issued before the step's stores.

`ring_pieces` reads both units of a piece and the pattern selectors before it
stores either unit.  That is valid only while no read of a step meets a store
of the same step.  The same order was tried, and not kept, for `ring_match`
(the next unit read before the current one is stored) and for L (both rounds'
literal pieces fetched before either round's are stored); the blocks for them
stay, since they pin the order those two have.  The blocks are crafted around
the places where a read and a store of one step lie closest:

* dealt batches (some ring match over 32 bytes): pieces one of whose units
  reads a lower piece's output while the other's source is final; copies whose
  source abuts their own output; overlaps whose period wrap falls in the first
  unit, the second, or both; patterns -- each ready in a batch's first step
  and in a later one;
* lane-per-match batches (no ring match over 32 bytes): matches of 17..32
  bytes, plain, overlapping and patterns, far and near (chains that are
  forwarded among them), in both rounds of a batch and around the output
  window's end;
* literal runs of 1, 15, 16 and 17 bytes in both rounds of a batch, round 1's
  beginning around the input ring's end, and in a block's last batch.

A model of the batch cut (test_gpu_dealt_overflow's) and of the piece rule
(test_gpu_ring_pieces32's) says which batch, round and step a case lands in;
the `test_model_*` tests (CPU) assert that every case listed occurs where it
is meant to.  The GPU tests require the oracle's bytes and length for every
block from each variant alone and from the linked planes, and that no variant
declines a block."""
import random

import pytest

import _lz4build
from test_gpu_dealt_overflow import BMAX, MAXSEQ, OW, RING_LANE_MAX, SUB, batches, match_pieces, seq_size
from test_gpu_ring_pieces32 import Builder, batch_ring, cut_pieces, model_block, pattern_step

ORING = 8192
IRING = 8192           # the input ring: 4 staged chunks of 2 KiB
ABUT_ML = [17, 31, 32, 33, 48]
ABUT_D = [0, 1, 15]
WIDE_OFF = [16, 17, 23, 31, 32]
# (lengths past 2 off + 1: the second piece has two units, both wrapping the period)
WIDE_MORE = [(17, 49), (17, 64), (19, 50), (21, 55)]
LIT_RUNS = [1, 15, 16, 17]
LIT_MIX = 2 * LIT_RUNS + [0, 3, 7]   # (the others vary the runs' payload positions)
LANE_ML = list(range(17, 33))
UNIT_REPS = 4


def wide_mls(off):
    return list(range(off + 1, 2 * off + 2))


def pat_mls(off):
    stp = pattern_step(off)
    return sorted({17, 33, stp + 16, stp + 17})


def unit_cuts(off, ml, k):
    """(cut1, cut2) of piece k of an overlap with off >= 16 (ring_pieces'
    packing: 16 where the unit's read does not wrap the period; cut2 None
    for a one-unit piece)."""
    base = 32 * k
    rem = base % off
    cut1 = off - rem if off - rem < 16 else 16
    if ml - base <= 16:
        return cut1, None
    rem2 = (rem + 16) % off if rem + 16 >= off else rem + 16
    cut2 = off - rem2 if off - rem2 < 16 else 16
    return cut1, cut2


# ---- dealt batches --------------------------------------------------------

def producer(b, rng, L=None, ml=40):
    """a far match over RING_LANE_MAX bytes: it deals its batch, and what
    follows it without literals reads this chunk's output"""
    return b.far(rng.randint(1, 3) if L is None else L, ml)


def unit_dep_block(rng):
    """Two-unit pieces with one unit's source final and the other's a lower
    piece's output."""
    b = Builder(rng)
    for rep in range(UNIT_REPS):
        # plain copy of 32: its first 16 source bytes are the producer's
        # literals (final), the second 16 the producer's first unit
        producer(b, rng, L=16 + rep, ml=64)
        b.add(0, 80, 32, "u2<-first")
        # ... the reverse: the source's first 16 bytes are the producer's last
        # unit (the exact-length store of its last piece), the rest literals
        producer(b, rng, L=rep, ml=48)
        b.add(16, 32, 32, "u1<-last")
        # ... and the producer's second unit of a two-unit piece, then literals
        producer(b, rng, ml=32)
        b.add(16 + rep, 32 + rep, 32, "u1<-second")
        # an overlap of period 48 = the producer's second unit and 32 literal
        # bytes: piece 0 reads (second unit, literals), piece 1 (literals, the
        # second unit again, past the wrap)
        producer(b, rng, ml=32)
        b.add(32, 48, 64 + rep, "wide:u2<-second")
        # a one-unit producer (its piece is one exact-length store)
        producer(b, rng, L=2, ml=40)
        b.add(20, 14, 4 + 8, "P1")
        b.add(16, 28, 28, "u1<-one-unit")
        producer(b, rng, L=2, ml=40)
        b.add(20, 14, 4 + 8)
        b.add(0, 28, 28, "u2<-one-unit")
    return b.finish()


def dealt_form_blocks(rng):
    """Abutting copies, overlaps and patterns, each with its source in its own
    literals (final: ready in the first step) and right behind a producer
    (ready later)."""
    cases = [("abut", ml, ml + d) for ml in ABUT_ML for d in ABUT_D]
    cases += [("wide", ml, off) for off in WIDE_OFF for ml in wide_mls(off)]
    cases += [("wide", ml, off) for off, ml in WIDE_MORE]
    cases += [("pat", ml, off) for off in range(1, 16) for ml in pat_mls(off)]
    # (twice, shuffled anew: a batch cut between a producer and its reader makes
    # that source final; the model test wants each case once as intended)
    cases = [(c, late) for c in cases for late in (False, True)]
    order = []
    for rep in range(2):
        rng.shuffle(cases)
        order += cases
    res = []
    for part in range(0, len(order), 110):
        b = Builder(rng)
        for i, ((kind, ml, off), late) in enumerate(order[part:part + 110]):
            if late:
                producer(b, rng, ml=max(40, off + 8))
                b.add(0, off, ml, (kind, ml, off, "late"))
            else:
                if i % 4 == 0:
                    producer(b, rng)
                b.add(off, off, ml, (kind, ml, off, "first"))
        res.append(b.finish())
    return res


# ---- lane-per-match batches -----------------------------------------------

def lane_form(kind, ml, rng):
    """an offset making a match of ml (17..32) bytes plain, overlapping or a pattern"""
    if kind == "plain":
        return ml + rng.choice([0, 1, 3, 15])
    if kind == "wide":
        return rng.randint(16, ml - 1)
    return rng.randint(1, 15)


def lane_blocks(rng):
    """Only matches of at most 32 bytes: every ring match keeps a lane.  Each
    form far (its source well before the batch, or, for the overlaps, its own
    literals) and near (right behind the match before it), and chains of plain
    copies each reading the one before."""
    res = []
    for rep in range(4):
        b = Builder(rng)
        order = [(k, ml, how) for k in ("plain", "wide", "pat") for ml in LANE_ML for how in range(3)]
        rng.shuffle(order)
        for i, (kind, ml, how) in enumerate(order):
            off = lane_form(kind, ml, rng)
            if how == 0:        # far
                if kind == "plain":
                    b.far(rng.randint(0, 3), ml, ("lane", kind, ml, "far"))
                else:
                    b.add(off, off, ml, ("lane", kind, ml, "far"))
            elif how == 1:      # near: the source is the match before it
                b.add(3, 14, 20)
                b.add(0, off, ml, ("lane", kind, ml, "near"))
            else:               # a chain of five plain copies behind it
                b.add(0, off, ml, ("lane", kind, ml, "near"))
                for j in range(5):
                    m = LANE_ML[(i + j) % len(LANE_ML)]
                    m = min(m, b.seqs[-1][2])
                    if m < 17:
                        break
                    b.add(0, m, m, ("lane", "chain", m, j))
            for j in range(rng.randint(0, 4)):
                b.add(14, 14, 4)
        res.append(b.finish())
    return res


EDGE_CLUSTERS = [
    [("far", 24), ("plain", 20), ("wide", 30), ("pat", 21), ("plain", 32)],
    [("pat", 32), ("far", 17), ("plain", 31), ("wide", 18), ("plain", 17)],
    [("wide", 32), ("plain", 25), ("far", 32), ("pat", 17), ("plain", 22)],
]


def edge_blocks(rng):
    """Clusters of 17..32-byte matches from 40 bytes before to 40 bytes past
    every multiple of 8 KiB of the output, each cluster at several phases."""
    res = []
    for rep in range(6):
        b = Builder(rng, filler=0)
        for k in range(1, 8):
            cl = EDGE_CLUSTERS[(k + rep) % len(EDGE_CLUSTERS)]
            L = b.to(ORING * k - 40 - 3 * rep, L_min=1)
            for j, (kind, ml) in enumerate(cl):
                tag = ("edge", k)
                if kind == "far":
                    b.far(L, ml, tag)
                else:
                    b.add(L, lane_form(kind, ml, rng), ml, tag)
                L = (j + rep) % 3
        res.append(b.finish())
    return res


def lane_info(seqs):
    """Every ring match of the block's lane-per-match batches:
    [(sequence, round, near, chain depth, mdst, off, ml)] (ring_lanes' rule: a
    match is far when its source ends before its round's first output byte or
    lies in its own literals; the chain depth counts the plain near matches
    before it, each wholly inside the one before)."""
    res = []
    for bt in batches([(L, ml) for L, _, ml in seqs]):
        if not bt:
            continue
        ring, dealt = batch_ring(seqs, bt)
        if dealt:
            continue
        o_batch, a, b = bt
        pos, rbeg = o_batch, {}
        for s in range(a, b):
            if (s - a) % 64 == 0:
                rbeg[(s - a) // 64] = pos
            pos += seqs[s][0] + seqs[s][2]
        prev = None  # (round, mdst, mend, plain and near, depth)
        for s, mdst, off, ml in ring:
            r = (s - a) // 64
            src = mdst - off
            dep_end = src + min(off, ml)
            near = not (dep_end <= rbeg[r] or off <= seqs[s][0])
            depth = 0
            if near and off >= ml and prev and prev[0] == r and prev[3] and prev[1] <= src and dep_end <= prev[2]:
                depth = prev[4] + 1
            res.append((s, r, near, depth, mdst, off, ml))
            prev = (r, mdst, mdst + ml, near and off >= ml, depth)
    return res


# ---- literals -------------------------------------------------------------

def literal_block(rng, shift, full_last=False):
    """Literal runs of 1, 15, 16 and 17 bytes throughout (4-byte matches
    between them), behind `shift` plain sequences that move the batch cut
    against the input ring.  full_last: as many sequences fewer as it takes
    for the block's last batch to hold all four runs in both its rounds."""
    seqs, pos = [], 0
    for i in range(shift):
        seqs.append((14, 14, 4))
        pos += 18
    i = 0
    while pos < BMAX - 64:
        L = rng.choice(LIT_MIX) if pos else 1  # (a match needs a byte before it)
        seqs.append((L, min(pos + L, 14 + (i % 5)), 4))
        pos += L + 4
        i += 1
    final = LIT_RUNS[shift % 4]
    while full_last and not last_batch_full(seqs + [(final, 0, 0)]):
        seqs.pop()
    lits = [rng.randbytes(L) for L, _, _ in seqs]
    comp, raw = _lz4build.encode([(l, off, ml) for l, (_, off, ml) in zip(lits, seqs)], rng.randbytes(final))
    assert len(raw) <= BMAX
    return comp, raw, seqs + [(final, 0, 0)], {}


def literal_info(seqs):
    """[(batch index, last batch?, round, L, payload position of the run)]"""
    starts, p = [], 0
    for L, _, ml in seqs:
        starts.append(p + 1 + (L >= 15))
        p += seq_size(L, ml) if ml else 1 + (L >= 15) + L
    bts = [bt for bt in batches([(L, ml) for L, _, ml in seqs]) if bt]
    res = []
    for n, (o_batch, a, b) in enumerate(bts):
        for s in range(a, b):
            res.append((n, n == len(bts) - 1, (s - a) // 64, seqs[s][0], starts[s]))
    return res


def last_batch_full(seqs):
    per = {}
    for n, last, r, L, p in literal_info(seqs):
        if last:
            per.setdefault(r, set()).add(L)
    return all(set(LIT_RUNS) <= per.get(r, set()) for r in (0, 1))


def literal_blocks(rng):
    return [literal_block(rng, 8 * j + j % 4, full_last=j % 4 == 0) for j in range(16)]


# ---- the blocks -----------------------------------------------------------

_built = {}


def groups():
    if not _built:
        rng = random.Random(0x5EAD51)
        _built.update(units=[unit_dep_block(rng)], forms=dealt_form_blocks(rng), lanes=lane_blocks(rng),
                      edges=edge_blocks(rng), lits=literal_blocks(rng))
    return _built


GROUPS = ("units", "forms", "lanes", "edges", "lits")


def blocks():
    g = groups()
    return [b for name in GROUPS for b in g[name]]


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


def unit_sources(piece):
    """the source ranges of a plain copy's units"""
    pd, pe, units, (s_lo, s_hi) = piece
    return [(s_lo + d - pd, s_lo + d - pd + n) for d, n in units]


def meets(rng_, out):
    return rng_[0] < out[1] and out[0] < rng_[1]


def test_model_unit_dependencies():
    seen = dealt_tags("units")

    def one_sided(tag, unit, which):
        """every piece of `tag` reads a producer's `which` store with unit
        `unit` alone, the other unit's source being final (a batch cut
        between the two leaves no producer: not in most)"""
        assert len(seen[tag]) == UNIT_REPS, tag
        assert sum(bool(prod) for _, _, prod in seen[tag]) >= UNIT_REPS - 1, tag
        for k, piece, prod in seen[tag]:
            srcs = unit_sources(piece)
            assert len(srcs) == 2
            for _, pk, (ppd, ppe, punits, _) in prod:
                outs = [(d, d + n) for d, n in punits]
                assert not any(meets(srcs[1 - unit], o) for o in outs), tag
                hit = [i for i, o in enumerate(outs) if meets(srcs[unit], o)]
                if which == "first":
                    assert hit == [0] and len(outs) == 2, tag
                elif which == "second":
                    assert hit == [1], tag
                else:
                    assert hit == [0] and len(outs) == 1, tag

    one_sided("u2<-first", 1, "first")
    one_sided("u1<-second", 0, "second")
    one_sided("u1<-last", 0, "one")
    one_sided("u1<-one-unit", 0, "one")
    one_sided("u2<-one-unit", 1, "one")
    # the overlap: piece 0's first unit and piece 1's second read the period's
    # first 16 bytes, which are the producer's second unit
    ws = seen["wide:u2<-second"]
    assert len(ws) >= 2 * UNIT_REPS and all(prod for _, _, prod in ws)
    for k, (pd, pe, units, (s_lo, s_hi)), prod in ws:
        assert s_hi - s_lo == 48
        (_, pk, (ppd, ppe, punits, _)), = prod
        assert len(punits) == 2 and punits[1][0] == s_lo and punits[1][1] == 16
        if k == 1:
            assert len(units) == 2 and (units[1][0] - s_hi) % 48 == 0 and (units[0][0] - s_hi) % 48 == 32


def test_model_dealt_forms():
    seen = dealt_tags("forms")

    def both(kind, ml, off):
        for when in ("first", "late"):
            v = seen.get((kind, ml, off, when))
            assert v, (kind, ml, off, when)
            # ready in the batch's first step: no producer in its chunk; later:
            # the match's first piece has one
            if when == "first":
                assert any(not prod for _, _, prod in v), (kind, ml, off, when)
            else:
                assert any(k == 0 and prod for k, _, prod in v), (kind, ml, off, when)
        return seen[(kind, ml, off, "first")] + seen[(kind, ml, off, "late")]

    for ml in ABUT_ML:
        for d in ABUT_D:
            for k, (pd, pe, units, (s_lo, s_hi)), _ in both("abut", ml, ml + d):
                assert s_hi <= pd  # a plain copy: the source ends at or before the piece
    where = set()
    for off, ml in [(off, ml) for off in WIDE_OFF for ml in wide_mls(off)] + WIDE_MORE:
        for k, piece, _ in both("wide", ml, off):
            c1, c2 = unit_cuts(off, ml, k)
            where.add((c1 < 16, c2 is not None and c2 < 16))
    # the period wrap in the first unit only, the second only, and both
    assert {(True, False), (False, True), (True, True)} <= where, where
    for off in range(1, 16):
        for ml in pat_mls(off):
            both("pat", ml, off)


def test_model_lane_batches():
    seen, chains = {}, 0
    for comp, raw, seqs, tags in groups()["lanes"]:
        for s, r, near, depth, mdst, off, ml in lane_info(seqs):
            if s in tags:
                _, kind, m, how = tags[s]
                seen.setdefault((kind, "near" if near else "far", r), set()).add(m)
                if kind == "chain":
                    chains = max(chains, depth)
    for kind in ("plain", "wide", "pat"):
        for how in ("near", "far"):
            for r in (0, 1):
                assert seen.get((kind, how, r)), (kind, how, r)
            assert seen[(kind, how, 0)] | seen[(kind, how, 1)] == set(LANE_ML), (kind, how)
    assert chains >= 3 and seen[("chain", "near", 0)] and seen[("chain", "near", 1)]
    # around the window's end: in every block, at every multiple of 8 KiB, a
    # lane match across it and others within 40 bytes before and after it
    across = {}
    for comp, raw, seqs, tags in groups()["edges"]:
        info = [x for x in lane_info(seqs) if x[0] in tags]
        for k in range(1, 8):
            w = ORING * k
            ms = [(mdst, mdst + ml) for s, r, near, depth, mdst, off, ml in info
                  if tags[s] == ("edge", k) and 17 <= ml <= 32]
            assert len(ms) == 5, (k, ms)  # all five in lane-per-match batches
            across[k] = across.get(k, 0) + any(a < w < e for a, e in ms)
            assert any(w - 40 < e <= w for a, e in ms) and any(w <= a < w + 40 for a, e in ms), (k, ms)
    assert all(across[k] >= 3 for k in range(1, 8)), across  # (a match may also end right at it)
    rounds = {(r, near) for comp, raw, seqs, tags in groups()["edges"]
              for s, r, near, depth, mdst, off, ml in lane_info(seqs) if s in tags}
    assert len(rounds) == 4, rounds


def test_model_literal_runs():
    both_rounds = last_ok = 0
    before, after = set(), set()
    for comp, raw, seqs, tags in groups()["lits"]:
        info = literal_info(seqs)
        per = {}
        for n, last, r, L, p in info:
            per.setdefault((n, last), {}).setdefault(r, set()).add(L)
            if r == 1 and L in LIT_RUNS:
                d = (p + IRING // 2) % IRING - IRING // 2  # signed distance to a multiple of 8 KiB
                if -16 <= d < 0:
                    before.add(L)
                elif 0 <= d <= 16:
                    after.add(L)
        for (n, last), rr in per.items():
            ok = all(set(LIT_RUNS) <= rr.get(r, set()) for r in (0, 1))
            both_rounds += ok
            last_ok += ok and last
    assert both_rounds >= 16 and last_ok >= 2
    assert before == set(LIT_RUNS) and after == set(LIT_RUNS), (before, after)


def test_model_sizes():
    bl = blocks()
    assert all(len(b[1]) <= BMAX for b in bl) and len(bl) <= 64
    assert MAXSEQ == 128 and SUB == 32 and OW == 4080 and RING_LANE_MAX == 32
    assert match_pieces(16, 33) == 3 and len(cut_pieces(100, 16, 33)) == 2


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
def test_reads_first(frames, variant):
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
@pytest.mark.parametrize("group", GROUPS)
def test_reads_first_linked(group):
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
