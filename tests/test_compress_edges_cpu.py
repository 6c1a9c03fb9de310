"""The in-block edge cases of tests/_compress_edge_cases.py do what they claim
(DESIGN.md §17).  The serial statement alone decides here: every case with
stated sequences parses to them, the blocks around the stored threshold fall on
both sides of it and are refused at both of the statement's checks, the
alignment ladder covers every combination, and a second reading of the rule in
plain Python, window by window as the kernel reads it, equals the statement on
every record it is given and counts how often the fuzz meets the window's
corner cases.  tests/test_gpu_compress_edges.py then compares the device with
the statement over the same records.  No GPU."""
import collections

import pytest

import _oracle as O
import lz4ada
from _compress_cases import KiB, frame_blocks, parse_block
from _compress_dict_cases import dict_frame_blocks, parse_block_dict
from _compress_edge_cases import (EDGE_DICT, alignment_ladder, continuation_cases, extension_grid, far_repeats,
                                  laid_out, length_edges, near_bound, small_alphabets, window_tail)
from _compress_linked_cases import B, parse_block_linked

ALL = dict(block_checksum=True, content_checksum=True, content_size=True)


def ext_len(v):
    return 0 if v < 15 else (v - 15) // 255 + 1


def seq_len(lit, ml):
    return 1 + ext_len(lit) + lit + 2 + ext_len(ml - 4)


def natural(rec):
    """The block when nothing bounds it."""
    return lz4ada.compress_block_host(rec, len(rec) + 1024)


# ------------------------------------------------------- stated sequences

STATED = [*extension_grid(), *length_edges(), *window_tail()]


def test_the_families_have_their_sizes():
    assert len(extension_grid()) == 149
    assert len(length_edges()) == 13 + 9
    assert len(window_tail()) == 5 * 64
    assert 650 <= len(small_alphabets()) <= 750
    assert 1.2e6 <= sum(len(r) for _, r, _ in small_alphabets()) <= 1.8e6
    names = [c[0] for f in (extension_grid, length_edges, near_bound, window_tail, far_repeats, small_alphabets,
                            alignment_ladder) for c in f()]
    assert len(set(names)) == len(names)


def test_stated_sequences():
    for name, rec, want in STATED:
        assert parse_block(lz4ada.compress_block_host(rec), rec) == want, name
    for name, rec, want in near_bound():
        assert parse_block(natural(rec), rec) == want, name


def test_stated_sequences_under_the_dictionary():
    """EDGE_DICT seeds the table and takes part in no planned sequence."""
    for name, rec, want in STATED:
        got = parse_block_dict(lz4ada.compress_block_host(rec, dict=EDGE_DICT), rec, EDGE_DICT)
        assert got == want, name
    for name, rec, want in near_bound():
        comp = lz4ada.compress_block_host(rec, len(rec) + 1024, dict=EDGE_DICT)
        assert parse_block_dict(comp, rec, EDGE_DICT) == want, name


def test_stated_sequences_in_a_continuation_block():
    """Behind 64 KiB of noise, as block 1 of a linked record: every table entry
    is seeded, and the planned sequences stand."""
    cases = continuation_cases()
    assert len(cases) == 26 + 25 + 18 and sum(len(r) for _, r, _ in cases) < 5 << 20
    stored = []
    for name, rec, want in cases:
        # block 1 is the block function with block 0 in the dictionary's place
        comp = lz4ada.compress_block_host(rec[B:], dict=rec[:B])
        assert parse_block_linked(comp, rec, 1, B) == want, name
        blocks = dict_frame_blocks(lz4ada.compress_frame_host(rec, linked=True))[4]
        assert [b[0] for b in blocks] == [True, len(comp) >= len(rec) - B], name
        if blocks[1][0]:
            stored.append(name)
        else:
            assert blocks[1][1] == comp, name
    assert stored == ["ext_end_ml7"]  # 1,024 literals and a match of 7: one byte over


def test_far_repeats():
    (_, near_rec, _), (_, far_rec, _) = far_repeats()
    assert (0, 65535, 32) in parse_block(lz4ada.compress_block_host(near_rec), near_rec)
    seqs = parse_block(lz4ada.compress_block_host(far_rec), far_rec)
    assert all(ml != 32 for _, _, ml in seqs) and seqs[-1][0] == 32 + 20


# ------------------------------------------------------------- near bound

def refusing_site(rec, seqs):
    """Which of the statement's two checks refuses the block at cap = n - 1:
    the first sequence with op + comp_seq_len > n - 1, else the last literals;
    None when the block fits."""
    op, cap = 0, len(rec) - 1
    for lit, _, ml in seqs[:-1]:
        if op + seq_len(lit, ml) > cap:
            return "sequence"
        op += seq_len(lit, ml)
    lit = seqs[-1][0]
    return "last literals" if op + 1 + ext_len(lit) + lit > cap else None


def near_bound_verdicts():
    """{name: (natural size - n, the refusing site or None)}"""
    return {name: (len(natural(rec)) - len(rec), refusing_site(rec, want)) for name, rec, want in near_bound()}


def test_near_bound_lies_on_both_sides():
    verdicts = near_bound_verdicts()
    for place in ("early", "late"):
        for n in (300, 600):
            diffs = {d for name, (d, _) in verdicts.items() if name.startswith(f"near_n{n}_{place}")}
            assert {-2, -1, 0, 1} <= diffs, (n, place, sorted(diffs))
    for n in (8192, 65536):
        assert sorted(d for name, (d, _) in verdicts.items() if name.startswith(f"near_n{n}_early")) == [-1, 0]
    for name, rec, _ in near_bound():
        comp = lz4ada.compress_block_host(rec, len(rec) - 1)
        d, site = verdicts[name]
        assert bool(comp) == (d <= -1) == (site is None), name
        if comp:
            assert comp == natural(rec), name


def test_near_bound_is_refused_at_both_sites():
    sites = collections.Counter(site for _, site in near_bound_verdicts().values())
    assert sites["sequence"] >= 6 and sites["last literals"] >= 6 and sites[None] >= 6, sites
    # the large late matches are the sequence site's: 1 + ext(lit) + lit + 2 > n - 1 already there
    for name, (_, site) in near_bound_verdicts().items():
        if name.startswith(("near_n8192_late", "near_n65536_late")):
            assert site == "sequence", name


# ------------------------------------------------------- alignment ladder

def ladder_combinations(**kw):
    """(stored, destination % 4, payload length % 4, source % 4) of every block
    of the ladder laid out as the GPU test lays it out."""
    recs = [r for _, r, _ in alignment_ladder()]
    data, spans, order = laid_out(recs, pad=4, shuffle=False)
    at, combos = 0, []
    for (in_off, n), i in zip(spans, order):
        frame = lz4ada.compress_frame_host(recs[i], **kw)
        blocks = frame_blocks(frame)[3]
        assert len(blocks) == (1 if n else 0)
        for stored, payload, _ in blocks:
            dest = at + (15 if kw.get("content_size") else 7) + 4
            assert frame[dest - at:dest - at + len(payload)] == payload
            combos.append((stored, dest % 4, len(payload) % 4, in_off % 4))
        at += len(frame)
    return combos


@pytest.mark.parametrize("kw", [dict(), dict(block_checksum=True)], ids=["plain", "block_checksum"])
def test_alignment_ladder_covers_every_combination(kw):
    combos = ladder_combinations(**kw)
    every = {(d, m) for d in range(4) for m in range(4)}
    assert {(d, m) for stored, d, m, _ in combos if stored} == every
    assert {(d, m) for stored, d, m, _ in combos if not stored} == every
    assert {s for stored, _, _, s in combos if stored} == {0, 1, 2, 3}


# ------------------------------------------------- the rule, read by windows

def rule_model(rec):
    """compress_block of lz4ada_compress_host.cpp with cap = n - 1, read a
    window at a time as the kernel reads it: every lane's lookup before any
    insert, the lowest valid lane, the prefix's inserts by maximum, the
    extension in steps of 256 bytes -> (the block or b"", counts)."""
    n, cap = len(rec), len(rec) - 1
    out, anchor, table, stats = bytearray(), 0, {}, collections.Counter()

    def u32(p):
        return int.from_bytes(rec[p:p + 4], "little")

    def length(v):
        return bytes([255] * ((v - 15) // 255) + [(v - 15) % 255]) if v >= 15 else b""

    if n >= 13:
        mlast, mend = n - 12, n - 5
        w = 0
        while w <= mlast:
            wn = min(64, mlast - w + 1)
            stats["partial last windows"] += wn < 64
            values = [u32(w + k) for k in range(wn)]
            hashes = [(v * 2654435761 & 0xFFFFFFFF) >> 20 for v in values]
            found = [table.get(h) for h in hashes]
            valid = []
            for k, c in enumerate(found):
                if c is not None and w + k - c <= 65535:
                    if u32(c) == values[k]:
                        valid.append(k)
                    else:
                        stats["collisions"] += 1
            winner = valid[0] if valid else wn - 1
            stats["windows with two or more valid lanes"] += len(valid) >= 2
            stats["winners past lane 0"] += bool(valid) and winner > 0
            stats["prefixes with a shared hash"] += len(set(hashes[:winner + 1])) <= winner
            for k in range(winner + 1):
                table[hashes[k]] = max(table.get(hashes[k], -1), w + k)
            if not valid:
                w += wn
                continue
            win, cand, ml, steps = w + winner, found[winner], 4, 0
            while True:
                steps += 1
                take, same = min(256, mend - (win + ml)), 0
                while same < take and rec[cand + ml + same] == rec[win + ml + same]:
                    same += 1
                ml += same
                if same < 256:
                    break
            stats["extensions of two or more steps"] += steps >= 2
            lit = win - anchor
            if len(out) + seq_len(lit, ml) > cap:
                return b"", stats
            out.append(min(lit, 15) << 4 | min(ml - 4, 15))
            out += length(lit) + rec[anchor:win] + (win - cand).to_bytes(2, "little") + length(ml - 4)
            w = anchor = win + ml
    lit = n - anchor
    if len(out) + 1 + ext_len(lit) + lit > cap:
        return b"", stats
    out.append(min(lit, 15) << 4)
    out += length(lit) + rec[anchor:]
    return bytes(out), stats


COUNTED = ["windows with two or more valid lanes", "winners past lane 0", "prefixes with a shared hash", "collisions",
           "partial last windows", "extensions of two or more steps"]


def test_the_model_equals_the_statement():
    """On the fuzz, the window tails and the extension grid; over the fuzz it
    meets every corner of the window's rule (the counts are in DESIGN.md §17)."""
    total = collections.Counter()
    for family in (small_alphabets, window_tail, extension_grid):
        for name, rec, _ in family():
            got, stats = rule_model(rec)
            assert got == lz4ada.compress_block_host(rec, max(len(rec) - 1, 0)), name
            if family is small_alphabets:
                total += stats
    print({k: total[k] for k in COUNTED})
    for k in COUNTED:
        assert total[k] >= 1, k


# ------------------------------------------------------------- the oracle

def test_every_frame_decodes():
    """What equals the statement also decodes: every family's frame with all
    three checksums, through the oracle."""
    cases = [(name, rec, dict()) for f in (extension_grid, length_edges, near_bound, window_tail, far_repeats,
                                           small_alphabets, alignment_ladder) for name, rec, _ in f()]
    cases += [(name + "_id5", rec, dict(block=256 * KiB)) for name, rec, _ in far_repeats()]
    for name, rec, kw in cases:
        st, out, _, msg = O.decode_stream(lz4ada.compress_frame_host(rec, **ALL, **kw), out_cap=len(rec) + 64)
        assert st == O.OK and out == rec, (name, msg)
