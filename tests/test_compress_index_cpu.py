"""The rule by which a compress call writes the seek index of its own frames
(lz4ada_compress_index.h), on the host through
lz4ada_compress_index_host, no GPU needed.  It sees a record's length, the
options and each block's written size; it is pinned here to what the index
build finds by reading the frame: the host frame walk (descriptors, block count,
verdict), the exact-size rule over every payload (lz4ada_block_size_host) and
the chain rule's groups (lz4ada_range_chains_host), over every record the
compressor's CPU tests compress, under every flag combination."""
import itertools

import pytest

import lz4ada
from _compress_cases import BLOCK_LEN, KiB, MiB, id4_records, noise, pseudo_text, record
from _compress_dict_cases import crafted as dict_crafted, text_dict
from _compress_linked_cases import B, LENGTHS, crafted, linked_records, mixed_jobs

FLAGS = [dict(block_checksum=b, content_checksum=c, content_size=s)
         for b, c, s in itertools.product((False, True), repeat=3)]
D64K = text_dict(65536)
EVERY = (0, 65536, 131072)
DEFAULT_EVERY = 1 << 20  # checkpoint_bytes 0


def r256(v):
    return (v + 255) & ~255


def slot_cap(in_len, stored, bmax):
    """walk_slot_cap (lz4ada_frame_walk.h)."""
    return in_len if stored else min(255 * in_len + 64, bmax)


def check(plain, block=65536, d=b"", dict_id=None, linked=False, frame_off=0, out_base=0, **kw):
    """One record: its frame from the serial statement, the rule over it, and
    the walk, the size rule and the chain rule over the frame's bytes."""
    frame = lz4ada.compress_frame_host(plain, block=block, dict=d, dict_id=dict_id, linked=linked, **kw)
    bmax = block
    v, info, want = lz4ada.frame_walk_host(frame, linked=linked)
    nb = info.nblocks
    assert nb == -(-len(plain) // bmax) and info.frame_len == len(frame)
    got = {}
    for every in EVERY:
        got[every] = lz4ada.compress_index_host(frame, len(plain), block=block, dict_id=dict_id, linked=linked,
                                                checkpoint_bytes=every, frame_off=frame_off, out_base=out_base, **kw)
    verdict, descs, sizes, _, _ = got[0]
    assert verdict == v, "the verdict is the walk's"
    assert len(descs) == len(sizes) == nb
    slot = out_base
    for i in range(nb):
        g, w = descs[i], want[i]
        stored = bool(w.flags & lz4ada.BLOCK_STORED)
        # the walk's own fields, one by one; its in_off is frame-relative
        assert (g.in_off - frame_off, g.in_len, g.flags, g.cksum) == (w.in_off, w.in_len, w.flags, w.cksum), i
        # the slots as a pass lays them out (frame_walk with slots == true)
        assert (g.out_off, g.out_cap) == (slot, slot_cap(w.in_len, stored, bmax)), i
        slot += r256(g.out_cap)
        payload = frame[w.in_off:w.in_off + w.in_len]
        assert sizes[i] == lz4ada.block_size_host(payload, stored) == len(plain[i * bmax:(i + 1) * bmax]), i
    for every in EVERY:
        ev, ed, es, group, nck = got[every]
        assert (ev, es) == (verdict, sizes) and [bytes(x) for x in ed] == [bytes(x) for x in descs]
        if not linked or nb == 0 or verdict != lz4ada.BATCH_OK:
            assert (group, nck) == (0, 0)
            continue
        assert group == max(1, -(-(every or DEFAULT_EVERY) // bmax)) or nb == 1
        # every block but the first touched once: the heads are the checkpoints
        marked, head, chains = lz4ada.range_chains_host(nb, group, [(i, 1) for i in range(nb)])
        assert head == list(range(group, nb, group)) and nck == len(head) == len(chains) - 1
    return verdict, nb


def all_records():
    recs = [p for _, p in id4_records()] + [p for _, p in linked_records()]
    recs += mixed_jobs()[2][-5:]  # the jobs that overlap others
    recs += [pseudo_text(n, n + 1) for n in LENGTHS] + [record(n) for n in (0, 1, 12, 13)]
    seen, out = set(), []
    for p in recs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


RECORDS = all_records()


@pytest.mark.parametrize("kw", FLAGS, ids=lambda kw: "".join("bcs"[i] for i, v in enumerate(kw.values()) if v) or "none")
def test_rule_equals_the_walk_on_every_record(kw):
    """Plain, dictionary and linked frames of every record, one flag combination."""
    assert any(len(p) > 2 * B for p in RECORDS) and any(len(p) == 0 for p in RECORDS)
    for k, plain in enumerate(RECORDS):
        check(plain, **kw)
        check(plain, d=D64K, dict_id=7 if k % 2 else None, frame_off=12345, out_base=256 * k, **kw)
        check(plain, linked=True, **kw)
        if k % 4 == 0:
            check(plain, d=D64K, dict_id=9, linked=True, frame_off=77, **kw)


def test_crafted_records():
    """Offsets of exactly 65,535 across a boundary: the dictionary's and the linked ones."""
    for _, d, rec, _ in dict_crafted():
        for kw in (FLAGS[0], FLAGS[-1]):
            check(rec, d=d, **kw)
    for _, rec, _ in crafted():
        for kw in FLAGS:
            assert check(rec, linked=True, **kw) == (lz4ada.BATCH_OK, 2)


def test_larger_blocks():
    """300,000 bytes at 256 KiB, and the lone-block rule: 1 MiB of noise at
    block id 6 is one stored block of 1 MiB, which the build's index stage hands
    to the lone-block path (LZ4ADA_BATCH_BIG_BLOCK); text of that length is not."""
    for kw in FLAGS:
        for linked in (False, True):
            assert check(record(300000), block=256 * KiB, linked=linked, **kw) == (lz4ada.BATCH_OK, 2)
    nz = noise(MiB, 5)
    for linked in (False, True):
        assert check(nz, block=MiB, linked=linked, **FLAGS[-1]) == (lz4ada.BATCH_BIG_BLOCK, 1)
        assert check(nz + nz[:1000], block=MiB, linked=linked) == (lz4ada.BATCH_BIG_BLOCK, 2)
        assert check(pseudo_text(MiB + 5, 3), block=MiB, linked=linked) == (lz4ada.BATCH_OK, 2)
        assert check(nz, block=256 * KiB, linked=linked) == (lz4ada.BATCH_OK, 4)
    assert BLOCK_LEN[6] == MiB


def test_misuse():
    plain = record(70000)
    frame = lz4ada.compress_frame_host(plain)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.compress_index_host(frame, len(plain) + B)  # another block count
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.compress_index_host(frame[:-1], len(plain))
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.compress_index_host(frame, len(plain), block_checksum=True)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.compress_index_host(frame, len(plain), checkpoint_bytes=-1)
