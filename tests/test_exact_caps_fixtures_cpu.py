"""The fixture blocks of test_gpu_exact_caps.py (tests/_capblocks.py), checked
without a GPU: the oracle decodes every block alone to the expected bytes, the
host statement of the size rule gives its length, every class holds the
residues and magnitudes it is there for, the two sparse classes are over the
thresholds that route them to k_decode_sparse, and the set stays small.  The
blocks with rewritten offsets keep their size under the rule; the oracle's
verdict on each is what the GPU test holds the decoders to."""
import pytest

import lz4ada
import lz4frame
import _capblocks as C
from test_gpu_frames_linked import oracle_alone
from test_gpu_lone import oracle_block

MiB = 1 << 20


@pytest.fixture(scope="module")
def blocks():
    return tuple(C.cap_blocks())


def test_oracle_decodes_every_block_alone(blocks):
    for b in blocks:
        if b.stored:  # no raw block decode for these: a frame of them alone, below
            assert b.payload == b.want, b
            continue
        ok, got = oracle_block(b.payload, C.BMAX)
        assert ok and got == b.want, b
    stored = [b for b in blocks if b.stored]
    frame, raw = lz4frame.build_frame([(b.payload, b.want, True) for b in stored], C.BMAX)
    assert lz4ada.frame_index(frame)[0].nblocks == len(stored)
    assert oracle_alone(frame) == raw == b"".join(b.want for b in stored)


def test_size_rule_gives_every_length(blocks):
    for b in blocks:
        assert lz4ada.block_size_host(b.payload, b.stored) == b.size, b


def test_classes_hold_their_residues_and_magnitudes(blocks):
    by = {}
    for b in blocks:
        by.setdefault(b.cls, []).append(b)
    assert set(by) == set(C.GEN) | {"rand", "stored", "empty", "sparse_ratio", "sparse_density"} | set(C.ENDINGS)
    # the empty block is its own case: one zero token, and a stored block of no bytes
    assert sorted((b.payload, b.stored) for b in by["empty"]) == [(b"", True), (b"\x00", False)]
    assert all(b.size == 0 for b in by["empty"])
    full = set(C.RESIDUES)
    for cls in C.GEN + ("rand", "stored"):
        bases = C.BASES + ((C.BIG_BASE,) if cls in C.GEN else ())
        for base in bases:
            have = {b.size - base for b in by[cls] if C.magnitude(b.size) == base}
            assert have == (full - {0} if base == 0 else full), (cls, base)
        assert all(C.magnitude(b.size) in bases for b in by[cls]), cls
    # the crafted endings: every residue per ending, every magnitude the ending fits in,
    # and all eight residues at each magnitude over the four endings together
    for cls in C.ENDINGS:
        assert {b.size % 256 for b in by[cls]} == full, cls
        mags = {C.magnitude(b.size) for b in by[cls]}
        assert mags == (set(C.BASES) - {0} if cls == "match300_off1" else set(C.BASES)), cls
        have = {b.size - 3840 for b in by[cls] if C.magnitude(b.size) == 3840}
        assert have == full, cls
    for base in C.BASES:
        have = {b.size - base for cls in C.ENDINGS for b in by[cls] if C.magnitude(b.size) == base}
        assert have == (full - {0} if base == 0 else full), base
    for cls in ("sparse_ratio", "sparse_density"):
        assert {b.size % 256 for b in by[cls]} >= set(C.SPARSE_RESIDUES), cls


def test_crafted_endings_end_as_named(blocks):
    for b in blocks:
        if b.cls not in C.ENDINGS:
            continue
        seqs, last = C.parse(b.payload)
        if b.cls == "match_end":
            assert last is None and seqs[-1]["out"] + seqs[-1]["ml"] == b.size, b
        elif b.cls == "match300_off1":
            assert last is not None and last[1] == 0, b
            assert seqs[-1]["off"] == 1 and seqs[-1]["ml"] >= 300 and seqs[-1]["out"] + seqs[-1]["ml"] == b.size, b
        elif b.cls == "lit16_end":
            assert last is not None and last[1] >= 16, b
        else:
            assert last is not None and last[1] == 1, b


def test_sparse_classes_are_over_the_thresholds(blocks):
    for b in blocks:
        n = len(b.payload)
        if b.cls == "sparse_ratio":  # RLE_MIN_IN payload bytes, and over 64 times them: by the exact cap and the nominal one
            assert n >= 4096 and b.size > 64 * n and 64 * n < min(C.BMAX, 255 * n + 64), b
        elif b.cls == "sparse_density":  # 64 KiB of payload and more, a handful of sequences
            assert n >= 65536 and len(C.parse(b.payload)[0]) < 128, b
        elif b.cls in ("rle", "literal") and b.size < C.BIG_BASE:
            # up to 64 KiB the generator's own blocks reach neither class (its 256 KiB literal
            # blocks have the payload for the density rule; whether pass 1 declines them is its call)
            assert n < 65536 and not (n >= 4096 and b.size > 64 * n), b


def test_the_set_is_small(blocks):
    assert sum(b.size for b in blocks) < 16 * MiB
    assert max(b.size for b in blocks) <= C.BMAX
    assert len({b.name for b in blocks}) == len(blocks)


# ------------------------------------------------------------ rewritten offsets

@pytest.fixture(scope="module")
def rewritten():
    return tuple(C.rewritten_blocks())


def test_rewritten_offsets_keep_the_size_and_split_the_oracle(rewritten):
    assert len(rewritten) >= 40
    rejected = changed = 0
    kinds = set()
    for w in rewritten:
        ok0, raw = oracle_block(w.original, C.BMAX)
        assert ok0 and len(raw) < 65000, w.name
        assert 1 <= len(w.fields) <= 3 and len(w.payload) == len(w.original), w.name
        differ = [i for i in range(len(w.payload)) if w.payload[i] != w.original[i]]
        assert differ and all(any(at <= i < at + 2 for at, _, _ in w.fields) for i in differ), w.name
        # the size rule does not judge offsets: these blocks reach a decoder with an exact cap
        assert lz4ada.block_size_host(w.payload) == lz4ada.block_size_host(w.original) == len(raw), w.name
        ok, got = oracle_block(w.payload, C.BMAX)
        kinds |= {k for _, k, _ in w.fields}
        if not ok:
            rejected += 1
            assert any(k != "other" for _, k, _ in w.fields), w.name  # every valid offset decodes
        else:
            assert len(got) == len(raw), w.name
            changed += got != raw
        if any(k in ("zero", "before_block", "max") for _, k, _ in w.fields):
            assert not ok, w.name  # offset 0 and a reference before the block are rejected
    assert kinds == set(C.REWRITES)
    assert rejected >= 10 and changed >= 10, (rejected, changed)
