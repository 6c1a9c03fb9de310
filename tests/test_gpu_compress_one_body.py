"""The three block compressors are one device body
(lz4ada_compress_block.inc) under three histories: what that promises between
k_compress_blocks, k_compress_blocks_dict and k_compress_blocks_linked, byte
for byte.  A history that holds nothing to match leaves the plain kernel's
bytes, and block 0 of a linked record is the unlinked block.  Every result is
also the serial statement's (lz4ada_compress_frame_host), so equal means equal
and right.  64 KiB blocks, no flag."""
import pytest
import torch

import lz4ada
from _compress_cases import record
from _compress_dict_cases import dict_frame_blocks, text_dict

pytestmark = pytest.mark.gpu

B = 65536
# around the shortest block with a match (13), one window (64 + 12), one block and two
LENGTHS = [0, 1, 12, 13, 14, 64 + 12, B, B + 1, B + 13, 2 * B + 1]
RECS = [record(n, kind) for kind in ("text", "noise") for n in LENGTHS]
SMALL = [r for r in RECS if len(r) <= B]
HLEN = 7  # magic, FLG, BD, HC


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES", raising=False)


def on_device(data):
    t = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda")
    t[:len(data)] = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8)[:len(data)]
    return t[:len(data)]


def frames(recs, d=None, linked=False):
    """One call, one pass, over the records laid out at odd places -> every
    record's frame, each checked against the serial statement.  d: the
    dictionary's bytes, None for a call without one."""
    data, spans = b"", []
    for i, r in enumerate(recs):
        data += b"\x55" * (1 + i % 3)
        spans.append((len(data), len(r)))
        data += r
    out, where = lz4ada.compress_frames_tensor(on_device(data), spans, dict=None if d is None else on_device(d),
                                               linked=linked)
    raw = out.cpu().numpy().tobytes()
    got = [raw[o:o + n] for o, n in where]
    for i, r in enumerate(recs):
        assert got[i] == lz4ada.compress_frame_host(r, dict=d or b"", linked=linked), \
            f"record {i} ({len(r)} bytes) differs from the serial statement"
    return got


@pytest.fixture(scope="module")
def plain():
    return frames(RECS)


def but_flg_and_hc(frame, twin):
    """`frame` with FLG's B.Indep bit and HC taken from `twin`."""
    assert frame[4] == twin[4] ^ 0x20
    return frame[:4] + twin[4:5] + frame[5:HLEN - 1] + twin[HLEN - 1:HLEN] + frame[HLEN:]


@pytest.mark.parametrize("dl", [0, 3])
def test_a_dictionary_too_short_to_seed_is_the_plain_call(dl, plain):
    """Both queue k_compress_blocks: a dictionary under 4 bytes holds no four
    bytes to match, and the call takes the plain kernel for it."""
    assert frames(RECS, text_dict(dl)) == plain


def test_a_dictionary_that_matches_nothing_leaves_the_plain_bytes(plain):
    """Four bytes that occur in no record: k_compress_blocks_dict runs, over a
    table with one entry that no position matches, and gives the frames of
    k_compress_blocks (no id is asked for, so the headers are equal too)."""
    d = bytes([0xff, 0xfe, 0xfd, 0xfc])
    assert not any(d in r for r in RECS)
    assert frames(RECS, d) == plain


def test_linked_without_a_dictionary_is_the_plain_block_0(plain):
    """Records of one block: the plain frame but for FLG and HC, from
    k_compress_blocks (a pass without a continuation block) and again from
    k_compress_blocks_linked (the same records in a pass that holds one)."""
    want = [p for r, p in zip(RECS, plain) if len(r) <= B]
    alone = frames(SMALL, linked=True)
    assert [but_flg_and_hc(f, p) for f, p in zip(alone, want)] == want
    together = frames(RECS, linked=True)
    assert any(len(dict_frame_blocks(f)[4]) == 3 for f in together), "no record of 2 * 65,536 + 1 bytes in the pass"
    assert [f for r, f in zip(RECS, together) if len(r) <= B] == alone


def test_linked_with_a_dictionary_is_the_dictionary_call_in_block_0():
    d = text_dict(4096)
    unlinked, linked = frames(RECS, d), frames(RECS, d, linked=True)
    for i, (u, k) in enumerate(zip(unlinked, linked)):
        assert dict_frame_blocks(k)[4][:1] == dict_frame_blocks(u)[4][:1], f"record {i}: block 0 differs"
