"""The seek index's linked build over more than one decode pass (DESIGN.md
§16, §19, §20): linked frames between independent, skippable and refused ones,
built under a byte budget that two linked frames fill, without a dictionary and
with a short and a full one.  Every taken frame is read back at every block
boundary against the whole-frame decode (with a dictionary the host decoder's,
without one the device decode's), and what the index holds -- the reasons, the
block starts, its device bytes -- against the values the parent of the commit
that moved the build onto the many-frame pass's stages gave for these frames."""
import struct

import pytest
import torch

import lz4ada
from test_gpu_frames_device import to_host
from test_gpu_frames_dict import dict_bytes, indep_frame, layout, linked_frame, to_device
from test_gpu_ranges import check, ranged
from test_gpu_ranges_linked import boundary_ranges

pytestmark = pytest.mark.gpu

LINKED_LENS = [65536] * 3
# per job, in the frames' order: linked, independent, skippable, linked, refused, linked, independent, linked
LENS = [LINKED_LENS, [3000, 500], [], LINKED_LENS, None, LINKED_LENS, [65536, 77], LINKED_LENS]
REFUSED = 4
# a linked frame's tight slots and the largest dictionary's gap in front of them: two such frames fill a pass
BUDGET = 2 * (3 * 65536 + 65792)

# From the parent commit's library, for these frames:
# the refused frame's reason, seek_index_debug's block starts, device_bytes by dictionary length.
PARENT_REASON = lz4ada.BATCH_NOT_INDEXED
PARENT_STARTS = [[0, 65536, 131072, 196608], [0, 3000, 3500], [0], [0, 65536, 131072, 196608], [0],
                 [0, 65536, 131072, 196608], [0, 65536, 65613], [0, 65536, 131072, 196608]]
PARENT_DEVICE_BYTES = {0: 525392, 4096: 529808, 65536: 591248}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def eight_frames(d):
    """The eight frames under the dictionary d (b"": none)."""
    frames = []
    for job, lens in enumerate(LENS):
        if lens == LINKED_LENS:
            frames.append(linked_frame(lens, d, 2000 + job, content_cksum=True)[0])
        elif lens == []:
            frames.append(struct.pack("<II", 0x184D2A55, 9) + b"skippable")
        elif lens is None:
            f = indep_frame([5000], d, 2000 + job)[0]
            frames.append(f[:len(f) - 40])  # cut short: the walk does not index it
        else:
            frames.append(indep_frame(lens, d, 2000 + job, block_cksum=True)[0])
    return frames


def whole_frames(frames, t, spans, d):
    """What every taken frame decodes to as a whole."""
    if d:
        return [lz4ada.decode_frame_dict_host(f, d)[0] if LENS[job] else b"" for job, f in enumerate(frames)]
    out, jobs = lz4ada.decode_frames_tensor(t, spans, linked=True)
    out = to_host(out)
    assert all(j.status == 0 for k, j in enumerate(jobs[:len(frames)]) if k != REFUSED)
    return [out[j.out_off:j.out_off + j.out_len] for j in jobs[:len(frames)]]


def build_facts(dict_len, monkeypatch):
    """The build under BUDGET -> (frames tensor, index, expected bytes per job, its decode passes)."""
    d = dict_bytes(dict_len, seed=dict_len) if dict_len else b""
    frames = eight_frames(d)
    data, spans = layout(frames)
    t, dt = to_device(data), (to_device(d, 3) if d else None)
    raws = whole_frames(frames, t, spans, d)
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(BUDGET))
    idx = lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=65536, dict=dt)
    built = lz4ada.last_batch_stats().passes
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES")
    return t, idx, raws, built


@pytest.mark.parametrize("dict_len", [0, 4096, 65536])
def test_linked_build_in_two_passes(dict_len, monkeypatch):
    t, idx, raws, built = build_facts(dict_len, monkeypatch)
    with idx:
        assert built >= 2  # four linked frames, two to a pass
        for job, lens in enumerate(LENS):
            j = idx.jobs[job]
            if job == REFUSED:
                assert (j.status, j.reason, j.out_len) == (lz4ada.EXACT_PATH, PARENT_REASON, 0)
            else:
                assert (j.status, j.reason, j.out_len) == (0, 0, sum(lens)), job
                assert len(raws[job]) == sum(lens), job
        stream = torch.cuda.current_stream().cuda_stream
        debug = lz4ada.seek_index_debug(idx, stream)
        assert [r for r, _ in debug] == [PARENT_REASON if job == REFUSED else 0 for job in range(len(LENS))]
        assert [s for _, s in debug] == PARENT_STARTS
        assert idx.device_bytes == PARENT_DEVICE_BYTES[dict_len]
        ranges = [r for job, lens in enumerate(LENS) if lens for r in boundary_ranges(lens, job, sizes=(2,))]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, raws)
