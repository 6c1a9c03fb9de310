"""The frame walk's take_linked option (LZ4ADA_FRAMES_LINKED)
on the host, no GPU needed: with the flag off lz4ada_frame_walk_host_opt is
lz4ada_frame_walk_host on every vector and fixture; with it on, a verdict
changes only where it was BATCH_LINKED, to BATCH_OK exactly when the frame's
slots are within lz4ada_batch_linked_max(); a linked frame that breaks the
lone-block rule is BATCH_BIG_BLOCK; lz4ada_stream_index_opt (classify, the
rules' other statement) says the same of every frame; and the walk with the
option runs clean under AddressSanitizer / UBSan as a stand-alone program
(tools/frame_walk_linked_asan.cpp)."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

import lz4ada
import lz4frame
from test_frame_walk_cpu import BUILT, FILES, stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINKED64K = os.path.join(ROOT, "tests", "golden", "lz4f", "linked64k.lz4")


def walk_opt(data, flags):
    """(verdict, info bytes, descriptor bytes) of lz4ada_frame_walk_host_opt."""
    info = lz4ada.FrameInfo()
    v = lz4ada._lib.lz4ada_frame_walk_host_opt(lz4ada._addr(data), len(data), flags, ctypes.byref(info), None, 0)
    descs = (lz4ada.BlockDesc * max(info.nblocks, 1))()
    v2 = lz4ada._lib.lz4ada_frame_walk_host_opt(lz4ada._addr(data), len(data), flags, ctypes.byref(info), descs,
                                                info.nblocks)
    assert v2 == v
    return v, bytes(info), bytes(descs)[:32 * info.nblocks] if v != lz4ada.BATCH_NOT_INDEXED else b""


def walk_plain(data):
    v, info, descs = lz4ada.frame_walk_host(data)
    return v, bytes(info), bytes(descs)[:32 * info.nblocks] if v != lz4ada.BATCH_NOT_INDEXED else b""


def slots_of(data):
    """Sum of the frame's slots as a pass lays them out (round256 of each slot capacity)."""
    info, descs = lz4ada.frame_index(data)
    total = 0
    for d in descs[:info.nblocks]:
        cap = d.in_len if d.flags & lz4ada.BLOCK_STORED else min(info.block_max, 255 * d.in_len + 64)
        total += (cap + 255) & ~255
    return total


def listed_reason(data, flags):
    """The first frame's reason from lz4ada_stream_index_opt, None when it does not index."""
    n = ctypes.c_int64()
    entries = (lz4ada.StreamEntry * 1)()
    lz4ada._lib.lz4ada_stream_index_opt(lz4ada._addr(data), len(data), flags, entries, 1, ctypes.byref(n))
    return entries[0].batchable if n.value >= 1 else None


def frames_of(data):
    """The input, and every later frame of a concatenated one with whatever follows it."""
    try:
        entries = lz4ada.stream_index(data)
    except lz4ada.LZ4AdaError as e:
        entries = e.entries
    return [data] + [data[e.offset:] for e in entries[1:]]


def check_on(data):
    """The flag on: the plain verdict unless that is BATCH_LINKED; then the cap
    decides, after the lone-block rule.  The host's other statement agrees."""
    v0, info0, descs0 = walk_plain(data)
    v1, info1, descs1 = walk_opt(data, lz4ada.FRAMES_LINKED)
    assert (info1, descs1) == (info0, descs0)  # info.independent stays 0 either way
    if v0 != lz4ada.BATCH_LINKED:
        assert v1 == v0
    elif v1 != lz4ada.BATCH_BIG_BLOCK:
        assert (v1 == lz4ada.BATCH_OK) == (slots_of(data) <= lz4ada.batch_linked_max())
        assert v1 in (lz4ada.BATCH_OK, lz4ada.BATCH_LINKED)
    listed = listed_reason(data, lz4ada.FRAMES_LINKED)
    assert v1 == (lz4ada.BATCH_NOT_INDEXED if listed is None else listed)
    return v0, v1


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    monkeypatch.delenv("LZ4ADA_BATCH_LINKED", raising=False)
    monkeypatch.delenv("LZ4ADA_BATCH_LINKED_MAX", raising=False)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_flag_off_is_the_plain_walk(path):
    with open(path, "rb") as fh:
        data = fh.read()
    for d in frames_of(data):
        assert walk_opt(d, 0) == walk_plain(d)
        listed = listed_reason(d, 0)
        assert walk_plain(d)[0] == (lz4ada.BATCH_NOT_INDEXED if listed is None else listed)


@pytest.mark.parametrize("name", sorted(BUILT))
def test_flag_off_is_the_plain_walk_on_built_frames(name):
    assert walk_opt(BUILT[name], 0) == walk_plain(BUILT[name])


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_flag_on_changes_only_linked_verdicts(path, monkeypatch):
    with open(path, "rb") as fh:
        data = fh.read()
    # a cap every fixture is within, then one only the small ones are
    for cap in (64 << 20, 300 << 10):
        monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(cap))
        for d in frames_of(data):
            check_on(d)


def test_linked_fixtures_are_seen():
    """Not vacuous: the fixtures hold linked frames on both sides of a cap."""
    seen = set()
    os.environ["LZ4ADA_BATCH_LINKED_MAX"] = str(300 << 10)
    try:
        for path in FILES:
            with open(path, "rb") as fh:
                seen.add(check_on(fh.read()))
    finally:
        del os.environ["LZ4ADA_BATCH_LINKED_MAX"]
    assert (lz4ada.BATCH_LINKED, lz4ada.BATCH_OK) in seen
    assert (lz4ada.BATCH_LINKED, lz4ada.BATCH_LINKED) in seen


def test_cap_just_below_and_just_above_a_fixture(monkeypatch):
    with open(LINKED64K, "rb") as fh:
        data = fh.read()
    slots = slots_of(data)
    assert slots == 17 * 65536  # 17 full blocks
    assert walk_plain(data)[0] == lz4ada.BATCH_LINKED
    for cap, want in ((slots - 1, lz4ada.BATCH_LINKED), (slots, lz4ada.BATCH_OK), (slots + 1, lz4ada.BATCH_OK)):
        monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(cap))
        assert lz4ada.batch_linked_max() == cap
        assert walk_opt(data, lz4ada.FRAMES_LINKED)[0] == want
        assert lz4ada.frame_walk_host(data, linked=True)[0] == want
        assert listed_reason(data, lz4ada.FRAMES_LINKED) == want
        assert lz4ada.stream_index(data, linked=True)[0].batchable == want
        # without the flag the cap changes nothing
        assert walk_opt(data, 0)[0] == lz4ada.BATCH_LINKED
        assert lz4ada.stream_index(data)[0].batchable == lz4ada.BATCH_LINKED
    v, info, _ = lz4ada.frame_walk_host(data, linked=True)
    assert (v, info.independent, info.nblocks) == (lz4ada.BATCH_OK, 0, 17)


def test_environment_switch_is_the_flag_of_the_plain_entries(monkeypatch):
    with open(LINKED64K, "rb") as fh:
        data = fh.read()
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(64 << 20))
    assert lz4ada.stream_index(data)[0].batchable == lz4ada.BATCH_LINKED
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED", "1")
    assert lz4ada.stream_index(data)[0].batchable == lz4ada.BATCH_OK
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED", "0")
    assert lz4ada.stream_index(data)[0].batchable == lz4ada.BATCH_LINKED


def test_linked_frame_under_the_lone_block_rule_is_big_block(monkeypatch):
    """The lone-block rule is judged before the cap.  (The 4 MiB slot rule
    cannot meet a linked frame: only a legacy block's slot exceeds 4 MiB, and a
    legacy frame is never linked.)"""
    rng = random.Random(12)
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(64 << 20))
    lone = lz4frame.build_frame([stored(rng.randbytes(600 << 10))], 4 << 20, indep=False)[0]
    assert walk_plain(lone)[0] == lz4ada.BATCH_LINKED
    assert check_on(lone)[1] == lz4ada.BATCH_BIG_BLOCK
    # 25 blocks: over the rule's count, so the cap decides
    many = lz4frame.build_frame([stored(rng.randbytes(600 << 10))] + [stored(rng.randbytes(5))] * 24, 4 << 20,
                                indep=False)[0]
    assert check_on(many)[1] == lz4ada.BATCH_OK
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(600 << 10))
    assert check_on(many)[1] == lz4ada.BATCH_LINKED
    assert check_on(lone)[1] == lz4ada.BATCH_BIG_BLOCK


def test_built_frames_with_the_flag(monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(1 << 20))
    for name, data in sorted(BUILT.items()):
        v0, v1 = check_on(data)
        assert v1 == (lz4ada.BATCH_OK if name == "linked" else v0), name


def test_walk_option_under_the_sanitizers(tmp_path):
    """The stand-alone program, host code only: every truncation of linked and
    other frames in exact-size heap blocks, the option off and on."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "frame_walk_linked_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "bo-lz4-ada_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_walk_linked_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "no sanitizer report, every verdict as expected" in r.stdout
    assert "FAIL" not in r.stdout
