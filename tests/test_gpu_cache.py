"""What the library keeps between calls, seen through device_cache_stats():
there is one device pool, one pinned pool and one stream pool for every host
unit, so release_device_cache() empties what the streaming facade, the bulk
path and the linked bulk path left, and LZ4ADA_POOL_KEEP_MB bounds each kind
once.  The frames are the smallest fixtures that reach each unit's pool use:
indep64k (17 independent 64 KiB blocks) for the facade and the bulk path,
linked256k (7 linked 256 KiB blocks) for the linked bulk path.  The cases
only read counters; nothing here forces a failure."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, PKG, ROOT

import lz4ada

pytestmark = pytest.mark.gpu

TABLE = json.load(open(os.path.join(GOLDEN, "lz4f_digests.json")))["frames"]
MiB = 1 << 20


def frame(name):
    with open(os.path.join(GOLDEN, "lz4f", name + ".lz4"), "rb") as fh:
        return fh.read()


def check(name, out):
    want = TABLE[name]["oracle_output"]
    assert len(out) == want["len"]
    assert hashlib.sha256(out).hexdigest() == want["sha256"]


def stats():
    s = lz4ada.device_cache_stats()
    return s.device_idle_bytes, s.pinned_idle_bytes, s.idle_streams


def facade_use():
    """One streaming context over indep64k until end of frame, then dropped."""
    data = frame("indep64k")
    ctx, pos, mbs = lz4ada.Decompressor.init_with_header(data)
    buf, out = bytearray(mbs), bytearray()
    while ctx.is_end_of_frame() != lz4ada.EndOfFrame.Yes:
        c, f, l = ctx.update(data, buf, pos)
        assert c > 0 or l >= f
        out += buf[f:l + 1] if l >= f else b""
        pos += c
    assert pos == len(data)
    check("indep64k", bytes(out))
    del ctx


def bulk_uses():
    out, _ = lz4ada.decode_frame(frame("indep64k"))
    assert lz4ada.last_path() == lz4ada.PATH_INDEPENDENT
    check("indep64k", out)
    out, _ = lz4ada.decode_frame(frame("linked256k"))
    assert lz4ada.last_path() & lz4ada.PATH_LINKED
    check("linked256k", out)


def test_release_after_facade_use():
    lz4ada.release_device_cache()
    assert stats() == (0, 0, 0)
    facade_use()
    dev, _, streams = stats()
    assert streams == 1 and dev > 0
    facade_use()  # the second context takes what the first gave back
    dev2, _, streams2 = stats()
    assert streams2 == 1 and dev2 == dev
    lz4ada.release_device_cache()
    assert stats() == (0, 0, 0)


def test_release_after_every_unit_ran():
    facade_use()
    bulk_uses()
    lz4ada.release_device_cache()
    assert stats() == (0, 0, 0)


def test_keep_limit_holds_once_per_kind():
    """A fresh process (the limit is read once) with LZ4ADA_POOL_KEEP_MB=1:
    after all three uses neither kind holds more than the documented 1 MiB."""
    code = ("import sys; sys.path[:0] = %r; import test_gpu_cache as t; "
            "t.facade_use(); t.bulk_uses(); print('STATS', *t.stats())"
            % [os.path.join(ROOT, "tests"), PKG, ROOT])
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, LZ4ADA_POOL_KEEP_MB="1"), cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("STATS ")][-1]
    dev, pin, _ = map(int, line.split()[1:])
    assert 0 <= dev <= MiB and 0 <= pin <= MiB, line
