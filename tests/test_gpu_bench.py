"""bench.py on the GPU at a toy size (5 x 64 KiB blocks, 3 unique): a plain
run times exactly --steps steps and does nothing beside the headline;
--dump-outputs writes what the last step produced, checked here against the
CPU oracle's decode of the same blocks; --full adds the golden check and the
rows that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import xxhash

from conftest import ROOT

import _oracle as O
import bench
import lz4ada
import lz4frame

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--blocks", "5", "--unique", "3", "--block-max", "65536"]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *argv],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    r = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert r["unit"] == "MiB/s" and r["dtype"] == "u8" and r["higher_is_better"] is True
    # value and ms_per_step are the same K steps (ms_per_step is rounded to 1 us, a step here
    # takes tens of us: a few percent)
    assert r["value"] == pytest.approx(5 * 65536 / (1 << 20) / (r["ms_per_step"] * 1e-3), rel=0.1)
    # nothing beside the headline
    assert r["cpu_baseline"] is None and r["roofline"]["alone_ms"] is None
    assert not {"e2e_content_checksum", "c3_one_gpu", "classes", "linked_c5", "c2_64k", "facade",
                "cpu_baseline_parallel"} & set(r)
    # the same blocks through the CPU oracle
    blocks = [lz4ada.gen_block(lz4ada.GEN_KINDS["mixed"], bench.SEED0 + i % 3, 65536) for i in range(5)]
    frame, _ = lz4frame.build_frame([(c, raw, False) for c, raw in blocks], 65536, block_cksum=True)
    st, want, _, msg = O.decode_stream(frame)
    assert st == O.OK, msg
    status = np.load(tmp_path / "status.npy")
    assert status.dtype == np.float64 and status.shape == (5, 3)
    assert status[:, 0].tolist() == [0] * 5
    assert status[:, 1].tolist() == [len(raw) for _, raw in blocks] and sum(status[:, 1]) == len(want)
    assert status[:, 2].tolist() == [xxhash.xxh32(c).intdigest() for c, _ in blocks]
    sample = np.load(tmp_path / "output_sample.npy")
    assert sample.dtype == np.float32
    assert sample.astype(np.uint8).tobytes() == want  # 320 KiB: every decoded byte is in the dump
    pos, n = 0, []
    for _, raw in blocks:
        n.append(xxhash.xxh32(want[pos:pos + len(raw)]).intdigest())
        pos += len(raw)
    digests = np.load(tmp_path / "output_xxh32.npy")
    assert digests.dtype == np.float64 and digests.tolist() == n


def test_full_run_keeps_the_other_rows():
    r = _bench("--steps", "2", "--warmup", "1", "--full", "--no-c3", "--no-linked", "--no-64k",
               "--no-facade", "--no-cpu-baseline", "--classes=rle", "--real=")
    assert r["steps"] == 2 and set(r["roofline"]["alone_ms"]) == {"block_checksums", "decode"}
    assert r["e2e_content_checksum"]["content_xxh32_s"] > 0
    assert r["classes"]["rle"]["blocks"] == 5 and r["cpu_baseline"] is None
