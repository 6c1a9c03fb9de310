#!/usr/bin/env python3
"""Device-resident many-frame decode against the host pass it grew from
(DESIGN.md section 11).  For each batch -- the 70 mixed frames of
tests/test_gpu_frames_device.py, 4,096 single-block 64 KiB frames, and one
frame of 4,096 blocks (the case a lane-per-frame walk serves worst) -- the
median of --reps calls after --warmup warm-ups of:

  device   lz4ada_decode_frames_device, device tensor to device tensor, between
           HIP events on the stream (the call is synchronous, so the events
           bracket its host work too);
  host     lz4ada_decode_frames on the same frames in host memory: the parent
           commit's path, with its H2D of the frames and D2H of the bytes;
  index    lz4ada_frames_device_bound (k_frames_walk and its one D2H) and
           lz4ada_frames_index_device_debug (walk, scan, fill and the D2H of the
           descriptors), between HIP events, against lz4ada_stream_index over
           the same frames on the host.

One process; the first failure ends the run.  Writes a table to --out.

    tools/frames_device_ab.py [--out profiles/frames_device_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import lz4ada  # noqa: E402
import lz4frame  # noqa: E402


def parity_batch():
    from conftest import read_vector
    from test_gpu_frames_batch import make_frame
    frames = []
    for i in range(70):
        if i == 10:
            frames.append(read_vector("z100legacy", "lz4"))
        elif i == 20:
            frames.append(struct.pack("<II", 0x184D2A57, 21) + bytes(range(21)))
        else:
            frames.append(make_frame(i, [65536] * 39 + [777] if i == 33 else None)[0])
    return frames


def single_block_frames(n):
    out = []
    for i in range(n):
        comp, raw = lz4ada.gen_block(1, 0x4652 + i, 65536)
        out.append(lz4frame.build_frame([(comp, raw, False)], 64 << 10, content_cksum=True)[0])
    return out


def one_frame_of(nblocks):
    blocks = [(*lz4ada.gen_block(1, 0x4652 + i, 65536), False) for i in range(nblocks)]
    return [lz4frame.build_frame(blocks, 64 << 10, content_cksum=True)[0]]


def median_ms(call, reps, warmup, events):
    times = []
    for r in range(warmup + reps):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        else:
            t0 = time.perf_counter()
            call()
            ms = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            times.append(ms)
    return statistics.median(times), min(times), max(times)


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} - {t[2]:.3f})"


def measure(name, frames, reps, warmup, lines):
    lib = lz4ada._lib
    data = b"".join(frames)
    spans, at = [], 0
    for f in frames:
        spans.append((at, len(f)))
        at += len(f)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans)
    out = torch.empty(max(bound, 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    n = len(frames)
    jobs = lz4ada._device_jobs(spans)
    olen, b64 = ctypes.c_int64(), ctypes.c_int64()

    def device():
        st = lib.lz4ada_decode_frames_device(t.data_ptr(), t.numel(), jobs, n, out.data_ptr(), out.numel(),
                                             ctypes.byref(olen), 0)
        if st or any(jobs[i].status for i in range(n)):
            raise SystemExit(f"{name}: device decode failed: {st} " + lz4ada._thread_error())
    dev = median_ms(device, reps, warmup, True)
    s = lz4ada.last_batch_stats()
    dev_stats = (s.passes, s.frames_batched, s.gpu_hashed, s.host_hashed)
    decoded = olen.value

    hjobs = (lz4ada.FrameJob * n)()
    for j, f in zip(hjobs, frames):
        j.frame, j.len = lz4ada._addr(f), len(f)
    p, hn = ctypes.c_void_p(), ctypes.c_int64()

    def host():
        st = lib.lz4ada_decode_frames(hjobs, n, ctypes.byref(p), ctypes.byref(hn))
        if st or hn.value != decoded:
            raise SystemExit(f"{name}: host decode failed: {st}, {hn.value} bytes")
        lib.lz4ada_buffer_free(p)
    hst = median_ms(host, reps, warmup, False)
    s = lz4ada.last_batch_stats()
    host_stats = (s.passes, s.frames_batched, s.frames_single)

    def walk():
        if lib.lz4ada_frames_device_bound(t.data_ptr(), t.numel(), jobs, n, ctypes.byref(b64), 0):
            raise SystemExit(f"{name}: bound failed: " + lz4ada._thread_error())
    wlk = median_ms(walk, reps, warmup, True)
    _, nblocks, _ = lz4ada.frames_index_device_debug(t.data_ptr(), t.numel(), spans)
    total = sum(nblocks)
    verdict = (ctypes.c_int32 * n)()
    nbl = (ctypes.c_int64 * n)()
    descs = (lz4ada.BlockDesc * max(total, 1))()

    def index():
        if lib.lz4ada_frames_index_device_debug(t.data_ptr(), t.numel(), jobs, n, verdict, nbl, descs, total, 0):
            raise SystemExit(f"{name}: index failed: " + lz4ada._thread_error())
    idx = median_ms(index, reps, warmup, True)
    entries = (lz4ada.StreamEntry * n)()
    cnt = ctypes.c_int64()

    def host_index():
        if lib.lz4ada_stream_index(data, len(data), entries, n, ctypes.byref(cnt)) or cnt.value != n:
            raise SystemExit(f"{name}: stream_index failed")
    hidx = median_ms(host_index, reps, warmup, False)

    lines.append(f"{name}: {n} frames, {total} blocks, {len(data)} compressed -> {decoded} bytes")
    lines.append(f"  device -> device  lz4ada_decode_frames_device   {fmt(dev)} ms   "
                 f"passes {dev_stats[0]}, frames {dev_stats[1]}, hashed gpu {dev_stats[2]} host {dev_stats[3]}")
    lines.append(f"  host -> host      lz4ada_decode_frames          {fmt(hst)} ms   "
                 f"passes {host_stats[0]}, batched {host_stats[1]}, single {host_stats[2]}")
    lines.append(f"  index, device     walk + D2H of the records     {fmt(wlk)} ms")
    lines.append(f"                    walk + scan + fill + D2H descs{fmt(idx)} ms")
    lines.append(f"  index, host       lz4ada_stream_index           {fmt(hidx)} ms")
    lines.append(f"  device / host decode: {hst[0] / dev[0]:.2f}x")
    lines.append("")
    print("\n".join(lines[-8:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_device_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["Many frames, device memory to device memory, against the host pass "
             "(tools/frames_device_ab.py)",
             f"one MI355X, one process, clocks as found; median of {args.reps} after {args.warmup} "
             "warm-ups (min - max)", ""]
    measure("parity batch", parity_batch(), args.reps, args.warmup, lines)
    measure("4,096 x 64 KiB", single_block_frames(4096), args.reps, args.warmup, lines)
    measure("1 frame x 4,096 blocks", one_frame_of(4096), args.reps, args.warmup, lines)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
