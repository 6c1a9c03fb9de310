#!/usr/bin/env python3
"""Ranged decode of linked frames through history checkpoints against decoding
the whole frames and slicing.  1,024 linked frames of
32 x 64 KiB mixed blocks with block checksums (16 distinct ones, repeated) in
device memory.  Between HIP events around the synchronous calls, the arms
alternating call by call in one process, the median of --reps after --warmup
warm-ups:

  A  4 KiB from the last block of every frame;
  B  4 KiB from block 0 of every frame;
  C  one whole frame per range.

  ranged    lz4ada_decode_ranges_device through an index built with
            LZ4ADA_SEEK_LINKED and a checkpoint every 64 KiB, 256 KiB, 1 MiB,
            or none (a spacing no frame reaches: every chain starts at block 0);
  baseline  lz4ada_decode_frames_device_opt with LZ4ADA_FRAMES_LINKED |
            LZ4ADA_FRAMES_EXACT over the whole frames into a buffer of their
            total, then the ranges' bytes picked out on the device by one torch
            gather over an index tensor built beforehand (C: no gather, the
            frames' bytes are the ranges');
  build     lz4ada_seek_index_build_opt + lz4ada_seek_index_free per spacing,
            reported apart with the index's device bytes: a reader pays it
            once per set of frames.

Every ranged arm's bytes are compared with the baseline's before anything is
timed.

    tools/ranges_linked_ab.py [--out profiles/ranges_linked_ab.txt] [--frames 1024]
"""
import argparse
import ctypes
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import lz4ada  # noqa: E402
import lz4frame  # noqa: E402

BLOCK = 65536
NBLOCKS = 32
DISTINCT = 16
SPACINGS = (("64 KiB", 64 << 10), ("256 KiB", 256 << 10), ("1 MiB", 1 << 20), ("none", 1 << 40))


def alternate(arms, reps, warmup):
    """arms: {name: call}.  The calls alternate; -> {name: (median, min, max)} in ms."""
    times = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, call in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} - {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranges_linked_ab.txt"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lib = lz4ada._lib
    n = args.frames
    distinct = []
    for k in range(DISTINCT):
        blocks = [(c, r, False) for c, r in
                  lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 0x7100 + k, 0, 0, lens=[BLOCK] * NBLOCKS)]
        distinct.append(lz4frame.build_frame(blocks, 64 << 10, indep=False, block_cksum=True)[0])
    spans, at = [], 0
    for i in range(n):
        spans.append((at, len(distinct[i % DISTINCT])))
        at += spans[-1][1]
    t = torch.cat([torch.frombuffer(bytearray(f), dtype=torch.uint8) for f in distinct] * (n // DISTINCT) +
                  [torch.frombuffer(bytearray(distinct[i % DISTINCT]), dtype=torch.uint8)
                   for i in range(n - n % DISTINCT, n)]).to("cuda:0")
    assert t.numel() == at
    size = NBLOCKS * BLOCK
    total = n * size
    jobs = lz4ada._device_jobs(spans)
    olen = ctypes.c_int64()
    dec = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    flags = lz4ada.FRAMES_LINKED | lz4ada.FRAMES_EXACT

    def decode_whole():
        st = lib.lz4ada_decode_frames_device_opt(t.data_ptr(), t.numel(), jobs, n, flags, dec.data_ptr(), dec.numel(),
                                                 ctypes.byref(olen), 0)
        if st or olen.value != total or any(jobs[i].status for i in range(n)):
            raise SystemExit(f"whole decode failed: {st} " + lz4ada._thread_error())

    lines = ["Ranged decode of linked frames through history checkpoints against the whole frames decoded and sliced "
             "(tools/ranges_linked_ab.py)",
             f"one MI355X, one process, clocks as found; HIP events around the synchronous calls, the arms "
             f"alternating; median of {args.reps} after {args.warmup} warm-ups (min - max)",
             f"{n} linked frames of {NBLOCKS} x 64 KiB mixed blocks ({DISTINCT} distinct), block checksums: "
             f"{t.numel()} compressed -> {total} bytes", ""]
    indexes = {}
    for name, cb in SPACINGS:
        indexes[name] = lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=cb)
        bad = [i for i in range(n) if indexes[name].jobs[i].status]
        if bad:
            raise SystemExit(f"the build with a checkpoint every {name} refused frame {bad[0]}")
    builds = {name: (lambda cb=cb: lz4ada.SeekIndex.build(t.data_ptr(), t.numel(), spans, linked=True,
                                                          checkpoint_bytes=cb).free()) for name, cb in SPACINGS}
    rb = alternate(builds, args.reps, args.warmup)
    lines.append("build  lz4ada_seek_index_build_opt(LZ4ADA_SEEK_LINKED) + lz4ada_seek_index_free")
    for name, _ in SPACINGS:
        b = indexes[name].device_bytes
        lines.append(f"  checkpoint every {name:<8} {fmt(rb[name])} ms   index {b} device bytes, "
                     f"{100.0 * b / total:.2f} % of the decoded size")
    lines.append("")
    print("\n".join(lines), flush=True)

    rng = random.Random(0x5242)
    arms = (("A  4 KiB from the last block of every frame",
             [(i, (NBLOCKS - 1) * BLOCK + rng.randrange(BLOCK - 4096), 4096) for i in range(n)], False),
            ("B  4 KiB from block 0 of every frame", [(i, rng.randrange(BLOCK - 4096), 4096) for i in range(n)], False),
            ("C  one whole frame per range", [(i, 0, size) for i in range(n)], True))
    for title, ranges, whole in arms:
        want = sum(r[2] for r in ranges)
        out = torch.empty(want, dtype=torch.uint8, device="cuda:0")
        arr, nr = lz4ada._frame_ranges(ranges)
        passes = {}
        decode_whole()
        base = [jobs[i].out_off for i in range(n)]
        pick = None
        if not whole:
            pick = torch.cat([torch.arange(base[j] + off, base[j] + off + ln, dtype=torch.int64)
                              for j, off, ln in ranges]).to("cuda:0")
        elif base != [i * size for i in range(n)]:
            raise SystemExit("the whole decode does not lay the frames back to back")

        def baseline():
            decode_whole()
            return dec if whole else dec[pick]

        def ranged(name):
            st = lib.lz4ada_decode_ranges_device(indexes[name]._ptr, t.data_ptr(), t.numel(), arr, nr, out.data_ptr(),
                                                 out.numel(), ctypes.byref(olen), 0)
            if st or olen.value != want or any(arr[i].status for i in range(nr)):
                raise SystemExit(f"{title}: ranged decode ({name}) failed: {st} " + lz4ada._thread_error())
            passes.setdefault(name, lz4ada.last_batch_stats().passes)

        ref = baseline()
        for name, _ in SPACINGS:  # bytes first
            out.zero_()
            ranged(name)
            if not torch.equal(ref, out):
                raise SystemExit(f"{title}: the index with a checkpoint every {name} delivers other bytes")
        calls = {"baseline": baseline}
        calls.update({name: (lambda name=name: ranged(name)) for name, _ in SPACINGS})
        r = alternate(calls, args.reps, args.warmup)
        part = [f"{title}: {nr} ranges, {want} bytes wanted",
                f"  baseline  whole frames, LINKED | EXACT" + ("          " if whole else ", + gather") +
                f"  {fmt(r['baseline'])} ms"]
        for name, _ in SPACINGS:
            part.append(f"  ranged    checkpoint every {name:<8}            {fmt(r[name])} ms   passes {passes[name]}   "
                        f"baseline / ranged {r['baseline'][0] / r[name][0]:.2f}")
        part.append("")
        lines += part
        print("\n".join(part), flush=True)
        del out, pick, ref
    for idx in indexes.values():
        idx.free()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
