#!/usr/bin/env python3
"""Linked frames in a many-frame pass against the path they took before
(DESIGN.md section 12): the cap sweep behind lz4ada_batch_linked_max() and
one headline row.

Sweep: linked frames of 1, 2, 4, 8, 16, 32 and 64 full 64 KiB blocks (kind
GEN_MIXED_NOD1, content checksum), a pass of 2 such frames and a pass of 256,
through lz4ada_decode_frames_opt with LZ4ADA_FRAMES_LINKED ("pass") and with
flags 0 ("single": every frame on its own, what the call did before the flag
existed).  The two arms alternate call by call in one process; median of
--reps after --warmup warm-ups, host clock around the synchronous call.  The
cap the file supports is the largest frame size at which the pass of 2 is no
slower than the single path, within 10 % plus the row's own run-to-run spread
((max - min) / median of the single arm).

Headline: 1,024 linked frames of 4 x 64 KiB, host to host (the two arms above)
and device to device: lz4ada_decode_frames_device_opt with the flag, against
the call without it followed by what its caller then has to do -- every frame
comes back LZ4ADA_EXACT_PATH, so the frames are fetched to the host, decoded
by lz4ada_decode_frames and the bytes sent back to the device.

--unique frames are generated per size and repeated to fill a pass.  The
first call of every arm is compared with the generator's plaintext.

    tools/frames_linked_ab.py [--out profiles/frames_linked_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

# every size of the sweep is within the cap while it is being measured
os.environ["LZ4ADA_BATCH_LINKED_MAX"] = str(1 << 40)
os.environ.pop("LZ4ADA_BATCH_LINKED", None)

import torch  # noqa: E402

import lz4ada  # noqa: E402
import lz4frame  # noqa: E402

BLOCK = 64 << 10


def linked_frames(nblocks, unique, count):
    """count linked frames of nblocks full blocks (unique distinct ones, repeated)
    -> [(frame, plaintext)]"""
    made = []
    for u in range(min(unique, count)):
        blocks = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 0x4C4B + 1000 * nblocks + 97 * u, BLOCK, nblocks)
        made.append(lz4frame.build_frame([(c, r, False) for c, r in blocks], BLOCK, indep=False,
                                         content_cksum=True))
    return [made[i % len(made)] for i in range(count)]


def alternate(arms, reps, warmup, events=False):
    """arms: {name: call}.  The calls alternate; -> {name: (median, min, max)} in ms."""
    times = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, call in arms.items():
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
                times[k].append(ms)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def fmt(t):
    return f"{t[0]:10.3f} ({t[1]:.3f} - {t[2]:.3f})"


def host_arms(items, name):
    """The two host-to-host arms over the frames -> ({arm: call}, check)."""
    lib = lz4ada._lib
    n = len(items)
    want = b"".join(raw for _, raw in items)
    jobs = (lz4ada.FrameJob * n)()
    for j, (f, _) in zip(jobs, items):
        j.frame, j.len = lz4ada._addr(f), len(f)
    p, hn = ctypes.c_void_p(), ctypes.c_int64()
    seen = {}

    def run(flags, arm):
        st = lib.lz4ada_decode_frames_opt(jobs, n, flags, ctypes.byref(p), ctypes.byref(hn))
        if st or hn.value != len(want) or any(jobs[i].status for i in range(n)):
            raise SystemExit(f"{name} {arm}: decode failed: {st} " + lz4ada._thread_error())
        if arm not in seen:  # the first call: the bytes, and the path the arm claims
            if ctypes.string_at(p, hn.value) != want:
                raise SystemExit(f"{name} {arm}: wrong bytes")
            s = lz4ada.last_batch_stats()
            seen[arm] = (s.passes, s.frames_batched, s.frames_single)
            if (arm == "pass") != (s.frames_batched == n):
                raise SystemExit(f"{name} {arm}: {s.frames_batched} of {n} frames batched")
        lib.lz4ada_buffer_free(p)
    return {"pass": lambda: run(lz4ada.FRAMES_LINKED, "pass"), "single": lambda: run(0, "single")}, seen


def sweep_row(nblocks, count, args, lines):
    items = linked_frames(nblocks, args.unique, count)
    arms, _ = host_arms(items, f"{nblocks} blocks x {count}")
    t = alternate(arms, args.reps, args.warmup)
    spread = (t["single"][2] - t["single"][1]) / t["single"][0]
    ok = t["pass"][0] <= t["single"][0] * (1.10 + spread)
    lines.append(f"{nblocks:3d} x 64 KiB  {count:4d} frames   pass {fmt(t['pass'])} ms   single {fmt(t['single'])} ms   "
                 f"single / pass {t['single'][0] / t['pass'][0]:6.2f}x   spread {100 * spread:5.1f} %   "
                 f"{'no slower' if ok else 'SLOWER'}")
    print(lines[-1], flush=True)
    return ok


def headline(args, lines):
    count, nblocks = 1024, 4
    items = linked_frames(nblocks, args.unique, count)
    name = f"{count} linked frames of {nblocks} x 64 KiB"
    arms, _ = host_arms(items, name)
    h = alternate(arms, args.reps, args.warmup)
    lines.append(f"{name}: {sum(len(f) for f, _ in items)} compressed -> {sum(len(r) for _, r in items)} bytes")
    lines.append(f"  host -> host      with the flag     {fmt(h['pass'])} ms")
    lines.append(f"                    without           {fmt(h['single'])} ms   "
                 f"without / with {h['single'][0] / h['pass'][0]:.2f}x")
    print("\n".join(lines[-3:]), flush=True)

    lib = lz4ada._lib
    data = b"".join(f for f, _ in items)
    want = b"".join(r for _, r in items)
    spans, at = [], 0
    for f, _ in items:
        spans.append((at, len(f)))
        at += len(f)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    out = torch.empty(len(want) + 4096, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    jobs = lz4ada._device_jobs(spans)
    olen = ctypes.c_int64()
    p, hn = ctypes.c_void_p(), ctypes.c_int64()
    fjobs = (lz4ada.FrameJob * count)()
    checked = set()

    def with_flag():
        st = lib.lz4ada_decode_frames_device_opt(t.data_ptr(), t.numel(), jobs, count, lz4ada.FRAMES_LINKED,
                                                 out.data_ptr(), out.numel(), ctypes.byref(olen), 0)
        if st or olen.value != len(want) or any(jobs[i].status for i in range(count)):
            raise SystemExit(f"{name}: device decode failed: {st} " + lz4ada._thread_error())
        if "with" not in checked:
            checked.add("with")
            if out[:olen.value].cpu().numpy().tobytes() != want:
                raise SystemExit(f"{name}: device decode: wrong bytes")

    def without():
        st = lib.lz4ada_decode_frames_device_opt(t.data_ptr(), t.numel(), jobs, count, 0, out.data_ptr(),
                                                 out.numel(), ctypes.byref(olen), 0)
        if st or not all(jobs[i].status == lz4ada.EXACT_PATH for i in range(count)):
            raise SystemExit(f"{name}: the call without the flag took a linked frame")
        # what the caller then does: the frames to the host, decoded there, the bytes back
        host = t.cpu().numpy().tobytes()
        for j, (off, n) in zip(fjobs, spans):
            j.frame, j.len = lz4ada._addr(host, off), n
        st = lib.lz4ada_decode_frames_opt(fjobs, count, 0, ctypes.byref(p), ctypes.byref(hn))
        if st or hn.value != len(want):
            raise SystemExit(f"{name}: host decode failed: {st}")
        back = torch.frombuffer(bytearray(ctypes.string_at(p, hn.value)), dtype=torch.uint8)
        out[:hn.value].copy_(back)
        torch.cuda.synchronize()
        lib.lz4ada_buffer_free(p)
        if "without" not in checked:
            checked.add("without")
            if out[:hn.value].cpu().numpy().tobytes() != want:
                raise SystemExit(f"{name}: fallback: wrong bytes")

    d = alternate({"with": with_flag, "without": without}, args.reps, args.warmup, events=True)
    lines.append(f"  device -> device  with the flag     {fmt(d['with'])} ms")
    lines.append(f"                    without           {fmt(d['without'])} ms   "
                 f"without / with {d['without'][0] / d['with'][0]:.2f}x   "
                 "(the refusing call, the frames to the host, lz4ada_decode_frames, the bytes back)")
    print("\n".join(lines[-2:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_linked_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--no-headline", action="store_true")
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["Linked frames in a many-frame pass against the single-frame path (tools/frames_linked_ab.py)",
             f"one MI355X, one process, clocks as found; the arms alternate; median of {args.reps} after "
             f"{args.warmup} warm-ups (min - max); {args.unique} distinct frames per size, repeated",
             "pass: lz4ada_decode_frames_opt with LZ4ADA_FRAMES_LINKED; single: flags 0 (every frame on its own)",
             ""]
    best = 0
    still = True
    for nb in args.sizes:
        ok2 = sweep_row(nb, 2, args, lines)
        sweep_row(nb, 256, args, lines)
        still = still and ok2
        if still:
            best = nb
    lines.append("")
    lines.append(f"largest size at which the pass of 2 is no slower (10 % over the row's spread), every smaller "
                 f"size too: {best} x 64 KiB = {best * BLOCK} slot bytes")
    lines.append("")
    print(lines[-2], flush=True)
    if not args.no_headline:
        headline(args, lines)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
