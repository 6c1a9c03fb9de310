#!/usr/bin/env python3
"""What a dictionary costs a many-frame device pass.

Arm A: frames whose blocks were generated with a 64 KiB dictionary as history,
through lz4ada_decode_frames_device_dict.  Arm B: the same shapes generated
without history, through lz4ada_decode_frames_device_opt, which the same
binary takes through code that is byte-identical to the parent's
(profiles/frames_dict_code_hash.txt).  The ratio A / B is the price of the
gaps and their fill -- a 64 KiB write per gapped block -- and of the
dictionary decoders' launch shape.

Shapes: 1,024 independent single-block frames decoding to 4 KiB and to 64 KiB,
and 1,024 linked frames of 4 x 64 KiB.  One process; the arms alternate call
by call; median of --reps after --warmup warm-ups, device events around the
synchronous call.  --unique frames are generated per shape and repeated.  The
first call of every arm is compared with the generator's plaintext.

    tools/frames_dict_ab.py [--out profiles/frames_dict_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.pop("LZ4ADA_BATCH_LINKED", None)
os.environ.pop("LZ4ADA_BATCH_BYTES", None)

import torch  # noqa: E402

import lz4ada  # noqa: E402
import lz4frame  # noqa: E402

BLOCK = 64 << 10
NOD1 = lz4ada.GEN_MIXED_NOD1


def dictionary(n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"iota", b"kappa"]
    out, x = bytearray(), 12345
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7fffffff
        out += words[(x >> 16) % len(words)] + bytes([32 + (x >> 8) % 90])
    return bytes(out[:n])


def frames(lens, linked, hist, unique, count):
    """count frames of blocks decoding to lens (unique distinct ones, repeated) -> [(frame, plaintext)]"""
    made = []
    for u in range(min(unique, count)):
        seed = 0xD1C7 + 131 * u + len(lens)
        if linked:
            blocks = lz4ada.gen_linked_blocks(NOD1, seed, 0, 0, lens=list(lens), hist=hist)
        else:
            blocks = [lz4ada.gen_linked_blocks(NOD1, seed + 7 * k, 0, 0, lens=[n], hist=hist)[0]
                      for k, n in enumerate(lens)]
        made.append(lz4frame.build_frame([(c, r, False) for c, r in blocks], BLOCK, indep=not linked,
                                         content_cksum=True))
    return [made[i % len(made)] for i in range(count)]


def arm(items, dd, name):
    """-> the call of one arm over the frames (dd: a DeviceDict, or None for the _opt call)."""
    lib = lz4ada._lib
    count = len(items)
    data = b"".join(f for f, _ in items)
    want = b"".join(r for _, r in items)
    spans, at = [], 0
    for f, _ in items:
        spans.append((at, len(f)))
        at += len(f)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, 0, True)  # the slot capacities
    out = torch.empty(bound + 4096, dtype=torch.uint8, device="cuda:0")
    jobs = lz4ada._device_jobs(spans)
    olen = ctypes.c_int64()
    checked = []

    def call():
        if dd is None:
            st = lib.lz4ada_decode_frames_device_opt(t.data_ptr(), t.numel(), jobs, count, lz4ada.FRAMES_LINKED,
                                                     out.data_ptr(), out.numel(), ctypes.byref(olen), 0)
        else:
            st = lib.lz4ada_decode_frames_device_dict(t.data_ptr(), t.numel(), jobs, count, lz4ada.FRAMES_LINKED,
                                                      ctypes.byref(dd), out.data_ptr(), out.numel(),
                                                      ctypes.byref(olen), 0)
        if st or olen.value != len(want) or any(jobs[i].status for i in range(count)):
            raise SystemExit(f"{name}: decode failed: {st} " + lz4ada._thread_error())
        if not checked:
            checked.append(lz4ada.last_batch_stats().passes)
            if out[:olen.value].cpu().numpy().tobytes() != want:
                raise SystemExit(f"{name}: wrong bytes")
    call.keep = (t, out)
    call.bytes = (len(data), len(want))
    call.passes = checked
    return call


def alternate(arms, reps, warmup):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_dict_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--count", type=int, default=1024)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    d = dictionary(BLOCK)
    dt = torch.frombuffer(bytearray(d), dtype=torch.uint8).to("cuda:0")
    dd = lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 0)
    lines = ["A dictionary in a many-frame device pass against the same shapes without one (tools/frames_dict_ab.py)",
             f"one MI355X, one process, clocks as found; the arms alternate; median of {args.reps} after "
             f"{args.warmup} warm-ups (min - max), device events; {args.unique} distinct frames per shape, repeated",
             "A: lz4ada_decode_frames_device_dict, a 64 KiB dictionary (a gap of 65,792 bytes per gapped block)",
             "B: lz4ada_decode_frames_device_opt, the same shapes generated without history; both LZ4ADA_FRAMES_LINKED",
             ""]
    for name, lens, linked in (("independent, 1 x 4 KiB", [4096], False), ("independent, 1 x 64 KiB", [BLOCK], False),
                               ("linked, 4 x 64 KiB", [BLOCK] * 4, True)):
        a = arm(frames(lens, linked, d, args.unique, args.count), dd, name + " A")
        b = arm(frames(lens, linked, b"", args.unique, args.count), None, name + " B")
        t = alternate({"A": a, "B": b}, args.reps, args.warmup)
        spread = (t["B"][2] - t["B"][1]) / t["B"][0]
        lines.append(f"{args.count} frames {name:24s} A {fmt(t['A'])} ms  {a.passes[0]} pass(es)   "
                     f"B {fmt(t['B'])} ms  {b.passes[0]} pass(es)   A / B {t['A'][0] / t['B'][0]:5.2f}x   "
                     f"B's spread {100 * spread:4.1f} %   ({a.bytes[0]} -> {a.bytes[1]} bytes)")
        print(lines[-1], flush=True)
        del a, b
        lz4ada.release_device_cache()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
