#!/usr/bin/env python3
"""Times streams of many small frames through decode_stream and, where the
library has it, decode_frames: for each shape (frames x bytes per frame,
gen_block kind 1, C.Checksum) the median of --reps C calls after --warmup
warm-ups.  One JSON line on stdout.

Every (shape, leg) runs in a fresh child process under its own timeout; the
first child that fails or times out ends the run (nothing more is started on
the GPU after it).  The script uses only what the library has had since the
bulk entries exist, so it runs unchanged on a commit without decode_frames
and then reports that leg as null.  --pkg names another build of the
package directory (lz4ada.py and its library) for an A/B in one place.

    tools/frames_batch_time.py [--pkg DIR] [--shapes 2x65536,256x65536,...]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "2x65536,256x65536,4096x65536,65536x4096"


def build(pkg, nframes, size):
    sys.path.insert(0, pkg)
    import lz4ada
    import lz4frame
    frames = []
    for i in range(nframes):
        comp, raw = lz4ada.gen_block(1, 0x4652 + i, size)
        frames.append(lz4frame.build_frame([(comp, raw, False)], 64 << 10, content_cksum=True)[0])
    return lz4ada, frames


def child(args):
    nframes, size = args.shape
    lz4ada, frames = build(args.pkg, nframes, size)
    lib = lz4ada._lib
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    if args.leg == "stream":
        data = b"".join(frames)

        def call():
            return lib.lz4ada_decode_stream_alloc(data, len(data), ctypes.byref(p), ctypes.byref(n))
    else:
        if not hasattr(lz4ada, "FrameJob"):
            print(json.dumps({"ms": None, "note": "no lz4ada_decode_frames in this library"}))
            return
        jobs = (lz4ada.FrameJob * nframes)()
        for j, f in zip(jobs, frames):
            j.frame = lz4ada._addr(f)
            j.len = len(f)

        def call():
            return lib.lz4ada_decode_frames(jobs, nframes, ctypes.byref(p), ctypes.byref(n))
    times = []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        st = call()  # synchronous: the bytes are in host memory when it returns
        t1 = time.perf_counter()
        if st != 0 or n.value != nframes * size:
            raise SystemExit(f"decode failed: status {st}, {n.value} bytes: " + lz4ada._thread_error())
        lib.lz4ada_buffer_free(p)
        if r >= args.warmup:
            times.append((t1 - t0) * 1e3)
    res = {"ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3),
           "max_ms": round(max(times), 3), "reps": len(times), "path": lz4ada.last_path()}
    if hasattr(lz4ada, "last_batch_stats"):
        s = lz4ada.last_batch_stats()
        res["passes"], res["batched"], res["single"] = s.passes, s.frames_batched, s.frames_single
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "bo-lz4-ada_amd"))
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--legs", default="stream,frames")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", type=lambda s: tuple(int(x) for x in s.split("x")))
    ap.add_argument("--leg")
    args = ap.parse_args()
    args.pkg = os.path.abspath(args.pkg)
    if args.child:
        return child(args)
    out = {"pkg": os.path.relpath(args.pkg, ROOT), "reps": args.reps, "warmup": args.warmup, "shapes": {}}
    for shape in args.shapes.split(","):
        row = out["shapes"].setdefault(shape, {})
        for leg in args.legs.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pkg", args.pkg,
                   "--shape", shape, "--leg", leg, "--reps", str(args.reps), "--warmup", str(args.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                row[leg] = {"error": f"timed out after {args.timeout} s"}
                out["stopped"] = f"{shape} {leg}"
                print(json.dumps(out))
                return 1
            if r.returncode != 0:
                row[leg] = {"error": (r.stderr or r.stdout).strip()[-400:], "exit": r.returncode}
                out["stopped"] = f"{shape} {leg}"
                print(json.dumps(out))
                return 1
            row[leg] = json.loads(r.stdout.strip().splitlines()[-1])
            print(shape, leg, json.dumps(row[leg]), file=sys.stderr, flush=True)  # progress
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
