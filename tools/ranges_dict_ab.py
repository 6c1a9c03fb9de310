#!/usr/bin/env python3
"""Records fetched by position from dictionary frames: the seek index built
with a dictionary against the loop a caller wrote before it (DESIGN.md section
19).  65,536 records of 1 KiB and of 4 KiB, slices of one pseudo-text, written
by lz4ada_compress_frames_device_dict against a dictionary of 65,536 bytes and
one of 4,096 bytes cut from the same text, in device memory.  Between HIP
events around the synchronous calls, the arms alternating call by call in one
process, the median of --reps after --warmup warm-ups:

  A  1,024 and 16,384 randomly chosen whole records through
     lz4ada_decode_ranges_device on an index from lz4ada_seek_index_build_dict;
  B  the same records through lz4ada_decode_frames_device_dict over just
     their frames' spans (LZ4ADA_FRAMES_EXACT): the call needs no index, so it
     walks and sizes the chosen frames every time;
  C  all records whole through lz4ada_decode_frames_device_dict.

  build  lz4ada_seek_index_build_dict + lz4ada_seek_index_free, reported apart
         with the index's device bytes: a reader pays it once per set of frames.

A's bytes are compared with B's, and both with the records, before anything is
timed.

    tools/ranges_dict_ab.py [--out profiles/ranges_dict_ab.txt] [--records 65536]
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
from _compress_cases import pseudo_text  # noqa: E402

TEXT = 2 << 20
PICKS = (1024, 16384)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranges_dict_ab.txt"))
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lib = lz4ada._lib
    n = args.records
    text = torch.frombuffer(bytearray(pseudo_text(TEXT, 0x1919)), dtype=torch.uint8).to("cuda:0")
    olen = ctypes.c_int64()
    lines = ["Whole records by position from dictionary frames: the seek index against decoding just their frames "
             "(tools/ranges_dict_ab.py)",
             f"one MI355X, one process, clocks as found; HIP events around the synchronous calls, the arms "
             f"alternating; median of {args.reps} after {args.warmup} warm-ups (min - max)", ""]
    print("\n".join(lines), flush=True)
    for rec in (1024, 4096):
        rng = random.Random(rec)
        offs = torch.tensor([65536 + rng.randrange(TEXT - 65536 - rec) for _ in range(n)], dtype=torch.int64,
                            device="cuda:0")
        records = text[offs[:, None] + torch.arange(rec, device="cuda:0")[None, :]].contiguous().view(-1)
        rspans = [(i * rec, rec) for i in range(n)]
        for dl in (65536, 4096):
            d = text[65536 - dl:65536].clone()
            frames, spans = lz4ada.compress_frames_tensor(records, rspans, dict=d)
            frames = frames.clone()
            dd = lz4ada.DeviceDict(d.data_ptr(), dl, 0, 0)
            gap = (dl + 32 + 255) // 256 * 256
            idx = lz4ada.SeekIndex.build_tensor(frames, spans, dict=d)
            bad = [i for i in range(n) if idx.jobs[i].status or idx.jobs[i].out_len != rec]
            if bad:
                raise SystemExit(f"the build refused record {bad[0]}")
            part = [f"{n} records of {rec} bytes, dictionary of {dl} bytes (a gap of {gap}): {frames.numel()} "
                    f"compressed -> {n * rec} bytes",
                    f"  index {idx.device_bytes} device bytes, {100.0 * idx.device_bytes / (n * rec):.2f} % of the "
                    f"decoded size"]

            def build():
                lz4ada.SeekIndex.build(frames.data_ptr(), frames.numel(), spans, dict=d.data_ptr(), dict_len=dl).free()

            all_jobs = lz4ada._device_jobs(spans)
            all_out = torch.empty(n * rec, dtype=torch.uint8, device="cuda:0")
            passes = {}

            def whole():
                st = lib.lz4ada_decode_frames_device_dict(frames.data_ptr(), frames.numel(), all_jobs, n,
                                                          lz4ada.FRAMES_EXACT, ctypes.byref(dd), all_out.data_ptr(),
                                                          all_out.numel(), ctypes.byref(olen), 0)
                if st or olen.value != n * rec:
                    raise SystemExit(f"C failed: {st} " + lz4ada._thread_error())
                passes.setdefault("C", lz4ada.last_batch_stats().passes)

            whole()
            if not torch.equal(all_out, records):
                raise SystemExit("C delivers other bytes than the records")
            arms = {"build": build, "C": whole}
            for np_ in PICKS:
                pick = sorted(rng.sample(range(n), min(np_, n)))
                want = len(pick) * rec
                ranges, nr = lz4ada._frame_ranges([(i, 0, rec) for i in pick])
                jobs = lz4ada._device_jobs([spans[i] for i in pick])
                out_a = torch.zeros(want, dtype=torch.uint8, device="cuda:0")
                out_b = torch.zeros(want, dtype=torch.uint8, device="cuda:0")

                def arm_a(ranges=ranges, nr=nr, out=out_a, want=want, key=f"A {np_}"):
                    st = lib.lz4ada_decode_ranges_device(idx._ptr, frames.data_ptr(), frames.numel(), ranges, nr,
                                                         out.data_ptr(), out.numel(), ctypes.byref(olen), 0)
                    if st or olen.value != want:
                        raise SystemExit(f"{key} failed: {st} " + lz4ada._thread_error())
                    passes.setdefault(key, lz4ada.last_batch_stats().passes)

                def arm_b(jobs=jobs, nj=len(pick), out=out_b, want=want, key=f"B {np_}"):
                    st = lib.lz4ada_decode_frames_device_dict(frames.data_ptr(), frames.numel(), jobs, nj,
                                                              lz4ada.FRAMES_EXACT, ctypes.byref(dd), out.data_ptr(),
                                                              out.numel(), ctypes.byref(olen), 0)
                    if st or olen.value != want:
                        raise SystemExit(f"{key} failed: {st} " + lz4ada._thread_error())
                    passes.setdefault(key, lz4ada.last_batch_stats().passes)

                arm_a(), arm_b()
                ref = records.view(n, rec)[torch.tensor(pick, device="cuda:0")].reshape(-1)
                if any(ranges[i].status for i in range(nr)) or not torch.equal(out_a, ref):
                    raise SystemExit(f"A {np_}: the index delivers other bytes than the records")
                if any(jobs[i].status for i in range(len(pick))) or not torch.equal(out_b, ref):
                    raise SystemExit(f"B {np_}: the frames decode to other bytes than the records")
                arms[f"A {np_}"], arms[f"B {np_}"] = arm_a, arm_b
            r = alternate(arms, args.reps, args.warmup)
            part.append(f"  build  lz4ada_seek_index_build_dict + free          {fmt(r['build'])} ms")
            for np_ in PICKS:
                a, b = r[f"A {np_}"], r[f"B {np_}"]
                part.append(f"  A  {np_:6} records through the index             {fmt(a)} ms   passes "
                            f"{passes[f'A {np_}']}   gaps filled {np_ * gap} bytes")
                part.append(f"  B  {np_:6} records' frames, decode_frames_dict   {fmt(b)} ms   passes "
                            f"{passes[f'B {np_}']}   B / A {b[0] / a[0]:.2f}")
            part.append(f"  C  all {n} records, decode_frames_dict          {fmt(r['C'])} ms   passes {passes['C']}")
            part.append("")
            lines += part
            print("\n".join(part), flush=True)
            idx.free()
            del all_out, frames
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
