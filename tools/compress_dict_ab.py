#!/usr/bin/env python3
"""What the dictionary costs and gains lz4ada_compress_frames_device (DESIGN.md
section 18).

Shapes: 65,536 records of 1 KiB, 65,536 of 4 KiB and 1,024 of 64 KiB, of text.
The dictionary is the first 64 KiB of one MiB of pseudo-text, the records are
cut from the rest of it, repeated (a period no record sees twice).  Arm
"plain": lz4ada_compress_frames_device.  Arm "dict":
lz4ada_compress_frames_device_dict with the dictionary and no id.  Arm
"decode": lz4ada_decode_frames_device_dict over the dictionary arm's frames,
compared with the records once.  One process; the arms alternate call by call;
median of --reps after --warmup warm-ups, device events around the synchronous
call.  The last lines time a call of one empty record with and without the
dictionary: no block is compressed, so the difference is the table's memset
and k_compress_dict_table.

    tools/compress_dict_ab.py [--out profiles/compress_dict_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.pop("LZ4ADA_BATCH_BYTES", None)
os.environ.pop("LZ4ADA_BATCH_LINKED", None)

import torch  # noqa: E402

import lz4ada  # noqa: E402
from _compress_cases import pseudo_text  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20
SHAPES = [("65,536 x 1 KiB", 65536, KiB), ("65,536 x 4 KiB", 65536, 4 * KiB), ("1,024 x 64 KiB", 1024, 64 * KiB)]


def arms(data, d, count, size):
    t = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).to("cuda:0")
    dt = torch.frombuffer(bytearray(d), dtype=torch.uint8).to("cuda:0")
    spans = [(i * size, size) for i in range(count)]
    bound = lz4ada.compress_frames_bound([size] * count)
    out = {k: torch.empty(max(bound, 1), dtype=torch.uint8, device="cuda:0") for k in ("plain", "dict")}
    jobs = lz4ada._compress_jobs(spans)
    opt = lz4ada.CompressOptions(4, 0)
    cd = lz4ada.CompressDict(dt.data_ptr(), dt.numel(), 0, 0)
    dd = lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 0)
    olen = {"plain": ctypes.c_int64(), "dict": ctypes.c_int64()}
    dlen = ctypes.c_int64()
    state = {}

    def plain():
        st = lz4ada._lib.lz4ada_compress_frames_device(t.data_ptr() if count * size else None, t.numel() if count * size
                                                       else 0, jobs, count, ctypes.byref(opt), out["plain"].data_ptr(),
                                                       bound, ctypes.byref(olen["plain"]), 0)
        if st:
            raise SystemExit("compress failed: " + lz4ada._thread_error())

    def with_dict():
        st = lz4ada._lib.lz4ada_compress_frames_device_dict(t.data_ptr() if count * size else None, t.numel() if
                                                            count * size else 0, jobs, count, ctypes.byref(opt),
                                                            ctypes.byref(cd), out["dict"].data_ptr(), bound,
                                                            ctypes.byref(olen["dict"]), 0)
        if st:
            raise SystemExit("compress with the dictionary failed: " + lz4ada._thread_error())
        if "djobs" not in state:
            state["where"] = [(jobs[i].out_off, jobs[i].out_len) for i in range(count)]
            state["djobs"] = lz4ada._device_jobs(state["where"])
            state["stored"] = sum(jobs[i].stored_blocks for i in range(count))

    def decode():
        if "back" not in state:
            cap, _ = lz4ada.frames_device_bound(out["dict"].data_ptr(), olen["dict"].value, state["where"], dict=dd)
            state["back"] = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        back = state["back"]
        st = lz4ada._lib.lz4ada_decode_frames_device_dict(out["dict"].data_ptr(), olen["dict"].value, state["djobs"],
                                                          count, 0, ctypes.byref(dd), back.data_ptr(), back.numel(),
                                                          ctypes.byref(dlen), 0)
        if st or dlen.value != len(data):
            raise SystemExit(f"decode failed: {st} {dlen.value} " + lz4ada._thread_error())
        if "checked" not in state:
            state["checked"] = True
            if not torch.equal(back[:dlen.value], t):
                raise SystemExit("the frames do not decode to the records")
    plain.keep = (t, dt, out)
    return plain, with_dict, decode, olen, state


def alternate(calls, reps, warmup):
    times = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_dict_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["lz4ada_compress_frames_device_dict against the plain call, and its frames' decode (tools/compress_dict_ab.py)",
             f"one MI355X, one process, clocks as found; the arms alternate; median of {args.reps} after {args.warmup} "
             "warm-ups (min - max), device events around the synchronous call; text, 64 KiB blocks, no flag, a "
             "65,536-byte dictionary, no id",
             ""]
    text = pseudo_text(MiB, 77)
    d, body = text[:65536], text[65536:]
    for name, count, size in SHAPES:
        total = count * size
        data = (body * (total // len(body) + 1))[:total]
        plain, with_dict, decode, olen, state = arms(data, d, count, size)
        t = alternate({"plain": plain, "dict": with_dict, "decode": decode}, args.reps, args.warmup)
        lines.append(f"{name:15s} {total:>10d} bytes  plain -> {olen['plain'].value:>10d} ({olen['plain'].value / total:.3f}) "
                     f"{t['plain'][0]:8.3f} ms ({t['plain'][1]:.3f} - {t['plain'][2]:.3f}) "
                     f"{total / t['plain'][0] / 1e6:7.2f} GB/s   dict -> {olen['dict'].value:>10d} "
                     f"({olen['dict'].value / total:.3f}, {state['stored']} stored) {t['dict'][0]:8.3f} ms "
                     f"({t['dict'][1]:.3f} - {t['dict'][2]:.3f}) {total / t['dict'][0] / 1e6:7.2f} GB/s   "
                     f"decode {t['decode'][0]:8.3f} ms ({t['decode'][1]:.3f} - {t['decode'][2]:.3f})")
        print(lines[-1], flush=True)
        del plain, with_dict, decode, data
        lz4ada.release_device_cache()
    # one empty record: header and end mark, no block; with the dictionary also the table
    plain, with_dict, _, _, _ = arms(b"", d, 1, 0)
    t = alternate({"plain": plain, "dict": with_dict}, args.reps, args.warmup)
    lines.append(f"one empty record   plain {t['plain'][0]:.3f} ms ({t['plain'][1]:.3f} - {t['plain'][2]:.3f})   "
                 f"dict {t['dict'][0]:.3f} ms ({t['dict'][1]:.3f} - {t['dict'][2]:.3f})   the difference, "
                 f"{1e3 * (t['dict'][0] - t['plain'][0]):.1f} us, is the table's memset and k_compress_dict_table "
                 "over 65,533 positions")
    print(lines[-1], flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
