#!/usr/bin/env python3
"""What lz4ada_compress_frames_device costs.

Shapes: 1,024 records of 64 KiB, 65,536 records of 4 KiB and one record of
256 MiB (64 KiB blocks throughout), each of text, random bytes and zeros.
Arm "compress": the device call.  Arm "decode": this library's own
decode_frames_device over the frames it produced, the read side's cost for the
same bytes.  One process; the two arms alternate call by call; median of --reps
after --warmup warm-ups, device events around the synchronous call.  The first
call's frames are decoded and compared with the records.

Yardstick: LZ4F_compressFrame (independent 64 KiB blocks, level 0) through the
system liblz4 on this machine's CPU with 1 and 16 threads, wall clock, median
of three -- where ctypes finds the library; the line says so when it does not.

    tools/compress_ab.py [--out profiles/compress_ab.txt]
    tools/compress_ab.py --profile      # the compress arm alone, three calls per text
                                        # shape: for a rocprofv3 --kernel-trace --stats run
"""
import argparse
import ctypes
import ctypes.util
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.pop("LZ4ADA_BATCH_BYTES", None)
os.environ.pop("LZ4ADA_BATCH_LINKED", None)

import torch  # noqa: E402

import lz4ada  # noqa: E402
from _compress_cases import pseudo_text  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20
SHAPES = [("1,024 x 64 KiB", 1024, 64 * KiB), ("65,536 x 4 KiB", 65536, 4 * KiB), ("1 x 256 MiB", 1, 256 * MiB)]


def payload(kind, total):
    """total bytes on the host: text (one MiB of pseudo-text repeated: a period
    no 64 KiB block sees twice), random bytes, zeros."""
    if kind == "text":
        return (pseudo_text(MiB, 77) * (total // MiB + 1))[:total]
    if kind == "random":
        return torch.randint(0, 256, (total,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)) \
            .numpy().tobytes()
    return bytes(total)


class Prefs(ctypes.Structure):  # LZ4F_preferences_t (lz4frame.h 1.9)
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int), ("compressionLevel", ctypes.c_int),
                ("autoFlush", ctypes.c_uint), ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def host_yardstick(data, count, size, threads):
    """Seconds for LZ4F_compressFrame over the records with `threads` threads
    (ctypes releases the GIL), median of three; None without liblz4."""
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    lz4 = ctypes.CDLL(name)
    lz4.LZ4F_compressFrame.restype = ctypes.c_size_t
    lz4.LZ4F_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]
    lz4.LZ4F_compressFrameBound.restype = ctypes.c_size_t
    lz4.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    prefs = Prefs(blockSizeID=4, blockMode=1)
    src = ctypes.create_string_buffer(data, len(data))
    base = ctypes.addressof(src)
    if count == 1:  # one record: the threads share its 64 KiB blocks as frames of their own
        count, size = len(data) // (4 * MiB), 4 * MiB
    cap = lz4.LZ4F_compressFrameBound(size, ctypes.byref(prefs))
    outs = [ctypes.create_string_buffer(cap) for _ in range(threads)]

    def work(k):
        for i in range(k, count, threads):
            lz4.LZ4F_compressFrame(outs[k], cap, base + i * size, size, ctypes.byref(prefs))

    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        th = [threading.Thread(target=work, args=(k,)) for k in range(threads)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def arms(data, count, size, block_id=4):
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    spans = [(i * size, size) for i in range(count)]
    bound = lz4ada.compress_frames_bound([size] * count, block_id)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
    jobs = lz4ada._compress_jobs(spans)
    opt = lz4ada.CompressOptions(block_id, 0)
    olen, dlen = ctypes.c_int64(), ctypes.c_int64()
    state = {}

    def compress():
        st = lz4ada._lib.lz4ada_compress_frames_device(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                       out.data_ptr(), bound, ctypes.byref(olen), 0)
        if st:
            raise SystemExit("compress failed: " + lz4ada._thread_error())
        if "djobs" not in state:
            state["where"] = [(jobs[i].out_off, jobs[i].out_len) for i in range(count)]
            state["djobs"] = lz4ada._device_jobs(state["where"])
            state["stored"] = sum(jobs[i].stored_blocks for i in range(count))

    def decode():
        if "back" not in state:  # the slot capacities: 64 KiB per block, whatever the record's length
            cap, _ = lz4ada.frames_device_bound(out.data_ptr(), olen.value, state["where"])
            state["back"] = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        back = state["back"]
        st = lz4ada._lib.lz4ada_decode_frames_device(out.data_ptr(), olen.value, state["djobs"], count,
                                                     back.data_ptr(), back.numel(), ctypes.byref(dlen), 0)
        if st or dlen.value != len(data):
            raise SystemExit(f"decode failed: {st} {dlen.value} " + lz4ada._thread_error())
        if "checked" not in state:
            state["checked"] = True
            if not torch.equal(back[:dlen.value], t):
                raise SystemExit("the frames do not decode to the records")
    compress.keep = (t, out)
    return compress, decode, olen, state


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the liblz4 yardstick")
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    if args.profile:
        for name, count, size in SHAPES:
            compress, _, olen, _ = arms(payload("text", count * size), count, size)
            for _ in range(3):
                compress()
            print(f"{name}: {count * size} -> {olen.value} bytes", flush=True)
            lz4ada.release_device_cache()
        return 0
    lines = ["lz4ada_compress_frames_device against its own read side and against liblz4 on the CPU (tools/compress_ab.py)",
             f"one MI355X, one process, clocks as found; compress and decode alternate; median of {args.reps} after "
             f"{args.warmup} warm-ups (min - max), device events around the synchronous call; 64 KiB blocks, no flag",
             "host: LZ4F_compressFrame (independent 64 KiB blocks) of the system liblz4 on the GPU machine's CPU, wall "
             "clock, median of 3, 1 and 16 threads (the 256 MiB record as 64 frames of 4 MiB there)",
             ""]
    for kind in ("text", "random", "zeros"):
        for name, count, size in SHAPES:
            data = payload(kind, count * size)
            compress, decode, olen, state = arms(data, count, size)
            t = alternate({"compress": compress, "decode": decode}, args.reps, args.warmup)
            host = [None, None] if args.no_host else [host_yardstick(data, count, size, n) for n in (1, 16)]
            gbs = len(data) / t["compress"][0] / 1e6
            hs = "  ".join("liblz4 x%d %s" % (n, "not on this machine" if h is None else
                                               f"{1e3 * h:9.1f} ms {len(data) / h / 1e9:6.2f} GB/s")
                           for n, h in zip((1, 16), host))
            lines.append(f"{kind:6s} {name:15s} {len(data):>10d} -> {olen.value:>10d} bytes ({olen.value / len(data):.3f}, "
                         f"{state['stored']} stored)  compress {t['compress'][0]:9.3f} ms ({t['compress'][1]:.3f} - "
                         f"{t['compress'][2]:.3f}) {gbs:7.2f} GB/s   decode {t['decode'][0]:8.3f} ms "
                         f"({t['decode'][1]:.3f} - {t['decode'][2]:.3f})   {hs}")
            print(lines[-1], flush=True)
            del compress, decode, data
            lz4ada.release_device_cache()
    # what a 4 MiB block costs: one wave's serial work (the read side takes such frames one at a time: no decode arm)
    for count in (16, 256):
        data = payload("text", count * 4 * MiB)
        compress, _, olen, state = arms(data, count, 4 * MiB, 7)
        t = alternate({"compress": compress}, 3, 1)["compress"]
        lines.append(f"text   {count:3d} x 4 MiB, one 4 MiB block each (id 7)  {len(data)} -> {olen.value} bytes  compress "
                     f"{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f}) {len(data) / t[0] / 1e6:7.2f} GB/s  (median of 3 after 1)")
        print(lines[-1], flush=True)
        del compress, data
        lz4ada.release_device_cache()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
