#!/usr/bin/env python3
"""Where G lies: k_xxh32_spans over 64 equal spans side by
side against the host chain (host_xxh32_update, one core) over the same
64 x size bytes, for sizes 4 KiB ... 16 MiB in powers of two.  G is the
largest size at which the kernel is not slower.  Prints a table and one
JSON line; needs the GPU (kernel time between device events, host time on
the wall clock, median of --reps after one warm-up each)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bo-lz4-ada_amd"))

import lz4ada  # noqa: E402
import torch  # noqa: E402
import xxhash  # noqa: E402

SPANS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-size", type=int, default=16 << 20)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x4C5A)
    d_buf = torch.randint(0, 256, (SPANS * args.max_size,), dtype=torch.uint8, device="cuda:0",
                          generator=gen)
    h_buf = d_buf.cpu().numpy()
    torch.cuda.synchronize()
    rows, g = [], 0
    size = 4096
    print(f"{'size':>10} {'kernel ms':>10} {'host ms':>10} {'kernel GB/s':>12} {'host GB/s':>10}")
    while size <= args.max_size:
        spans = [(i * size, size) for i in range(SPANS)]
        kms = []
        for r in range(args.reps + 1):
            got, ms = lz4ada.xxh32_spans_device(d_buf.data_ptr(), spans)
            if r:
                kms.append(ms)
        assert got[0] == xxhash.xxh32(h_buf[:size].tobytes()).intdigest()
        assert got[-1] == xxhash.xxh32(h_buf[(SPANS - 1) * size:SPANS * size].tobytes()).intdigest()
        hms = []
        for r in range(args.reps + 1):
            st = lz4ada.XXH32State()
            lz4ada._lib.lz4ada_xxh32_reset(ctypes.byref(st), 0)
            t0 = time.perf_counter()
            lz4ada._lib.lz4ada_xxh32_update(ctypes.byref(st), h_buf.ctypes.data, SPANS * size)
            t1 = time.perf_counter()
            if r:
                hms.append((t1 - t0) * 1e3)
        k, h = statistics.median(kms), statistics.median(hms)
        gb = SPANS * size / 1e6
        print(f"{size:>10} {k:>10.3f} {h:>10.3f} {gb / k:>12.2f} {gb / h:>10.2f}")
        rows.append({"size": size, "kernel_ms": round(k, 4), "host_ms": round(h, 4)})
        if k <= h:
            g = size
        size *= 2
    print(json.dumps({"spans": SPANS, "rows": rows, "G": g}))


if __name__ == "__main__":
    main()
