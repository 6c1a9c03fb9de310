"""Writes tests/golden/compress_sizes.json: what liblz4's LZ4_compress_default
makes of every 64 KiB, 4 KiB and 1 KiB block of the seeded pseudo-text that
tests/test_compress_host_cpu.py compresses for its ratio check (the first
16 x 64 KiB, 64 x 4 KiB and 64 x 1 KiB of it).  The yardstick of that check is
these recorded sizes, not this library.  Needs the system liblz4; the tests do
not.  Run from anywhere: python tests/golden/make_compress_sizes.py"""
import ctypes
import ctypes.util
import json
import os

SEED = 2024
SHAPES = [(64 * 1024, 16), (4 * 1024, 64), (1024, 64)]


def pseudo_text(n, seed):
    s = [(seed * 2654435761 + 1) & 0xFFFFFFFF or 1]
    def r(k):
        x = s[0]; x ^= (x << 13) & 0xFFFFFFFF; x ^= x >> 17; x ^= (x << 5) & 0xFFFFFFFF; s[0] = x; return x % k
    abc = "etaoinshrdlucmfwypvbgkqjxz"
    vocab = ["".join(abc[min(r(26), r(26))] for _ in range(2 + r(9))) for _ in range(600)]
    out, size = [], 0
    while size < n:
        out.append(vocab[min(r(600), r(600), r(600))] + (" ", " ", " ", " ", ", ", ". ", "\n")[r(7)])
        size += len(out[-1])
    return "".join(out).encode()[:n]


def main():
    lz4 = ctypes.CDLL(ctypes.util.find_library("lz4"))
    text = pseudo_text(SHAPES[0][0] * SHAPES[0][1], SEED)
    sizes = {}
    for block, count in SHAPES:
        cap = lz4.LZ4_compressBound(block)
        dst = ctypes.create_string_buffer(cap)
        sizes[str(block)] = [lz4.LZ4_compress_default(text[i * block:(i + 1) * block], dst, block, cap)
                             for i in range(count)]
        assert min(sizes[str(block)]) > 0
    doc = {"seed": SEED, "liblz4_version": lz4.LZ4_versionNumber(), "function": "LZ4_compress_default",
           "sizes": sizes}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "compress_sizes.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print({k: sum(v) for k, v in sizes.items()})


if __name__ == "__main__":
    main()
