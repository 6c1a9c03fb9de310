"""Writes tests/golden/compress_linked_sizes.json: the payload bytes of five
records as frames of linked blocks -- what this library's
serial statement gives linked and unlinked, and what liblz4 makes of the same
blocks linked: one stream per record, LZ4_compress_fast_continue at
acceleration 1 over the record's blocks where they lie, each block decoded back
through LZ4_decompress_safe_usingDict against the 64 KiB in front of it.  The
records are those of tests/_compress_linked_cases.size_rows.  The yardstick of
the ratio check in tests/test_compress_linked_host_cpu.py is liblz4's recorded
sizes, not this library.  Needs the system liblz4 and the built library; the
tests need only the latter.  Run from anywhere:
python tests/golden/make_compress_linked_sizes.py"""
import ctypes
import ctypes.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")]

import lz4ada  # noqa: E402
from _compress_dict_cases import dict_frame_blocks  # noqa: E402
from _compress_linked_cases import size_rows  # noqa: E402


def payload(frame):
    return sum(len(b[1]) for b in dict_frame_blocks(frame)[4])


def main():
    lz4 = ctypes.CDLL(ctypes.util.find_library("lz4"))
    lz4.LZ4_createStream.restype = ctypes.c_void_p
    lz4.LZ4_freeStream.argtypes = [ctypes.c_void_p]
    lz4.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int]
    lz4.LZ4_decompress_safe_usingDict.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_int]
    rows = []
    for name, rec, blen in size_rows():
        src = ctypes.create_string_buffer(rec, len(rec))  # the blocks where they lie, contiguous
        base = ctypes.addressof(src)
        cap = lz4.LZ4_compressBound(blen)
        dst, back = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(blen)
        stream = lz4.LZ4_createStream()
        sizes = []
        for at in range(0, len(rec), blen):
            n = min(blen, len(rec) - at)
            c = lz4.LZ4_compress_fast_continue(stream, base + at, dst, n, cap, 1)
            assert c > 0
            hist = min(at, 65536)
            got = lz4.LZ4_decompress_safe_usingDict(dst, back, c, n, base + at - hist, hist)
            assert got == n and back.raw[:n] == rec[at:at + n]
            sizes.append(min(c, n))  # a frame stores a block that does not shrink
        lz4.LZ4_freeStream(stream)
        row = {"name": name, "record": len(rec), "block": blen,
               "linked": payload(lz4ada.compress_frame_host(rec, block=blen, linked=True)),
               "independent": payload(lz4ada.compress_frame_host(rec, block=blen)), "liblz4_linked": sizes}
        rows.append(row)
        print(name, row["independent"], row["linked"], sum(sizes))
    doc = {"liblz4_version": lz4.LZ4_versionNumber(),
           "function": "LZ4_compress_fast_continue over a record's blocks, acceleration 1", "rows": rows}
    with open(os.path.join(HERE, "compress_linked_sizes.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
