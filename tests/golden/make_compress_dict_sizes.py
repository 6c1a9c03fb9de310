"""Writes tests/golden/compress_dict_sizes.json: what liblz4 makes of small
text records against a shared dictionary -- LZ4_loadDict, then
LZ4_compress_fast_continue at acceleration 1, a fresh stream per record, each
block decoded back through LZ4_decompress_safe_usingDict -- for the six rows
of tests/test_compress_dict_host_cpu.py's ratio check.  The
text is pseudo_text(65536 + record * count, seed); the dictionary is the last
`dict` bytes of its first 65,536, the records are the pieces that follow.  The
yardstick of that check is these recorded sizes, not this library.  Needs the
system liblz4; the tests do not.  Run from anywhere:
python tests/golden/make_compress_dict_sizes.py"""
import ctypes
import ctypes.util
import json
import os

SEED = 7
ROWS = [(65536, 256, 64), (65536, 1024, 64), (65536, 4096, 64), (65536, 65536, 4), (4096, 1024, 64),
        (1000, 1024, 64)]  # (dictionary bytes, record bytes, records)


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
    lz4.LZ4_createStream.restype = ctypes.c_void_p
    lz4.LZ4_freeStream.argtypes = [ctypes.c_void_p]
    lz4.LZ4_loadDict.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lz4.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int]
    lz4.LZ4_decompress_safe_usingDict.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_char_p, ctypes.c_int]
    rows = []
    for dl, rl, cnt in ROWS:
        text = pseudo_text(65536 + rl * cnt, SEED)
        d = text[:65536][-dl:]
        cap = lz4.LZ4_compressBound(rl)
        dst, back = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(rl)
        sizes = []
        for i in range(cnt):
            rec = text[65536 + i * rl:65536 + (i + 1) * rl]
            stream = lz4.LZ4_createStream()
            assert lz4.LZ4_loadDict(stream, d, dl) == dl
            n = lz4.LZ4_compress_fast_continue(stream, rec, dst, rl, cap, 1)
            lz4.LZ4_freeStream(stream)
            assert n > 0
            assert lz4.LZ4_decompress_safe_usingDict(dst, back, n, rl, d, dl) == rl and back.raw == rec
            sizes.append(n)
        rows.append({"dict": dl, "record": rl, "count": cnt, "sizes": sizes})
        print(dl, rl, cnt, sum(sizes))
    doc = {"seed": SEED, "liblz4_version": lz4.LZ4_versionNumber(),
           "function": "LZ4_loadDict + LZ4_compress_fast_continue, acceleration 1", "rows": rows}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "compress_dict_sizes.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
