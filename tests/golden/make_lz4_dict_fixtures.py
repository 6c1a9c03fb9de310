"""Writes tests/golden/lz4f_dict/: LZ4 frames compressed against a dictionary
by the system's liblz4 (LZ4F_compressFrame_usingCDict), the two dictionaries,
and a manifest with every plaintext's length and XXH32.  Run by hand where
liblz4.so.1 is installed; the tests read the files and need no liblz4.

Every frame is checked three ways before it is written: it round-trips through
LZ4F_decompress_usingDict, it fails through LZ4F_decompress without the
dictionary (so it really uses it), and pass 1 of the index decoder will not
decline any of its blocks (block maximum at most 256 KiB, and the payload
under 4 * 16 KiB or at least a quarter of the first 16 KiB's 32-byte
sub-segments holding a sequence start) -- the condition under which the GPU
test may demand LZ4ADA_OK for every fixture.  A fourth check keeps the
fixtures clear of decode_block's one remaining caution: no
match starts before its block with an offset of 65,529 or more.
"""
import ctypes
import json
import os
import random
import struct

import xxhash

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lz4f_dict")
L = ctypes.CDLL("liblz4.so.1")
VERSION = 100
c_size = ctypes.c_size_t


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Prefs(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


L.LZ4F_createCDict.restype = ctypes.c_void_p
L.LZ4F_createCDict.argtypes = [ctypes.c_char_p, c_size]
L.LZ4F_freeCDict.argtypes = [ctypes.c_void_p]
L.LZ4F_createCompressionContext.restype = c_size
L.LZ4F_createCompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
L.LZ4F_freeCompressionContext.argtypes = [ctypes.c_void_p]
L.LZ4F_compressFrameBound.restype = c_size
L.LZ4F_compressFrameBound.argtypes = [c_size, ctypes.POINTER(Prefs)]
L.LZ4F_compressFrame_usingCDict.restype = c_size
L.LZ4F_compressFrame_usingCDict.argtypes = [ctypes.c_void_p, ctypes.c_char_p, c_size, ctypes.c_char_p, c_size,
                                            ctypes.c_void_p, ctypes.POINTER(Prefs)]
L.LZ4F_createDecompressionContext.restype = c_size
L.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
L.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
L.LZ4F_decompress_usingDict.restype = c_size
L.LZ4F_decompress_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(c_size), ctypes.c_char_p,
                                        ctypes.POINTER(c_size), ctypes.c_char_p, c_size, ctypes.c_void_p]
L.LZ4F_decompress.restype = c_size
L.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(c_size), ctypes.c_char_p,
                              ctypes.POINTER(c_size), ctypes.c_void_p]
L.LZ4F_isError.restype = ctypes.c_uint
L.LZ4F_isError.argtypes = [c_size]


def compress(data, dict_bytes, *, linked, content_cksum, block_cksum, content_size, dict_id):
    cdict = L.LZ4F_createCDict(dict_bytes, len(dict_bytes))
    cctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(cctx), VERSION))
    p = Prefs()
    p.frameInfo.blockSizeID = 4  # 64 KiB
    p.frameInfo.blockMode = 0 if linked else 1
    p.frameInfo.contentChecksumFlag = int(content_cksum)
    p.frameInfo.blockChecksumFlag = int(block_cksum)
    p.frameInfo.contentSize = len(data) if content_size else 0
    p.frameInfo.dictID = dict_id or 0
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    n = L.LZ4F_compressFrame_usingCDict(cctx, dst, cap, data, len(data), cdict, ctypes.byref(p))
    assert not L.LZ4F_isError(n)
    L.LZ4F_freeCompressionContext(cctx)
    L.LZ4F_freeCDict(cdict)
    return dst.raw[:n]


def decompress(frame, cap, dict_bytes=None):
    """-> (error?, bytes)"""
    dctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(dctx), VERSION))
    dst = ctypes.create_string_buffer(max(cap, 1))
    out, pos = b"", 0
    err = False
    while pos < len(frame):
        dn, sn = c_size(cap), c_size(len(frame) - pos)
        src = frame[pos:]
        if dict_bytes is None:
            r = L.LZ4F_decompress(dctx, dst, ctypes.byref(dn), src, ctypes.byref(sn), None)
        else:
            r = L.LZ4F_decompress_usingDict(dctx, dst, ctypes.byref(dn), src, ctypes.byref(sn), dict_bytes,
                                            len(dict_bytes), None)
        if L.LZ4F_isError(r):
            err = True
            break
        out += dst.raw[:dn.value]
        pos += sn.value
        if r == 0 or (sn.value == 0 and dn.value == 0):
            break
    L.LZ4F_freeDecompressionContext(dctx)
    return err, out


def sequences(payload):
    """(sequence start, literal count, offset, match length) of a block; the
    last one has offset 0."""
    p, n = 0, len(payload)
    while p < n:
        start = p
        tok = payload[p]
        p += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = payload[p]
                p += 1
                lit += b
                if b != 255:
                    break
        p += lit
        if p >= n:
            yield start, lit, 0, 0
            return
        off = payload[p] | (payload[p + 1] << 8)
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = payload[p]
                p += 1
                ml += b
                if b != 255:
                    break
        yield start, lit, off, ml + 4


def check_blocks(frame):
    """Assertions three and four of the module text, over every block."""
    flg, bd = frame[4], frame[5]
    bmax = 65536 << (2 * (((bd >> 4) & 7) - 4))
    assert bmax <= 256 << 10
    pos = 4 + 2 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0) + 1
    while True:
        word, = struct.unpack_from("<I", frame, pos)
        pos += 4
        if word == 0:
            break
        n = word & 0x7fffffff
        if not word & 0x80000000:
            payload = frame[pos:pos + n]
            seqs = list(sequences(payload))
            if n >= 4 * 16384:
                used = {s // 32 for s, _, _, _ in seqs if s < 16384}
                assert len(used) >= 16384 // 32 // 4
            o = 0
            for _, lit, off, ml in seqs:
                o += lit
                assert not (off >= 65529 and off > o), "a match in quirk D1's offset range before the block"
                o += ml
        pos += n + (4 if flg & 16 else 0)


def vocabulary(rng, n):
    syll = ["ta", "re", "mi", "lo", "ken", "sha", "dor", "vin", "pa", "qu", "est", "ing", "ion", "ar", "ul", "be",
            "co", "di", "fa", "gra", "hy", "ju", "ly", "mo", "ne", "ob", "pre", "sto", "tri", "un", "ver", "wo"]
    return ["".join(rng.choice(syll) for _ in range(rng.randint(1, 4))) for _ in range(n)]


def text(rng, words, n, extra=0.0):
    out = []
    size = 0
    while size < n:
        if rng.random() < extra:
            w = "%d" % rng.randint(0, 10 ** rng.randint(1, 9))
        else:
            # phrases of the dictionary's order now and then, so matches run long
            w = rng.choice(words)
        sep = rng.choice([" ", " ", " ", ", ", ". ", "\n", ": ", "=", "\t"])
        out.append(w + sep)
        size += len(w) + len(sep)
    return "".join(out).encode()[:n]


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20261020)
    words = vocabulary(rng, 1500)
    dicts = {"dict_a": (text(rng, words, 20480), 0x0A0B0C0D), "dict_b": (text(rng, words, 100000), 0x51DEC0DE)}
    for name, (d, _) in dicts.items():
        with open(os.path.join(OUT, name + ".bin"), "wb") as fh:
            fh.write(d)
    frames = []

    def add(data, dname, **kw):
        d, did = dicts[dname]
        with_id = kw.pop("with_id")
        frame = compress(data, d, dict_id=did if with_id else None, **kw)
        err, back = decompress(frame, len(data) + 64, d)
        assert not err and back == data, "round trip"
        err, back = decompress(frame, len(data) + 64, None)
        assert err, "the frame decodes without its dictionary"
        check_blocks(frame)
        name = "f%02d.lz4" % len(frames)
        with open(os.path.join(OUT, name), "wb") as fh:
            fh.write(frame)
        frames.append({"file": name, "dict": dname, "dict_id": did if with_id else None,
                       "linked": not frame[4] & 0x20, "content_checksum": bool(frame[4] & 4),
                       "block_checksum": bool(frame[4] & 16), "content_size": bool(frame[4] & 8),
                       "size": len(data), "xxh32": xxhash.xxh32(data).intdigest(), "frame_len": len(frame)})

    sizes = [200, 256, 333, 512, 777, 1024, 1500, 2048, 3000, 4096, 5000, 6144, 7000, 8192]
    for i in range(40):
        n = sizes[i % len(sizes)] if i < 28 else rng.randint(200, 8192)
        add(text(rng, words, n, extra=0.08), "dict_a" if i % 2 == 0 else "dict_b", linked=bool(i & 1) ^ bool(i & 8),
            content_cksum=bool(i & 2), block_cksum=bool(i & 4), content_size=bool(i % 3 == 0), with_id=bool(i % 5 < 2))
    # two multi-block frames, 64 KiB blocks: linked (4 blocks) and independent (3 and a part)
    add(text(rng, words, 4 * 65536, extra=0.15), "dict_b", linked=True, content_cksum=True, block_cksum=False,
        content_size=True, with_id=True)
    add(text(rng, words, 3 * 65536 + 12345, extra=0.15), "dict_a", linked=False, content_cksum=True, block_cksum=True,
        content_size=False, with_id=False)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump({"dicts": {k: {"file": k + ".bin", "size": len(d), "dict_id": did, "xxh32": xxhash.xxh32(d).intdigest()}
                             for k, (d, did) in dicts.items()}, "frames": frames}, fh, indent=1)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    assert total < 1000000, total
    print(len(frames), "frames,", total, "bytes")


if __name__ == "__main__":
    main()
