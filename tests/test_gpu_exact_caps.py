"""Every block decoder pinned to its output extent ("Why exact
caps are safe for the decoders as they stand"): the blocks of _capblocks.py,
whose sizes sit around the 16-byte piece, the 32-byte ring piece and the slot
rounding, through each decoder with descriptors written here -- out_cap equal
to the decoded size, a little over it, and under it.  The output buffer starts
as a sentinel, every block is followed by a guard of 256 bytes and more that
belongs to nobody, and after the launch every byte outside the blocks'
[out_off, out_off + out_cap) must still be the sentinel; each case runs with
two sentinels, so a stray store of the sentinel's own value shows in one of
them.  The stride between blocks does not depend on the cap and the buffer
starts 64 KiB and more before the first block: a decoder that ignored its cap
or its block start altogether would still stay inside the allocation.  Blocks
with rewritten offsets (the size rule does not judge offsets, so they are the
corrupt blocks that reach a decoder with an exact cap) are held to the
oracle's verdict and bytes."""
import bisect
import ctypes

import numpy as np
import pytest
import torch

import _capblocks as C
import lz4ada
import lz4frame
import test_gpu_frames_linked as L
from test_gpu_lone import oracle_block

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
LEAD = 65536 + 256   # sentinel before the first block: further than any offset reaches
GUARD = 256          # behind every block's round256(size), whatever its cap
TAIL = 4096
SLACK = (1, 15, 16, 17, 255)
SHORT = (1, 15, 16, 17, "half", "zero")
MODES = ["exact"] + [f"slack{s}" for s in SLACK] + [f"short_{d}" for d in SHORT]
DECLINES = (lz4ada.DS_RETRY, lz4ada.DS_SPARSE)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def cap_of(mode, size):
    if mode == "exact":
        return size
    if mode.startswith("slack"):
        return size + int(mode[5:])
    d = mode[6:]
    return 0 if d == "zero" else size - (size // 2 if d == "half" else min(int(d), size))


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def to_device(b):
    return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to("cuda:0")


class Laid:
    """Input bytes on the device, where each block's payload lies in them
    (in_off rising, as the index table needs) and the output layout: out_off
    256-aligned, a stride of round256(size) + GUARD whatever the cap is; a
    block in `joined` (a full block inside a linked frame) has its successor
    directly behind it."""

    def __init__(self, data, src, sizes, joined=()):
        """src: [(in_off, in_len, flags)] per block; sizes: the decoded sizes."""
        self.data, self.src, self.sizes, self.n = data, src, sizes, len(src)
        assert all(a[0] < b[0] for a, b in zip(src, src[1:]))
        self.d_in = to_device(data)
        self.offs, at = [], LEAD
        for b, size in enumerate(sizes):
            self.offs.append(at)
            at += size if b in joined else C.round256(size) + GUARD
            assert at % 256 == 0
        self.total = at + TAIL

    @classmethod
    def of_blocks(cls, items):
        """items: [(payload, decoded size, stored)], independent blocks: one frame of them."""
        frame, _ = lz4frame.build_frame([(p, b"", st) for p, _, st in items], C.BMAX)
        info, descs = lz4ada.frame_index(frame)
        assert info.nblocks == len(items)
        src = [(d.in_off, d.in_len, d.flags) for d in descs[:len(items)]]
        assert [s[1] for s in src] == [len(p) for p, _, _ in items]
        return cls(frame, src, [size for _, size, _ in items])

    def descs(self, caps):
        arr = (lz4ada.BlockDesc * self.n)(*[lz4ada.BlockDesc(i, n, f, o, c, 0)
                                            for (i, n, f), o, c in zip(self.src, self.offs, caps)])
        return to_device(bytes(arr))

    def owned(self, caps):
        m = np.zeros(self.total, dtype=bool)
        for o, c in zip(self.offs, caps):
            m[o:o + c] = True
        return torch.from_numpy(m).to("cuda:0")


def check_outside(d_out, owned, fill, offs, caps, names, decoder):
    """Every byte outside the blocks' [out_off, out_off + out_cap) is the fill."""
    bad = (d_out != fill) & ~owned
    if bool(bad.any()):
        at = int(bad.nonzero()[0])
        k = max(bisect.bisect_right(offs, at) - 1, 0)
        pytest.fail(f"{decoder}: block {k} ({names[k]}, out_cap {caps[k]}): a stray byte "
                    f"{at - (offs[k] + caps[k]):+d} from the block's end, fill {fill:#x}")


def statuses(d_st, n):
    return (lz4ada.BlockStatus * n).from_buffer_copy(d_st.cpu().numpy().tobytes())


# ------------------------------------------------------------ the bulk decoders

BULK = {
    "pc": lz4ada.DECODE_PC,
    "idx1_alone": lz4ada.DECODE_IDX1_ALONE,
    "pp2_alone": lz4ada.DECODE_PP2_ALONE,
    "idx_split": lz4ada.DECODE_IDX_SPLIT,
    "idx_sparse": lz4ada.DECODE_IDX_SPARSE,
    "idx_chain": lz4ada.DECODE_IDX,
    "blocks_device": None,  # launch_decode_checked: the passes' own entry, with its fused mode
}
ALONE = ("pc", "idx1_alone", "pp2_alone", "idx_split")
WHOLE = ("idx_chain", "blocks_device")


def launch_bulk(decoder, laid, d_desc, d_out, d_st):
    if BULK[decoder] is None:
        lz4ada.decode_blocks_device(laid.d_in.data_ptr(), len(laid.data), d_desc.data_ptr(), laid.n,
                                    d_out.data_ptr(), d_st.data_ptr(), cur_stream())
    else:
        lz4ada.launch_decode_variant(laid.d_in.data_ptr(), len(laid.data), d_desc.data_ptr(), laid.n,
                                     d_out.data_ptr(), d_st.data_ptr(), BULK[decoder], cur_stream())
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world():
    """(blocks, their layout, per mode the caps, the device descriptors and the
    owned mask).  Never modified."""
    blocks = C.cap_blocks()
    laid = Laid.of_blocks([(b.payload, b.size, b.stored) for b in blocks])
    modes = {}
    for mode in MODES:
        caps = [cap_of(mode, b.size) for b in blocks]
        assert all(0 <= c < C.round256(s) + GUARD for c, s in zip(caps, laid.sizes))
        modes[mode] = (caps, laid.descs(caps), laid.owned(caps))
    return tuple(blocks), laid, modes


@pytest.mark.parametrize("decoder", list(BULK))
def test_bulk_decoder_stays_inside_its_caps(world, decoder):
    blocks, laid, modes = world
    names = [b.name for b in blocks]
    declined = {}
    for mode in MODES:
        caps, d_desc, owned = modes[mode]
        for fill in FILLS:
            d_out = torch.full((laid.total,), fill, dtype=torch.uint8, device="cuda:0")
            d_st = torch.zeros(laid.n * 32, dtype=torch.uint8, device="cuda:0")
            launch_bulk(decoder, laid, d_desc, d_out, d_st)
            check_outside(d_out, owned, fill, laid.offs, caps, names, f"{decoder} {mode}")
            st = statuses(d_st, laid.n)
            host = d_out.cpu().numpy()
            for k, b in enumerate(blocks):
                code, where = st[k].code, (decoder, mode, hex(fill), b.name, st[k].code)
                if caps[k] < b.size:
                    assert code != 0, where
                    continue
                if decoder in WHOLE or (decoder == "idx_sparse" and b.cls.startswith("sparse")):
                    assert code == 0, where
                assert code == 0 or code in DECLINES, where
                if code == 0:
                    assert st[k].out_len == b.size, where
                    assert host[laid.offs[k]:laid.offs[k] + b.size].tobytes() == b.want, where
            if mode == "exact" and fill == FILLS[0]:
                declined = {b.name: st[k].code for k, b in enumerate(blocks) if st[k].code != 0}
    if decoder in ALONE:
        # not vacuous: under exact caps every residue has a dense, mixed or chain block the variant took
        took = {b.size % 256 for b in blocks if b.cls in ("dense", "mixed", "chain") and b.name not in declined}
        assert took >= set(C.RESIDUES), (decoder, sorted(set(C.RESIDUES) - took))
    if decoder == "idx1_alone":  # pass 1 does hand the two crafted classes to k_decode_sparse
        for cls in ("sparse_ratio", "sparse_density"):
            assert any(declined.get(b.name) == lz4ada.DS_SPARSE for b in blocks if b.cls == cls), cls
    by_cls = {}
    for name in declined:
        cls = next(b.cls for b in blocks if b.name == name)
        by_cls[cls] = by_cls.get(cls, 0) + 1
    print(f"exact caps, {decoder}: declined {len(declined)} of {len(blocks)} blocks {by_cls}")


# ------------------------------------------------------------ rewritten offsets

@pytest.fixture(scope="module")
def rewritten():
    """(blocks, layout, per block the oracle's (accepted, bytes), descriptors
    with exact caps, the owned mask)."""
    blocks = C.rewritten_blocks()
    sizes = [lz4ada.block_size_host(w.payload) for w in blocks]
    laid = Laid.of_blocks([(w.payload, n, False) for w, n in zip(blocks, sizes)])
    verdicts = [oracle_block(w.payload, C.BMAX) for w in blocks]
    assert sum(1 for ok, _ in verdicts if not ok) >= 10
    assert sum(1 for (ok, got), w in zip(verdicts, blocks) if ok and got != oracle_block(w.original, C.BMAX)[1]) >= 10
    return tuple(blocks), laid, verdicts, sizes, laid.descs(sizes), laid.owned(sizes)


@pytest.mark.parametrize("decoder", ["idx_chain", "blocks_device", "pc", "idx1_alone", "pp2_alone"])
def test_rewritten_offsets_under_exact_caps(rewritten, decoder):
    blocks, laid, verdicts, sizes, d_desc, owned = rewritten
    names = [w.name for w in blocks]
    for fill in FILLS:
        d_out = torch.full((laid.total,), fill, dtype=torch.uint8, device="cuda:0")
        d_st = torch.zeros(laid.n * 32, dtype=torch.uint8, device="cuda:0")
        launch_bulk(decoder, laid, d_desc, d_out, d_st)
        check_outside(d_out, owned, fill, laid.offs, sizes, names, f"{decoder} rewritten")
        st = statuses(d_st, laid.n)
        host = d_out.cpu().numpy()
        for k, w in enumerate(blocks):
            ok, want = verdicts[k]
            where = (decoder, hex(fill), w.name, w.fields, st[k].code)
            if st[k].code == 0:
                assert ok and st[k].out_len == len(want), where
                assert host[laid.offs[k]:laid.offs[k] + len(want)].tobytes() == want, where
            if decoder in WHOLE:
                assert (st[k].code == 0) == ok, where


# ----------------------------------------------------------- the lone-block decoder

LONE_SIZES = [base + r for base in (65536, 300000) for r in C.SPARSE_RESIDUES]


@pytest.mark.parametrize("kind", ["mixed", "literal"])
def test_lone_decoder_stays_inside_its_cap(kind):
    for size in LONE_SIZES:
        comp, raw = lz4ada.gen_block(lz4ada.GEN_KINDS[kind], 0xCA9 + size, size)
        d_in = to_device(comp + b"\0" * 16)
        total = LEAD + C.round256(size) + GUARD + TAIL
        for mode in MODES:
            cap = cap_of(mode, size)
            owned = torch.zeros(total, dtype=torch.bool, device="cuda:0")
            owned[LEAD:LEAD + cap] = True
            sb = lz4ada.lone_scratch_bytes(len(comp), cap)
            d_sc = torch.empty(sb, dtype=torch.uint8, device="cuda:0")
            for fill in FILLS:
                where = (kind, size, mode, hex(fill))
                d_out = torch.full((total,), fill, dtype=torch.uint8, device="cuda:0")
                d_st = torch.zeros(ctypes.sizeof(lz4ada.BlockStatus), dtype=torch.uint8, device="cuda:0")
                args = (d_in.data_ptr(), len(comp), d_out.data_ptr() + LEAD, cap, d_st.data_ptr(),
                        d_sc.data_ptr(), sb, cur_stream())
                if cap == 0:  # the launcher refuses a block without room
                    with pytest.raises(lz4ada.LZ4AdaError):
                        lz4ada.launch_decode_lone(*args)
                else:
                    lz4ada.launch_decode_lone(*args)
                torch.cuda.synchronize()
                check_outside(d_out, owned, fill, [LEAD], [cap], [f"{kind}_{size}"], f"lone {mode}")
                st = statuses(d_st, 1)[0]
                if cap == 0:
                    continue
                if cap < size:
                    assert st.code == lz4ada.DS_RETRY, where
                else:
                    assert (st.code, st.out_len) == (0, size), where
                    assert d_out[LEAD:LEAD + size].cpu().numpy().tobytes() == raw, where


# ------------------------------------------------- linked frames, one wave per frame

def frames_world():
    """Linked frames of [65536, n] and [65536, 65536, n], n over the residues
    (256 for the residue 0): (frames, the oracle's bytes, block lengths)."""
    frames, raws, lens_of = [], [], []
    for k, full in enumerate((1, 2)):
        for r in C.RESIDUES:
            lens = [65536] * full + [r or 256]
            frame, raw = L.linked_frame(lens, seed=500 + 16 * k + r)
            assert L.oracle_alone(frame) == raw
            frames.append(frame)
            raws.append(raw)
            lens_of.append(lens)
    return frames, raws, lens_of


def test_frames_decoder_stays_inside_its_caps():
    """k_index + k_decode_idx_frames, called as test_kernel_chain calls it: a
    frame's blocks back to back, the cap mode on its last block, the guard and
    then the next frame's first slot behind it."""
    frames, raws, lens_of = frames_world()
    data, src, first, sizes = b"", [], [0], []
    for f, lens in zip(frames, lens_of):
        info, ds = lz4ada.frame_index(f)
        assert info.nblocks == len(lens)
        src += [(len(data) + d.in_off, d.in_len, d.flags) for d in ds[:info.nblocks]]
        sizes += lens
        first.append(len(src))
        data += f
    last = {b - 1 for b in first[1:]}
    laid = Laid(data, src, sizes, joined=set(range(len(src))) - last)
    offs, nb = laid.offs, laid.n
    names = [f"frame {i} block {b - first[i]}" for i in range(len(frames)) for b in range(first[i], first[i + 1])]
    for mode in MODES:
        caps = [cap_of(mode, n) if b in last else n for b, n in enumerate(sizes)]
        d_desc, owned = laid.descs(caps), laid.owned(caps)
        for fill in FILLS:
            d_out = torch.full((laid.total,), fill, dtype=torch.uint8, device="cuda:0")
            d_st = torch.zeros(nb * 32, dtype=torch.uint8, device="cuda:0")
            lz4ada.decode_idx_frames_debug(laid.d_in.data_ptr(), len(data), d_desc.data_ptr(), nb, first,
                                           [True] * len(frames), d_out.data_ptr(), d_st.data_ptr())
            torch.cuda.synchronize()
            check_outside(d_out, owned, fill, offs, caps, names, f"idx_frames {mode}")
            st = statuses(d_st, nb)
            host = d_out.cpu().numpy()
            for i, raw in enumerate(raws):
                pos = 0
                for b in range(first[i], first[i + 1]):
                    where = (mode, hex(fill), names[b], st[b].code)
                    if caps[b] < sizes[b]:
                        assert st[b].code != 0, where
                        continue
                    assert (st[b].code, st[b].out_len) == (0, sizes[b]), where
                    assert host[offs[b]:offs[b] + sizes[b]].tobytes() == raw[pos:pos + sizes[b]], where
                    pos += sizes[b]
