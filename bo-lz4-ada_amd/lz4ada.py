"""lz4ada -- Python host binding of the MI355X-native LZ4Ada decompressor.

Mirrors the reference's public Ada package (lib/lz4ada.ads) over the C-ABI
in include/lz4ada_hip.h, loaded with ctypes from the in-tree
bo-lz4-ada_amd/liblz4ada_hip.so:

    LZ4Ada.Init / Init_With_Header / Init_For_Block   -> Decompressor.init*
    LZ4Ada.Update / Is_End_Of_Frame                   -> Decompressor.update / is_end_of_frame
    LZ4Ada.XXHash32.Init/Reset/Update/Final/Hash      -> XXHash32
    Checksum_Error, Data_Corruption, Not_Supported,
    Too_Few_Header_Bytes, Too_Little_Memory           -> exceptions of the same names

Every block byte is decoded on the GPU; there is no CPU fallback.  Importing
fails loudly when the shared library is missing; decoding fails with
DeviceError when no GPU is usable.
"""
import ctypes
import enum
import os

# PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64.so.1.  Two
# HIP runtimes cannot share a GPU inside one process, so when torch is
# installed it is loaded first and liblz4ada_hip.so binds to torch's runtime
# (same SONAME): torch device pointers, streams and RCCL then work with it.
try:  # pragma: no cover - depends on the image
    import torch  # noqa: F401
except Exception:  # torch is optional for this binding
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# LZ4ADA_LIB selects a diagnostic build (tools/stamps.py); default: the product.
LIB_PATH = os.environ.get("LZ4ADA_LIB") or os.path.join(_HERE, "liblz4ada_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: build it with `make -C bo-lz4-ada_amd/csrc` "
                      "or __graft_entry__.build() (no CPU fallback exists)")

_lib = ctypes.CDLL(LIB_PATH)

# Decompressor.update through the CPython module (csrc/pyfast.c: no ctypes
# conversion per call) when it binds this same library.
_fast = None
if not os.environ.get("LZ4ADA_LIB") and not os.environ.get("LZ4ADA_NO_PYFAST"):
    try:
        import _lz4ada_fast as _fast  # noqa: E402  (bo-lz4-ada_amd/ is on sys.path)
    except ImportError:
        _fast = None

_i64 = ctypes.c_int64
_pi64 = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p


class Reservation(enum.IntEnum):
    """Flexible_Memory_Reservation (lz4ada.ads:79-106)."""
    SZ_64_KiB = 0
    SZ_256_KiB = 1
    SZ_1_MiB = 2
    SZ_4_MiB = 3
    SZ_8_MiB = 4
    Use_First = 5
    Single_Frame = 6


FOR_MODERN = Reservation.SZ_4_MiB   # lz4ada.ads:92
FOR_LEGACY = Reservation.SZ_8_MiB   # lz4ada.ads:100
FOR_ALL = Reservation.SZ_8_MiB      # lz4ada.ads:106


class EndOfFrame(enum.IntEnum):
    """End_Of_Frame (lz4ada.ads:124)."""
    Yes = 0
    No = 1
    Maybe = 2


# ------------------------------------------------------------------ errors

class LZ4AdaError(Exception):
    """Base: str() is the reference's Exception_Information line."""
    ada_name = "LZ4ADA.ERROR"

    def __init__(self, message: str):
        super().__init__(message)
        self.message = message

    def __str__(self):
        return f"raised {self.ada_name} : {self.message}"


class ChecksumError(LZ4AdaError):
    ada_name = "LZ4ADA.CHECKSUM_ERROR"


class DataCorruption(LZ4AdaError):
    ada_name = "LZ4ADA.DATA_CORRUPTION"


class NotSupported(LZ4AdaError):
    ada_name = "LZ4ADA.NOT_SUPPORTED"


class TooFewHeaderBytes(LZ4AdaError):
    ada_name = "LZ4ADA.TOO_FEW_HEADER_BYTES"


class TooLittleMemory(LZ4AdaError):
    ada_name = "LZ4ADA.TOO_LITTLE_MEMORY"


class AssertionFailure(LZ4AdaError):
    ada_name = "ADA.ASSERTIONS.ASSERTION_ERROR"


class ConstraintError(LZ4AdaError):
    ada_name = "CONSTRAINT_ERROR"


class DeviceError(LZ4AdaError):
    ada_name = "LZ4ADA.DEVICE_ERROR"


class NeedsExactPath(LZ4AdaError):
    """A device-only call declined the frame: lz4ada.decode_frame gives the
    reference's result (output or exception)."""
    ada_name = "LZ4ADA.EXACT_PATH"


_ERRORS = {1: ChecksumError, 2: DataCorruption, 3: NotSupported, 4: TooFewHeaderBytes,
           5: TooLittleMemory, 6: AssertionFailure, 7: ConstraintError, 8: DeviceError,
           9: NeedsExactPath}


def _check(status: int, message: str):
    if status:
        raise _ERRORS.get(status, LZ4AdaError)(message)


def _thread_error() -> str:
    return _lib.lz4ada_thread_last_error().decode()


# ---------------------------------------------------------------- signatures

class BlockDesc(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("out_off", ctypes.c_uint64),
                ("out_cap", ctypes.c_uint32), ("cksum", ctypes.c_uint32)]


class BlockStatus(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("aux", ctypes.c_int32), ("detail", ctypes.c_int64),
                ("err_out_pos", ctypes.c_int64), ("out_len", ctypes.c_uint32),
                ("cksum", ctypes.c_uint32)]


class FrameInfo(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("flg", ctypes.c_uint8), ("bd", ctypes.c_uint8),
                ("block_checksum", ctypes.c_uint8), ("content_checksum", ctypes.c_uint8),
                ("has_content_size", ctypes.c_uint8), ("independent", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 2), ("block_max", ctypes.c_int64),
                ("header_len", ctypes.c_int64), ("nblocks", ctypes.c_int64),
                ("frame_len", ctypes.c_int64), ("content_size", ctypes.c_uint64),
                ("content_checksum_declared", ctypes.c_uint32), ("pad2", ctypes.c_uint32)]


class XXH32State(ctypes.Structure):
    _fields_ = [("state", ctypes.c_uint32 * 4), ("buffer", ctypes.c_uint8 * 16),
                ("buffer_size", ctypes.c_int32), ("hash", ctypes.c_uint32),
                ("total_length", ctypes.c_uint64)]


class StreamEntry(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("frame_len", ctypes.c_int64), ("info", FrameInfo),
                ("batchable", ctypes.c_int32), ("pad", ctypes.c_int32)]


class FrameJob(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_void_p), ("len", ctypes.c_int64), ("out_off", ctypes.c_int64),
                ("out_len", ctypes.c_int64), ("consumed", ctypes.c_int64),
                ("status", ctypes.c_int32), ("path", ctypes.c_int32)]


class BatchStats(ctypes.Structure):
    _fields_ = [("frames_batched", ctypes.c_int64), ("frames_single", ctypes.c_int64),
                ("passes", ctypes.c_int64), ("gpu_hashed", ctypes.c_int64),
                ("host_hashed", ctypes.c_int64)]


class DeviceFrameJob(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_int64), ("in_len", ctypes.c_int64), ("out_off", ctypes.c_int64),
                ("out_len", ctypes.c_int64), ("consumed", ctypes.c_int64),
                ("status", ctypes.c_int32), ("reason", ctypes.c_int32)]


class DeviceDict(ctypes.Structure):
    """The dictionary of the _dict device calls: the last 65,536 bytes of
    dict_len bytes of device memory at d_dict; dict_id is compared with a
    frame's only under DICT_CHECK_ID in flags."""
    _fields_ = [("d_dict", ctypes.c_void_p), ("dict_len", ctypes.c_int64), ("dict_id", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class FrameRange(ctypes.Structure):
    """One range of decode_ranges_device: decoded bytes [off, off + len) of job."""
    _fields_ = [("job", ctypes.c_int64), ("off", ctypes.c_int64), ("len", ctypes.c_int64),
                ("out_off", ctypes.c_int64), ("out_len", ctypes.c_int64),
                ("status", ctypes.c_int32), ("reason", ctypes.c_int32)]


class SeekOptions(ctypes.Structure):
    """lz4ada_seek_options: flags (SEEK_LINKED), reserved (0), checkpoint_bytes
    (decoded bytes between history checkpoints; 0: the default, 1 MiB)."""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("checkpoint_bytes", ctypes.c_int64)]


SEEK_LINKED = 1  # SeekOptions.flags: the index takes linked frames, with checkpoints


class CompressOptions(ctypes.Structure):
    """lz4ada_compress_options: block_id (4..7 = 64 KiB..4 MiB; 0 means 4), flags (COMP_*)."""
    _fields_ = [("block_id", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class CompressJob(ctypes.Structure):
    """One record of compress_frames_device and, after the call, its frame."""
    _fields_ = [("in_off", ctypes.c_int64), ("in_len", ctypes.c_int64), ("out_off", ctypes.c_int64),
                ("out_len", ctypes.c_int64), ("status", ctypes.c_int32), ("stored_blocks", ctypes.c_int32)]


class CompressDict(ctypes.Structure):
    """lz4ada_compress_dict, the dictionary of the compress calls: the last
    65,536 bytes of dict_len bytes of device memory at d_dict; dict_id goes
    into every header under COMP_DICT_WRITE_ID in flags."""
    _fields_ = [("d_dict", ctypes.c_void_p), ("dict_len", ctypes.c_int64), ("dict_id", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class CompressIndexOptions(ctypes.Structure):
    """lz4ada_compress_index_options: flags (COMP_INDEX_LINKED), reserved (0),
    checkpoint_bytes (as SeekOptions')."""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("checkpoint_bytes", ctypes.c_int64)]


COMP_INDEX_LINKED = 1  # CompressIndexOptions.flags: frames of linked blocks
COMP_BLOCK_CHECKSUM, COMP_CONTENT_CHECKSUM, COMP_CONTENT_SIZE = 1, 2, 4
COMP_DICT_WRITE_ID = 1
_COMP_BLOCK_ID = {65536: 4, 262144: 5, 1 << 20: 6, 4 << 20: 7}

# DeviceFrameJob.reason: 1..4 are the BATCH_* reasons
DEVFRAME_OK, DEVFRAME_BLOCK, DEVFRAME_SIZE, DEVFRAME_CHECKSUM = 0, 5, 6, 7
DEVFRAME_DICT = 8  # the frame names another dictionary id (DeviceDict with DICT_CHECK_ID)
DICT_CHECK_ID = 1
EXACT_PATH = 9  # DeviceFrameJob.status of a frame the device pass did not decode

BLOCK_STORED = 1
BLOCK_HAS_CKSUM = 2
FORMAT_MODERN, FORMAT_LEGACY, FORMAT_SKIPPABLE = 1, 2, 3
# StreamEntry.batchable: why a frame does not take the many-frame pass
BATCH_OK, BATCH_LINKED, BATCH_BIG_BLOCK, BATCH_OVER_BUDGET, BATCH_NOT_INDEXED = 0, 1, 2, 3, 4
# flags of the many-frame calls (the `linked` keyword): linked frames up to
# batch_linked_max() share the pass
FRAMES_LINKED = 1
# (the `exact` keyword): the passes are laid out by the exact decoded sizes
FRAMES_EXACT = 2

_P = ctypes.POINTER
_len = len  # range_blocks_host has a parameter named len, as the C-ABI has
_dict = dict  # the compress and decode calls have a keyword named dict
_sig = {
    "lz4ada_stream_index": ([ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                             ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "lz4ada_decode_frames": ([ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p),
                              ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "lz4ada_frames_error": ([ctypes.c_int64], ctypes.c_char_p),
    "lz4ada_last_batch_stats": ([ctypes.POINTER(BatchStats)], None),
    "lz4ada_batch_hash_max": ([], ctypes.c_int64),
    "lz4ada_xxh32_spans_device": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                   ctypes.POINTER(ctypes.c_uint32),
                                   ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "lz4ada_frames_device_bound": ([_vp, _i64, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_decode_frames_device": ([_vp, _i64, _vp, _i64, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_frame_walk_host": ([_vp, _i64, ctypes.POINTER(FrameInfo), _vp, _i64], ctypes.c_int),
    "lz4ada_decode_frames_opt": ([_vp, _i64, ctypes.c_uint32, ctypes.POINTER(_vp), _pi64], ctypes.c_int),
    "lz4ada_stream_index_opt": ([_vp, _i64, ctypes.c_uint32, _vp, _i64, _pi64], ctypes.c_int),
    "lz4ada_frames_device_bound_opt": ([_vp, _i64, _vp, _i64, ctypes.c_uint32, _pi64, _vp], ctypes.c_int),
    "lz4ada_decode_frames_device_opt": ([_vp, _i64, _vp, _i64, ctypes.c_uint32, _vp, _i64, _pi64, _vp],
                                        ctypes.c_int),
    "lz4ada_frame_walk_host_opt": ([_vp, _i64, ctypes.c_uint32, ctypes.POINTER(FrameInfo), _vp, _i64],
                                   ctypes.c_int),
    "lz4ada_frames_device_bound_dict": ([_vp, _i64, _vp, _i64, ctypes.c_uint32, _vp, _pi64, _vp], ctypes.c_int),
    "lz4ada_decode_frames_device_dict": ([_vp, _i64, _vp, _i64, ctypes.c_uint32, _vp, _vp, _i64, _pi64, _vp],
                                         ctypes.c_int),
    "lz4ada_decode_frame_dict_host": ([_vp, _i64, _vp, _i64, _vp, _i64, _pi64, _pi64], ctypes.c_int),
    "lz4ada_frames_device_sizes": ([_vp, _i64, _vp, _i64, ctypes.c_uint32, _pi64, _vp], ctypes.c_int),
    "lz4ada_block_size_host": ([_vp, _i64, ctypes.c_int], _i64),
    "lz4ada_seek_index_build": ([_vp, _i64, _vp, _i64, ctypes.c_uint32, ctypes.POINTER(_vp), _vp], ctypes.c_int),
    "lz4ada_seek_index_build_opt": ([_vp, _i64, _vp, _i64, _vp, ctypes.POINTER(_vp), _vp], ctypes.c_int),
    "lz4ada_seek_index_build_dict": ([_vp, _i64, _vp, _i64, _vp, _vp, ctypes.POINTER(_vp), _vp], ctypes.c_int),
    "lz4ada_decode_idx_chains_debug": ([_vp, ctypes.c_uint64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
                                       ctypes.c_int),
    "lz4ada_range_gaps_host": ([_i64, _i64, ctypes.c_int32, _i64, _i64, _pi64, _pi64], ctypes.c_int),
    "lz4ada_range_chains_host": ([_i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _pi64], ctypes.c_int),
    "lz4ada_seek_index_free": ([_vp], None),
    "lz4ada_seek_index_bytes": ([_vp], _i64),
    "lz4ada_decode_ranges_device": ([_vp, _vp, _i64, _vp, _i64, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_range_blocks_host": ([_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp], ctypes.c_int),
    "lz4ada_seek_index_debug": ([_vp, _i64, ctypes.POINTER(ctypes.c_int32), _pi64, _vp, _i64, _vp],
                                ctypes.c_int),
    "lz4ada_ranges_select_debug": ([_vp, _vp, _i64, _pi64, _pi64, _pi64, _vp], ctypes.c_int),
    "lz4ada_batch_linked_max": ([], ctypes.c_int64),
    "lz4ada_decode_idx_frames_debug": ([_vp, ctypes.c_uint64, _vp, _i64, _pi64, _vp, _i64, _vp, _vp, _vp],
                                       ctypes.c_int),
    "lz4ada_frames_index_device_debug": ([_vp, _i64, _vp, _i64, ctypes.POINTER(ctypes.c_int32), _pi64,
                                          _vp, _i64, _vp], ctypes.c_int),
    "lz4ada_compress_frames_bound": ([_vp, _i64, _vp], _i64),
    "lz4ada_compress_frames_device": ([_vp, _i64, _vp, _i64, _vp, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_compress_block_host": ([_vp, _i64, _vp, _i64], _i64),
    "lz4ada_compress_frame_host": ([_vp, _i64, _vp, _vp, _i64], _i64),
    "lz4ada_compress_frames_bound_dict": ([_vp, _i64, _vp, _vp], _i64),
    "lz4ada_compress_frames_device_dict": ([_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_compress_block_dict_host": ([_vp, _i64, _vp, _i64, _vp, _i64], _i64),
    "lz4ada_compress_frames_device_linked": ([_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_compress_frame_linked_host": ([_vp, _i64, _vp, _vp, _i64, ctypes.c_uint32, ctypes.c_uint32, _vp, _i64],
                                          _i64),
    "lz4ada_compress_frames_device_indexed": ([_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _pi64, _vp,
                                               ctypes.POINTER(_vp), _vp], ctypes.c_int),
    "lz4ada_compress_index_host": ([_vp, _i64, _i64, _vp, ctypes.c_uint32, ctypes.c_uint32, _i64, ctypes.c_uint64,
                                    ctypes.c_uint64, _vp, _vp, _i64, _pi64, ctypes.POINTER(ctypes.c_int32), _pi64,
                                    _pi64], ctypes.c_int),
    "lz4ada_seek_index_store_debug": ([_vp, _vp, _i64, _pi64, _vp], ctypes.c_int),
    "lz4ada_seek_index_concat": ([_vp, _vp, _i64, _i64, ctypes.POINTER(_vp), _vp], ctypes.c_int),
    "lz4ada_index_merge_plan_host": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp],
                                     ctypes.c_int),
    "lz4ada_seek_index_arrays_debug": ([_vp, _pi64, _pi64, _pi64, ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                                       ctypes.c_int),
    "lz4ada_compress_frame_dict_host": ([_vp, _i64, _vp, _vp, _i64, ctypes.c_uint32, ctypes.c_uint32, _vp, _i64],
                                        _i64),
    "lz4ada_abi_version": ([], ctypes.c_int),
    "lz4ada_device_check": ([], ctypes.c_int),
    "lz4ada_error_name": ([ctypes.c_int], ctypes.c_char_p),
    "lz4ada_thread_last_error": ([], ctypes.c_char_p),
    "lz4ada_last_error": ([_vp], ctypes.c_char_p),
    "lz4ada_exact_blocks": ([_vp], _i64),
    "lz4ada_init": ([ctypes.c_int, _pi64, _P(_vp)], ctypes.c_int),
    "lz4ada_init_with_header": ([_vp, _i64, ctypes.c_int, _pi64, _pi64, _P(_vp)], ctypes.c_int),
    "lz4ada_init_for_block": ([_i64, ctypes.c_int, _pi64, _P(_vp)], ctypes.c_int),
    "lz4ada_update": ([_vp, _vp, _i64, _pi64, _vp, _i64, _pi64, _pi64], ctypes.c_int),
    "lz4ada_is_end_of_frame": ([_vp], ctypes.c_int),
    "lz4ada_free": ([_vp], None),
    "lz4ada_to_hex8": ([ctypes.c_uint8, ctypes.c_char_p], None),
    "lz4ada_to_hex32": ([ctypes.c_uint32, ctypes.c_char_p], None),
    "lz4ada_xxh32_init": ([_P(XXH32State), ctypes.c_uint32], None),
    "lz4ada_xxh32_reset": ([_P(XXH32State), ctypes.c_uint32], None),
    "lz4ada_xxh32_update": ([_P(XXH32State), _vp, _i64], ctypes.c_int),
    "lz4ada_xxh32_update_device": ([_P(XXH32State), _vp, _i64, _vp], ctypes.c_int),
    "lz4ada_content_xxh32_d2h": ([_P(XXH32State), _vp, _i64, _vp, _vp], ctypes.c_int),
    "lz4ada_xxh32_final": ([_P(XXH32State)], ctypes.c_uint32),
    "lz4ada_xxh32_hash": ([_vp, _i64, _P(ctypes.c_uint32)], ctypes.c_int),
    "lz4ada_frame_index": ([_vp, _i64, _P(FrameInfo), _vp, _i64], ctypes.c_int),
    "lz4ada_decode_blocks_device": ([_vp, ctypes.c_uint64, _vp, _i64, _vp, _vp, _vp],
                                    ctypes.c_int),
    "lz4ada_launch_decode": ([_vp, ctypes.c_uint64, _vp, _i64, _vp, _vp, _vp], ctypes.c_int),
    "lz4ada_launch_decode_variant": ([_vp, ctypes.c_uint64, _vp, _i64, _vp, _vp, ctypes.c_int, _vp],
                                     ctypes.c_int),
    "lz4ada_index_table_debug": ([_vp, ctypes.c_uint64, _vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_int],
                                 ctypes.c_int),
    "lz4ada_launch_block_checksums": ([_vp, _vp, _i64, _vp, _vp], ctypes.c_int),
    "lz4ada_output_checksums_device": ([_vp, _vp, _vp, _i64, _vp, _vp], ctypes.c_int),
    "lz4ada_decode_frame": ([_vp, _i64, _vp, _i64, _pi64, _pi64], ctypes.c_int),
    "lz4ada_decode_stream": ([_vp, _i64, _vp, _i64, _pi64], ctypes.c_int),
    "lz4ada_decode_frame_alloc": ([_vp, _i64, _P(_vp), _pi64, _pi64], ctypes.c_int),
    "lz4ada_decode_stream_alloc": ([_vp, _i64, _P(_vp), _pi64], ctypes.c_int),
    "lz4ada_decode_frame_partial": ([_vp, _i64, _P(_vp), _pi64, _pi64], ctypes.c_int),
    "lz4ada_buffer_free": ([_vp], None),
    "lz4ada_last_path": ([], ctypes.c_int),
    "lz4ada_bulk_decoder_kernel": ([ctypes.c_int64], ctypes.c_char_p),
    "lz4ada_release_device_cache": ([], None),
    "lz4ada_device_cache_stats": ([_vp], None),
    "lz4ada_decode_linked_device": ([_vp, ctypes.c_uint64, _vp, _i64, _i64, _vp, _i64, _pi64, _vp],
                                    ctypes.c_int),
    "lz4ada_decoded_bound": ([_vp, _i64], _i64),
    "lz4ada_decode_frame_multi": ([_vp, _i64, ctypes.c_int, _P(ctypes.c_int), _vp, _i64, _pi64,
                                   _pi64], ctypes.c_int),
    "lz4ada_decode_frame_multi_gather": ([_vp, _i64, ctypes.c_int, _P(ctypes.c_int), _vp, _i64,
                                          _pi64, _pi64], ctypes.c_int),
    "lz4ada_plan_shards": ([_vp, _i64, ctypes.c_int, _pi64], ctypes.c_int),
    "lz4ada_multi_device_allocs": ([ctypes.c_int], _i64),
    "lz4ada_rccl_version": ([], ctypes.c_int),
    "lz4ada_lone_scratch_bytes": ([_i64, _i64], _i64),
    "lz4ada_launch_decode_lone": ([_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp], ctypes.c_int),
    "lz4ada_gen_block": ([ctypes.c_int, ctypes.c_uint64, _vp, _i64, _vp, _i64], _i64),
    "lz4ada_gen_block_linked": ([ctypes.c_int, ctypes.c_uint64, _vp, _i64, _i64, _vp, _i64], _i64),
}
for _name, (_args, _res) in _sig.items():
    _f = getattr(_lib, _name)
    _f.argtypes = _args
    _f.restype = _res

EXPORTED = tuple(_sig)


def _addr(obj, offset=0):
    """Address of a bytes / bytearray / memoryview / ctypes buffer (+offset)."""
    if obj is None:
        return None
    if isinstance(obj, bytes):
        return ctypes.cast(ctypes.c_char_p(obj), _vp).value + offset
    if isinstance(obj, (bytearray, memoryview)):
        mv = memoryview(obj)
        if mv.readonly:
            obj = bytes(mv)
            return ctypes.cast(ctypes.c_char_p(obj), _vp).value + offset
        if mv.nbytes == 0:
            return None
        return ctypes.addressof(ctypes.c_char.from_buffer(mv)) + offset
    return ctypes.addressof(obj) + offset


def device_available() -> bool:
    return _lib.lz4ada_device_check() == 0


def error_name(status: int) -> str:
    return _lib.lz4ada_error_name(status).decode()


def to_hex(num: int, width: int = 32) -> str:
    """LZ4Ada.To_Hex (lz4ada.ads:306-307)."""
    if width == 8:
        b = ctypes.create_string_buffer(3)
        _lib.lz4ada_to_hex8(num, b)
    else:
        b = ctypes.create_string_buffer(9)
        _lib.lz4ada_to_hex32(num, b)
    return b.value.decode()


# ------------------------------------------------------------ Decompressor

class Decompressor:
    """LZ4Ada.Decompressor (lz4ada.ads:126).  Caller owns `buffer`."""

    def __init__(self, ptr: int):
        self._p = _vp(ptr)
        # per-call ctypes objects made once (an Update loop calls this once
        # per 4 KiB read: unlz4ada.adb:84-103)
        self._out = (_i64(), _i64(), _i64())
        self._refs = tuple(ctypes.byref(x) for x in self._out)
        self._data = self._data_addr = None
        self._buf = self._buf_view = None

    def __del__(self):
        p = getattr(self, "_p", None)
        if p is not None and p.value and _lib is not None:
            _lib.lz4ada_free(p)
            self._p = None

    @classmethod
    def init(cls, reservation=FOR_ALL):
        """Init (lz4ada.ads:218-220) -> (ctx, min_buffer_size)."""
        mbs, p = _i64(), _vp()
        _check(_lib.lz4ada_init(int(reservation), ctypes.byref(mbs), ctypes.byref(p)),
               _thread_error())
        return cls(p.value), mbs.value

    @classmethod
    def init_with_header(cls, data, reservation=Reservation.Single_Frame):
        """Init_With_Header (lz4ada.ads:238-243) -> (ctx, num_consumed, min_buffer_size)."""
        cons, mbs, p = _i64(), _i64(), _vp()
        st = _lib.lz4ada_init_with_header(_addr(data), len(data), int(reservation),
                                          ctypes.byref(cons), ctypes.byref(mbs), ctypes.byref(p))
        _check(st, _thread_error())
        return cls(p.value), cons.value, mbs.value

    @classmethod
    def init_for_block(cls, compressed_length: int, reservation=FOR_ALL):
        """Init_For_Block (lz4ada.ads:255-258) -> (ctx, min_buffer_size)."""
        mbs, p = _i64(), _vp()
        _check(_lib.lz4ada_init_for_block(compressed_length, int(reservation),
                                          ctypes.byref(mbs), ctypes.byref(p)), _thread_error())
        return cls(p.value), mbs.value

    def update(self, data, buffer, start: int = 0, stop=None):
        """Update (lz4ada.ads:281-287) on data[start:stop] ->
        (num_consumed, output_first, output_last); output is buffer[first:last+1]."""
        stop = len(data) if stop is None else stop
        if _fast is not None and isinstance(buffer, bytearray):
            st, c, f, l = _fast.update(self._p.value, data, start, stop, buffer)
            if st:
                _check(st, _lib.lz4ada_last_error(self._p).decode())
            return c, f, l
        n = stop - start
        cons, first, last = self._out
        rc, rf, rl = self._refs
        if data is not self._data:  # the same input object: its address is kept
            self._data = data
            self._data_addr = _addr(data) if isinstance(data, bytes) else None
        src = (self._data_addr + start if self._data_addr is not None else _addr(data, start)) \
            if n > 0 else None
        if buffer is not self._buf:
            # a ctypes view pins the bytearray (no resize while this context
            # holds it), so its address can be kept
            self._buf = buffer
            self._buf_view = (ctypes.c_char * len(buffer)).from_buffer(buffer) \
                if isinstance(buffer, bytearray) and len(buffer) else None
        dst = self._buf_view if self._buf_view is not None else _addr(buffer)
        st = _lib.lz4ada_update(self._p, src, n, rc, dst, len(buffer), rf, rl)
        if st:
            _check(st, _lib.lz4ada_last_error(self._p).decode())
        return cons.value, first.value, last.value

    def exact_blocks(self) -> int:
        """Blocks this context decoded on the reference-exact serial path."""
        return int(_lib.lz4ada_exact_blocks(self._p))

    def is_end_of_frame(self) -> EndOfFrame:
        return EndOfFrame(_lib.lz4ada_is_end_of_frame(self._p))


# ---------------------------------------------------------------- XXHash32

class XXHash32:
    """LZ4Ada.XXHash32 (lz4ada.ads:311-344).  update() hashes host bytes on the
    host (one serial chain); update_device / update_device_d2h take
    device-resident bytes."""

    def __init__(self, seed: int = 0):
        self._s = XXH32State()
        _lib.lz4ada_xxh32_init(ctypes.byref(self._s), seed)  # seed ignored (Q1)

    def reset(self, seed: int = 0):
        _lib.lz4ada_xxh32_reset(ctypes.byref(self._s), seed)

    def update(self, data):
        _check(_lib.lz4ada_xxh32_update(ctypes.byref(self._s), _addr(data), len(data)),
               _thread_error())

    def update_device(self, d_ptr: int, length: int, stream: int = 0):
        _check(_lib.lz4ada_xxh32_update_device(ctypes.byref(self._s), d_ptr, length, stream),
               _thread_error())

    def update_device_d2h(self, d_ptr, length, host_out=None, stream=0):
        """Update over device bytes via the D2H + host-chain pipeline; the
        bytes are also copied into host_out (a writable buffer) if given."""
        _check(_lib.lz4ada_content_xxh32_d2h(ctypes.byref(self._s), d_ptr, length,
                                             _addr(host_out) if host_out is not None else None,
                                             stream), _thread_error())

    def final(self) -> int:
        return _lib.lz4ada_xxh32_final(ctypes.byref(self._s))

    @staticmethod
    def hash(data) -> int:
        out = ctypes.c_uint32()
        _check(_lib.lz4ada_xxh32_hash(_addr(data), len(data), ctypes.byref(out)),
               _thread_error())
        return out.value


# ------------------------------------------------------------- bulk decode

def frame_index(data, offset: int = 0):
    """Host frame indexer -> (FrameInfo, ctypes array of BlockDesc)."""
    info = FrameInfo()
    n = len(data) - offset
    _check(_lib.lz4ada_frame_index(_addr(data, offset), n, ctypes.byref(info), None, 0),
           _thread_error())
    descs = (BlockDesc * max(info.nblocks, 1))()
    _check(_lib.lz4ada_frame_index(_addr(data, offset), n, ctypes.byref(info), descs,
                                   info.nblocks), _thread_error())
    return info, descs


def decoded_bound(data) -> int:
    return _lib.lz4ada_decoded_bound(_addr(data), len(data))


def _take(p, n: int) -> bytes:
    """Copy out and release a buffer from a lz4ada_decode_*_alloc call."""
    try:
        return ctypes.string_at(p, n) if n else b""
    finally:
        _lib.lz4ada_buffer_free(p)


def decode_frame(data, offset: int = 0):
    """One frame (Single_Frame semantics) -> (decoded bytes, bytes consumed).
    The library sizes the output itself, so any frame -- also one whose
    later bytes do not index -- raises the reference's own exception."""
    n = len(data) - offset
    p, olen, cons = _vp(), _i64(), _i64()
    _check(_lib.lz4ada_decode_frame_alloc(_addr(data, offset), n, ctypes.byref(p),
                                          ctypes.byref(olen), ctypes.byref(cons)),
           _thread_error())
    return _take(p, olen.value), cons.value


def decode_frame_partial(data, offset: int = 0):
    """One frame -> (decoded bytes, bytes consumed, exception or None).  On
    an error the bytes are what the reference had output before raising
    (every block before the failing one), as its CLI writes them."""
    n = len(data) - offset
    p, olen, cons = _vp(), _i64(), _i64()
    st = _lib.lz4ada_decode_frame_partial(_addr(data, offset), n, ctypes.byref(p),
                                          ctypes.byref(olen), ctypes.byref(cons))
    out = _take(p, olen.value) if p.value else b""
    exc = _ERRORS.get(st, LZ4AdaError)(_thread_error()) if st else None
    return out, cons.value, exc


def decode_stream(data) -> bytes:
    """Every frame of a concatenated stream -> decoded bytes."""
    p, olen = _vp(), _i64()
    _check(_lib.lz4ada_decode_stream_alloc(_addr(data), len(data), ctypes.byref(p),
                                           ctypes.byref(olen)), _thread_error())
    return _take(p, olen.value)


def _index(linked, plain, opt):
    """The C entry for a `linked` keyword: the plain one (which takes
    LZ4ADA_BATCH_LINKED from the environment) when it is False, else the
    _opt one with FRAMES_LINKED bound in."""
    if not linked:
        return plain
    return lambda *a: opt(*a[:2], FRAMES_LINKED, *a[2:])


def stream_index(data, linked=False):
    """Host walk of every frame of a concatenated stream -> list of
    StreamEntry (offset, frame_len, info, batchable: a BATCH_* reason code).
    Raises the exception of the first frame that does not index or is cut
    short; the frames before it are in the exception's `entries`.  linked:
    linked frames up to batch_linked_max() are batchable."""
    index = _index(linked, _lib.lz4ada_stream_index, _lib.lz4ada_stream_index_opt)
    n = _i64()
    st = index(_addr(data), len(data), None, 0, ctypes.byref(n))
    msg = _thread_error() if st else ""
    entries = (StreamEntry * max(n.value, 1))()
    m = _i64()
    index(_addr(data), len(data), entries, n.value, ctypes.byref(m))
    out = [entries[i] for i in range(n.value)]
    if st:
        exc = _ERRORS.get(st, LZ4AdaError)(msg)
        exc.entries = out
        raise exc
    return out


def decode_frames_jobs(frames, linked=False):
    """lz4ada_decode_frames as it is -> (the output buffer as bytes, the
    FrameJob array: out_off, out_len, consumed, status, path per frame).
    linked: lz4ada_decode_frames_opt with FRAMES_LINKED."""
    frames = [f if isinstance(f, bytes) else bytes(f) for f in frames]
    jobs = (FrameJob * max(len(frames), 1))()
    for j, f in zip(jobs, frames):
        j.frame = _addr(f)
        j.len = len(f)
    p, olen = _vp(), _i64()
    decode = _index(linked, _lib.lz4ada_decode_frames, _lib.lz4ada_decode_frames_opt)
    _check(decode(jobs, len(frames), ctypes.byref(p), ctypes.byref(olen)), _thread_error())
    return _take(p, olen.value), jobs


def decode_frames(frames, linked=False):
    """Many independent frames (each with Single_Frame semantics) in as few
    device passes as the byte budget allows -> list of (decoded bytes, bytes
    consumed, exception or None), one per frame.  One bad frame does not
    cost the others: a failed frame holds what the reference had output
    before raising, as decode_frame_partial gives it.  linked: linked frames
    up to batch_linked_max() share the passes too."""
    out, jobs = decode_frames_jobs(frames, linked)
    res = []
    for i in range(len(frames)):
        j = jobs[i]
        exc = _ERRORS.get(j.status, LZ4AdaError)(_lib.lz4ada_frames_error(i).decode()) \
            if j.status else None
        res.append((out[j.out_off:j.out_off + j.out_len], j.consumed, exc))
    return res


def last_batch_stats() -> BatchStats:
    """Counters of the last decode_frames / decode_stream call on this thread."""
    s = BatchStats()
    _lib.lz4ada_last_batch_stats(ctypes.byref(s))
    return s


def batch_hash_max() -> int:
    """G: the decoded length up to which a pass hashes a frame's content
    checksum on the GPU (LZ4ADA_BATCH_HASH_MAX overrides the default)."""
    return int(_lib.lz4ada_batch_hash_max())


def batch_linked_max() -> int:
    """The slot bytes up to which a linked frame shares a pass
    (LZ4ADA_BATCH_LINKED_MAX overrides the default)."""
    return int(_lib.lz4ada_batch_linked_max())


def xxh32_spans_device(d_buf: int, spans):
    """k_xxh32_spans alone over spans [(offset, length)] of device memory ->
    (list of XXH32 values, kernel milliseconds)."""
    n = len(spans)
    off = (_i64 * max(n, 1))(*[s[0] for s in spans])
    ln = (_i64 * max(n, 1))(*[s[1] for s in spans])
    h = (ctypes.c_uint32 * max(n, 1))()
    ms = ctypes.c_float()
    _check(_lib.lz4ada_xxh32_spans_device(d_buf, off, ln, n, h, ctypes.byref(ms)), _thread_error())
    return list(h[:n]), ms.value


# ------------------------------------- many frames, device memory to device

def _device_jobs(spans):
    """[(in_off, in_len)] -> DeviceFrameJob array (one spare entry when empty)."""
    jobs = (DeviceFrameJob * max(len(spans), 1))()
    for j, (off, n) in zip(jobs, spans):
        j.in_off, j.in_len = off, n
    return jobs


def _device_entry(linked, plain, opt, exact=False):
    if not linked and not exact:
        return plain
    flags = (FRAMES_LINKED if linked else 0) | (FRAMES_EXACT if exact else 0)
    if exact and not linked:  # as the plain entry reads it
        e = os.environ.get("LZ4ADA_BATCH_LINKED", "")
        flags |= FRAMES_LINKED if e and e[0] != "0" else 0
    return lambda *a: opt(*a[:4], flags, *a[4:])


def _dict_flags(linked, exact):
    """The flags a _dict call gets: what _device_entry gives the _opt call."""
    flags = (FRAMES_LINKED if linked else 0) | (FRAMES_EXACT if exact else 0)
    if not linked:  # as the plain entry reads it
        e = os.environ.get("LZ4ADA_BATCH_LINKED", "")
        flags |= FRAMES_LINKED if e and e[0] != "0" else 0
    return flags


def frames_device_bound(d_in: int, in_len: int, spans, stream: int = 0, linked=False, dict=None):
    """Index the frames at spans [(in_off, in_len)] of the device buffer d_in
    (raw pointer) on the device -> (an out_cap that always suffices, the
    DeviceFrameJob array with the index's verdict per frame).  dict: a
    DeviceDict (lz4ada_frames_device_bound_dict: with DICT_CHECK_ID a frame
    naming another id is EXACT_PATH / DEVFRAME_DICT)."""
    jobs = _device_jobs(spans)
    bound = _i64()
    if dict is not None:
        _check(_lib.lz4ada_frames_device_bound_dict(d_in, in_len, jobs, len(spans), _dict_flags(linked, False),
                                                    ctypes.byref(dict), ctypes.byref(bound), stream),
               _thread_error())
        return bound.value, jobs
    call = _device_entry(linked, _lib.lz4ada_frames_device_bound, _lib.lz4ada_frames_device_bound_opt)
    _check(call(d_in, in_len, jobs, len(spans), ctypes.byref(bound), stream), _thread_error())
    return bound.value, jobs


def frames_device_sizes(d_in: int, in_len: int, spans, stream: int = 0, linked=False):
    """The exact decoded sizes of the frames at spans [(in_off, in_len)] of the
    device buffer d_in (raw pointer), found on the device without decoding ->
    (total: an out_cap that suffices for decode_frames_device(exact=True), the
    DeviceFrameJob array: out_len is a frame's decoded length; status and
    reason as frames_device_bound gives them, or EXACT_PATH with
    DEVFRAME_BLOCK / DEVFRAME_SIZE from the sizes)."""
    jobs = _device_jobs(spans)
    total = _i64()
    _check(_lib.lz4ada_frames_device_sizes(d_in, in_len, jobs, len(spans), FRAMES_LINKED if linked else 0,
                                           ctypes.byref(total), stream), _thread_error())
    return total.value, jobs


def block_size_host(block, stored=False) -> int:
    """Test-only: the size rule on the host -> the decoded length of one
    block payload, or -1 when its sequence chain is malformed."""
    return int(_lib.lz4ada_block_size_host(_addr(block, 0) if len(block) else None, len(block),
                                           1 if stored else 0))


def decode_frames_device(d_in: int, in_len: int, spans, d_out: int, out_cap: int, stream: int = 0,
                         linked=False, exact=False, dict=None):
    """Decode the frames at spans [(in_off, in_len)] of the device buffer d_in
    into the device buffer d_out (raw pointers) -> (bytes written, the
    DeviceFrameJob array: out_off, out_len, consumed, status, reason).  A
    frame with status EXACT_PATH was not decoded: explain_frame gives the
    reference's verdict.  TooLittleMemory carries the needed size as .bound.
    exact: the frames are sized first (frames_device_sizes) and laid out by
    their sizes, so out_cap need only be that call's total.  dict: a
    DeviceDict shared by every frame (lz4ada_decode_frames_device_dict, the LZ4
    specification's semantics; decode_frame_dict_host is the way for a frame it
    answers with EXACT_PATH)."""
    jobs = _device_jobs(spans)
    n = _i64()
    if dict is not None:
        st = _lib.lz4ada_decode_frames_device_dict(d_in, in_len, jobs, len(spans), _dict_flags(linked, exact),
                                                   ctypes.byref(dict), d_out, out_cap, ctypes.byref(n), stream)
    else:
        call = _device_entry(linked, _lib.lz4ada_decode_frames_device, _lib.lz4ada_decode_frames_device_opt,
                             exact)
        st = call(d_in, in_len, jobs, len(spans), d_out, out_cap, ctypes.byref(n), stream)
    if st:
        exc = _ERRORS.get(st, LZ4AdaError)(_thread_error())
        exc.bound = n.value
        raise exc
    return n.value, jobs


def decode_frame_dict_host(frame, dict=b"", out_cap=None):
    """One modern frame decoded against a dictionary (bytes) on the host, no
    GPU involved: lz4ada_decode_frame_dict_host, the LZ4 specification's
    semantics -> (decoded bytes, bytes of the frame consumed).  out_cap: the
    output buffer's size (default: the declared content size, else every block
    at the frame's block maximum)."""
    frame, dict = bytes(frame), bytes(dict)
    if out_cap is None:
        info = FrameInfo()
        _lib.lz4ada_frame_walk_host_opt(_addr(frame) if frame else None, len(frame), FRAMES_LINKED,
                                        ctypes.byref(info), None, 0)
        out_cap = int(info.content_size) if info.has_content_size else int(info.nblocks) * int(info.block_max)
    buf = ctypes.create_string_buffer(max(out_cap, 1))
    n, used = _i64(), _i64()
    _check(_lib.lz4ada_decode_frame_dict_host(_addr(frame) if frame else None, len(frame),
                                              _addr(dict) if dict else None, len(dict), buf, out_cap,
                                              ctypes.byref(n), ctypes.byref(used)), _thread_error())
    return buf.raw[:n.value], used.value


def decode_frames_tensor(t, spans, out=None, linked=False, exact=False, dict=None, dict_id=None):
    """decode_frames_device for a CUDA torch.uint8 tensor holding the frames,
    on torch's current stream -> (the decoded bytes as a uint8 tensor on the
    same device, the DeviceFrameJob array).  out: a uint8 tensor there to
    decode into; by default one is allocated from frames_device_bound, or,
    exact, from frames_device_sizes.  dict: a CUDA uint8 tensor on the same
    device holding the dictionary every frame shares; dict_id: when given,
    a frame naming another dictionary id is rejected (DEVFRAME_DICT)."""
    if torch is None:
        raise RuntimeError("decode_frames_tensor needs torch")
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise ValueError("the frames must be a contiguous CUDA uint8 tensor")
    dd = None
    if dict is not None:
        if not (dict.is_cuda and dict.device == t.device and dict.dtype == torch.uint8 and dict.is_contiguous()):
            raise ValueError("the dictionary must be a contiguous CUDA uint8 tensor on the frames' device")
        dd = DeviceDict(dict.data_ptr() if dict.numel() else None, dict.numel(),
                        0 if dict_id is None else dict_id, 0 if dict_id is None else DICT_CHECK_ID)
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream().cuda_stream
        if out is None and dd is not None and not exact:
            bound, _ = frames_device_bound(t.data_ptr(), t.numel(), spans, stream, linked, dd)
            out = torch.empty(max(bound, 1), dtype=torch.uint8, device=t.device)
        elif out is None:
            size_of = frames_device_sizes if exact else frames_device_bound
            bound, _ = size_of(t.data_ptr(), t.numel(), spans, stream, linked)
            out = torch.empty(max(bound, 1), dtype=torch.uint8, device=t.device)
        elif not (out.is_cuda and out.device == t.device and out.dtype == torch.uint8
                  and out.is_contiguous()):
            raise ValueError("out must be a contiguous CUDA uint8 tensor on the frames' device")
        n, jobs = decode_frames_device(t.data_ptr(), t.numel(), spans, out.data_ptr(), out.numel(),
                                       stream, linked, exact, dd)
    return out[:n], jobs


# ------------------- records compressed into frames, device memory to device
# 

def _compress_options(block, block_checksum, content_checksum, content_size):
    """block: the block maximum in bytes (65536, 262144, 1 MiB, 4 MiB) or a
    block id as it is (0, 4..7, and whatever a misuse test passes)."""
    return CompressOptions(_COMP_BLOCK_ID.get(block, block),
                           (COMP_BLOCK_CHECKSUM if block_checksum else 0)
                           | (COMP_CONTENT_CHECKSUM if content_checksum else 0)
                           | (COMP_CONTENT_SIZE if content_size else 0))


def _compress_jobs(spans):
    jobs = (CompressJob * max(len(spans), 1))()
    for j, (off, n) in zip(jobs, spans):
        j.in_off, j.in_len = off, n
    return jobs


def _compress_dict(dict, dict_id):
    """The `dict` / `dict_id` keywords of the compress calls -> a CompressDict
    or None.  dict: a CompressDict as it is, or (d_dict, dict_len) of device
    memory; dict_id: when given, written into every header."""
    if isinstance(dict, CompressDict):
        return dict
    if dict is None and dict_id is None:
        return None
    d_dict, dict_len = dict if dict is not None else (None, 0)
    return CompressDict(d_dict, dict_len, 0 if dict_id is None else dict_id,
                        0 if dict_id is None else COMP_DICT_WRITE_ID)


def compress_frames_bound(lens, block=65536, block_checksum=False, content_checksum=False, content_size=False,
                          dict=None, dict_id=None):
    """An out_cap that always suffices for records of these lengths, one frame
    each: the header's exact worst-case arithmetic (every block stored).  No
    GPU involved.  dict, dict_id: as compress_frames_device takes them; only
    whether an id is written enters the bound (4 bytes per frame)."""
    opt = _compress_options(block, block_checksum, content_checksum, content_size)
    jobs = _compress_jobs([(0, n) for n in lens])
    cd = _compress_dict(dict, dict_id)
    if cd is None:
        bound = int(_lib.lz4ada_compress_frames_bound(jobs, len(lens), ctypes.byref(opt)))
    else:
        bound = int(_lib.lz4ada_compress_frames_bound_dict(jobs, len(lens), ctypes.byref(opt), ctypes.byref(cd)))
    if bound < 0:
        raise AssertionFailure("lz4ada_compress_frames_bound: a negative length, or options out of range")
    return bound


def compress_frames_device(d_in: int, in_len: int, spans, d_out: int, out_cap: int, stream: int = 0, block=65536,
                           block_checksum=False, content_checksum=False, content_size=False, dict=None,
                           dict_id=None, linked=False, index=False, checkpoint_bytes=0):
    """Compress the records at spans [(in_off, in_len)] of the device buffer
    d_in into LZ4 frames laid back to back into the device buffer d_out (raw
    pointers) -> (bytes written, the CompressJob array: out_off, out_len,
    status, stored_blocks).  TooLittleMemory carries the needed size as .bound
    and leaves d_out untouched.  dict: a CompressDict, or (d_dict, dict_len)
    of device memory, the dictionary every frame shares
    (lz4ada_compress_frames_device_dict; decode_frames_device with the same
    dictionary reads the frames); dict_id: when given, every header carries
    it, None writes none.  linked: frames of linked blocks
    (lz4ada_compress_frames_device_linked): a block after a
    record's first is compressed against the 65,536 bytes in front of it;
    decode_frames_device(linked=True) reads the frames.  index: the call
    also writes the frames' seek index (lz4ada_compress_frames_device_indexed,
    DESIGN.md §22) and returns it as a third value, a SeekIndex over (d_out,
    bytes written) whose .jobs is the call's report of the frames;
    checkpoint_bytes: as SeekIndex.build's, for linked frames."""
    opt = _compress_options(block, block_checksum, content_checksum, content_size)
    jobs = _compress_jobs(spans)
    n = _i64()
    cd = _compress_dict(dict, dict_id)
    if index:
        xopt = CompressIndexOptions(COMP_INDEX_LINKED if linked else 0, 0, checkpoint_bytes)
        frames = (DeviceFrameJob * max(len(spans), 1))()
        ptr = _vp()
        st = _lib.lz4ada_compress_frames_device_indexed(d_in, in_len, jobs, len(spans), ctypes.byref(opt),
                                                        None if cd is None else ctypes.byref(cd),
                                                        ctypes.byref(xopt), d_out, out_cap, ctypes.byref(n), frames,
                                                        ctypes.byref(ptr), stream)
        if st:
            exc = _ERRORS.get(st, LZ4AdaError)(_thread_error())
            exc.bound = n.value
            raise exc
        return n.value, jobs, SeekIndex(ptr.value, frames, len(spans), n.value)
    if linked:
        st = _lib.lz4ada_compress_frames_device_linked(d_in, in_len, jobs, len(spans), ctypes.byref(opt),
                                                       None if cd is None else ctypes.byref(cd), d_out, out_cap,
                                                       ctypes.byref(n), stream)
    elif cd is None:
        st = _lib.lz4ada_compress_frames_device(d_in, in_len, jobs, len(spans), ctypes.byref(opt), d_out, out_cap,
                                                ctypes.byref(n), stream)
    else:
        st = _lib.lz4ada_compress_frames_device_dict(d_in, in_len, jobs, len(spans), ctypes.byref(opt),
                                                     ctypes.byref(cd), d_out, out_cap, ctypes.byref(n), stream)
    if st:
        exc = _ERRORS.get(st, LZ4AdaError)(_thread_error())
        exc.bound = n.value
        raise exc
    return n.value, jobs


def compress_frames_tensor(t, spans, out=None, block=65536, block_checksum=False, content_checksum=False,
                           content_size=False, dict=None, dict_id=None, linked=False, index=False,
                           checkpoint_bytes=0):
    """compress_frames_device for a CUDA torch.uint8 tensor holding the
    records, on torch's current stream -> (the frames as a uint8 tensor on the
    same device, [(off, len)] of every record's frame inside it).  out: a uint8
    tensor there to write into; by default one of compress_frames_bound bytes
    is allocated.  dict: a CUDA uint8 tensor on the same device holding the
    dictionary every frame shares; dict_id: when given, written into every
    header.  linked: frames of linked blocks, as compress_frames_device's.
    index, checkpoint_bytes: as compress_frames_device's; the SeekIndex over the
    returned tensor comes as a third value."""
    if torch is None:
        raise RuntimeError("compress_frames_tensor needs torch")
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise ValueError("the records must be a contiguous CUDA uint8 tensor")
    if dict is not None:
        if not (dict.is_cuda and dict.device == t.device and dict.dtype == torch.uint8 and dict.is_contiguous()):
            raise ValueError("the dictionary must be a contiguous CUDA uint8 tensor on the records' device")
        dict = (dict.data_ptr() if dict.numel() else None, dict.numel())
    kw = _dict(block=block, block_checksum=block_checksum, content_checksum=content_checksum,
               content_size=content_size, dict=_compress_dict(dict, dict_id))
    with torch.cuda.device(t.device):
        if out is None:
            out = torch.empty(max(compress_frames_bound([n for _, n in spans], **kw), 1), dtype=torch.uint8,
                              device=t.device)
        elif not (out.is_cuda and out.device == t.device and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous CUDA uint8 tensor on the records' device")
        got = compress_frames_device(t.data_ptr() if t.numel() else None, t.numel(), spans, out.data_ptr(),
                                     out.numel(), torch.cuda.current_stream().cuda_stream, linked=linked,
                                     index=index, checkpoint_bytes=checkpoint_bytes, **kw)
    n, jobs = got[0], got[1]
    frames = [(jobs[i].out_off, jobs[i].out_len) for i in range(len(spans))]
    return (out[:n], frames, got[2]) if index else (out[:n], frames)


def compress_block_host(data, cap=None, dict=b"") -> bytes:
    """The serial statement of the block compressor (no GPU involved): data as
    one LZ4 block of at most cap bytes (default: whatever it takes) -> the
    block, or b"" when it does not fit into cap bytes.  dict (bytes): the
    dictionary in front of the block (lz4ada_compress_block_dict_host)."""
    data, dict = bytes(data), bytes(dict)
    if cap is None:
        cap = len(data) + len(data) // 255 + 16
    buf = ctypes.create_string_buffer(max(cap, 1))
    if dict:
        n = int(_lib.lz4ada_compress_block_dict_host(_addr(data) if data else None, len(data), _addr(dict),
                                                     len(dict), buf, cap))
    else:
        n = int(_lib.lz4ada_compress_block_host(_addr(data) if data else None, len(data), buf, cap))
    if n < 0:
        raise AssertionFailure("lz4ada_compress_block_host: a NULL pointer or a length out of range")
    return buf.raw[:n]


def compress_frame_host(data, block=65536, block_checksum=False, content_checksum=False, content_size=False,
                        cap=None, dict=b"", dict_id=None, linked=False) -> bytes:
    """The serial statement of one frame (no GPU involved): the bytes
    compress_frames_device writes for this record.  cap: the destination's
    size (default: the bound); below the bound: TooLittleMemory.  dict
    (bytes), dict_id: the dictionary and the id of that call
    (lz4ada_compress_frame_dict_host).  linked: the frame of linked blocks of
    compress_frames_device(linked=True) (lz4ada_compress_frame_linked_host)."""
    data, dict = bytes(data), bytes(dict)
    opt = _compress_options(block, block_checksum, content_checksum, content_size)
    if cap is None:
        cap = compress_frames_bound([len(data)], block, block_checksum, content_checksum, content_size,
                                    dict_id=dict_id)
    buf = ctypes.create_string_buffer(max(cap, 1))
    if linked:
        n = int(_lib.lz4ada_compress_frame_linked_host(_addr(data) if data else None, len(data), ctypes.byref(opt),
                                                       _addr(dict) if dict else None, len(dict),
                                                       0 if dict_id is None else dict_id,
                                                       0 if dict_id is None else COMP_DICT_WRITE_ID, buf, cap))
    elif dict or dict_id is not None:
        n = int(_lib.lz4ada_compress_frame_dict_host(_addr(data) if data else None, len(data), ctypes.byref(opt),
                                                     _addr(dict) if dict else None, len(dict),
                                                     0 if dict_id is None else dict_id,
                                                     0 if dict_id is None else COMP_DICT_WRITE_ID, buf, cap))
    else:
        n = int(_lib.lz4ada_compress_frame_host(_addr(data) if data else None, len(data), ctypes.byref(opt), buf,
                                                cap))
    if n < 0:
        raise _ERRORS.get(-n, LZ4AdaError)(f"lz4ada_compress_frame_host: {error_name(-n)}")
    return buf.raw[:n]


# ----------------------------- seek index and ranged decode

class SeekIndex:
    """A seek index over frames lying in device memory: per accepted frame its
    block descriptors and the decoded offset at which each block starts, in
    device memory the index owns (it survives release_device_cache()).  Built
    once and never changed, so any number of threads may decode ranges through
    it.  .jobs: the DeviceFrameJob array of the build (status, reason, out_len
    = exact decoded size, as frames_device_sizes gives them); .in_len: the
    input it was built over.  free() releases it; also a context manager."""

    def __init__(self, ptr, jobs, njobs, in_len):
        self._ptr, self.jobs, self.njobs, self.in_len = ptr, jobs, njobs, in_len

    @classmethod
    def build(cls, d_in: int, in_len: int, spans, stream: int = 0, flags: int = 0, linked: bool = False,
              checkpoint_bytes: int = 0, dict=None, dict_len: int = 0, dict_id=None):
        """Index the frames at spans [(in_off, in_len)] of the device buffer
        d_in (raw pointer).  Linked frames are refused (BATCH_LINKED) unless
        linked is set: then the build decodes each once and keeps a history
        checkpoint every checkpoint_bytes decoded bytes (0: 1 MiB), through
        lz4ada_seek_index_build_opt.  flags goes to
        lz4ada_seek_index_build as it is.  dict: a raw device pointer to
        dict_len bytes, the dictionary every frame shares, or a DeviceDict
        (lz4ada_seek_index_build_dict): the index keeps its own
        copy, so the ranged calls take none.  dict_id: when given, a frame
        naming another dictionary id is rejected (DEVFRAME_DICT)."""
        jobs = _device_jobs(spans)
        ptr = _vp()
        if dict is not None or dict_len or dict_id is not None:
            dd = dict if isinstance(dict, DeviceDict) else _seek_dict(dict, dict_len, dict_id)
            opt = SeekOptions(SEEK_LINKED if linked else 0, 0, checkpoint_bytes)
            st = _lib.lz4ada_seek_index_build_dict(d_in, in_len, jobs, len(spans), ctypes.byref(opt),
                                                   ctypes.byref(dd), ctypes.byref(ptr), stream)
        elif linked or checkpoint_bytes:
            opt = SeekOptions(SEEK_LINKED if linked else 0, 0, checkpoint_bytes)
            st = _lib.lz4ada_seek_index_build_opt(d_in, in_len, jobs, len(spans), ctypes.byref(opt),
                                                  ctypes.byref(ptr), stream)
        else:
            st = _lib.lz4ada_seek_index_build(d_in, in_len, jobs, len(spans), flags, ctypes.byref(ptr), stream)
        _check(st, _thread_error())
        return cls(ptr.value, jobs, len(spans), in_len)

    @classmethod
    def build_tensor(cls, t, spans, linked: bool = False, checkpoint_bytes: int = 0, dict=None, dict_id=None):
        """build for a CUDA torch.uint8 tensor, on torch's current stream.
        dict: a CUDA uint8 tensor on the same device holding the dictionary
        every frame shares (it may be freed after the build); dict_id: as in
        build."""
        _frames_tensor(t)
        dd = None
        if dict is not None:
            if not (dict.is_cuda and dict.device == t.device and dict.dtype == torch.uint8 and dict.is_contiguous()):
                raise ValueError("the dictionary must be a contiguous CUDA uint8 tensor on the frames' device")
            dd = _seek_dict(dict.data_ptr() if dict.numel() else None, dict.numel(), dict_id)
        with torch.cuda.device(t.device):
            return cls.build(t.data_ptr(), t.numel(), spans, torch.cuda.current_stream().cuda_stream,
                             linked=linked, checkpoint_bytes=checkpoint_bytes, dict=dd)

    @classmethod
    def concat(cls, parts, bases, in_len: int, stream: int = 0):
        """The indexes `parts` (SeekIndex objects, e.g. one per compress call)
        laid into one index over an input of in_len bytes in which the input
        of parts[p] lies at bases[p] (lz4ada_seek_index_concat, DESIGN.md
        §23).  Job j of parts[p] is job (jobs of the parts before) + j of the
        result; .jobs is the parts' reports in that order with in_off grown by
        the base.  The parts stay as they are and may be freed at once."""
        parts, bases = list(parts), list(bases)
        if len(parts) != len(bases):
            raise ValueError("one base per part")
        arr = (_vp * max(len(parts), 1))(*[p._ptr for p in parts])
        base = (_i64 * max(len(parts), 1))(*bases)
        ptr = _vp()
        _check(_lib.lz4ada_seek_index_concat(arr, base, len(parts), in_len, ctypes.byref(ptr), stream),
               _thread_error())
        njobs = sum(p.njobs for p in parts)
        jobs = (DeviceFrameJob * max(njobs, 1))()
        at = 0
        for p, b in zip(parts, bases):
            for i in range(p.njobs):
                ctypes.memmove(ctypes.byref(jobs[at]), ctypes.byref(p.jobs[i]), ctypes.sizeof(DeviceFrameJob))
                jobs[at].in_off += b
                at += 1
        return cls(ptr.value, jobs, njobs, in_len)

    @property
    def device_bytes(self) -> int:
        return int(_lib.lz4ada_seek_index_bytes(self._ptr))

    def free(self):
        if self._ptr:
            _lib.lz4ada_seek_index_free(self._ptr)
        self._ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _seek_dict(d_dict, dict_len, dict_id):
    """The DeviceDict of SeekIndex.build's keywords, as decode_frames_tensor
    makes its own: the id is compared only when one is given."""
    return DeviceDict(d_dict if dict_len else None, dict_len, 0 if dict_id is None else dict_id,
                      0 if dict_id is None else DICT_CHECK_ID)


def _frames_tensor(t):
    if torch is None:
        raise RuntimeError("this call needs torch")
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise ValueError("the frames must be a contiguous CUDA uint8 tensor")


def _frame_ranges(ranges):
    """[(job, off, len)] or a FrameRange array -> (FrameRange array, count)."""
    if isinstance(ranges, ctypes.Array):
        return ranges, len(ranges)
    arr = (FrameRange * max(len(ranges), 1))()
    for r, (job, off, n) in zip(arr, ranges):
        r.job, r.off, r.len = job, off, n
    return arr, len(ranges)


def decode_ranges_device(idx: SeekIndex, d_in: int, in_len: int, ranges, d_out: int, out_cap: int,
                         stream: int = 0):
    """Decode the ranges [(job, off, len)] of the decoded frames of idx: only
    the blocks they touch are decoded, and their bytes land back to back in
    the device buffer d_out in the order given -> (bytes written, the
    FrameRange array: out_off, out_len, status, reason).  A range is clipped to
    its frame; one with status EXACT_PATH was not delivered (its frame was not
    accepted, or a block it touches failed: DEVFRAME_BLOCK).  TooLittleMemory
    carries the clipped total as .bound (out_cap = 0 asks for it)."""
    arr, n = _frame_ranges(ranges)
    got = _i64()
    st = _lib.lz4ada_decode_ranges_device(idx._ptr, d_in, in_len, arr, n, d_out, out_cap, ctypes.byref(got),
                                          stream)
    if st:
        exc = _ERRORS.get(st, LZ4AdaError)(_thread_error())
        exc.bound = got.value
        raise exc
    return got.value, arr


def decode_ranges_tensor(idx: SeekIndex, t, ranges, out=None):
    """decode_ranges_device for the CUDA torch.uint8 tensor the index was
    built over, on torch's current stream -> (the ranges' bytes as a uint8
    tensor on the same device, the FrameRange array).  out: a uint8 tensor
    there to decode into; by default the clipped total is allocated."""
    _frames_tensor(t)
    arr, n = _frame_ranges(ranges)
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream().cuda_stream
        if out is None:
            try:
                total, _ = decode_ranges_device(idx, t.data_ptr(), t.numel(), arr, None, 0, stream)
            except TooLittleMemory as e:
                total = e.bound
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=t.device)
        elif not (out.is_cuda and out.device == t.device and out.dtype == torch.uint8
                  and out.is_contiguous()):
            raise ValueError("out must be a contiguous CUDA uint8 tensor on the frames' device")
        got, arr = decode_ranges_device(idx, t.data_ptr(), t.numel(), arr, out.data_ptr(), out.numel(), stream)
    return out[:got], arr


def range_blocks_host_many(starts, offs, lens):
    """Test-only: the block search on the host for many ranges of one frame.
    starts: the frame's exclusive prefix sum of block sizes and its size
    (nblocks + 1 entries) -> ctypes int64 arrays (first touched block, count,
    clipped length), one entry per range."""
    def i64(seq, kind=_i64):  # a list, or a numpy array of 64-bit integers
        if hasattr(seq, "tobytes"):
            return (kind * max(_len(seq), 1)).from_buffer_copy(seq.tobytes().ljust(8, b"\0"))
        return (kind * max(_len(seq), 1))(*seq)
    nb, n = _len(starts) - 1, _len(offs)
    a, off, ln = i64(starts, ctypes.c_uint64), i64(offs), i64(lens)
    first, count, want = (_i64 * max(n, 1))(), (_i64 * max(n, 1))(), (_i64 * max(n, 1))()
    _check(_lib.lz4ada_range_blocks_host(a, nb, off, ln, n, first, count, want),
           "range_blocks_host: a NULL or negative argument")
    return first, count, want


def range_blocks_host(starts, off: int, len: int):
    """Test-only: range_blocks_host_many for one range -> (first touched
    block, count, clipped length)."""
    first, count, want = range_blocks_host_many(starts, [off], [len])
    return first[0], count[0], want[0]


def range_chains_host(nblocks: int, group: int, touched):
    """Test-only: the chain rule on the host (lz4ada_range_chains.h) for one
    linked frame of nblocks blocks in groups of `group` and the touched
    intervals [(first, count)] of its ranges -> (marked blocks, heads, chains
    as [(first, count)]), the first two as sorted lists of block numbers."""
    n = _len(touched)
    first = (_i64 * max(n, 1))(*[t[0] for t in touched])
    count = (_i64 * max(n, 1))(*[t[1] for t in touched])
    marked, head = (ctypes.c_uint8 * max(nblocks, 1))(), (ctypes.c_uint8 * max(nblocks, 1))()
    cf, cc, nc = (_i64 * max(nblocks, 1))(), (_i64 * max(nblocks, 1))(), _i64()
    _check(_lib.lz4ada_range_chains_host(nblocks, group, first, count, n, marked, head, cf, cc, ctypes.byref(nc)),
           "range_chains_host: a NULL or out-of-range argument")
    return ([b for b in range(nblocks) if marked[b]], [b for b in range(nblocks) if head[b]],
            [(cf[i], cc[i]) for i in range(nc.value)])


def range_gaps_host(nblocks: int, group: int, kind: int, lo: int, hi: int):
    """Test-only: the gap count of the blocks [lo, hi) of one frame on the host
    (lz4ada_range_chains.h) -> (heads, dictionary-gapped blocks).  kind: 0 none
    read the dictionary, 1 a linked frame (block 0 does), 2 an independent
    modern frame (every block does)."""
    heads, gaps = _i64(), _i64()
    _check(_lib.lz4ada_range_gaps_host(nblocks, group, kind, lo, hi, ctypes.byref(heads), ctypes.byref(gaps)),
           "range_gaps_host: a NULL or out-of-range argument")
    return heads.value, gaps.value


def seek_index_debug(idx: SeekIndex, stream: int = 0):
    """Test-only: per job of the index (reason, start[] copied to the host: the
    decoded offset at which each block starts, and the frame's size; [0] for a
    frame the index did not accept)."""
    res = []
    for job in range(idx.njobs):
        reason, nb = ctypes.c_int32(), _i64()
        _check(_lib.lz4ada_seek_index_debug(idx._ptr, job, ctypes.byref(reason), ctypes.byref(nb), None, 0,
                                            stream), _thread_error())
        start = (ctypes.c_uint64 * (nb.value + 1))()
        _check(_lib.lz4ada_seek_index_debug(idx._ptr, job, ctypes.byref(reason), ctypes.byref(nb), start,
                                            nb.value + 1, stream), _thread_error())
        res.append((reason.value, list(start)))
    return res


def compress_index_host(frame, record_len, block=65536, block_checksum=False, content_checksum=False,
                        content_size=False, dict_id=None, linked=False, checkpoint_bytes=0, frame_off=0, out_base=0):
    """Test-only: the rule of the indexed compress call over one frame that
    compress_frame_host wrote with the same keywords (no GPU involved) ->
    (verdict, [BlockDesc], [decoded size], K, checkpoints)."""
    frame = bytes(frame)
    opt = _compress_options(block, block_checksum, content_checksum, content_size)
    cap = record_len // 65536 + 2
    descs, sizes = (BlockDesc * cap)(), (ctypes.c_uint32 * cap)()
    nb, verdict, group, ck = _i64(), ctypes.c_int32(), _i64(), _i64()
    st = _lib.lz4ada_compress_index_host(_addr(frame), len(frame), record_len, ctypes.byref(opt),
                                         0 if dict_id is None else COMP_DICT_WRITE_ID, 1 if linked else 0,
                                         checkpoint_bytes, frame_off, out_base, descs, sizes, cap, ctypes.byref(nb),
                                         ctypes.byref(verdict), ctypes.byref(group), ctypes.byref(ck))
    _check(st, "lz4ada_compress_index_host: the frame is not the record's, or an argument is out of range")
    return verdict.value, [descs[i] for i in range(nb.value)], list(sizes[:nb.value]), group.value, ck.value


def seek_index_store_debug(idx: SeekIndex, stream: int = 0) -> bytes:
    """Test-only: the checkpoint store of an index, 65,536 bytes per checkpoint."""
    n = _i64()
    _check(_lib.lz4ada_seek_index_store_debug(idx._ptr, None, 0, ctypes.byref(n), stream), _thread_error())
    buf = ctypes.create_string_buffer(max(n.value * 65536, 1))
    _check(_lib.lz4ada_seek_index_store_debug(idx._ptr, buf, n.value * 65536, ctypes.byref(n), stream),
           _thread_error())
    return buf.raw[:n.value * 65536]


def seek_index_arrays_debug(idx: SeekIndex, stream: int = 0):
    """Test-only: the index's device arrays copied to the host -> a dict:
    nframes, nblocks, nckpt, desc (a tuple of its six fields per block), first,
    start, slotp, and kgrp, ckfirst / fkind as lists, or None where the index
    holds none."""
    n, nb, nck = _i64(), _i64(), _i64()
    has_ck, has_kind = ctypes.c_int32(), ctypes.c_int32()

    def call(*arrays):
        _check(_lib.lz4ada_seek_index_arrays_debug(idx._ptr, ctypes.byref(n), ctypes.byref(nb), ctypes.byref(nck),
                                                   ctypes.byref(has_ck), ctypes.byref(has_kind), *arrays, stream),
               _thread_error())
    call(*[None] * 7)
    u64 = ctypes.c_uint64
    desc = (BlockDesc * max(nb.value, 1))()
    first, ckfirst = (u64 * (n.value + 1))(), (u64 * (n.value + 1))()
    start, slotp = (u64 * max(nb.value + n.value, 1))(), (u64 * max(nb.value + n.value, 1))()
    kgrp, fkind = (u64 * max(n.value, 1))(), (u64 * max(n.value, 1))()
    call(desc, first, start, slotp, kgrp, ckfirst, fkind)
    held = n.value > 0
    return _dict(nframes=n.value, nblocks=nb.value, nckpt=nck.value,
                 desc=[(d.in_off, d.in_len, d.flags, d.out_off, d.out_cap, d.cksum) for d in desc[:nb.value]],
                 first=list(first) if held else None,
                 start=list(start[:nb.value + n.value]) if held else None,
                 slotp=list(slotp[:nb.value + n.value]) if held else None,
                 kgrp=list(kgrp[:n.value]) if has_ck.value else None,
                 ckfirst=list(ckfirst) if has_ck.value else None,
                 fkind=list(fkind[:n.value]) if has_kind.value else None)


MERGE_PREFIX_NAMES = ("frames", "blocks", "words", "checkpoints", "slots")


def index_merge_plan_host(parts, bases, in_len: int, queries=()):
    """Test-only: the merge rule on the host (lz4ada_index_merge.h, no GPU
    involved).  parts: [(jobs, blocks, checkpoints, input length, nominal
    slots)]; bases: where each part's input lies in an input of in_len bytes;
    queries: [(prefix 0..4, merged element)] -> (the five exclusive prefixes as
    lists of len(parts) + 1, in MERGE_PREFIX_NAMES' order; the part of every
    query).  AssertionFailure for what lz4ada_seek_index_concat calls misuse,
    ConstraintError from 2^31 jobs or blocks."""
    parts, bases, queries = list(parts), list(bases), list(queries)
    if len(parts) != len(bases):
        raise ValueError("one base per part")
    m, nq = len(parts), len(queries)
    cols = [(_i64 * max(m, 1))(*[p[k] for p in parts]) for k in range(5)]
    base = (_i64 * max(m, 1))(*bases)
    prefix = (ctypes.c_uint64 * (5 * (m + 1)))()
    kind = (_i64 * max(nq, 1))(*[q[0] for q in queries])
    elem = (_i64 * max(nq, 1))(*[q[1] for q in queries])
    part_of = (_i64 * max(nq, 1))()
    _check(_lib.lz4ada_index_merge_plan_host(*cols, base, m, in_len, prefix, kind, elem, nq, part_of),
           "lz4ada_index_merge_plan_host: parts that do not rise inside in_len, a query out of range, or too many jobs")
    return [list(prefix[k * (m + 1):(k + 1) * (m + 1)]) for k in range(5)], list(part_of[:nq])


def ranges_select_debug(idx: SeekIndex, ranges, stream: int = 0):
    """Test-only: the selection alone -> ([(first block, count)] per range,
    blocks marked once shared ones count once)."""
    arr, n = _frame_ranges(ranges)
    first, count, marked = (_i64 * max(n, 1))(), (_i64 * max(n, 1))(), _i64()
    _check(_lib.lz4ada_ranges_select_debug(idx._ptr, arr, n, first, count, ctypes.byref(marked), stream),
           _thread_error())
    return [(first[i], count[i]) for i in range(n)], marked.value


def explain_frame(t_or_bytes, job):
    """What the reference makes of one job's frame: its bytes are fetched to
    the host (from a tensor or a bytes-like object holding the device input)
    and decoded on their own -> decode_frame_partial's (decoded bytes, bytes
    consumed, exception or None)."""
    lo, hi = job.in_off, job.in_off + job.in_len
    if torch is not None and isinstance(t_or_bytes, torch.Tensor):
        data = t_or_bytes[lo:hi].cpu().numpy().tobytes()
    else:
        data = bytes(t_or_bytes[lo:hi])
    return decode_frame_partial(data)


def frame_walk_host(data, offset: int = 0, linked=False):
    """Test-only: the device index's frame walk run on the host ->
    (verdict: a BATCH_* reason, FrameInfo, ctypes array of BlockDesc as
    frame_index lays them out).  linked: lz4ada_frame_walk_host_opt with
    FRAMES_LINKED (plain flags otherwise: no environment switch here)."""
    n = len(data) - offset
    info = FrameInfo()
    walk = _index(linked, _lib.lz4ada_frame_walk_host, _lib.lz4ada_frame_walk_host_opt)
    v = walk(_addr(data, offset), n, ctypes.byref(info), None, 0)
    descs = (BlockDesc * max(info.nblocks, 1))()
    info2 = FrameInfo()
    v2 = walk(_addr(data, offset), n, ctypes.byref(info2), descs, info.nblocks)
    assert v2 == v and bytes(info2) == bytes(info)
    return v, info, descs


def frames_index_device_debug(d_in: int, in_len: int, spans, stream: int = 0):
    """Test-only: the index kernels alone -> (verdict per job, nblocks per
    job, BlockDesc array of the accepted frames' blocks in rising in_off)."""
    jobs = _device_jobs(spans)
    n = len(spans)
    verdict = (ctypes.c_int32 * max(n, 1))()
    nblocks = (_i64 * max(n, 1))()
    # without room for descriptors first: the verdicts and the block counts
    st = _lib.lz4ada_frames_index_device_debug(d_in, in_len, jobs, n, verdict, nblocks, None, 0, stream)
    if st and not (st == 7 and _thread_error() == "descriptor capacity exceeded"):
        _check(st, _thread_error())
    total = sum(nblocks[i] for i in range(n) if verdict[i] == BATCH_OK)
    descs = (BlockDesc * max(total, 1))()
    _check(_lib.lz4ada_frames_index_device_debug(d_in, in_len, jobs, n, verdict, nblocks, descs,
                                                 total, stream), _thread_error())
    return list(verdict[:n]), list(nblocks[:n]), descs


def _devices(n_gpus: int, devices):
    if devices is None:
        return None
    if len(devices) != n_gpus:
        raise ValueError("devices must name n_gpus ordinals")
    return (ctypes.c_int * n_gpus)(*devices)


def decode_frame_multi(data, n_gpus: int, devices=None, offset: int = 0):
    """One frame over n_gpus GPUs from this process (lz4ada_decode_frame_multi:
    one worker thread per device, RCCL for the verdict all-reduce) ->
    (decoded bytes, bytes consumed).  Frames that do not shard (linked,
    legacy) or that the bulk path rejects decode on the first device with
    the reference's result."""
    n = len(data) - offset
    bound = _lib.lz4ada_decoded_bound(_addr(data, offset), n)
    if bound < 0:  # does not index: the reference's own exception
        return decode_frame(data, offset)
    out = bytearray(max(bound, 1))
    olen, cons = _i64(), _i64()
    _check(_lib.lz4ada_decode_frame_multi(_addr(data, offset), n, n_gpus,
                                          _devices(n_gpus, devices), _addr(out), bound,
                                          ctypes.byref(olen), ctypes.byref(cons)), _thread_error())
    del out[olen.value:]
    return bytes(out), cons.value


def decode_frame_multi_gather(data, n_gpus: int, d_out: int, out_cap: int, devices=None,
                              offset: int = 0):
    """decode_frame_multi with the output gathered (RCCL send/recv) into
    device memory d_out on the first device -> (decoded length, consumed)."""
    n = len(data) - offset
    olen, cons = _i64(), _i64()
    _check(_lib.lz4ada_decode_frame_multi_gather(_addr(data, offset), n, n_gpus,
                                                 _devices(n_gpus, devices), d_out, out_cap,
                                                 ctypes.byref(olen), ctypes.byref(cons)),
           _thread_error())
    return olen.value, cons.value


def plan_shards(descs, nblocks: int, n_gpus: int):
    """lz4ada_plan_shards -> [(lo, hi)] block ranges per device."""
    b = (ctypes.c_int64 * (n_gpus + 1))()
    _check(_lib.lz4ada_plan_shards(descs, nblocks, n_gpus, b), _thread_error())
    return [(b[r], b[r + 1]) for r in range(n_gpus)]


PATH_INDEPENDENT, PATH_LINKED, PATH_EXACT, PATH_MULTI = 1, 2, 4, 8
PATH_BATCH = 16  # the frame was committed from a many-frame pass


def multi_device_allocs(device: int) -> int:
    """Device allocations the multi-GPU worker of `device` made so far (-1:
    no worker yet); a repeated call of the same size adds none."""
    return int(_lib.lz4ada_multi_device_allocs(device))


def rccl_version() -> int:
    """ncclGetVersion of the RCCL this process bound (22606 = 2.26.6)."""
    return int(_lib.lz4ada_rccl_version())


def bulk_decoder_kernel(nblocks: int) -> str:
    """The kernel the product bulk call launches for `nblocks` blocks."""
    return _lib.lz4ada_bulk_decoder_kernel(nblocks).decode()


def last_path() -> int:
    """PATH_* bits of the paths the last decode_frame / decode_stream call on
    this thread took (bulk independent, bulk linked, reference-exact)."""
    return _lib.lz4ada_last_path()


def release_device_cache():
    """Free the bulk path's cached device scratch of the calling thread and
    empty the process-wide memory pools and the stream pool."""
    _lib.lz4ada_release_device_cache()


class CacheStats(ctypes.Structure):
    _fields_ = [("device_idle_bytes", _i64), ("pinned_idle_bytes", _i64), ("idle_streams", _i64)]


def device_cache_stats() -> CacheStats:
    """What the pools hold idle: device bytes, pinned bytes, stream sets."""
    s = CacheStats()
    _lib.lz4ada_device_cache_stats(ctypes.byref(s))
    return s


def decode_blocks_device(d_frame: int, frame_len: int, d_descs: int, nblocks: int, d_out: int,
                         d_status: int, stream: int = 0):
    """Launch block checksums + decode over device-resident buffers (async)."""
    _check(_lib.lz4ada_decode_blocks_device(d_frame, frame_len, d_descs, nblocks, d_out,
                                            d_status, stream), _thread_error())


def decode_linked_device(d_frame: int, frame_len: int, descs, nblocks: int, block_max: int,
                         d_out: int, out_cap: int, stream: int = 0) -> int:
    """Linked-frame bulk path over a device-resident frame (host descriptors
    from frame_index) into contiguous device output -> decoded length.
    Raises NeedsExactPath when decode_frame must give the reference's result."""
    olen = _i64()
    _check(_lib.lz4ada_decode_linked_device(d_frame, frame_len, descs, nblocks, block_max, d_out,
                                            out_cap, ctypes.byref(olen), stream), _thread_error())
    return olen.value


def launch_decode(d_frame, frame_len, d_descs, nblocks, d_out, d_status, stream=0):
    _check(_lib.lz4ada_launch_decode(d_frame, frame_len, d_descs, nblocks, d_out, d_status,
                                     stream), _thread_error())


DECODE_PC, DECODE_IDX, DECODE_IDX_ALONE, DECODE_IDX_LINKED = 0, 3, 4, 5
DECODE_IDX_SPARSE = 6
DECODE_IDX1_ALONE, DECODE_IDX2_ALONE = 7, 8  # fused index decoder alone: one / two waves per block
DECODE_PP2_ALONE = 9  # the pipelined two-wave decoder alone
DECODE_IDX_SPLIT = 10  # k_index, then k_decode_idx's pass 2: two launches


def launch_decode_variant(d_frame, frame_len, d_descs, nblocks, d_out, d_status, variant,
                          stream=0):
    """One of the bulk decoders: DECODE_IDX (default: index-driven + two-wave
    retry), DECODE_PC, DECODE_IDX_ALONE."""
    _check(_lib.lz4ada_launch_decode_variant(d_frame, frame_len, d_descs, nblocks, d_out,
                                             d_status, variant, stream), _thread_error())


def index_table_debug(d_frame, frame_len, d_descs, nblocks, d_status, stream=0, waves=1) -> bytes:
    """Test-only: pass 1 (k_index) alone, by 1 or 2 waves per block (the pass 1
    of k_decode_idx / k_decode_pp2); the sequence-index table as bytes.
    Block b's 8-byte records (bitmap | count << 32, one per 32 payload bytes)
    start at byte 64 * ((in_off >> 8) + b); d_status gets pass 1's verdicts."""
    cap = ((frame_len >> 8) + nblocks + 2) * 64
    buf = (ctypes.c_uint8 * cap)()
    _check(_lib.lz4ada_index_table_debug(d_frame, frame_len, d_descs, nblocks, buf, cap, d_status,
                                         stream, waves), _thread_error())
    return bytes(buf)


def decode_idx_frames_debug(d_frame, frame_len, d_descs, nblocks, first, linked, d_out, d_status,
                            stream=0):
    """Test-only: k_index + k_decode_idx_frames alone.  first: nframes + 1
    rising block indices (frame i holds blocks first[i] .. first[i + 1] - 1 of
    d_descs); linked[i] true marks the frames to walk (one wave each, the
    blocks in order with the earlier output as history); the others' statuses
    and slots are left alone.  Returns after the stream has drained."""
    nframes = len(first) - 1
    f = (_i64 * (nframes + 1))(*first)
    m = (ctypes.c_uint8 * max(nframes, 1))(*[1 if x else 0 for x in linked])
    _check(_lib.lz4ada_decode_idx_frames_debug(d_frame, frame_len, d_descs, nblocks, f, m, nframes,
                                               d_out, d_status, stream), _thread_error())


def decode_idx_chains_debug(d_frame, frame_len, descs, nblocks, chains, d_out, d_status, stream=0):
    """Test-only: k_index + k_decode_idx_chains alone.  descs: a
    BlockDesc array on the host; chains: [(first block, count, history bytes,
    gapped)], rising and disjoint -- the history lies in front of the first
    block's slot in d_out, and gapped marks that block as having such a gap.
    d_status: zeroed device statuses.  Returns after the stream has drained."""
    n = len(chains)
    first = (_i64 * max(n, 1))(*[c[0] for c in chains])
    count = (_i64 * max(n, 1))(*[c[1] for c in chains])
    hist = (ctypes.c_uint32 * max(n, 1))(*[c[2] for c in chains])
    gapped = (ctypes.c_uint8 * max(n, 1))(*[1 if c[3] else 0 for c in chains])
    _check(_lib.lz4ada_decode_idx_chains_debug(d_frame, frame_len, descs, nblocks, first, count, hist, gapped, n,
                                               d_out, d_status, stream), _thread_error())


def lone_scratch_bytes(n: int, cap: int) -> int:
    return _lib.lz4ada_lone_scratch_bytes(n, cap)


def launch_decode_lone(d_blk, n, d_out, cap, d_status, d_scratch, scratch_bytes, stream=0):
    """One block by the whole GPU (lz4ada_lone.hip); status DS_OK or DS_RETRY."""
    _check(_lib.lz4ada_launch_decode_lone(d_blk, n, d_out, cap, d_status, d_scratch,
                                          scratch_bytes, stream), _thread_error())


DS_RETRY = 10
DS_SPARSE = 11  # pass 1 declined a literal-heavy block (k_decode_sparse takes it)


def launch_block_checksums(d_frame, d_descs, nblocks, d_status, stream=0):
    _check(_lib.lz4ada_launch_block_checksums(d_frame, d_descs, nblocks, d_status, stream),
           _thread_error())


def output_checksums_device(d_out, d_descs, d_status, nblocks, d_hash, stream=0):
    _check(_lib.lz4ada_output_checksums_device(d_out, d_descs, d_status, nblocks, d_hash,
                                               stream), _thread_error())


# ---------------------------------------------------------- synthetic data

GEN_DENSE, GEN_MIXED, GEN_RLE, GEN_LITERAL, GEN_CHAIN, GEN_MIXED_NOD1 = 0, 1, 2, 3, 4, 5
GEN_KINDS = {"dense": GEN_DENSE, "mixed": GEN_MIXED, "rle": GEN_RLE, "literal": GEN_LITERAL,
             "chain": GEN_CHAIN, "mixed_nod1": GEN_MIXED_NOD1}


def gen_block(kind: int, seed: int, raw_len: int):
    """One synthetic compressed block -> (payload bytes, decoded bytes)."""
    raw = ctypes.create_string_buffer(max(raw_len, 1))
    cap = raw_len + raw_len // 128 + 64 + raw_len // 200 + 1024
    comp = ctypes.create_string_buffer(cap)
    n = _lib.lz4ada_gen_block(kind, seed, raw, raw_len, comp, cap)
    if n < 0:
        raise RuntimeError("gen_block: capacity")
    return comp.raw[:n], raw.raw[:raw_len]


def gen_linked_blocks(kind: int, seed: int, block_len: int, nblocks: int, last_len=None,
                      lens=None, hist=b""):
    """Blocks of one linked frame whose matches reach back into the earlier
    blocks' output (up to 64 KiB) -> list of (payload, decoded).  lens: the
    decoded length of every block (overrides block_len / nblocks / last_len).
    hist: bytes that precede the first block (a dictionary), which its matches
    may read too."""
    if lens is None:
        lens = [block_len] * nblocks
        if last_len is not None and nblocks:
            lens[-1] = last_len
    out, hist = [], bytes(hist)
    for i, raw_len in enumerate(lens):
        h = hist[-65536:]
        buf = ctypes.create_string_buffer(h + bytes(max(raw_len, 1)), len(h) + max(raw_len, 1))
        cap = raw_len + raw_len // 128 + 64 + raw_len // 200 + 1024
        comp = ctypes.create_string_buffer(cap)
        n = _lib.lz4ada_gen_block_linked(kind, seed + i, buf, len(h), raw_len, comp, cap)
        if n < 0:
            raise RuntimeError("gen_block_linked: capacity")
        raw = buf.raw[len(h):len(h) + raw_len]
        out.append((comp.raw[:n], raw))
        hist += raw
    return out
