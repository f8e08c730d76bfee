"""ctypes binding of libhiccup_hip.so (include/hiccup_hip.h).

This is the drop-in boundary: hiccup's Python surface (transform / quantization /
codec / compression) calls these C-ABI entry points, which launch the gfx950
HIP kernels.  There is no CPU fallback anywhere in the package: if the shared
library or a GPU is missing, every call raises ``HipUnavailable``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HICCUP_HIP_LIB", os.path.join(_HERE, "lib", "libhiccup_hip.so"))

HIC_OK = 0
HIC_ERR_ARG = -1
HIC_ERR_HIP = -2
HIC_ERR_CAPACITY = -3

TABLE_LUMINANCE = 0
TABLE_CHROMINANCE = 1

LAYOUT_RASTER_I32 = 0
LAYOUT_RASTER_I16 = 1
LAYOUT_ZIGZAG_I16 = 2

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_sz = ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/hiccup_hip.h exactly
class RleJob16(ctypes.Structure):
    """hic_rle_job16 (include/hiccup_hip.h)."""
    _fields_ = [("blocks", _vp), ("nblk", _i64), ("d_stitch", _vp), ("dc_diff", _vp), ("sym_len", _vp),
                ("sym_val", _vp), ("sym_cap", _i64), ("d_count", _vp), ("workspace", _vp), ("records_per_tile", _i64),
                ("workspace_bytes", _i64), ("d_index", _vp)]


class SlotJob(ctypes.Structure):
    """hic_slot_job (include/hiccup_hip.h): one channel of the slot-layout encode."""
    _fields_ = [("nblk", _i64), ("records_per_tile", _i64), ("slot_len", _vp), ("slot_val", _vp), ("dc_diff", _vp),
                ("d_index", _vp), ("workspace", _vp), ("workspace_bytes", _i64), ("d_count", _vp), ("sym_len", _vp),
                ("sym_val", _vp), ("sym_cap", _i64)]


class KeyStream(ctypes.Structure):
    """hic_key_stream (include/hiccup_hip.h): one int32 key stream of hic_huffman_batch_*."""
    _fields_ = [("keys", _vp), ("n", _i64)]


class WireJob(ctypes.Structure):
    """hic_wire_job (include/hiccup_hip.h): one segment of a batched wire pack / unpack."""
    _fields_ = [("blocks", _vp), ("wire", _vp), ("nblk", _i64), ("table_id", ctypes.c_int32), ("d_flag", _vp),
                ("rec_src", _vp), ("nrec", _i64), ("pos_shift", _i64), ("rec_dst", _vp), ("d_count", _vp)]


class SlotFillJob(ctypes.Structure):
    """hic_slot_fill_job (include/hiccup_hip.h): one segment of hic_slots_fill_batch."""
    _fields_ = [("wire", _vp), ("blocks", _vp), ("nblk", _i64), ("block0", _i64), ("channel", _int),
                ("table_id", _int)]


class Encode420Job(ctypes.Structure):
    """hic_encode420_job (include/hiccup_hip.h): one encode of hic_encode420_batch_u8."""
    _fields_ = [("rgb_rows", _vp), ("in_row0", _i64), ("in_rows", _i64), ("H", _i64), ("W", _i64),
                ("out_row0", _i64), ("out_rows", _i64), ("coef_y", _vp), ("coef_cr", _vp), ("coef_cb", _vp),
                ("ws_y", _vp), ("ws_cr", _vp), ("ws_cb", _vp)]


class HuffDecodeJob(ctypes.Structure):
    """hic_huffman_decode_job (include/hiccup_hip.h): one stream of hic_huffman_decode_batch."""
    _fields_ = [("d_bits", _vp), ("nbits", _i64), ("h_child", _vp), ("nnodes", ctypes.c_int32), ("h_values", _vp),
                ("nleaves", ctypes.c_int32), ("d_out", _vp), ("out_cap", _i64), ("workspace", _vp),
                ("count", _i64), ("status", ctypes.c_int32)]


class DctPlaneJob(ctypes.Structure):
    """hic_dct_plane_job (include/hiccup_hip.h)."""
    _fields_ = [("plane", _vp), ("H", _i64), ("W", _i64), ("stride", _i64), ("table_id", _int), ("out", _vp),
                ("rle_workspace", _vp)]


class Window(ctypes.Structure):
    """hic_window (include/hiccup_hip.h): hic_window_plan's geometry of a region decode."""
    _fields_ = [("Y0", _i64), ("X0", _i64), ("Y1", _i64), ("X1", _i64), ("cy0", _i64), ("cx0", _i64), ("ch", _i64),
                ("cw", _i64)]


STREAM_INDEXED = 0
STREAM_SLOTS = 1


class DecodePlane(ctypes.Structure):
    """hic_decode_plane (include/hiccup_hip.h): one channel of one image of a batched decode."""
    _fields_ = [("sym_len", _vp), ("sym_val", _vp), ("d_nsym", _vp), ("dc_diff", _vp), ("d_index", _vp),
                ("out", _vp), ("d_status", _vp)]


class DecodeImage(ctypes.Structure):
    """hic_decode_image (include/hiccup_hip.h): Y, Cr, Cb of one image."""
    _fields_ = [("c", DecodePlane * 3)]


class WinGeo(ctypes.Structure):
    """WinGeo (csrc/decode_batch.h): the kernels' geometry of one window launch."""
    _fields_ = [(f, _int) for f in ("bi0", "nrows", "bj0", "bj1", "tpr", "oy", "ox", "cy0", "cx0", "ch", "cw",
                                    "cpitch")] + [("n_ac", _i64)]


class DecodeWindowEntry(ctypes.Structure):
    """DecWinBatchEntry (csrc/decode_batch.h): one image of a batched region decode's table."""
    _fields_ = [("c", DecodePlane * 3), ("g", WinGeo * 2), ("y0", ctypes.c_int32), ("x0", ctypes.c_int32),
                ("pad", _i64 * 28)]


class DecodeWindowHeader(ctypes.Structure):
    """DecWinBatchHeader (csrc/decode_batch.h)."""
    _fields_ = [("magic", ctypes.c_uint64), ("kind", ctypes.c_int32), ("n", ctypes.c_int32), ("H", _i64), ("W", _i64),
                ("h", _i64), ("w", _i64), ("out_row_stride", _i64), ("chroma_pitch", _i64), ("chroma_rows", _i64),
                ("waves_y", ctypes.c_int32), ("waves_c", ctypes.c_int32), ("grid_y", ctypes.c_int32),
                ("grid_c", ctypes.c_int32), ("nblk_y", _i64), ("nblk_c", _i64), ("pad", _i64 * 3)]


assert ctypes.sizeof(DecodeWindowEntry) == 512 and ctypes.sizeof(DecodeWindowHeader) == 128

SIGNATURES = {
    "hic_abi_version": (_int, []),
    "hic_last_error": (_int, [ctypes.c_char_p, _sz]),
    "hic_device_count": (_int, [ctypes.POINTER(_int)]),
    "hic_stream_sync": (_int, [_vp]),
    "hic_probe_copy": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp]),
    "hic_probe_plane": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp]),
    "hic_probe_encode420": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hic_set_knob": (_int, [_int, _int]),
    "hic_get_knob": (_int, [_int, ctypes.POINTER(_int)]),
    "hic_dct_quant_u8": (_int, [_vp, _i64, _i64, _i64, _int, _int, _vp, _vp]),
    "hic_dct_quant_u8_timed": (_int, [_vp, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "hic_dct_quant_rle_u8": (_int, [_vp, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "hic_dct_quant_rle_u8_batch": (_int, [_int, _vp, _int, _vp, _vp, _vp]),
    "hic_rle_encode_i16_tiles": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hic_rle_shard_summary_tiles": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "hic_rle_shard_summary_records": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "hic_key_range": (_int, [_vp, _int, _i64, _vp, _vp]),
    "hic_key_histogram": (_int, [_vp, _int, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp]),
    "hic_huffman_pack_workspace_bytes": (_sz, [_i64]),
    "hic_wire_bytes": (_sz, [_i64, _int]),
    "hic_rle_decode_idct_u8_indexed": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _i64, _vp, _vp]),
    "hic_rle_decode_idct_u8_indexed_pair": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _i64, _vp, _vp]),
    "hic_rle_decode_idct_rgb_indexed": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
    "hic_rle_tile_index_i16": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "hic_rle_decode_i16_indexed": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hic_rle_tile_records_i16": (_int, [_vp, _i64, _int, _vp, _vp]),
    "hic_wire_pack_i16": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "hic_wire_unpack_i16": (_int, [_vp, _i64, _int, _vp, _vp]),
    "hic_rle_records_rebase": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "hic_huffman_decode_workspace_bytes": (_sz, [_i64, ctypes.c_int32, ctypes.c_int32]),
    "hic_huffman_decode": (_int, [_vp, _i64, _vp, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _i64, _vp, _vp, _vp]),
    "hic_huffman_build": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "hic_zigzag8_blocks_i16": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "hic_event_record": (_int, [_vp, _vp]),
    "hic_wire_pack_batch": (_int, [_int, _vp, _vp]),
    "hic_wire_unpack_batch": (_int, [_int, _vp, _vp]),
    "hic_wire_flags_apply": (_int, [_int, _vp, _vp]),
    "hic_slots_fill_batch": (_int, [_int, _vp, _int, _vp, _int, _vp]),
    "hic_encode420_batch_u8": (_int, [_int, _vp, _int, _vp, _vp, _vp]),
    "hic_huffman_decode_batch": (_int, [_int, _vp, _vp]),
    "hic_huffman_decode_table_workspace_bytes": (_sz, [_int, _vp]),
    "hic_huffman_decode_table": (_int, [_int, _vp, _vp, _sz, _vp]),
    "hic_huffman_from_codes": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hic_huffman_pack": (_int, [_vp, _int, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _i64, _vp, _vp,
                                _vp]),
    "hic_encode420_u8": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp,
                                _vp, _vp]),
    "hic_rle_encode_i16_tiles_batch": (_int, [_int, _vp, _int, _vp]),
    "hic_encode420_seg_u8": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                    _i64, _int, _vp, _vp, _vp]),
    "hic_rle_encode_i16_rows_batch": (_int, [_int, _vp, _vp, _int, _vp]),
    "hic_rle_slots_workspace_bytes": (_sz, [_i64, _int]),
    "hic_encode420_slots_u8": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp]),
    "hic_rle_slots_close": (_int, [_int, _vp, _int, _vp]),
    "hic_slots_batch_table_bytes": (_sz, [_int]),
    "hic_slots_batch_table": (_int, [_int, _i64, _i64, _vp, _vp, _sz]),
    "hic_encode420_slots_batch_u8": (_int, [_vp, _i64, _vp, _vp, _int, _vp, _vp, _vp]),
    "hic_rle_slots_close_batch": (_int, [_vp, _vp, _int, _vp]),
    "hic_probe_encode420_slots": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hic_rle_slots_compact": (_int, [_int, _vp, _int, _vp]),
    "hic_slot_key_range": (_int, [_int, _vp, _int, _vp, _vp]),
    "hic_slot_key_histogram": (_int, [_int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hic_slot_huffman_pack_workspace_bytes": (_sz, [_int, _vp]),
    "hic_slot_huffman_pack": (_int, [_int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hic_huffman_batch_key_range_workspace_bytes": (_sz, [_int]),
    "hic_huffman_batch_key_range": (_int, [_int, _vp, _vp, _int, _vp, _vp, _sz, _vp]),
    "hic_huffman_batch_histogram_workspace_bytes": (_sz, [_int, _vp, _vp, _vp]),
    "hic_huffman_batch_histogram": (_int, [_int, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "hic_huffman_batch_pack_workspace_bytes": (_sz, [_int, _vp, _vp]),
    "hic_huffman_batch_pack": (_int, [_int, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "hic_huffman_build_batch": (_int, [_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "hic_rle_decode_i16_slots": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "hic_rle_decode_idct_u8_slots": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _int, _vp, _i64, _vp, _vp]),
    "hic_rle_decode_idct_u8_slots_pair": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _int, _vp, _i64, _vp,
                                                 _vp]),
    "hic_rle_decode_idct_rgb_slots": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp, _vp, _i64, _vp,
                                             _vp]),
    "hic_rle_stream_index_workspace_bytes": (_sz, [_i64, _i64]),
    "hic_rle_stream_index_i16": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hic_window_plan": (_int, [_i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(Window)]),
    "hic_rle_decode_idct_u8_window_pair": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64,
                                                  ctypes.POINTER(Window), _vp, _i64, _vp, _vp]),
    "hic_rle_decode_idct_rgb_window": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, ctypes.POINTER(Window),
                                              _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "hic_decode_batch_table_bytes": (_sz, [_int]),
    "hic_decode_batch_table": (_int, [_int, _int, _i64, _i64, _i64, _i64, _vp, _vp, _sz]),
    "hic_decode420_batch_u8": (_int, [_vp, _vp, _vp]),
    "hic_decode_window_batch_table_bytes": (_sz, [_int]),
    "hic_decode_window_batch_table": (_int, [_int, _int, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _sz]),
    "hic_decode420_window_batch_u8": (_int, [_vp, _vp, _vp]),
    "hic_event_create": (_int, [_vp]),
    "hic_event_destroy": (_int, [_vp]),
    "hic_event_elapsed_ms": (_int, [_vp, _vp, _vp]),
    "hic_dequant_idct_u8": (_int, [_vp, _int, _i64, _i64, _int, _vp, _i64, _vp]),
    "hic_dct2_f64": (_int, [_vp, _i64, _vp, _vp]),
    "hic_idct2_f64": (_int, [_vp, _i64, _vp, _vp]),
    "hic_quantize_f64": (_int, [_vp, _i64, _int, _vp, _vp]),
    "hic_dequantize_i32": (_int, [_vp, _i64, _int, _vp, _vp]),
    "hic_rgb_to_ycrcb420": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hic_rgb_to_ycrcb420_rows": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hic_rgb_to_ycrcb": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hic_pyr_down_u8": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp]),
    "hic_pyr_up_u8": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp]),
    "hic_ycrcb420_to_rgb": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp]),
    "hic_ycrcb420_to_rgb_rows": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "hic_zigzag_blocks_i32": (_int, [_vp, _i64, _i64, _int, _vp, _vp]),
    "hic_izigzag_blocks_i32": (_int, [_vp, _i64, _i64, _int, _vp, _vp]),
    "hic_rle_workspace_bytes": (_sz, [_i64, _int]),
    "hic_rle_rows_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "hic_rle_shard_summary_i16": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "hic_rle_shard_summary_i32": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "hic_rle_encode_i16": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hic_rle_encode_i32": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hic_rle_stitch": (_int, [_vp, _int, _int, _int, _vp, _vp]),
    "hic_rle_stream_encode_i32": (_int, [_vp, _i64, _int, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hic_rle_stream_decode_i32": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "hic_rld_workspace_bytes": (_sz, [_i64, _i64]),
    "hic_rle_decode_i16": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "hic_rle_decode_i16_shard": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hic_rle_decode_i32": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "hic_gather_unique_id": (_int, [_vp]),
    "hic_gather_comm_init": (_int, [_vp, _vp, _int, _int]),
    "hic_gather_comm_info": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "hic_gather_comm_destroy": (_int, [_vp]),
    "hic_gather_group_begin": (_int, []),
    "hic_gather_group_end": (_int, []),
    "hic_gather_bytes": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _int, _vp]),
}
GATHER_ID_BYTES = 128


class HipUnavailable(RuntimeError):
    """The HIP extension (libhiccup_hip.so) or an MI355X device is missing."""


class HipError(RuntimeError):
    """A C-ABI call returned a HIP runtime error."""


_lib = None


def load():
    """Load the shared library (no GPU needed: symbol resolution only)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipUnavailable(
                "libhiccup_hip.so not found at %s: build it with `python -c "
                "'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        # an explicitly chosen older library (HICCUP_HIP_LIB, A/B timing) may predate
        # an entry point: it stays unbound and fails when called; the in-tree library
        # must export every one
        override = "HICCUP_HIP_LIB" in os.environ
        for name, (res, args) in SIGNATURES.items():
            if override and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def last_error():
    buf = ctypes.create_string_buffer(512)
    load().hic_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(status, what=""):
    """Map a C-ABI status to the reference's error behaviour."""
    if status == HIC_OK:
        return
    msg = "%s: %s" % (what, last_error()) if what else last_error()
    if status == HIC_ERR_ARG:
        raise ValueError(msg)
    if status == HIC_ERR_CAPACITY:
        raise MemoryError(msg)
    raise HipError(msg)


def call(name, *args):
    check(getattr(load(), name)(*args), name)


# A/B knobs (include/hiccup_hip.h HIC_KNOB_*): every selectable path is bit-exact
KNOBS = {"dct_path": 0, "dct_waves_per_cu": 1, "color_tiled": 2, "color_seg": 3, "rld_generic": 7,
         "dev": 8, "encode_order": 13, "encode_band": 16}
DCT_PATH_F64, DCT_PATH_EXACT = 1, 0  # (2 = 1 since round 6: its LDS-DMA prefetch form was removed)


def set_knob(name, value):
    call("hic_set_knob", KNOBS[name], int(value))
    _knob_set[name] = int(value)


def get_knob(name):
    v = _int(0)
    call("hic_get_knob", KNOBS[name], ctypes.byref(v))
    return v.value


class knobs:
    """Context manager: `with _lib.knobs(dct_path=0): ...` sets knobs, restoring
    the values they had on entry (nested contexts and earlier set_knob calls keep
    their settings)."""

    def __init__(self, **kw):
        self.kw = kw
        self.saved = {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.saved[k] = _raw_knob(k)
            set_knob(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            set_knob(k, v)
        return False


_knob_set = {}  # name -> the value last given to set_knob (-1: default)


def _raw_knob(name):
    """The value set_knob last stored for `name` (-1 = the library default)."""
    return _knob_set.get(name, -1)
