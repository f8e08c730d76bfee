"""CPU tests of the slot-reading Huffman entry points (hic_slot_key_range /
hic_slot_key_histogram / hic_slot_huffman_pack, include/hiccup_hip.h) and of the
one-call surface codec.encode / codec.decode: what they refuse before any device
call.  No GPU, nothing launched."""
import ctypes

import numpy as np
import pytest

from hiccup_amd import _lib, codec

P = 1 << 20  # a 16-byte aligned address, never dereferenced


def _job(nblk=128, rpt=1, **kw):
    ws = _lib.load().hic_rle_slots_workspace_bytes(nblk, rpt)
    f = dict(nblk=nblk, records_per_tile=rpt, slot_len=P, slot_val=P, dc_diff=P, d_index=P, workspace=P,
             workspace_bytes=ws, d_count=P, sym_len=P, sym_val=P, sym_cap=nblk * 63 + 1)
    f.update(kw)
    return _lib.SlotJob(**f)


def _calls(lib, n, jobs, max_len=15):
    """The three entry points' statuses for the same BAD jobs (every other argument
    is in order, so each must be refused on the jobs alone)."""
    m = 2 * max(n, 1)
    i32 = (ctypes.c_int32 * m)(*[0] * m)
    nb = (ctypes.c_int32 * m)(*[1] * m)
    off = (ctypes.c_int64 * m)(*range(m))
    ptrs = (ctypes.c_void_p * m)(*[P] * m)
    nbytes = (ctypes.c_int64 * m)(*[64] * m)
    return (lib.hic_slot_key_range(n, jobs, max_len, P, None),
            lib.hic_slot_key_histogram(n, jobs, max_len, i32, nb, P, P, off, None),
            lib.hic_slot_huffman_pack(n, jobs, max_len, i32, nb, ptrs, ptrs, ptrs, nbytes, P, P, None))


def test_slot_huffman_entry_points_refuse_bad_jobs():
    """Every job is checked before any device call: refused here without a GPU
    (HIC_ERR_ARG, nothing launched)."""
    lib = _lib.load()
    bad = (_lib.HIC_ERR_ARG,) * 3
    one = (_lib.SlotJob * 1)(_job())
    four = (_lib.SlotJob * 4)(*[_job()] * 4)
    assert _calls(lib, 0, one) == bad  # job counts outside 1..3
    assert _calls(lib, 4, four) == bad
    assert _calls(lib, 1, None) == bad  # null job array
    assert _calls(lib, 1, one, max_len=14) == bad
    assert "max_len 15" in _lib.last_error()
    for field in ("slot_len", "slot_val", "d_index", "workspace", "d_count"):
        jobs = (_lib.SlotJob * 2)(_job(), _job(64, 2, **{field: None}))
        assert _calls(lib, 2, jobs) == bad, field
        assert "job 1: null pointer" in _lib.last_error(), field
    for kw in (dict(nblk=0), dict(nblk=100), dict(records_per_tile=3), dict(slot_len=P + 4), dict(slot_val=P + 8),
               dict(workspace_bytes=8)):
        assert _calls(lib, 1, (_lib.SlotJob * 1)(_job(**kw))) == bad, kw
    # the streams' own arguments, with jobs that are in order (each call below is one
    # that must be refused: nothing here may reach the device)
    E = _lib.HIC_ERR_ARG
    zero, one_bin, no_bin = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 2)(1, 1), (ctypes.c_int32 * 2)(1, 0)
    off = (ctypes.c_int64 * 2)(0, 1)
    ptrs = (ctypes.c_void_p * 2)(P, P)
    n64, n62 = (ctypes.c_int64 * 2)(64, 64), (ctypes.c_int64 * 2)(64, 62)
    assert lib.hic_slot_key_range(1, one, 15, None, None) == E
    hist = lambda **kw: lib.hic_slot_key_histogram(  # noqa: E731
        1, one, 15, kw.get("key_min", zero), kw.get("nbins", one_bin), kw.get("counts", P), kw.get("first", P),
        kw.get("off", off), None)
    for kw in (dict(key_min=None), dict(nbins=None), dict(nbins=no_bin), dict(counts=None), dict(first=None),
               dict(off=None), dict(off=(ctypes.c_int64 * 2)(0, -1))):
        assert hist(**kw) == E, kw
    pack = lambda **kw: lib.hic_slot_huffman_pack(  # noqa: E731
        1, one, 15, zero, kw.get("nbins", one_bin), kw.get("bits", ptrs), kw.get("lens", ptrs), kw.get("out", ptrs),
        kw.get("nbytes", n64), kw.get("nbits", P), kw.get("ws", P), None)
    for kw in (dict(nbins=no_bin), dict(bits=None), dict(lens=(ctypes.c_void_p * 2)(P, None)), dict(out=None),
               dict(nbytes=n62), dict(nbytes=(ctypes.c_int64 * 2)(64, 0)), dict(nbits=None), dict(ws=None)):
        assert pack(**kw) == E, kw
    assert pack(out=(ctypes.c_void_p * 2)(P, P + 2)) == E  # a misaligned output
    assert "aligned" in _lib.last_error()


def test_slot_huffman_pack_workspace_bytes():
    """Two int64 per record (a length and a value stream each) plus slack."""
    lib = _lib.load()
    jobs = (_lib.SlotJob * 3)(_job(8100 * 64, 1), _job(4050 * 32, 2), _job(4050 * 32, 2))
    assert lib.hic_slot_huffman_pack_workspace_bytes(3, jobs) >= 8 * 2 * (8100 + 4050 + 4050)
    assert lib.hic_slot_huffman_pack_workspace_bytes(1, jobs) >= 8 * 2 * 8100


def test_codec_encode_decode_surface():
    """codec.encode / codec.decode exist; encode validates shape and dtype before any
    device call (ValueError, as compression.jpeg_compression)."""
    assert hasattr(codec, "encode") and hasattr(codec, "decode")
    with pytest.raises(ValueError):
        codec.encode(np.zeros((16, 16, 3), np.float32))
    with pytest.raises(ValueError):
        codec.encode(np.zeros((16, 16), np.uint8))
    with pytest.raises(ValueError):
        codec.encode(np.zeros((16, 16, 4), np.uint8))
