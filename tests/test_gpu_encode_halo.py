"""The fused encoder's stacked bands (knob encode_band, default 1): a
workgroup's four waves are four vertically adjacent 16-row units of one strip, and
the pyrDown halo rows two of them share are converted once and passed through LDS
(hiccup_amd/csrc/encode.hip, EncColour::band_edges / band_rows).

The slot tests compare the slot layout with the coefficient chain, and both run this
same colour stage: a wrong halo row would pass them.  These tests compare against
the C oracle (cvtColor -> pyrDown -> dct_channel -> zig-zag -> DPCM / RLE, the
restatement test_gpu_codec.py pins the encoder to), at the smallest shapes at which
each case of the exchange exists, on a random image and on a row-distinct one (every
row its own colour: a halo taken from the wrong row, the wrong wave or a stale slot
changes the chroma).  Reference: compression.jpeg_compression (compression.py:16-39),
codec.jpeg_encode (codec.py:286-301)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.oracle_c as orcc  # noqa: E402
from hiccup_amd import _lib, device, pipeline, sharding  # noqa: E402

# slot layout (W % 512 == 0): a lone unit (every halo its own), a short band of two,
# exactly one band (every interior exchange), a band + a lone unit (a halo across a
# band edge), 4 + 3, two bands x two strips
SLOT_SHAPES = [(16, 512), (32, 512), (64, 512), (80, 512), (112, 512), (128, 1024)]
# the fused coefficient path with a ragged last strip
RAGGED_SHAPES = [(80, 528), (80, 48), (144, 16)]
KINDS = ["random", "rows"]


def _img(kind, H, W):
    rng = np.random.default_rng(1000 * H + W)
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "rows":  # row r is the constant colour (7 r, 11 r + 3, 13 r + 5) mod 256, but for a few random columns
        r = np.arange(H)
        img = np.stack([7 * r, 11 * r + 3, 13 * r + 5], -1)[:, None, :].repeat(W, 1) % 256
        cols = rng.integers(0, W, 5)
        img[:, cols] = rng.integers(0, 256, (H, 5, 3))
        return img.astype(np.uint8)
    raise ValueError(kind)


def _oracle_encode(rgb):
    y, cr, cb = orcc.rgb_to_ycrcb(rgb)
    planes = {"lum": (y, 0), "cr": (orcc.pyr_down(cr), 1), "cb": (orcc.pyr_down(cb), 1)}
    out = {}
    for k, (p, t) in planes.items():
        q = orcc.dct_channel(p, t, threads=16)
        zz = orcc.zigzag_blocks(q, 8)
        L, V = orcc.rle_encode(zz[:, 1:].reshape(-1), 15)
        out[k] = (zz, orcc.dpcm(zz[:, 0].copy()), L, V)
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """(image, the oracle's encode of it): computed once, shared, never written."""
    rgb = _img(kind, H, W)
    return rgb, _oracle_encode(rgb)


def _assert_equals_oracle(got, exp, msg):
    for k in pipeline.CHANNELS:
        for j, what in enumerate(("blocks", "dc", "sym_len", "sym_val")):
            np.testing.assert_array_equal(np.asarray(got[k][j]).astype(np.int32), exp[k][j],
                                          err_msg="%s %s %s" % (msg, k, what))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SLOT_SHAPES)
def test_halo_slots_vs_oracle(kind, H, W):
    """The default encoder (slot layout, stacked bands) == the C oracle."""
    rgb, exp = _case(kind, H, W)
    assert _lib.get_knob("encode_band") == 1
    enc = pipeline.Encoder(H, W)
    assert enc.slots
    enc.encode(device.to_device(rgb))
    _assert_equals_oracle(enc.result(), exp, "slots")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", RAGGED_SHAPES)
def test_halo_ragged_vs_oracle(kind, H, W):
    """The fused coefficient kernel with a ragged last strip (lanes past W, the right
    border pixel in the strip's last lane) in stacked bands == the C oracle."""
    rgb, exp = _case(kind, H, W)
    assert _lib.get_knob("encode_band") == 1
    enc = pipeline.Encoder(H, W, fused=True)
    assert enc.fused and not enc.slots
    enc.encode(device.to_device(rgb))
    _assert_equals_oracle(enc.result(), exp, "fused")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SLOT_SHAPES + RAGGED_SHAPES)
def test_halo_band_0_equals_1(kind, H, W):
    """encode_band 0 (one unit per wave, every wave its own 19 rows, encode_order 6)
    and 1 (stacked bands) give identical device outputs, both equal to the oracle's."""
    rgb, exp = _case(kind, H, W)
    x = device.to_device(rgb)
    out = {}
    try:
        for band in (0, 1):
            _lib.set_knob("encode_band", band)
            enc = pipeline.Encoder(H, W, fused=True)
            enc.encode(x)
            out[band] = (enc.result(), enc.counts.cpu().tolist())
    finally:
        _lib.set_knob("encode_band", -1)
    assert _lib.get_knob("encode_order") == 6
    assert out[0][1] == out[1][1]
    for k in pipeline.CHANNELS:
        for j in range(4):
            np.testing.assert_array_equal(out[0][0][k][j], out[1][0][k][j], err_msg=(k, j))
    _assert_equals_oracle(out[0][0], exp, "band 0")


@pytest.mark.parametrize("kind", KINDS)
def test_halo_shards_band_at_out_row0(kind):
    """Two row shards of 160 x 512 (sharding.ShardEncoder's plan and encoders, on one
    device): the second shard's out_row0 is 80, so a band starts there and its first
    unit's upper halo rows are the first shard's rows; stitched, the shards equal the
    whole-image encode and the oracle."""
    H, W, world = 160, 512, 2
    rgb, exp = _case(kind, H, W)
    ses = [sharding.ShardEncoder(H, W, rank=r, world=world) for r in range(world)]
    assert [se.rows for se in ses] == [(0, 80), (80, 160)]
    for se in ses:
        assert se.enc.fused
        a, b = se.span
        se.enc.transform(device.to_device(rgb[a:b]), in_row0=a)
    summ = np.stack([se.enc.shard_summaries().cpu().numpy() for se in ses])  # (world, 3, 4)
    allsum = device.to_device(summ)
    for r, se in enumerate(ses):
        st = device.zeros((3, 4), torch.int64)
        for c in range(3):
            _lib.call("hic_rle_stitch", ctypes.c_void_p(allsum.data_ptr() + 32 * c), world, r, 12,
                      device.ptr(st[c]), device.stream_ptr())
        se.enc.entropy(stitch=st)
    parts = [se.enc.result() for se in ses]
    got = {k: tuple(np.concatenate([p[k][j] for p in parts]) for j in range(4)) for k in pipeline.CHANNELS}
    _assert_equals_oracle(got, exp, "shards")
    whole = pipeline.Encoder(H, W)
    whole.encode(device.to_device(rgb))
    _assert_equals_oracle(whole.result(), exp, "whole")
