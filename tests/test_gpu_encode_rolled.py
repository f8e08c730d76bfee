"""Round 11's slot encoder (hiccup_amd/csrc/slots.h, encode.hip) against the C
oracle: the two rare emissions are out-of-line functions now (slot_block_wide,
slot_block_packed), the block summary comes from the even / odd nonzero masks
without their interleave (summarize_eo15) and ycc8 no longer clamps Cb.  Small
shapes, one strip or two, a short band (1, 2 or 4 unit rows) and a band plus a
short one; data that takes each path in BOTH Y block rows of a unit, with block
row 1 always different from block row 0 (so a pass that read the other row's
registers, record pointers or positions would show):
  random   dense blocks, the hot path alone;
  zero     every AC zero (grey levels that change per block row: the DCs differ);
  sparse   runs of >= 15 zeros inside blocks and carried across records: the
           out-of-line packed emission (checked on the oracle's blocks);
  wide     grey rows [255 255 0 0 0 0 255 255]: zig-zag slot 3 outside 12 bits in
           both Y block rows of every unit, the out-of-line direct emission, beside
           coloured blocks whose chroma must come out untouched;
  colours  only (0,0,255), (255,255,0) (the Cb extremes) and (255,0,0), (255,0,1),
           (255,0,2) (the three inputs at which the Cr clamp fires).
(The file is named after the rolled Y loop planned for the round; the loop was not
shipped, DESIGN.md §0 "Round 11", and these cases hold for either form.)
Reference: compression.jpeg_compression + codec.jpeg_encode's DC / AC coding, as
restated in oracle/hiccup_oracle.c."""
import functools

import numpy as np
import pytest

import oracle.oracle_c as orcc
from hiccup_amd import _lib, device, pipeline

pytestmark = pytest.mark.gpu

SHAPES = [(16, 512), (32, 512), (64, 512), (80, 1024)]
KINDS = ["random", "zero", "sparse", "wide", "colours"]
COLOURS = np.array([(0, 0, 255), (255, 255, 0), (255, 0, 0), (255, 0, 1), (255, 0, 2)], np.uint8)


def _img(kind, H, W):
    rng = np.random.default_rng(1000 * H + W)
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "zero":  # grey (Cr = Cb = 128), one level per Y block row
        lv = (40 + 23 * np.arange(H // 8)) % 256
        return np.broadcast_to(lv.repeat(8)[:, None, None], (H, W, 3)).astype(np.uint8).copy()
    if kind == "sparse":
        # flat, but a third of the blocks carry a horizontal ramp (low zig-zag slots)
        # plus the highest DCT basis function (the last slot): a long zero run between
        # them.  Every third 16-row unit stays flat but for one block per block row, so
        # runs cross records.
        y, x = np.mgrid[0:8, 0:8]
        top = np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)
        img = np.full((H, W), 128.0)
        for by in range(H // 8):
            for bx in range(W // 8):
                on = rng.random() < 1 / 3
                if (by // 2) % 3 == 2:
                    on = bx == 5 + by
                if on:
                    amp, hi = rng.integers(2, 6), rng.integers(30, 70)
                    img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] += amp * (x - 3.5) + hi * top
        g = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        return np.stack([g, g, g], -1)
    if kind == "wide":
        row = np.array([255, 255, 0, 0, 0, 0, 255, 255], np.uint8)
        g = np.tile(row, W // 8)[None, :].repeat(H, 0)
        flip = rng.integers(0, 2, (H // 8, W // 8)).repeat(8, 0).repeat(8, 1) == 1
        img = np.where(flip, g, 255 - g)[..., None].repeat(3, 2).astype(np.uint8)
        # coloured blocks in the same waves (every other 64 columns of a strip)
        col = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask = ((np.arange(W) // 64) % 2 == 1)[None, :, None]
        return np.where(mask, col, img)
    if kind == "colours":
        return COLOURS[rng.integers(0, len(COLOURS), (H, W))]
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """The image and the oracle's (zig-zag blocks, DC differences, lengths, values)
    per channel, computed once and left unchanged."""
    rgb = _img(kind, H, W)
    y, cr, cb = orcc.rgb_to_ycrcb(rgb)
    exp = {}
    for k, (p, t) in {"lum": (y, 0), "cr": (orcc.pyr_down(cr), 1), "cb": (orcc.pyr_down(cb), 1)}.items():
        zz = orcc.zigzag_blocks(orcc.dct_channel(p, t), 8)
        L, V = orcc.rle_encode(zz[:, 1:].reshape(-1), 15)
        exp[k] = (zz, orcc.dpcm(zz[:, 0].copy()), L, V)
    for v in exp.values():
        for a in v:
            a.setflags(write=False)
    rgb.setflags(write=False)
    return rgb, exp


def _inner_run15(zz_rows):
    """blocks (rows of zig-zag int) with >= 15 zeros between two nonzero AC"""
    out = np.zeros(len(zz_rows), bool)
    for i, b in enumerate(zz_rows):
        nz = np.flatnonzero(b[1:])
        out[i] = nz.size > 1 and np.diff(nz).max() > 15
    return out


def _check_data(kind, H, W, rgb, exp):
    """The data takes the path it is meant to, in both Y block rows of every unit,
    and block row 1 differs from block row 0."""
    nbx = W // 8
    lum = exp["lum"][0].reshape(H // 8, nbx, 64)
    for u in range(H // 16):
        assert not np.array_equal(lum[2 * u], lum[2 * u + 1]), u
    if kind == "zero":
        assert not exp["lum"][0][:, 1:].any() and not exp["cr"][0][:, 1:].any()
        assert all(exp[k][2].tolist() == [0] and exp[k][3].tolist() == [0] for k in pipeline.CHANNELS)
    if kind == "sparse":
        for br in range(H // 8):
            if (br // 2) % 3 != 2:
                assert _inner_run15(lum[br]).any(), br
        L = exp["lum"][2]
        assert (L[:-1] == 14).any() and not exp["lum"][0][:64, 1:].all()
    if kind == "wide":
        for br in range(H // 8):
            for s in range(W // 512):
                assert np.abs(lum[br, 64 * s:64 * s + 64, 3]).max() > 2047, (br, s)
        assert exp["cr"][0][:, 1:].any() and exp["cb"][0][:, 1:].any()
    if kind == "colours":
        y, cr, cb = orcc.rgb_to_ycrcb(rgb)
        assert cr.max() == 255 and cb.max() == 255 and cb.min() <= 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_slot_encoder_equals_oracle(kind, H, W):
    rgb, exp = _case(kind, H, W)
    _check_data(kind, H, W, rgb, exp)
    x = device.to_device(rgb.copy())
    for band in (1, 0):  # the stacked units of a band (default) and one unit per wave
        with _lib.knobs(encode_band=band):
            enc = pipeline.Encoder(H, W)
            assert enc.slots and enc.fused
            enc.encode(x)
            got = enc.result()
        for k in pipeline.CHANNELS:
            for j, what in enumerate(("coef", "dc", "sym_len", "sym_val")):
                np.testing.assert_array_equal(np.asarray(got[k][j]).astype(np.int64), exp[k][j],
                                              err_msg="%s %s band %d" % (k, what, band))
