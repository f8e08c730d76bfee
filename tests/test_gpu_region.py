"""GPU tests of region decode: pipeline.RegionDecoder (the window forms of the fused
tile decoders, both stream kinds) against the crop of the unchanged whole-image
indexed decode and against the C oracle's inverse chain; pipeline.stream_index against
the encoder's own tile index; codec.open / codec.decode_region against codec.decode."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.oracle as orc  # noqa: E402
import oracle.oracle_c as orcc  # noqa: E402
from hiccup_amd import codec, device, pipeline  # noqa: E402

# (64, 1024): luma 2 tiles per block row, chroma 1 tile = 2 records; (48, 1536): chroma
# nbx 96, tiles wrap rows inside the slot layout; (80, 208): nbx 26 / 13, every tile
# wraps; (96, 1040): nbx 130 / 65; (16, 16): one chroma block
SHAPES = [(64, 1024, True), (48, 1536, True), (80, 208, False), (96, 1040, False), (16, 16, False)]
KINDS = ["random", "levels", "flat"]
CANARY = 0xA5


def _rgb(kind, H, W):
    rng = np.random.default_rng(H * 31 + W)
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "levels":  # 4 grey levels: exact quantiser ties
        return (rng.integers(0, 4, (H, W, 1)) * 85).astype(np.uint8).repeat(3, 2)
    if kind == "flat":  # zero runs carried from far before most windows
        img = np.full((H, W, 3), 128, np.uint8)
        img[H // 2:H // 2 + 3, W // 3] = 7
        return img
    if kind == "all128":  # every coefficient zero: the stream is one EOB
        return np.full((H, W, 3), 128, np.uint8)
    raise ValueError(kind)


def _windows(H, W):
    ws = [(0, 0, H, W), (0, 0, 16, 16), (0, W - 16, 16, 16), (H - 16, 0, 16, 16), (H - 16, W - 16, 16, 16)]
    if H >= 48 and W >= 48:
        ws.append((16, 16, 16, 16))  # touches no edge
    x0 = 496 if W >= 544 else max(0, W // 2 // 16 * 16 - 16)  # across luma block column 64 where there is one
    ws.append((min(16, H - 16), x0, 16, min(48, W - x0)))
    ws.append((5, 13, min(21, H - 5), min(35, W - 13)))  # unaligned
    ws.append((8 if H >= 16 else 0, 0, 8, W))  # one full-width block row
    ws.append((0, 32 if W >= 48 else 0, H, 16))  # one full-height 16-pixel column
    ws.append((H - 1, W - 1, 1, 1))
    return list(dict.fromkeys(ws))


@functools.lru_cache(maxsize=None)
def _encoded(kind, H, W):
    """(the encoder, the whole-image indexed decode and its chroma planes): computed
    once per image and left unchanged."""
    enc = pipeline.Encoder(H, W, index=True)
    enc.encode(device.to_device(_rgb(kind, H, W)))
    dec = pipeline.Decoder(H, W)
    full = dec.decode(enc.sym_len, enc.sym_val, enc.counts, enc.dc, index=enc.index).clone()
    dec.check_status()
    return enc, full, dec.pix["cr"].clone(), dec.pix["cb"].clone()


def _region(rd, enc, win, counts=None):
    for b in (rd.rgb, rd.cr, rd.cb):
        b.fill_(CANARY)
    return rd.decode(*win, enc.sym_len, enc.sym_val, enc.counts if counts is None else counts, enc.dc, enc.index)


def _untouched(t):
    return bool((t == CANARY).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,slots", SHAPES)
def test_region_equals_crop_of_full_decode(H, W, slots, kind):
    enc, full, cr, cb = _encoded(kind, H, W)
    assert enc.slots == slots
    rd = pipeline.RegionDecoder(H, W, H, W)
    for win in _windows(H, W):
        y0, x0, h, w = win
        got = _region(rd, enc, win)
        assert tuple(got.shape) == (h, w, 3)
        assert torch.equal(got, full[y0:y0 + h, x0:x0 + w]), win
        p = rd.plan
        assert tuple(p) == tuple(pipeline.window_plan(H, W, *win))
        # the whole aligned window is written, and is the reference's (on a random image
        # no byte of it can keep the canary by accident) ...
        assert torch.equal(rd.window(), full[p.Y0:p.Y1, p.X0:p.X1]), win
        gcr, gcb = rd.chroma()
        assert torch.equal(gcr, cr[p.cy0:p.cy0 + p.ch, p.cx0:p.cx0 + p.cw]), win
        assert torch.equal(gcb, cb[p.cy0:p.cy0 + p.ch, p.cx0:p.cx0 + p.cw]), win
        # ... and no byte outside it / outside the planned chroma span
        assert _untouched(rd.rgb[rd.window().numel():]), win
        assert _untouched(rd.cr[p.ch * p.cw:]) and _untouched(rd.cb[p.ch * p.cw:]), win
        # 63 AC positions per block of each launch's window
        assert rd.status.cpu().tolist() == rd.expected_status(), win
        assert rd.expected_status()[0] == (p.Y1 - p.Y0) * (p.X1 - p.X0) // 64 * 63
        rd.check_status()


def test_region_decoder_capacity():
    """A decoder sized for small windows: its buffers are the capacity formula's, hold the
    worst-placed request, and larger requests are refused."""
    H, W = 96, 1040
    enc, full, _, _ = _encoded("random", H, W)
    rd = pipeline.RegionDecoder(H, W, 20, 40)
    (wh, ww), (ch, cw) = pipeline.region_capacity(H, W, 20, 40)
    assert rd.rgb.numel() == wh * ww * 3 and rd.cr.numel() == rd.cb.numel() == ch * cw
    assert rd.rgb.numel() < H * W * 3 // 16
    for win in ((15, 15, 20, 40), (0, 0, 20, 40), (76, 1000, 20, 40), (31, 527, 18, 34), (47, 1023, 1, 1)):
        y0, x0, h, w = win
        assert torch.equal(_region(rd, enc, win), full[y0:y0 + h, x0:x0 + w]), win
        assert _untouched(rd.rgb[rd.window().numel():])
    for win in ((0, 0, 21, 40), (0, 0, 20, 41)):
        with pytest.raises(ValueError):
            rd.decode(*win, enc.sym_len, enc.sym_val, enc.counts, enc.dc, enc.index)
    with pytest.raises(ValueError):
        rd.decode(90, 0, 20, 40, enc.sym_len, enc.sym_val, enc.counts, enc.dc, enc.index)  # outside the image


@pytest.mark.parametrize("H,W,slots", [(64, 1024, True), (80, 208, False)])
def test_region_equals_oracle_inverse_chain(H, W, slots):
    """Not only this repository's own decoder: the windows against the C oracle's
    dequantize + IDCT, pyrUp and YCrCb -> RGB of the oracle-checked blocks."""
    rgb = _rgb("random", H, W)
    enc = pipeline.Encoder(H, W, index=True)
    assert enc.slots == slots
    enc.encode(device.to_device(rgb))
    got = enc.result()
    planes = {}
    for k, (h, w, t) in {"lum": (H, W, 0), "cr": (H // 2, W // 2, 1), "cb": (H // 2, W // 2, 1)}.items():
        zz = got[k][0].astype(np.int32)
        raster = orc.merge_blocks(zz[:, np.argsort(orc.ZZ8)].reshape(-1, 8, 8), (h, w))
        planes[k] = orcc.inv_dct_channel(raster, t)
    exp = orcc.ycrcb_to_rgb(planes["lum"], orcc.pyr_up(planes["cr"]), orcc.pyr_up(planes["cb"]))
    rd = pipeline.RegionDecoder(H, W, H, W)
    for win in _windows(H, W):
        y0, x0, h, w = win
        np.testing.assert_array_equal(_region(rd, enc, win).cpu().numpy(), exp[y0:y0 + h, x0:x0 + w], err_msg=str(win))


@pytest.mark.parametrize("H,W,slots", [(64, 1024, True), (80, 208, False)])
def test_region_failed_count(H, W, slots):
    """A failed encode's symbol count (< 1): status -1 for that channel and none of its
    launch's output written; the other channels report their windows as usual."""
    enc, _, _, _ = _encoded("random", H, W)
    rd = pipeline.RegionDecoder(H, W, H, W)
    win = (5, 13, 21, 35)
    for ch in range(3):
        counts = enc.counts.clone()
        counts[ch] = 0
        _region(rd, enc, win, counts)
        want = rd.expected_status()
        want[ch] = -1
        assert rd.status.cpu().tolist() == want, ch
        assert _untouched((rd.rgb, rd.cr, rd.cb)[ch]), ch
        for other in {1, 2} - {ch}:
            assert not _untouched((rd.rgb, rd.cr, rd.cb)[other][:rd.plan.ch * rd.plan.cw])
        with pytest.raises(ValueError):
            rd.check_status()


_IX_SHAPES = [(80, 208), (96, 1040), (16, 16), (250, 330), (8, 8), (512, 1024)]


@pytest.mark.parametrize("kind", KINDS + ["all128"])
@pytest.mark.parametrize("H,W", _IX_SHAPES)
def test_stream_index_equals_encoder_index(H, W, kind):
    """The index built from the bare stream equals the emit's own, word for word, and
    its status is the un-indexed decode's; decoding with it equals the plain decode."""
    enc = pipeline.Encoder(H, W, index=True, slots=False)
    enc.encode(device.to_device(_rgb(kind, H, W)))
    counts = enc.counts.cpu().tolist()
    assert min(counts) >= 1
    if kind == "all128":
        assert counts == [1, 1, 1]
    index, status = pipeline.stream_index(enc.sym_len, enc.sym_val, counts, enc.dc, H, W)
    nblk = [enc.coef[k].shape[0] for k in pipeline.CHANNELS]
    assert status.cpu().tolist() == [n * 63 for n in nblk]
    for k in pipeline.CHANNELS:
        assert index[k].shape == enc.index[k].shape
        assert torch.equal(index[k], enc.index[k]), (k, index[k].view(-1, 3)[:8], enc.index[k].view(-1, 3)[:8])
    plain = pipeline.Decoder(H, W)
    exp = plain.decode(enc.sym_len, enc.sym_val, counts, enc.dc).clone()
    plain.check_status()
    dec = pipeline.Decoder(H, W)
    got = dec.decode(enc.sym_len, enc.sym_val, enc.counts, enc.dc, index=index)
    dec.check_status()
    assert torch.equal(got, exp)


def test_stream_index_status_of_a_short_stream():
    """A stream without its EOB that stops early reports its own length, as
    hic_rle_decode_i16 does."""
    H, W = 80, 208
    enc = pipeline.Encoder(H, W, index=True, slots=False)
    enc.encode(device.to_device(_rgb("random", H, W)))
    counts = enc.counts.cpu().tolist()
    cut = [c // 2 for c in counts]
    _, status = pipeline.stream_index(enc.sym_len, enc.sym_val, cut, enc.dc, H, W)
    dec = pipeline.Decoder(H, W)
    dec.decode(enc.sym_len, enc.sym_val, cut, enc.dc)
    assert status.cpu().tolist() == dec.status.cpu().tolist()
    assert status.cpu().tolist() != [enc.coef[k].shape[0] * 63 for k in pipeline.CHANNELS]


def _outcome(f):
    try:
        return ("ok", f())
    except Exception as e:  # noqa: BLE001 -- compared below
        return (type(e), str(e))


@pytest.mark.parametrize("H,W", [(64, 1024), (80, 208), ("lenna", 0)])
def test_codec_open_and_decode_region(H, W, golden_lenna):
    rgb = golden_lenna["rgb"] if H == "lenna" else _rgb("random", H, W)
    H, W = rgb.shape[:2]
    hic = codec.encode(rgb)
    full = codec.decode(hic)
    o = codec.open(hic)
    assert o._streams is not None  # the device-resident path, not the whole-image fallback
    assert o.shape == full.shape
    for win in _windows(H, W):
        y0, x0, h, w = win
        got = o.decode_region(*win)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, full[y0:y0 + h, x0:x0 + w], err_msg=str(win))
        dev = o.decode_region_device(*win)
        assert dev.is_cuda and tuple(dev.shape) == (h, w, 3)
        np.testing.assert_array_equal(dev.cpu().numpy(), full[y0:y0 + h, x0:x0 + w], err_msg=str(win))
    np.testing.assert_array_equal(o.decode(), full)
    for win in ((5, 13, min(21, H - 5), min(35, W - 13)), (H - 1, W - 1, 1, 1)):
        y0, x0, h, w = win
        np.testing.assert_array_equal(codec.decode_region(hic, *win), full[y0:y0 + h, x0:x0 + w])
    for win in ((0, 0, H + 1, 1), (-1, 0, 1, 1), (0, W, 1, 1), (0, 0, 0, 1)):
        with pytest.raises(ValueError):
            o.decode_region(*win)
        with pytest.raises(ValueError):
            codec.decode_region(hic, *win)


def test_codec_decode_region_ragged_fallback():
    """(250, 330) is not the fast path's: decode_region is the crop of whatever
    codec.decode gives for the file -- its result, or the exception it raises."""
    rgb = _rgb("random", 250, 330)
    hic = codec.encode(rgb)
    exp = _outcome(lambda: codec.decode(hic)[5:26, 13:48])
    for f in (lambda: codec.decode_region(hic, 5, 13, 21, 35), lambda: codec.open(hic).decode_region(5, 13, 21, 35)):
        got = _outcome(f)
        assert got[0] == exp[0]
        if exp[0] == "ok":
            np.testing.assert_array_equal(got[1], exp[1])
        else:
            assert got[1] == exp[1]
    if exp[0] == "ok":
        assert codec.open(hic)._streams is None
        np.testing.assert_array_equal(codec.open(hic).decode(), codec.decode(hic))
