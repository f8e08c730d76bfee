"""GPU tests of the batched region decode: pipeline.BatchRegionDecoder (one window per
image, n images, two launches, the luma store cropped into one dense tensor) against
the crop of each image's unchanged whole-image indexed decode and against the C oracle's
inverse chain, with guard bytes around and inside the result; codec.decode_regions
against the per-file loop."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.oracle as orc  # noqa: E402
import oracle.oracle_c as orcc  # noqa: E402
from hiccup_amd import codec, device, pipeline  # noqa: E402

# the region tests' shapes -- (64, 1024): luma 2 tiles per block row; (48, 1536): chroma
# tiles wrap rows inside the slot layout; (80, 208): every tile wraps; (96, 1040): nbx
# 130 / 65; (16, 16): one chroma block
SHAPES = [(64, 1024, True), (48, 1536, True), (80, 208, False), (96, 1040, False), (16, 16, False)]
# the images of a batch differ: three seeds, zero runs carried from far before the
# window, a stream that is a single EOB.  A batch of n takes the first n.
IMAGES = ["random0", "flat", "all128", "random1", "random2"]
CANARY = 0xA5
GUARD = 64


def _rgb(kind, H, W):
    if kind.startswith("random"):
        return np.random.default_rng(H * 31 + W + 1000 * int(kind[6:])).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img = np.full((H, W, 3), 128, np.uint8)
    if kind == "flat":
        img[H // 2:H // 2 + 3, W // 3] = 7
    return img


@functools.lru_cache(maxsize=None)
def _encoded(H, W):
    """Per image of IMAGES (its encoder, its whole-image indexed decode, that decode's
    chroma planes): computed once per shape and left unchanged."""
    out = []
    for kind in IMAGES:
        enc = pipeline.Encoder(H, W, index=True)
        enc.encode(device.to_device(_rgb(kind, H, W)))
        dec = pipeline.Decoder(H, W)
        full = dec.decode(enc.sym_len, enc.sym_val, enc.counts, enc.dc, index=enc.index).clone()
        dec.check_status()
        out.append((enc, full, dec.pix["cr"].clone(), dec.pix["cb"].clone()))
    return out


def _windows(H, W):
    return list(dict.fromkeys((min(h, H), min(w, W)) for h, w in ((1, 1), (16, 16), (21, 35), (H, W))))


def _origins(H, W, h, w, n, turn=0):
    """Per image a different origin: 16-aligned, (5, 13), the far corner, x0 across luma
    block column 64 (in 490..500) where W allows, one touching no edge; clipped into the
    image, rotated by `turn`."""
    my, mx = H - h, W - w
    o = [(min(16, my) // 16 * 16, min(32, mx) // 16 * 16), (min(5, my), min(13, mx)), (my, mx),
         (min(3, my), 493 if mx >= 493 else mx // 2), (min(17, max(my - 1, 0)), min(19, max(mx - 1, 0)))]
    return [o[(i + turn) % 5] for i in range(n)]


def _guarded(n, h, w, pad):
    """An (n, h, w, 3) view inside a canary-filled buffer: GUARD bytes before and after,
    `pad` bytes after every pixel row (pad odd: every row base misaligned) and one more
    odd gap between images."""
    row = 3 * w + pad
    img = h * row + (7 if pad else 0)
    buf = torch.full((GUARD + n * img + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    return buf, buf.as_strided((n, h, w, 3), (img, row, 3, 1), GUARD)


def _check(dec, buf, view, enc, origins, skip=()):
    """Every byte of the guarded buffer (the crops where they belong, the canary everywhere
    else), of the chroma window buffers (each image's planned span, the canary beyond) and
    of the status words."""
    n, h, w = dec.n, dec.h, dec.w
    want, want_view = _guarded(n, h, w, view.stride(1) - 3 * w)
    wcr, wcb = torch.full_like(dec.cr, CANARY), torch.full_like(dec.cb, CANARY)
    status = dec.expected_status()
    for i, (y0, x0) in enumerate(origins):
        if i in skip:
            status[i] = [-1, -1, -1]
            continue
        _, full, cr, cb = enc[i]
        want_view[i] = full[y0:y0 + h, x0:x0 + w]
        p = pipeline.window_plan(dec.H, dec.W, y0, x0, h, w)
        wcr[i, :p.ch, :p.cw] = cr[p.cy0:p.cy0 + p.ch, p.cx0:p.cx0 + p.cw]
        wcb[i, :p.ch, :p.cw] = cb[p.cy0:p.cy0 + p.ch, p.cx0:p.cx0 + p.cw]
    what = (n, h, w, origins)
    assert torch.equal(view, want_view), what
    assert torch.equal(buf, want), "a guard byte changed: %r" % (what,)
    assert torch.equal(dec.cr, wcr) and torch.equal(dec.cb, wcb), what
    assert dec.status.cpu().tolist() == status, what


def _fresh(dec, buf):
    for b in (buf, dec.cr, dec.cb):
        b.fill_(CANARY)
    dec.status.fill_(-7)


@pytest.mark.parametrize("H,W,slots", SHAPES)
def test_batch_region_equals_crops_of_full_decodes(H, W, slots):
    enc = _encoded(H, W)
    assert all(e[0].slots == slots for e in enc)
    for n in (1, 2, 5):
        for k, (h, w) in enumerate(_windows(H, W)):
            for pad in (0, 5):
                buf, view = _guarded(n, h, w, pad)
                dec = pipeline.BatchRegionDecoder(n, H, W, h, w, out=view)
                _fresh(dec, buf)
                origins = _origins(H, W, h, w, n, turn=k + n)
                got = dec.decode([e[0] for e in enc[:n]], origins)
                assert got is view and tuple(got.shape) == (n, h, w, 3)
                _check(dec, buf, view, enc, origins)
                dec.check_status()
    # the decoder's own dense result
    dec = pipeline.BatchRegionDecoder(5, H, W, *_windows(H, W)[-2])
    origins = _origins(H, W, dec.h, dec.w, 5)
    got = dec.decode([e[0] for e in enc], origins)
    assert got.is_contiguous() and tuple(got.shape) == (5, dec.h, dec.w, 3)
    for i, (y0, x0) in enumerate(origins):
        assert torch.equal(got[i], enc[i][1][y0:y0 + dec.h, x0:x0 + dec.w]), i


@pytest.mark.parametrize("H,W,slots", [(64, 1024, True), (80, 208, False)])
def test_batch_region_equals_oracle_inverse_chain(H, W, slots):
    """Not only this repository's own decoder: the crops against the C oracle's
    dequantize + IDCT, pyrUp and YCrCb -> RGB of the oracle-checked blocks."""
    enc = _encoded(H, W)[:2]
    exp = []
    for e, _, _, _ in enc:
        assert e.slots == slots
        got, planes = e.result(), {}
        for k, (ph, pw, t) in {"lum": (H, W, 0), "cr": (H // 2, W // 2, 1), "cb": (H // 2, W // 2, 1)}.items():
            zz = got[k][0].astype(np.int32)
            raster = orc.merge_blocks(zz[:, np.argsort(orc.ZZ8)].reshape(-1, 8, 8), (ph, pw))
            planes[k] = orcc.inv_dct_channel(raster, t)
        exp.append(orcc.ycrcb_to_rgb(planes["lum"], orcc.pyr_up(planes["cr"]), orcc.pyr_up(planes["cb"])))
    for k, (h, w) in enumerate(_windows(H, W)):
        dec = pipeline.BatchRegionDecoder(2, H, W, h, w)
        origins = _origins(H, W, h, w, 2, turn=k + 1)
        got = dec.decode([e[0] for e in enc], origins).cpu().numpy()
        for i, (y0, x0) in enumerate(origins):
            np.testing.assert_array_equal(got[i], exp[i][y0:y0 + h, x0:x0 + w], err_msg=str((h, w, i, y0, x0)))


@pytest.mark.parametrize("H,W,slots", [(64, 1024, True), (96, 1040, False)])
def test_batch_region_failed_count_in_the_middle(H, W, slots):
    """One image in the middle of the batch with a failed encode's counts (< 1): its
    status row is -1, its pixels and chroma buffers keep the canary, the others are right."""
    enc = _encoded(H, W)
    h, w = 21, 35
    buf, view = _guarded(5, h, w, 5)
    dec = pipeline.BatchRegionDecoder(5, H, W, h, w, out=view)
    _fresh(dec, buf)
    e = enc[2][0]
    sources = [x[0] for x in enc]
    sources[2] = (e.sym_len, e.sym_val, torch.zeros_like(e.counts), e.dc, e.index)
    origins = _origins(H, W, h, w, 5, turn=1)
    dec.decode(sources, origins)
    _check(dec, buf, view, enc, origins, skip={2})
    assert bool((view[2] == CANARY).all()) and bool((dec.cr[2] == CANARY).all()) and bool((dec.cb[2] == CANARY).all())
    with pytest.raises(ValueError):
        dec.check_status()


def test_batch_region_refusals():
    H, W = 64, 1024
    enc = [e[0] for e in _encoded(H, W)]
    other = pipeline.Encoder(H, W, index=True, slots=False)
    other.encode(device.to_device(_rgb("random1", H, W)))
    dec = pipeline.BatchRegionDecoder(2, H, W, 21, 35)
    with pytest.raises(ValueError):
        dec.decode([enc[0], other], [(0, 0), (0, 0)])  # mixed kinds
    with pytest.raises(ValueError):
        dec.decode(enc[:3], [(0, 0)] * 3)  # wrong n
    with pytest.raises(ValueError):
        dec.decode(enc[:2], [(0, 0)])  # wrong number of origins
    for bad in ((H - 20, 0), (0, W - 34), (-1, 0)):
        with pytest.raises(ValueError):
            dec.decode(enc[:2], [(0, 0), bad])  # a window outside the second image
    for h, w in ((H + 1, 35), (21, W + 1), (0, 35)):
        with pytest.raises(ValueError):
            pipeline.BatchRegionDecoder(2, H, W, h, w)  # a window too large
    with pytest.raises(ValueError):
        pipeline.BatchRegionDecoder(2, H, W, 21, 35, out=torch.empty((2, 21, 36, 3), dtype=torch.uint8, device="cuda"))
    # the decoder still works after the refusals
    got = dec.decode(enc[:2], [(5, 13), (H - 21, W - 35)])
    assert torch.equal(got[1], _encoded(H, W)[1][1][H - 21:, W - 35:])


@pytest.mark.parametrize("H,W,slots", [(64, 1024, True), (80, 208, False)])
def test_batch_region_cached_sources_then_a_replaced_one(H, W, slots):
    enc = _encoded(H, W)
    n, h, w = 5, 21, 35
    buf, view = _guarded(n, h, w, 0)
    dec = pipeline.BatchRegionDecoder(n, H, W, h, w, out=view)
    sources = [e[0] for e in enc]
    for turn in (0, 2):  # the second call: the same Encoder objects, new origins
        _fresh(dec, buf)
        origins = _origins(H, W, h, w, n, turn=turn)
        if turn:
            assert dec._resolve(sources) is None  # the addresses are not read again
        dec.decode(sources, origins)
        _check(dec, buf, view, enc, origins)
    # image 1's source replaced by image 3's encoder
    swapped = list(sources)
    swapped[1] = sources[3]
    _fresh(dec, buf)
    origins = _origins(H, W, h, w, n, turn=4)
    dec.decode(swapped, origins)
    _check(dec, buf, view, [enc[0], enc[3]] + enc[2:], origins)


def _outcome(f):
    try:
        return ("ok", f())
    except Exception as e:  # noqa: BLE001 -- compared below
        return (type(e), str(e))


def test_codec_decode_regions(monkeypatch):
    h, w = 21, 35
    rgbs = [_rgb("random0", 80, 208), _rgb("random1", 64, 1024), _rgb("random2", 80, 208), _rgb("random2", 64, 1024),
            _rgb("random1", 80, 208), _rgb("flat", 80, 208)]
    files = [codec.encode(a) for a in rgbs]
    origins = [(5, 13), (64 - h, 1024 - w), (80 - h, 208 - w), (3, 493), (16, 32), (33, 60)]
    exp = np.stack([codec.decode_region(f, y0, x0, h, w) for f, (y0, x0) in zip(files, origins)])
    got = codec.decode_regions(files, origins, h, w)  # a list mixing two shapes
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (6, h, w, 3)
    np.testing.assert_array_equal(got, exp)
    # OpenImages passed directly, one shape: one batch, straight into the result
    opened = [codec.open(files[i]) for i in (0, 2, 4)]
    assert all(o._streams is not None for o in opened)
    dev = codec.decode_regions_device(opened, [origins[i] for i in (0, 2, 4)], h, w)
    assert dev.is_cuda and tuple(dev.shape) == (3, h, w, 3)
    np.testing.assert_array_equal(dev.cpu().numpy(), exp[[0, 2, 4]])
    # a file of a shape that is no multiple of 16 is not the fast path's: whatever the
    # per-file loop gives for the list -- its result, or the exception it raises
    ragged = codec.encode(_rgb("random2", 250, 330))
    lists = ([files[0], ragged, files[1]], [(5, 13), (7, 200), (3, 493)])
    loop = _outcome(lambda: np.stack([codec.decode_region(f, y0, x0, h, w) for f, (y0, x0) in zip(*lists)]))
    both = _outcome(lambda: codec.decode_regions(*lists, h, w))
    assert both[0] == loop[0]
    if loop[0] == "ok":
        np.testing.assert_array_equal(both[1], loop[1])
    else:
        assert both[1] == loop[1]
    # images that took OpenImage's whole-decode fallback are served per image, beside a batch
    with monkeypatch.context() as m:
        m.setattr(codec, "_fast_streams", lambda f: None)
        slow = [codec.open(files[i]) for i in (1, 2)]
    assert all(o._streams is None for o in slow)
    mixed = [opened[0], slow[0], opened[1], slow[1], files[4]]
    np.testing.assert_array_equal(codec.decode_regions(mixed, [origins[i] for i in (0, 1, 2, 2, 4)], h, w),
                                  exp[[0, 1, 2, 2, 4]])
    for bad in ((80 - h + 1, 0), (0, 208 - w + 1), (-1, 0)):
        with pytest.raises(ValueError):
            codec.decode_regions(files[:3], [(0, 0), (0, 0), bad], h, w)  # outside the third image
        with pytest.raises(ValueError):
            codec.decode_regions(opened, [(0, 0), bad, (0, 0)], h, w)
    with pytest.raises(ValueError):
        codec.decode_regions(files[:2], [(0, 0)], h, w)
    with pytest.raises(ValueError):
        codec.decode_regions(files[:1], [(0, 0)], 0, w)
