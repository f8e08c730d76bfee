"""The batched decode (pipeline.BatchDecoder: hic_decode420_batch_u8, two launches for
n images of one shape) leaves, per image and bit for bit, what n one-image
Decoder(H, W).decode(..., index=...) calls leave on the same streams: the RGB pixels,
the Cr / Cb planes and the status words.  Image i is _img(KINDS[i % 7], ...) with its
own seed, so an all-zero and a sparse image sit between noisy ones: a carried zero
run or a DC chain must not leak across images.  The shapes are the smallest at which
each mechanism can go wrong (see SHAPES).  Reference: codec.jpeg_decode's RLE / DC /
izigzag half (codec.py:397-425) + compression.jpeg_decompression (compression.py:42-56)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle.oracle as orc
import oracle.oracle_c as orcc
from hiccup_amd import _lib, codec, device, hicimage, pipeline
from test_gpu_slots import KINDS, _img

pytestmark = pytest.mark.gpu

SLOTS, INDEXED = "slots", "indexed"
SHAPES = [
    (1, 16, 512, SLOTS),     # chroma is one half tile (32 live lanes); Y is 2 tiles
    (5, 16, 512, SLOTS),     # 1 chroma tile per plane: every chroma workgroup straddles images, the last is partly empty
    (3, 80, 1024, SLOTS),    # chroma is 5 tiles per plane: the Cr / Cb boundary falls inside a workgroup
    (2, 4112, 512, SLOTS),   # many tiles per image
    (3, 48, 80, INDEXED),    # Y one partial tile (60 blocks), chroma 15 blocks: three images in one workgroup, dead lanes
    (4, 16, 16, INDEXED),    # one block per chroma plane
    (2, 96, 1040, INDEXED),  # tiles that wrap block rows
]
CANARY = 0xA5


def _images(n, H, W, salt=0):
    return np.stack([_img(KINDS[i % 7], H, W, 1000 * salt + 31 * i + H + W) for i in range(n)])


def _decode_one(enc, counts=None):
    """(rgb, cr, cb, status) of a fresh one-image Decoder on the encoder's streams."""
    dec = pipeline.Decoder(enc.H, enc.W)
    rgb = dec.decode(enc.sym_len, enc.sym_val, enc.counts if counts is None else counts, enc.dc, index=enc.index)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), dec.pix["cr"].cpu().numpy(), dec.pix["cb"].cpu().numpy(), dec.status.cpu().tolist()


@functools.lru_cache(maxsize=None)
def _encoded(n, H, W, kind, salt=0):
    """(host images, the n encoders holding their streams, the per-image reference
    decodes): computed once per case and left unchanged.  slots: one BatchEncoder's
    encoders; indexed: n Encoder(index=True)."""
    imgs = _images(n, H, W, salt)
    if kind == SLOTS:
        batch = pipeline.BatchEncoder(n, H, W)
        batch.encode(device.to_device(imgs))
        src, encs = batch, batch.encoders
    else:
        encs = [pipeline.Encoder(H, W, index=True, slots=False) for _ in range(n)]
        for e, x in zip(encs, imgs):
            e.encode(device.to_device(x))
        src = encs
    torch.cuda.synchronize()
    assert all(e.slots == (kind == SLOTS) for e in encs)
    return imgs, src, [_decode_one(e) for e in encs]


def _assert_batch(dec, refs, msg, skip=()):
    torch.cuda.synchronize()
    rgb, cr, cb, st = dec.rgb.cpu().numpy(), dec.cr.cpu().numpy(), dec.cb.cpu().numpy(), dec.status.cpu().tolist()
    for i, ref in enumerate(refs):
        if i in skip:
            continue
        np.testing.assert_array_equal(rgb[i], ref[0], err_msg="%s image %d rgb" % (msg, i))
        np.testing.assert_array_equal(cr[i], ref[1], err_msg="%s image %d cr" % (msg, i))
        np.testing.assert_array_equal(cb[i], ref[2], err_msg="%s image %d cb" % (msg, i))
        assert st[i] == ref[3], "%s image %d status" % (msg, i)


def _poison(dec):
    for b in (dec.rgb, dec.cr, dec.cb):
        b.fill_(CANARY)
    dec.status.fill_(-7)


@pytest.mark.parametrize("n,H,W,kind", SHAPES)
def test_batch_equals_per_image_decoder(n, H, W, kind):
    imgs, src, refs = _encoded(n, H, W, kind)
    dec = pipeline.BatchDecoder(n, H, W)
    assert tuple(dec.rgb.shape) == (n, H, W, 3) and tuple(dec.cr.shape) == tuple(dec.cb.shape) == (n, H // 2, W // 2)
    assert tuple(dec.status.shape) == (n, 3)
    _poison(dec)
    out = dec.decode(src)
    assert out.data_ptr() == dec.rgb.data_ptr()
    _assert_batch(dec, refs, "first")
    dec.check_status()
    assert dec.status.cpu().tolist() == [dec.expected_status()] * n
    # the references are the decodes of what was encoded: lossy, but close to the images
    assert np.abs(refs[0][0].astype(int) - imgs[0]).mean() < 64


@pytest.mark.parametrize("n,H,W,kind", [(3, 80, 1024, SLOTS), (3, 48, 80, INDEXED)])
def test_batch_table_reuse_and_rebuild(n, H, W, kind):
    """The same sources after a second encode with other images (the table is reused: the
    addresses are the same), then n separate encoders at other addresses (rebuilt)."""
    imgs = _images(n, H, W, salt=1)
    if kind == SLOTS:
        src = pipeline.BatchEncoder(n, H, W)
        encode = lambda x: src.encode(device.to_device(x))  # noqa: E731
        encs = src.encoders
    else:
        src = encs = [pipeline.Encoder(H, W, index=True, slots=False) for _ in range(n)]
        encode = lambda x: [e.encode(device.to_device(y)) for e, y in zip(encs, x)]  # noqa: E731
    dec = pipeline.BatchDecoder(n, H, W)
    encode(imgs)
    dec.decode(src)
    _assert_batch(dec, [_decode_one(e) for e in encs], "first")
    table = dec._d_table.data_ptr()
    other = _images(n, H, W, salt=2)
    assert not np.array_equal(imgs, other)
    encode(other)
    _poison(dec)
    dec.decode(src)
    refs = [_decode_one(e) for e in encs]
    _assert_batch(dec, refs, "second encode")
    assert dec._d_table.data_ptr() == table, "the table was rebuilt for unchanged addresses"
    assert not np.array_equal(refs[0][0], _encoded(n, H, W, kind)[2][0][0])
    # n separate encoders at other addresses
    sep = [pipeline.Encoder(H, W, index=True, slots=None if kind == SLOTS else False) for _ in range(n)]
    for e, x in zip(sep, imgs):
        e.encode(device.to_device(x))
    key = dec._key
    _poison(dec)
    dec.decode(sep)
    assert dec._key != key
    _assert_batch(dec, [_decode_one(e) for e in sep], "separate encoders")
    dec.check_status()
    # ... and as the tuples Decoder.decode takes
    _poison(dec)
    dec.decode([(e.sym_len, e.sym_val, e.counts, e.dc, e.index) for e in sep])
    _assert_batch(dec, [_decode_one(e) for e in sep], "tuples")


@pytest.mark.parametrize("n,H,W,kind", [
    (3, 80, 1024, SLOTS),
    (3, 48, 80, INDEXED),
    (2, 96, 1040, INDEXED),  # tiles that wrap block rows, a partial last tile
    (1, 16, 512, SLOTS),     # chroma is one half tile: dead lanes in the RGB form
])
def test_batch_equals_oracle_inverse_chain(n, H, W, kind):
    """Independent of the project's own decoder: the C oracle's dequantize + IDCT, pyrUp
    and YCrCb -> RGB of each image's blocks.  Image 0 from a one-image Decoder against
    the same: the batch and the one-image kernels run one tile body, so their equality
    alone does not check it."""
    _, src, refs = _encoded(n, H, W, kind)
    dec = pipeline.BatchDecoder(n, H, W)
    got = dec.decode(src).cpu().numpy()
    dec.check_status()
    encs = src.encoders if kind == SLOTS else src
    for i, enc in enumerate(encs):
        res = enc.result()
        planes = {}
        for k, (h, w, t) in {"lum": (H, W, 0), "cr": (H // 2, W // 2, 1), "cb": (H // 2, W // 2, 1)}.items():
            zz = res[k][0].astype(np.int32)
            raster = orc.merge_blocks(zz[:, np.argsort(orc.ZZ8)].reshape(-1, 8, 8), (h, w))
            planes[k] = orcc.inv_dct_channel(raster, t)
        exp = orcc.ycrcb_to_rgb(planes["lum"], orcc.pyr_up(planes["cr"]), orcc.pyr_up(planes["cb"]))
        np.testing.assert_array_equal(got[i], exp, err_msg="image %d" % i)
        if i == 0:
            np.testing.assert_array_equal(refs[0][0], exp, err_msg="one-image Decoder, image 0")


@pytest.mark.parametrize("n,H,W,kind", [(3, 80, 1024, SLOTS), (3, 48, 80, INDEXED)])
def test_c_abi_strides_and_canaries(n, H, W, kind):
    """Through the C-ABI: per-image RGB bases with gap rows between the images, padded RGB
    and chroma strides; every pixel equals the reference and every gap and pad byte
    still holds the canary."""
    _, src, refs = _encoded(n, H, W, kind)
    encs = src.encoders if kind == SLOTS else src
    rs, cs, gap = 3 * W + 8, W // 2 + 4, 2
    rgb = torch.full((n, H + gap, rs), CANARY, dtype=torch.uint8, device="cuda")
    cr = torch.full((n, H // 2 + gap, cs), CANARY, dtype=torch.uint8, device="cuda")
    cb = torch.full((n, H // 2 + gap, cs), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((n, 3), -7, dtype=torch.int64, device="cuda")
    images = (_lib.DecodeImage * n)()
    for i, e in enumerate(encs):
        sl, sv = (e.slot_len, e.slot_val) if kind == SLOTS else (e.sym_len, e.sym_val)
        for c, (k, out) in enumerate(zip(pipeline.CHANNELS, (rgb, cr, cb))):
            assert out[i].data_ptr() % 8 == 0
            images[i].c[c] = _lib.DecodePlane(sl[k].data_ptr(), sv[k].data_ptr(), e.counts.data_ptr() + 8 * c,
                                              e.dc[k].data_ptr(), e.index[k].data_ptr(), out[i].data_ptr(),
                                              status[i, c:].data_ptr())
    nbytes = _lib.load().hic_decode_batch_table_bytes(n)
    h_table = ctypes.create_string_buffer(nbytes)
    _lib.call("hic_decode_batch_table", _lib.STREAM_SLOTS if kind == SLOTS else _lib.STREAM_INDEXED, n, H, W, rs, cs,
              images, h_table, nbytes)
    d_table = device.to_device(np.frombuffer(h_table, np.uint8, nbytes))
    _lib.call("hic_decode420_batch_u8", h_table, device.ptr(d_table), device.stream_ptr())
    torch.cuda.synchronize()
    rgb, cr, cb = rgb.cpu().numpy(), cr.cpu().numpy(), cb.cpu().numpy()
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(rgb[i, :H, :3 * W].reshape(H, W, 3), ref[0], err_msg="image %d rgb" % i)
        np.testing.assert_array_equal(cr[i, :H // 2, :W // 2], ref[1], err_msg="image %d cr" % i)
        np.testing.assert_array_equal(cb[i, :H // 2, :W // 2], ref[2], err_msg="image %d cb" % i)
    assert status.cpu().tolist() == [r[3] for r in refs]
    for name, buf, h, w in (("rgb", rgb, H, 3 * W), ("cr", cr, H // 2, W // 2), ("cb", cb, H // 2, W // 2)):
        assert (buf[:, :h, w:] == CANARY).all(), "%s: a pad byte was written" % name
        assert (buf[:, h:] == CANARY).all(), "%s: a gap row was written" % name


@pytest.mark.parametrize("n,H,W,kind", [(5, 16, 512, SLOTS), (3, 48, 80, INDEXED)])
def test_batch_failed_count(n, H, W, kind):
    """One image's one channel count set to 0 (a failed encode's): that status word is
    -1 and check_status names it; every other image is untouched by it."""
    _, src, refs = _encoded(n, H, W, kind)
    encs = src.encoders if kind == SLOTS else src
    dec = pipeline.BatchDecoder(n, H, W)
    bad = n // 2
    for ch, name in enumerate(pipeline.CHANNELS):
        counts = encs[bad].counts.clone()
        counts[ch] = 0
        sources = [(e.sym_len, e.sym_val, counts if i == bad else e.counts, e.dc, e.index) for i, e in enumerate(encs)]
        _poison(dec)
        dec.decode(sources)
        _assert_batch(dec, refs, "count %d" % ch, skip=(bad,))
        want = list(refs[bad][3])
        want[ch] = -1
        assert dec.status[bad].cpu().tolist() == want, ch
        # the one-image decoder on the same count leaves the same image behind
        one = _decode_one(encs[bad], counts)
        assert one[3] == want
        np.testing.assert_array_equal(dec.rgb[bad].cpu().numpy(), one[0])
        with pytest.raises(ValueError, match="image %d channel %s" % (bad, name)):
            dec.check_status()


def test_batch_side_stream():
    n, H, W, kind = 3, 80, 1024, SLOTS
    _, src, refs = _encoded(n, H, W, kind)
    dec = pipeline.BatchDecoder(n, H, W)
    _poison(dec)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    dec.decode(src, stream=side)
    dec.decode(src, stream=side)  # the reused table on the same stream
    side.synchronize()
    _assert_batch(dec, refs, "side stream")


def test_batch_refuses_bad_sources():
    n, H, W = 5, 16, 512
    _, src, _ = _encoded(n, H, W, SLOTS)
    dec = pipeline.BatchDecoder(n, H, W)
    indexed = pipeline.Encoder(H, W, index=True, slots=False)
    indexed.encode(device.to_device(_images(1, H, W)[0]))
    with pytest.raises(ValueError, match="one kind"):
        dec.decode(src.encoders[:n - 1] + [indexed])
    with pytest.raises(ValueError, match="sources for a batch"):
        dec.decode(src.encoders[:n - 1])
    with pytest.raises(ValueError, match="sources for a batch"):
        pipeline.BatchDecoder(n + 1, H, W).decode(src)
    with pytest.raises(ValueError):
        pipeline.BatchDecoder(n, 32, W).decode(src)
    other = pipeline.Encoder(32, W)
    with pytest.raises(ValueError, match="source 4"):
        dec.decode(src.encoders[:n - 1] + [other])
    e = src.encoders[0]
    with pytest.raises(ValueError, match="counts"):
        dec.decode([(e.sym_len, e.sym_val, [1, 1, 1], e.dc, e.index)] * n)
    with pytest.raises(ValueError):
        dec.decode([pipeline.Encoder(H, W, slots=False)] * n)  # no index
    for bad in ((0, H, W), (pipeline.DECODE_BATCH_MAX + 1, H, W), (2, 24, 512), (2, 16, 40)):
        with pytest.raises(ValueError):
            pipeline.BatchDecoder(*bad)
    # nothing above disturbed the decoder
    dec.decode(src)
    dec.check_status()


def test_codec_decode_batch():
    a = [_img(KINDS[i % 7], 64, 1024, 70 + i) for i in range(5)]
    b = [_img(KINDS[(i + 3) % 7], 80, 208, 80 + i) for i in range(3)]
    imgs = [a[0], b[0], a[1], b[1], a[2], a[3], b[2], a[4]]
    files = [codec.encode(x) for x in imgs]
    want = [codec.decode(h) for h in files]
    got = codec.decode_batch(files)
    assert [x.shape for x in got] == [x.shape for x in want] == [x.shape for x in imgs]
    assert [x.dtype for x in got] == [x.dtype for x in want]
    assert [x.tobytes() for x in got] == [x.tobytes() for x in want]
    assert codec.decode_batch([]) == []
    assert codec.decode_batch(iter(files[:1]))[0].tobytes() == want[0].tobytes()
    # plus one (250, 330) file, which the fast path refuses: it goes through decode's
    # per-file path, and the list's outcome is the loop's.  (The reference's jpeg_decode
    # asserts on planes that are not whole 8 x 8 blocks, codec.py:418, so for this file
    # the loop's outcome is that exception, as in test_codec_decode_region_ragged_fallback.)
    rag = codec.encode(_img("random", 250, 330, 90))
    assert codec._fast_header(rag) is None
    mixed = files[:3] + [rag] + files[3:]
    loop = _outcome(lambda: [codec.decode(h) for h in mixed])
    assert _outcome(lambda: codec.decode_batch(mixed)) == loop
    assert loop == _outcome(lambda: [codec.decode(rag)])


def _outcome(fn):
    try:
        return [(x.shape, x.tobytes()) for x in fn()]
    except Exception as e:  # noqa: BLE001 -- the type is what is compared
        return type(e)


def _truncated(h, stream, keep):
    """The file with the bit string of one of its nine streams cut to `keep` of its bits."""
    p = list(h.payloads)
    packed, nbits = p[9 + stream].packed_bits()
    p[9 + stream] = hicimage.BitStringP.from_packed(np.array(packed, copy=True), int(int(nbits) * keep))
    return hicimage.HicImage.jpeg_image(p)


@pytest.mark.parametrize("stream,keep", [(3, 0.5), (0, 0.9), (7, 0.25)])
def test_codec_decode_batch_corrupted_file(stream, keep):
    """One file with a truncated bit string among good ones: the same exception type (or,
    if the loop accepts it, the same bytes) as decoding the list file by file."""
    files = [codec.encode(_img("random", 64, 1024, 60 + i)) for i in range(3)]
    files[1] = _truncated(files[1], stream, keep)
    loop = _outcome(lambda: [codec.decode(h) for h in files])
    assert _outcome(lambda: codec.decode_batch(files)) == loop
    if stream == 3:
        assert isinstance(loop, type) and issubclass(loop, Exception), "the truncated values stream was accepted"
