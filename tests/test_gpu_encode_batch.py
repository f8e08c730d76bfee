"""The batched slot encode (pipeline.BatchEncoder: hic_encode420_slots_batch_u8 +
hic_rle_slots_close_batch, one fused launch and one scan launch for n images of
one shape) leaves, per image and bit for bit, what Encoder(H, W).encode leaves:
counts, DC differences, record index, every record's symbols, the materialized
stream and blocks, and the .hic bytes coded from the slots.  The shapes are the
smallest at which each mechanism can fail (see SHAPES); image i is
_img(KINDS[i % 7], ...) with its own seed, so an all-zero and a sparse image sit
between noisy ones: carried zero runs, the EOB and the first block's DC difference
must not leak across image boundaries.  Reference: compression.jpeg_compression
(compression.py:16-39) + codec.jpeg_encode's DC / RLE half (codec.py:47-99,286-301)."""
import functools

import numpy as np
import pytest
import torch

import oracle.oracle_c as orcc
from hiccup_amd import _lib, codec, device, pipeline
from test_gpu_slots import KINDS, _img
from test_gpu_slots_fill import _assert_equal, _snapshot

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 16, 512),    # one live wave of one band
    (5, 16, 512),    # 5 workgroups: fewer than the 8 XCDs, remainder 5
    (3, 80, 1024),   # two strips, a short last band, 12 workgroups: remainder 4
    (2, 48, 1536),   # three strips
    (9, 64, 512),    # 18 workgroups: remainder 2
    (2, 4112, 512),  # 257 Y records: two scan partitions per Y channel (the close's hand-off in a batch)
]


def _images(n, H, W, salt=0):
    return np.stack([_img(KINDS[i % 7], H, W, 1000 * salt + 31 * i + H + W) for i in range(n)])


@functools.lru_cache(maxsize=None)
def _reference(n, H, W, salt=0):
    """(host images, per image the snapshot of a fresh one-image Encoder): computed
    once per shape and left unchanged."""
    imgs = _images(n, H, W, salt)
    refs = []
    for i in range(n):
        enc = pipeline.Encoder(H, W)
        assert enc.slots
        enc.encode(device.to_device(imgs[i]))
        torch.cuda.synchronize()
        refs.append(_snapshot(enc))
    return imgs, refs


def _check(batch, refs, msg):
    torch.cuda.synchronize()
    for i, ref in enumerate(refs):
        _assert_equal(_snapshot(batch[i]), ref, "%s image %d" % (msg, i))


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_batch_equals_per_image_encoder(n, H, W):
    imgs, refs = _reference(n, H, W)
    batch = pipeline.BatchEncoder(n, H, W)
    assert len(batch) == n and all(batch[i].slots for i in range(n))
    assert tuple(batch.counts.shape) == (n, 3)
    batch.encode(device.to_device(imgs))
    torch.cuda.synchronize()
    assert batch.counts.cpu().tolist() == [r["counts"] for r in refs]
    assert all(batch[i].counts.data_ptr() == batch.counts[i].data_ptr() for i in range(n))
    _check(batch, refs, "%dx%dx%d" % (n, H, W))
    # the one-read path: hic_images == the per-image bytes
    assert [h.byte_stream() for h in batch.hic_images()] == [r["bytes"] for r in refs]


@pytest.mark.parametrize("n,H,W", [(3, 80, 1024), (2, 4112, 512)])
def test_batch_equals_c_oracle(n, H, W):
    """Independent of the project's own kernels: every image of the batch against the C
    oracle, and image 0 from a one-image Encoder(H, W) against it too -- the batch's
    close and the one-image close run one scan body, so their equality alone does not
    check it.  (2, 4112, 512): 257 Y records, two scan partitions per Y channel, the
    smallest shape whose close crosses the granule hand-off."""
    imgs = _images(n, H, W)
    batch = pipeline.BatchEncoder(n, H, W)
    batch.encode(device.to_device(imgs))
    one = pipeline.Encoder(H, W)
    assert one.slots
    one.encode(device.to_device(imgs[0]))
    for i in range(n):
        results = [("batch", batch[i].result())] + ([("one-image", one.result())] if i == 0 else [])
        y, cr, cb = orcc.rgb_to_ycrcb(imgs[i])
        for k, (p, t) in {"lum": (y, 0), "cr": (orcc.pyr_down(cr), 1), "cb": (orcc.pyr_down(cb), 1)}.items():
            zz = orcc.zigzag_blocks(orcc.dct_channel(p, t), 8)
            L, V = orcc.rle_encode(zz[:, 1:].reshape(-1), 15)
            dc = orcc.dpcm(zz[:, 0].copy())
            for who, got in results:
                assert np.array_equal(got[k][0].astype(np.int32), zz), (who, i, k)
                assert np.array_equal(got[k][1], dc), (who, i, k)
                assert np.array_equal(got[k][2].astype(np.int32), L), (who, i, k)
                assert np.array_equal(got[k][3].astype(np.int32), V), (who, i, k)


@pytest.mark.parametrize("knob,value", [("encode_band", 0), ("encode_band", 1), ("encode_order", 0),
                                        ("encode_order", 6)])
def test_batch_knobs(knob, value):
    n, H, W = 3, 80, 1024
    imgs, refs = _reference(n, H, W)
    before = _lib._raw_knob(knob)
    try:
        _lib.set_knob(knob, value)
        batch = pipeline.BatchEncoder(n, H, W)
        batch.encode(device.to_device(imgs))
        _check(batch, refs, "%s=%d" % (knob, value))
    finally:
        _lib.set_knob(knob, before)


def test_batch_reuse():
    """A second encode on the same batch, other inputs: stale hand-off granules and the
    close's in-place DC subtraction would show."""
    n, H, W = 2, 4112, 512
    first, _ = _reference(n, H, W)
    imgs, refs = _reference(n, H, W, 1)
    assert not np.array_equal(first, imgs)
    batch = pipeline.BatchEncoder(n, H, W)
    batch.encode(device.to_device(first))
    batch.encode(device.to_device(imgs))
    _check(batch, refs, "second encode")


def test_batch_strides_and_streams():
    n, H, W = 3, 80, 1024
    imgs, refs = _reference(n, H, W)
    big = device.to_device(np.concatenate([imgs, np.full((n, 16, W, 3), 7, np.uint8)], axis=1))
    view = big[:, :H]
    assert view.stride(0) == (H + 16) * W * 3 and not view.is_contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    batch = pipeline.BatchEncoder(n, H, W)
    torch.cuda.synchronize()
    batch.encode(view, stream=side)
    side.synchronize()
    _check(batch, refs, "strided, side stream")
    with pytest.raises(ValueError):
        batch.encode(big[:, 8:8 + H, :, :].transpose(1, 2))          # wrong shape
    with pytest.raises(ValueError):
        batch.encode(device.to_device(np.zeros((n, W, H, 3), np.uint8)).transpose(1, 2))  # non-contiguous images
    with pytest.raises(ValueError):
        batch.encode(device.to_device(imgs[:2]))
    with pytest.raises(ValueError):
        batch.encode(device.to_device(imgs).to(torch.int8))
    with pytest.raises(ValueError):
        pipeline.BatchEncoder(2, 40, 200)


def test_batch_decode():
    n, H, W = 5, 16, 512
    imgs, _ = _reference(n, H, W)
    batch = pipeline.BatchEncoder(n, H, W)
    batch.encode(device.to_device(imgs))
    for i in range(n):
        one = pipeline.Encoder(H, W)
        one.encode(device.to_device(imgs[i]))
        d1, d2 = pipeline.Decoder(H, W), pipeline.Decoder(H, W)
        e = batch[i]
        r1 = d1.decode(e.sym_len, e.sym_val, e.counts, e.dc, index=e.index)
        r2 = d2.decode(one.sym_len, one.sym_val, one.counts, one.dc, index=one.index)
        torch.cuda.synchronize()
        d1.check_status()
        assert torch.equal(r1, r2), i


def test_codec_encode_batch():
    n, H, W = 3, 80, 1024
    imgs, refs = _reference(n, H, W)
    want = [codec.encode(x).byte_stream() for x in imgs]
    assert want == [r["bytes"] for r in refs]
    for form in (imgs, list(imgs), device.to_device(imgs), [device.to_device(x) for x in imgs]):
        assert [h.byte_stream() for h in codec.encode_batch(form)] == want
    # an ineligible shape, and mixed shapes: per image, the same bytes
    rag = np.stack([_img("random", 40, 200, s) for s in (1, 2)])
    assert [h.byte_stream() for h in codec.encode_batch(rag)] == [codec.encode(x).byte_stream() for x in rag]
    mixed = [imgs[0], rag[0]]
    assert [h.byte_stream() for h in codec.encode_batch(mixed)] == [codec.encode(x).byte_stream() for x in mixed]
    assert codec.encode_batch([]) == []
