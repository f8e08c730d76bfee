"""The batched Huffman encode (huffman.BatchStreams, hic_huffman_batch_key_range /
_histogram / _pack + hic_huffman_build_batch; BatchEncoder.hic_images(batched=True)):
per image and byte for byte what the per-image stage (huffman.DeviceStreams, unchanged)
gives, from a number of library calls and host reads that does not depend on n.
Image i of a batch is _img(KINDS[i % 7], ...) with its own seed, so an all-zero, a
sparse, a wide-valued and a last-block image sit between noisy ones: neighbouring
images differ in key range, bin count and bit length, and nothing of image i -- bins,
positions, bit offsets, the filler runs' edge words -- may show in image i + 1.
Reference: codec.jpeg_encode (codec.py:304-334), huffman.py:11-142."""
import functools

import numpy as np
import pytest
import torch

import oracle.oracle_c as orcc
from hiccup_amd import _lib, codec, compression, device, hicimage, huffman, pipeline
from hiccup_amd.huffman import HuffmanTree
from test_gpu_slot_huffman import KINDS, ORDER, _img, _streams

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 16, 512),     # one image, one Y band: n = 1 through the batched path
    (7, 16, 512),     # all seven kinds; chroma channels of one record; streams that are a single EOB; one-key trees
    (3, 80, 1024),    # two strips, a short last band
    (2, 272, 1536),   # image 0 last_block: a filler run above 20000 (the cooperative long-run path) beside `random`
    (2, 4112, 512),   # over 256 Y records: further rounds of the fill's 256-record loop, a scan past one workgroup's width
]
CH = pipeline.CHANNELS


def _kinds(n, H, W):
    if (n, H, W) == (2, 272, 1536):
        return ["last_block", "random"]
    return [KINDS[i % 7] for i in range(n)]


def _images(n, H, W, salt=0):
    if salt:  # flatter inputs: every image's streams shorter than the first encode's
        return np.stack([_img("sparse" if i % 2 else "zero", H, W, 1000 * salt + i) for i in range(n)])
    return np.stack([_img(k, H, W, 31 * i + H + W) for i, k in enumerate(_kinds(n, H, W))])


@functools.lru_cache(maxsize=None)
def _reference(n, H, W, salt=0):
    """(host images, per image the bytes of a fresh one-image Encoder(H, W)'s
    hic_image(from_slots=True)): computed once per shape and left unchanged."""
    imgs = _images(n, H, W, salt)
    out = []
    for i in range(n):
        enc = pipeline.Encoder(H, W)
        assert enc.slots
        enc.encode(device.to_device(imgs[i]))
        out.append(enc.hic_image(from_slots=True).byte_stream())
    return imgs, out


def _batch(n, H, W, imgs):
    batch = pipeline.BatchEncoder(n, H, W)
    batch.encode(device.to_device(imgs))
    torch.cuda.synchronize()
    return batch


def _batch_streams(batch):
    counts = batch.counts.cpu().tolist()
    return huffman.BatchStreams([[e.dc[k] for k in CH] for e in batch.encoders],
                                [e._slot_jobs() for e in batch.encoders], counts), counts


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_batch_primitives_equal_per_image(n, H, W):
    """Every stream of every image: key range, counts, the present keys in first-
    appearance order, the code table and the packed bits with their bit count == one
    huffman.DeviceStreams over that image alone."""
    imgs, _ = _reference(n, H, W)
    batch = _batch(n, H, W, imgs)
    got, counts = _batch_streams(batch)
    got_packed = got.packed()
    kinds = _kinds(n, H, W)
    for i in range(n):
        enc = batch[i]
        ss, c = _streams(enc, True)
        assert c == [int(v) for v in counts[i]]
        exp = huffman.DeviceStreams(ss)
        exp_packed = exp.packed()
        assert got.lo[i] == exp.lo and got.nbins[i] == exp.nbins, i
        for p, (k, j) in enumerate(ORDER):
            msg = str((i, kinds[i], k, j))
            np.testing.assert_array_equal(got.counts[i][p], exp.counts[p], err_msg=msg)
            assert got.trees[i][p].leaf_keys == exp.trees[p].leaf_keys, msg
            # the first-appearance positions of the present keys, in that order, ascend
            f = got.first[i][p][np.asarray(got.trees[i][p].leaf_keys) - got.lo[i][p]].astype(np.int64)
            assert np.all(np.diff(f) > 0) and f[0] == 0, msg
            assert np.all(got.first[i][p][got.counts[i][p] == 0] == 0xFFFFFFFF), msg
            assert got.trees[i][p].encode_table() == exp.trees[p].encode_table(), msg
            for a, b in zip(got.trees[i][p].code_table(got.lo[i][p], got.nbins[i][p]),
                            exp.trees[p].code_table(exp.lo[p], exp.nbins[p])):
                np.testing.assert_array_equal(a, b, err_msg=msg)
            assert got_packed[i][p][1] == exp_packed[p][1], msg
            np.testing.assert_array_equal(got_packed[i][p][0], exp_packed[p][0], err_msg=msg)
        # non-vacuity, from the close's record index {n, P, pdc, nfill} and the counts
        if kinds[i] == "zero":
            assert c == [1, 1, 1]
            assert [t.encode_table()[0][1] for t in got.trees[i][3:]] == ["1"] * 6  # one-key trees: code "1"
        if kinds[i] == "last_block" and (H, W) == (272, 1536):
            assert enc.sidx["lum"].cpu().numpy()[3::4].max() > 20000  # 6528 flat blocks x 63 / 15
    if n >= 2:  # neighbours differ on the same stream: nothing here is one table applied n times
        assert any(len({(got.lo[i][p], got.nbins[i][p]) for i in range(n)}) >= 2 for p in range(9))
    if (n, H, W) == (2, 4112, 512):
        assert batch[0].sidx["lum"].numel() // 4 > 256  # more than one round of the 256-record loops


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_batch_bytes(n, H, W):
    """hic_images(batched=True) == hic_images(batched=False) == a fresh one-image
    Encoder's bytes; at (7, 16, 512) also the chained reference calls'."""
    imgs, want = _reference(n, H, W)
    batch = _batch(n, H, W, imgs)
    got = [h.byte_stream() for h in batch.hic_images(batched=True)]
    assert got == [h.byte_stream() for h in batch.hic_images(batched=False)]
    assert got == want
    assert got == [h.byte_stream() for h in batch.hic_images(batched=True)]  # twice without re-encoding
    if (n, H, W) == (7, 16, 512):
        assert got == [codec.jpeg_encode(compression.jpeg_compression(x)).byte_stream() for x in imgs]
    with pytest.raises(ValueError):
        batch.hic_images(batched=True, from_slots=False)


def test_batch_independent_of_the_kernels():
    """(7, 16, 512): the symbols from the C oracle, the nine trees and bit strings of
    each image from the pure-Python HuffmanTree, against the table payloads and the
    unpacked bit strings of the batched .hic."""
    n, H, W = 7, 16, 512
    imgs, _ = _reference(n, H, W)
    batch = _batch(n, H, W, imgs)
    hics = batch.hic_images(batched=True)
    for i in range(n):
        y, cr, cb = orcc.rgb_to_ycrcb(imgs[i])
        sym = {}
        for k, (p, t) in {"lum": (y, 0), "cr": (orcc.pyr_down(cr), 1), "cb": (orcc.pyr_down(cb), 1)}.items():
            zz = orcc.zigzag_blocks(orcc.dct_channel(p, t), 8)
            L, V = orcc.rle_encode(zz[:, 1:].reshape(-1), 15)
            sym[k] = (orcc.dpcm(zz[:, 0].copy()).tolist(), [int(v) for v in V], [int(v) for v in L])
        pay = hics[i].payloads
        for p, (k, j) in enumerate(ORDER):
            tree = HuffmanTree.construct_from_data(sym[k][j])
            table = [tuple(t.numbers) for t in pay[p].payloads]
            assert [(int(v), c) for v, c in table] == [(int(v), c) for v, c in tree.encode_table()], (i, k, j)
            assert pay[9 + p].payload == tree.encode_data(), (i, k, j)


def test_batch_reuse():
    """A second encode on the same objects with flatter inputs (every stream
    shorter): stale bits or bins of the first pass would show."""
    n, H, W = 3, 80, 1024
    first, _ = _reference(n, H, W)
    second, want = _reference(n, H, W, 1)
    batch = pipeline.BatchEncoder(n, H, W)
    batch.encode(device.to_device(first))
    a = [h.byte_stream() for h in batch.hic_images(batched=True)]
    batch.encode(device.to_device(second))
    b = [h.byte_stream() for h in batch.hic_images(batched=True)]
    assert b == want
    size = lambda parts: sum(len(p) for p in parts)  # noqa: E731 -- (byte_stream: a list of payload bytes)
    assert all(size(y) < size(x) for x, y in zip(a, b)), ([size(x) for x in a], [size(y) for y in b])
    fresh = pipeline.BatchEncoder(n, H, W)
    fresh.encode(device.to_device(second))
    assert [h.byte_stream() for h in fresh.hic_images(batched=True)] == want


def _count_calls(monkeypatch, fn):
    """(library calls, device-to-host reads) fn() makes: every call on the loaded
    library (_lib.call's go through it too), device.to_host and .cpu()."""
    seen = {"lib": 0, "read": 0}
    real_to_host, real_cpu, lib = device.to_host, torch.Tensor.cpu, _lib.load()

    class Counting:
        def __getattr__(self, name):
            f = getattr(lib, name)
            if not callable(f):
                return f

            def g(*a):
                seen["lib"] += 1
                return f(*a)
            return g

    def to_host(t):
        seen["read"] += 1
        return real_to_host(t)

    def cpu(self, *a, **kw):
        seen["read"] += 1
        return real_cpu(self, *a, **kw)

    with monkeypatch.context() as m:
        m.setattr(_lib, "_lib", Counting())
        m.setattr(device, "to_host", to_host)
        m.setattr(torch.Tensor, "cpu", cpu)
        out = fn()
    return out, seen


def test_batch_call_count_independent_of_n(monkeypatch):
    H, W = 16, 512
    seen = {}
    for n in (2, 7):
        imgs, want = _reference(n, H, W)
        batch = _batch(n, H, W, imgs)
        batch.hic_images(batched=True)  # (warm: pools and side streams exist)
        out, seen[n] = _count_calls(monkeypatch, lambda: batch.hic_images(batched=True))
        assert [h.byte_stream() for h in out] == want
    assert seen[2] == seen[7], seen
    assert seen[2]["lib"] > 0
    # the counts, every key range, every histogram, every stream's bits with the bit counts
    assert seen[2]["read"] == 4
    # the loop, for contrast: its calls grow with n
    batch = _batch(2, H, W, _reference(2, H, W)[0])
    _, loop = _count_calls(monkeypatch, lambda: batch.hic_images(batched=False))
    assert loop["lib"] > seen[2]["lib"] and loop["read"] > seen[2]["read"]


def test_codec_encode_batch_uses_the_default():
    n, H, W = 7, 16, 512
    imgs, want = _reference(n, H, W)
    assert pipeline.batched_default(n, H, W)
    assert [h.byte_stream() for h in codec.encode_batch(np.array(imgs))] == [codec.encode(x).byte_stream() for x in imgs]
    assert [h.byte_stream() for h in codec.encode_batch(list(imgs))] == want


def test_batch_streams_side_stream():
    """Everything on the caller's stream: a non-current stream, the same bytes."""
    n, H, W = 3, 80, 1024
    imgs, want = _reference(n, H, W)
    side = torch.cuda.Stream()
    batch = pipeline.BatchEncoder(n, H, W)
    x = device.to_device(imgs)
    torch.cuda.synchronize()
    batch.encode(x, stream=side)
    assert [h.byte_stream() for h in batch.hic_images(stream=side, batched=True)] == want
    assert isinstance(batch.hic_images(stream=side)[0], hicimage.HicImage)
