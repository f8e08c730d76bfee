"""The Huffman stage read straight from the slot layout (csrc/huffman.hip,
hic_slot_key_range / hic_slot_key_histogram / hic_slot_huffman_pack; csrc/slots.h):
key ranges, histograms in first-appearance order, code tables and packed bits of a
slot-layout encoder's six AC streams equal the contiguous entry points' on the
compacted stream, on images that stress each part of the virtual stream (fillers
before a record, one carried run across almost every record, the EOB alone);
Encoder.hic_image(from_slots=True) without a compaction; and the one-call surface
codec.encode / codec.decode against the chained calls it replaces.  Reference:
codec.jpeg_encode / jpeg_decode (codec.py:275-426), huffman.py:11-142."""
import numpy as np
import pytest
import torch

from hiccup_amd import codec, compression, device, hicimage, huffman, pipeline

pytestmark = pytest.mark.gpu


def _img(kind, H, W, seed):
    """tests/test_gpu_slots.py's small images, plus last_block."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "levels":  # 4 grey levels: exact quantiser ties
        return (rng.integers(0, 4, (H, W, 1)) * 85).astype(np.uint8).repeat(3, 2)
    if kind == "smooth":  # natural-image-like: few nonzero AC, long runs inside blocks
        y, x = np.mgrid[0:H, 0:W]
        base = 128 + 60 * np.sin(x / 37.0) * np.cos(y / 23.0) + rng.normal(0, 3, (H, W))
        return np.clip(np.stack([base, base * 0.9 + 10, 255 - base], -1), 0, 255).astype(np.uint8)
    if kind == "sparse":  # flat but for scattered pixels: zero runs carried across many records
        img = np.full((H, W, 3), 128, np.uint8)
        n = max(1, H * W // 20000)
        img[rng.integers(0, H, n), rng.integers(0, W, n)] = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        return img
    if kind == "zero":  # every AC coefficient zero: the stream is the single EOB
        return np.full((H, W, 3), 128, np.uint8)
    if kind == "wide":  # grey rows [255 255 0 0 0 0 255 255]: raster (0, 2) = zig-zag slot 3 ~ +-2130
        row = np.array([255, 255, 0, 0, 0, 0, 255, 255], np.uint8)
        img = np.tile(row, W // 8)[None, :].repeat(H, 0)
        img = np.where(rng.integers(0, 2, (H // 8, W // 8)).repeat(8, 0).repeat(8, 1) == 1, img, 255 - img)
        img[: H // 2, : W // 2] = rng.integers(0, 256, (H // 2, W // 2))  # beside ordinary blocks
        return img[..., None].repeat(3, 2).astype(np.uint8)
    if kind == "last_block":  # flat but for the bottom-right 8 x 8 block: ONE zero run carried over every record
        img = np.full((H, W, 3), 128, np.uint8)
        img[H - 8:, W - 8:] = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
        return img
    raise ValueError(kind)


KINDS = ["random", "levels", "smooth", "sparse", "zero", "wide", "last_block"]
ORDER = [(k, j) for j in range(3) for k in pipeline.CHANNELS]  # payload order; j: 0 DC, 1 AC values, 2 AC lengths


def _streams(enc, from_slots):
    """The nine streams of an encoded slot-layout encoder in payload order: the AC
    ones from the slots, or contiguous (after compact())."""
    counts = [int(c) for c in enc.counts.cpu().tolist()]
    jobs = enc._slot_jobs()
    out = []
    for k, j in ORDER:
        i = pipeline.CHANNELS.index(k)
        if j == 0:
            out.append((enc.dc[k], enc.dc[k].numel()))
        elif from_slots:
            out.append(huffman.SlotStream(jobs[i], counts[i], 2 - j))
        else:
            out.append(((enc.sym_val if j == 1 else enc.sym_len)[k], counts[i]))
    return out, counts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", [(16, 512), (48, 1024), (272, 1536)])
def test_slot_primitives_equal_contiguous(kind, H, W):
    """Key range, histogram (counts and first-appearance order), the code tables
    built from them and the packed bits, read from the slots == the contiguous
    entry points on the compacted stream, for all nine streams."""
    enc = pipeline.Encoder(H, W)
    assert enc.slots
    enc.encode(device.to_device(_img(kind, H, W, H + W)))
    ss, counts = _streams(enc, True)
    got = huffman.DeviceStreams(ss)
    got_packed = got.packed()
    # non-vacuity, from the close's record index {n, P, pdc, nfill} and the counts
    nfill = {k: enc.sidx[k].cpu().numpy()[3::4] for k in pipeline.CHANNELS}
    if (H, W) == (272, 1536) and kind in ("sparse", "last_block"):
        assert max(int(nfill[k].max()) for k in pipeline.CHANNELS) > 0
    if (H, W) == (272, 1536) and kind == "last_block":
        assert nfill["lum"].max() > 20000  # 6528 flat blocks x 63 / 15
    if kind == "zero":
        assert counts == [1, 1, 1]
    enc.compact()
    cs, _ = _streams(enc, False)
    exp = huffman.DeviceStreams(cs)
    exp_packed = exp.packed()
    assert got.lo == exp.lo and got.nbins == exp.nbins
    for i, (k, j) in enumerate(ORDER):
        np.testing.assert_array_equal(got.counts[i], exp.counts[i], err_msg=str((k, j)))
        assert got.trees[i].leaf_keys == exp.trees[i].leaf_keys, (k, j)  # keys in first-appearance order
        for a, b in zip(got.trees[i].code_table(got.lo[i], got.nbins[i]),
                        exp.trees[i].code_table(exp.lo[i], exp.nbins[i])):
            np.testing.assert_array_equal(a, b, err_msg=str((k, j)))
        assert got_packed[i][1] == exp_packed[i][1], (k, j)
        np.testing.assert_array_equal(got_packed[i][0], exp_packed[i][0], err_msg=str((k, j)))
    # where value key 0 first appears: in a filler run (last_block: the carried run
    # opens the stream) or at the EOB (zero: the stream is the EOB)
    if kind in ("zero", "last_block") and (H, W) == (272, 1536):
        for i, k in enumerate(pipeline.CHANNELS):
            L = enc.sym_len[k][:counts[i]].cpu().numpy()
            V = enc.sym_val[k][:counts[i]].cpu().numpy()
            at = int(np.flatnonzero(V == 0)[0])
            if kind == "zero":
                assert at == counts[i] - 1 and L[at] == 0, k
            else:
                assert at < counts[i] - 1 and L[at] == 14, k


def _check_from_slots(enc, x, stream=None):
    """enc.hic_image(stream, from_slots=True) of image x == a fresh coefficient-chain
    encoder's hic_image, and no compaction ran: a sentinel written over sym_len /
    sym_val after encode() survives everywhere but at the EOB's position."""
    enc.encode(x, stream=stream)
    torch.cuda.synchronize()
    counts = [int(c) for c in enc.counts.cpu().tolist()]
    for k in pipeline.CHANNELS:
        enc.sym_len[k].fill_(0x5A)
        enc.sym_val[k].fill_(0x5A5A)
    torch.cuda.synchronize()
    got = enc.hic_image(stream=stream, from_slots=True)
    ref = pipeline.Encoder(enc.H, enc.W, slots=False)
    ref.encode(x)
    want = ref.hic_image().byte_stream()
    assert got.byte_stream() == want
    assert ref.hic_image(from_slots=True).byte_stream() == want  # a coefficient chain: as the default
    for i, k in enumerate(pipeline.CHANNELS):
        keep = np.ones(enc.cap[k], bool)
        keep[counts[i] - 1] = False
        assert np.all(enc.sym_len[k].cpu().numpy()[keep] == 0x5A), k
        assert np.all(enc.sym_val[k].cpu().numpy()[keep] == 0x5A5A), k


@pytest.mark.parametrize("kind", KINDS)
def test_hic_image_from_slots(kind):
    H, W = 272, 1024
    enc = pipeline.Encoder(H, W)
    assert enc.slots
    _check_from_slots(enc, device.to_device(_img(kind, H, W, 7)))


def test_hic_image_from_slots_side_stream_and_repeat():
    """The same on a non-current stream, with a second image into the same encoder."""
    H, W = 272, 1024
    side = torch.cuda.Stream()
    enc = pipeline.Encoder(H, W)
    for seed, kind in ((1, "sparse"), (2, "random")):
        x = device.to_device(_img(kind, H, W, seed))
        torch.cuda.synchronize()  # the input and the encoder's zero-filled workspaces: written on the current stream
        _check_from_slots(enc, x, stream=side)


def _chained_encode(rgb):
    return codec.jpeg_encode(compression.jpeg_compression(rgb))


def _chained_decode(h):
    return compression.jpeg_decompression(codec.jpeg_decode(h))


@pytest.mark.parametrize("H,W", [(272, 1024), (48, 80), (250, 330), (37, 53), ("lenna", 0)])
def test_codec_encode_decode(H, W, golden_lenna):
    """codec.encode == jpeg_encode(jpeg_compression(.)) byte for byte (slot layout,
    fused with W % 512 != 0, the ragged chain, an odd shape, the Lenna fixture), from
    a host array and from a device tensor; codec.decode == the chained decode."""
    if H == "lenna":
        rgb = golden_lenna["rgb"]
    else:
        rgb = _img("smooth" if H == 272 else "random", H, W, H * W)
    ref = _chained_encode(rgb)
    got = codec.encode(rgb)
    assert got.byte_stream() == ref.byte_stream()
    assert codec.encode(device.to_device(rgb)).byte_stream() == ref.byte_stream()
    # (a plane that is not whole 8 x 8 blocks fails jpeg_decode's length assertion:
    # codec.decode then raises what the chained call raises)
    exp = _outcome(_chained_decode, ref)
    if H == "lenna" or (H % 16 == 0 and W % 16 == 0):
        assert exp[0] == "ok"
    _same_outcome(_outcome(codec.decode, ref), exp)
    _same_outcome(_outcome(lambda x: codec.decode(codec.encode(x)), rgb), exp)  # the round trip


def _outcome(f, x):
    try:
        return ("ok", f(x))
    except Exception as e:  # noqa: BLE001 -- compared by _same_outcome
        return (type(e), str(e))


def _same_outcome(a, b):
    assert a[0] == b[0]
    if a[0] == "ok":
        assert a[1].dtype == b[1].dtype and a[1].shape == b[1].shape
        np.testing.assert_array_equal(a[1], b[1])
    else:
        assert a[1] == b[1]


def test_codec_decode_fallback_non_int_leaf():
    """A HicImage whose AC-length table holds a non-int leaf goes through the
    chained calls: the same result or the same exception as compression.decode."""
    rgb = _img("random", 48, 80, 5)
    h = codec.encode(rgb)
    p = list(h.payloads)
    t = p[6]  # the luminance AC-length table
    pl = list(t.payloads)
    v, c = pl[0].numbers
    pl[0] = hicimage.TupP(float(v) + 0.5, c)
    p[6] = hicimage.PayloadStringP(hicimage.TupP, pl)
    bad = hicimage.HicImage.jpeg_image(p)
    _same_outcome(_outcome(codec.decode, bad), _outcome(compression.decode, bad))
