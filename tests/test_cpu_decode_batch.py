"""CPU tests of the batched decode's host side (hic_decode_batch_table,
hic_decode420_batch_u8): every bad image, stride, shape or table is refused before
anything launches and before a byte of the blob is written, and the header a good
call writes holds the wave counts and grids of its shape.  No GPU, no kernel calls:
the pointers are fakes that are never dereferenced, so the launch calls below are all
ones the library refuses (the table builder launches nothing and may succeed).

One item of the builder's list cannot be reached through its own arguments: a grid
above INT32_MAX workgroups needs more than 2^33 waves, and n <= 4096 images of planes
below 2^31 AC positions (at most 532 610 tiles each) stay under 2^32.  The check is in
the library; test_table_refuses_sizes pins the bounds that make it unreachable."""
import ctypes
import struct

from hiccup_amd import _lib, pipeline

P = 1 << 32          # fake device addresses (16-byte aligned), never dereferenced
GAP = 1 << 30        # per plane and kind: more than any range of the shapes below
IDX, SLOTS = _lib.STREAM_INDEXED, _lib.STREAM_SLOTS
FIELDS = ("sym_len", "sym_val", "d_nsym", "dc_diff", "d_index", "out", "d_status")
MAGIC = struct.unpack("<Q", b"HICDECB1")[0]


def _images(n):
    """n good images: every range of every kind apart from every other."""
    arr = (_lib.DecodeImage * max(n, 1))()
    for i in range(n):
        for k in range(3):
            base = P + 8 * GAP * (3 * i + k)
            arr[i].c[k] = _lib.DecodePlane(*(base + j * GAP for j in range(7)))
    return arr


def _build(kind, n, H, W, images=None, rgb_stride=None, chroma_stride=None, nbytes=None, null_images=False,
           null_table=False):
    lib = _lib.load()
    size = lib.hic_decode_batch_table_bytes(n) if nbytes is None else nbytes
    buf = ctypes.create_string_buffer(b"\xaa" * max(size, 1), max(size, 1))
    images = _images(min(max(n, 1), 8)) if images is None else images
    rc = lib.hic_decode_batch_table(kind, n, H, W, 3 * W if rgb_stride is None else rgb_stride,
                                    W // 2 if chroma_stride is None else chroma_stride,
                                    None if null_images else images, None if null_table else buf, size)
    return rc, buf


def _refused(needle, *a, **kw):
    rc, buf = _build(*a, **kw)
    assert rc == _lib.HIC_ERR_ARG, needle
    assert needle in _lib.last_error(), (needle, _lib.last_error())
    assert set(buf.raw) == {0xAA}, "a refused call wrote into the table (%s)" % needle


def _table(kind=IDX, n=3, H=48, W=80, **kw):
    rc, buf = _build(kind, n, H, W, images=_images(n), **kw)
    assert rc == _lib.HIC_OK, _lib.last_error()
    return buf


def _header(buf):
    names = ("magic", "kind", "n", "H", "W", "rgb_stride", "chroma_stride", "tiles_y", "tiles_c", "grid_y", "grid_c",
             "nblk_y", "nblk_c")
    return dict(zip(names, struct.unpack_from("<QiiqqqqiiiiQQ", buf.raw, 0)))


def test_abi_version_unchanged():
    assert _lib.load().hic_abi_version() == 4


def test_table_bytes():
    lib = _lib.load()
    assert pipeline.DECODE_BATCH_MAX == 4096
    sizes = [lib.hic_decode_batch_table_bytes(n) for n in (1, 2, 3, 64, 4095, 4096)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.hic_decode_batch_table_bytes(0) == 0 == lib.hic_decode_batch_table_bytes(4097)
    assert lib.hic_decode_batch_table_bytes(-1) == 0


def test_table_refuses_sizes():
    lib = _lib.load()
    _refused("HIC_DECODE_BATCH_MAX", IDX, 0, 48, 80)
    _refused("HIC_DECODE_BATCH_MAX", IDX, 4097, 48, 80)
    _refused("stream kind", 2, 2, 48, 80)
    _refused("null pointer", IDX, 2, 48, 80, null_images=True)
    _refused("null pointer", IDX, 2, 48, 80, null_table=True)
    _refused("needed", IDX, 2, 48, 80, nbytes=lib.hic_decode_batch_table_bytes(2) - 8)
    _refused("needed", IDX, 2, 48, 80, nbytes=lib.hic_decode_batch_table_bytes(1))
    # the largest batch of the largest planes stays within 32-bit wave counts (module docstring)
    tiles = ((2**31 - 1) // 63 + 63) // 64
    assert 4096 * tiles + 3 < 2**32


def test_table_refuses_shapes_and_strides():
    for H, W in ((8, 80), (48, 8), (40, 80), (48, 72), (0, 80), (48, -16), (1 << 20, 16)):
        _refused("image shape", IDX, 1, H, W)
    _refused("rgb_stride", IDX, 1, 48, 80, rgb_stride=3 * 80 - 8)
    _refused("rgb_stride", IDX, 1, 48, 80, rgb_stride=3 * 80 + 4)
    _refused("chroma_stride", IDX, 1, 48, 80, chroma_stride=36)
    _refused("chroma_stride", IDX, 1, 48, 80, chroma_stride=42)
    # nblk * 63 >= 2^31 (5888 x 5792 blocks); just below it the one-image entry points'
    # own block limit (2^23) still refuses the shape, and 8176 x 8192 (2^20 - 1024 blocks) fits
    _refused("plane too large", IDX, 1, 47104, 46336)
    _refused("image shape", IDX, 1, 47040, 46336)
    rc, _ = _build(IDX, 1, 8176, 8192, images=_images(1))
    assert rc == _lib.HIC_OK, _lib.last_error()
    # slots: whole records (Y: 64 blocks, chroma: 32)
    _refused("whole records", SLOTS, 1, 48, 80)      # Y 60 blocks
    _refused("whole records", SLOTS, 1, 16, 256)     # Y 64 blocks, chroma 16
    rc, _ = _build(SLOTS, 1, 16, 512, images=_images(1))
    assert rc == _lib.HIC_OK, _lib.last_error()


def _bad(images, i, k, **kw):
    for f, v in kw.items():
        setattr(images[i].c[k], f, v)
    return images


def test_table_refuses_bad_planes_in_any_image():
    for i in (0, 2, 4):
        for k in range(3):
            who = "image %d channel %d" % (i, k)
            for f in FIELDS:
                _refused(who + ": null pointer", IDX, 5, 48, 80, images=_bad(_images(5), i, k, **{f: None}))
            base = P + 8 * GAP * (3 * i + k)
            _refused(who + ": symbol arrays must be 16-byte aligned", IDX, 5, 48, 80,
                     images=_bad(_images(5), i, k, sym_len=base + 8))
            _refused(who + ": slot arrays must be 16-byte aligned", SLOTS, 5, 16, 512,
                     images=_bad(_images(5), i, k, sym_val=base + GAP + 2))
            _refused(who + ": out must be 8-byte aligned", IDX, 5, 48, 80,
                     images=_bad(_images(5), i, k, out=base + 5 * GAP + 4))
            _refused(who + ": count / status / DC / index alignment", IDX, 5, 48, 80,
                     images=_bad(_images(5), i, k, d_nsym=base + 2 * GAP + 4))
            _refused(who + ": count / status / DC / index alignment", IDX, 5, 48, 80,
                     images=_bad(_images(5), i, k, d_index=base + 4 * GAP + 4))
            # (the slot layout's record index is int32: 4 bytes are enough)
            rc, _ = _build(SLOTS, 5, 16, 512, images=_bad(_images(5), i, k, d_index=base + 4 * GAP + 4))
            assert rc == _lib.HIC_OK, _lib.last_error()


def test_table_refuses_overlapping_outputs():
    H, W = 48, 80
    for k in range(3):  # two images' RGB / Cr / Cb: equal, then overlapping by one byte
        imgs = _images(3)
        imgs[2].c[k].out = imgs[0].c[k].out
        _refused("overlaps", IDX, 3, H, W, images=imgs)
        imgs = _images(3)
        size = (H - 1) * 3 * W + 3 * W if k == 0 else (H // 2 - 1) * (W // 2) + W // 2
        imgs[1].c[k].out = imgs[0].c[k].out + (size + 7) // 8 * 8 - 8
        _refused("image 1 channel %d: its output overlaps the output of image 0 channel %d" % (k, k), IDX, 3, H, W,
                 images=imgs)
        imgs[1].c[k].out = imgs[0].c[k].out + (size + 7) // 8 * 8  # the first address past it: accepted
        rc, _ = _build(IDX, 3, H, W, images=imgs)
        assert rc == _lib.HIC_OK, _lib.last_error()
        imgs = _images(3)
        imgs[2].c[k].d_status = imgs[1].c[(k + 1) % 3].d_status
        _refused("status word", IDX, 3, H, W, images=imgs)
    # an image's RGB over another image's chroma plane, and over its own
    imgs = _images(3)
    imgs[2].c[1].out = imgs[0].c[0].out + 3 * W * 8
    _refused("image 2 channel 1: its output overlaps the output of image 0 channel 0", IDX, 3, H, W, images=imgs)
    imgs = _images(3)
    imgs[1].c[2].out = imgs[1].c[0].out + 16
    _refused("overlaps", IDX, 3, H, W, images=imgs)
    # a padded stride widens the range that must stay free
    imgs = _images(2)
    imgs[1].c[0].out = imgs[0].c[0].out + H * 3 * W
    rc, _ = _build(IDX, 2, H, W, images=imgs)
    assert rc == _lib.HIC_OK, _lib.last_error()
    _refused("overlaps", IDX, 2, H, W, images=imgs, rgb_stride=3 * W + 8)


def test_table_header_and_entries():
    lib = _lib.load()
    for kind, n, H, W in ((IDX, 3, 48, 80), (SLOTS, 5, 16, 512), (IDX, 4096, 16, 16), (SLOTS, 3, 80, 1024)):
        imgs = _images(n)
        rc, buf = _build(kind, n, H, W, images=imgs, rgb_stride=3 * W + 8, chroma_stride=W // 2 + 4)
        assert rc == _lib.HIC_OK, _lib.last_error()
        h = _header(buf)
        ny, nc = (H // 8) * (W // 8), (H // 16) * (W // 16)
        ty, tc = -(-ny // 64), 2 * -(-nc // 64)
        assert h == dict(magic=MAGIC, kind=kind, n=n, H=H, W=W, rgb_stride=3 * W + 8, chroma_stride=W // 2 + 4,
                         tiles_y=ty, tiles_c=tc, grid_y=-(-n * ty // 4), grid_c=-(-n * tc // 4), nblk_y=ny, nblk_c=nc)
        # one 256-byte entry per image after the 128-byte header: Y, Cr, Cb, 7 pointers each
        assert len(buf.raw) == lib.hic_decode_batch_table_bytes(n) == 128 + 256 * n
        for i in (0, n // 2, n - 1):
            words = struct.unpack_from("<21Q", buf.raw, 128 + 256 * i)
            want = [getattr(imgs[i].c[k], f) for k in range(3) for f in FIELDS]
            assert list(words) == want, i
    # the shapes of the GPU tests: waves per image and grids
    for (n, H, W), (ty, tc, gy, gc) in {(3, 48, 80): (1, 2, 1, 2), (5, 16, 512): (2, 2, 3, 3),
                                        (4096, 16, 16): (1, 2, 1024, 2048)}.items():
        h = _header(_table(IDX, n, H, W))
        assert (h["tiles_y"], h["tiles_c"], h["grid_y"], h["grid_c"]) == (ty, tc, gy, gc), (n, H, W)


def _launch_refused(needle, table, d_table=P):
    rc = _lib.load().hic_decode420_batch_u8(table, d_table, None)
    assert rc == _lib.HIC_ERR_ARG, needle
    assert needle in _lib.last_error(), (needle, _lib.last_error())


def test_launch_refuses_bad_tables():
    bad = _table()
    bad[3] = bytes([bad.raw[3] ^ 0x40])
    _launch_refused("magic", bad)
    _launch_refused("magic", ctypes.create_string_buffer(128 + 256))
    bad = _table()
    struct.pack_into("<i", bad, 56, 99)  # a grid that is not the shape's
    _launch_refused("damaged", bad)
    bad = _table()
    struct.pack_into("<q", bad, 16, 40)  # H no multiple of 16
    _launch_refused("image shape", bad)
    bad = _table()
    struct.pack_into("<i", bad, 12, 4097)
    _launch_refused("HIC_DECODE_BATCH_MAX", bad)
    _launch_refused("null pointer", _table(), d_table=None)
    _launch_refused("null pointer", ctypes.c_void_p(None))
    _launch_refused("16-byte aligned", _table(), d_table=P + 8)


def test_batch_decode_eligible_agrees_with_the_table():
    shapes = [(48, 80), (16, 512), (16, 16), (80, 1024), (96, 1040), (4320, 7680), (40, 80), (48, 72), (8, 16),
              (16, 256), (47104, 46336), (47040, 46336)]
    for H, W in shapes:
        for n in (1, 3, 4096):
            for kind in (IDX, SLOTS):
                rc, _ = _build(kind, n, H, W, images=_images(min(n, 8)) if n <= 8 else None, null_images=n > 8)
                # (n > 8: the shape checks come before the images are looked at)
                ok = rc == _lib.HIC_OK if n <= 8 else "null pointer" in _lib.last_error()
                assert pipeline.batch_decode_eligible(n, H, W, slots=kind == SLOTS) == ok, (n, H, W, kind)
    for n in (0, -1, 4097):
        assert not pipeline.batch_decode_eligible(n, 48, 80)
