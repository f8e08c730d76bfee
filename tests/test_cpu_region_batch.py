"""CPU tests of the batched region decode's host side (hic_decode_window_batch_table,
hic_decode420_window_batch_u8): everything wrong with the batch is refused before a
byte of the blob is written and before anything launches, every entry's geometry is
pipeline.window_plan's and window_tiles', and the whole-image batch's table is
unchanged.  No GPU, no kernel calls: the pointers are fakes that are never dereferenced,
so every launch call below is one the library refuses."""
import ctypes
import struct

from hiccup_amd import _lib, pipeline

P = 1 << 32          # fake device addresses (16-byte aligned), never dereferenced
GAP = 1 << 30        # per plane and kind: more than any range of the shapes below
IDX, SLOTS = _lib.STREAM_INDEXED, _lib.STREAM_SLOTS
FIELDS = ("sym_len", "sym_val", "d_nsym", "dc_diff", "d_index", "out", "d_status")
MAGIC = struct.unpack("<Q", b"HICDECW1")[0]
H, W, h, w = 96, 1040, 21, 35


def _images(n):
    arr = (_lib.DecodeImage * max(n, 1))()
    for i in range(n):
        for k in range(3):
            base = P + 8 * GAP * (3 * i + k)
            arr[i].c[k] = _lib.DecodePlane(*(base + j * GAP for j in range(7)))
    return arr


def _build(kind=IDX, n=3, H=H, W=W, h=h, w=w, images=None, origins=None, row_stride=None, pitch=None, rows=None,
           nbytes=None, null=()):
    lib = _lib.load()
    size = lib.hic_decode_window_batch_table_bytes(n) if nbytes is None else nbytes
    buf = ctypes.create_string_buffer(b"\xaa" * max(size, 1), max(size, 1))
    images = _images(min(max(n, 1), 8)) if images is None else images
    origins = [(0, 0)] * max(n, 1) if origins is None else origins
    flat = (ctypes.c_int64 * (2 * len(origins)))(*(v for o in origins for v in o))
    try:
        _, (ch, cw) = pipeline.region_capacity(H, W, h, w)
    except Exception:  # noqa: BLE001 -- a shape the call below refuses anyway
        ch, cw = 8, 8
    rc = lib.hic_decode_window_batch_table(kind, n, H, W, h, w, None if "images" in null else images,
                                           None if "origins" in null else flat,
                                           3 * w if row_stride is None else row_stride, cw if pitch is None else pitch,
                                           ch if rows is None else rows, None if "table" in null else buf, size)
    return rc, buf


def _refused(needle, **kw):
    rc, buf = _build(**kw)
    assert rc == _lib.HIC_ERR_ARG, (needle, kw)
    assert needle in _lib.last_error(), (needle, _lib.last_error())
    assert set(buf.raw) == {0xAA}, "a refused call wrote into the table (%s)" % needle


def _table(**kw):
    rc, buf = _build(**kw)
    assert rc == _lib.HIC_OK, _lib.last_error()
    return buf


def _header(buf):
    return _lib.DecodeWindowHeader.from_buffer_copy(buf.raw[:128])


def _entry(buf, i):
    return _lib.DecodeWindowEntry.from_buffer_copy(buf.raw[128 + 512 * i:128 + 512 * (i + 1)])


def test_exports_and_abi_version():
    lib = _lib.load()
    assert lib.hic_abi_version() == 4
    for name in ("hic_decode_window_batch_table_bytes", "hic_decode_window_batch_table",
                 "hic_decode420_window_batch_u8"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(pipeline.BatchRegionDecoder) and callable(pipeline.batch_region_eligible)
    from hiccup_amd import codec
    assert callable(codec.decode_regions) and callable(codec.decode_regions_device)


def test_table_bytes():
    lib = _lib.load()
    f = lib.hic_decode_window_batch_table_bytes
    assert f(1) == 128 + 512 and f(4096) == 128 + 512 * 4096
    assert f(0) == 0 == f(4097) and f(-1) == 0
    # an entry size that is a power of two
    assert (f(2) - f(1)) & (f(2) - f(1) - 1) == 0


def test_table_refuses_kind_n_shape_window():
    _refused("stream kind", kind=2)
    _refused("HIC_DECODE_BATCH_MAX", n=0)
    _refused("HIC_DECODE_BATCH_MAX", n=4097)
    for HH, WW in ((8, 80), (48, 8), (40, 80), (48, 72), (0, 80), (48, -16), (1 << 20, 16)):
        _refused("image shape", H=HH, W=WW, h=1, w=1)
    _refused("plane too large", H=47104, W=46336)
    _refused("whole records", kind=SLOTS, H=48, W=80)
    for hh, ww in ((0, 35), (21, 0), (-1, 35), (H + 1, 35), (21, W + 1)):
        _refused("window shape", h=hh, w=ww)
    _refused("null pointer", null=("images",))
    _refused("null pointer", null=("origins",))
    _refused("null pointer", null=("table",))
    size = _lib.load().hic_decode_window_batch_table_bytes(3)
    _refused("needed", nbytes=size - 8)


def test_table_refuses_windows_outside_any_image():
    good = [(0, 0), (5, 13), (H - h, W - w)]
    _table(origins=good)
    for i in range(3):
        for bad in ((-1, 0), (0, -1), (H - h + 1, 0), (0, W - w + 1), (H, 0), (1 << 40, 0)):
            o = list(good)
            o[i] = bad
            _refused("image %d: window" % i, origins=o)


def test_table_refuses_strides():
    _refused("out_row_stride", row_stride=3 * w - 1)
    _refused("out_row_stride", row_stride=0)
    _table(row_stride=3 * w + 5)  # any pitch >= 3 w, of any alignment
    _, (ch, cw) = pipeline.region_capacity(H, W, h, w)
    _refused("chroma_pitch", pitch=cw - 8)
    _refused("chroma_pitch", pitch=cw + 4)
    _refused("chroma_rows", rows=ch - 1)
    _table(pitch=cw + 8, rows=ch + 3)


def _bad(images, i, k, **kw):
    for f, v in kw.items():
        setattr(images[i].c[k], f, v)
    return images


def test_table_refuses_bad_pointers_in_any_image():
    for i in (0, 2, 4):
        for k in range(3):
            who = "image %d channel %d" % (i, k)
            for f in FIELDS:
                _refused(who + ": null pointer", n=5, images=_bad(_images(5), i, k, **{f: None}))
            base = P + 8 * GAP * (3 * i + k)
            _refused(who + ": symbol arrays must be 16-byte aligned", n=5,
                     images=_bad(_images(5), i, k, sym_len=base + 8))
            _refused(who + ": slot arrays must be 16-byte aligned", kind=SLOTS, n=5, H=64, W=1024,
                     images=_bad(_images(5), i, k, sym_val=base + GAP + 2))
            _refused(who + ": count / status / DC / index alignment", n=5,
                     images=_bad(_images(5), i, k, d_nsym=base + 2 * GAP + 4))
            _refused(who + ": count / status / DC / index alignment", n=5,
                     images=_bad(_images(5), i, k, d_index=base + 4 * GAP + 4))
            if k:
                _refused(who + ": the chroma window buffer must be 8-byte aligned", n=5,
                         images=_bad(_images(5), i, k, out=base + 5 * GAP + 4))
    # the pixels may start anywhere
    _table(n=5, images=_bad(_images(5), 3, 0, out=P + 8 * GAP * 9 + 5 * GAP + 3))


def test_table_refuses_overlapping_outputs():
    _, (ch, cw) = pipeline.region_capacity(H, W, h, w)
    for k in range(3):
        imgs = _images(3)
        imgs[2].c[k].out = imgs[0].c[k].out
        _refused("overlaps", images=imgs)
        size = (h - 1) * 3 * w + 3 * w if k == 0 else ch * cw
        imgs = _images(3)
        imgs[1].c[k].out = imgs[0].c[k].out + (size - 8 if k else size - 1)
        _refused("image 1 channel %d: its output overlaps the output of image 0 channel %d" % (k, k), images=imgs)
        imgs[1].c[k].out = imgs[0].c[k].out + size  # the first address past it: accepted
        _table(images=imgs)
        imgs = _images(3)
        imgs[2].c[k].d_status = imgs[1].c[(k + 1) % 3].d_status
        _refused("status word", images=imgs)
    imgs = _images(3)
    imgs[2].c[1].out = imgs[0].c[0].out + 8
    _refused("image 2 channel 1: its output overlaps the output of image 0 channel 0", images=imgs)
    # a padded row stride widens the range that must stay free
    imgs = _images(2)
    imgs[1].c[0].out = imgs[0].c[0].out + h * 3 * w
    _table(n=2, images=imgs)
    _refused("overlaps", n=2, images=imgs, row_stride=3 * w + 7)


def _origin_sets(HH, WW, hh, ww):
    o = [(0, 0), (HH - hh, WW - ww), (min(5, HH - hh), min(13, WW - ww)), (min(7, HH - hh), min(3, WW - ww))]
    if WW - ww >= 500:
        o += [(min(16, HH - hh), x0) for x0 in (490, 496, 500, 505)]  # across luma block column 64
    if HH - hh >= 17 and WW - ww >= 17:
        o.append((17, 17))
    return o


def test_entries_are_the_window_plan():
    for kind, HH, WW in ((IDX, 96, 1040), (IDX, 80, 208), (SLOTS, 64, 1024), (SLOTS, 48, 1536), (IDX, 16, 16)):
        for hh, ww in ((1, 1), (16, 16), (21, 35), (HH, WW)):
            hh, ww = min(hh, HH), min(ww, WW)
            origins = _origin_sets(HH, WW, hh, ww)
            n = len(origins)
            imgs = _images(n)
            buf = _table(kind=kind, n=n, H=HH, W=WW, h=hh, w=ww, images=imgs, origins=origins, row_stride=3 * ww + 5)
            (wh, wwid), (ch, cw) = pipeline.region_capacity(HH, WW, hh, ww)
            hd = _header(buf)
            assert (hd.magic, hd.kind, hd.n, hd.H, hd.W, hd.h, hd.w) == (MAGIC, kind, n, HH, WW, hh, ww)
            assert (hd.out_row_stride, hd.chroma_pitch, hd.chroma_rows) == (3 * ww + 5, cw, ch)
            assert (hd.nblk_y, hd.nblk_c) == ((HH // 8) * (WW // 8), (HH // 16) * (WW // 16))
            need_y = need_c = 0
            for i, (y0, x0) in enumerate(origins):
                e = _entry(buf, i)
                p = pipeline.window_plan(HH, WW, y0, x0, hh, ww)
                for k in range(3):
                    assert [getattr(e.c[k], f) for f in FIELDS] == [getattr(imgs[i].c[k], f) for f in FIELDS]
                assert (e.y0, e.x0) == (y0, x0)
                gy, gc = e.g[0], e.g[1]
                assert (gy.bi0, gy.nrows, gy.bj0, gy.bj1) == (p.Y0 // 8, (p.Y1 - p.Y0) // 8, p.X0 // 8, p.X1 // 8)
                assert (gy.oy, gy.ox) == (y0, x0)  # the store crops: out's first pixel is the request's
                assert (gc.bi0, gc.nrows, gc.bj0, gc.bj1) == (p.cy0 // 8, p.ch // 8, p.cx0 // 8, (p.cx0 + p.cw) // 8)
                assert (gc.oy, gc.ox) == (p.cy0, p.cx0)
                for g in (gy, gc):
                    assert (g.cy0, g.cx0, g.ch, g.cw, g.cpitch) == (p.cy0, p.cx0, p.ch, p.cw, cw)
                    assert g.n_ac == g.nrows * (g.bj1 - g.bj0) * 63
                assert p.ch <= ch and p.cw <= cw and p.Y1 - p.Y0 <= wh and p.X1 - p.X0 <= wwid
                # the waves of each launch: per block row as many as the row with the most
                # tiles needs, and their enumeration covers window_tiles' pairs exactly
                for g, chroma, nbx in ((gy, False, WW // 8), (gc, True, WW // 16)):
                    tiles = pipeline.window_tiles(p, WW, chroma=chroma)
                    per_row = {}
                    for bi, t in tiles:
                        per_row.setdefault(bi, []).append(t)
                    assert g.tpr == max(len(v) for v in per_row.values())
                    got = []
                    for r in range(g.nrows * g.tpr):
                        row = r // g.tpr
                        bi = g.bi0 + row
                        t = (bi * nbx + g.bj0) // 64 + (r - row * g.tpr)
                        if t <= (bi * nbx + g.bj1 - 1) // 64:
                            got.append((bi, t))
                    assert got == tiles
                need_y, need_c = max(need_y, gy.nrows * gy.tpr), max(need_c, 2 * gc.nrows * gc.tpr)
            # T: the largest any image of this batch plans, so >= every image's own count
            assert (hd.waves_y, hd.waves_c) == (need_y, need_c)
            assert (hd.grid_y, hd.grid_c) == (-(-n * need_y // 4), -(-n * need_c // 4))


def _launch_refused(needle, table, d_table=P):
    rc = _lib.load().hic_decode420_window_batch_u8(table, d_table, None)
    assert rc == _lib.HIC_ERR_ARG, needle
    assert needle in _lib.last_error(), (needle, _lib.last_error())


def test_launch_refuses_bad_tables():
    off = {name: getattr(_lib.DecodeWindowHeader, name).offset for name, _ in _lib.DecodeWindowHeader._fields_}
    bad = _table()
    bad[3] = bytes([bad.raw[3] ^ 0x40])
    _launch_refused("magic", bad)
    _launch_refused("magic", ctypes.create_string_buffer(128 + 512))
    for field, fmt, value, needle in (("grid_y", "<i", 99, "damaged"), ("grid_c", "<i", 0, "damaged"),
                                      ("waves_y", "<i", 0, "damaged"), ("waves_y", "<i", 1 << 20, "damaged"),
                                      ("waves_c", "<i", 3, "damaged"), ("nblk_y", "<q", 7, "damaged"),
                                      ("pad", "<q", 1, "damaged"), ("H", "<q", 40, "image shape"),
                                      ("n", "<i", 4097, "HIC_DECODE_BATCH_MAX"), ("h", "<q", H + 1, "window shape"),
                                      ("out_row_stride", "<q", 3 * w - 1, "out_row_stride"),
                                      ("chroma_pitch", "<q", 12, "chroma_pitch"), ("chroma_rows", "<q", 1, "chroma_rows")):
        bad = _table()
        struct.pack_into(fmt, bad, off[field], value)
        _launch_refused(needle, bad)
    _launch_refused("null pointer", _table(), d_table=None)
    _launch_refused("null pointer", ctypes.c_void_p(None))
    _launch_refused("16-byte aligned", _table(), d_table=P + 8)
    # the two batched decodes refuse each other's tables
    lib = _lib.load()
    whole = ctypes.create_string_buffer(lib.hic_decode_batch_table_bytes(3))
    assert lib.hic_decode_batch_table(IDX, 3, H, W, 3 * W, W // 2, _images(3), whole, len(whole)) == _lib.HIC_OK
    _launch_refused("magic", whole)
    assert lib.hic_decode420_batch_u8(_table(), P, None) == _lib.HIC_ERR_ARG
    assert "magic" in _lib.last_error()


def test_batch_region_eligible_agrees_with_the_table():
    shapes = [(48, 80), (16, 512), (16, 16), (64, 1024), (96, 1040), (4320, 7680), (40, 80), (48, 72), (8, 16),
              (16, 256), (47104, 46336), (47040, 46336)]
    for HH, WW in shapes:
        for hh, ww in ((1, 1), (16, 16), (21, 35), (HH, WW), (HH + 1, 1), (1, WW + 1), (0, 1), (1, 0)):
            for n in (1, 3, 4096, 0, 4097):
                for kind in (IDX, SLOTS):
                    few = 1 <= n <= 8
                    rc, _ = _build(kind=kind, n=n, H=HH, W=WW, h=hh, w=ww, images=_images(n) if few else None,
                                   null=() if few else ("images",))
                    # (n > 8: the shape checks come before the images are looked at)
                    ok = rc == _lib.HIC_OK if few else "null pointer" in _lib.last_error()
                    assert pipeline.batch_region_eligible(n, HH, WW, hh, ww, slots=kind == SLOTS) == ok, \
                        (n, HH, WW, hh, ww, kind, _lib.last_error())


def test_whole_image_batch_table_is_unchanged():
    """hic_decode_batch_table's blob for a fixed input, byte for byte what the parent of
    the batched region decode wrote (the layout spelled out)."""
    lib = _lib.load()
    n, HH, WW = 3, 48, 80
    imgs = _images(n)
    buf = ctypes.create_string_buffer(b"\xaa" * lib.hic_decode_batch_table_bytes(n), lib.hic_decode_batch_table_bytes(n))
    assert lib.hic_decode_batch_table(IDX, n, HH, WW, 3 * WW + 8, WW // 2 + 4, imgs, buf, len(buf)) == _lib.HIC_OK
    want = struct.pack("<QiiqqqqiiiiQQ", struct.unpack("<Q", b"HICDECB1")[0], IDX, n, HH, WW, 3 * WW + 8, WW // 2 + 4,
                       1, 2, 1, 2, 60, 15) + bytes(48)
    for i in range(n):
        want += struct.pack("<21Q", *(getattr(imgs[i].c[k], f) for k in range(3) for f in FIELDS)) + bytes(88)
    assert buf.raw == want
    assert len(buf.raw) == 128 + 256 * n
