"""CPU tests of region decode: the window geometry (pipeline.window_plan and its C
twin hic_window_plan) against brute force, the argument checks of the window entry
points and of hic_rle_stream_index_i16, and hic_window's ctypes layout.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hiccup_amd import _lib, pipeline

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 1024), (48, 1536), (80, 208), (96, 1040), (16, 16)]


def _windows(H, W, n=200):
    rng = np.random.default_rng(H * 10007 + W)
    out = [(0, 0, H, W), (H - 1, W - 1, 1, 1), (0, 0, 1, 1), (0, 0, 16, W), (0, 0, H, min(16, W))]
    while len(out) < n:
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        out.append((y0, x0, int(rng.integers(1, H - y0 + 1)), int(rng.integers(1, W - x0 + 1))))
    return out


def _c_plan(H, W, y0, x0, h, w):
    win = _lib.Window()
    rc = _lib.load().hic_window_plan(H, W, y0, x0, h, w, ctypes.byref(win))
    return rc, tuple(getattr(win, f) for f, _ in _lib.Window._fields_)


def _pyr_up_taps(i, n):
    """The chroma samples pyrUp reads for output sample i of a 2n-sample axis: i // 2
    and its neighbours, reflect-101 at 0 and replicate at the end (pyr_up_at)."""
    c = i // 2
    taps = (c - 1, c, c + 1) if i % 2 == 0 else (c, c + 1)
    return {1 if t < 0 else min(t, n - 1) for t in taps}


@pytest.mark.parametrize("H,W", SHAPES)
def test_window_plan_brute_force(H, W):
    for (y0, x0, h, w) in _windows(H, W):
        p = pipeline.window_plan(H, W, y0, x0, h, w)
        rc, c = _c_plan(H, W, y0, x0, h, w)
        assert rc == _lib.HIC_OK and c == tuple(p), (y0, x0, h, w)
        # the aligned window covers the request, inside the image, 16-aligned
        assert p.Y0 <= y0 and p.X0 <= x0 and p.Y1 >= y0 + h and p.X1 >= x0 + w
        assert 0 <= p.Y0 < p.Y1 <= H and 0 <= p.X0 < p.X1 <= W
        assert not any(v % 16 for v in (p.Y0, p.X0, p.Y1, p.X1))
        assert p.Y0 > y0 - 16 and p.Y1 < y0 + h + 16 and p.X0 > x0 - 16 and p.X1 < x0 + w + 16
        # the chroma span: whole 8x8 blocks inside the plane ...
        assert not any(v % 8 for v in (p.cy0, p.cx0, p.ch, p.cw))
        assert 0 <= p.cy0 and p.cy0 + p.ch <= H // 2 and 0 <= p.cx0 and p.cx0 + p.cw <= W // 2
        # ... holding every sample pyrUp reads for a pixel of the aligned window
        rows = set().union(*(_pyr_up_taps(y, H // 2) for y in range(p.Y0, p.Y1)))
        cols = set().union(*(_pyr_up_taps(x, W // 2) for x in range(p.X0, p.X1)))
        assert min(rows) >= p.cy0 and max(rows) < p.cy0 + p.ch, (y0, x0, h, w)
        assert min(cols) >= p.cx0 and max(cols) < p.cx0 + p.cw, (y0, x0, h, w)
        # ... and no more than one block beyond them
        assert p.cy0 > min(rows) - 8 and p.cy0 + p.ch < max(rows) + 1 + 8
        assert p.cx0 > min(cols) - 8 and p.cx0 + p.cw < max(cols) + 1 + 8
        # every block of either launch's window lies in an enumerated tile of its row
        for chroma in (False, True):
            nbx = W // 16 if chroma else W // 8
            if chroma:
                bi0, bi1, bj0, bj1 = p.cy0 // 8, (p.cy0 + p.ch) // 8, p.cx0 // 8, (p.cx0 + p.cw) // 8
            else:
                bi0, bi1, bj0, bj1 = p.Y0 // 8, p.Y1 // 8, p.X0 // 8, p.X1 // 8
            tiles = pipeline.window_tiles(p, W, chroma)
            have = set(tiles)
            assert len(have) == len(tiles)
            for bi in range(bi0, bi1):
                for bj in range(bj0, bj1):
                    assert (bi, (bi * nbx + bj) // 64) in have
            # and every enumerated tile holds a block of its row's columns (none is wasted)
            for bi, t in tiles:
                assert any((bi * nbx + bj) // 64 == t for bj in range(bj0, bj1))
        # the buffers fit the capacity of any RegionDecoder that accepts the request
        for mh, mw in ((h, w), (H, W), (min(H, h + 7), min(W, w + 3))):
            (wh, ww), (ch, cw) = pipeline.region_capacity(H, W, mh, mw)
            assert (p.Y1 - p.Y0) * (p.X1 - p.X0) <= wh * ww and p.Y1 - p.Y0 <= wh and p.X1 - p.X0 <= ww
            assert p.ch <= ch and p.cw <= cw


def test_window_plan_refuses():
    for args in ((64, 1024, -1, 0, 4, 4), (64, 1024, 0, 0, 65, 4), (64, 1024, 60, 1020, 4, 5), (64, 1024, 0, 0, 0, 4),
                 (60, 1024, 0, 0, 4, 4), (64, 1000, 0, 0, 4, 4), (0, 0, 0, 0, 1, 1)):
        with pytest.raises(ValueError):
            pipeline.window_plan(*args)
        assert _c_plan(*args)[0] == _lib.HIC_ERR_ARG, args
    assert _lib.load().hic_window_plan(64, 64, 0, 0, 4, 4, None) == _lib.HIC_ERR_ARG


# Every call below must be refused: an accepted one would launch a kernel on these fake
# pointers on a machine with a GPU.
P = 1 << 20  # never dereferenced (16-byte aligned)


def _refused(fn, args, needle=None):
    assert fn(*args) == _lib.HIC_ERR_ARG, (fn.__name__, args)
    if needle is not None:
        assert needle in _lib.last_error(), (fn.__name__, args, _lib.last_error())


def _win(H=64, W=1024, y0=16, x0=496, h=16, w=48, **over):
    d = pipeline.window_plan(H, W, y0, x0, h, w)._asdict()
    d.update(over)
    return _lib.Window(**d)


def test_window_entry_points_refuse_bad_input():
    """hic_rle_decode_idct_rgb_window / _u8_window_pair check everything before any device
    call: null pointers, the stream kind, a window outside the image, an unaligned
    window, a chroma span that is not the plan's, misaligned pitches and planes,
    misaligned symbol arrays, the slot forms' record geometry."""
    lib = _lib.load()
    two = lambda a=P, b=P: (ctypes.c_void_p * 2)(a, b)  # noqa: E731

    def rgb(kind=0, L=P, rpt=1, H=64, W=1024, win="plan", cr=P, cstride=None, out=P, stride=None, status=P):
        wn = _win(H, W) if win == "plan" else win
        cs = wn.cw if cstride is None and wn is not None else cstride
        st = 3 * (wn.X1 - wn.X0) if stride is None and wn is not None else stride
        return [kind, L, P, P, P, P, rpt, H, W, ctypes.byref(wn) if wn is not None else None, cr, P, cs or 0, out,
                st or 0, status, None]

    def pair(kind=0, L=None, rpt=2, H=64, W=1024, win="plan", out=None, stride=None, status=None):
        wn = _win(H, W) if win == "plan" else win
        st = wn.cw if stride is None and wn is not None else stride
        return [kind, L or two(), two(), two(), two(), two(), rpt, H, W, ctypes.byref(wn) if wn is not None else None,
                out or two(), st or 0, status or two(), None]

    f_rgb, f_pair = lib.hic_rle_decode_idct_rgb_window, lib.hic_rle_decode_idct_u8_window_pair
    for kind in (_lib.STREAM_INDEXED, _lib.STREAM_SLOTS):
        # null pointers
        _refused(f_rgb, rgb(kind, L=None), "null pointer")
        _refused(f_rgb, rgb(kind, status=None), "null pointer")
        _refused(f_rgb, rgb(kind, cr=None), "null pointer")
        _refused(f_rgb, rgb(kind, win=None), "null pointer")
        _refused(f_pair, pair(kind, L=two(b=None)), "plane 1: null pointer")
        _refused(f_pair, pair(kind, win=None), "null pointer")
        args = pair(kind)
        args[1] = None
        _refused(f_pair, args, "null pointer")
        # a window outside the image, an unaligned kernel-level window, a foreign chroma span
        for fn, mk in ((f_rgb, rgb), (f_pair, pair)):
            _refused(fn, mk(kind, win=_win(Y1=80)), "outside")
            _refused(fn, mk(kind, win=_win(X0=1024, X1=1040)), "outside")
            _refused(fn, mk(kind, win=_win(Y0=32, Y1=32)), "outside")
            _refused(fn, mk(kind, win=_win(X0=500)), "16-pixel aligned")
            _refused(fn, mk(kind, win=_win(Y1=40)), "16-pixel aligned")
            _refused(fn, mk(kind, win=_win(cx0=248)), "chroma span")
            _refused(fn, mk(kind, win=_win(ch=16)), "chroma span")
            _refused(fn, mk(kind, H=60, win=_win()), "multiples of 16")
            _refused(fn, mk(kind, W=1000, win=_win()), "multiples of 16")
        # misaligned chroma pitch / planes, RGB pitch
        _refused(f_rgb, rgb(kind, cstride=_win().cw + 2), "chroma pitch")
        _refused(f_rgb, rgb(kind, cstride=_win().cw - 4), "chroma pitch")
        _refused(f_rgb, rgb(kind, cr=P + 2), "4-byte aligned")
        _refused(f_rgb, rgb(kind, stride=3 * 48 + 4), "rgb stride")
        _refused(f_rgb, rgb(kind, stride=3 * 48 - 8), "rgb stride")
        _refused(f_rgb, rgb(kind, out=P + 4), "rgb stride")
        _refused(f_pair, pair(kind, stride=_win().cw + 4), "chroma pitch")
        _refused(f_pair, pair(kind, stride=_win().cw - 8), "chroma pitch")
        _refused(f_pair, pair(kind, out=two(b=P + 4)), "8-byte aligned")
        # symbol arrays
        _refused(f_rgb, rgb(kind, L=P + 8), "16-byte aligned")
        _refused(f_pair, pair(kind, L=two(b=P + 8)), "16-byte aligned")
    _refused(f_rgb, rgb(2), "stream kind")
    _refused(f_pair, pair(-1), "stream kind")
    # the slot forms: records per tile, whole records
    _refused(f_rgb, rgb(_lib.STREAM_SLOTS, rpt=3), "records_per_tile")
    _refused(f_pair, pair(_lib.STREAM_SLOTS, rpt=3), "records_per_tile")
    _refused(f_pair, pair(_lib.STREAM_SLOTS, rpt=0), "records_per_tile")
    w16 = _win(16, 16, 0, 0, 16, 16)
    _refused(f_rgb, rgb(_lib.STREAM_SLOTS, H=16, W=16, win=w16), "whole records")  # 4 blocks
    _refused(f_pair, pair(_lib.STREAM_SLOTS, H=16, W=16, win=w16), "whole records")


def test_stream_index_refuses_bad_input():
    lib = _lib.load()
    fn = lib.hic_rle_stream_index_i16
    ok = lambda L=P, V=P, nsym=100, D=P, nblk=64, ix=P, st=P, ws=P: [L, V, nsym, D, nblk, ix, st, ws, None]  # noqa: E731
    for k in ("L", "V", "D", "ix", "st", "ws"):
        _refused(fn, ok(**{k: None}), "null pointer")
    _refused(fn, ok(nsym=-1), "nsym")
    _refused(fn, ok(nblk=0), "nblk")
    _refused(fn, ok(nblk=(1 << 31) // 63 + 1), "nblk")
    _refused(fn, ok(L=P + 8), "16-byte aligned")
    _refused(fn, ok(V=P + 2), "16-byte aligned")
    # the workspace grows with both arguments and is never empty
    size = lib.hic_rle_stream_index_workspace_bytes
    assert size(0, 1) > 0 and size(1 << 20, 1 << 16) > size(1 << 10, 1 << 16) > size(1 << 10, 64)


def test_window_struct_matches_header(tmp_path):
    """_lib.Window has hic_window's size and field offsets, as gcc lays them out."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hiccup_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(hic_window));']
    for f, _ in _lib.Window._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(hic_window, %s));' % (f, f))
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                         text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.Window)
    for f, _ in _lib.Window._fields_:
        assert int(got[f]) == getattr(_lib.Window, f).offset, f
