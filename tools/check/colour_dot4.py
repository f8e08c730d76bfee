"""Exhaustive check (all 2^24 RGB triples) that the fused encoder's colour
arithmetic (encode.hip ycc8: two v_dot4_u32_u8 on the high / low bytes of the 4x
luma weights, chroma on 4x-scaled weights read from byte 2, Cr clamped to
[0, 2^24 - 1], Cb not clamped) equals the oracle's OpenCV RGB2YCrCb restatement
(oracle.rgb_to_ycrcb), and that the ranges the missing Cb clamp rests on hold
(ranges()).  Run: python tools/check/colour_dot4.py (about 5 s); also run by
tests/test_cpu_host.py::test_fused_colour_arithmetic_exhaustive and
tests/test_cpu_colour_ranges.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))


CC4 = 4 * ((128 << 14) + (1 << 13))


def dot4_y(r, g, b):
    w4 = (4 * 4899, 4 * 9617, 4 * 1868)
    lo = [w & 255 for w in w4]
    hi = [w >> 8 for w in w4]
    L = r * lo[0] + g * lo[1] + b * lo[2] + 32768
    H = r * hi[0] + g * hi[1] + b * hi[2] + (L >> 8)
    assert int(H.max()) < 1 << 16
    return (H >> 8) & 255


def dot4_ycc(r, g, b):
    y = dot4_y(r, g, b)
    cr = np.clip((r - y) * (4 * 11682) + CC4, 0, 0xFFFFFF) >> 16
    cb = ((b - y) * (4 * 9241) + CC4) >> 16  # no clamp: ranges()
    return y, cr, cb


def all_rgb():
    v = np.arange(1 << 24, dtype=np.int64)
    return v >> 16, (v >> 8) & 255, v & 255


def ranges():
    """Over all 2^24 inputs: b - y lies in [-226, 226], so ycc8's Cb word
    (b - y) * 36964 + 4 * (2^21 + 2^13) lies in [67512, 16775240], inside 24 bits: its
    clamp never fires (and is not there).  The Cr word leaves 24 bits at r - y = 179
    alone, the three inputs r = 255, g = 0, b <= 2: its clamp stays."""
    r, g, b = all_rgb()
    y = dot4_y(r, g, b)
    d = b - y
    assert (int(d.min()), int(d.max())) == (-226, 226)
    vb = d * (4 * 9241) + CC4
    assert (int(vb.min()), int(vb.max())) == (67512, 16775240)
    assert 0 <= int(vb.min()) and int(vb.max()) <= 0xFFFFFF
    vr = (r - y) * (4 * 11682) + CC4
    assert int(vr.min()) >= 0
    over = np.flatnonzero(vr > 0xFFFFFF)
    assert [(int(r[i]), int(g[i]), int(b[i])) for i in over] == [(255, 0, 0), (255, 0, 1), (255, 0, 2)]
    assert all(int(r[i] - y[i]) == 179 for i in over) and int((r - y).max()) == 179
    return True


def check():
    from oracle import oracle
    r, g, b = all_rgb()
    y, cr, cb = dot4_ycc(r, g, b)
    img = np.stack([r, g, b], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    ry, rcr, rcb = (p.reshape(-1).astype(np.int64) for p in oracle.rgb_to_ycrcb(img))
    assert np.array_equal(ry, y) and np.array_equal(rcr, cr) and np.array_equal(rcb, cb)
    return True


if __name__ == "__main__":
    print("dot4 colour arithmetic == oracle on all 2^24 inputs:", check())
    print("Cb word inside 24 bits, Cr clamp at 3 inputs:", ranges())
