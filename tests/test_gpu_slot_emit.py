"""Round 13's emission loop of the slot encoder (slot_pass section 3,
hiccup_amd/csrc/slots.h) against the C oracle.  The loop carries two values per
lane, each a multiply-add on the coefficient's zero flag: the run counter
c = (zeros since the last nonzero), which starts at rem - first and is NEGATIVE
when the block opens with more zeros than the carried run, and the store address
less twice the coefficient index, which sinks up to 124 bytes below the lane's
first slot.  Data that the other files' kinds do not pin, each built from DCT basis
functions (the oracle's own inverse transform of chosen quantized coefficients)
added to a flat grey image, and each checked on the ORACLE's blocks before the GPU
is touched:
  late   blocks whose first nonzero AC has index >= 40: the head lane of a record
         (lane 0, rem = 0) and blocks after all-zero blocks (carried run: fillers
         and a remainder before the first symbol);
  edge   blocks with AC 62 nonzero, blocks with AC 0 nonzero and nothing else, an
         all-zero block in lane 0 of a record whose later lanes have symbols, and
         one in lane 63;
  run14  runs of exactly 14 zeros inside a block (the largest length the loop
         writes itself: a length-14 symbol with a value, no filler in that block)
         and, in other blocks, runs of exactly 15 (the first to take the out-of-line
         packed emission);
  comb   nonzero / zero coefficients alternating over all 63 AC of a block, on the
         even and on the odd AC, in luminance and in both chroma planes (the
         two-record pass).
Shapes: one unit (wave 0 / lane 0 holds the lowest stage address), a full 4-unit
band, two strips, a band plus a short band; both encode_band values.  One case
drives the same slot_pass through hic_slots_fill_batch (the "slots" gather of two
shards on one device).
Reference: compression.jpeg_compression + codec.jpeg_encode's DC / AC coding, as
restated in oracle/hiccup_oracle.c."""
import functools

import numpy as np
import pytest

import oracle.oracle as orc
import oracle.oracle_c as orcc
from hiccup_amd import _lib, device, pipeline

SHAPES = [(16, 512), (32, 512), (64, 1024), (80, 1024)]
KINDS = ["late", "edge", "run14", "comb"]
UNZZ = np.argsort(orc.ZZ8)  # zig-zag blocks [:, UNZZ] -> raster order


def _spatial(tz, table_id):
    """(nblk, 64) quantized zig-zag targets -> (nblk, 8, 8) pixel offsets from 128."""
    deq = tz[:, UNZZ].reshape(-1, 8, 8) * orc.TABLES[table_id]
    return orc.idct2(deq.astype(np.float64))


def _pyr_matrix(n):
    """pyrDown along one axis as an (n / 2, n) matrix (reflect-101 borders)."""
    D = np.zeros((n // 2, n))
    for i in range(n // 2):
        for k, wgt in zip(range(-2, 3), (1, 4, 6, 4, 1)):
            j = 2 * i + k
            j = -j if j < 0 else (2 * n - 2 - j if j >= n else j)
            D[i, j] += wgt / 16.0
    return D


def _rgb(Y, Cr, Cb):
    """RGB whose YCrCb is (Y, Cr, Cb) up to rounding (the inverse of the oracle's
    fixed-point forward transform, in floating point)."""
    R = Y + (Cr - 128.0) / 0.713
    B = Y + (Cb - 128.0) / 0.564
    G = (Y - 0.299 * R - 0.114 * B) / 0.587
    return np.clip(np.rint(np.stack([R, G, B], -1)), 0, 255).astype(np.uint8)


def _targets(kind, H, W):
    """Quantized zig-zag targets per channel: {k: (nblk, 64) int}."""
    nby, nbx = H // 8, W // 8
    rng = np.random.default_rng(100 * H + W)
    T = {"lum": np.zeros((nby * nbx, 64), np.int64), "cr": np.zeros((nby * nbx // 4, 64), np.int64),
         "cb": np.zeros((nby * nbx // 4, 64), np.int64)}
    L = T["lum"].reshape(nby, nbx, 64)
    for br in range(nby):
        for rec in range(nbx // 64):
            blk = L[br, 64 * rec:64 * rec + 64]  # one luminance record: lane = block
            sgn = lambda: int(rng.choice((-2, 2)))  # noqa: E731
            if kind == "late":
                # head lane with its first nonzero late; then late blocks after 0-3 zero blocks
                blk[0, 1 + 40 + (br + rec) % 23] = sgn()
                lane = 1
                while lane < 64:
                    lane += int(rng.integers(0, 4))
                    if lane >= 64:
                        break
                    f = int(rng.integers(40, 63))
                    blk[lane, 1 + f] = sgn()
                    if f < 62 and rng.random() < 0.5:
                        blk[lane, 1 + int(rng.integers(f + 1, 63))] = sgn()
                    lane += 1
            elif kind == "edge":
                for lane in range(1, 63):  # lanes 0 and 63 stay all-zero
                    r = (lane + br) % 4
                    if r == 0:
                        blk[lane, 1 + 62] = sgn()
                    elif r == 1:
                        blk[lane, 1 + 0] = sgn()
                    elif r == 2:
                        blk[lane, 1 + 0] = sgn()
                        blk[lane, 1 + 62] = sgn()
            elif kind == "run14":
                for lane in range(64):
                    r = (lane + 2 * br + rec) % 3
                    if r == 2:
                        continue
                    gap = 15 if r == 0 else 16  # 14 / 15 zeros between the two
                    a = int(rng.integers(0, 63 - gap))
                    blk[lane, 1 + a] = sgn()
                    blk[lane, 1 + a + gap] = sgn()
            elif kind == "comb":
                for lane in range(4, 64, 2):  # (block columns clear of the chroma combs)
                    if lane % 8 < 4:
                        continue
                    ph = (lane // 2 + br) % 2  # the comb on the even or on the odd AC
                    blk[lane, 1 + ph:64:2] = rng.choice((-2, 2), len(range(1 + ph, 64, 2)))
            else:
                raise ValueError(kind)
    if kind == "comb":
        for k in ("cr", "cb"):
            C = T[k]
            for b in range(0, len(C), 4):  # luminance block columns 8m, 8m + 1
                ph = (b // 4 + (k == "cb")) % 2
                idx = np.arange(1 + ph, 64, 2)
                C[b, idx] = rng.choice((-2, 2), len(idx))
    return T


def _dct_float(plane, table_id):
    """the unquantized DCT of a uint8 plane's blocks over the table: (nblk, 64) zig-zag"""
    b = orc.dct2(orc.split_blocks(plane.astype(np.int64) - 128).astype(np.float64)) / orc.TABLES[table_id]
    return b.reshape(-1, 64)[:, orc.ZZ8]


def _img(kind, H, W):
    """The image whose quantized blocks have the targets' zero / nonzero pattern.
    A pixel's rounding moves a coefficient by a few units (the transform is not
    normalized: a basis function of amplitude 1 is a coefficient of 16), which is
    comparable to the smallest table entries.  Chroma: the float planes are corrected
    by the coefficients that miss and rounded again.  Luminance (grey blocks, where
    Y = R = G = B): single pixels are stepped by one, greedily, until every AC that
    should be zero rounds to zero and every other one does not."""
    T = _targets(kind, H, W)
    PH, PW = np.linalg.pinv(_pyr_matrix(H)), np.linalg.pinv(_pyr_matrix(W)).T
    want = {k: T[k].astype(np.float64) for k in ("cr", "cb")}
    Y = 128.0 + orc.merge_blocks(_spatial(T["lum"], 0), (H, W))
    near = {}
    for k in want:
        on = orc.merge_blocks(np.repeat((T[k] != 0).any(1), 64).reshape(-1, 8, 8), (H // 2, W // 2))
        on = np.pad(on.repeat(2, 0).repeat(2, 1), 8)
        near[k] = np.max([np.roll(on, (dy, dx), (0, 1)) for dy in (-8, 0, 8) for dx in (-8, 0, 8)], 0)[8:-8, 8:-8]
    for _ in range(40):
        # the full-resolution planes whose pyrDown is the target (minimum norm)
        # (cut off 8 pixels beyond the blocks with a target, so the rest of the image
        # stays grey: what that costs those blocks the correction below makes up)
        full = {k: 128.0 + near[k] * (PH @ orc.merge_blocks(_spatial(want[k], 1), (H // 2, W // 2)) @ PW)
                for k in want}
        rgb = _rgb(Y, full["cr"], full["cb"])
        _, cr, cb = orcc.rgb_to_ycrcb(rgb)
        bad = 0
        for k, p in (("cr", orcc.pyr_down(cr)), ("cb", orcc.pyr_down(cb))):
            got = _dct_float(p, 1)
            miss = _misses(got, T[k])
            bad += int(miss.sum())
            want[k] = want[k] - np.where(miss, got - T[k], 0.0)
        if bad == 0:
            break
    # luminance, block by block
    rng = np.random.default_rng(H + W)
    unit = _dct_float((128 + np.eye(64, dtype=np.int64)).reshape(64 * 8, 8), 0)  # [pixel] -> its coefficients
    moves = np.concatenate([unit, -unit])  # pixel + 1 (64), pixel - 1 (64)
    blocks = orc.split_blocks(rgb[..., 0].astype(np.int64))
    grey = orc.split_blocks(((rgb[..., 0] == rgb[..., 1]) & (rgb[..., 1] == rgb[..., 2])).astype(np.int64))
    for b in np.flatnonzero(grey.reshape(-1, 64).all(1)):
        px = blocks[b].reshape(64).copy()
        g = (px - 128) @ unit
        for _ in range(800):
            c = _cost(g, T["lum"][b])
            if c == 0:
                break
            cand = _cost(g[None, :] + moves, T["lum"][b][None, :])
            cand = np.where(np.concatenate([px < 255, px > 0]), cand, np.inf)
            m = int(np.argmin(cand))
            if cand[m] >= c:  # a local minimum: one of the eight least bad steps instead
                m = int(rng.choice(np.argsort(cand)[:8]))
            px[m % 64] += 1 if m < 64 else -1
            g = g + moves[m]
        blocks[b] = px.reshape(8, 8)
    grey_px = orc.merge_blocks(grey, (H, W)) == 1
    lum = orc.merge_blocks(blocks, (H, W)).astype(np.uint8)
    return np.where(grey_px[..., None], lum[..., None], rgb)


# a coefficient over its table entry that should round to 0 lies within 0.45, with a
# margin to the rounding point (the oracle's transform and this one agree to 1e-10);
# one that should not (a target of magnitude >= 1) at 0.55 or beyond
def _misses(got, target):
    miss = np.where(target == 0, np.abs(got) > 0.45, np.abs(got) < 0.55)
    miss[..., 0] = False
    return miss


def _cost(got, target):
    over = np.where(target == 0, np.maximum(np.abs(got) - 0.45, 0.0), np.maximum(0.55 - np.abs(got), 0.0))
    over[..., 0] = 0.0
    return (over * over).sum(-1)


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """The image and the oracle's (zig-zag blocks, DC differences, lengths, values)
    per channel, computed once and left unchanged."""
    rgb = _img(kind, H, W)
    y, cr, cb = orcc.rgb_to_ycrcb(rgb)
    exp = {}
    for k, (p, t) in {"lum": (y, 0), "cr": (orcc.pyr_down(cr), 1), "cb": (orcc.pyr_down(cb), 1)}.items():
        zz = orcc.zigzag_blocks(orcc.dct_channel(p, t), 8)
        Ln, V = orcc.rle_encode(zz[:, 1:].reshape(-1), 15)
        exp[k] = (zz, orcc.dpcm(zz[:, 0].copy()), Ln, V)
    for v in exp.values():
        for a in v:
            a.setflags(write=False)
    rgb.setflags(write=False)
    return rgb, exp


def _first_last(ac):
    """first / last nonzero AC index of each block (rows of 63), -1 if none"""
    nz = ac != 0
    first = np.where(nz.any(1), nz.argmax(1), -1)
    last = np.where(nz.any(1), 62 - nz[:, ::-1].argmax(1), -1)
    return first, last


def _max_inner_run(ac_row):
    nz = np.flatnonzero(ac_row)
    return int(np.diff(nz).max()) - 1 if nz.size > 1 else 0


def _is_comb(ac_row, ph, n):
    """nonzero exactly at AC ph, ph + 2, ... below n, zero at the others below n"""
    want = (np.arange(n) % 2) == ph
    return np.array_equal(ac_row[:n] != 0, want)


def _check_data(kind, H, W, exp):
    """The oracle's blocks have the property the kind is named after."""
    nbx = W // 8
    ac = exp["lum"][0][:, 1:]
    first, last = _first_last(ac)
    rec = ac.reshape(-1, 64, 63)  # luminance records: 64 consecutive blocks
    rfirst, rlast = first.reshape(-1, 64), last.reshape(-1, 64)
    assert rec.shape[0] == (H // 8) * (nbx // 64)
    if kind == "late":
        assert (first[first >= 0] >= 40).all()
        neg = carried = 0
        for r in range(rec.shape[0]):
            assert rfirst[r, 0] >= 40, r  # the head lane: rem = 0, counter -first
            prev = rlast[r, 0]
            for lane in range(1, 64):
                if rfirst[r, lane] < 0:
                    continue
                run0 = lane * 63 + rfirst[r, lane] - prev - 1
                nf0, rem = divmod(run0, 15)
                neg += rem - rfirst[r, lane] < 0
                carried += nf0 > 0 and rem > 0 and rfirst[r, lane - 1] < 0
                prev = lane * 63 + rlast[r, lane]
            assert neg > 0 and carried > 0, r
    if kind == "edge":
        only0 = (ac[:, 0] != 0) & ~(ac[:, 1:] != 0).any(1)
        assert (ac[:, 62] != 0).any() and only0.any()
        assert ((ac[:, 62] != 0) & (ac[:, 0] != 0)).any()
        for r in range(rec.shape[0]):
            assert rfirst[r, 0] < 0 and rfirst[r, 63] < 0 and (rfirst[r, 1:63] >= 0).any(), r
    if kind == "run14":
        inner = np.array([_max_inner_run(b) for b in ac])
        assert (inner == 14).any() and (inner == 15).any() and inner.max() == 15
        for r in range(rec.shape[0]):
            i = inner[64 * r:64 * r + 64]
            assert (i == 14).any() and (i == 15).any(), r
        # in every block whose inner run is 14: the oracle's symbol that ends on the
        # nonzero after that run is (14, its value) -- a filler would be (14, 0) -- and
        # no symbol in between ends inside the run (no filler in that block)
        Ln, V = exp["lum"][2].astype(np.int64), exp["lum"][3]
        end = np.cumsum(Ln + 1) - 1  # the AC stream position each symbol ends on
        for b in np.flatnonzero(inner == 14):
            nz = np.flatnonzero(ac[b])
            g = int(np.argmax(np.diff(nz)))  # the run lies between nz[g] and nz[g + 1]
            p0, p1 = b * 63 + int(nz[g]), b * 63 + int(nz[g + 1])
            assert p1 - p0 == 15
            i = int(np.searchsorted(end, p1))
            assert end[i] == p1 and Ln[i] == 14 and V[i] == ac[b, nz[g + 1]] != 0, b
            assert end[i - 1] == p0, b
    if kind == "comb":
        for ph in (0, 1):
            assert any(_is_comb(b, ph, 63) for b in ac), ph
        for r in range(rec.shape[0]):
            assert any(_is_comb(b, 0, 63) or _is_comb(b, 1, 63) for b in rec[r]), r
        for k in ("cr", "cb"):
            cac = exp[k][0][:, 1:]
            for ph in (0, 1):
                assert any(_is_comb(b, ph, 63) for b in cac), (k, ph)
            for r in range(len(cac) // 32):  # every 32-block chroma record
                assert any(_is_comb(b, 0, 63) or _is_comb(b, 1, 63)
                           for b in cac[32 * r:32 * r + 32]), (k, r)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_emit_data_has_its_property(kind, H, W):
    """No GPU: the generators against the oracle."""
    _check_data(kind, H, W, _case(kind, H, W)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_slot_emission_equals_oracle(kind, H, W):
    rgb, exp = _case(kind, H, W)
    _check_data(kind, H, W, exp)
    x = device.to_device(rgb.copy())
    for band in (1, 0):  # the stacked units of a band (default) and one unit per wave
        with _lib.knobs(encode_band=band):
            enc = pipeline.Encoder(H, W)
            assert enc.slots and enc.fused
            enc.encode(x)
            got = enc.result()
        for k in pipeline.CHANNELS:
            for j, what in enumerate(("coef", "dc", "sym_len", "sym_val")):
                np.testing.assert_array_equal(np.asarray(got[k][j]).astype(np.int64), exp[k][j],
                                              err_msg="%s %s band %d" % (k, what, band))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["late", "run14"])
def test_slot_fill_emission_equals_oracle(kind):
    """The same slot_pass in the fill kernel (wire.hip): two shards' ShardEncoders on
    this device, rank 0's own blocks and rank 1's wire segment filled into rank 0's
    landing zone."""
    from test_gpu_slots_fill import _gather
    H, W = 64, 1024
    rgb, exp = _case(kind, H, W)
    _check_data(kind, H, W, exp)
    recv, senders = _gather(H, W, 2, 0, rgb.copy())
    assert all(int(se.wire_flag.item()) == 0 for se in senders)
    got = recv.whole.result()
    for k in pipeline.CHANNELS:
        for j, what in enumerate(("coef", "dc", "sym_len", "sym_val")):
            np.testing.assert_array_equal(np.asarray(got[k][j]).astype(np.int64), exp[k][j],
                                          err_msg="%s %s" % (k, what))
