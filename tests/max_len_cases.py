"""Inputs with known run-length properties and their expected streams at any
max_len, for the tests of the encoder's generic-max_len kernels
(tests/test_gpu_max_len.py; tests/test_cpu_max_len_data.py proves the properties
on the CPU oracle alone).  Test infrastructure: every image is deterministic, and
every expected value comes from the C oracle (oracle/hiccup_oracle.c)."""
import functools

import numpy as np

import oracle.oracle as orc
import oracle.oracle_c as orcc

CHANNELS = ("lum", "cr", "cb")
KINDS = ("noise_band", "speckle", "late", "basis")
# the caps under test: 1 (a filler equals the EOB), 2, both sides of the specialised 15,
# 32, both sides of summarize_ac's M <= 63 cut, and the largest (length 255 in a uint8)
M_VALUES = (1, 2, 14, 16, 32, 63, 64, 256)
M_RLE = M_VALUES + (255,)  # the RLE-level tests also take 255
STAGE = 4096  # emit_tile16 stages a tile in LDS while its symbols fit (kWSyms, rle.hip)

# the shapes each path of test_gpu_max_len.py runs, with the kinds whose CPU property
# matters there (test_cpu_max_len_data.py checks every pair listed here)
ALIGNED = ((16, 512), (48, 1024))
RAGGED = ((32, 528), (16, 1040), (48, 16))
CHAIN = ((250, 330), (37, 53))
KINDS_AT = {
    (16, 512): ("noise_band", "speckle"),
    (48, 1024): KINDS,
    (32, 528): ("noise_band", "speckle", "late"),
    (16, 1040): ("noise_band", "speckle"),
    (48, 16): ("noise_band", "late"),
    (250, 330): ("noise_band", "speckle"),
    (37, 53): ("noise_band", "late"),
}
LARGEST_ALIGNED = (48, 1024)
# row shards: (H, W, world, flat rows or None) of image("shards", ...); shard r = rows
# sharding.plan(H, world)[r].  (64, 512): the fused kernel's records; the third shard of
# four is flat by itself, flat=(16, 32) makes the second flat as well
SHARDS = ((96, 64, 2, None), (144, 96, 3, (48, 96)), (64, 512, 4, None), (64, 512, 4, (16, 32)))
# the batched shard transform: image j of N (H = 16 N rows, 16 per shard, W = 512)
BATCH_KINDS = ("noise_band", "speckle", "late")


def batch_image_key(N, j):
    """(kind, H, W, seed) of image j of a batch of N, as image() / oracle_encode() take it."""
    return BATCH_KINDS[j % len(BATCH_KINDS)], 16 * N, 512, 7 + j


def band_rows(H):
    """noise_band's flat rows [r0, r1).  Whole 16-row units, so that whole chroma block
    rows are flat too, with noise below them (the dense tile follows the run) and,
    from three units on, above them.  An image of one unit: its upper luminance block
    row (image() adds a flat strip of whole chroma blocks at the left)."""
    nu = H // 16
    if nu < 2:
        return 0, 8
    if nu == 2:
        return 0, 16
    return 16, 16 * (1 + max(1, nu // 3))


def image(kind, H, W, seed=7, flat=None):
    """The H x W x 3 uint8 image of one kind.  flat (kind "shards" only): rows [a, b)
    set to 128 as well."""
    rng = np.random.default_rng(seed)
    if kind == "shards":  # test_shards_stitch_to_single_stream's: zero runs that cross shard borders
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[H // 3:H // 3 + 40] = 128
        if flat:
            img[flat[0]:flat[1]] = 128
        return img
    if kind == "noise_band":  # cross-block runs, and dense tiles right after a carried run
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        r0, r1 = band_rows(H)
        img[r0:r1] = 128
        if H // 16 < 2:
            img[:, :max(16, W // 4 // 16 * 16)] = 128
        return img
    if kind == "speckle":  # long cross-block runs in all three channels
        img = np.full((H, W, 3), 128, np.uint8)
        m = rng.random((H, W)) < 0.004
        img[m] = rng.integers(0, 256, (int(m.sum()), 3), dtype=np.uint8)
        return img
    if kind == "late":  # one carried run over most of each channel
        img = np.full((H, W, 3), 128, np.uint8)
        img[max(0, H - 16):] = rng.integers(0, 256, (H - max(0, H - 16), W, 3), dtype=np.uint8)
        return img
    if kind == "basis":
        # grey; about half of the 8 x 8 blocks = 128 + a low DCT basis function + the
        # (7, 7) one: two nonzeros with an in-block zero run of up to 60 between them
        x = (2 * np.arange(8) + 1) * np.pi / 16
        hb, wb = -(-H // 8), -(-W // 8)
        plane = np.full((hb * 8, wb * 8), 128.0)
        low = [(u, v) for u in range(4) for v in range(4) if 0 < u + v <= 3]
        for bi in range(hb):
            for bj in range(wb):
                if rng.random() < 0.5:
                    u, v = low[rng.integers(len(low))]
                    blk = 40 * np.outer(np.cos(u * x), np.cos(v * x)) + 40 * np.outer(np.cos(7 * x), np.cos(7 * x))
                    plane[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8] += blk
        return np.round(plane[:H, :W]).astype(np.uint8)[:, :, None].repeat(3, 2)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def oracle_blocks(kind, H, W, seed=7, flat=None):
    """{channel: (zig-zag blocks (n, 64) int32, DC differences)} of image(kind, H, W, ...):
    the oracle's colour, pyr_down, dct_channel, zigzag_blocks and dpcm.  Cached and
    read-only."""
    y, cr, cb = orcc.rgb_to_ycrcb(image(kind, H, W, seed, flat))
    out = {}
    for k, (p, t) in {"lum": (y, 0), "cr": (orcc.pyr_down(cr), 1), "cb": (orcc.pyr_down(cb), 1)}.items():
        zz = orcc.zigzag_blocks(orcc.dct_channel(p, t), 8)
        dc = orcc.dpcm(zz[:, 0].copy())
        zz.setflags(write=False)
        dc.setflags(write=False)
        out[k] = (zz, dc)
    return out


@functools.lru_cache(maxsize=None)
def oracle_encode(kind, H, W, max_len, seed=7, flat=None):
    """{channel: (zig-zag blocks, DC differences, sym_len, sym_val)}: the expected
    output of an encoder of the whole image at this max_len (test_gpu_codec's
    _oracle_encode with the cap as a parameter)."""
    out = {}
    for k, (zz, dc) in oracle_blocks(kind, H, W, seed, flat).items():
        L, V = orcc.rle_encode(zz[:, 1:].reshape(-1), max_len)
        L.setflags(write=False)
        V.setflags(write=False)
        out[k] = (zz, dc, L, V)
    return out


@functools.lru_cache(maxsize=None)
def oracle_decode(kind, H, W, seed=7, flat=None):
    """The oracle's inverse chain of the oracle's blocks: dequantize + IDCT, pyrUp of
    the chroma, YCrCb -> RGB (what any decode of any max_len's stream must give)."""
    rec = {}
    for k, (zz, _) in oracle_blocks(kind, H, W, seed, flat).items():
        h, w = (H, W) if k == "lum" else (H // 2, W // 2)
        raster = orc.merge_blocks(zz[:, np.argsort(orc.ZZ8)].reshape(-1, 8, 8), (h, w))
        rec[k] = orcc.inv_dct_channel(raster, 0 if k == "lum" else 1)
    h, w = H // 2, W // 2
    out = orcc.ycrcb_to_rgb(rec["lum"][:2 * h, :2 * w], orcc.pyr_up(rec["cr"]), orcc.pyr_up(rec["cb"]))
    out.setflags(write=False)
    return out


def run_counts(zz, max_len):
    """From zig-zag blocks alone: (zero runs >= max_len that lie inside one block,
    zero runs >= max_len that cross a block border, 64-block tiles whose symbols
    exceed STAGE).  A run is the zeros between two nonzeros of the channel's AC
    stream (or from the stream's start); the trailing run is the EOB and counts
    nowhere.  A tile's symbols: one per nonzero plus run // max_len fillers each."""
    ac = np.asarray(zz)[:, 1:].reshape(-1)
    p = np.flatnonzero(ac)
    q = np.concatenate(([-1], p[:-1]))
    run = p - q - 1
    inside = q + 1 >= (p // 63) * 63  # the run starts in the block of the nonzero that ends it
    long = run >= max_len
    syms = np.bincount(p // (63 * 64), weights=1 + run // max_len, minlength=1)
    return int((long & inside).sum()), int((long & ~inside).sum()), int((syms > STAGE).sum())


def counts(kind, H, W, max_len):
    """{channel: run_counts} of image(kind, H, W)."""
    return {k: run_counts(zz, max_len) for k, (zz, _) in oracle_blocks(kind, H, W).items()}


def carried_run(zz, block0):
    """The zero run of the channel's AC stream that crosses into block `block0`: (zeros
    of it before the block, its whole length); (0, 0) if the block before ends in a
    nonzero or no nonzero follows."""
    ac = np.asarray(zz)[:, 1:].reshape(-1)
    cut = block0 * 63
    before, after = np.flatnonzero(ac[:cut]), np.flatnonzero(ac[cut:])
    if after.size == 0:
        return 0, 0
    q = int(before[-1]) if before.size else -1
    return cut - q - 1, cut + int(after[0]) - q - 1


# ---- int16 blocks set directly (the RLE-level tests) ---------------------------------
CRAFTED_NBLK = 64 * 5 + 17


def gap_positions(max_len):
    """AC indices k for a block holding AC 0 and AC k: in-block runs k - 1 of max_len - 2
    .. max_len + 1, 2 max_len - 1, 2 max_len (where a divide can be off by one) and 61."""
    M = max_len
    return sorted({k for k in (M - 1, M, M + 1, M + 2, 2 * M, 2 * M + 1, 62) if 1 <= k <= 62})


def residue_sequences(max_len, budget):
    """[(r, j)]: r empty blocks, then a block whose only nonzero is AC j, after a block
    that ends in a nonzero AC 62: a carried run of 63 r + j >= max_len whose remainder
    mod max_len is 0 and max_len - 1.  Per remainder the shortest such run with any j,
    and the shortest with j = 62 where one exists within `budget` blocks."""
    M, out = max_len, []
    for target in sorted({0, M - 1}):
        anyj = next(((r, j) for r in range(budget) for j in range(63)
                     if 63 * r + j >= M and (63 * r + j) % M == target), None)
        j62 = next(((r, 62) for r in range(budget) if 63 * r + 62 >= M and (63 * r + 62) % M == target), None)
        out += [s for s in (anyj, j62) if s is not None]
    return list(dict.fromkeys(out))


def crafted_blocks(max_len, variant):
    """(CRAFTED_NBLK, 64) int16 zig-zag blocks, by 64-block tile:
    variant 0: 32 gap blocks + 32 empty | 64 empty | 64 empty | 63 dense blocks + a gap
               block (after 160 empty blocks the tile passes the emit's LDS stage at
               every max_len <= 64, with an in-block run in it) | 62 gap blocks + 2
               empty | 17 dense blocks;
    variant 1: 58 gap blocks + 6 empty | 64 empty | a dense tile (after 70 empty blocks) |
               61 gap blocks + 3 empty | a dense tile | 17 gap blocks, the last one ending
               in a nonzero AC 62 (the stream has no EOB);
    variant 2: residue sequences (the longest first), then empty blocks (a long EOB).
    Gap blocks: AC 0 and AC k, k cycling over gap_positions; every third one AC 62 too.
    Returns (blocks, [carried run of each residue sequence placed])."""
    M = max_len
    rng = np.random.default_rng(1000 * M + variant)
    n = CRAFTED_NBLK
    b = np.zeros((n, 64), np.int16)

    def val(size=None):
        return (rng.integers(1, 41, size) * rng.choice((-1, 1), size)).astype(np.int16)

    def gaps(lo, hi):
        ks = gap_positions(M)
        for i in range(lo, hi):
            b[i, 1] = val()
            b[i, 1 + ks[(i - lo) % len(ks)]] = val()
            if (i - lo) % 3 == 2:
                b[i, 63] = val()

    def dense(lo, hi):
        b[lo:hi, 1:] = val((hi - lo, 63))

    def residues(lo, hi, seqs):
        runs, i = [], lo
        for r, j in seqs:
            if i + r + 2 > hi:
                continue
            b[i, 63] = val()      # the run starts after this AC 62
            b[i + 1 + r, 1 + j] = val()
            runs.append(63 * r + j)
            i += 1 + r            # the block that ends the run starts the next sequence
            if j != 62:
                i += 1
        return runs

    runs = []
    if variant == 0:
        gaps(0, 32)
        dense(192, 255)
        b[255, 1], b[255, 63] = val(), val()  # a run of 61 inside the block
        gaps(256, 318)
        dense(320, n)
    elif variant == 1:
        gaps(0, 58)
        dense(128, 192)
        gaps(192, 253)
        dense(256, 320)
        gaps(320, n)
        b[n - 1, 63] = val()
    else:
        seqs = sorted(residue_sequences(M, 300), reverse=True)
        runs = residues(0, n - 20, seqs)
    b[:, 0] = rng.integers(-900, 901, n)
    return b, runs


def tile_segments(nblk, rpt):
    """Block ranges of the records of a tiles job: one per 64 / rpt blocks."""
    seg = 64 // rpt
    return [(s, min(s + seg, nblk)) for s in range(0, nblk, seg)]


def row_segments(nblk, rowb, rpt):
    """Block ranges of the records of a rows job: each row of rowb blocks cut into 64 /
    rpt blocks from its start, the last one shorter."""
    seg = 64 // rpt
    return [(r + s, min(r + s + seg, r + rowb)) for r in range(0, nblk, rowb) for s in range(0, rowb, seg)]


def records(blocks, max_len, segments):
    """The RLE records of rle_core.h for block ranges `segments`, (len(segments), 3)
    int64: the stream position of the range's first nonzero AC (-1: none), of its last,
    and the symbols of every nonzero after the first (one each + run // max_len
    fillers)."""
    ac = np.asarray(blocks)[:, 1:].reshape(-1)
    out = np.empty((len(segments), 3), np.int64)
    for i, (b0, b1) in enumerate(segments):
        p = np.flatnonzero(ac[b0 * 63:b1 * 63]) + b0 * 63
        if p.size == 0:
            out[i] = (-1, -1, 0)
        else:
            run = np.diff(p) - 1
            out[i] = (p[0], p[-1], int((1 + run // max_len).sum()))
    return out
