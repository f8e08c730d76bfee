"""The inputs of tests/test_gpu_max_len.py reach what they claim (no GPU): every
property below is read from the C oracle's zig-zag blocks and streams alone, for
the shapes, kinds and max_len values the GPU tests run.  A GPU test that passes on
data that never leaves the easy path proves nothing; this test is that condition."""
import numpy as np
import pytest

import max_len_cases as mc
import oracle.oracle_c as orcc
from hiccup_amd import sharding

SHAPES = tuple(mc.KINDS_AT)


def _uses(kind):
    return [s for s in SHAPES if kind in mc.KINDS_AT[s]]


def test_every_listed_shape_has_its_kinds():
    assert set(mc.ALIGNED + mc.RAGGED + mc.CHAIN) == set(SHAPES)
    assert mc.LARGEST_ALIGNED == max(mc.ALIGNED, key=lambda s: s[0] * s[1])
    for s in SHAPES:
        assert "noise_band" in mc.KINDS_AT[s] and {"speckle", "late"} & set(mc.KINDS_AT[s])
    assert set(mc.KINDS_AT[mc.LARGEST_ALIGNED]) == set(mc.KINDS)


def test_basis_has_in_block_runs():
    """Luminance: an in-block run >= M for every tested M <= 32 (and none can exist
    above 61, the longest run between two nonzeros of one block)."""
    for H, W in _uses("basis"):
        for M in mc.M_VALUES:
            inside, _, _ = mc.counts("basis", H, W, M)["lum"]
            if M <= 32:
                assert inside >= 1, (H, W, M)
            if M >= 63:
                assert inside == 0, (H, W, M)


def test_noise_band_luminance_passes_the_stage():
    """A 64-block luminance tile over the emit's 4096-symbol stage: at 48 x 1024 for
    every M <= 16; at every other shape for M = 1 wherever the image has a dense
    64-block tile after its band (the narrow shapes have no 64 dense blocks at all)."""
    for H, W in _uses("noise_band"):
        for M in mc.M_VALUES:
            big = mc.counts("noise_band", H, W, M)["lum"][2]
            if (H, W) == (48, 1024) and M <= 16:
                assert big >= 1, (H, W, M)
        wide = (W // 8) * (H // 8) >= 128 and W >= 330
        assert (mc.counts("noise_band", H, W, 1)["lum"][2] >= 1) == wide, (H, W)


def test_noise_band_chroma_runs():
    """Each chroma channel: an in-block run >= M at M <= 2, a cross-block run >= M at
    M <= 16."""
    for H, W in _uses("noise_band"):
        for M in mc.M_VALUES:
            c = mc.counts("noise_band", H, W, M)
            for k in ("cr", "cb"):
                if M <= 2:
                    assert c[k][0] >= 1, (H, W, M, k)
                if M <= 16:
                    assert c[k][1] >= 1, (H, W, M, k)


def test_speckle_and_late_cross_block_runs():
    """speckle at the largest aligned shape: a cross-block run >= M in all three
    channels for every tested M (255 included); speckle and late at every shape that
    uses them: in at least one channel."""
    H, W = mc.LARGEST_ALIGNED
    for M in mc.M_RLE:
        c = mc.counts("speckle", H, W, M)
        assert all(c[k][1] >= 1 for k in mc.CHANNELS), (M, c)
    for kind in ("speckle", "late"):
        for H, W in _uses(kind):
            for M in mc.M_VALUES:
                c = mc.counts(kind, H, W, M)
                assert any(c[k][1] >= 1 for k in mc.CHANNELS), (kind, H, W, M)


def test_length_255_appears_at_256():
    """At M = 256 the expected length stream holds 255 (the largest uint8) at every
    shape, in at least one of its kinds' channels."""
    for H, W in SHAPES:
        n = sum(int((mc.oracle_encode(kind, H, W, 256)[k][2] == 255).sum())
                for kind in mc.KINDS_AT[H, W] for k in mc.CHANNELS)
        assert n >= 1, (H, W)
    for v in range(3):
        blocks, _ = mc.crafted_blocks(256, v)
        L, _ = orcc.rle_encode(blocks[:, 1:].reshape(-1).astype(np.int32), 256)
        assert v == 0 or (L == 255).any(), v


@pytest.mark.parametrize("H,W,world,flat", mc.SHARDS)
def test_shard_images_carry_runs_across_borders(H, W, world, flat):
    """A luminance zero run of >= 256 (every tested M) crosses into a shard, so the
    shard's stream opens with run // M fillers; where a shard is flat the run crosses
    two borders; and at M = 1 every shard's expected symbols fit Encoder.cap."""
    zz = mc.oracle_blocks("shards", H, W, 7, flat)["lum"][0]
    rows = sharding.plan(H, world)
    crossing = []
    for r0, _ in rows[1:]:
        before, whole = mc.carried_run(zz, (r0 // 8) * -(-W // 8))
        crossing.append((before, whole))
    assert any(b >= 256 and w >= b for b, w in crossing), crossing
    if flat or (H, W) == (64, 512):
        # a shard without any nonzero luminance AC: the same run crosses both its borders
        nb = -(-W // 8)
        empty = [not zz[(r0 // 8) * nb:(r1 // 8) * nb, 1:].any() for r0, r1 in rows]
        assert any(empty[1:-1]), empty
    for M in mc.M_VALUES:
        ac = zz[:, 1:].reshape(-1)
        L, _ = orcc.rle_encode(ac, M)
        p = np.flatnonzero(ac)
        q = np.concatenate(([-1], p[:-1]))
        syms = 1 + (p - q - 1) // M
        for r0, r1 in rows:
            nb = -(-W // 8)
            lo, hi = (r0 // 8) * nb * 63, (r1 // 8) * nb * 63
            need = int(syms[(p >= lo) & (p < hi)].sum()) + 1
            n = (r1 - r0) // 8 * nb
            lead = (r0 // 8) * nb
            assert need <= n * 63 + 1 + lead * 63 // M, (M, r0)
        assert len(L) >= 1


@pytest.mark.parametrize("N", [2, 8])
def test_batch_images_have_long_runs(N):
    """The batched shard transform's images: a cross-block run >= M in some channel of
    every image, for every tested M below 256 (H = 32 leaves few blocks)."""
    for j in range(N):
        kind, H, W, seed = mc.batch_image_key(N, j)
        blocks = mc.oracle_blocks(kind, H, W, seed)
        for M in mc.M_VALUES:
            if M < 256:
                assert any(mc.run_counts(blocks[k][0], M)[1] >= 1 for k in mc.CHANNELS), (j, kind, M)


@pytest.mark.parametrize("M", mc.M_RLE)
def test_crafted_blocks_reach_every_emit_branch(M):
    """The blocks set directly: in-block runs on both sides of M (M <= 61), carried
    runs whose remainder mod M is 0 and M - 1, a tile that passes the stage with
    in-block and carried fillers in it (M <= 64), staged dense tiles with and without a
    carried run, one stream that ends in a nonzero and one with a long EOB; the host
    records describe the oracle's stream."""
    b = [mc.crafted_blocks(M, v) for v in range(3)]
    assert all(x[0].shape == (mc.CRAFTED_NBLK, 64) and x[0].dtype == np.int16 for x in b)
    if M <= 61:
        ks = mc.gap_positions(M)
        assert {M - 1, M, 62} <= {k - 1 for k in ks} | {62} and 62 in ks
        inside = mc.run_counts(b[0][0], M)[0]
        assert inside >= 1
    runs = b[2][1]
    assert all(r >= M for r in runs)
    assert {0, M - 1} <= {r % M for r in runs}, (M, runs)
    for v, want in ((0, M <= 64), (1, M <= 64)):
        assert (mc.run_counts(b[v][0], M)[2] >= 1) == want, (v, M)
    if M <= 61:
        # variant 0's tile 3 passes the stage and holds a run of 61 inside its last block
        ac = b[0][0][192:256, 1:]
        assert (ac[:63] != 0).all() and np.flatnonzero(ac[63]).tolist() == [0, 62]
    assert b[1][0][-1, 63] != 0 and not b[2][0][-20:, 1:].any()
    # the records on the host: their symbol counts add up to the oracle's stream
    for v in range(3):
        blocks = b[v][0]
        L, _ = orcc.rle_encode(blocks[:, 1:].reshape(-1).astype(np.int32), M)
        for segs in (mc.tile_segments(len(blocks), 1), mc.tile_segments(len(blocks), 2),
                     mc.row_segments(330, 66, 2), mc.row_segments(40, 2, 1)):
            n = segs[-1][1]
            rec = mc.records(blocks[:n], M, segs)
            Ln, _ = orcc.rle_encode(blocks[:n, 1:].reshape(-1).astype(np.int32), M)
            total, prev = 0, -1
            for first, last, cnt in rec:
                if first >= 0:
                    total += 1 + (first - prev - 1) // M + cnt
                    prev = last
            eob = 0 if prev == n * 63 - 1 else 1
            assert total + eob == len(Ln), (v, len(segs))
        assert len(L) <= len(blocks) * 63 + 1
