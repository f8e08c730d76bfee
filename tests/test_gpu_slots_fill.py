"""The slot fill (hic_slots_fill_batch, hiccup_amd/csrc/wire.hip) and the gather
kind built on it (sharding.ShardEncoder, gather_kind "slots"): blocks that are
already quantized -- int16 zig-zag blocks, or a shard in the wire format -- go
straight into the slot layout, and after the close the landing zone equals, bit
for bit, what the fused slot encoder (hic_encode420_slots_u8) leaves for the same
image: counts, DC differences, record index, every record's symbols, the
materialized stream and blocks, and the .hic bytes coded from the slots.  The
sharded cases run every rank's ShardEncoder on the one device (the stream kinds
need no process group) and are also pinned to the C oracle.  Reference:
codec.run_length_coding / differential_coding (codec.py:47-99,286-301)."""
import functools

import numpy as np
import pytest
import torch

from hiccup_amd import _lib, device, pipeline, sharding
from test_gpu_slots import _img

pytestmark = pytest.mark.gpu

CH = pipeline.CHANNELS
BPR = {"lum": 64, "cr": 32, "cb": 32}  # blocks per record
CAP = {k: 63 * BPR[k] for k in CH}     # slot capacity (symbols)


def _landing(H, W):
    return pipeline.Encoder(H, W, landing_rpt=pipeline.SLOT_RPT, slots=True)


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """(chain, ref) of one image, computed once and left unchanged: the coefficient
    chain's encoder (its int16 blocks feed the fill) and the fused slot encoder's
    outputs the fill has to reproduce."""
    rgb = device.to_device(_img(kind, H, W, H + W))
    chain = pipeline.Encoder(H, W, slots=False)
    chain.encode(rgb)
    enc = pipeline.Encoder(H, W)
    assert enc.slots and not chain.slots
    enc.encode(rgb)
    torch.cuda.synchronize()
    ref = _snapshot(enc)
    return chain, ref


def _snapshot(enc):
    """Everything the comparisons read from a closed slot encoder, as host data."""
    out = {"bytes": enc.hic_image(from_slots=True).byte_stream()}
    torch.cuda.synchronize()
    out["counts"] = enc.counts.cpu().tolist()
    out["dc"] = {k: enc.dc[k].cpu().numpy() for k in CH}
    out["sidx"] = {k: enc.sidx[k].cpu().numpy().reshape(-1, 4) for k in CH}
    out["slot_len"] = {k: enc.slot_len[k].cpu().numpy().reshape(-1, CAP[k]) for k in CH}
    out["slot_val"] = {k: enc.slot_val[k].cpu().numpy().reshape(-1, CAP[k]) for k in CH}
    out["result"] = enc.result()
    return out


def _assert_equal(got, ref, msg):
    assert got["counts"] == ref["counts"], msg
    for k in CH:
        np.testing.assert_array_equal(got["dc"][k], ref["dc"][k], err_msg="%s %s dc" % (msg, k))
        np.testing.assert_array_equal(got["sidx"][k], ref["sidx"][k], err_msg="%s %s sidx" % (msg, k))
        # each record's first n_r symbols (the rest of a slot is unspecified)
        n = ref["sidx"][k][:, 0]
        assert n.min() >= 0 and n.max() <= CAP[k]
        used = np.arange(CAP[k])[None, :] < n[:, None]
        for what in ("slot_len", "slot_val"):
            np.testing.assert_array_equal(np.where(used, got[what][k], 0), np.where(used, ref[what][k], 0),
                                          err_msg="%s %s %s" % (msg, k, what))
        for j, what in enumerate(("coef", "dc_diff", "sym_len", "sym_val")):
            np.testing.assert_array_equal(got["result"][k][j], ref["result"][k][j], err_msg="%s %s %s" % (msg, k, what))
    assert got["bytes"] == ref["bytes"], msg


def _split3(nrec):
    """Three record counts summing to nrec, the middle one odd."""
    a = 1 if nrec < 10 else 5
    b = (nrec - a) // 2
    if b % 2 == 0:
        b += 1
    c = nrec - a - b
    assert a > 0 and b > 0 and c > 0 and b % 2 == 1, nrec
    return a, b, c


def _pack(blocks, k):
    """A device int16 block range in the wire format (its own tiles), flag checked."""
    n = blocks.shape[0]
    wire = device.empty((_lib.load().hic_wire_bytes(n, pipeline.TABLES[k]),), torch.uint8)
    flag = device.zeros((1,), torch.int32)
    _lib.call("hic_wire_pack_i16", device.ptr(blocks), n, pipeline.TABLES[k], device.ptr(wire), device.ptr(flag),
              device.stream_ptr())
    assert int(flag.item()) == 0
    return wire


@pytest.mark.parametrize("kind", ["random", "sparse", "smooth", "wide", "zero", "levels"])
@pytest.mark.parametrize("H,W", [(16, 512), (48, 1024), (272, 1536)])
def test_fill_from_blocks_equals_fused_slot_encoder(kind, H, W):
    """(16, 512) has ONE 32-block record per chroma plane: the absent half of the
    two-record pass.  wide: luminance zig-zag slot 3 outside 12 bits (the direct
    stores); zero: the stream is the single EOB."""
    chain, ref = _case(kind, H, W)
    zone = _landing(H, W)
    assert zone.slots and zone.landing and isinstance(zone.index, pipeline.SlotIndex)
    zone.fill([pipeline.slot_fill_job(k, 0, chain.coef[k].shape[0], blocks=chain.coef[k]) for k in CH])
    zone.entropy()
    _assert_equal(_snapshot(zone), ref, "%s %dx%d" % (kind, H, W))
    if kind == "wide":
        assert np.abs(ref["result"]["lum"][0][:, 3].astype(np.int32)).max() > 2047
    if kind == "zero":
        for k in CH:
            assert ref["result"][k][2].tolist() == [0] and ref["result"][k][3].tolist() == [0], k


@pytest.mark.parametrize("kind", ["random", "wide"])
@pytest.mark.parametrize("H,W", [(48, 1024), (272, 1536)])
def test_fill_from_wire_equals_fused_slot_encoder(kind, H, W):
    """Each channel as one wire segment, then as three (split at record boundaries,
    an odd number of chroma records in the middle one: its last tile holds a single
    32-block record) passed in shuffled order."""
    chain, ref = _case(kind, H, W)
    if kind == "wide":
        assert np.abs(ref["result"]["lum"][0][:, 3].astype(np.int32)).max() > 2047
    one, three, keep = [], [], []
    for k in CH:
        blocks = chain.coef[k]
        w = _pack(blocks, k)
        keep.append(w)
        one.append(pipeline.slot_fill_job(k, 0, blocks.shape[0], wire=w))
        b0 = 0
        for nrec in _split3(blocks.shape[0] // BPR[k]):
            n = nrec * BPR[k]
            w = _pack(blocks[b0:b0 + n], k)
            keep.append(w)
            three.append(pipeline.slot_fill_job(k, b0, n, wire=w))
            b0 += n
        assert b0 == blocks.shape[0]
    order = np.random.default_rng(7).permutation(len(three))
    for name, segs in (("one", one), ("three", [three[i] for i in order])):
        zone = _landing(H, W)
        zone.fill(segs)
        zone.entropy()
        _assert_equal(_snapshot(zone), ref, "%s %s %dx%d" % (name, kind, H, W))


def test_fill_stays_inside_its_records():
    """Only the middle of three segments is filled: every byte that belongs to the
    other two segments' records -- slots, DC differences, records, last DCs -- and
    the whole record index still hold the sentinel."""
    H, W = 48, 1024
    chain, ref = _case("random", H, W)
    zone = _landing(H, W)
    lib = _lib.load()
    segs, mid = [], {}
    for k in CH:
        for t in (zone.slot_len[k], zone.slot_val[k], zone.dc[k], zone.sidx[k], zone.ws[k]):
            t.view(torch.uint8).fill_(0x5A)
        nrec = chain.coef[k].shape[0] // BPR[k]
        a, b, _ = _split3(nrec)
        mid[k] = (a, a + b)
        segs.append(pipeline.slot_fill_job(k, a * BPR[k], b * BPR[k], blocks=chain.coef[k][a * BPR[k]:(a + b) * BPR[k]]))
    zone.fill(segs)
    torch.cuda.synchronize()
    for k in CH:
        r0, r1 = mid[k]
        nrec = chain.coef[k].shape[0] // BPR[k]
        outside = np.ones(nrec, bool)
        outside[r0:r1] = False
        sl = zone.slot_len[k].cpu().numpy().reshape(nrec, CAP[k])
        sv = zone.slot_val[k].cpu().numpy().reshape(nrec, CAP[k])
        dc = zone.dc[k].cpu().numpy().reshape(nrec, BPR[k])
        assert (sl[outside] == 0x5A).all() and (sv[outside] == 0x5A5A).all() and (dc[outside] == 0x5A5A5A5A).all(), k
        assert (zone.sidx[k].cpu().numpy() == 0x5A5A5A5A).all(), k
        # the workspace: records (3 int64 each) first, the last DCs (int32 each) in its
        # last (nrec + 1) / 2 + 2 words' first part (hic_rle_slots_workspace_bytes)
        ws = zone.ws[k].cpu().numpy().view(np.uint8)
        nbytes = lib.hic_rle_slots_workspace_bytes(chain.coef[k].shape[0], zone.rpt[k])
        rdc0 = nbytes - 8 * ((nrec + 1) // 2 + 2)
        touched = np.zeros(ws.size, bool)
        touched[24 * r0:24 * r1] = True
        touched[rdc0 + 4 * r0:rdc0 + 4 * r1] = True
        assert (ws[~touched] == 0x5A).all(), k
        # and the middle was written: its records' symbols and DCs are the reference's
        # (values only: the close has rewritten each first length and first DC there)
        n = ref["sidx"][k][:, 0]
        used = (np.arange(CAP[k])[None, :] < n[:, None]) & ~outside[:, None]
        np.testing.assert_array_equal(sv[used], ref["slot_val"][k][used], err_msg=k)
        np.testing.assert_array_equal(dc[r0:r1, 1:], ref["dc"][k].reshape(nrec, BPR[k])[r0:r1, 1:], err_msg=k)
        rdc = ws[rdc0 + 4 * r0:rdc0 + 4 * r1].view(np.int32)
        np.testing.assert_array_equal(rdc, ref["result"][k][0][:, 0].reshape(nrec, BPR[k])[r0:r1, -1], err_msg=k)


# ---- the sharded gather, every rank in this process ----
def _image(H, W, flat_rows=None):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[H // 3: H // 3 + H // 5] = 128   # all-zero AC runs across a shard boundary
    rgb[:, : W // 5] = 40                # a flat band: long carried runs
    if flat_rows:                        # a whole shard without any nonzero AC
        rgb[flat_rows[0]:flat_rows[1]] = 128
    return rgb


@functools.lru_cache(maxsize=None)
def _single(H, W, flat):
    """The single-GPU encode, decode and .hic bytes of _image(H, W, flat), and the C
    oracle's encode, computed once."""
    from test_gpu_codec import _oracle_encode
    rgb = _image(H, W, flat)
    enc = pipeline.Encoder(H, W)
    enc.encode(device.to_device(rgb))
    dec = pipeline.Decoder(H, W)
    out = dec.decode(enc.sym_len, enc.sym_val, enc.counts, enc.dc, index=enc.index)
    dec.check_status()
    return rgb, enc.hic_image().byte_stream(), device.to_host(out), enc.result(), _oracle_encode(rgb)


def _gather(H, W, world, gather_to, rgb, spoil=None):
    """Every rank's ShardEncoder(gather_kind="slots") on this device; returns (the
    receiver, the senders) after the receiver's finish()."""
    ses = [sharding.ShardEncoder(H, W, rank=r, world=world, gather_to=gather_to, gather_kind="slots")
           for r in range(world)]
    for se in ses:
        a, b = se.span
        sharding.encode_group([se], [device.to_device(rgb[a:b])])
    if spoil is not None:
        torch.cuda.synchronize()
        ses[spoil].enc.coef["lum"][0, 5] = 32000  # > any luminance slot width
    recv = ses[gather_to]
    assert recv.whole is not None and recv.whole.slots and recv.wire_send is None and not recv.records
    for se in ses:
        if se.rank == gather_to:
            continue
        assert se.whole is None and se.wire_full is None
        se.pack()
        for k in CH:
            o0, o1 = recv.wranges[k][se.rank]
            recv.wire_full[k][o0:o1].copy_(se.wire_send[k])
    recv.finish()
    torch.cuda.synchronize()
    return recv, [se for se in ses if se.rank != gather_to]


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("H,W,world,flat", [(64, 512, 3, (12, 36)), (256, 1024, 2, None), (256, 1024, 2, (120, 256)),
                                            (1088, 1024, 8, (264, 408))])
def test_sharded_slots_gather(H, W, world, flat, last):
    """flat: rows without any nonzero AC that cover a whole shard (rank 1 of 3, the
    last of 2, rank 2 of 8) and its halo, so carried runs chain through a segment."""
    rgb, hic_bytes, exp_rgb, single, oracle = _single(H, W, flat)
    recv, senders = _gather(H, W, world, world - 1 if last else 0, rgb)
    whole = recv.whole
    assert all(int(se.wire_flag.item()) == 0 for se in senders)
    assert whole.hic_image(from_slots=True).byte_stream() == hic_bytes
    dec = pipeline.Decoder(H, W)
    out = dec.decode(whole.sym_len, whole.sym_val, whole.counts, whole.dc, index=whole.index)
    dec.check_status()
    np.testing.assert_array_equal(device.to_host(out), exp_rgb)
    got = whole.result()
    for k in CH:
        for j, what in enumerate(("coef", "dc_diff", "sym_len", "sym_val")):
            np.testing.assert_array_equal(got[k][j], single[k][j], err_msg="%s %s vs single" % (k, what))
            np.testing.assert_array_equal(got[k][j].astype(np.int64), np.asarray(oracle[k][j]).astype(np.int64),
                                          err_msg="%s %s vs oracle" % (k, what))


def test_sharded_slots_gather_overflow():
    """A sender's coefficient outside its wire width: its flag rides in the trailer and
    turns that channel's count on the receiver into COUNT_WIRE_OVERFLOW."""
    H, W = 256, 1024
    recv, senders = _gather(H, W, 2, 0, _image(H, W), spoil=1)
    c = recv.whole.counts.cpu().tolist()
    assert c[0] == pipeline.COUNT_WIRE_OVERFLOW and c[1] >= 0 and c[2] >= 0, c
    assert int(senders[0].wire_flag.item()) == 1


def test_slots_gather_refusals():
    """No silent fallback: a shape the kind cannot take raises, naming the condition."""
    with pytest.raises(ValueError, match="512"):
        sharding.ShardEncoder(64, 768, rank=0, world=2, gather_to=0, gather_kind="slots")
    with pytest.raises(ValueError, match="512"):
        sharding.ShardEncoder(250, 330, rank=0, world=2, gather_to=0, gather_kind="slots")
    with pytest.raises(ValueError, match="16"):
        sharding.ShardEncoder(72, 512, rank=0, world=2, gather_to=0, gather_kind="slots")
    with pytest.raises(ValueError, match="fused"):
        sharding.ShardEncoder(64, 512, rank=0, world=2, gather_to=0, gather_kind="slots", fused=False)
    with pytest.raises(ValueError, match="gather_to"):
        sharding.ShardEncoder(64, 512, rank=0, world=2, gather_kind="slots")
