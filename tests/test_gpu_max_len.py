"""GPU parity at max_len other than 15: every encoder path that books run-length
records has a generic instance beside the one specialised for 15 (k_encode420<0> in
both forms with tile_record16_half<0>, k_encode420_batch<0>, k_dct_planes<...,
ZIGZAG_I16, 0>, k_rle_tile16<0>, k_rle_emit16b<0>), and the decoders must read a
stream whose fillers are (max_len - 1, 0) for any max_len.  Every path runs here at
max_len 1, 2, 14, 16, 32, 63, 64 and 256 (the RLE-level tests at 255 too) on inputs
whose run-length properties tests/test_cpu_max_len_data.py proves on the CPU, and
is compared bit for bit with the C oracle (tests/max_len_cases.py): the zig-zag
blocks, the DC differences, the symbol count, sym_len and sym_val."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import max_len_cases as mc  # noqa: E402
import oracle.oracle_c as orcc  # noqa: E402
from hiccup_amd import _lib, device, pipeline, sharding  # noqa: E402

CH = pipeline.CHANNELS
MS = mc.M_VALUES


def _cases(shapes, kinds=None):
    return [(H, W, k) for H, W in shapes for k in (kinds or mc.KINDS_AT[H, W]) if k in mc.KINDS_AT[H, W]]


def _check(got, exp, what=""):
    """An encoder's result() against the oracle's: blocks, DC differences, symbol count,
    lengths, values."""
    for k in CH:
        zz, dc, L, V = got[k]
        ezz, edc, eL, eV = exp[k]
        np.testing.assert_array_equal(zz.astype(np.int32), ezz, err_msg="%s %s blocks" % (what, k))
        np.testing.assert_array_equal(dc, edc, err_msg="%s %s dc" % (what, k))
        assert len(L) == len(eL), "%s %s: %d symbols, expected %d" % (what, k, len(L), len(eL))
        np.testing.assert_array_equal(L.astype(np.int32), eL, err_msg="%s %s sym_len" % (what, k))
        np.testing.assert_array_equal(V.astype(np.int32), eV, err_msg="%s %s sym_val" % (what, k))


def _encode(H, W, kind, M, **kw):
    enc = pipeline.Encoder(H, W, max_len=M, **kw)
    enc.encode(device.to_device(mc.image(kind, H, W)))
    return enc


def _status(enc):
    return [enc.coef[k].shape[0] * 63 for k in CH]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W,kind", _cases(mc.ALIGNED))
def test_fused_aligned(H, W, kind, M):
    """Encoder(H, W, max_len=M), W % 512 == 0: the coefficient chain (the slot layout is
    max_len 15 only) on the fused kernel in its band form and its one-unit-per-wave
    form, half-tile chroma records, tiles scan and emit with 1 and 2 records per tile."""
    exp = mc.oracle_encode(kind, H, W, M)
    for band in (1, 0):
        with _lib.knobs(encode_band=band):
            enc = _encode(H, W, kind, M)
            assert enc.slots is False and enc.fused and not enc.seg
            assert enc.rpt == {"lum": 1, "cr": 2, "cb": 2}
            _check(enc.result(), exp, "band %d" % band)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("kind", mc.KINDS_AT[mc.LARGEST_ALIGNED])
def test_fused_index_and_indexed_decode(kind, M):
    """index=True: the emit also writes the tile index at a generic max_len; the
    indexed decode of it gives the oracle's inverse chain, 63 positions per block."""
    H, W = mc.LARGEST_ALIGNED
    enc = _encode(H, W, kind, M, index=True)
    assert enc.slots is False and enc.fused and enc.index is not None
    _check(enc.result(), mc.oracle_encode(kind, H, W, M))
    for k in CH:  # the emit's index == the index pass's
        ix = torch.full_like(enc.index[k], -5)
        _lib.call("hic_rle_tile_index_i16", device.ptr(enc.coef[k]), enc.coef[k].shape[0], enc.rpt[k],
                  device.ptr(enc.ws[k]), device.ptr(ix), device.stream_ptr())
        assert torch.equal(ix, enc.index[k]), k
    for kw in ({}, {"keep_blocks": True}, {"planes": True}):
        dec = pipeline.Decoder(H, W)
        rgb = device.to_host(dec.decode(enc.sym_len, enc.sym_val, enc.counts, enc.dc, index=enc.index, **kw))
        assert dec.status.cpu().tolist() == _status(enc), kw
        np.testing.assert_array_equal(rgb, mc.oracle_decode(kind, H, W), err_msg=str(kw))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W,kind", _cases(mc.RAGGED))
def test_fused_ragged_segments(H, W, kind, M):
    """W % 512 != 0: hic_encode420_seg_u8's records per strip segment and the
    row-segment scan and emit (hic_rle_encode_i16_rows_batch)."""
    enc = _encode(H, W, kind, M)
    assert enc.seg and enc.fused
    _check(enc.result(), mc.oracle_encode(kind, H, W, M))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W,kind", _cases(mc.CHAIN) + _cases([mc.LARGEST_ALIGNED], ("noise_band", "speckle", "basis")))
def test_two_kernel_chain(H, W, kind, M):
    """The colour kernel + the plane DCT with its fused record epilogue on the fast
    planes, the tile pass on the ragged ones."""
    enc = _encode(H, W, kind, M, fused=False)
    assert not enc.fused and not enc.slots and enc.y is not None
    _check(enc.result(), mc.oracle_encode(kind, H, W, M))


def _plane(kind, H, W):
    """test_gpu_transform's _structured_plane, the two kinds used here."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    if kind == "random":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    return (128 + rng.integers(-4, 5, (H, W))).astype(np.uint8)  # nearflat


@pytest.mark.parametrize("M", mc.M_RLE)
@pytest.mark.parametrize("kind", ["random", "nearflat"])
@pytest.mark.parametrize("H,W", [(8, 16), (8 * 33, 8 * 130)])
def test_plane_dct_rle_records(kind, H, W, M):
    """test_gpu_transform's test of the same name with M in place of 15: the plane
    entry point alone (hic_dct_quant_rle_u8, a partial last set included) + the tiles
    scan and emit, both tables, both DCT paths."""
    plane = _plane(kind, H, W)
    d = device.to_device(plane)
    nblk = (H // 8) * (W // 8)
    lib = _lib.load()
    for tab in (0, 1):
        exp = orcc.zigzag_blocks(orcc.dct_channel(plane, tab), 8)
        eL, eV = orcc.rle_encode(exp[:, 1:].reshape(-1), M)
        for path in (_lib.DCT_PATH_F64, _lib.DCT_PATH_EXACT):
            out = device.empty((nblk, 64), torch.int16)
            ws = device.workspace(lib.hic_rle_workspace_bytes(nblk, 64))
            with _lib.knobs(dct_path=path):
                _lib.call("hic_dct_quant_rle_u8", device.ptr(d), H, W, W, tab, M, device.ptr(out), device.ptr(ws),
                          device.stream_ptr(), None, None)
            cap = nblk * 63 + 1
            L, V = device.empty((cap,), torch.uint8), device.empty((cap,), torch.int16)
            dc, cnt = device.empty((nblk,), torch.int32), device.zeros((1,), torch.int64)
            job = (_lib.RleJob16 * 1)()
            job[0] = _lib.RleJob16(out.data_ptr(), nblk, None, dc.data_ptr(), L.data_ptr(), V.data_ptr(), cap,
                                   cnt.data_ptr(), ws.data_ptr(), 1)
            _lib.call("hic_rle_encode_i16_tiles_batch", 1, job, M, device.stream_ptr())
            np.testing.assert_array_equal(device.to_host(out).astype(np.int32), exp, err_msg=str((tab, path)))
            c = int(cnt.cpu().item())
            assert c == len(eL), (tab, path, c, len(eL))
            np.testing.assert_array_equal(device.to_host(L[:c]).astype(np.int32), eL, err_msg=str((tab, path)))
            np.testing.assert_array_equal(device.to_host(V[:c]).astype(np.int32), eV, err_msg=str((tab, path)))
            np.testing.assert_array_equal(device.to_host(dc), orcc.dpcm(exp[:, 0].copy()), err_msg=str((tab, path)))


def _stitch_and_close(encs):
    """hic_rle_stitch of every shard from all shards' summaries (== the host
    restatement), then each shard's entropy; returns the stitch records."""
    world = len(encs)
    summ = np.stack([e.shard_summaries().cpu().numpy() for e in encs])  # (world, 3, 4)
    allsum = device.to_device(summ)
    stitches = []
    for r, e in enumerate(encs):
        st = device.zeros((3, 4), torch.int64)
        for c in range(3):
            _lib.call("hic_rle_stitch", ctypes.c_void_p(allsum.data_ptr() + 32 * c), world, r, 12, device.ptr(st[c]),
                      device.stream_ptr())
            np.testing.assert_array_equal(st[c].cpu().numpy(), sharding.stitch_host(summ[:, c], r))
        e.entropy(stitch=st)
        stitches.append(st)
    return stitches


def _check_parts(parts, exp, what=""):
    """The shards' results, concatenated, against a whole stream."""
    got = {k: tuple(np.concatenate([p[k][j] for p in parts]) for j in range(4)) for k in CH}
    _check(got, exp, what)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W,world,flat", mc.SHARDS)
def test_shards_stitch_to_single_stream(H, W, world, flat, M):
    """test_gpu_codec's test of the same name with max_len=M on the whole encoder and
    on every shard: a carried run becomes run // M fillers at a shard's head (within
    Encoder.cap's lead term), the concatenated shard streams equal the whole stream
    and the oracle's, each shard's decode equals its rows of the whole decode."""
    rgb = mc.image("shards", H, W, 7, flat)
    exp = mc.oracle_encode("shards", H, W, M, 7, flat)
    whole = pipeline.Encoder(H, W, max_len=M)
    assert not whole.slots
    whole.encode(device.to_device(rgb))
    ref = whole.result()
    _check(ref, exp, "whole")
    encs = []
    for rows in sharding.plan(H, world):
        e = pipeline.Encoder(H, W, rows=rows, max_len=M)
        a, b = e.input_span()
        e.transform(device.to_device(rgb[a:b]))
        encs.append(e)
    stitches = _stitch_and_close(encs)
    for r, e in enumerate(encs):
        counts = e.counts.cpu().tolist()
        assert all(0 <= c <= e.cap[k] for c, k in zip(counts, CH)), (r, counts, e.cap)
    parts = [e.result() for e in encs]
    _check_parts(parts, ref, "shards vs whole")
    _check_parts(parts, exp, "shards vs oracle")
    whole_dec = pipeline.Decoder(H, W)
    full = device.to_host(whole_dec.decode(whole.sym_len, whole.sym_val, whole.counts.cpu().tolist(), whole.dc))
    np.testing.assert_array_equal(full, mc.oracle_decode("shards", H, W, 7, flat))
    decs = [sharding.ShardDecoder(H, W, rank=r, world=world) for r in range(world)]
    for d, e, st in zip(decs, encs, stitches):
        d.planes(e.sym_len, e.sym_val, e.counts.cpu().tolist(), e.dc, st)
    for r, d in enumerate(decs):  # the halo rows, copied between the shards' buffers
        for i, (buf, top, n) in enumerate(d.halo_views()):
            if r > 0:
                pb, pt, pn = decs[r - 1].halo_views()[i]
                buf[0].copy_(pb[pt + pn - 1])
            if r < world - 1:
                nb, nt, _ = decs[r + 1].halo_views()[i]
                buf[top + n].copy_(nb[nt])
    for r, d in enumerate(decs):
        got = device.to_host(d.colour())
        d.check_status()
        a, b = d.out_rows
        np.testing.assert_array_equal(got, full[a:b], err_msg="rank %d" % r)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", [2, 8])
def test_transform_batch(N, M):
    """pipeline.transform_batch (hic_encode420_batch_u8, the generic batched kernel) of
    N shard encoders at max_len=M, one image each: shard r of every image in one
    launch, for every r.  Coefficients and records equal the one-launch-per-shard
    encoders'; each image's stitched stream equals the oracle's.  (Before the entry
    point took what hic_encode420_u8 takes, this raised "max_len 15 or 0".)"""
    keys = [mc.batch_image_key(N, j) for j in range(N)]
    H, W = keys[0][1], keys[0][2]
    imgs = [device.to_device(mc.image(kind, H, W, seed)) for kind, _, _, seed in keys]
    rows = sharding.plan(H, N)
    assert all(r1 - r0 == 16 for r0, r1 in rows)
    grid = [[None] * N for _ in range(N)]  # [image][shard]
    for r in range(N):
        one = [pipeline.Encoder(H, W, rows=rows[r], max_len=M) for _ in range(N)]
        bat = [pipeline.Encoder(H, W, rows=rows[r], max_len=M) for _ in range(N)]
        assert all(e.batchable() for e in bat)
        a, b = one[0].input_span()
        ins = [img[a:b] for img in imgs]
        for e, x in zip(one, ins):
            e.transform(x, in_row0=a)
        pipeline.transform_batch(bat, ins, in_row0s=[a] * N)
        torch.cuda.synchronize()
        for j, (e1, e2) in enumerate(zip(one, bat)):
            for k in CH:
                assert torch.equal(e1.coef[k], e2.coef[k]), (r, j, k)
                assert torch.equal(e1.ws[k], e2.ws[k]), (r, j, k)
            grid[j][r] = e2
    for j, (kind, _, _, seed) in enumerate(keys):
        _stitch_and_close(grid[j])
        for e in grid[j]:
            assert all(0 <= c <= e.cap[k] for c, k in zip(e.counts.cpu().tolist(), CH))
        _check_parts([e.result() for e in grid[j]], mc.oracle_encode(kind, H, W, M, seed), "image %d" % j)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W,kind", _cases([(48, 1024), (32, 528)], ("noise_band", "speckle", "late")))
def test_decode_of_a_foreign_cap(H, W, kind, M):
    """The flat decode (no index) of an M-coded stream gives the oracle's inverse
    chain: a filler is (M - 1, 0) of any length, and at M = 1 it is (0, 0), identical
    to the EOB (only the last symbol is trailing).  The index built from the bare
    stream equals the emit's own, and decoding with it gives the same."""
    enc = _encode(H, W, kind, M, index=True, slots=False)
    _check(enc.result(), mc.oracle_encode(kind, H, W, M))
    counts = enc.counts.cpu().tolist()
    exp = mc.oracle_decode(kind, H, W)
    plain = pipeline.Decoder(H, W)
    rgb = device.to_host(plain.decode(enc.sym_len, enc.sym_val, counts, enc.dc))
    plain.check_status()
    for k in CH:
        assert torch.equal(plain.blocks[k], enc.coef[k]), k
    np.testing.assert_array_equal(rgb, exp)
    with _lib.knobs(rld_generic=1):  # the generic scatter decode
        gen = pipeline.Decoder(H, W)
        np.testing.assert_array_equal(device.to_host(gen.decode(enc.sym_len, enc.sym_val, counts, enc.dc)), exp)
        gen.check_status()
    index, status = pipeline.stream_index(enc.sym_len, enc.sym_val, counts, enc.dc, H, W)
    assert status.cpu().tolist() == _status(enc)
    for k in CH:
        assert torch.equal(index[k], enc.index[k]), (k, index[k].view(-1, 3)[:8], enc.index[k].view(-1, 3)[:8])
    dec = pipeline.Decoder(H, W)
    np.testing.assert_array_equal(device.to_host(dec.decode(enc.sym_len, enc.sym_val, enc.counts, enc.dc, index=index)),
                                  exp)
    dec.check_status()


CANARY = 0x5A


def _rle_job(blocks, M, rec, rpt, ws_bytes):
    """One hic_rle_job16 over host blocks with the records `rec` (host, (nrec, 3)) in a
    zeroed workspace; symbol buffers with a canary tail past sym_cap."""
    n = blocks.shape[0]
    cap = n * 63 + 1
    t = {"blocks": device.to_device(blocks), "ws": device.workspace(ws_bytes),
         "L": torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda"),
         "V": torch.full((cap + 64,), CANARY, dtype=torch.int16, device="cuda"),
         "dc": device.empty((n,), torch.int32), "cnt": device.zeros((1,), torch.int64), "cap": cap}
    assert t["ws"].numel() * 8 >= ws_bytes
    if rec is not None:
        assert ws_bytes >= 40 * len(rec)  # 3 record words + 2 offset words each
        t["ws"][:3 * len(rec)] = device.to_device(np.ascontiguousarray(rec).reshape(-1))
    t["job"] = _lib.RleJob16(t["blocks"].data_ptr(), n, None, t["dc"].data_ptr(), t["L"].data_ptr(), t["V"].data_ptr(),
                             cap, t["cnt"].data_ptr(), t["ws"].data_ptr(), rpt, ws_bytes, None)
    return t


def _check_rle(t, blocks, M, what):
    eL, eV = orcc.rle_encode(blocks[:, 1:].reshape(-1).astype(np.int32), M)
    c = int(t["cnt"].cpu().item())
    assert c == len(eL), (what, c, len(eL))
    L, V = device.to_host(t["L"]), device.to_host(t["V"])
    np.testing.assert_array_equal(L[:c].astype(np.int32), eL, err_msg=what)
    np.testing.assert_array_equal(V[:c].astype(np.int32), eV, err_msg=what)
    np.testing.assert_array_equal(device.to_host(t["dc"]), orcc.dpcm(blocks[:, 0].astype(np.int32)), err_msg=what)
    assert (L[t["cap"]:] == CANARY).all() and (V[t["cap"]:] == CANARY).all(), what


@pytest.mark.parametrize("M", mc.M_RLE)
def test_rle_tiles_crafted_blocks(M):
    """hic_rle_encode_i16_tiles_batch, three jobs (records per tile 1 / 2 / 2) over
    blocks set directly (max_len_cases.crafted_blocks): every branch of the emit --
    staged dense, staged with gaps, direct write with wave-written fillers -- and the
    divides at the remainders 0 and M - 1.  Job 0's records come from the tile pass
    (k_rle_tile16) and equal the host's; the half-tile records are the host's."""
    lib = _lib.load()
    n = mc.CRAFTED_NBLK
    ws_bytes = lib.hic_rle_workspace_bytes(n, 64)
    blocks = [mc.crafted_blocks(M, v)[0] for v in range(3)]
    rpts = (1, 2, 2)
    recs = [mc.records(b, M, mc.tile_segments(n, rpt)) for b, rpt in zip(blocks, rpts)]
    ts = [_rle_job(b, M, rec if rpt == 2 else None, rpt, ws_bytes) for b, rec, rpt in zip(blocks, recs, rpts)]
    _lib.call("hic_rle_tile_records_i16", device.ptr(ts[0]["blocks"]), n, M, device.ptr(ts[0]["ws"]),
              device.stream_ptr())
    np.testing.assert_array_equal(device.to_host(ts[0]["ws"][:3 * len(recs[0])]).reshape(-1, 3), recs[0])
    jobs = (_lib.RleJob16 * 3)(*[t["job"] for t in ts])
    _lib.call("hic_rle_encode_i16_tiles_batch", 3, jobs, M, device.stream_ptr())
    for v, (t, b) in enumerate(zip(ts, blocks)):
        _check_rle(t, b, M, "job %d" % v)
    # the one-call form (tile pass + scan + emit) on the same blocks
    for v, b in enumerate(blocks):
        t = _rle_job(b, M, None, 1, ws_bytes)
        _lib.call("hic_rle_encode_i16", device.ptr(t["blocks"]), n, 64, M, None, device.ptr(t["dc"]),
                  device.ptr(t["L"]), device.ptr(t["V"]), t["cap"], device.ptr(t["cnt"]), device.ptr(t["ws"]),
                  device.stream_ptr())
        _check_rle(t, b, M, "one call %d" % v)


@pytest.mark.parametrize("M", mc.M_RLE)
def test_rle_rows_crafted_blocks(M):
    """hic_rle_encode_i16_rows_batch over the same blocks in rows of 66 blocks (a
    64-block tile and a 2-block one per row; records per tile 1 and 2) and of 2 blocks
    (one short record per row), the records computed on the host."""
    lib = _lib.load()
    full = [mc.crafted_blocks(M, v)[0] for v in range(3)]
    spec = [(full[0][:330], 66, 1), (full[1][:330], 66, 2), (full[2][:330], 66, 2), (full[1][:40], 2, 2)]
    ts = []
    for b, rowb, rpt in spec:
        b = np.ascontiguousarray(b)
        rec = mc.records(b, M, mc.row_segments(len(b), rowb, rpt))
        ts.append(_rle_job(b, M, rec, rpt, lib.hic_rle_rows_workspace_bytes(len(b), rowb, rpt)))
    jobs = (_lib.RleJob16 * 4)(*[t["job"] for t in ts])
    rowb = (ctypes.c_int64 * 4)(*[s[1] for s in spec])
    _lib.call("hic_rle_encode_i16_rows_batch", 4, jobs, rowb, M, device.stream_ptr())
    for i, (t, (b, rb, rpt)) in enumerate(zip(ts, spec)):
        _check_rle(t, np.ascontiguousarray(b), M, "job %d rows of %d rpt %d" % (i, rb, rpt))


@pytest.mark.parametrize("M", [0, 257])
def test_encoder_refuses_max_len_outside_1_256(M):
    """Host-side argument errors: encode raises ValueError, and nothing is written past
    the workspaces or the symbol buffers (no symbol is written at all)."""
    H, W = 64, 512
    enc = pipeline.Encoder(H, W, max_len=M)
    assert not enc.slots and enc.fused
    pad = {}
    for k in CH:
        n = enc.ws[k].numel()
        ws = device.zeros((n + 64,), torch.int64)
        ws[n:] = 0x5A5A5A5A5A5A5A5A
        enc.ws[k] = ws
        enc.sym_len[k] = torch.full((enc.cap[k] + 64,), CANARY, dtype=torch.uint8, device="cuda")
        enc.sym_val[k] = torch.full((enc.cap[k] + 64,), CANARY, dtype=torch.int16, device="cuda")
        pad[k] = n
    with pytest.raises(ValueError, match="max_len"):
        enc.encode(device.to_device(mc.image("noise_band", H, W)))
    torch.cuda.synchronize()
    for k in CH:
        assert (enc.ws[k][pad[k]:] == 0x5A5A5A5A5A5A5A5A).all().item(), k
        assert (enc.sym_len[k] == CANARY).all().item() and (enc.sym_val[k] == CANARY).all().item(), k
    assert enc.counts.cpu().tolist() == [0, 0, 0]
