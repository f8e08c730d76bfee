"""CPU tests of the batched slot encode's host side (hic_slots_batch_table,
hic_encode420_slots_batch_u8, hic_rle_slots_close_batch): every bad job, table or
launch argument is refused before anything launches, and the table the builder
writes holds what it was given.  No GPU, no kernel calls: the pointers are fakes
that are never dereferenced, so every launch call below must be one the library
refuses (the table builder launches nothing and may succeed)."""
import ctypes
import struct

from hiccup_amd import _lib, pipeline

P = 1 << 32          # fake device addresses (16-byte aligned), never dereferenced
GAP = 1 << 26        # per job and kind: far more than any range of the shapes below
H, W = 32, 512


def _nblk(k, h=H, w=W):
    return (h // 8) * (w // 8) if k == 0 else (h // 16) * (w // 16)


def _jobs(n, h=H, w=W):
    """3 n good jobs: every range of every kind apart from every other."""
    lib = _lib.load()
    out = []
    for i in range(3 * n):
        k, base = i % 3, P + 8 * GAP * i
        nb, rpt = _nblk(k, h, w), 1 if k == 0 else 2
        out.append(_lib.SlotJob(nb, rpt, base, base + GAP, base + 2 * GAP, base + 3 * GAP, base + 4 * GAP,
                                lib.hic_rle_slots_workspace_bytes(nb, rpt), base + 5 * GAP, base + 6 * GAP,
                                base + 7 * GAP, nb * 63 + 1))
    return out


def _build(n, jobs, h=H, w=W, nbytes=None, null_jobs=False, null_table=False, n_arg=None):
    lib = _lib.load()
    size = lib.hic_slots_batch_table_bytes(n) if nbytes is None else nbytes
    buf = ctypes.create_string_buffer(b"\xaa" * max(size, 1), max(size, 1))
    arr = (_lib.SlotJob * max(1, len(jobs)))(*jobs)
    rc = lib.hic_slots_batch_table(n if n_arg is None else n_arg, h, w, None if null_jobs else arr,
                                   None if null_table else buf, size)
    return rc, buf


def _refused(needle, n, jobs, **kw):
    rc, buf = _build(n, jobs, **kw)
    assert rc == _lib.HIC_ERR_ARG, needle
    assert needle in _lib.last_error(), (needle, _lib.last_error())
    assert set(buf.raw) == {0xAA}, "a refused call wrote into the table (%s)" % needle


def _table(n=3):
    rc, buf = _build(n, _jobs(n))
    assert rc == _lib.HIC_OK, _lib.last_error()
    return buf


def test_table_refuses_bad_counts_and_buffers():
    lib = _lib.load()
    assert pipeline.BATCH_MAX == 4096
    _refused("HIC_SLOTS_BATCH_MAX", 1, _jobs(1), n_arg=0)
    _refused("HIC_SLOTS_BATCH_MAX", 1, _jobs(1), n_arg=pipeline.BATCH_MAX + 1)
    _refused("null pointer", 2, _jobs(2), null_jobs=True)
    _refused("null pointer", 2, _jobs(2), null_table=True)
    _refused("needed", 2, _jobs(2), nbytes=lib.hic_slots_batch_table_bytes(2) - 8)
    _refused("needed", 2, _jobs(2), nbytes=lib.hic_slots_batch_table_bytes(1))


def test_table_refuses_bad_shapes():
    _refused("W % 512", 1, _jobs(1, 32, 520), w=520)
    _refused("H % 16", 1, _jobs(1, 24, 512), h=24)


def _bad(jobs, i, **kw):
    j = jobs[i]
    for f, v in kw.items():
        setattr(j, f, v)
    return jobs


def test_table_refuses_bad_jobs():
    lib = _lib.load()
    _refused("nblk", 2, _bad(_jobs(2), 3, nblk=_nblk(0) + 64))
    _refused("records_per_tile", 2, _bad(_jobs(2), 4, records_per_tile=1))
    _refused("records_per_tile", 2, _bad(_jobs(2), 0, records_per_tile=2))
    _refused("16-byte aligned", 2, _bad(_jobs(2), 5, slot_len=P + 8))
    _refused("16-byte aligned", 2, _bad(_jobs(2), 0, slot_val=P + GAP + 2))
    need = lib.hic_rle_slots_workspace_bytes(_nblk(0), 1)
    _refused("workspace", 2, _bad(_jobs(2), 3, workspace_bytes=need - 8))
    for f in ("slot_len", "slot_val", "dc_diff", "d_index", "workspace", "d_count", "sym_len", "sym_val"):
        _refused("null pointer", 2, _bad(_jobs(2), 1, **{f: None}))


def test_table_refuses_shared_buffers():
    for f in ("slot_len", "slot_val", "dc_diff", "workspace"):
        jobs = _jobs(3)
        setattr(jobs[6], f, getattr(jobs[0], f))  # images 0 and 2, both Y
        _refused("share a " + f, 3, jobs)
    # overlapping, not equal: image 1's Cr slots start inside image 0's
    jobs = _jobs(2)
    jobs[4].slot_len = jobs[1].slot_len + 16
    _refused("share a slot_len", 2, jobs)


def test_table_refuses_a_bad_job_in_any_image():
    for img in (0, 2, 4):
        for k in range(3):
            _refused("image %d job %d" % (img, k), 5, _bad(_jobs(5), 3 * img + k, slot_val=None))
            _refused("image %d job %d" % (img, k), 5, _bad(_jobs(5), 3 * img + k, workspace_bytes=8))


def test_table_success_and_header():
    lib = _lib.load()
    sizes = [lib.hic_slots_batch_table_bytes(n) for n in (1, 2, 3, 64, pipeline.BATCH_MAX)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert lib.hic_slots_batch_table_bytes(0) == 0 == lib.hic_slots_batch_table_bytes(pipeline.BATCH_MAX + 1)
    for n in (1, 3, 5):
        buf = _table(n)
        magic, got_n, max_len, h, w = struct.unpack_from("<QiiQQ", buf.raw, 0)
        assert magic != 0xAAAAAAAAAAAAAAAA and (got_n, max_len, h, w) == (n, 15, H, W)
        # every job's slot arrays are in the blob, image by image
        jobs = _jobs(n)
        words = struct.unpack_from("<%dQ" % ((len(buf.raw) - 128) // 8), buf.raw, 128)
        for i, j in enumerate(jobs):
            entry = words[32 * (i // 3):32 * (i // 3 + 1)]
            assert j.slot_len in entry and j.slot_val in entry and j.dc_diff in entry and j.workspace in entry, i


def _launch_refused(needle, which, table=None, d_table=P, max_len=15, stride=H * W * 3, rgb=P):
    lib = _lib.load()
    table = _table() if table is None else table
    if which == "encode":
        rc = lib.hic_encode420_slots_batch_u8(rgb, stride, table, d_table, max_len, None, None, None)
    else:
        rc = lib.hic_rle_slots_close_batch(table, d_table, max_len, None)
    assert rc == _lib.HIC_ERR_ARG, (needle, which)
    assert needle in _lib.last_error(), (needle, _lib.last_error())


def test_launches_refuse_bad_tables_and_arguments():
    for which in ("encode", "close"):
        bad = _table()
        bad[3] = bytes([bad.raw[3] ^ 0x40])
        _launch_refused("magic", which, table=bad)
        bad = _table()
        struct.pack_into("<i", bad, 32, 99)  # a workgroup count that is not the shape's
        _launch_refused("damaged", which, table=bad)
        _launch_refused("max_len 15", which, max_len=14)
        _launch_refused("null pointer", which, d_table=None)
        _launch_refused("null pointer", which, table=ctypes.c_void_p(None))
        _launch_refused("16-byte aligned", which, d_table=P + 8)
    _launch_refused("image_stride", "encode", stride=H * W * 3 - 8)
    _launch_refused("image_stride", "encode", stride=H * W * 3 + 4)
    _launch_refused("8-byte aligned", "encode", rgb=P + 4)
    _launch_refused("null pointer", "encode", rgb=None)


def test_batch_slots_eligible():
    shapes = [(16, 512), (80, 1024), (48, 1536), (4320, 7680), (40, 200), (24, 512), (32, 520), (8, 512)]
    for h, w in shapes:
        for n in (1, 2, 9, 64):
            assert pipeline.batch_slots_eligible(n, h, w) == pipeline.slots_eligible(h, w), (n, h, w)
        for n in (0, -1):
            assert not pipeline.batch_slots_eligible(n, h, w)
    assert not pipeline.batch_slots_eligible(4, 64, 512, max_len=14)
    assert not pipeline.batch_slots_eligible(pipeline.BATCH_MAX + 1, 64, 512)
