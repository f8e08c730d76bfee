"""CPU tests of the batched Huffman encode (include/hiccup_hip.h, round 17): the
hic_huffman_batch_* entry points exist and refuse every bad argument before any
device call, and hic_huffman_build_batch builds, per stream, what numpy's
flatnonzero + stable argsort by `first` + hic_huffman_build build today, which is the
reference's heap order (HuffmanTree.construct_from_counts).  No GPU, nothing launched."""
import ctypes

import numpy as np
import pytest

from hiccup_amd import _lib
from hiccup_amd.huffman import HuffmanTree

P = 1 << 20  # a 16-byte aligned address, never dereferenced
E = _lib.HIC_ERR_ARG
NAMES = ["hic_huffman_batch_key_range_workspace_bytes", "hic_huffman_batch_key_range",
         "hic_huffman_batch_histogram_workspace_bytes", "hic_huffman_batch_histogram",
         "hic_huffman_batch_pack_workspace_bytes", "hic_huffman_batch_pack", "hic_huffman_build_batch"]


def _job(nblk=128, rpt=1, **kw):
    ws = _lib.load().hic_rle_slots_workspace_bytes(nblk, rpt)
    f = dict(nblk=nblk, records_per_tile=rpt, slot_len=P, slot_val=P, dc_diff=P, d_index=P, workspace=P,
             workspace_bytes=ws, d_count=P, sym_len=P, sym_val=P, sym_cap=nblk * 63 + 1)
    f.update(kw)
    return _lib.SlotJob(**f)


def _image_jobs(n, bad=None):
    """3 n jobs of n 16 x 512 images (Y: 128 blocks, chroma: 32 blocks in half-tile
    records); bad = (index, fields) replaces one job's fields."""
    jobs = [_job(128, 1), _job(32, 2), _job(32, 2)] * n
    if bad is not None:
        k, kw = bad
        jobs[k] = _job(**dict(dict(nblk=jobs[k].nblk, rpt=jobs[k].records_per_tile), **kw))
    return (_lib.SlotJob * (3 * n))(*jobs)


def _dc(n, **over):
    dc = [_lib.KeyStream(P, 128), _lib.KeyStream(P, 32), _lib.KeyStream(P, 32)] * n
    for k, v in over.items():
        dc[int(k[1:])] = v
    return (_lib.KeyStream * (3 * n))(*dc)


def _arr(ct, v):
    return (ct * len(v))(*v)


def _calls(n, jobs, dc, max_len=15, **kw):
    """The three entry points' statuses, every argument in order except those given."""
    lib = _lib.load()
    m = 9 * max(n, 1)
    lo = kw.get("key_min", _arr(ctypes.c_int32, [0] * m))
    nb = kw.get("nbins", _arr(ctypes.c_int32, [1] * m))
    ob = kw.get("out_bytes", _arr(ctypes.c_int64, [64] * m))
    ws, big = kw.get("ws", P), kw.get("ws_bytes", 1 << 30)
    return (lib.hic_huffman_batch_key_range(n, jobs, dc, max_len, kw.get("mm", P), ws, big, None),
            lib.hic_huffman_batch_histogram(n, jobs, dc, max_len, lo, nb, kw.get("counts", P), kw.get("first", P), ws,
                                            big, None),
            lib.hic_huffman_batch_pack(n, jobs, dc, max_len, lo, nb, kw.get("cbits", P), kw.get("clen", P),
                                       kw.get("out", P), ob, kw.get("nbits", P), ws, big, None))


def test_entry_points_exist():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert hasattr(_lib, "KeyStream")
    assert lib.hic_abi_version() == 4  # functions were added, nothing changed


def test_batch_entry_points_refuse_bad_jobs():
    """Everything is checked before any device call: refused here without a GPU."""
    lib = _lib.load()
    bad = (E, E, E)
    n = 2
    jobs, dc = _image_jobs(n), _dc(n)
    for k in (0, -1, 4097):  # n outside 1 .. HIC_SLOTS_BATCH_MAX
        assert _calls(k, jobs, dc) == bad, k
        assert "HIC_SLOTS_BATCH_MAX" in _lib.last_error()
    assert _calls(n, None, dc) == bad and _calls(n, jobs, None) == bad
    assert _calls(n, jobs, dc, max_len=14) == bad
    assert "max_len 15" in _lib.last_error()
    assert _calls(n, jobs, dc, max_len=0) == bad
    # every slot job, as hic_slot_key_range checks it: the LAST job of the batch is the bad one
    for field in ("slot_len", "slot_val", "d_index", "workspace", "d_count"):
        assert _calls(n, _image_jobs(n, (5, {field: None})), dc) == bad, field
        assert "job 5: null pointer" in _lib.last_error(), field
    for kw in (dict(nblk=0), dict(nblk=100), dict(rpt=3), dict(slot_len=P + 4), dict(slot_val=P + 8),
               dict(d_index=P + 4), dict(workspace_bytes=8)):
        assert _calls(n, _image_jobs(n, (4, kw)), dc) == bad, kw
        assert "job 4" in _lib.last_error(), kw
    # the DC streams
    for ks, what in ((_lib.KeyStream(None, 32), "null pointer"), (_lib.KeyStream(P + 4, 32), "aligned"),
                     (_lib.KeyStream(P, 0), "n"), (_lib.KeyStream(P, 1 << 31), "n")):
        assert _calls(n, jobs, _dc(n, k5=ks)) == bad, what
        assert "DC stream 5" in _lib.last_error() and what in _lib.last_error()
    # the workspace: null, misaligned, too small (the queries say how much)
    assert _calls(n, jobs, dc, ws=None) == bad
    assert _calls(n, jobs, dc, ws=P + 8) == bad
    assert "workspace must be 16-byte aligned" in _lib.last_error()
    one = _arr(ctypes.c_int32, [1] * (9 * n))
    need = (lib.hic_huffman_batch_key_range_workspace_bytes(n),
            lib.hic_huffman_batch_histogram_workspace_bytes(n, jobs, dc, one),
            lib.hic_huffman_batch_pack_workspace_bytes(n, jobs, dc))
    assert min(need) > 0
    for i, nbytes in enumerate(need):
        assert _calls(n, jobs, dc, ws_bytes=nbytes - 1)[i] == E, i
    assert "workspace too small" in _lib.last_error()
    # the per-stream host arrays and the device outputs
    m = 9 * n
    for v in (0, -3, (1 << 24) + 1):  # nbins outside 1 .. 2^24, in the last stream
        assert _calls(n, jobs, dc, nbins=_arr(ctypes.c_int32, [1] * (m - 1) + [v]))[1:] == (E, E), v
        assert "stream %d: nbins" % (m - 1) in _lib.last_error()
    assert _calls(n, jobs, dc, nbins=None)[1:] == (E, E)
    assert _calls(n, jobs, dc, key_min=None)[1:] == (E, E)
    assert _calls(n, jobs, dc, mm=None)[0] == E
    assert _calls(n, jobs, dc, counts=None)[1] == E and _calls(n, jobs, dc, first=None)[1] == E
    assert _calls(n, jobs, dc, counts=P + 2)[1] == E
    for kw in (dict(cbits=None), dict(clen=None), dict(out=None), dict(out_bytes=None), dict(nbits=None),
               dict(cbits=P + 4), dict(nbits=P + 4)):
        assert _calls(n, jobs, dc, **kw)[2] == E, kw
    assert _calls(n, jobs, dc, out=P + 2)[2] == E  # a misaligned output
    assert "aligned" in _lib.last_error()
    for v in (62, 0, -4):  # outputs not 4-byte sized
        assert _calls(n, jobs, dc, out_bytes=_arr(ctypes.c_int64, [64] * (m - 1) + [v]))[2] == E, v
        assert "stream %d: out must be 4-byte aligned and sized" % (m - 1) in _lib.last_error()


def test_workspace_queries():
    """0 for what the calls refuse; the tables plus the phase's scratch otherwise."""
    lib = _lib.load()
    n = 3
    jobs, dc = _image_jobs(n), _dc(n)
    assert lib.hic_huffman_batch_key_range_workspace_bytes(0) == 0
    assert lib.hic_huffman_batch_key_range_workspace_bytes(4097) == 0
    table = lib.hic_huffman_batch_key_range_workspace_bytes(n)
    assert table >= 3 * n * 16 * 8  # a slot job alone holds more than 16 pointers
    assert lib.hic_huffman_batch_pack_workspace_bytes(n, _image_jobs(n, (1, dict(nblk=100))), dc) == 0
    # pack: two int64 per record (Y: 2 records, chroma: 1 each) and one per DC tile
    assert lib.hic_huffman_batch_pack_workspace_bytes(n, jobs, dc) >= table + 8 * n * (2 * 4 + 3)
    small = _arr(ctypes.c_int32, [10] * (9 * n))
    wide = _arr(ctypes.c_int32, [10] * (9 * n - 1) + [9000])  # the last channel's bins exceed the LDS: no partials
    a = lib.hic_huffman_batch_histogram_workspace_bytes(n, jobs, dc, small)
    b = lib.hic_huffman_batch_histogram_workspace_bytes(n, jobs, dc, wide)
    assert a >= table + 4 * 3 * n * 2 * 20 and b == a - 4 * 2 * 20
    assert lib.hic_huffman_batch_histogram_workspace_bytes(n, jobs, dc, _arr(ctypes.c_int32, [0] * (9 * n))) == 0


# ---------------------------------------------------------------- the trees
def _build_batch(streams, text=True):
    """hic_huffman_build_batch over [(counts, first)]: per stream (bins in order, lens,
    bits, code strings)."""
    m = len(streams)
    off = np.concatenate([[0], np.cumsum([len(c) for c, _ in streams])]).astype(np.int64)
    total = int(off[-1])
    c_all = np.concatenate([np.asarray(c, np.uint32) for c, _ in streams])
    f_all = np.concatenate([np.asarray(f, np.uint32) for _, f in streams])
    leaf_off, text_off = np.full(m + 1, -1, np.int64), np.full(m + 1, -1, np.int64)
    bins, lens, bits = np.full(total, -1, np.int32), np.zeros(total, np.uint8), np.zeros(total, np.uint64)
    buf = np.zeros(65 * total, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.call("hic_huffman_build_batch", m, p(c_all), p(f_all), p(off), p(leaf_off), p(bins), p(lens), p(bits),
              p(buf) if text else None, buf.size, p(text_off) if text else None)
    out = []
    for i in range(m):
        a, b = int(leaf_off[i]), int(leaf_off[i + 1])
        strs = buf[text_off[i]:text_off[i + 1]].tobytes().decode().split() if text else None
        out.append((bins[a:b].tolist(), lens[a:b].copy(), bits[a:b].copy(), strs))
    assert int(leaf_off[m]) == sum(int(np.count_nonzero(c)) for c, _ in streams)
    return out


def _per_stream(counts, first):
    """Today's sequence for one stream: flatnonzero, stable argsort by first,
    hic_huffman_build; and the pure-Python tree over the same leaves."""
    c, f = np.asarray(counts, np.uint32), np.asarray(first, np.uint32)
    present = np.flatnonzero(c)
    order = present[np.argsort(f[present], kind="stable")]
    cc = np.ascontiguousarray(c[order], dtype=np.int64)
    n = len(order)
    lens, bits = np.empty(n, np.uint8), np.empty(n, np.uint64)
    text = ctypes.create_string_buffer(65 * n)
    _lib.call("hic_huffman_build", cc.ctypes.data_as(ctypes.c_void_p), n, lens.ctypes.data_as(ctypes.c_void_p),
              bits.ctypes.data_as(ctypes.c_void_p), text)
    py = HuffmanTree.construct_from_counts(order.tolist(), cc.tolist()).encode_table()
    return order.tolist(), lens, bits, text.value.decode().split(), py


ABSENT = 0xFFFFFFFF
rng = np.random.default_rng(17)
_many = rng.permutation(200)
STREAMS = {
    "one key": ([0, 0, 7, 0], [ABSENT, ABSENT, 0, ABSENT]),
    "one bin": ([3], [0]),
    "two keys": ([5, 9], [1, 0]),
    "equal counts (tie order)": ([4] * 13, list(range(13))),
    "equal counts, first reversed": ([4] * 13, list(range(12, -1, -1))),
    "absent keys between present ones": ([2, 0, 0, 9, 0, 1, 1, 0, 30], [5, ABSENT, ABSENT, 0, ABSENT, 9, 2, ABSENT, 1]),
    "first disagrees with key order": ([1, 2, 3, 4, 5, 6], [40, 3, 17, 0, 99, 4]),
    "equal first (stable: by bin)": ([3, 1, 2], [0, 0, 0]),
    "many": ((rng.integers(0, 50, 200) * (rng.random(200) < 0.7)).tolist(), _many.tolist()),
    "skewed": ([1 << k for k in range(20)], list(range(20))),
}
for _c, _f in STREAMS.values():  # (an absent key's first is 0xFFFFFFFF, as the histogram leaves it)
    for _i, _v in enumerate(_c):
        if _v == 0:
            _f[_i] = ABSENT
    assert any(_c)


@pytest.mark.parametrize("name", list(STREAMS))
def test_build_batch_one_stream(name):
    counts, first = STREAMS[name]
    (bins, lens, bits, strs), = _build_batch([(counts, first)])
    order, elens, ebits, estrs, py = _per_stream(counts, first)
    assert bins == order
    np.testing.assert_array_equal(lens, elens)
    np.testing.assert_array_equal(bits, ebits)
    assert strs == estrs
    assert list(zip(bins, strs)) == py  # the reference's heap order
    if name in ("one key", "one bin"):
        assert strs == ["1"]


def test_build_batch_stream_boundaries():
    """Several streams of different nbins in one call, each equal to its own build:
    in both orders, so every stream has a different neighbour on each side."""
    names = list(STREAMS)
    for order in (names, names[::-1]):
        got = _build_batch([STREAMS[k] for k in order])
        for name, (bins, lens, bits, strs) in zip(order, got):
            ebins, elens, ebits, estrs, py = _per_stream(*STREAMS[name])
            assert bins == ebins and strs == estrs, name
            np.testing.assert_array_equal(lens, elens, err_msg=name)
            np.testing.assert_array_equal(bits, ebits, err_msg=name)
            assert list(zip(bins, strs)) == py, name
    # without the text: the same codes
    for (b0, l0, c0, _), (b1, l1, c1, s1) in zip(got, _build_batch([STREAMS[k] for k in names[::-1]], text=False)):
        assert s1 is None and b0 == b1 and np.array_equal(l0, l1) and np.array_equal(c0, c1)


def test_build_batch_refusals():
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    c, f = np.array([1, 0, 2], np.uint32), np.array([0, ABSENT, 1], np.uint32)
    off = np.array([0, 3], np.int64)
    lo, to = np.zeros(2, np.int64), np.zeros(2, np.int64)
    bins, lens, bits, text = np.zeros(3, np.int32), np.zeros(3, np.uint8), np.zeros(3, np.uint64), np.zeros(195, np.uint8)

    def call(**kw):
        a = dict(m=1, c=p(c), f=p(f), off=p(off), lo=p(lo), bins=p(bins), lens=p(lens), bits=p(bits), text=p(text),
                 cap=text.size, to=p(to))
        a.update(kw)
        return lib.hic_huffman_build_batch(a["m"], a["c"], a["f"], a["off"], a["lo"], a["bins"], a["lens"], a["bits"],
                                           a["text"], a["cap"], a["to"])
    assert call() == _lib.HIC_OK
    for k in ("c", "f", "off", "lo", "bins", "lens", "bits", "to"):
        assert call(**{k: None}) == E, k
    assert call(m=0) == E
    assert call(off=p(np.array([1, 3], np.int64))) == E
    assert call(off=p(np.array([0, 0], np.int64))) == E  # a stream without bins
    assert call(c=p(np.zeros(3, np.uint32))) == E  # no key present
    assert "no key present" in _lib.last_error()
    assert call(cap=3) == E  # two leaves: "1 0 " needs four bytes
    assert "text buffer too small" in _lib.last_error()
