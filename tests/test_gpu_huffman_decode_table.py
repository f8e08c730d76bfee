"""GPU tests of the table form of the Huffman decode: hic_huffman_decode_table (m
streams, one launch per phase over a table in device memory) against
HuffmanTree.decode_data's walk and against hic_huffman_decode_batch, stream for
stream; the chain path with a Python model of the rounds in front of it; errors;
codec.decode_batch / decode_regions end to end on both paths; the number of calls."""
import ctypes

import numpy as np
import pytest
import torch

from hiccup_amd import _lib, codec, device, hicimage, huffman

pytestmark = pytest.mark.gpu

GUARD = 8  # int32 words after every stream's out_cap
SENTINEL = 0x5A5A5A5A
K_SUB, K_DT, K_MAX_ROUNDS = 256, 256, 24  # huffdec.hip's kSub, kDT, kMaxRounds


# ------------------------------------------------------------------ helpers
def _pack(bits):
    return hicimage.BitStringP(bits).packed_bits()


def _run(entry, streams, caps=None, stream=None):
    """One call of `entry` ('table' or 'batch') over streams = [(bits, tree)]:
    (rc, [(out tensor with its guard words, count, status)]).  caps[i] overrides
    stream i's out_cap (default: nbits // the shortest code)."""
    lib = _lib.load()
    m = len(streams)
    packed = [_pack(b) for b, _ in streams]
    offs, tot = [], 0
    for _, nb in packed:
        offs.append(tot)
        tot += -(-max(nb, 1) // 32) * 4
    keep = []
    with device.on_stream(stream):
        dbits = device.to_device_parts([p[:-(-nb // 8)] for p, nb in packed], offs, tot)
        jobs = (_lib.HuffDecodeJob * m)()
        for k, ((_, tree), (_, nb)) in enumerate(zip(streams, packed)):
            child, nnodes, h_vals, nleaves, ml = tree.decode_args()
            ml = ml() if callable(ml) else ml
            cap = max(nb // ml, 1) if caps is None or caps[k] is None else caps[k]
            out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
            ws = None
            if entry == "batch":
                ws = device.workspace(lib.hic_huffman_decode_workspace_bytes(nb, nnodes, nleaves))
            keep.append((out, cap, ws, child, h_vals))
            jobs[k] = _lib.HuffDecodeJob(dbits.data_ptr() + offs[k], nb, child.ctypes.data, nnodes,
                                         h_vals.ctypes.data if h_vals is not None else None, nleaves, out.data_ptr(),
                                         cap, ws.data_ptr() if ws is not None else None, -1, -9)
        if entry == "batch":
            rc = lib.hic_huffman_decode_batch(m, jobs, device.stream_ptr(stream))
        else:
            ws = device.workspace(lib.hic_huffman_decode_table_workspace_bytes(m, jobs))
            rc = lib.hic_huffman_decode_table(m, jobs, device.ptr(ws), ws.numel() * 8, device.stream_ptr(stream))
    return rc, [(k[0], k[1], int(j.count), int(j.status)) for k, j in zip(keep, jobs)]


def _values(tree, out, n):
    """The first n decoded symbols as the reference's values (leaf indices mapped back)."""
    got = out[:n].cpu().tolist()
    if tree.decode_args()[2] is not None:
        return got
    leaves = tree.flat()[1]
    return [leaves[i].value for i in got]


def _check_guards(results):
    for out, cap, _, _ in results:
        assert out[cap:].cpu().tolist() == [SENTINEL] * GUARD


def _both_equal(streams, want, caps=None):
    """Both entry points on the same streams: equal rc, statuses, counts and symbols,
    guard words untouched; where want[i] is a list, stream i == want[i] in full."""
    rt, table = _run("table", streams, caps)
    rb, batch = _run("batch", streams, caps)
    assert rt == rb
    _check_guards(table)
    _check_guards(batch)
    for i, ((bits, tree), t, b) in enumerate(zip(streams, table, batch)):
        assert t[2:] == b[2:], (i, t[2:], b[2:])
        n = min(t[2], t[1])
        assert torch.equal(t[0][:n], b[0][:n]), i
        if want[i] is not None:
            assert t[3] == _lib.HIC_OK and t[2] == len(want[i]), (i, t[2:], len(want[i]))
            assert _values(tree, t[0], n) == want[i], i
    return rt, table


def _coded(keys):
    """(bits, decoding tree, walk tree) of int keys under the encoder's own codes."""
    table = huffman.CodeBook(*huffman.first_appearance_counts(keys)).encode_table()
    codes = dict(table)
    bits = "".join(codes[int(k)] for k in keys)
    walk = huffman.HuffmanTree.construct_from_coding(table)
    return bits, huffman.FlatCodes.from_table(table) or walk, walk, codes


_mixed_cache = {}


def _mixed():
    """The stream kinds of test_huffman_decode_batch_streams and equal8, sized from
    less than one subsequence to several workgroups (65536 bits each): streams
    [(bits, tree)] and their decode_data walks, computed once."""
    if not _mixed_cache:
        rng = np.random.default_rng(20)
        streams, want, names = [], [], []
        for kind in ("values", "lengths", "none_leaf", "empty", "equal8", "single", "skewed"):
            names.append(kind)
            if kind == "none_leaf":
                t = huffman.HuffmanTree.construct_from_coding([(5, "1"), (6, "01")])  # "00" decodes to None
                bits = "1011" * 300 + "1"
                streams.append((bits, t))
                want.append(t.decode_data(bits))
                continue
            keys = {"values": np.round(rng.laplace(0, 40, 40_001)), "lengths": rng.integers(0, 15, 3_000),
                    "empty": np.array([4, 4, 9]), "single": np.full(33, 7), "equal8": rng.integers(0, 8, 50_000),
                    "skewed": (rng.geometric(0.35, 30_000) - 1) * 3 - 40}[kind].astype(np.int64)
            bits, tree, walk, codes = _coded(keys)
            if kind == "empty":
                bits = ""
            if kind == "equal8":  # equal-length codes: subsequences of 258 bits, not 256
                assert {len(c) for c in codes.values()} == {3}
            if kind == "skewed":
                assert max(len(c) for c in codes.values()) > 12  # past the LUT: the bit walk over child[]
            streams.append((bits, tree))
            want.append(walk.decode_data(bits))
            assert want[-1] == ([] if kind == "empty" else keys.tolist())
        nwg = [-(-len(b) // (K_SUB * K_DT)) for b, _ in streams]
        assert min(len(b) for b, _ in streams if b) < K_SUB and max(nwg) >= 4 and len(set(nwg)) >= 4, nwg
        assert any(a != b for a, b in zip(nwg, nwg[1:]))
        _mixed_cache["v"] = (streams, want, names)
    return _mixed_cache["v"]


# ------------------------------------------------------------------ tests
def test_mixed_streams_one_call():
    streams, want, _ = _mixed()
    rc, _ = _both_equal(streams, want)
    assert rc == _lib.HIC_OK
    # the Python entry: the same values and counts
    got = huffman.decode_streams([_pack(b) for b, _ in streams], [t for _, t in streams])
    for (d, n), (_, tree), w in zip(got, streams, want):
        assert n == len(w) and _values(tree, d, n) == w


def test_boundaries():
    """nbits = kDT * kSub - 1, + 0, + 1 (the last subsequence of a workgroup, the first
    of the next) and 1, 2, 5 bits short of each: decode_data of the truncated bits."""
    rng = np.random.default_rng(3)
    bits, tree, walk, _ = _coded(np.round(rng.laplace(0, 12, 20_000)).astype(np.int64))
    base = K_DT * K_SUB
    assert len(bits) > base + 1
    sizes = sorted({n - d for n in (base - 1, base, base + 1) for d in (0, 1, 2, 5)})
    streams = [(bits[:n], tree) for n in sizes]
    _both_equal(streams, [walk.decode_data(b) for b, _ in streams])


def _chain_input():
    """The complete prefix code "1", "01", ..., 28 zeros + "1", 29 zeros; a stream of
    300 all-zero codes (8700 zero bits: subsequences 0..32 all zero), then 5000 random
    symbols."""
    codes = ["0" * k + "1" for k in range(29)] + ["0" * 29]
    tree = huffman.HuffmanTree.construct_from_coding(list(enumerate(codes)))
    rng = np.random.default_rng(29)
    syms = [29] * 300 + rng.integers(0, 30, 5000).tolist()
    return "".join(codes[s] for s in syms), tree, syms


def _model_rounds(bits, limit=200):
    """huffdec.hip's rounds over 256-bit subsequences for _chain_input's code, on the
    host: (the first round without a change, per subsequence the round that gave it
    its final start).  A code at p: its zeros up to 29, plus the '1' if fewer."""
    n = len(bits)
    z = np.zeros(n + 1, np.int64)  # zeros from p on, capped at 29
    for p in range(n - 1, -1, -1):
        z[p] = min(z[p + 1] + 1, 29) if bits[p] == "0" else 0
    length = np.where(z[:n] >= 29, 29, z[:n] + 1)
    END = 1 << 62

    def exit_of(s, end):
        p = s
        while p < end:
            if p >= n or p + length[p] > n:
                return END
            p += int(length[p])
        return p

    nsub = -(-n // K_SUB)
    start = [i * K_SUB for i in range(nsub)]
    ex = [exit_of(start[i], (i + 1) * K_SUB) for i in range(nsub)]
    settled = [0] * nsub
    for rnd in range(1, limit):
        changed = False
        new = list(ex)
        for i in range(1, nsub):
            if ex[i - 1] != start[i]:
                start[i] = ex[i - 1]
                new[i] = exit_of(start[i], (i + 1) * K_SUB)
                settled[i] = rnd
                changed = True
        ex = new
        if not changed:
            return rnd, settled, start
    raise AssertionError("the model did not converge")


def test_chain_path():
    """A stream the rounds cannot synchronise within kMaxRounds: in the all-zero head
    every code is 29 bits and 256 i = 0 (mod 29) only for 29 | i, so each round gives
    exactly one more subsequence its true start; the model shows subsequence 28 settled
    in round 28 > 24, so the GPU result below comes through the serial chain.  Beside it
    in the same call: a stream that synchronises in a few rounds."""
    bits, tree, syms = _chain_input()
    assert len(bits) > K_DT * K_SUB  # two workgroups
    quiet, settled, start = _model_rounds(bits)
    assert settled[28] == 28 and quiet > K_MAX_ROUNDS + 1, (settled[:32], quiet)
    truth, p = set(), 0
    codes_len = [k + 1 for k in range(29)] + [29]
    for s in syms:
        truth.add(p)
        p += codes_len[s]
    assert all(s in truth or s >= len(bits) for s in start)  # the model ends on codeword starts
    assert tree.decode_data(bits) == syms
    mixed, want, names = _mixed()
    k = names.index("skewed")
    _both_equal([mixed[k], (bits, tree), mixed[names.index("lengths")]],
                [want[k], syms, want[names.index("lengths")]])


def test_errors_in_one_call():
    """One stream walks into a missing child, another has too small an out_cap: status
    and count as hic_huffman_decode_batch gives them, every other stream whole, no
    write at or past any out_cap."""
    mixed, want, names = _mixed()
    bad = huffman.HuffmanTree.construct_from_data([3, 3, 3])  # one leaf: '0' is a missing child
    bad_bits = "1" * 5000 + "0" + "1" * 50
    streams = [mixed[names.index("lengths")], (bad_bits, bad), mixed[names.index("skewed")],
               mixed[names.index("equal8")], mixed[names.index("values")]]
    full = [want[names.index("lengths")], None, want[names.index("skewed")], None, want[names.index("values")]]
    short = len(want[names.index("equal8")]) - 10
    caps = [None, None, None, short, None]
    rc, table = _both_equal(streams, full, caps)
    assert rc == _lib.HIC_ERR_ARG  # the first non-OK job's
    assert table[1][2:] == (5000, _lib.HIC_ERR_ARG)
    assert table[1][0][:5000].cpu().tolist() == [3] * 5000  # the symbols before the missing child
    assert table[3][2:] == (short + 10, _lib.HIC_ERR_CAPACITY)
    assert table[3][0][:short].cpu().tolist() == want[names.index("equal8")][:short]
    # capacity alone: that status comes back
    rc, _ = _both_equal([streams[0], streams[3]], [full[0], None], [None, short])
    assert rc == _lib.HIC_ERR_CAPACITY


def test_streams_device_raises_alike():
    mixed, want, names = _mixed()
    pay = [hicimage.BitStringP(b) for b, _ in mixed]
    trees = [t for _, t in mixed]
    bad = huffman.HuffmanTree.construct_from_data([3, 3, 3])
    bad_bits = hicimage.BitStringP("1" * 5000 + "0" + "1" * 50)
    big = huffman.HuffmanTree.construct_from_coding([(2 ** 40, "1"), (1, "0")])
    leaf = huffman.HuffmanTree.construct_from_leaves([(7, 3)])
    raised = {}
    for table in (True, False):
        got = codec._huffman_streams_device(pay, trees, table=table)
        for (d, n), w in zip(got, want):
            assert n == len(w) and d[:n].cpu().tolist() == w
        seen = []
        for p, t in (([bad_bits], [bad]), ([hicimage.BitStringP("10"), bad_bits], [big, bad]),
                     ([bad_bits, hicimage.BitStringP("10")], [bad, big])):
            with pytest.raises(Exception) as e:  # noqa: PT011 -- the two paths' exceptions are compared below
                codec._huffman_streams_device(pay[:2] + p + pay[2:], trees[:2] + t + trees[2:], table=table)
            seen.append((type(e.value), str(e.value)))
        raised[table] = seen
        if leaf.root.is_leaf:  # a one-node tree never reaches the library on either path
            with pytest.raises(Exception) as e:  # noqa: PT011
                codec._huffman_streams_device(pay[:1] + [hicimage.BitStringP("1")], trees[:1] + [leaf], table=table)
            raised[table].append((type(e.value), str(e.value)))
    assert raised[True] == raised[False]
    assert [t for t, _ in raised[True][:3]] == [AttributeError, ValueError, AttributeError]


def _images(kind, n, H, W):
    rng = np.random.default_rng(n + H + W)
    if kind == "random":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = 128 + 60 * np.sin(x / (31.0 + i)) * np.cos(y / (19.0 + i)) + rng.normal(0, 3, (H, W))
        out.append(np.clip(np.stack([base, base * 0.9 + 10, 255 - base], -1), 0, 255).astype(np.uint8))
    return np.stack(out)


_files_cache = {}


def _files(kind, n, H, W):
    key = (kind, n, H, W)
    if key not in _files_cache:
        _files_cache[key] = codec.encode_batch(_images(kind, n, H, W))
    return _files_cache[key]


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("shape", [(2, 16, 512), (7, 16, 512), (3, 32, 1024)])
def test_end_to_end(monkeypatch, shape, kind):
    n, H, W = shape
    files = _files(kind, n, H, W)
    origins = [(0, 16 * (i % 8)) for i in range(n)]
    monkeypatch.setattr(huffman, "decode_table_default", lambda m, bits: False)
    want = [codec.decode(f) for f in files]
    want_regions = codec.decode_regions(files, origins, 16, 48)
    for table in (False, True):
        monkeypatch.setattr(huffman, "decode_table_default", lambda m, bits, t=table: t)
        got = codec.decode_batch(files)
        assert len(got) == n and all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(got, want))
        assert codec.decode_regions(files, origins, 16, 48).tobytes() == want_regions.tobytes()
        assert codec.decode(files[-1]).tobytes() == want[-1].tobytes()
    monkeypatch.undo()
    assert huffman.decode_table_default(9 * n, 1) in (True, False)
    assert codec.decode_batch(files)[0].tobytes() == want[0].tobytes()  # whatever the default says


def _count_calls(monkeypatch, fn):
    """(library calls, device-to-host reads) fn() makes: every call on the loaded
    library (_lib.call's go through it too), device.to_host and .cpu()."""
    seen = {"lib": 0, "read": 0}
    real_to_host, real_cpu, lib = device.to_host, torch.Tensor.cpu, _lib.load()

    class Counting:
        def __getattr__(self, name):
            f = getattr(lib, name)
            if not callable(f):
                return f

            def g(*a):
                seen["lib"] += 1
                return f(*a)
            return g

    def to_host(t):
        seen["read"] += 1
        return real_to_host(t)

    def cpu(self, *a, **kw):
        seen["read"] += 1
        return real_cpu(self, *a, **kw)

    with monkeypatch.context() as m:
        m.setattr(_lib, "_lib", Counting())
        m.setattr(device, "to_host", to_host)
        m.setattr(torch.Tensor, "cpu", cpu)
        out = fn()
    return out, seen


def test_calls_do_not_grow_with_n(monkeypatch):
    """The Huffman stage of 2 and of 7 images of 16 x 512 (18 and 63 streams): the table
    path makes 2 library calls (the workspace size, the decode) and no host read of its
    own in Python (the library reads the round flags once per four rounds and the totals
    once, inside its one call); the loop's library calls grow with the streams."""
    seen = {}
    for n in (2, 7):
        files = _files("random", n, 16, 512)
        pay = [f.payloads[9 + j] for f in files for j in range(9)]
        trees = [codec._decoding_tree(f.payloads[j]) for f in files for j in range(9)]
        for table in (True, False):
            codec._huffman_streams_device(pay, trees, table=table)  # (warm)
            out, seen[n, table] = _count_calls(
                monkeypatch, lambda t=table: codec._huffman_streams_device(pay, trees, table=t))
            assert len(out) == 9 * n
    assert seen[2, True] == seen[7, True] == {"lib": 2, "read": 0}, seen
    assert seen[7, False]["lib"] > seen[2, False]["lib"] > seen[2, True]["lib"], seen


def test_side_stream():
    streams, want, _ = _mixed()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = huffman.decode_streams([_pack(b) for b, _ in streams], [t for _, t in streams], stream=side)
    for (d, n), (_, tree), w in zip(got, streams, want):
        assert n == len(w) and _values(tree, d, n) == w
    rc, res = _run("table", streams, stream=side)
    assert rc == _lib.HIC_OK
    for (out, cap, n, st), (_, tree), w in zip(res, streams, want):
        assert st == _lib.HIC_OK and _values(tree, out, n) == w
