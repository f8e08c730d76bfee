"""CPU tests of the table form of the Huffman decode (hic_huffman_decode_table): the
exports, the workspace rule, every refusal (nothing may reach a device: the pointers
are fake), the calls that have nothing to do, and the lookup-table entry rule the
host loop and k_hd_lut_table share (csrc/huffdec_lut.h, compiled alone here)."""
import ctypes
import os
import subprocess

import numpy as np

from hiccup_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # never dereferenced (16-byte aligned)
BIG = 1 << 40  # a workspace size no layout below reaches

# node 0: '1' -> node 1, '0' -> leaf 2; node 1: leaves 0 and 1
CHILD = np.array([1, -4, -2, -3], np.int32)
VALUES = np.array([7, 8, 9], np.int32)


def _job(nbits=64, child=CHILD, nnodes=2, nleaves=3, bits=P, out=P, values=None, cap=64):
    return _lib.HuffDecodeJob(bits, nbits, child.ctypes.data if child is not None else None, nnodes,
                              values.ctypes.data if values is not None else None, nleaves, out, cap, None, 0, 0)


def _arr(*jobs):
    return (_lib.HuffDecodeJob * len(jobs))(*jobs)


def test_exports_and_abi():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "hic_huffman_decode_table") and hasattr(lib, "hic_huffman_decode_table_workspace_bytes")
    assert "hic_huffman_decode_table" in _lib.SIGNATURES
    assert "hic_huffman_decode_table_workspace_bytes" in _lib.SIGNATURES
    assert _lib.load().hic_abi_version() == 4


def _need(jobs):
    """A lower bound of what the table form keeps per call, from the issue's list:
    per stream a 152-byte table row, 16 bytes of totals, 16 of round flags, 4 of
    chain id, and for a stream with bits its tree, a 4096-entry LUT, start / exit_a /
    exit_b / cnt per 256-bit subsequence and a sum per 256 subsequences."""
    tot = 0
    for j in jobs:
        tot += 152 + 16 + 16 + 4
        if j.nbits:
            nsub = -(-j.nbits // 256)
            tot += 2 * j.nnodes * 4 + j.nleaves * 4 + 4096 * 4 + nsub * (3 * 8 + 4) + (-(-nsub // 256) + 1) * 8
    return tot


def test_workspace_rule():
    size = _lib.load().hic_huffman_decode_table_workspace_bytes
    sizes = (0, 1, 255, 256, 257, 65535, 65536, 65537, 1 << 20, (1 << 24) + 3)
    for other in (0, 5000):
        last = 0
        for nb in sizes:
            jobs = [_job(nbits=nb), _job(nbits=other, values=VALUES), _job(nbits=777)]
            got = size(3, _arr(*jobs))
            assert got >= last and got >= _need(jobs), (nb, other, got, _need(jobs))
            last = got
    # one more stream never needs less
    assert size(2, _arr(_job(), _job())) > size(1, _arr(_job()))
    # what the call refuses has no size
    assert size(0, None) == 0 and size(-1, _arr(_job())) == 0 and size(65536, _arr(_job())) == 0
    assert size(1, None) == 0 and size(1, _arr(_job(nbits=-1))) == 0


def test_refusals():
    lib = _lib.load()
    call = lib.hic_huffman_decode_table
    ok = _job()

    def refused(m, jobs, ws=P, nbytes=BIG, needle=None):
        assert call(m, jobs, ws, nbytes, None) == _lib.HIC_ERR_ARG, (m, needle)
        if needle is not None:
            assert needle in _lib.last_error(), (needle, _lib.last_error())

    bad_child = np.array([0, -2], np.int32)  # the root as its own child
    twice = np.array([1, 1, -2, -3], np.int32)  # node 1 the child of two edges
    refused(2, _arr(ok, _job(child=bad_child, nnodes=1, nleaves=1)), needle="tree edge")
    refused(2, _arr(ok, _job(child=twice)), needle="tree edge")
    refused(2, _arr(ok, _job(nleaves=2)), needle="tree edge")  # leaf 2 of 2
    refused(2, _arr(ok, _job(nnodes=0)), needle="tree size")
    refused(2, _arr(ok, _job(child=None)), needle="null pointer")
    refused(2, _arr(_job(bits=None), ok), needle="null pointer")
    refused(2, _arr(ok, _job(out=None)), needle="null pointer")
    refused(1, _arr(_job(bits=P + 2)), needle="4-byte aligned")
    refused(1, _arr(_job(nbits=-1)), needle="nbits")
    refused(1, _arr(_job(cap=-1)), needle="out_cap")
    refused(-1, _arr(ok), needle="65535")
    refused(65536, _arr(ok), needle="65535")
    refused(1, None, needle="jobs")
    need = lib.hic_huffman_decode_table_workspace_bytes(2, _arr(ok, ok))
    assert need > 0
    refused(2, _arr(ok, ok), ws=None, needle="null pointer")
    refused(2, _arr(ok, ok), nbytes=need - 1, needle="workspace")
    refused(2, _arr(ok, ok), nbytes=0, needle="workspace")
    refused(2, _arr(ok, ok), ws=P + 4, needle="aligned")
    # a job's own workspace field plays no part: a refusal is the same with one
    with_ws = _job()
    with_ws.workspace = P
    refused(2, _arr(with_ws, _job(child=bad_child, nnodes=1, nleaves=1)), needle="tree edge")


def test_nothing_to_do():
    lib = _lib.load()
    assert lib.hic_huffman_decode_table(0, None, None, 0, None) == _lib.HIC_OK
    jobs = _arr(_job(nbits=0, bits=None, out=None), _job(nbits=0))
    jobs[0].count, jobs[0].status = 5, -3
    need = lib.hic_huffman_decode_table_workspace_bytes(2, jobs)
    assert lib.hic_huffman_decode_table(2, jobs, P, need, None) == _lib.HIC_OK
    assert [(j.count, j.status) for j in jobs] == [(0, 0), (0, 0)]
    # an empty stream's tree is still checked
    bad_child = np.array([0, -2], np.int32)
    assert lib.hic_huffman_decode_table(1, _arr(_job(nbits=0, child=bad_child, nnodes=1, nleaves=1)), P, BIG,
                                        None) == _lib.HIC_ERR_ARG


def _walk_entry(child, v, bits=12):
    """One LUT entry by the header comment's definition: walk v's bits from the MSB."""
    node = 0
    for k in range(bits):
        c = int(child[2 * node + 1 - ((v >> (bits - 1 - k)) & 1)])
        if c == -1:
            return k | (2 << 4)
        if c <= -2:
            return k | (0 << 4) | ((-2 - c) << 8)
        node = c
    return (bits - 1) | (1 << 4) | (node << 8)


def test_lut_entry_rule(tmp_path):
    """hic_hd_lut_entry (the one body of decode_prepare's host loop and of
    k_hd_lut_table) == a bit-by-bit walk, on a tree with a missing child and on one
    whose codes run past the 12 LUT bits."""
    missing = [1, -1, -2, 2, -3, -1]  # '0' at the root and "100" walk into nothing
    deep = []
    for k in range(14):  # codes "1", "01", ..., 14 zeros + "1", 15 zeros
        deep += [-2 - k, k + 1]
    deep += [-2 - 14, -2 - 15]
    trees = {"missing": missing, "deep": deep}
    src = ['#include <stdio.h>', '#include "huffdec_lut.h"']
    for name, child in trees.items():
        src.append("static const int32_t %s[] = {%s};" % (name, ", ".join(map(str, child))))
    src.append("int main(void) {")
    for name in trees:
        src.append('  for (int v = 0; v < (1 << HIC_HD_LUT_BITS); ++v) printf("%s %%d %%u\\n", v, '
                   "hic_hd_lut_entry(%s, v));" % (name, name))
    src.append("  return 0;\n}")
    c = tmp_path / "lut.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "lut"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "hiccup_amd", "csrc"), str(c), "-o", str(exe)],
                   check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        name, v, e = line.split()
        got[name, int(v)] = int(e)
    assert len(got) == 2 * 4096
    kinds = {name: set() for name in trees}
    for (name, v), e in got.items():
        assert e == _walk_entry(trees[name], v), (name, v, e)
        kinds[name].add((e >> 4) & 3)
    assert kinds == {"missing": {0, 2}, "deep": {0, 1}}
