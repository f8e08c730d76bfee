"""CPU tests of the slot fill (hic_slots_fill_batch, the receiving rank of a
gather_kind "slots" gather): every bad job is refused before anything launches,
the job struct's ctypes mirror has the header's layout, and the eligibility rule
of the gather kind.  No GPU, no kernel calls: every call below must be one the
library refuses (an accepted call would launch on these fake pointers)."""
import ctypes
import os
import subprocess

from hiccup_amd import _lib, sharding

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # never dereferenced (16-byte aligned)


def _chan(nblk=128, rpt=1, slot_len=P, slot_val=P, dc=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _lib.load().hic_rle_slots_workspace_bytes(nblk, rpt if rpt in (1, 2) else 1)
    return _lib.SlotJob(nblk, rpt, slot_len, slot_val, dc, P, ws, ws_bytes, P, P, P, nblk * 63 + 1)


def _seg(wire=None, blocks=P, nblk=64, block0=0, channel=0, table=0):
    return _lib.SlotFillJob(wire, blocks, nblk, block0, channel, table)


def _refused(needle, chans=None, segs=None, nchan=None, n=None, max_len=15):
    chans = [_chan(), _chan(64, 2)] if chans is None else chans
    segs = [_seg()] if segs is None else segs
    ca = (_lib.SlotJob * max(1, len(chans)))(*chans)
    sa = (_lib.SlotFillJob * max(1, len(segs)))(*segs)
    rc = _lib.load().hic_slots_fill_batch(len(chans) if nchan is None else nchan, ca,
                                          len(segs) if n is None else n, sa, max_len, None)
    assert rc == _lib.HIC_ERR_ARG, needle
    assert needle in _lib.last_error(), (needle, _lib.last_error())


def test_fill_refuses_bad_counts_and_max_len():
    _refused("nchan", nchan=0)
    _refused("nchan", chans=[_chan()] * 4)
    _refused("segments", n=0)
    _refused("segments", segs=[_seg()] * 33)
    _refused("max_len 15", max_len=14)
    lib = _lib.load()
    one = (_lib.SlotFillJob * 1)(_seg())
    assert lib.hic_slots_fill_batch(1, None, 1, one, 15, None) == _lib.HIC_ERR_ARG
    assert lib.hic_slots_fill_batch(1, (_lib.SlotJob * 1)(_chan()), 1, None, 15, None) == _lib.HIC_ERR_ARG


def test_fill_refuses_bad_channels():
    for kw in ({"slot_len": None}, {"slot_val": None}, {"dc": None}, {"ws": None}):
        _refused("null pointer", chans=[_chan(**kw)])
    _refused("16-byte aligned", chans=[_chan(slot_len=P + 8)])
    _refused("16-byte aligned", chans=[_chan(slot_val=P + 2)])
    _refused("records_per_tile", chans=[_chan(rpt=3)])
    _refused("records_per_tile", chans=[_chan(rpt=0)])
    _refused("whole records", chans=[_chan(nblk=96, rpt=1)])
    _refused("nblk", chans=[_chan(nblk=0)])
    need = _lib.load().hic_rle_slots_workspace_bytes(128, 1)
    _refused("workspace", chans=[_chan(ws_bytes=need - 8)])
    # a bad channel is refused even when no segment names it
    _refused("workspace", chans=[_chan(), _chan(64, 2, ws_bytes=8)])


def test_fill_refuses_bad_segments():
    _refused("exactly one", segs=[_seg(wire=P, blocks=P)])
    _refused("exactly one", segs=[_seg(wire=None, blocks=None)])
    _refused("16-byte aligned", segs=[_seg(blocks=P + 8)])
    _refused("16-byte aligned", segs=[_seg(wire=P + 4, blocks=None)])
    _refused("record boundaries", segs=[_seg(nblk=32)])             # half a 64-block record
    _refused("record boundaries", segs=[_seg(nblk=0)])
    _refused("record boundaries", segs=[_seg(nblk=-64)])
    _refused("record boundaries", segs=[_seg(block0=32)])
    _refused("record boundaries", segs=[_seg(block0=-64)])
    _refused("record boundaries", segs=[_seg(nblk=48, channel=1, table=1)])   # 32-block records
    _refused("record boundaries", segs=[_seg(nblk=32, block0=16, channel=1, table=1)])
    _refused("past the channel", segs=[_seg(nblk=128, block0=64)])
    _refused("past the channel", segs=[_seg(nblk=64, block0=128)])
    _refused("past the channel", segs=[_seg(nblk=64, block0=32, channel=1, table=1)])
    _refused("channel", segs=[_seg(channel=2)])
    _refused("channel", segs=[_seg(channel=-1)])
    _refused("table", segs=[_seg(table=2)])
    _refused("table", segs=[_seg(table=-1)])
    # a good segment does not excuse a bad one after it
    _refused("table", segs=[_seg(), _seg(nblk=32, channel=1, table=1), _seg(table=5)])


def test_fill_job_struct_matches_header(tmp_path):
    """_lib.SlotFillJob has hic_slot_fill_job's size and field offsets, as gcc lays them out."""
    cname, py = "hic_slot_fill_job", _lib.SlotFillJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hiccup_hip.h"', "int main(void) {",
             '  printf("size %%zu\\n", sizeof(%s));' % cname]
    for f, _ in py._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f))
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                         text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(py)
    assert [f for f, _ in py._fields_] == ["wire", "blocks", "nblk", "block0", "channel", "table_id"]
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


def test_slots_gather_eligible():
    for H, W, world in ((64, 512, 3), (1088, 1024, 8), (4320, 7680, 8)):
        assert sharding.slots_gather_eligible(H, W, world), (H, W, world)
    for H, W, world in ((64, 768, 2), (72, 512, 2), (32, 512, 3)):
        assert not sharding.slots_gather_eligible(H, W, world), (H, W, world)
    assert not sharding.slots_gather_eligible(64, 512, 3, max_len=14)
    assert sharding.slots_gather_eligible(64, 512, 3, max_len=15)
