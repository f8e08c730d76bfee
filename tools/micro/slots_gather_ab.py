#!/usr/bin/env python3
"""A/B of the receiving rank's work in a multi-GPU gather, on ONE GPU:
ShardEncoder.finish() of gather_kind "stream" (wire unpack into whole-image int16
blocks + records placed + the whole image's scan + emit) against gather_kind
"slots" (hic_slots_fill_batch from the wire segments and the rank's own blocks +
hic_rle_slots_close).

Every rank's ShardEncoder of an 8K image (world 8) is built on the one device for
both kinds; the shards are encoded and packed once and every sender's segment is
copied into the receiver's wire buffer, so the segments are in place before
anything is timed.  finish() is then timed with device events (REPS calls in a
row between one pair of events, so the queue stays full and the figure is the
GPU's time per call, not the host's launch pace), the two kinds back to back and
swapping places every pair, WARMUP untimed pairs, then PAIRS timed ones.  Both
landing zones' results are compared once at the end.  Under `rocprofv3
--kernel-trace --stats -- python tools/micro/slots_gather_ab.py` the kernel
statistics give the per-kernel times.  Writes slots_gather_ab.json under --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hiccup_amd import device, pipeline, sharding  # noqa: E402

KINDS = ("stream", "slots")


def build(kind, H, W, world, gather_to, rgb):
    """The receiver of one image's gather, its segments in place."""
    ses = [sharding.ShardEncoder(H, W, rank=r, world=world, gather_to=gather_to, gather_kind=kind)
           for r in range(world)]
    for se in ses:
        a, b = se.span
        sharding.encode_group([se], [device.to_device(rgb[a:b])])
    recv = ses[gather_to]
    for se in ses:
        if se.rank == gather_to:
            continue
        se.pack()
        for k in pipeline.CHANNELS:
            o0, o1 = recv.wranges[k][se.rank]
            recv.wire_full[k][o0:o1].copy_(se.wire_send[k])
    torch.cuda.synchronize()
    return recv


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = lambda p: round(float(np.percentile(v, p)), 2)  # noqa: E731
    return {"median": q(50), "min": q(0), "max": q(100), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--gather-to", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "slots_gather"))
    a = ap.parse_args()
    if a.pairs < 5:
        ap.error("at least 5 timed pairs")
    device.require_gpu()
    H, W = a.height, a.width
    if not sharding.slots_gather_eligible(H, W, a.world):
        ap.error("gather_kind 'slots' does not take %dx%d over %d ranks" % (W, H, a.world))
    rgb = np.random.default_rng(9).integers(0, 256, (H, W, 3), dtype=np.uint8)
    recv = {k: build(k, H, W, a.world, a.gather_to, rgb) for k in KINDS}
    t = {k: [] for k in KINDS}
    for p in range(a.warmup + a.pairs):
        for k in KINDS[::-1 if p % 2 else 1]:  # the kinds swap places every pair
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                recv[k].finish()
            e1.record()
            torch.cuda.synchronize()
            if p >= a.warmup:
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    res = {k: recv[k].whole.result() for k in KINDS}
    same = all(np.array_equal(res["stream"][c][i], res["slots"][c][i]) for c in pipeline.CHANNELS for i in range(4))
    if not same:
        raise SystemExit("the two kinds' streams differ")
    s = {k: stats(t[k]) for k in KINDS}
    gap = s["stream"]["median"] - s["slots"]["median"]
    spread = max(s[k]["max"] - s[k]["min"] for k in KINDS)
    out = {"workload": "%dx%d random RGB over %d ranks on one device, receiver rank %d, segments in place; "
                       "%d finish() calls between device events, per call; %d warm-up + %d timed alternating pairs" %
                       (W, H, a.world, a.gather_to, a.reps, a.warmup, a.pairs),
           "device": torch.cuda.get_device_name(0), "unit": "us",
           "finish": s, "samples": {k: [round(x, 2) for x in t[k]] for k in KINDS},
           "slots_below_stream": {"gap_us": round(gap, 2), "spread_us": round(spread, 2),
                                  "paired_gap_median_us": round(float(np.median(np.asarray(t["stream"]) -
                                                                                np.asarray(t["slots"]))), 2),
                                  "holds": bool(gap > spread)},
           "wire_bytes": {k: recv[k].wire_bytes for k in KINDS}, "streams_equal": bool(same)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "slots_gather_ab.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
