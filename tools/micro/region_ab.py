#!/usr/bin/env python3
"""Region decode against the whole-image indexed decode, in one process:

  per stream kind (the slot layout, the contiguous stream + tile index), one random
  16384 x 16384 image encoded once:
    full    Decoder.decode(index=...)                      the whole image
    w4096   RegionDecoder.decode of an unaligned 4096 x 4096 window (1/16 of the image)
    w1024   RegionDecoder.decode of an unaligned 1024 x 1024 window (1/256)
  the legs of a round run back to back in an order that rotates every round, each
  between device events after a synchronise; WARMUP untimed rounds, then ROUNDS timed
  ones.  Every window is checked once against the crop of the full decode.  Reported
  per leg: median and quartiles (ms), the 64-block tiles decoded (a tile that wraps
  two block rows of a window counts once per row) and microseconds per tile.
  window_below_full: the medians' gap against the larger interquartile range.
  For the contiguous stream also pipeline.stream_index: the index rebuilt from the bare
  stream, checked equal to the encoder's own, and timed.

  codec.open against codec.decode on one random 8K (7680 x 4320) .hic, host clock
  around the call (both end with data on the host or a status read), alternating;
  then decode_region(1024 x 1024) from the opened file, copy to the host included.

Writes region_ab.json under --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hiccup_amd import codec, device, pipeline, settings  # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = lambda p: round(float(np.percentile(v, p)), 4)  # noqa: E731
    return {"median": q(50), "p25": q(25), "p75": q(75), "min": q(0), "max": q(100), "n": int(v.size)}


def compare(slow, fast):
    s, f = stats(slow), stats(fast)
    gap = s["median"] - f["median"]
    spread = max(s["p75"] - s["p25"], f["p75"] - f["p25"])
    return {"gap_ms": round(gap, 4), "spread_ms": round(spread, 4), "holds": bool(gap > spread)}


def timed(f):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = f()
    b.record()
    torch.cuda.synchronize()
    return r, a.elapsed_time(b)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def ntiles(plan, W):
    return len(pipeline.window_tiles(plan, W)) + 2 * len(pipeline.window_tiles(plan, W, chroma=True))


def stream_kind(name, S, rounds, warmup, slots):
    g = torch.Generator(device="cuda")
    g.manual_seed(10)
    rgb = torch.randint(0, 256, (S, S, 3), dtype=torch.uint8, device="cuda", generator=g)
    enc = pipeline.Encoder(S, S, index=True, slots=slots)
    enc.encode(rgb)
    del rgb
    args = (enc.sym_len, enc.sym_val, enc.counts, enc.dc)
    dec = pipeline.Decoder(S, S)
    wins = {"w4096": (S // 2 - 2047 + 6, S // 2 - 2047 + 10, 4096, 4096),
            "w1024": (S // 2 + 1001, S // 2 - 3003, 1024, 1024)}
    rds = {k: pipeline.RegionDecoder(S, S, w[2], w[3]) for k, w in wins.items()}
    legs = {"full": lambda: dec.decode(*args, index=enc.index)}
    for k, w in wins.items():
        legs[k] = (lambda k=k, w=w: rds[k].decode(*w, *args, enc.index))
    full = legs["full"]()
    dec.check_status()
    for k, (y0, x0, h, w) in wins.items():
        assert torch.equal(legs[k](), full[y0:y0 + h, x0:x0 + w]), k
        rds[k].check_status()
    t = {k: [] for k in legs}
    order = list(legs)
    for rnd in range(warmup + rounds):
        for k in order[rnd % 3:] + order[:rnd % 3]:
            _, ms = timed(legs[k])
            if rnd >= warmup:
                t[k].append(ms)
    nb = pipeline._nblk
    tiles = {"full": -(-nb(S, S) // 64) + 2 * -(-nb(S // 2, S // 2) // 64)}
    for k, w in wins.items():
        tiles[k] = ntiles(pipeline.window_plan(S, S, *w), S)
    out = {"layout": name, "slots": bool(enc.slots), "legs": {}}
    for k in legs:
        st = stats(t[k])
        out["legs"][k] = dict(st, tiles=tiles[k], us_per_tile=round(st["median"] * 1e3 / tiles[k], 4),
                              window=list(wins[k]) if k in wins else None,
                              resident_bytes=(sum(b.numel() for b in (rds[k].rgb, rds[k].cr, rds[k].cb)) if k in wins
                                              else dec.rgb.numel() + sum(p.numel() for p in dec.pix.values())))
    for k in wins:
        out[k + "_below_full"] = compare(t["full"], t[k])
    if not enc.slots:
        # the index rebuilt from the bare stream: equal to the emit's own, and its cost
        counts = enc.counts.cpu().tolist()
        build = lambda: pipeline.stream_index(enc.sym_len, enc.sym_val, counts, enc.dc, S, S)  # noqa: E731
        index, status = build()
        assert all(torch.equal(index[k], enc.index[k]) for k in pipeline.CHANNELS)
        assert status.cpu().tolist() == [enc.coef[k].shape[0] * 63 for k in pipeline.CHANNELS]
        out["stream_index"] = dict(stats([timed(build)[1] for _ in range(rounds)]), symbols=counts,
                                   what="pipeline.stream_index of the three channels (workspaces allocated inside)")
    return out


def codec_open(H, W, rounds):
    rng = np.random.default_rng(8)
    hic = codec.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    t = {"decode": [], "open": [], "region_1024": []}
    full = None
    for rnd in range(2 + rounds):
        res = {}
        for k, f in (("decode", codec.decode), ("open", codec.open))[::-1 if rnd % 2 else 1]:
            res[k] = wall(lambda: f(hic))
        o = res["open"][0]
        o.decode_region(0, 0, 1024, 1024)  # the window buffers' allocation and the kernels' first launch
        res["region_1024"] = wall(lambda: o.decode_region(H // 2 - 333, W // 2 + 77, 1024, 1024))
        if full is None:
            full = res["decode"][0]
            assert np.array_equal(res["region_1024"][0], full[H // 2 - 333:H // 2 + 691, W // 2 + 77:W // 2 + 1101])
        if rnd >= 2:
            for k in t:
                t[k].append(res[k][1])
    st = o._streams
    resident = sum(x.numel() * x.element_size() for d in (st[0], st[1], st[3], st[4]) for x in d.values())
    return {"workload": "%dx%d random .hic, host clock, ms" % (W, H), "legs": {k: stats(v) for k, v in t.items()},
            "open_below_decode": compare(t["decode"], t["open"]), "open_resident_bytes": int(resident)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--codec-rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "region"))
    a = ap.parse_args()
    device.require_gpu()
    settings.DEBUG = False
    out = {"workload": "%d x %d random RGB, %d warm-up + %d timed rounds, device events, one process" %
                       (a.size, a.size, a.warmup, a.rounds),
           "device": torch.cuda.get_device_name(0), "unit": "ms", "kinds": []}
    for name, slots in (("slot layout", None), ("contiguous stream + tile index", False)):
        out["kinds"].append(stream_kind(name, a.size, a.rounds, a.warmup, slots))
        torch.cuda.empty_cache()
    out["codec_8k"] = codec_open(4320, 7680, a.codec_rounds)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "region_ab.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
