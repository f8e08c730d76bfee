#!/usr/bin/env python3
"""A/B of the Huffman decode in front of codec.decode_batch on ONE GPU, both legs on
the current stream:

  loop   codec._huffman_streams_device(..., table=False): hic_huffman_decode_batch,
         every phase once per stream (17 or more runtime calls per stream and a
         4096-entry lookup table built on the host and uploaded for each)
  table  codec._huffman_streams_device(..., table=True): hic_huffman_decode_table, one
         launch per phase over a table of all 9 n streams, the lookup tables built on
         the GPU

per shape n x H x W (default 64x512^2, 16x1024^2, 4x2048^2, 1x4320x7680), over the
files of an untimed codec.encode_batch and their trees built beforehand.  What the
table form removes is runtime calls, uploads and host table steps, which device
events between kernels do not see: both legs are timed as HOST WALL TIME around
synchronised calls.  Before anything is timed the legs' symbols are compared.  WARMUP
untimed pairs, then PAIRS timed windows of STEPS calls each, the legs swapping places
every pair, Python's cyclic collector paused inside every window (codec.decode_batch
pauses it too); per leg the min-max range of the per-call means is reported, and a
leg counts as faster only when the ranges do not overlap.  Timed the same way: the
whole of codec.decode_batch with the stage forced either way (e2e_loop / e2e_table),
and what stays per image after the stage: the trees from the tables
(huffman.FlatCodes.from_table, host only), codec._fast_symbols (narrowing and range
checks) and pipeline.stream_index, each over all n images.

--legs loop runs only what a checkout without the table form has
(_huffman_streams_device and codec.decode_batch as they are there): that run, with
that checkout's library, is the parent's measurement.  Writes
huffman_decode_table_ab.json (or --name) under --out.  Needs a GPU."""
import argparse
import gc
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hiccup_amd import codec, device, huffman, pipeline  # noqa: E402

SHAPES = "64x512x512,16x1024x1024,4x2048x2048,1x4320x7680"
HAS_TABLE = "table" in inspect.signature(codec._huffman_streams_device).parameters


def images(kind, n, H, W):
    rng = np.random.default_rng(n + H + W)
    if kind == "random":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    # natural-image-like: few nonzero AC coefficients, long zero runs
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = 128 + 60 * np.sin(x / (31.0 + i)) * np.cos(y / (19.0 + i)) + rng.normal(0, 3, (H, W))
        out.append(np.clip(np.stack([base, base * 0.9 + 10, 255 - base], -1), 0, 255).astype(np.uint8))
    return np.stack(out)


def wall(f, steps):
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    finally:
        gc.enable()


class forced:
    """huffman.decode_table_default answering `value` inside the context (where it exists)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = getattr(huffman, "decode_table_default", None)
        if self.saved is not None:
            huffman.decode_table_default = lambda *a: self.value

    def __exit__(self, *exc):
        if self.saved is not None:
            huffman.decode_table_default = self.saved
        return False


def run_shape(n, H, W, a):
    files = codec.encode_batch(images(a.kind, n, H, W))
    tables = [[[q.numbers for q in f.payloads[i].payloads] for i in range(9)] for f in files]
    payloads = [f.payloads[9 + i] for f in files for i in range(9)]
    build_trees = lambda: [huffman.FlatCodes.from_table(t) for ft in tables for t in ft]  # noqa: E731
    trees = build_trees()
    assert all(t is not None for t in trees)
    torch.cuda.synchronize()

    def stage(table):
        if HAS_TABLE:
            return codec._huffman_streams_device(payloads, trees, table=table)
        return codec._huffman_streams_device(payloads, trees)

    def e2e(value):
        with forced(value):
            return codec.decode_batch(files)

    legs = {}
    if "loop" in a.legs:
        legs["loop"] = lambda: stage(False)
        legs["e2e_loop"] = lambda: e2e(False)
    if "table" in a.legs:
        legs["table"] = lambda: stage(True)
        legs["e2e_table"] = lambda: e2e(True)
    outs = {k: f() for k, f in legs.items()}
    sym = {k: [(int(c), d[:c].cpu().numpy().tobytes()) for d, c in v] for k, v in outs.items() if not k.startswith("e2e")}
    rgb = {k: [x.tobytes() for x in v] for k, v in outs.items() if k.startswith("e2e")}
    for group in (sym, rgb):
        first = next(iter(group.values()))
        if any(v != first for v in group.values()):
            raise SystemExit("%dx%dx%d: the legs' outputs differ" % (n, H, W))
    streams = next(v for k, v in outs.items() if not k.startswith("e2e"))
    nbits = sum(int(p.packed_bits()[1]) for p in payloads)
    del outs, sym, rgb
    names = list(legs)
    t = {k: [] for k in names}
    for p in range(a.warmup + a.pairs):
        for k in names[::-1 if p % 2 else 1]:
            ms = wall(legs[k], a.steps)
            if p >= a.warmup:
                t[k].append(ms)
    # what stays per image after the stage, each over all n images
    per_image = [streams[9 * m:9 * m + 9] for m in range(n)]
    syms = [codec._fast_symbols(H, W, s) for s in per_image]
    rest = {"host_trees": build_trees,
            "fast_symbols": lambda: [codec._fast_symbols(H, W, s) for s in per_image],
            "stream_index": lambda: [pipeline.stream_index(s[0], s[1], s[2], s[3], H, W) for s in syms]}
    for k, f in rest.items():
        f()
        t[k] = [wall(f, a.steps) for _ in range(a.pairs)]
    r = {k: {"min": round(min(v), 3), "max": round(max(v), 3), "median": round(float(np.median(v)), 3),
             "samples": [round(x, 3) for x in v]} for k, v in t.items()}
    res = {"n": n, "H": H, "W": W, "kind": a.kind, "streams": 9 * n, "coded_bits": nbits,
           "unit": "ms of host wall time per call on the whole batch", "outputs_equal": True, **r}
    for x, y in (("loop", "table"), ("e2e_loop", "e2e_table")):
        if x in r and y in r:
            res["verdict_" + y] = ("faster (ranges apart)" if r[y]["max"] < r[x]["min"] else
                                   "slower (ranges apart)" if r[x]["max"] < r[y]["min"] else "ranges overlap: no claim")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x H x W")
    ap.add_argument("--legs", default="loop,table", help="loop, table or both")
    ap.add_argument("--kind", default="random", choices=("random", "smooth"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r20", "huffman_decode_table"))
    ap.add_argument("--name", default="huffman_decode_table_ab.json")
    a = ap.parse_args()
    a.legs = a.legs.split(",")
    if a.steps < 1 or a.pairs < 5 or a.warmup < 1 or not set(a.legs) <= {"loop", "table"}:
        ap.error("at least 1 call per window, 5 timed pairs and 1 warm-up pair; legs loop and / or table")
    if "table" in a.legs and not HAS_TABLE:
        ap.error("this checkout has no table form: --legs loop")
    device.require_gpu()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    out = {"workload": "%s RGB; files of an untimed codec.encode_batch; host wall time around synchronised calls; %d "
                       "calls per window; %d warm-up + %d timed alternating pairs" % (a.kind, a.steps, a.warmup, a.pairs),
           "legs": a.legs, "table_form_present": HAS_TABLE, "device": torch.cuda.get_device_name(0), "shapes": []}
    os.makedirs(a.out, exist_ok=True)
    for n, H, W in shapes:
        out["shapes"].append(run_shape(n, H, W, a))
        print(json.dumps(out["shapes"][-1]), flush=True)
        with open(os.path.join(a.out, a.name), "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
