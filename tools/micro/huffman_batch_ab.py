#!/usr/bin/env python3
"""A/B of the batched Huffman stage on ONE GPU, both legs on the current stream:

  loop   BatchEncoder.hic_images(batched=False): one huffman.DeviceStreams per image
         (about 40 runtime calls and 3 host waits per image)
  batch  BatchEncoder.hic_images(batched=True): huffman.BatchStreams, one pass per
         phase over all 9 n streams

per shape n x H x W (default 64x512^2, 16x1024^2, 4x2048^2, 1x4320x7680), after an
untimed BatchEncoder.encode.  What the batch removes is host waits and launch
overhead, which device events between kernels do not see: both legs are timed as
HOST WALL TIME around one synchronised call.  Before anything is timed the legs'
bytes are compared at the timed size.  WARMUP untimed pairs, then PAIRS timed ones of
STEPS calls each, the legs swapping places every pair; per leg the min-max range of
the per-call means is reported, and a leg counts as faster only when the ranges do
not overlap.  Python's cyclic collector is paused inside every timed window, as
codec.encode_batch pauses it (with it running, full collections set off by the
payload objects add 10-160 ms to single calls of either leg).  Also timed the same
way: the whole of codec.encode_batch from host arrays with the stage forced either
way (e2e_loop / e2e_batch), and -- with the GPU idle -- the Python payload assembly
of the batch leg (host_payloads: the table payloads and the HicImage objects), to
show what is left on the host.

--legs loop runs only what a checkout without the batched stage has (hic_images()
and codec.encode_batch as they are there): that run is the parent's measurement.
Writes huffman_batch_ab.json under --out.  Needs a GPU."""
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
from hiccup_amd import codec, device, pipeline  # noqa: E402

SHAPES = "64x512x512,16x1024x1024,4x2048x2048,1x4320x7680"
HAS_BATCHED = "batched" in inspect.signature(pipeline.BatchEncoder.hic_images).parameters


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
    """pipeline.batched_default answering `value` inside the context (where it exists)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = getattr(pipeline, "batched_default", None)
        if self.saved is not None:
            pipeline.batched_default = lambda *a: self.value

    def __exit__(self, *exc):
        if self.saved is not None:
            pipeline.batched_default = self.saved
        return False


def run_shape(n, H, W, a):
    host = images(a.kind, n, H, W)
    batch = pipeline.BatchEncoder(n, H, W)
    batch.encode(device.to_device(host))
    torch.cuda.synchronize()

    def e2e(value):
        with forced(value):
            return codec.encode_batch(host)

    legs = {}
    if "loop" in a.legs:
        legs["loop"] = (lambda: batch.hic_images(batched=False)) if HAS_BATCHED else (lambda: batch.hic_images())
        legs["e2e_loop"] = lambda: e2e(False)
    if "batch" in a.legs:
        legs["batch"] = lambda: batch.hic_images(batched=True)
        legs["e2e_batch"] = lambda: e2e(True)
    outs = {k: [h.byte_stream() for h in f()] for k, f in legs.items()}
    first = next(iter(outs.values()))
    if any(v != first for v in outs.values()):
        raise SystemExit("%dx%dx%d: the legs' bytes differ" % (n, H, W))
    names = list(legs)
    t = {k: [] for k in names}
    for p in range(a.warmup + a.pairs):
        for k in names[::-1 if p % 2 else 1]:
            ms = wall(legs[k], a.steps)
            if p >= a.warmup:
                t[k].append(ms)
    if "batch" in a.legs:  # the batch leg's Python payload assembly alone, the GPU idle
        from hiccup_amd import huffman
        counts = batch.counts.cpu().tolist()
        bs = huffman.BatchStreams([[e.dc[k] for k in pipeline.CHANNELS] for e in batch.encoders],
                                  [e._slot_jobs() for e in batch.encoders], counts)
        packed = bs.packed()
        t["host_payloads"] = [wall(lambda: batch._assemble(bs.trees, packed), a.steps) for _ in range(a.pairs)]
    r = {k: {"min": round(min(v), 3), "max": round(max(v), 3), "median": round(float(np.median(v)), 3),
             "samples": [round(x, 3) for x in v]} for k, v in t.items()}
    res = {"n": n, "H": H, "W": W, "kind": a.kind, "unit": "ms of host wall time per call on the whole batch",
           "outputs_equal": True, "hic_bytes": sum(len(p) for b in first for p in b), **r}
    for x, y in (("loop", "batch"), ("e2e_loop", "e2e_batch")):
        if x in r and y in r:
            res["verdict_" + y] = ("faster (ranges apart)" if r[y]["max"] < r[x]["min"] else
                                   "slower (ranges apart)" if r[x]["max"] < r[y]["min"] else "ranges overlap: no claim")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x H x W")
    ap.add_argument("--legs", default="loop,batch", help="loop, batch or both")
    ap.add_argument("--kind", default="random", choices=("random", "smooth"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "huffman_batch"))
    ap.add_argument("--name", default="huffman_batch_ab.json")
    a = ap.parse_args()
    a.legs = a.legs.split(",")
    if a.steps < 1 or a.pairs < 5 or a.warmup < 1 or not set(a.legs) <= {"loop", "batch"}:
        ap.error("at least 1 call per window, 5 timed pairs and 1 warm-up pair; legs loop and / or batch")
    if "batch" in a.legs and not HAS_BATCHED:
        ap.error("this checkout has no batched stage: --legs loop")
    device.require_gpu()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    out = {"workload": "%s RGB; after an untimed BatchEncoder.encode; host wall time around synchronised calls; %d "
                       "calls per window; %d warm-up + %d timed alternating pairs" % (a.kind, a.steps, a.warmup, a.pairs),
           "legs": a.legs, "batched_stage_present": HAS_BATCHED, "device": torch.cuda.get_device_name(0), "shapes": []}
    os.makedirs(a.out, exist_ok=True)
    for n, H, W in shapes:
        out["shapes"].append(run_shape(n, H, W, a))
        print(json.dumps(out["shapes"][-1]), flush=True)
        with open(os.path.join(a.out, a.name), "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
