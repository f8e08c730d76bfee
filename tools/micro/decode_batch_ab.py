#!/usr/bin/env python3
"""A/B of the batched decode on ONE GPU, both legs on one stream, from the slot-layout
streams of one BatchEncoder:

  loop   n Decoder.decode(index=batch[i].index) calls on n separate decoders (two
         launches per image: the chroma pair, then Y straight to RGB)
  batch  BatchDecoder.decode of the same n images (two launches for all of them)

per shape n x H x W (default 64x512^2, 16x1024^2, 4x2048^2, 1x4320x7680).  Before
anything is timed the two legs' outputs are compared at the timed size (RGB, the Cr /
Cb planes, the status words).  Each window is STEPS decodes of the whole batch between
one pair of device events (the queue stays full: the figure is the GPU's time per
batch, launch gaps included, not the host's launch pace unless the host is the
bottleneck -- which for the loop leg at small images is the point); WARMUP untimed
pairs, then PAIRS timed ones, the legs swapping places every pair.  Per leg the
min-max range is reported, and the batch counts as faster (or slower) only when the
two ranges do not overlap.  Writes decode_batch_ab.json under --out.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hiccup_amd import device, pipeline  # noqa: E402

LEGS = ("loop", "batch")
SHAPES = "64x512x512,16x1024x1024,4x2048x2048,1x4320x7680"


def equal(decs, bdec):
    """The loop's decoders against the batch's: pixels, chroma planes, status words."""
    torch.cuda.synchronize()
    for i, d in enumerate(decs):
        if not (torch.equal(d.rgb, bdec.rgb[i]) and torch.equal(d.pix["cr"], bdec.cr[i])
                and torch.equal(d.pix["cb"], bdec.cb[i]) and torch.equal(d.status, bdec.status[i])):
            return False
    return True


def run_shape(n, H, W, a):
    rng = np.random.default_rng(n + H + W)
    enc = pipeline.BatchEncoder(n, H, W)
    enc.encode(device.to_device(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)))
    decs = [pipeline.Decoder(H, W) for _ in range(n)]
    bdec = pipeline.BatchDecoder(n, H, W)

    def loop():
        for e, d in zip(enc.encoders, decs):
            d.decode(e.sym_len, e.sym_val, e.counts, e.dc, index=e.index)

    legs = {"loop": loop, "batch": lambda: bdec.decode(enc)}
    for f in legs.values():
        f()
    same = equal(decs, bdec)
    if not same:
        raise SystemExit("%dx%dx%d: the batch differs from the per-image decoders" % (n, H, W))
    bdec.check_status()
    t = {k: [] for k in LEGS}
    for p in range(a.warmup + a.pairs):
        for k in LEGS[::-1 if p % 2 else 1]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                legs[k]()
            e1.record()
            torch.cuda.synchronize()
            if p >= a.warmup:
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    r = {k: {"min": round(min(t[k]), 2), "max": round(max(t[k]), 2), "median": round(float(np.median(t[k])), 2),
             "samples": [round(x, 2) for x in t[k]]} for k in LEGS}
    if r["batch"]["max"] < r["loop"]["min"]:
        verdict = "batch faster (ranges apart)"
    elif r["loop"]["max"] < r["batch"]["min"]:
        verdict = "batch slower (ranges apart)"
    else:
        verdict = "ranges overlap: no claim"
    return {"n": n, "H": H, "W": W, "unit": "us per batch of n images", "outputs_equal": bool(same), **r,
            "per_image_us": {k: [round(r[k]["min"] / n, 2), round(r[k]["max"] / n, 2)] for k in LEGS},
            "verdict": verdict}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x H x W")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r14", "decode_batch"))
    a = ap.parse_args()
    if a.steps < 200 or a.pairs < 5 or a.warmup < 1:
        ap.error("at least 200 steps per window, 5 timed pairs and 1 warm-up pair")
    device.require_gpu()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    out = {"workload": "random RGB encoded by one BatchEncoder (slot layout); loop: n Decoder.decode(index=...) on n "
                       "decoders; batch: BatchDecoder.decode; one stream; %d decodes of the batch per window between "
                       "device events; %d warm-up + %d timed alternating pairs" % (a.steps, a.warmup, a.pairs),
           "device": torch.cuda.get_device_name(0), "shapes": []}
    os.makedirs(a.out, exist_ok=True)
    for n, H, W in shapes:
        out["shapes"].append(run_shape(n, H, W, a))
        print(json.dumps(out["shapes"][-1]), flush=True)
        with open(os.path.join(a.out, "decode_batch_ab.json"), "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
