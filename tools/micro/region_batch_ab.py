#!/usr/bin/env python3
"""A/B of the batched region decode on ONE GPU: a crop from each of n images.

  loop   what a caller had to do before: n RegionDecoder.decode calls (two launches
         per image, each into its own aligned scratch window) plus the n copies of the
         returned views into one (n, h, w, 3) tensor
  batch  BatchRegionDecoder.decode of the same n windows (one table upload, two
         launches, the crops stored straight into the tensor)

per configuration n x H x W : h x w (default 64x512x512:224x224, 16x1024x1024:224x224,
4x2048x2048:512x512, 1x4320x7680:1024x1024), from the slot-layout streams of one
BatchEncoder, with fresh random origins in every call (the same sequence for both legs,
drawn before anything is timed).  Each leg runs in FRESH processes, the legs
alternating, PAIRS pairs; --parent-lib names the library the loop leg loads (the parent
commit's build: the loop is then computed by the code a caller has today).  In a
process, per configuration: the leg's result is checked against the crops of the whole
decodes, WARMUP untimed windows, then one window of STEPS calls between a pair of device
events (the queue stays full: GPU time per call, launch gaps and the host's pace
included where the host is the bottleneck).  Per leg the min-max range over the
processes is reported; the batch counts as faster (or slower) only when the ranges lie
apart.  Writes region_batch_ab.json under --out.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("loop", "batch")
CONFIGS = "64x512x512:224x224,16x1024x1024:224x224,4x2048x2048:512x512,1x4320x7680:1024x1024"


def parse(configs):
    out = []
    for c in configs.split(","):
        img, win = c.split(":")
        out.append(tuple(int(v) for v in img.split("x")) + tuple(int(v) for v in win.split("x")))
    return out


def child(a):
    """One leg, every configuration, in this process: a JSON line {config: us per call}."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from hiccup_amd import device, pipeline

    device.require_gpu()
    res = {}
    for n, H, W, h, w in parse(a.configs):
        rng = np.random.default_rng(n + H + W + h)
        enc = pipeline.BatchEncoder(n, H, W)
        enc.encode(device.to_device(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)))
        calls = a.steps * (a.warmup + 1) + 1
        origins = np.stack([rng.integers(0, H - h + 1, (calls, n)), rng.integers(0, W - w + 1, (calls, n))], -1).tolist()
        out = device.empty((n, h, w, 3), torch.uint8)
        if a.leg == "batch":
            bdec = pipeline.BatchRegionDecoder(n, H, W, h, w, out=out)
            srcs = list(enc.encoders)

            def call(o):
                bdec.decode(srcs, o)
        else:
            rds = [pipeline.RegionDecoder(H, W, h, w) for _ in range(n)]
            args = [(e.sym_len, e.sym_val, e.counts, e.dc, e.index) for e in enc.encoders]

            def call(o):
                for i in range(n):
                    out[i].copy_(rds[i].decode(o[i][0], o[i][1], h, w, *args[i]))
        # the leg's result against the crops of the whole-image decodes, once
        call(origins[-1])
        full = pipeline.BatchDecoder(n, H, W).decode(enc)
        for i, (y0, x0) in enumerate(origins[-1]):
            if not torch.equal(out[i], full[i, y0:y0 + h, x0:x0 + w]):
                raise SystemExit("%s: image %d differs from the crop of its whole decode" % (a.leg, i))
        del full
        at = 0
        for win in range(a.warmup + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                call(origins[at])
                at += 1
            e1.record()
            torch.cuda.synchronize()
        res["%dx%dx%d:%dx%d" % (n, H, W, h, w)] = e0.elapsed_time(e1) * 1e3 / a.steps
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"leg": a.leg, "device": torch.cuda.get_device_name(0), "us": res}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default=CONFIGS, help="comma-separated n x H x W : h x w")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libhiccup_hip.so, loaded by the loop leg")
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "region_batch"))
    ap.add_argument("--leg", choices=LEGS, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg is not None:
        return child(a)
    if a.steps < 100 or a.pairs < 5 or a.warmup < 1:
        ap.error("at least 100 calls per window, 5 pairs of processes and 1 warm-up window")
    t = {k: {} for k in LEGS}
    dev = None
    for p in range(a.pairs):
        for leg in LEGS[::-1 if p % 2 else 1]:
            env = dict(os.environ)
            if leg == "loop" and a.parent_lib:
                env["HICCUP_HIP_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--configs", a.configs, "--steps",
                   str(a.steps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode or not line:
                # a leg that failed ends the run: nothing more is started on the GPU
                raise SystemExit("the %s leg failed (status %d):\n%s\n%s" % (leg, r.returncode, r.stdout, r.stderr))
            got = json.loads(line[0][7:])
            dev = got["device"]
            for c, us in got["us"].items():
                t[leg].setdefault(c, []).append(us)
            print(leg, json.dumps(got["us"]), flush=True)
    rows = []
    for c in t["batch"]:
        r = {k: {"min": round(min(t[k][c]), 2), "max": round(max(t[k][c]), 2),
                 "samples": [round(x, 2) for x in t[k][c]]} for k in LEGS}
        if r["batch"]["max"] < r["loop"]["min"]:
            verdict = "batch faster (ranges apart)"
        elif r["loop"]["max"] < r["batch"]["min"]:
            verdict = "batch slower (ranges apart)"
        else:
            verdict = "ranges overlap: no claim"
        rows.append({"config": c, "unit": "us per call (a crop from each of the n images)", **r,
                     "loop_over_batch": [round(r["loop"]["min"] / r["batch"]["max"], 2),
                                         round(r["loop"]["max"] / r["batch"]["min"], 2)], "verdict": verdict})
    out = {"workload": "random RGB encoded by one BatchEncoder (slot layout); fresh random origins per call; loop: n "
                       "RegionDecoder.decode + n copies into one tensor%s; batch: BatchRegionDecoder.decode; %d fresh "
                       "processes per leg, alternating; per process %d warm-up + 1 timed window of %d calls between "
                       "device events" % (" (the parent commit's library)" if a.parent_lib else "", a.pairs, a.warmup,
                                          a.steps),
           "device": dev, "configs": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "region_batch_ab.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
