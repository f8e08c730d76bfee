#!/usr/bin/env python3
"""A/B of the paths from an 8K RGB image to a HicImage and back, in one process:

  (a) Encoder.hic_image()                   compaction + the contiguous Huffman stage
  (b) Encoder.hic_image(from_slots=True)    the Huffman stage straight from the slots
  (c) codec.encode(host array)              one upload + the device-resident path
  (d) compression.encode(host array)        jpeg_compression + jpeg_encode through host planes
  (e) codec.decode(HicImage)
  (f) compression.decode(HicImage)          jpeg_decode + jpeg_decompression through host planes

Random 8K images, NIMG of them rotated (their RGB alone exceeds the 256 MiB
Infinity Cache); every leg runs once per round on the round's image, the legs of a
pair back to back and swapping places every round, WARMUP untimed rounds, then
ROUNDS timed ones.  (a) and (b) time hic_image() alone (the encode before it is synchronised first) and also report the
GPU-side time of their range + histogram + pack phases (compaction included for
(a)): device events around the serial launches and around each fanned-out phase --
the host tree building and the copy back of the bits are common to both legs.
(c) and (e) are also given as multiples of their PCIe floors (bench.py's formula
for 8k_reference_api: the call's bytes up / the pinned H2D rate + bytes down / the
pinned D2H rate).  Writes hic_path_ab.json under --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hiccup_amd import _lib, codec, compression, device, huffman, pipeline, settings  # noqa: E402

PHASE_CALLS = ("hic_rle_slots_compact", "hic_key_range", "hic_slot_key_range")


class PhaseTimer:
    """Device events around the Huffman stage's GPU phases while active: each serial
    launch of PHASE_CALLS, and each huffman._fan_out (histograms, packing) as a
    whole on the stream it joins back into."""

    def __init__(self):
        self.pairs, self.on = [], False
        self._call, self._fan = _lib.call, huffman._fan_out
        _lib.call = self.call
        huffman._fan_out = self.fan_out

    def _timed(self, f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        self.pairs.append((a, b))

    def call(self, name, *args):
        if self.on and name in PHASE_CALLS:
            self._timed(lambda: self._call(name, *args))
        else:
            self._call(name, *args)

    def fan_out(self, calls, stream=None):
        if self.on:
            self._timed(lambda: self._fan(calls, stream))
        else:
            self._fan(calls, stream)

    def run(self, f):
        """(f(), the phases' GPU milliseconds)."""
        self.pairs, self.on = [], True
        try:
            r = f()
        finally:
            self.on = False
        torch.cuda.synchronize()
        return r, sum(a.elapsed_time(b) for a, b in self.pairs)


def pinned_rates(nbytes=256 << 20, reps=4):
    h = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = {}
    for name, f in (("h2d_gbs", lambda: d.copy_(h, non_blocking=True)), ("d2h_gbs", lambda: h.copy_(d, non_blocking=True))):
        f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        out[name] = round(reps * nbytes / (time.perf_counter() - t) / 1e9, 1)
    return out


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = lambda p: round(float(np.percentile(v, p)), 3)  # noqa: E731
    return {"median": q(50), "p25": q(25), "p75": q(75), "min": q(0), "max": q(100), "n": int(v.size)}


def compare(slow, fast):
    """fast below slow by more than the spread of the timed regions: the medians'
    gap against the larger interquartile range (holds); the paired gaps (same image,
    back to back) are reported beside it."""
    s, f = stats(slow), stats(fast)
    gap = s["median"] - f["median"]
    spread = max(s["p75"] - s["p25"], f["p75"] - f["p25"])
    paired = np.asarray(slow) - np.asarray(fast)
    return {"gap_ms": round(gap, 3), "spread_ms": round(spread, 3), "paired_gap_median_ms": round(float(np.median(paired)), 3),
            "paired_gap_min_ms": round(float(paired.min()), 3), "holds": bool(gap > spread)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r07", "hic_path"))
    a = ap.parse_args()
    if a.rounds < 8:
        ap.error("at least 8 timed rounds")
    device.require_gpu()
    settings.DEBUG = False
    H, W = a.height, a.width
    rng = np.random.default_rng(7)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(a.images)]
    dev = [device.to_device(x) for x in host]
    enc = pipeline.Encoder(H, W)
    timer = PhaseTimer()
    hics, t = [None] * a.images, {k: [] for k in ("a", "b", "c", "d", "e", "f", "a_gpu", "b_gpu")}

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    for rnd in range(a.warmup + a.rounds):
        i = rnd % a.images
        keep = rnd >= a.warmup
        res = {}
        flip = rnd % 2 == 1  # the legs of a pair swap places every round
        for leg, kw in (("a", {}), ("b", {"from_slots": True}))[::-1 if flip else 1]:
            enc.encode(dev[i])
            (img, gpu_ms), ms = wall(lambda: timer.run(lambda: enc.hic_image(**kw)))
            res[leg] = (img, ms, gpu_ms)
        for leg, f in (("c", codec.encode), ("d", compression.encode))[::-1 if flip else 1]:
            res[leg] = wall(lambda: f(host[i]))
        if hics[i] is None:  # every leg's bytes, checked once per image
            want = res["d"][0].byte_stream()
            assert all(res[k][0].byte_stream() == want for k in "abc")
            hics[i] = res["d"][0]
        for leg, f in (("e", codec.decode), ("f", compression.decode))[::-1 if flip else 1]:
            res[leg] = wall(lambda: f(hics[i]))
        if rnd < a.images:
            assert np.array_equal(res["e"][0], res["f"][0])
        if keep:
            for k in "abcdef":
                t[k].append(res[k][1])
            t["a_gpu"].append(res["a"][2])
            t["b_gpu"].append(res["b"][2])
    rates = pinned_rates()
    px = H * W
    bits = sum(int(p.packed_bits()[0].size) for p in hics[0].payloads[9:18])
    floor = lambda up, down: up / rates["h2d_gbs"] / 1e6 + down / rates["d2h_gbs"] / 1e6  # noqa: E731
    f_enc, f_dec = floor(3 * px, bits), floor(bits, 3 * px)
    names = {"a": "hic_image()", "b": "hic_image(from_slots=True)", "c": "codec.encode(host)",
             "d": "compression.encode(host)", "e": "codec.decode", "f": "compression.decode",
             "a_gpu": "(a) GPU-side range + histogram + pack phases (with the compaction)",
             "b_gpu": "(b) GPU-side range + histogram + pack phases"}
    out = {"workload": "%dx%d random RGB, %d images rotated, %d warm-up + %d timed rounds, one process" %
                       (W, H, a.images, a.warmup, a.rounds),
           "device": torch.cuda.get_device_name(0), "unit": "ms",
           "legs": {k: dict(stats(v), what=names[k]) for k, v in t.items()},
           "b_below_a": compare(t["a"], t["b"]), "b_below_a_gpu_phases": compare(t["a_gpu"], t["b_gpu"]),
           "c_below_d": compare(t["d"], t["c"]), "e_below_f": compare(t["f"], t["e"]),
           "pcie": dict(rates, coded_bytes=bits,
                        codec_encode={"floor_ms": round(f_enc, 2), "ratio": round(stats(t["c"])["median"] / f_enc, 2)},
                        codec_decode={"floor_ms": round(f_dec, 2), "ratio": round(stats(t["e"])["median"] / f_dec, 2)})}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "hic_path_ab.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
