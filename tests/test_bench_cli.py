"""bench.py's command line: a plain run prints the headline only, --full moves
everything else behind it, --dump-outputs writes the last timed encode's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BENCH = os.path.join(REPO, "bench.py")


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_options_default_off(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(["--full", "--dump-outputs", "x"], monkeypatch)
    assert a.full is True and a.dump_outputs == "x"


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    """One plain 4K run in a child process: the line holds the headline and none of
    the side measurements, value and ms_per_step describe the same K steps, and the
    dump is float32 / float64 arrays within 64 MB that agree with the line."""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "4", "--warmup", "1", "--workload", "4k",
                        "--dump-outputs", out], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    for k in ("roofline", "memory_floors", "extra_configs", "cpu_baseline", "ms_per_step_regions"):
        assert k not in d, k
    # both are rounded in the line (4 and 2 decimals)
    ms = d["ms_per_step"]
    assert ms > 0
    lo, hi = 4096 * 4096 / ((ms + 5e-5) * 1e-3) / 1e6, 4096 * 4096 / ((ms - 5e-5) * 1e-3) / 1e6
    assert lo - 0.01 <= d["value"] <= hi + 0.01
    names = sorted(os.listdir(out))
    want = ["counts.npy"] + ["%s_%s.npy" % (a, c) for a in ("dc", "index", "sym_len", "sym_val")
                             for c in ("cb", "cr", "lum")]
    assert names == sorted(want)
    arrs = {n[:-4]: np.load(os.path.join(out, n), allow_pickle=False) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    # (4 rotating encoders: step 1 + 4 - 1 ran on the encoder the line's symbol counts are read from)
    assert arrs["counts"].tolist() == [float(c) for c in d["config"]["symbols_per_image_rank0"]]
    for i, (c, nblk) in enumerate((("lum", 512 * 512), ("cr", 256 * 256), ("cb", 256 * 256))):
        assert arrs["dc_" + c].shape == (nblk,)
        n = min(int(arrs["counts"][i]), 1 << 20)
        assert arrs["sym_len_" + c].shape == arrs["sym_val_" + c].shape == (n,)
        ln = arrs["sym_len_" + c]
        assert ln.min() >= 0 and ln.max() <= 15 and np.array_equal(ln, np.round(ln))
        # the record index: n_r symbols in a record of 64 (Y) or 32 (Cr, Cb) blocks
        ix = arrs["index_" + c]
        assert ix.shape == (nblk // (64 if c == "lum" else 32), 4)
        assert ix[:, 0].min() >= 0 and ix[:, 0].max() <= 63 * (64 if c == "lum" else 32)
