"""tools/window_probe.py [--size 10000] [--reps 3] [--commit TEXT] — first, untuned timings of downstream, moving_average
and moving_median on the N x N synthetic river raster made in HBM: ``moving_average`` at n = 5, ``moving_median`` at n = 5
(windows of 11 cells, sorted in LDS) and at one n beyond WMAX (sorted in the global workspace, which serves the raster in
chunks).  Warm host calls on a handle with ``cache=True`` (the main upstream cells are derived once, before the timing;
every call uploads them again with its own per-cell inputs); the arena is reserved first; one warm-up, then the median of
``reps`` runs.  Per call: the wall time, the upload and download (bytes and milliseconds, pfd_transfer_stats) and,
separately, the GPU milliseconds of the library call's kernels (pfd_last_timing)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pyflwdir_amd as pyflwdir  # noqa: E402
from pyflwdir_amd import _hip  # noqa: E402
from pyflwdir_amd._affine import Affine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=10000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--commit", default=None, help="names the build in the first line (default: git rev-parse of the tree)")
args = ap.parse_args()
if args.commit is None:
    import subprocess

    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        args.commit = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True,
                                              stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        args.commit = "unknown"


def timed(name, fn):
    fn()  # warm-up
    _hip.transfer_stats(reset=True)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    tr = _hip.transfer_stats(reset=True)
    segs = flw._h.last_timing()
    gpu = sum(s["ms"] for s in segs)
    print(f"  {name:34s} {statistics.median(ts) * 1e3:8.0f} ms per call; upload {tr['h2d_bytes'] / args.reps / 1e9:.2f} GB "
          f"{tr['h2d_ms'] / args.reps:.0f} ms, download {tr['d2h_ms'] / args.reps:.0f} ms; GPU {gpu:.2f} ms ("
          + ", ".join(f"{s['name']} {s['ms']:.2f} in {s['launches']} launch(es)" for s in segs) + ")", flush=True)


size = args.size
n = size * size
wmax32, wmax64 = _hip.window_wmax(np.float32), _hip.window_wmax(np.float64)
beyond = wmax32 // 2 + 5
print(f"window_probe: commit {args.commit}; {size} x {size} = {n / 1e6:.0f} Mcells; reps {args.reps} (median, after one "
      f"warm-up); WMAX {wmax32} (float32) / {wmax64} (float64)", flush=True)
_hip.reserve(min(64 * n, _hip.mem_info(0)["free"] // 2), 0)
buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
d8 = buf.download(np.uint8, (size, size))
buf.free()
flw = pyflwdir.from_array(d8, ftype="d8", cache=True, latlon=False, transform=Affine(90.0, 0.0, 0.0, 0.0, -90.0, 0.0))
rng = np.random.default_rng(0)
data = rng.random((size, size), dtype=np.float32) * 99 + 1
data64 = data.astype(np.float64)
flw.idxs_us_main  # (derived once, kept by cache=True)
flw._h.set_profiling(True)
print(f"  {flw.idxs_pit.size} pits; per-cell inputs float32 / {flw.idxs_ds.dtype} ({4 * n / 1e9:.2f} GB each per upload)", flush=True)
timed("downstream (float32)", lambda: flw.downstream(data))
timed("moving_average n=5 (float32)", lambda: flw.moving_average(data, 5))
timed("moving_median n=5 (float32, LDS)", lambda: flw.moving_median(data, 5))
timed("moving_median n=5 (float64, LDS)", lambda: flw.moving_median(data64, 5))
timed(f"moving_median n={beyond} (float32, workspace)", lambda: flw.moving_median(data, beyond))
