"""tools/upscale_probe.py [--size 10000] [--reps 3] [--commit TEXT] — first timings of upscale (dmm, eam, eam_plus),
upscale_error and ucat_outlets on the N x N synthetic river raster made in HBM, at cellsize 10 and 100.  Host calls
(the upstream area goes up, the coarse lists come down); the arena is reserved first; one warm-up, then the median of
``reps`` runs with the host <-> device traffic per call, and the GPU milliseconds of the library call's kernels
(pfd_last_timing: the arg-max pass over the fine raster, the walks).  upscale() includes building the coarse
FlwdirRaster and its validity check."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pyflwdir_amd as pyflwdir  # noqa: E402
from pyflwdir_amd import _hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=10000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()


def timed(name, fn, note=lambda out: "", kernels=False):
    fn()  # warm-up
    _hip.transfer_stats(reset=True)
    ts, out = [], None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    tr = _hip.transfer_stats(reset=True)
    seg = "; kernels " + ", ".join(f"{s['name']} {s['ms']:.2f} ms" for s in flw._h.last_timing()) if kernels else ""
    print(f"  {name:34s} {statistics.median(ts) * 1e3:8.0f} ms per call (h2d {tr['h2d_bytes'] / args.reps / 1e9:.2f} GB "
          f"{tr['h2d_ms'] / args.reps:.0f} ms, d2h {tr['d2h_bytes'] / args.reps / 1e9:.2f} GB {tr['d2h_ms'] / args.reps:.0f} ms)"
          f"{note(out)}{seg}", flush=True)
    return out


size = args.size
n = size * size
print(f"upscale_probe: commit {args.commit}; {size} x {size} = {n / 1e6:.0f} Mcells; reps {args.reps} (median, after one warm-up)",
      flush=True)
_hip.reserve(min(64 * n, _hip.mem_info(0)["free"] // 2), 0)
buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
d8 = buf.download(np.uint8, (size, size))
buf.free()
flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
upa = flw.upstream_area()
flw._h.set_profiling(True)
print(f"  {flw.idxs_pit.size} pits; uparea int32 ({upa.nbytes / 1e9:.2f} GB per upload)", flush=True)
for cellsize in (10, 100):
    print(f" cellsize {cellsize}: {-(-size // cellsize)} x {-(-size // cellsize)} coarse cells", flush=True)
    for m in ("dmm", "eam_plus"):
        timed(f"ucat_outlets({m})", lambda: flw.ucat_outlets(cellsize, uparea=upa, method=m), kernels=True)
    for m in ("dmm", "eam", "eam_plus"):
        flw1, idxs_out = timed(f"upscale({m})", lambda: flw.upscale(cellsize, method=m, uparea=upa))
        timed(f"upscale_error({m})", lambda: flw.upscale_error(flw1, idxs_out), lambda o: f"; {int((o == 0).sum())} errors",
              kernels=True)
