"""tools/basins_probe.py [--size 10000] [--reps 3] [--commit TEXT] — first timings of interbasin_mask, inflow_idxs,
basin_bounds and subbasins_pfafstetter on the N x N synthetic river raster made in HBM, next to outflow_idxs on the same
handle for scale.  Host calls (inputs up, results down); the arena is reserved first; one warm-up, then the median of
``reps`` runs, with the host <-> device traffic per call.  The region is the centred rectangle of half the rows and
columns, the stream mask upstream_area > 1000 cells, the basin map ``basins()``; Pfafstetter at depth 1, 2 and 3 on the
upstream cell count with upa_min 1000."""
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


def timed(name, fn, note=lambda out: ""):
    fn()  # warm-up
    _hip.transfer_stats(reset=True)
    ts, out = [], None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    tr = _hip.transfer_stats(reset=True)
    print(f"  {name:34s} {statistics.median(ts) * 1e3:8.0f} ms per call (h2d {tr['h2d_bytes'] / args.reps / 1e9:.2f} GB "
          f"{tr['h2d_ms'] / args.reps:.0f} ms, d2h {tr['d2h_bytes'] / args.reps / 1e9:.2f} GB {tr['d2h_ms'] / args.reps:.0f} ms)"
          f"{note(out)}", flush=True)
    return out


size = args.size
n = size * size
print(f"basins_probe: commit {args.commit}; {size} x {size} = {n / 1e6:.0f} Mcells; reps {args.reps} (median, after one warm-up)",
      flush=True)
_hip.reserve(min(64 * n, _hip.mem_info(0)["free"] // 2), 0)
buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
d8 = buf.download(np.uint8, (size, size))
buf.free()
flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
region = np.zeros((size, size), bool)
region[size // 4:size - size // 4, size // 4:size - size // 4] = True
upa = flw.upstream_area()
stream = upa > 1000
basins = flw.basins()
print(f"  {flw.idxs_pit.size} pits, {int(stream.sum())} stream cells", flush=True)
timed("outflow_idxs (for scale)", lambda: flw.outflow_idxs(region), lambda o: f"; {o.size} cells")
timed("interbasin_mask(region)", lambda: flw.interbasin_mask(region), lambda o: f"; {int(o.sum())} cells")
timed("interbasin_mask(region, stream)", lambda: flw.interbasin_mask(region, stream=stream), lambda o: f"; {int(o.sum())} cells")
timed("inflow_idxs(region)", lambda: flw.inflow_idxs(region), lambda o: f"; {o.size} cells")
timed("basin_bounds(basins)", lambda: flw.basin_bounds(basins), lambda o: f"; {o[0].size} labels")
for depth in (1, 2, 3):
    timed(f"subbasins_pfafstetter(depth={depth})", lambda: flw.subbasins_pfafstetter(depth=depth, uparea=upa, upa_min=1000),
          lambda o: f"; {o[1].size} outlets")
