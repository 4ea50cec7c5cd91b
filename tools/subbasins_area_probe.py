"""tools/subbasins_area_probe.py [--size 10000] [--reps 3] [--commit TEXT] — first timings of subbasins_area on the N x N
synthetic river raster made in HBM, next to subbasins_pfafstetter at depth 1 on the same handle (the nearest existing
call).  Host calls (areas up, map and list down); the arena is reserved first; one warm-up, then the median of ``reps``
runs.  The areas are the upstream cell count (int32); two thresholds, chosen for about 10^3 and about 10^5 outlets at the
default size.  Per threshold: the call, the GPU time of its parts (HIP events: sequence, closure check, rounds, compaction,
fill), the mode, the rounds, the jobs and the lane steps."""
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

PARTS = {"idxs_seq_exact_order": "sequence", "subarea_import": "import", "subarea_closure": "closure check",
         "subarea_rounds": "rounds", "subarea_list": "compaction"}  # (what follows the compaction is the label fill)


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
print(f"subbasins_area_probe: commit {args.commit}; {size} x {size} = {n / 1e6:.0f} Mcells; reps {args.reps} (median, after one "
      "warm-up)", flush=True)
_hip.reserve(min(64 * n, _hip.mem_info(0)["free"] // 2), 0)
buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
d8 = buf.download(np.uint8, (size, size))
buf.free()
flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
upa = flw.upstream_area()
print(f"  {flw.idxs_pit.size} pits, {flw.idxs_seq.size} cells in the sequence", flush=True)
timed("subbasins_pfafstetter(depth=1)", lambda: flw.subbasins_pfafstetter(depth=1, uparea=upa, upa_min=1000),
      lambda o: f"; {o[1].size} outlets")
flat = np.ascontiguousarray(upa.ravel())
for area_min in (n // 1000, n // 100000):
    timed(f"subbasins_area({area_min})", lambda: flw.subbasins_area(area_min, uparea=upa), lambda o: f"; {o[1].size} outlets")
    flw._h.set_profiling(True)
    _, idxs, st = flw._h.subbasins_area(flat, _hip.PFD_I32, area_min, _hip.PFD_COMPARE_OWN, None, flw._idx_dtype)
    segs = flw._h.last_timing()
    flw._h.set_profiling(False)
    parts, after_list = {}, False
    for s in segs:
        part = PARTS.get(s["name"], "fill" if after_list else "sequence")
        after_list = after_list or s["name"] == "subarea_list"
        parts[part] = parts.get(part, 0.0) + s["ms"]
    print("    GPU ms: " + ", ".join(f"{k} {v:.1f}" for k, v in parts.items()), flush=True)
    print("    segments: " + ", ".join(f"{s['name']} {s['ms']:.1f} ms / {s['launches']} launches" for s in segs), flush=True)
    print(f"    mode {'full' if st[0] else 'pruned'}, {st[1]} rounds, {st[2]} jobs, {st[3]} lane steps, {idxs.size} outlets",
          flush=True)
