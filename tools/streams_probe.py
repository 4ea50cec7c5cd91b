"""tools/streams_probe.py [--size 10000] [--steps 5] [--warmup 2] [--commit TEXT] — pfd_streams (csrc/streams.hip) with the
mask and the three lists in device memory, warm: the median of ``steps`` calls after ``warmup`` calls, and the per-kernel
segments of one profiled call (pfd_last_timing).  The raster is the synthetic river raster made in HBM; the masks are
none, ``strahler >= 4`` (closed downstream) and ``strahler >= 3`` with every other 64 x 64 block knocked out (not
closed: the W sweep runs, and the walks pass through the gaps)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyflwdir_amd import _hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=10000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()


def last_timing(h, room=48):
    ms, ln = (C.c_double * room)(), (C.c_int64 * room)()
    names, k = C.create_string_buffer(2048), C.c_int(0)
    _hip.check(_hip.lib().pfd_last_timing(h._h, room, ms, ln, names, 2048, C.byref(k)))
    nm = names.value.decode().split(";") if k.value else []
    return [(nm[i], ms[i], int(ln[i])) for i in range(k.value)]


size = args.size
n = size * size
print(f"streams_probe: commit {args.commit}; {size} x {size} = {n / 1e6:.0f} Mcells; steps {args.steps} (median), "
      f"warmup {args.warmup}", flush=True)
_hip.reserve(min(64 * n, _hip.mem_info(0)["free"] // 2), 0)
buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
h = _hip.RasterHandle(buf, size, size, memspace=_hip.PFD_DEVICE)
strord = h.strahler().reshape(size, size)
blocks = (np.add.outer(np.arange(size) // 64, np.arange(size) // 64) & 1).astype(bool)
masks = [("none", None), ("strahler >= 4", strord >= 4), ("strahler >= 3 minus blocks (not closed)", (strord >= 3) & blocks)]
print(f"Strahler max {int(strord.max())}", flush=True)
for name, mask in masks:
    dmask = None
    if mask is not None:
        m8 = np.ascontiguousarray(mask.ravel()).view(np.uint8)
        dmask = _hip.DeviceBuffer(m8.nbytes).upload(m8)
    K, M = h.streams(dmask, np.int32, memspace=_hip.PFD_DEVICE)  # sizing call (also the first, cold, call)
    didx, doff, dpit = _hip.DeviceBuffer(4 * max(M, 1)), _hip.DeviceBuffer(8 * (K + 1)), _hip.DeviceBuffer(max(K, 1))

    def call():
        t0 = time.perf_counter()
        got = h.streams(dmask, np.int32, didx, doff, dpit, M, K, memspace=_hip.PFD_DEVICE)
        assert got == (K, M)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        call()
    ts = [call() for _ in range(args.steps)]
    lens = np.diff(doff.download(np.int64, (K + 1,)))
    print(f"mask {name}: {0 if mask is None else int(mask.sum())} mask cells, K = {K} segments, M = {M} indices, longest "
          f"{int(lens.max(initial=0))}, mean {M / max(K, 1):.1f}; pfd_streams {statistics.median(ts):.2f} ms "
          f"(min {min(ts):.2f}, max {max(ts):.2f})", flush=True)
    h.set_profiling(True)
    call()
    segs = last_timing(h)
    h.set_profiling(False)
    total = sum(ms for _, ms, _ in segs)
    walks = sum(ms for nm, ms, _ in segs if nm.startswith("streams_walk"))
    for nm, ms, ln in segs:
        print(f"    {nm:28s} {ms:9.3f} ms  {ln:5d} launches", flush=True)
    print(f"    kernel segments {total:.2f} ms; the two walks {walks:.2f} ms = {100 * walks / max(total, 1e-9):.0f} %", flush=True)
    for b in (dmask, didx, doff, dpit):
        if b is not None:
            b.free()
h.close()
buf.free()
_hip.check(_hip.lib().pfd_trim(0))
_hip.reserve(0, 0)
