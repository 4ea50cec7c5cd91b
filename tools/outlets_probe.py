"""tools/outlets_probe.py [--sizes 10000,30000] [--reps 5] [--commit TEXT] — subbasins_streamorder on the device against
what a user did before it existed: ``flw.idxs_seq``, ``flw.idxs_ds`` and the stream order to numpy, the mark and the
numbering in numpy, the outlets back through ``flw.basins(idxs=, ids=)``.  Synthetic river rasters made in HBM,
``min_sto`` -2 and 2; the arena is reserved first, every step has one warm-up and reports the median of ``reps`` runs, and
the two paths must return the same bytes.  Both paths start from the same host stream order (its cost is printed, and is
common to both); ``idxs_seq`` / ``idxs_ds`` are exports a user keeps per raster, so the host path is given with and
without them."""
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
ap.add_argument("--sizes", default="10000,30000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()


def timed(fn, reps):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


print(f"outlets_probe: commit {args.commit}; reps {args.reps} (median, after one warm-up)", flush=True)
for size in [int(s) for s in args.sizes.split(",")]:
    n = size * size
    _hip.reserve(min(64 * n, _hip.mem_info(0)["free"] // 2), 0)
    buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
    d8 = buf.download(np.uint8, (size, size))
    buf.free()
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    t_sto, strord = timed(lambda: flw.stream_order(), args.reps)
    print(f"{size} x {size} = {n / 1e6:.0f} Mcells, Strahler max {int(strord.max())}; stream_order() to the host "
          f"{t_sto * 1e3:.0f} ms (common to both paths)", flush=True)

    def export_seq():
        flw._seq = None
        return flw.idxs_seq

    def export_ds():
        flw._idxs_ds = None
        return flw.idxs_ds

    t_seq, seq = timed(export_seq, args.reps)
    t_ds, ds = timed(export_ds, args.reps)
    print(f"  host path, per raster: idxs_seq {t_seq * 1e3:.0f} ms ({seq.nbytes / 1e9:.2f} GB D2H), idxs_ds {t_ds * 1e3:.0f} ms "
          f"({ds.nbytes / 1e9:.2f} GB D2H)", flush=True)
    flat = strord.ravel()
    for min_sto in (-2, 2):
        def host_mark():
            m = int(flat.max()) + min_sto if min_sto < 0 else min_sto
            rev = seq[::-1]
            s = flat[rev]
            sel = np.flatnonzero(s >= m)  # (the cells of high enough order first: the gathers below touch only those)
            cells = rev[sel]
            down = ds[cells]
            return cells[(down == cells) | (flat[down] != s[sel])]

        t_np, idxs = timed(host_mark, args.reps)
        t_bas, sub = timed(lambda: flw.basins(idxs=idxs, ids=np.arange(1, idxs.size + 1, dtype=np.int32)), args.reps)
        _hip.transfer_stats(reset=True)
        t_dev, (dsub, didxs) = timed(lambda: flw.subbasins_streamorder(strord=strord, min_sto=min_sto), args.reps)
        tr = _hip.transfer_stats(reset=True)
        calls = args.reps + 1
        assert dsub.dtype == sub.dtype and dsub.tobytes() == sub.tobytes(), "maps differ"
        assert didxs.dtype == idxs.dtype and didxs.tobytes() == idxs.tobytes(), "outlet lists differ"
        host_call, host_all = t_np + t_bas, t_np + t_bas + t_seq + t_ds
        print(f"  min_sto {min_sto:2d}: {idxs.size} outlets | host: numpy mark {t_np * 1e3:.0f} ms + basins() {t_bas * 1e3:.0f} ms = "
              f"{host_call * 1e3:.0f} ms per call, {host_all * 1e3:.0f} ms with the two exports | device: "
              f"{t_dev * 1e3:.0f} ms per call (h2d {tr['h2d_bytes'] / calls / 1e9:.2f} GB {tr['h2d_ms'] / calls:.0f} ms, "
              f"d2h {tr['d2h_bytes'] / calls / 1e9:.2f} GB {tr['d2h_ms'] / calls:.0f} ms) | device / host per call "
              f"{t_dev / host_call:.2f}, with exports {t_dev / host_all:.2f}; results equal", flush=True)
    del flw, seq, ds, strord, d8
    _hip.check(_hip.lib().pfd_trim(0))
    _hip.reserve(0, 0)
