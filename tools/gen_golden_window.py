"""Record tests/golden/wide_window.npz from the reference's FlwdirRaster.downstream, moving_average, moving_median
(reference pyflwdir/flwdir.py:394-410, :435-504) and path (pyflwdir/pyflwdir.py:443-500), imported as
tools/gen_golden_subgrid_riv.py does (the oracle's shim, no numba JIT).  The cases are tests/window_cases.py; the small
raster keeps its outputs in full, the others their digests (tests/golden_util.digest, every NaN made the same NaN first).
Per raster the record holds the missing value in the index dtype, the digests of the main upstream cells and of the
Strahler order the reference derived itself, and the start cells of the paths; per raster and grid every path call as
(cells of all paths, lengths, distances).

    python tools/gen_golden_window.py /path/to/the/reference
"""
from __future__ import annotations

import hashlib
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PYFLWDIR_REFERENCE", "")
sys.path[:] = [q for q in sys.path if os.path.abspath(q or ".") != HERE]
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["NUMBA_DISABLE_JIT"] = "1"

import window_cases as WC  # noqa: E402
import pyflwdir  # noqa: E402  (the reference)
from affine import Affine  # noqa: E402  (the shim's)

GOLD = os.path.join(ROOT, "tests", "golden")


def digest(a):  # (tests/golden_util.digest)
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(str(a.dtype.str).encode())
    h.update(str(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def window_call(flw, method, inp, kw, strord):
    kw = dict(kw)
    data = inp[kw.pop("data")].reshape(flw.shape)
    if method == "downstream":
        return flw.downstream(data)
    if "weights" in kw:
        kw["weights"] = inp[kw["weights"]].reshape(flw.shape)
    if kw.get("strord") == "given":
        kw["strord"] = strord
    if method == "average":
        return flw.moving_average(data, **kw)
    return flw.moving_median(data, **kw)


def main():
    store = {}
    warnings.simplefilter("ignore", RuntimeWarning)  # (All-NaN slices)
    for raster in WC.RASTERS:
        for grid in WC.GRIDS:
            tr, latlon = WC.transform_of(raster, grid)
            flw = pyflwdir.from_array(WC.d8_of(raster), ftype="d8", check_ftype=False, transform=Affine(*tr), latlon=latlon,
                                      cache=True)
            inp = WC.inputs(flw.size)

            def keep(name, a, full=raster in WC.FULL):
                a = WC.canon(a)
                if full:
                    store[f"out_{name}"] = a
                else:
                    store[f"digest_{name}"] = np.array(digest(a))

            if grid == WC.GRIDS[0]:
                strord = flw.stream_order()
                store[f"mv_{raster}"] = np.array(flw._mv).astype(flw.idxs_ds.dtype)
                store[f"usmain_{raster}"] = np.array(digest(flw.idxs_us_main))
                store[f"strord_{raster}"] = np.array(digest(strord))
                store[f"starts_{raster}"] = WC.path_starts(flw.idxs_ds, flw.idxs_us_main, flw._mv, inp["mask"])
                for name, method, kw in WC.window_calls(raster):
                    res = window_call(flw, method, inp, kw, strord)
                    assert res.shape == flw.shape
                    keep(f"{raster}_{name}", res)
                    if res.dtype.kind == "f":
                        store[f"nan_{raster}_{name}"] = np.array(int(np.count_nonzero(np.isnan(res))))
                    print(raster, name, "done", flush=True)
            starts = store[f"starts_{raster}"].astype(flw.idxs_ds.dtype if flw.idxs_ds.dtype.kind == "i" else np.int64)
            for name, kw in WC.path_calls(raster, grid):
                kw = dict(kw)
                if "mask" in kw:
                    kw["mask"] = inp[kw["mask"]].reshape(flw.shape)
                paths, dists = flw.path(idxs=starts, **kw)
                assert all(p.dtype == flw.idxs_ds.dtype for p in paths) and dists.dtype == np.float64
                cells, lens = WC.flat_paths(list(paths), flw.idxs_ds.dtype)
                keep(f"{raster}_{grid}_path_{name}_cells", cells)
                keep(f"{raster}_{grid}_path_{name}_lens", lens)
                keep(f"{raster}_{grid}_path_{name}_dists", dists)
            print(raster, grid, "paths done", flush=True)
    fn = os.path.join(GOLD, WC.RECORD)
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
