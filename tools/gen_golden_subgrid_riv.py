"""Record tests/golden/wide_subgrid_riv.npz from the reference's FlwdirRaster.ucat_volume, subgrid_rivlen, subgrid_rivslp
(method "mean") and subgrid_rivavg (reference pyflwdir/pyflwdir.py:1193-1398) and from subgrid.segment_median
(pyflwdir/subgrid.py:277-337; the reference's subgrid_rivmed itself raises TypeError: it passes ``weights=`` on), imported
as tools/gen_golden_upscale.py does (the oracle's shim, no numba JIT).  The cases are tests/subgrid_riv_cases.py; the
small raster keeps its outputs in full, the others their digests (tests/golden_util.digest, every NaN made the same NaN
first).  Per configuration the record holds the outlets (the reference's ucat_outlets), the unit catchment map and every
call's result; per raster and grid the digests of the inputs the reference derived itself: main upstream cells, distances
to the outlet in metres and cells, cell areas per row.

    python tools/gen_golden_subgrid_riv.py /path/to/the/reference
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

import subgrid_riv_cases as SC  # noqa: E402
import pyflwdir  # noqa: E402  (the reference)
from pyflwdir import subgrid  # noqa: E402
from affine import Affine  # noqa: E402  (the shim's)

GOLD = os.path.join(ROOT, "tests", "golden")


def digest(a):  # (tests/golden_util.digest)
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(str(a.dtype.str).encode())
    h.update(str(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def call(flw, method, idxs_out, inp, kw):
    kw = dict(kw)
    for name in ("mask", "elevtn", "data", "weights", "hand"):
        if name in kw:
            kw[name] = inp[kw[name]].reshape(flw.shape) if name != "weights" else inp[kw[name]]
    if method == "rivlen":
        return flw.subgrid_rivlen(idxs_out, **kw)
    if method == "rivslp":
        return flw.subgrid_rivslp(idxs_out, method="mean", **kw)
    if method == "rivavg":
        return flw.subgrid_rivavg(idxs_out, **kw)
    if method == "rivmed":
        shape = flw.shape if idxs_out is None else idxs_out.shape
        flat = np.arange(flw.size, dtype=np.intp) if idxs_out is None else idxs_out.ravel()
        mask = kw.get("mask")
        res = subgrid.segment_median(idxs_out=flat, idxs_nxt=flw.idxs_ds if kw["direction"] == "down" else flw.idxs_us_main,
                                     data=kw["data"].ravel(), mask=None if mask is None else mask.ravel(), nodata=SC.NODATA,
                                     mv=flw._mv)
        return res.reshape(shape)
    if method == "volume":
        return flw.ucat_volume(idxs_out, kw["hand"], depths=SC.depths_of(kw["depths"]))
    raise ValueError(method)


def main():
    store, flws = {}, {}
    warnings.simplefilter("ignore", RuntimeWarning)  # (All-NaN slices, 0 / 0 of a flat segment)
    for key, raster, grid, cellsize, variant in SC.configs():
        if (raster, grid) not in flws:
            tr, latlon = SC.transform_of(raster, grid)
            flw = pyflwdir.from_array(SC.d8_of(raster), ftype="d8", check_ftype=False, transform=Affine(*tr), latlon=latlon,
                                      cache=True)
            flws[raster, grid] = flw
            store[f"mv_{raster}"] = np.array(flw._mv).astype(flw.idxs_ds.dtype)  # (the missing value in the index dtype)
            store[f"usmain_{raster}"] = np.array(digest(flw.idxs_us_main))
            store[f"distcell_{raster}"] = np.array(digest(flw.stream_distance(unit="cell")))
            store[f"distnc_{raster}_{grid}"] = np.array(digest(flw.distnc))
            store[f"area_{raster}_{grid}"] = np.array(digest(np.ascontiguousarray(flw.area[:, 0])))
        flw = flws[raster, grid]
        inp = SC.inputs(flw.size)
        if variant == "none":
            idxs_out = None
        else:
            idxs_out = flw.ucat_outlets(cellsize)
            idxs_out = SC.variant_outlets(idxs_out, variant, flw._mv)
            store[f"outlets_{key}"] = idxs_out

        def keep(name, a):
            a = SC.canon(a)
            if raster in SC.FULL:
                store[f"out_{key}_{name}"] = a
            else:
                store[f"digest_{key}_{name}"] = np.array(digest(a))

        for name, method, kw in SC.calls(variant):
            res = call(flw, method, idxs_out, inp, kw)
            if method == "volume":
                keep("ucatmap", res[0])
                res = res[1]
            keep(name, res)
            store[f"nan_{key}_{name}"] = np.array(int(np.count_nonzero(np.isnan(res))))
        print(key, "done", flush=True)
    fn = os.path.join(GOLD, SC.RECORD)
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
