"""Record tests/golden/wide_upscale.npz from the reference's FlwdirRaster.upscale (methods dmm, eam, eam_plus), upscale_error
and ucat_outlets (reference pyflwdir/pyflwdir.py:1013-1157, upscale.py, subgrid.py:13-48), imported as
tools/gen_golden_basins.py does (the oracle's shim, no numba JIT).  The cases are tests/upscale_cases.py; small rasters
keep their outputs in full, the others their digests (tests/golden_util.digest).  Per case and method the record holds
the coarse idxs_ds, the fine idxs_out, the upscale_error map, its number of zeros (``nerr_``), the number of coarse links
outside the 8 neighbours (``far_``), and ``raises_`` where the reference refuses the upscaled network; per case the
ucat_outlets of both of its methods; per raster and area kind the digest of the upstream area the case was run with.

    python tools/gen_golden_upscale.py /path/to/the/reference
"""
from __future__ import annotations

import hashlib
import os
import sys

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

import upscale_cases as UC  # noqa: E402
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


def main():
    store, flws, caches = {}, {}, {}

    def keep(raster, name, a):
        a = np.asarray(a)
        if raster in UC.FULL:
            store[f"out_{name}"] = a
        else:
            store[f"digest_{name}"] = np.array(digest(a))

    for key, raster, kind, cellsize in UC.keys():
        if raster not in flws:
            tr, latlon = UC.transform_of(raster)
            flws[raster] = pyflwdir.from_array(UC.d8_of(raster), ftype="d8", check_ftype=False, transform=Affine(*tr),
                                               latlon=latlon, cache=False)
            caches[raster] = {}
        flw = flws[raster]
        upa = UC.uparea_of(flw, kind, caches[raster])
        store[f"upa_{raster}_{kind}"] = np.array(digest(upa))
        for m in UC.METHODS:
            try:
                flw1, idxs_out = flw.upscale(cellsize, method=m, uparea=upa)
            except ValueError as e:
                store[f"raises_{key}_{m}"] = np.array(str(e))
                continue
            err = flw.upscale_error(flw1, idxs_out)
            assert flw1.idxs_ds.dtype == flw.idxs_ds.dtype
            keep(raster, f"{key}_{m}_ds", flw1.idxs_ds)
            keep(raster, f"{key}_{m}_idxs", idxs_out)
            keep(raster, f"{key}_{m}_err", err)
            store[f"nerr_{key}_{m}"] = np.array(int(np.count_nonzero(err == 0)))
            store[f"far_{key}_{m}"] = np.array(UC.far_links(flw1.idxs_ds, flw1.shape, flw._mv))
        for m in ("eam_plus", "dmm"):
            keep(raster, f"{key}_{m}_ucat", flw.ucat_outlets(cellsize, uparea=upa, method=m))
        print(key, "done", {m: int(store[f"nerr_{key}_{m}"]) for m in UC.METHODS if f"nerr_{key}_{m}" in store},
              {m: int(store[f"far_{key}_{m}"]) for m in UC.METHODS if f"far_{key}_{m}" in store},
              [m for m in UC.METHODS if f"raises_{key}_{m}" in store], flush=True)
    fn = os.path.join(GOLD, "wide_upscale.npz")
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
