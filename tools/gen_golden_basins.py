"""Record tests/golden/wide_basins.npz from the reference's FlwdirRaster.interbasin_mask, inflow_idxs, basin_bounds and
subbasins_pfafstetter (reference pyflwdir/pyflwdir.py:742-766, :804-818, :694-718, :631-663; basins.py:25-64, core.py:
485-497, regions.py:57-125, basins.py:106-191), imported as oracle/gen_golden_wide.py does (its shim, no numba JIT).
The cases are tests/basin_cases.py (the golden rasters and one raster built there); small rasters keep their outputs in full, the others their digests
(tests/golden_util.digest).  basin_bounds needs scipy.ndimage.find_objects: where scipy is not importable the slices come
from numpy (basin_cases.label_slices), which is then what the record holds.

A Pfafstetter case with a tie among the sort keys that decide which tributaries are taken, or their order
(basin_cases.pfaf_ties), is NOT recorded: the reference sorts unstably there, and only a case without such a tie is
decided by the reference alone.  Every depth must keep at least one case.

    python tools/gen_golden_basins.py /path/to/the/reference
"""
from __future__ import annotations

import hashlib
import os
import sys
import types

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

import basin_cases as BC  # noqa: E402

try:
    import scipy.ndimage  # noqa: F401,E402
except ImportError:  # find_objects with numpy: a list with one entry per label value 1 .. max, None where it is absent
    def _find_objects(regions):
        lbs, slices = BC.label_slices(regions)
        out = [None] * (int(lbs.max()) if lbs.size else 0)
        for l, s in zip(lbs.tolist(), slices):
            out[l - 1] = s
        return out

    scipy = types.ModuleType("scipy")
    scipy.ndimage = types.ModuleType("scipy.ndimage")
    scipy.ndimage.find_objects = _find_objects
    sys.modules["scipy"], sys.modules["scipy.ndimage"] = scipy, scipy.ndimage

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
    store, kept = {}, {d: 0 for d in BC.DEPTHS}
    for name in BC.RASTERS:
        d8 = BC.d8_of(name)
        flws, cache = {}, {}
        for kind in BC.TRANSFORMS:
            tr, latlon = BC.transform_of(name, kind)
            flws[kind] = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, transform=Affine(*tr), latlon=latlon, cache=False)
        for key, call, args in BC.keys(name):
            flw = flws[args[1]] if call == "bounds" else flws["own"]
            if call == "pfaf":
                uparea, upa_min = BC.pfaf_args(flw, cache, args[1], args[2])
                upa = cache[args[1]].ravel()
                tie = BC.pfaf_ties(flw.idxs_pit, flw.idxs_ds, flw.idxs_seq, flw.idxs_us_main, upa, upa >= upa_min, args[0])
                store[f"tie_{key}"] = np.array(bool(tie))
                if tie:
                    continue
                kept[args[0]] += 1
            outs = BC.run(flw, call, args, cache)
            for i, o in enumerate(outs):
                o = np.asarray(o)
                if name in BC.FULL:
                    store[f"out_{key}_{i}"] = o
                else:
                    store[f"digest_{key}_{i}"] = np.array(digest(o))
        print(name, "done", flush=True)
    assert all(kept.values()), f"a depth kept no tie-free Pfafstetter case: {kept}"
    fn = os.path.join(GOLD, "wide_basins.npz")
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes; tie-free Pfafstetter cases per depth:", kept)


if __name__ == "__main__":
    main()
