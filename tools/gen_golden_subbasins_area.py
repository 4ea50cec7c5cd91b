"""Record tests/golden/wide_subbasins_area.npz from the reference's FlwdirRaster.subbasins_area (reference pyflwdir/
pyflwdir.py:665-692, basins.py:194-233), imported as tools/gen_golden_basins.py does (the oracle's shim, no numba JIT:
the interpreted loop, whose comparisons with ``area_min`` follow numpy's promotion rules).  The cases are
tests/subbasins_area_cases.py; small rasters keep their outputs in full, the others their digests
(tests/golden_util.digest).  The reference has no unspecified sort in this call: every case is recorded.

    python tools/gen_golden_subbasins_area.py /path/to/the/reference
"""
from __future__ import annotations

import hashlib
import io
import os
import sys
import zipfile

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
import subbasins_area_cases as SC  # noqa: E402

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
    store = {}
    for name in SC.RASTERS:
        d8 = BC.d8_of(name)
        made = {}

        def make_flw(kind, cache):
            if (kind, cache) not in made:
                tr, latlon = BC.transform_of(name, kind)
                made[kind, cache] = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, transform=Affine(*tr), latlon=latlon,
                                                        cache=cache)
            return made[kind, cache]

        src = SC.FromFlw({kind: make_flw(kind, False) for kind in ("own", "south")})
        for key, spec in SC.keys(name):
            for i, o in enumerate(SC.run(make_flw, spec, src)):
                o = np.asarray(o)
                if name in SC.FULL:
                    store[f"out_{key}_{i}"] = o
                else:
                    store[f"digest_{key}_{i}"] = np.array(digest(o))
        print(name, "done", flush=True)
    fn = os.path.join(GOLD, "wide_subbasins_area.npz")
    # an .npz with fixed entry times (np.savez_compressed stamps the clock): the record regenerates byte for byte
    with zipfile.ZipFile(fn, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
