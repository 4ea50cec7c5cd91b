"""Record tests/golden/wide_outlets.npz from the reference's FlwdirRaster.subbasins_streamorder, outflow_idxs and
basin_outlets (reference pyflwdir/pyflwdir.py:601-629, :820-835, :720-740; basins.py:67-103, core.py:501-514,
regions.py:129-163), imported as oracle/gen_golden_wide.py does (its shim, no numba JIT).  The cases are
tests/outlet_cases.py; small rasters keep their outputs in full, the others their digests (tests/golden_util.digest).

    python tools/gen_golden_outlets.py /path/to/the/reference
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

import pyflwdir  # noqa: E402  (the reference)

import outlet_cases as OC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def digest(a):  # (tests/golden_util.digest)
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(str(a.dtype.str).encode())
    h.update(str(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def rasters():
    for name in OC.RASTERS:
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        yield name, pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
    W = np.load(os.path.join(GOLD, "wide_general.npz"))
    nxy = W["in_flwdir0_nextxy"]
    yield "flwdir0_nextxy", pyflwdir.from_array(nxy, ftype="nextxy", cache=False)
    yield "flwdir0_ds2", pyflwdir.FlwdirRaster(idxs_ds=W["in_flwdir0_ds2"], shape=nxy.shape[1:], ftype="d8", cache=False)


def main():
    store = {}
    for name, flw in rasters():
        cache = {}
        for key, call, arg in OC.keys(name):
            outs = OC.run(flw, call, arg, cache)
            if call == "sto_strahler":
                want = OC.KNOWN_COUNTS.get(name, {}).get(arg)
                assert want is None or outs[1].size == want, (key, outs[1].size, want)
                assert int(outs[0].max(initial=0)) == outs[1].size and (outs[1].size or not outs[0].any()), key
            if call.startswith("outlets_"):  # (one outlet per label: np.argsort's order among equal labels plays no part)
                assert np.unique(outs[0]).size == outs[0].size, key
            for i, o in enumerate(outs):
                o = np.asarray(o)
                if name in OC.FULL:
                    store[f"out_{key}_{i}"] = o
                else:
                    store[f"digest_{key}_{i}"] = np.array(digest(o))
            store[f"count_{key}"] = np.array(np.asarray(outs[-1]).size, np.int64)
        if name in OC.KNOWN_STRAHLER_MAX:
            assert int(cache["strahler"].max()) == OC.KNOWN_STRAHLER_MAX[name], name
        print(name, "done", flush=True)
    fn = os.path.join(GOLD, "wide_outlets.npz")
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
