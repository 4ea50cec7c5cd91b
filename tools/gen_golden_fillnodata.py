"""Record tests/golden/wide_fillnodata.npz from the reference's FlwdirRaster.fillnodata (reference
pyflwdir/flwdir.py:360-392, core.py:120-188), imported as oracle/gen_golden_wide.py does (its shim, no numba JIT).
The cases and payloads are tests/fill_cases.py; small rasters keep their outputs in full, the others their digests
(tests/golden_util.digest).

    python tools/gen_golden_fillnodata.py /path/to/the/reference
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

import fill_cases as FC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def digest(a):  # (tests/golden_util.digest)
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(str(a.dtype.str).encode())
    h.update(str(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def rasters():
    for name in FC.RASTERS:
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        yield name, pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
    W = np.load(os.path.join(GOLD, "wide_general.npz"))
    nxy = W["in_flwdir0_nextxy"]
    yield "flwdir0_nextxy", pyflwdir.from_array(nxy, ftype="nextxy", cache=False)
    yield "flwdir0_ds2", pyflwdir.FlwdirRaster(idxs_ds=W["in_flwdir0_ds2"], shape=nxy.shape[1:], ftype="d8", cache=False)


def main():
    store = {}
    import warnings

    warnings.simplefilter("ignore")  # (integer sums that wrap: numpy's overflow warnings)
    for name, flw in rasters():
        for dt in FC.DTYPES:
            for ndname, nd in FC.NODATAS:
                data = FC.payload(flw.size, dt, nd).reshape(flw.shape)
                for direction, how in FC.CALLS:
                    out = flw.fillnodata(data, nd, direction=direction, how=how)
                    k = FC.key(name, dt, ndname, direction, how)
                    if name in FC.FULL:
                        store["out_" + k] = out
                    else:
                        store["digest_" + k] = np.array(digest(out))
        print(name, "done", flush=True)
    fn = os.path.join(GOLD, "wide_fillnodata.npz")
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
