"""The fillnodata golden cases (tests/golden/wide_fillnodata.npz, written by tools/gen_golden_fillnodata.py): rasters,
payload dtypes, nodata values and the deterministic payloads — integer hashing of the cell index, no random generator."""
from __future__ import annotations

import numpy as np

RASTERS = ["synth_tiny_5x7", "flwdir0", "flwdir1", "synth_loops_96x80", "synth_river_nodata_768x1024"]
GENERAL = ["flwdir0_nextxy", "flwdir0_ds2"]  # graphs of tests/golden/wide_general.npz
FULL = {"synth_tiny_5x7", "flwdir0", "flwdir1", "flwdir0_nextxy", "flwdir0_ds2"}  # outputs in full; the others: digests
DTYPES = ["int8", "int32", "uint32", "int64", "float32", "float64"]
NODATAS = [("m9999", -9999), ("zero", 0), ("nan", float("nan"))]
CALLS = [("up", "max"), ("down", "max"), ("down", "min"), ("down", "sum")]


def _hash(n, salt):
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt * 97531 + 12345)) % np.uint64(1 << 32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(2246822519)) % np.uint64(1 << 32)
    h ^= h >> np.uint64(16)
    return h


def payload(n, dtype, nodata, salt=0):
    """Payload of n cells: about 30 % nodata (when the dtype can hold it), small values whose running sums meet 0, and
    for int8 large values whose sums wrap; floats carry NaN, -0.0 and 0.0; uint32 values around 2**31 as well."""
    dt = np.dtype(dtype)
    h = _hash(n, salt)
    small = (h % np.uint64(7)).astype(np.int64) - 3
    if dt.kind == "f":
        v = ((h % np.uint64(2001)).astype(np.float64) - 1000.0) / 8.0
        sel = (h >> np.uint64(7)) % np.uint64(50)
        v[sel == 0] = np.nan
        v[sel == 1] = -0.0
        v[sel == 2] = 0.0
        v = v.astype(dt)
    else:
        big = ((h >> np.uint64(8)) % np.uint64(241)).astype(np.int64) - 120
        v = np.where((h >> np.uint64(20)) % np.uint64(4) == 0, big, small)
        if dt.kind == "u":
            v = np.abs(v) + np.where((h >> np.uint64(24)) % np.uint64(5) == 0, 1 << 31, 0)
        v = v.astype(dt)
    nd_cells = (h >> np.uint64(4)) % np.uint64(10) < 3
    if nodata == nodata:  # (not NaN)
        if dt.kind == "f" or np.iinfo(dt).min <= nodata <= np.iinfo(dt).max:
            v[nd_cells] = nodata
    return v


def key(raster, dtype, ndname, direction, how):
    return f"{raster}_{dtype}_{ndname}_{direction}_{how}"
