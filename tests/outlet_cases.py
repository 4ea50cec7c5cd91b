"""The outlet golden cases (tests/golden/wide_outlets.npz, written by tools/gen_golden_outlets.py): rasters, the
``min_sto`` values of ``subbasins_streamorder``, the two region masks of ``outflow_idxs`` and the keys of the records —
shared by the generator (which runs the reference) and tests/test_gpu_outlets.py (which runs the device)."""
from __future__ import annotations

import numpy as np

RASTERS = ["flwdir0", "flwdir1", "rhine", "synth_tiny_5x7", "synth_river_256", "synth_loops_96x80",
           "synth_rough_nodata_384x512", "synth_river_nodata_768x1024"]
GENERAL = ["flwdir0_nextxy", "flwdir0_ds2"]  # graphs of tests/golden/wide_general.npz
FULL = {"flwdir0", "flwdir1", "synth_tiny_5x7", "flwdir0_nextxy", "flwdir0_ds2"}  # outputs in full; the others: digests
MIN_STO = [-2, 1, 2, 4]
REGIONS = ["rect", "blob"]
# what the reference gives (checked by the generator and by tests/test_outlets_static.py): raster -> {min_sto: outlets}
KNOWN_COUNTS = {"rhine": {-2: 18, 4: 1535}, "synth_river_nodata_768x1024": {-2: 99, 4: 1803}, "flwdir1": {4: 0},
                "synth_tiny_5x7": {-2: 28}}
KNOWN_STRAHLER_MAX = {"rhine": 9}


def _hash(n, salt):
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt * 97531 + 12345)) % np.uint64(1 << 32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(2246822519)) % np.uint64(1 << 32)
    h ^= h >> np.uint64(16)
    return h


def region(shape, kind):
    """Boolean region mask of ``shape``: "rect" is the centred rectangle of half the rows and columns, "blob" a
    seeded mask of 8 x 8 blocks, about 40 % of them set (an integer hash of the block index, no random generator)."""
    nrow, ncol = shape
    if kind == "rect":
        m = np.zeros(shape, bool)
        m[nrow // 4:nrow - nrow // 4, ncol // 4:ncol - ncol // 4] = True
        return m
    br, bc = -(-nrow // 8), -(-ncol // 8)
    blocks = (_hash(br * bc, 7) % np.uint64(10) < 4).reshape(br, bc)
    return np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:nrow, :ncol].copy()


def label_blocks(shape, salt):
    """int32 label map of 8 x 8 blocks with labels 0 (background) .. 4: regions that are NOT connected sub-basins, so a
    label has many outlets."""
    nrow, ncol = shape
    br, bc = -(-nrow // 8), -(-ncol // 8)
    blocks = (_hash(br * bc, salt) % np.uint64(5)).astype(np.int32).reshape(br, bc)
    return np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:nrow, :ncol].copy()


def keys(raster):
    """Every record of one raster: (key, call, argument)."""
    out = [(f"{raster}_sto_strahler_{m}", "sto_strahler", m) for m in MIN_STO]
    out.append((f"{raster}_sto_classic_-2", "sto_classic", -2))
    out += [(f"{raster}_outflow_{r}", "outflow", r) for r in REGIONS]
    out += [(f"{raster}_outlets_basins", "outlets_basins", None), (f"{raster}_outlets_sub2", "outlets_sub2", None)]
    return out


def run(flw, call, arg, cache):
    """One case on ``flw`` (the reference's FlwdirRaster or the device's): a tuple of arrays.  ``cache``: a dict kept
    per raster for the stream orders."""
    if "strahler" not in cache:
        cache["strahler"] = flw.stream_order()
    if call == "sto_strahler":
        return flw.subbasins_streamorder(strord=cache["strahler"], min_sto=arg)
    if call == "sto_classic":
        if "classic" not in cache:
            cache["classic"] = flw.stream_order(type="classic")
        return flw.subbasins_streamorder(strord=cache["classic"], min_sto=arg)
    if call == "outflow":
        return (flw.outflow_idxs(region(flw.shape, arg)),)
    if call == "outlets_basins":
        return flw.basin_outlets(flw.basins())
    if call == "outlets_sub2":
        return flw.basin_outlets(flw.subbasins_streamorder(strord=cache["strahler"], min_sto=2)[0])
    raise ValueError(call)
