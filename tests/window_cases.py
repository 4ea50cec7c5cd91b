"""The cases of FlwdirRaster.downstream / moving_average / moving_median / path (tests/golden/wide_window.npz, written by
tools/gen_golden_window.py) and plain numpy restatements of the serial loops of the reference they stand for
(Flwdir.downstream; arithmetics.moving_average / moving_median over core._window with arithmetics._average and
np.nanmedian; core.path over core._trace), written from their documented behaviour — shared by the generator (which runs
the reference), tests/test_window_cases.py (CPU) and tests/test_gpu_window.py (device).  Nothing of the library is
imported here.

The window of a cell holds 2n + 1 positions: the centre at n, the cells reached by at most n steps down the downstream
links after it (a pit, a missing link and — with a stream order — a cell of a higher order than the centre end the walk
before they are entered), the cells reached by at most n steps up the main upstream cells before it, the farthest first.
Empty positions are dropped; what is left, in position order, is the order of the float sums.  The restatement builds
the windows of ALL cells at once, one step per numpy operation, and folds them position by position in exactly the types
the interpreted reference (numpy >= 2, NEP 50) ends up with — stated explicitly at every fold below.
"""
from __future__ import annotations

import os

import numpy as np

from subgrid_riv_cases import GOLD, PROJECTED, canon, d8_of, transform_of  # noqa: F401  (the rasters of those cases)

RECORD = "wide_window.npz"
RASTERS = ["flwdir0", "flwdir_large", "rhine400"]
FULL = {"flwdir0"}  # outputs in full; else digests
GRIDS = ["ll", "pr"]  # (the paths in metres; the window calls do not look at the grid)
NODATA = -9999.0
NS = [0, 1, 3, 10]

FUZZ_SHAPES = [(1, 300), (300, 1), (65, 129), (257, 255)]
FUZZ_COUNTS = [255, 256, 257]  # start cells of the paths, around the 256-thread workgroup
FUZZ_SEED_BASE = 6600


def inputs(n, seed=0):
    """The seeded per-cell inputs of a raster of n cells: data (float32 / float64) with 5 % nodata and 2 % NaN, weights
    (float32 / float64) with 10 % zeros, a mask with 15 % True, payloads of other dtypes for ``downstream``.  No zeros
    among the data (the order of -0.0 and 0.0 in a sort is nobody's contract)."""
    rng = np.random.default_rng([88, n, seed])
    data32 = (rng.random(n) * 99.0 + 1.0).astype(np.float32)
    data32[rng.random(n) < 0.05] = NODATA
    data32[rng.random(n) < 0.02] = np.nan
    data64 = rng.random(n) * 99.0 + 1.0
    data64[rng.random(n) < 0.05] = NODATA
    data64[rng.random(n) < 0.02] = np.nan
    w32 = (rng.random(n) + 0.5).astype(np.float32)
    w32[rng.random(n) < 0.10] = 0.0
    w64 = rng.random(n) + 0.5
    w64[rng.random(n) < 0.10] = 0.0
    mask = rng.random(n) < 0.15
    return dict(data32=data32, data64=data64, w32=w32, w64=w64, mask=mask, flag=rng.random(n) < 0.5,
                i16=rng.integers(-30000, 30000, n).astype(np.int16), i64=rng.integers(-2**62, 2**62, n))


def window_calls(raster=""):
    """The recorded window calls: (name, method, keyword arguments by input name).  ``strord="given"``: the recorded
    Strahler order is passed while restrict_strord stays False (the reference honours it all the same)."""
    nan = float("nan")
    c = [
        ("ds_f32", "downstream", dict(data="data32")),
        ("ds_f64", "downstream", dict(data="data64")),
        ("ds_bool", "downstream", dict(data="flag")),
        ("ds_i16", "downstream", dict(data="i16")),
        ("ds_i64", "downstream", dict(data="i64")),
        ("avg_f32_n0", "average", dict(data="data32", n=0)),
        ("avg_f32_n3", "average", dict(data="data32", n=3)),
        ("avg_f32_w32_n1", "average", dict(data="data32", n=1, weights="w32")),
        ("avg_f32_w64_n3", "average", dict(data="data32", n=3, weights="w64")),
        ("avg_f64_n10", "average", dict(data="data64", n=10)),
        ("avg_f64_w32_n3", "average", dict(data="data64", n=3, weights="w32")),
        ("avg_f64_w64_n10", "average", dict(data="data64", n=10, weights="w64")),
        ("avg_f32_nan_n3", "average", dict(data="data32", n=3, nodata=nan)),
        ("avg_f64_w64_nan_n0", "average", dict(data="data64", n=0, weights="w64", nodata=nan)),
        ("avg_f32_so_n10", "average", dict(data="data32", n=10, restrict_strord=True)),
        ("avg_f64_w64_given_n3", "average", dict(data="data64", n=3, weights="w64", strord="given")),
        ("med_f32_n0", "median", dict(data="data32", n=0)),
        ("med_f32_n1", "median", dict(data="data32", n=1)),
        ("med_f32_n3", "median", dict(data="data32", n=3)),
        ("med_f64_n10", "median", dict(data="data64", n=10)),
        ("med_f32_nan_n3", "median", dict(data="data32", n=3, nodata=nan)),
        ("med_f64_nan_n0", "median", dict(data="data64", n=0, nodata=nan)),
        ("med_f32_so_n10", "median", dict(data="data32", n=10, restrict_strord=True)),
        ("med_f64_given_n3", "median", dict(data="data64", n=3, strord="given")),
    ]
    if raster == "rhine400":  # (the interpreted reference takes its time on 160000 cells)
        keep = {"ds_f32", "ds_bool", "avg_f32_w64_n3", "avg_f64_w64_n10", "avg_f32_so_n10", "med_f32_n3", "med_f64_n10",
                "med_f32_so_n10"}
        c = [x for x in c if x[0] in keep]
    return c


def max_length_m(raster, grid):
    """A max_length in metres of about three and a half cells."""
    tr, latlon = transform_of(raster, grid)
    return 3.5 * abs(tr[4]) * (111000.0 if latlon else 1.0)


def path_calls(raster, grid):
    """The recorded path calls of one raster and grid: (name, keyword arguments; mask by input name)."""
    mx = max_length_m(raster, grid)
    c = [
        ("down_m", dict(direction="down", unit="m")),
        ("up_m_mask", dict(direction="up", unit="m", mask="mask")),
        ("down_m_max", dict(direction="down", unit="m", max_length=mx)),
        ("up_m_max_mask", dict(direction="up", unit="m", max_length=2 * mx, mask="mask")),
    ]
    if grid == "ll":  # (cell units do not look at the grid)
        c += [
            ("down", dict(direction="down")),
            ("up", dict(direction="up")),
            ("down_mask", dict(direction="down", mask="mask")),
            ("up_mask", dict(direction="up", mask="mask")),
            ("down_max5", dict(direction="down", max_length=5)),
            ("up_max2_5", dict(direction="up", max_length=2.5)),
        ]
    return c


def path_starts(ds, us, mv, mask, seed=0, count=40):
    """A start list with a pit, a headwater, a nodata cell, a masked cell, a repeated cell and ``count`` random valid
    cells (int64).  ``ds`` / ``us``: downstream and main upstream cells with ``mv`` for none."""
    ds, us = np.asarray(ds).astype(np.int64), np.asarray(us).astype(np.int64)
    mv = int(np.int64(np.asarray(mv).astype(np.int64)))
    idx = np.arange(ds.size)
    valid = np.flatnonzero(ds != mv)
    rng = np.random.default_rng([99, ds.size, seed])
    some = rng.choice(valid, size=count, replace=valid.size < count)
    special = [np.flatnonzero(ds == idx)[:1], np.flatnonzero((ds != mv) & (us == mv))[:1], np.flatnonzero(ds == mv)[:1],
               np.flatnonzero((ds != mv) & np.asarray(mask).ravel())[:1], some[:1]]
    return np.concatenate([some] + special).astype(np.int64)


# ---- the serial loops, restated ------------------------------------------------------------------------------------------
class Graph:
    """What the loops need of a raster: downstream links and main upstream cells (int64, -1 for the missing value), the
    index dtype, the shape and — for paths in metres — the length of a step as ``steps[row + next row, kind]`` (kind 0: same
    column, 1: same row, 2: diagonal; float64)."""

    def __init__(self, idxs_ds, idxs_us_main, mv, shape, steps=None):
        ds, us = np.asarray(idxs_ds).ravel(), np.asarray(idxs_us_main).ravel()
        self.idx_dtype = ds.dtype
        self.ds = np.where(ds == mv, -1, ds.astype(np.int64))
        self.us = np.where(us == mv, -1, us.astype(np.int64))
        self.n, self.shape, self.steps = ds.size, tuple(shape), steps


def downstream(g, data):
    """out = data.copy(); out[valid] = data[idxs_ds[valid]] (a pit: itself)."""
    data = np.asarray(data).ravel()
    out = data.copy()
    valid = g.ds >= 0
    out[valid] = data[g.ds[valid]]
    return out


def windows(g, n, strord=None, stats=None):
    """int64 [n_cells, 2n + 1], -1 for an empty position.  ``stats`` counts what cut the windows short."""
    idx = np.arange(g.n, dtype=np.int64)
    win = np.full((g.n, 2 * n + 1), -1, np.int64)
    win[:, n] = idx
    so = None if strord is None else np.asarray(strord).ravel().astype(np.int64)
    cur, alive = idx.copy(), np.ones(g.n, bool)
    why = dict(pit=0, nodata=0, strord=0, headwater=0)
    for i in range(n):
        nxt = g.ds[cur]
        pit, missing = nxt == cur, nxt < 0
        higher = np.zeros(g.n, bool) if so is None else (~missing & (so[np.maximum(nxt, 0)] > so))
        why["pit"] += int(np.count_nonzero(alive & pit))
        why["nodata"] += int(np.count_nonzero(alive & missing))
        why["strord"] += int(np.count_nonzero(alive & ~pit & ~missing & higher))
        alive &= ~(pit | missing | higher)
        cur = np.where(alive, nxt, cur)
        win[alive, n + i + 1] = cur[alive]
    cur, alive = idx.copy(), np.ones(g.n, bool)
    for i in range(n):
        nxt = g.us[cur]
        why["headwater"] += int(np.count_nonzero(alive & (nxt < 0) & (g.ds >= 0)))
        alive &= nxt >= 0
        cur = np.where(alive, nxt, cur)
        win[alive, n - i - 1] = cur[alive]
    if stats is not None:
        for key, v in why.items():
            stats[key] = stats.get(key, 0) + v
    return win


def moving_average(g, data, n, weights=None, strord=None, nodata=NODATA, stats=None):
    """arithmetics._average over each window.  With T / W the dtypes of data / weights (float64 ones without weights) and
    P their common type: ``v = 0.0; v += w0 * v0`` makes v a P after the first add (the Python float is weak), the product
    rounded to P before the add; ``w += w0`` is a W; ``v / w`` a P, stored as T; nodata where the weights sum to 0 and
    where ``data == nodata`` (compared in T: a NaN nodata skips no cell)."""
    data = np.asarray(data).ravel()
    T = data.dtype.type
    weights = np.ones(g.n, np.float64) if weights is None else np.asarray(weights).ravel()
    W = weights.dtype.type
    P = np.result_type(T, W).type
    nd = T(nodata)
    win = windows(g, n, strord)
    centre = ~(data == nd)
    v, w = np.zeros(g.n, P), np.zeros(g.n, W)
    for j in range(2 * n + 1):
        c = win[:, j]
        a = np.flatnonzero((c >= 0) & centre)
        v0 = data[c[a]]
        a = a[~np.isnan(v0) if np.isnan(nodata) else v0 != nd]
        cc = c[a]
        with np.errstate(all="ignore"):
            v[a] = v[a] + (weights[cc].astype(P) * data[cc].astype(P))
            w[a] = w[a] + weights[cc]
    res = np.full(g.n, nd, T)
    ok = centre & (w != 0)
    with np.errstate(all="ignore"):
        res[ok] = (v[ok] / w[ok].astype(P)).astype(T)
    if stats is not None:
        stats["w0"] = stats.get("w0", 0) + int(np.count_nonzero(centre & (w == 0)))
    return res


def moving_median(g, data, n, strord=None, nodata=NODATA, stats=None):
    """np.nanmedian of each window's values that are not nodata: the middle value, or ``(a + b) / 2`` in the data's dtype
    for an even count; NaN for a window whose values are all nodata or NaN; nodata where ``data == nodata``."""
    data = np.asarray(data).ravel()
    T = data.dtype.type
    nd = T(nodata)
    win = windows(g, n, strord)
    vals = np.where(win >= 0, data[np.maximum(win, 0)], T(np.nan))
    vals[vals == nd] = np.nan
    vals.sort(axis=1)  # (NaNs last)
    cnt = np.count_nonzero(~np.isnan(vals), axis=1)
    centre = ~(data == nd)
    rows = np.arange(g.n)
    res = np.full(g.n, nd, T)
    res[centre & (cnt == 0)] = np.nan
    odd = centre & (cnt % 2 == 1)
    res[odd] = vals[rows[odd], cnt[odd] // 2]
    even = centre & (cnt > 0) & (cnt % 2 == 0)
    with np.errstate(all="ignore"):
        res[even] = (vals[rows[even], cnt[even] // 2 - 1] + vals[rows[even], cnt[even] // 2]) / T(2)
    if stats is not None:
        stats["empty"] = stats.get("empty", 0) + int(np.count_nonzero(centre & (cnt == 0)))
        stats["odd"] = stats.get("odd", 0) + int(np.count_nonzero(odd))
        stats["even"] = stats.get("even", 0) + int(np.count_nonzero(even))
    return res


def path(g, idxs0, direction="down", mask=None, max_length=None, unit="cell", stats=None):
    """core._trace per start cell: (list of index arrays in the index dtype, float64 distances).  The start cell is always
    part of the path; the first masked cell is included and ends it; a pit, a headwater and a missing link end it; with
    max_length it ends before the step that would make ``dist + d > max_length``.  Distances add up as Python floats."""
    nxt = (g.ds if direction == "down" else g.us).tolist()
    m = None if mask is None else np.asarray(mask).ravel().astype(bool).tolist()
    steps = g.steps if unit == "m" else None
    ncol = g.shape[1]
    paths, dists = [], np.zeros(len(idxs0), np.float64)
    why = dict(mask=0, end=0, max_length=0)
    for i, idx0 in enumerate(np.asarray(idxs0).ravel().tolist()):
        cells, dist, d = [idx0], 0.0, 1.0
        while True:
            if m is not None and m[idx0]:
                why["mask"] += 1
                break
            idx1 = nxt[idx0]
            if idx1 == idx0 or idx1 < 0:
                why["end"] += 1
                break
            if steps is not None:
                r0, r1 = idx0 // ncol, idx1 // ncol
                kind = 1 if r0 == r1 else (0 if idx0 % ncol == idx1 % ncol else 2)
                d = float(steps[r0 + r1, kind])
            if max_length is not None and dist + d > max_length:
                why["max_length"] += 1
                break
            dist += d
            idx0 = idx1
            cells.append(idx0)
        paths.append(np.asarray(cells, g.idx_dtype))
        dists[i] = dist
    if stats is not None:
        for key, v in why.items():
            stats[key] = stats.get(key, 0) + v
    return paths, dists


def run_window(g, method, inp, kw, strord, stats=None):
    """One recorded window call on the restated loops; ``strord``: the raster's Strahler order."""
    kw = dict(kw)
    data = inp[kw.pop("data")]
    if method == "downstream":
        return downstream(g, data)
    so = strord if (kw.pop("restrict_strord", False) or kw.pop("strord", None) == "given") else None
    kw.pop("strord", None)
    if method == "average":
        w = inp[kw.pop("weights")] if "weights" in kw else None
        return moving_average(g, data, kw["n"], w, so, kw.get("nodata", NODATA), stats)
    return moving_median(g, data, kw["n"], so, kw.get("nodata", NODATA), stats)


def flat_paths(paths, dtype):
    """(cells of all paths in one array, int64 lengths)"""
    lens = np.asarray([len(p) for p in paths], np.int64)
    cells = np.concatenate([np.asarray(p, dtype) for p in paths]) if len(paths) else np.zeros(0, dtype)
    return cells, lens


def fuzz_cases():
    """(shape, number of path start cells, seed) of the random rasters."""
    return [(s, c, 10 * i + j) for i, s in enumerate(FUZZ_SHAPES) for j, c in enumerate(FUZZ_COUNTS)]
