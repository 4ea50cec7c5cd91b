"""The cases of FlwdirRaster.ucat_volume / subgrid_rivlen / subgrid_rivslp / subgrid_rivavg / subgrid_rivmed
(tests/golden/wide_subgrid_riv.npz, written by tools/gen_golden_subgrid_riv.py) and plain numpy restatements of the loops
of the reference they stand for (pyflwdir/subgrid.py: ucat_volume, segment_length, segment_average, segment_median,
segment_slope, fixed_length_slope; arithmetics._average), written from their documented behaviour — shared by the
generator (which runs the reference), tests/test_subgrid_riv_cases.py (CPU) and tests/test_gpu_subgrid_riv.py (device).
Nothing of the library is imported here.

A segment is the list of cells a walk visits from an outlet cell along ``nxt`` (the downstream links, or the main upstream
cells).  Three stop rules:
* ``onto``    (segment_length) the walk steps onto the next outlet and includes it; it stops before a masked-out cell, at
              a pit (``nxt`` is the cell itself) and at a missing next cell;
* ``before``  (segment_average, _median, _slope) the walk stops before the next outlet, too;
* ``fixed``   (fixed_length_slope) down while distnc > x0, ending at a pit; from there up the main stem while distnc < x1,
              ending at a headwater.
The walks run over Python lists; the arithmetic is then done for all segments at once, position by position, in exactly
the types the interpreted reference (numpy >= 2, NEP 50) ends up with — stated explicitly at every fold below.
"""
from __future__ import annotations

import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = "wide_subgrid_riv.npz"
RASTERS = ["flwdir0", "flwdir_large", "rhine400"]  # rhine400: the 400 x 400 corner of rhine
FULL = {"flwdir0"}  # outputs in full; else digests
GRIDS = ["ll", "pr"]  # the raster's own lat/lon transform; a projected grid of 90 m cells
CELLSIZES = [1, 3, 7]
PROJECTED = (90.0, 0.0, 300000.0, 0.0, -90.0, 5700000.0)
MVDUP = ("flwdir_large", "ll", 7)  # this case is also run with a missing-value entry and a repeated outlet in the list
SPARSE = ("rhine400", "pr", 7)  # ... and this one with every 40th outlet only, as a 1D list: walks of hundreds of cells
NONE_CASE = ("flwdir0", "ll")  # idxs_out=None: every cell is an outlet
DEPTHS_DEFAULT = np.arange(0.5, 3.0, 0.5, dtype=np.float32)
DEPTHS_ONE = np.array([1.0], np.float32)
DEPTHS_NINE = np.linspace(0.25, 4.25, 9)  # float64
NODATA = -9999.0

# random rasters of tests/test_gpu_subgrid_riv.py: one row, one column, not a multiple of the 64-cell tile and more than
# one tile each way; outlet counts around the 256-thread workgroup of the walks
FUZZ_SHAPES = [(1, 300), (300, 1), (65, 129), (257, 255)]
FUZZ_COUNTS = [255, 256, 257]
FUZZ_SEED_BASE = 5500


def d8_of(raster):
    if raster == "rhine400":
        return np.ascontiguousarray(np.load(os.path.join(GOLD, "rhine.npz"))["d8"][:400, :400])
    return np.load(os.path.join(GOLD, raster + ".npz"))["d8"]


def transform_of(raster, grid):
    """(six affine coefficients, latlon)"""
    if grid == "pr":
        return PROJECTED, False
    with open(os.path.join(GOLD, "manifest.json")) as f:
        ent = json.load(f)["rhine" if raster == "rhine400" else raster]
    return tuple(ent["transform"]), bool(ent["latlon"])


def configs():
    """Every recorded configuration: (key, raster, grid, cellsize, variant); variant "" (the outlets of ucat_outlets),
    "mvdup" (the same list with a missing value and a repeat), "sparse" (every 40th outlet) or "none" (idxs_out=None)."""
    out = [(f"{r}_{g}_{c}", r, g, c, "") for r in RASTERS for g in GRIDS for c in CELLSIZES]
    out.append(("%s_%s_%d_mvdup" % MVDUP, *MVDUP, "mvdup"))
    out.append(("%s_%s_%d_sparse" % SPARSE, *SPARSE, "sparse"))
    out.append(("%s_%s_none" % NONE_CASE, *NONE_CASE, 0, "none"))
    return out


def mvdup(idxs_out, mv):
    """The outlet list with entry 3 missing and entry 5 a repeat of entry 4."""
    out = np.array(idxs_out, copy=True)
    flat = out.reshape(-1)
    flat[3] = mv
    flat[5] = flat[4]
    return out


def sparse(idxs_out):
    """Every 40th outlet, as a 1D list."""
    return np.ascontiguousarray(np.asarray(idxs_out).ravel()[::40])


def variant_outlets(idxs_out, variant, mv):
    """The outlet list of a configuration from the outlets of ucat_outlets."""
    return mvdup(idxs_out, mv) if variant == "mvdup" else (sparse(idxs_out) if variant == "sparse" else idxs_out)


def inputs(n, seed=0):
    """The seeded per-cell inputs of a raster of n cells: elevation (float32 / float64), data with 5 % nodata (float32 /
    float64), float64 weights, a mask with 85 % True, HAND (float32 / float64).  No zeros among the data (the order of
    -0.0 and 0.0 in a sort is nobody's contract)."""
    rng = np.random.default_rng([77, n, seed])
    elev32 = (rng.random(n) * 500.0).astype(np.float32)
    elev64 = rng.random(n) * 500.0
    data32 = (rng.random(n) * 99.0 + 1.0).astype(np.float32)
    data32[rng.random(n) < 0.05] = NODATA
    data64 = rng.random(n) * 99.0 + 1.0
    data64[rng.random(n) < 0.05] = NODATA
    w64 = rng.random(n) + 0.5
    mask = rng.random(n) < 0.85
    hand32 = (rng.random(n) * 4.0).astype(np.float32)
    hand64 = rng.random(n) * 4.0
    return dict(elev32=elev32, elev64=elev64, data32=data32, data64=data64, w64=w64, mask=mask, hand32=hand32, hand64=hand64)


def calls(variant=""):
    """The recorded calls of one configuration: (name, method, keyword arguments by input name)."""
    c = [
        ("rivlen_up_cell", "rivlen", dict(direction="up", unit="cell")),
        ("rivlen_down_m", "rivlen", dict(direction="down", unit="m")),
        ("rivlen_down_m_mask", "rivlen", dict(direction="down", unit="m", mask="mask")),
        ("rivslp_both_1000", "rivslp", dict(elevtn="elev32", length=1000, direction="both")),
        ("rivslp_both_2000", "rivslp", dict(elevtn="elev64", length=2000, direction="both")),
        ("rivslp_up", "rivslp", dict(elevtn="elev64", direction="up")),
        ("rivslp_down", "rivslp", dict(elevtn="elev32", direction="down")),
        ("rivslp_both_1000_mask", "rivslp", dict(elevtn="elev32", length=1000, direction="both", mask="mask")),
        ("rivavg_f32", "rivavg", dict(data="data32", direction="up")),
        ("rivavg_f32_mask", "rivavg", dict(data="data32", direction="up", mask="mask")),
        ("rivavg_f64_w64_down", "rivavg", dict(data="data64", weights="w64", direction="down")),
        ("rivmed_up", "rivmed", dict(data="data32", direction="up")),
        ("rivmed_down", "rivmed", dict(data="data64", direction="down", mask="mask")),
        ("vol_h32", "volume", dict(hand="hand32", depths="default")),
        ("vol_h64", "volume", dict(hand="hand64", depths="default")),
        ("vol_h32_one", "volume", dict(hand="hand32", depths="one")),
        ("vol_h32_nine", "volume", dict(hand="hand32", depths="nine")),
        ("vol_h64_nine", "volume", dict(hand="hand64", depths="nine")),
    ]
    if variant == "none":
        # (fixed_length_slope is left out: from an outlet on a nodata cell the reference steps to its missing value, which
        #  as an index is the raster's last cell, and goes on from there)
        keep = {"rivlen_up_cell", "rivlen_down_m_mask", "rivslp_up", "rivslp_down", "rivavg_f32", "rivavg_f64_w64_down",
                "rivmed_up", "rivmed_down"}
        c = [x for x in c if x[0] in keep]
    return c


def depths_of(name):
    return {"default": DEPTHS_DEFAULT, "one": DEPTHS_ONE, "nine": DEPTHS_NINE}[name]


def canon(a):
    """NaNs count as equal when they sit in the same positions: every NaN becomes the same NaN."""
    a = np.array(a, copy=True)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


# ---- the serial loops, restated ------------------------------------------------------------------------------------------
class Graph:
    """What the loops need of a raster: downstream links, main upstream cells, the cell sequence, the missing value,
    distances to the outlet (float32 metres, int32 cells) and the area of a cell per row (float64 on lat/lon grids,
    float32 on projected ones)."""

    def __init__(self, idxs_ds, idxs_us_main, seq, mv, shape, distnc=None, distnc_cell=None, area_rows=None):
        self.mv = int(mv)
        self.n = int(np.asarray(idxs_ds).size)
        self.shape = tuple(shape)
        self.ds = [int(v) for v in np.asarray(idxs_ds).tolist()]
        self.us = None if idxs_us_main is None else [int(v) for v in np.asarray(idxs_us_main).tolist()]
        self.seq = None if seq is None else [int(v) for v in np.asarray(seq).tolist()]
        self.distnc, self.distnc_cell, self.area_rows = distnc, distnc_cell, area_rows

    def nxt(self, direction):
        return self.ds if direction == "down" else self.us

    def outlets(self, idxs_out):
        """(list of outlet cells with None for a missing value, outlet flags)"""
        out = [None if int(v) == self.mv else int(v) for v in np.asarray(idxs_out).ravel().tolist()]
        flag = bytearray(self.n)
        for c in out:
            if c is not None:
                flag[c] = 1
        return out, flag


def walk_segments(g, idxs_out, direction, mask=None, onto=False, stats=None):
    """The cells of every outlet's segment as a CSR pair (offsets int64[k + 1], cells int64[M]); a missing outlet has an
    empty segment.  ``stats`` counts what ended the walks: "mask", "pit", "missing" (no next cell), "outlet"."""
    out, flag = g.outlets(idxs_out)
    nxt, mv = g.nxt(direction), g.mv
    m = None if mask is None else np.asarray(mask).ravel().astype(bool).tolist()
    offs, cells = [0], []
    why = dict(mask=0, pit=0, missing=0, outlet=0)
    for idx0 in out:
        if idx0 is not None:
            cells.append(idx0)
            idx = idx0
            while True:
                idx1 = nxt[idx]
                if idx1 == mv or idx1 == idx or (m is not None and not m[idx1]):
                    why["missing" if idx1 == mv else ("pit" if idx1 == idx else "mask")] += 1
                    break
                if not onto and flag[idx1]:
                    why["outlet"] += 1
                    break
                idx = idx1
                cells.append(idx)
                if onto and flag[idx1]:
                    why["outlet"] += 1
                    break
        offs.append(len(cells))
    if stats is not None:
        for key, v in why.items():
            stats[key] = stats.get(key, 0) + v
        stats["longest"] = max(stats.get("longest", 0), int(np.diff(offs).max()) if len(offs) > 1 else 0)
    return np.asarray(offs, np.int64), np.asarray(cells, np.int64), out


def _by_position(offs):
    """For a position-by-position fold over all segments at once: yields (segment ids that hold a j-th cell, index of that
    cell in the CSR list) for j = 0, 1, ... — within a segment the cells are taken in walk order, one after the other."""
    lens = np.diff(offs)
    order = np.argsort(-lens, kind="stable")
    sl = lens[order]
    for j in range(int(lens.max()) if lens.size else 0):
        act = order[: int(np.searchsorted(-sl, -j, side="left"))]  # segments with more than j cells
        yield act, offs[act] + j


def segment_length(g, idxs_out, direction, distnc, mask=None):
    """|distnc[last] - distnc[outlet]| in the dtype of distnc; -9999 for a missing outlet."""
    distnc = np.asarray(distnc).ravel()
    offs, cells, out = walk_segments(g, idxs_out, direction, mask, onto=True)
    res = np.full(len(out), NODATA, distnc.dtype)
    has = np.diff(offs) > 0
    first, last = cells[offs[:-1][has]], cells[offs[1:][has] - 1]
    res[has] = np.abs(distnc[last] - distnc[first])  # (int32 - int32, float32 - float32)
    return res


def segment_average(g, idxs_out, direction, data, weights=None, nodata=NODATA, mask=None):
    """arithmetics._average over each segment.  With T / W the dtypes of data / weights and P their common type:
    ``v = 0.0; v += w0 * v0`` makes v a P after the first add (the Python float is weak), ``w += w0`` a W; the result
    ``v / w`` is a P, stored as T; nodata where nothing was added or the weights sum to 0.  ``v0 == nodata`` compares in T."""
    data = np.asarray(data).ravel()
    T = data.dtype.type
    weights = np.ones(g.n, np.float32) if weights is None else np.asarray(weights).ravel()
    W = weights.dtype.type
    P = np.result_type(T, W).type
    offs, cells, out = walk_segments(g, idxs_out, direction, mask)
    k = len(out)
    v, w = np.zeros(k, P), np.zeros(k, W)
    nd = T(nodata)
    for act, pos in _by_position(offs):
        c = cells[pos]
        v0, w0 = data[c], weights[c]
        use = ~np.isnan(v0) if np.isnan(nodata) else v0 != nd
        a, c = act[use], c[use]
        v[a] = v[a] + (weights[c].astype(P) * data[c].astype(P))  # the product rounded to P, then the add
        w[a] = w[a] + weights[c]
    res = np.full(k, nd, T)
    ok = w != 0
    with np.errstate(all="ignore"):
        res[ok] = (v[ok] / w[ok].astype(P)).astype(T)
    return res


def segment_median(g, idxs_out, direction, data, nodata=NODATA, mask=None):
    """np.nanmedian of the segment's values that are not nodata: the middle value, or ``(a + b) / 2`` in the data's dtype
    for an even count; NaN for a segment whose values are all nodata (or NaN); nodata for a missing outlet."""
    data = np.asarray(data).ravel()
    T = data.dtype.type
    offs, cells, out = walk_segments(g, idxs_out, direction, mask)
    k = len(out)
    seg = np.repeat(np.arange(k), np.diff(offs))
    vals = data[cells]
    keep = ~(np.isnan(vals) | (vals == T(nodata)))
    seg, vals = seg[keep], vals[keep]
    order = np.lexsort((vals, seg))
    seg, vals = seg[order], vals[order]
    cnt = np.bincount(seg, minlength=k)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    res = np.full(k, T(nodata), T)
    present = np.array([c is not None for c in out], bool)
    res[present & (cnt == 0)] = np.nan
    odd = present & (cnt % 2 == 1)
    res[odd] = vals[start[odd] + cnt[odd] // 2]
    even = present & (cnt > 0) & (cnt % 2 == 0)
    with np.errstate(all="ignore"):
        res[even] = (vals[start[even] + cnt[even] // 2 - 1] + vals[start[even] + cnt[even] // 2]) / T(2)
    return res, cnt


def segment_slope(g, idxs_out, direction, elevtn, distnc):
    """|dz / dx| between the first and the last cell of the segment: dz in the dtype of elevtn, dx in float32, the
    quotient in their common type, stored in the dtype of elevtn; 0 for a one-cell segment; the mask is not looked at
    (the interpreted reference tests ``mask[i] is False``, which never holds)."""
    elevtn, distnc = np.asarray(elevtn).ravel(), np.asarray(distnc).ravel()
    E = elevtn.dtype.type
    offs, cells, out = walk_segments(g, idxs_out, direction, None)
    res = np.full(len(out), NODATA, E)
    lens = np.diff(offs)
    res[lens == 1] = 0.0
    m = lens > 1
    a, b = cells[offs[:-1][m]], cells[offs[1:][m] - 1]
    with np.errstate(all="ignore"):
        res[m] = np.abs((elevtn[a] - elevtn[b]) / (distnc[a] - distnc[b])).astype(E)
    return res


def fixed_length_slope(g, idxs_out, elevtn, distnc, length=1000, stats=None):
    """|dz / dx| between the cell reached by walking down while distnc > distnc[outlet] - length / 2 (a pit ends it) and
    the cell reached from there by walking up the main stem while distnc < distnc[outlet] + length / 2 (a headwater ends
    it).  ``length / 2`` is a Python float and joins the float32 of distnc; the quotient is taken in the common type of
    elevtn and float32 and stored as float32; 0 where both walks stay on one cell."""
    elevtn, distnc = np.asarray(elevtn).ravel(), np.asarray(distnc).ravel()
    assert distnc.dtype == np.float32
    out, _ = g.outlets(idxs_out)
    half = np.float32(length / 2)
    dl = distnc.tolist()  # (float32 values as Python floats: comparisons are exact)
    lo, hi = [], []
    cut_pit = cut_head = 0
    for idx0 in out:
        if idx0 is None:
            lo.append(-1), hi.append(-1)
            continue
        x0, x1 = float(distnc[idx0] - half), float(distnc[idx0] + half)
        idx = idx0
        while dl[idx] > x0:
            d = g.ds[idx]
            if d == idx or d == g.mv:
                cut_pit += 1
                break
            idx = d
        lo.append(idx)
        while dl[idx] < x1:
            u = g.us[idx]
            if u == g.mv:
                cut_head += 1
                break
            idx = u
        hi.append(idx)
    if stats is not None:
        stats.update(cut_pit=cut_pit, cut_head=cut_head)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    res = np.full(len(out), NODATA, np.float32)
    res[(lo >= 0) & (lo == hi)] = 0.0
    m = (lo >= 0) & (lo != hi)
    with np.errstate(all="ignore"):
        res[m] = np.abs((elevtn[lo[m]] - elevtn[hi[m]]) / (distnc[lo[m]] - distnc[hi[m]])).astype(np.float32)
    return res


def ucat_map(g, idxs_out, dtype):
    """The unit catchment map: label i + 1 on outlet i (the last entry wins a repeated cell), handed upstream in
    sequence order to every cell without a label; plus, per label, its cells in the order they were added."""
    out, _ = g.outlets(idxs_out)
    lab = [0] * g.n
    for i, c in enumerate(out):
        if c is not None:
            lab[c] = i + 1
    added_cell, added_lab = [], []
    for idx0 in g.seq:
        u = lab[g.ds[idx0]]
        if lab[idx0] == 0 and u != 0:
            lab[idx0] = u
            added_cell.append(idx0), added_lab.append(u - 1)
    return np.asarray(lab, dtype), np.asarray(added_cell, np.int64), np.asarray(added_lab, np.int64), out


def ucat_volume(g, idxs_out, hand, depths, map_dtype=np.int32):
    """(map, volume[depths.size, k]).  With D / H / A the dtypes of depths / hand / area: ``dh = max(0, depths - hand)`` in
    the common type of D and H, ``area * dh`` in P, the common type of all three; a column starts as D(area * dh) of its
    outlet cell and then takes ``col = D(P(col) + area * dh)`` for each added cell, in sequence order."""
    hand, depths = np.asarray(hand).ravel(), np.asarray(depths)
    area = np.asarray(g.area_rows)
    ncol = g.shape[1]
    D = depths.dtype.type
    DH = np.result_type(depths.dtype, hand.dtype).type
    P = np.result_type(DH, area.dtype).type
    lab, cells, labs, out = ucat_map(g, idxs_out, map_dtype)
    k = len(out)

    def term(c):  # [nd, len(c)] in P
        dh = np.maximum(DH(0), depths.astype(DH)[:, None] - hand[c].astype(DH)[None, :])
        return area[c // ncol].astype(P)[None, :] * dh.astype(P)

    vol = np.full((depths.size, k), NODATA, D)
    present = np.flatnonzero([c is not None for c in out])
    oc = np.asarray([out[i] for i in present], np.int64)
    with np.errstate(all="ignore"):
        if present.size:
            vol[:, present] = term(oc).astype(D)
        order = np.argsort(labs, kind="stable")
        cells, labs = cells[order], labs[order]
        offs = np.concatenate([[0], np.cumsum(np.bincount(labs, minlength=k))]).astype(np.int64)
        for act, pos in _by_position(offs):
            vol[:, act] = (vol[:, act].astype(P) + term(cells[pos])).astype(D)
    return lab, vol


def run(g, method, idxs_out, inp, kw, stats=None):
    """One recorded call on the restated loops (the counterpart of the generator's call of the reference)."""
    kw = dict(kw)
    mask = inp[kw.pop("mask")] if "mask" in kw else None
    if method == "rivlen":
        d = g.distnc if kw["unit"] == "m" else g.distnc_cell
        return segment_length(g, idxs_out, kw["direction"], d, mask)
    if method == "rivslp":
        if kw["direction"] == "both":
            return fixed_length_slope(g, idxs_out, inp[kw["elevtn"]], g.distnc, kw["length"], stats)
        return segment_slope(g, idxs_out, kw["direction"], inp[kw["elevtn"]], g.distnc)
    if method == "rivavg":
        w = inp[kw["weights"]] if "weights" in kw else None
        return segment_average(g, idxs_out, kw["direction"], inp[kw["data"]], w, NODATA, mask)
    if method == "rivmed":
        return segment_median(g, idxs_out, kw["direction"], inp[kw["data"]], NODATA, mask)[0]
    if method == "volume":
        return ucat_volume(g, idxs_out, inp[kw["hand"]], depths_of(kw["depths"]))
    raise ValueError(method)


def fuzz_cases():
    """(shape, outlet count, seed) of the random rasters."""
    return [(s, c, 10 * i + j) for i, s in enumerate(FUZZ_SHAPES) for j, c in enumerate(FUZZ_COUNTS)]


def fuzz_outlets(rng, valid_cells, count, mv, dtype):
    """``count`` outlets drawn from the valid cells (with repeats when there are fewer), one entry missing."""
    out = rng.choice(valid_cells, size=count, replace=valid_cells.size < count).astype(dtype)
    out[rng.integers(0, count)] = mv
    return out
