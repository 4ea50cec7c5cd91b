"""The golden cases of interbasin_mask / inflow_idxs / basin_bounds / subbasins_pfafstetter (tests/golden/
wide_basins.npz, written by tools/gen_golden_basins.py): rasters, regions, stream masks, basin maps, transforms and the
keys of the records, plain restatements of the four serial loops of the reference (pyflwdir/basins.py:25-64, core.py:
485-497, regions.py:57-125, basins.py:106-191), and ``pfaf_ties``, which says whether a Pfafstetter case holds a tie
among the sort keys that decide a selection or an order — shared by the generator (which runs the reference),
tests/test_basin_cases.py (CPU) and tests/test_gpu_basins_ext.py (device)."""
from __future__ import annotations

import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORNER = "confluence_13x24"  # built here (confluence_d8), not a golden raster
RASTERS = ["synth_tiny_5x7", "synth_onerow_1x300", "synth_onecol_300x1", "flwdir0", "flwdir1", "synth_loops_96x80", "rhine",
           "synth_rough_nodata_384x512", CORNER]
FULL = {"synth_tiny_5x7", "synth_onerow_1x300", "synth_onecol_300x1", "flwdir0", "flwdir1", CORNER}  # in full; else digests
REGIONS = ["rect", "checker", "empty", "all"]
STREAMS = ["none", "upa"]
DEPTHS = [1, 2, 3]
UPAREAS = ["cell", "km2"]
UPA_MINS = ["zero", "pos"]
MAPS = ["basins", "sub"]
TRANSFORMS = ["own", "south"]  # the raster's own (north-up) transform, and one with yres > 0
SOUTH_UP = (0.5, 0.0, -10.0, 0.0, 0.25, 20.0)


def confluence_d8():
    """A 13 x 24 raster made for one branch of the Pfafstetter loop: a main stem along row 7 to a pit at its east end,
    four tributaries from the north of 3, 6, 5 and 4 cells (columns 20, 16, 12, 9) and one cell from the south that joins
    at column 12 as well.  The four long ones become the sub-basins of depth 1 (five candidates, no equal areas); the
    short one is the only candidate of an inter-basin at depth 2, and the inter-basin outlet it asks for — the main
    stem cell west of the three-way confluence — is in the outlet list already (``idx1 not in idxs`` is False)."""
    d8 = np.full((13, 24), 247, np.uint8)
    d8[7, :23], d8[7, 23] = 1, 0
    for col, length in ((20, 3), (16, 6), (12, 5), (9, 4)):
        d8[7 - length:7, col] = 4
    d8[8, 12] = 64
    return d8


def d8_of(raster):
    """The D8 codes of a case raster."""
    return confluence_d8() if raster == CORNER else np.load(os.path.join(GOLD, raster + ".npz"))["d8"]


def transform_of(raster, kind):
    """(six affine coefficients, latlon) of a raster's case transform."""
    if kind == "south":
        return SOUTH_UP, False
    if raster == CORNER:
        return (0.01, 0.0, 5.0, 0.0, -0.01, 50.0), True
    with open(os.path.join(GOLD, "manifest.json")) as f:
        ent = json.load(f)[raster]
    return tuple(ent["transform"]), bool(ent["latlon"])


def region(shape, kind):
    """Boolean region of ``shape``: "rect" the centred rectangle of half the rows and columns (the whole extent along
    an axis of one cell), "checker" 4 x 4 blocks in a checkerboard — every river longer than a block leaves it and
    enters it again —, "empty" and "all"."""
    nrow, ncol = shape
    if kind == "empty":
        return np.zeros(shape, bool)
    if kind == "all":
        return np.ones(shape, bool)
    if kind == "rect":
        m = np.zeros(shape, bool)
        m[nrow // 4:nrow - nrow // 4 if nrow > 1 else 1, ncol // 4:ncol - ncol // 4 if ncol > 1 else 1] = True
        return m
    r, c = np.indices(shape)
    return (r // 4 + c // 4) % 2 == 0


def threshold(upa):
    """The positive area threshold of a case: the value of the (n // 40 + 2)-th largest upstream area."""
    flat = np.sort(np.asarray(upa).ravel())
    return float(flat[-min(flat.size, flat.size // 40 + 2)])


def keys(raster):
    """Every record of one raster: (key, call, arguments)."""
    out = [(f"{raster}_ib_{r}_{s}", "interbasin", (r, s)) for r in REGIONS for s in STREAMS]
    out += [(f"{raster}_in_{r}", "inflow", (r,)) for r in REGIONS]
    out += [(f"{raster}_bb_{m}_{t}", "bounds", (m, t)) for m in MAPS for t in TRANSFORMS]
    out += [(f"{raster}_pf_{d}_{u}_{t}", "pfaf", (d, u, t)) for d in DEPTHS for u in UPAREAS for t in UPA_MINS]
    return out


def pfaf_args(flw, cache, unit, tmin):
    """(uparea or None, upa_min) of a Pfafstetter case on ``flw`` (the reference's FlwdirRaster or the device's)."""
    if unit not in cache:
        cache[unit] = flw.upstream_area(unit)
    return (None if unit == "cell" else cache[unit]), (0.0 if tmin == "zero" else threshold(cache[unit]))


def run(flw, call, args, cache):
    """One case on ``flw`` (made with the case's transform): a tuple of arrays.  ``cache``: a dict kept per raster."""
    if call == "interbasin":
        stream = None
        if args[1] == "upa":
            if "cell" not in cache:
                cache["cell"] = flw.upstream_area()
            stream = cache["cell"] > threshold(cache["cell"])
        return (flw.interbasin_mask(region(flw.shape, args[0]), stream=stream),)
    if call == "inflow":
        return (flw.inflow_idxs(region(flw.shape, args[0])),)
    if call == "bounds":
        if args[0] not in cache:
            cache[args[0]] = flw.basins() if args[0] == "basins" else flw.subbasins_streamorder(min_sto=-1)[0]
        return flw.basin_bounds(basins=cache[args[0]])
    if call == "pfaf":
        uparea, upa_min = pfaf_args(flw, cache, args[1], args[2])
        return flw.subbasins_pfafstetter(depth=args[0], uparea=uparea, upa_min=upa_min)
    raise ValueError(call)


# ---- the four serial loops, restated ---------------------------------------------------------------------------------
def _ref_interbasin(ds, seq, region, stream=None):
    """basins.interbasin_mask (basins.py:47-64) on plain lists."""
    ds, seq = np.asarray(ds).tolist(), np.asarray(seq).tolist()
    region = np.asarray(region, bool).ravel()
    reg = region.tolist()
    mask = [True] * len(ds) if stream is None else np.asarray(stream, bool).ravel().tolist()
    if stream is not None:
        for x in reversed(seq):
            if mask[x]:
                mask[ds[x]] = True
    for x in seq:
        y = ds[x]
        mask[x] = mask[y] and not (not reg[x] and reg[y])
    return np.logical_and(np.array(mask, bool), region)


def _ref_inflow(ds, seq, region):
    """core.inflow_idxs (core.py:485-497) on plain lists: the listed cells."""
    ds, seq = np.asarray(ds).tolist(), np.asarray(seq).tolist()
    reg = np.asarray(region, bool).ravel().tolist()
    mask = [True] * len(ds)
    out = []
    for x in reversed(seq):
        y = ds[x]
        if x != y:
            if mask[x] and reg[y] and not reg[x]:
                out.append(x)
                mask[y] = False
            else:
                mask[y] = mask[x]
    return out


def label_slices(regions):
    """What scipy.ndimage.find_objects gives for the labels > 0 that occur, with numpy alone: sorted labels and
    (row slice, column slice) per label."""
    regions = np.asarray(regions)
    r, c = np.nonzero(regions > 0)
    lab = regions[r, c]
    lbs = np.unique(lab)
    out = []
    for l in lbs.tolist():
        m = lab == l
        out.append((slice(int(r[m].min()), int(r[m].max()) + 1), slice(int(c[m].min()), int(c[m].max()) + 1)))
    return lbs, out


def _ref_bounds(regions, transform):
    """regions.region_bounds (regions.py:107-125): (labels, boxes [xmin, ymin, xmax, ymax], total box)."""
    regions = np.asarray(regions)
    lbs, slices = label_slices(regions)
    if lbs.size == 0:
        raise ValueError("No regions found in data")
    a, b, c, d, e, f = [float(v) for v in tuple(transform)[:6]]
    nrow, ncol = regions.shape
    lons = (np.arange(ncol) + 0.5) * a + (np.zeros(ncol) + 0.5) * b + c
    lats = (np.zeros(nrow) + 0.5) * d + (np.arange(nrow) + 0.5) * e + f
    ix = [0, -1] if a >= 0 else [-1, 0]
    iy = [0, -1] if e >= 0 else [-1, 0]
    dx, dy = np.abs(a) / 2, np.abs(e) / 2
    boxes = []
    for ys, xs in slices:
        xmin, xmax = lons[xs][ix]
        ymin, ymax = lats[ys][iy]
        boxes.append([xmin - dx, ymin - dy, xmax + dx, ymax + dy])
    boxes = np.asarray(boxes)
    return lbs, boxes, np.hstack([boxes[:, :2].min(axis=0), boxes[:, 2:].max(axis=0)])


def _ref_classic(ds, seq, us_main, mask, mv=-1):
    """streams.stream_order (streams.py:213-225) on plain lists: uint8."""
    ds_a = np.asarray(ds)
    n = ds_a.size
    src = (ds_a != mv) & (ds_a != np.arange(n)) & np.asarray(mask, bool)
    nup = np.bincount(ds_a[src].astype(np.int64), minlength=n).tolist()
    ds, us, m = ds_a.tolist(), np.asarray(us_main).tolist(), np.asarray(mask, bool).tolist()
    strord = [0] * n
    for x in np.asarray(seq).tolist():
        if not m[x]:
            continue
        y = ds[x]
        if y == x:
            strord[x] = 1
        elif nup[y] > 1 and us[y] != x:
            strord[x] = (strord[y] + 1) & 255
        else:
            strord[x] = strord[y]
    return np.array(strord, np.uint8)


def _ref_pfafstetter(pits, ds, seq, us_main, uparea, mask, depth, mv=-1):
    """basins.subbasins_pfafstetter (basins.py:120-191) with STABLE sorts on the negated areas: (int32 map, list of
    outlets, info).  ``info`` counts what the cases are meant to reach and holds ``ties``: True when two sort keys
    that decide which tributaries are taken, or in which order, are equal (or NaN)."""
    ds_a, seq_a = np.asarray(ds).astype(np.int64), np.asarray(seq).astype(np.int64)
    upa = np.asarray(uparea).ravel()
    strord = _ref_classic(ds_a, seq_a, us_main, mask, mv)
    strord = np.where(strord <= depth + 1, strord, 0).astype(np.uint8)
    s_seq = strord[seq_a]
    trib = seq_a[(s_seq > 0) & (s_seq > strord[ds_a[seq_a]])]
    us = np.asarray(us_main).astype(np.int64)
    us[np.asarray(us_main) == mv] = -1
    us, so = us.tolist(), strord.tolist()
    branch = np.zeros(ds_a.size, np.int32)
    # (the tributaries that join a cell, and the cells a label was painted on: the candidates of a label — the tributaries
    #  `idx` in list order with pfaf_branch[idx] == 0 and pfaf_branch[idxs_ds[idx]] == label — without a scan of the list)
    joins, painted = {}, {}
    for j, (x, y) in enumerate(zip(trib.tolist(), ds_a[trib].tolist())):
        joins.setdefault(y, []).append((j, x))
    info = dict(ties=False, more_than_4=0, fewer_than_4=0, already_listed=0, stem_ends_at_order_0=0, labels=0)
    idxs, labs = [], []
    pfaf0 = 1 + sum(10**d0 for d0 in range(1, depth))

    def paint_up(x, label):
        cells = painted.setdefault(label, [])
        branch[x] = label
        cells.append(x)
        while True:
            x = us[x]
            if x == -1:
                break
            if so[x] == 0:
                info["stem_ends_at_order_0"] += 1
                break
            branch[x] = label
            cells.append(x)

    for i, x in enumerate(np.asarray(pits).tolist()):
        idxs.append(x)
        labs.append((pfaf0 + (i + 1) * 10**depth, 1))
        paint_up(x, labs[-1][0])
    seen = set(idxs)
    while labs:
        lab0, d0 = labs.pop(0)
        cand = sorted(t for y in painted.get(lab0, ()) if branch[y] == lab0 for t in joins.get(y, ()) if branch[t[1]] == 0)
        cand = np.array([x for _, x in cand], np.int64)
        if cand.size == 0:
            continue
        info["labels"] += 1
        if cand.size != 4:
            info["more_than_4" if cand.size > 4 else "fewer_than_4"] += 1
        key = -upa[cand]
        order = np.argsort(key, kind="stable")
        ks = key[order]
        top = ks[:5]
        if np.any(top[1:] == top[:-1]) or np.any(top != top):
            info["ties"] = True
        sel = cand[order][:4]
        key2 = -upa[ds_a[sel]]
        if np.unique(key2).size != key2.size or np.any(key2 != key2):
            info["ties"] = True
        sel = sel[np.argsort(key2, kind="stable")]
        int_ds = lab0
        step = 10 ** (depth - d0)
        for i, x in enumerate(sel.tolist()):
            idxs.append(x)
            seen.add(x)
            x1 = us[int(ds_a[x])]
            sub = lab0 + (i * 2 + 1) * step
            paint_up(x, sub)
            if d0 < depth:
                labs.append((sub, d0 + 1))
            if x1 in seen:
                info["already_listed"] += 1
                continue
            idxs.append(x1)
            seen.add(x1)
            pint = lab0 + (i + 1) * 2 * step
            cells = painted.setdefault(pint, [])
            branch[x1] = pint
            cells.append(x1)
            while True:
                x1 = us[x1]
                if x1 == -1 or branch[x1] != int_ds:
                    break
                branch[x1] = pint
                cells.append(x1)
            int_ds = pint
            if d0 < depth:
                labs.append((pint, d0 + 1))
    out = branch.copy()
    for x, y in zip(seq_a.tolist(), ds_a[seq_a].tolist()):  # core.fillnodata_upstream
        if out[x] == 0 and out[y] != 0:
            out[x] = out[y]
    return (out % 10**depth).astype(np.int32), idxs, info


def pfaf_ties(pits, ds, seq, us_main, uparea, mask, depth, mv=-1):
    """True when the Pfafstetter case holds a tie among the sort keys that decide a selection or an order: the
    reference's unstable sorts may then answer differently, and the case is not recorded."""
    return _ref_pfafstetter(pits, ds, seq, us_main, uparea, mask, depth, mv)[2]["ties"]


# ---- the inputs of a case without the reference and without a GPU ----------------------------------------------------
def graph(raster, O):
    """(d8, idxs_ds, idxs_pit, idxs_seq) of a case raster from the CPU oracle ``O``."""
    d8 = d8_of(raster)
    ds, pits, _ = O.from_array(d8)
    return d8, ds, pits, O.idxs_seq(ds, pits)


def areas(O, ds, seq, shape, transform, latlon):
    """{"cell": the upstream cell count, "km2": the upstream area in km2} as FlwdirRaster.upstream_area gives them."""
    from pyflwdir_amd import gis
    from pyflwdir_amd._affine import Affine

    out = {}
    for unit in UPAREAS:
        if unit == "cell":
            a = np.ones(ds.size, np.int32)
        else:
            a = np.ascontiguousarray(gis.area_grid(Affine(*transform), shape, latlon, unit="m2").ravel() / gis.AREA_FACTORS[unit])
        upa = O.accuflux(ds, seq, a, nodata=-9999)
        upa[ds == -1] = -9999
        out[unit] = upa.reshape(shape)
    return out
