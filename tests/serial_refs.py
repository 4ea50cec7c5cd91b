"""Restatements of the reference's serial loops over ``idxs_ds`` and a cell sequence, shared by the GPU tests:
fillnodata (core.fillnodata_upstream / _downstream, core.py:120-188), the three outlet loops (basins.py:67-103,
core.py:501-514, regions.py:129-163), upstream_sum (arithmetics.py:147-169), ucat_area (subgrid.py:51-93), floodplains
(dem.py:333-379) and snap with its step length (core.py:308-366, 440-480, gis_utils.py:415-486).  They take any graph and
any sequence, so they answer general graphs and an installed sort order as well as D8 rasters.
tests/test_serial_refs.py pins the last five to the reference's recorded outputs."""
from __future__ import annotations

import math

import numpy as np


# ---- fillnodata: numpy arrays in, so that sums and comparisons happen in the payload's dtype --------------------------
def _ref_up(idxs_ds, seq, data, nodata):
    out = data.copy()
    for x in seq:
        d = idxs_ds[x]
        if out[x] == nodata and out[d] != nodata:
            out[x] = out[d]
    return out


def _ref_down(idxs_ds, seq, data, nodata, how):
    out = data.copy()
    for x in seq[::-1]:
        d = idxs_ds[x]
        if d == x:
            continue
        if data[d] == nodata and out[x] != nodata:
            if out[d] == nodata:
                out[d] = out[x]
            elif how == "max":
                out[d] = max(out[x], out[d])
            elif how == "min":
                out[d] = min(out[x], out[d])
            else:
                out[d] += out[x]
    return out


# ---- outlets (plain lists: several times faster than numpy scalars) ----------------------------------------------------
def _ref_streamorder(ds, seq, strord, min_sto):
    if min_sto < 0:
        min_sto = max(strord) + min_sto
    sub, idxs = [0] * len(ds), []
    for x in seq[::-1]:
        if strord[x] >= min_sto and (ds[x] == x or strord[ds[x]] != strord[x]):
            idxs.append(x)
            sub[x] = len(idxs)
    for x in seq:  # (core.fillnodata_upstream)
        if sub[x] == 0 and sub[ds[x]] != 0:
            sub[x] = sub[ds[x]]
    return sub, idxs


def _ref_outflow(ds, seq, region):
    mask, idxs = [True] * len(ds), []
    for x in seq:
        if mask[ds[x]] and region[x] and (ds[x] == x or not region[ds[x]]):
            idxs.append(x)
            mask[x] = False
        else:
            mask[x] = mask[ds[x]]
    return idxs


def _ref_outlets(ds, seq, regions):
    lbs, idxs = [], []
    for x in seq[::-1]:
        if regions[x] > 0 and (ds[x] == x or regions[ds[x]] != regions[x]):
            idxs.append(x)
            lbs.append(regions[x])
    return lbs, idxs


# ---- upstream_sum: one loop over ascending cell index; sums and the nodata test in the payload's dtype ----------------
def _ref_upstream_sum(idxs_ds, data, nodata, mv):
    out = np.zeros(data.size, data.dtype)
    ds = idxs_ds.tolist()
    mv = int(mv)
    with np.errstate(over="ignore"):  # (integer adds wrap silently, as the compiled reference's do)
        for i in range(data.size):
            d = ds[i]
            if d != mv and d != i:
                if data[i] == nodata or data[d] == nodata:
                    out[i] = nodata
                else:
                    out[d] += data[i]
    return out


# ---- ucat_area: labels i + 1 from the outlets upstream; areas added in sequence order in the dtype of `area` ------------
def _ref_ucat_area(idxs_out, idxs_ds, seq, area, mv):
    ucat_map = [0] * idxs_ds.size
    ucat_are = np.full(idxs_out.size, -9999, area.dtype)
    ds = idxs_ds.tolist()
    mv = int(mv)
    for i, x in enumerate(idxs_out.tolist()):
        if x != mv:
            ucat_map[x] = i + 1  # (of a repeated outlet the last entry owns the cell; every entry starts with the cell's area)
            ucat_are[i] = area[x]
    with np.errstate(over="ignore"):
        for x in seq.tolist():
            u = ucat_map[ds[x]]
            if ucat_map[x] == 0 and u != 0:
                ucat_map[x] = u
                ucat_are[u - 1] += area[x]
    return np.array(ucat_map, idxs_ds.dtype), ucat_are


# ---- floodplains: the drain's elevation and height are float32 whatever the elevation's dtype --------------------------
def _ref_floodplains(idxs_ds, seq, elevtn, uparea, upa_min, b):
    drainh = np.full(uparea.size, -9999.0, np.float32)
    drainz = np.full(uparea.size, -9999.0, np.float32)
    fldpln = np.full(uparea.size, -1, np.int8)
    fldpln[seq] = 0
    ds = idxs_ds.tolist()
    with np.errstate(invalid="ignore", over="ignore"):
        for x in seq.tolist():
            if uparea[x] >= upa_min:
                drainh[x] = uparea[x] ** b
                drainz[x] = elevtn[x]
                fldpln[x] = 1
            elif fldpln[ds[x]] == 1:
                z0, h0 = drainz[ds[x]], drainh[ds[x]]
                dh = elevtn[x] - z0  # (numpy scalars: float32 - float32 stays float32, float64 - float32 is float64)
                if dh <= h0:
                    fldpln[x] = 1
                    drainz[x] = z0
                    drainh[x] = h0
    return fldpln


# ---- snap: one walk per start cell along `idxs_nxt` (downstream cells, or main upstream cells with `mv` for none) ---------
def _ref_step_length_f64(idx0, idx1, ncol, latlon, transform):
    """Length of the step idx0 -> idx1 as a Python float: metres on a lat/lon grid; on a projected one the reference takes
    the row step from xres and the column step from yres, which is part of what it computes."""
    xres, yres, north = transform[0], transform[4], transform[5]
    r0, r1 = idx0 // ncol, idx1 // ncol
    dr = abs(r1 - r0)
    dc = abs(idx1 % ncol - idx0 % ncol)
    if latlon:
        lat = north + (r0 + r1) / 2.0 * yres
        rad = np.radians(lat)
        dy = dx = 0.0
        if dr != 0:
            dy = (111132.92 + (-559.82 * np.cos(2.0 * rad)) + (1.175 * np.cos(4.0 * rad)) + (-0.0023 * np.cos(6.0 * rad))) * yres
        if dc != 0:
            dx = ((111412.84 * np.cos(rad)) + (-93.5 * np.cos(3.0 * rad)) + (0.118 * np.cos(5.0 * rad))) * xres
    else:
        dy, dx = xres, yres
    return math.hypot(dy * dr, dx * dc)


def _ref_snap(idxs0, idxs_nxt, mv, mask, max_length, step):
    """``step(idx0, idx1)`` is 1.0 (cells) or the float64 length of the step.  The reference never returns from a walk
    round a cycle; a walk of more than n + 1 hops is therefore an error of the caller's inputs and raises."""
    idxs = np.full(idxs0.size, mv, idxs0.dtype)
    dists = np.zeros(idxs0.size, np.float32)
    nxt = idxs_nxt.tolist()
    mv = int(mv)
    cap = idxs_nxt.size + 1
    for i, x in enumerate(idxs0.tolist()):
        dist, hops = 0.0, 0
        while mask is None or not mask[x]:
            y = nxt[x]
            if y == x or y == mv:  # a pit, a nodata cell, or no main upstream cell
                break
            d = step(x, y)
            if max_length is not None and dist + d > max_length:
                break
            dist += d
            x = y
            hops += 1
            if hops >= cap:
                raise RuntimeError(f"_ref_snap: start {i} walks round a cycle")
        idxs[i] = x
        dists[i] = dist  # (a Python float, rounded to float32 here)
    return idxs, dists
