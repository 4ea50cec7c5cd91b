"""Restatements of the reference's serial loops over ``idxs_ds`` and a cell sequence, shared by the GPU tests:
fillnodata (core.fillnodata_upstream / _downstream, core.py:120-188) and the three outlet loops (basins.py:67-103,
core.py:501-514, regions.py:129-163).  They take any graph and any sequence, so they answer general graphs and an
installed sort order as well as D8 rasters."""
from __future__ import annotations


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
