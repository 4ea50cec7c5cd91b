"""The stream-segment golden cases (tests/golden/wide_streams.npz, written by tools/gen_golden_streams.py): rasters,
masks, ``max_len`` values and the keys of the records, and ``_ref_streams``, a plain restatement of the reference's
serial loop (pyflwdir/streams.py:154-188) — shared by the generator (which runs the reference), tests/
test_stream_cases.py (CPU) and tests/test_gpu_streams.py (device)."""
from __future__ import annotations

import os

import numpy as np

import outlet_cases as OC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIPS = ["synth_onecol_300x1", "synth_onerow_1x300"]  # one cell wide: segments of up to 35 cells, cut by max_len
RASTERS = OC.RASTERS + STRIPS
GENERAL = OC.GENERAL  # graphs of tests/golden/wide_general.npz
FULL = set(OC.FULL) | set(STRIPS)  # outputs in full; the others: digests
MASKS = ["none", "sto2", "sto4", "blob"]  # "blob" is not closed downstream: W reaches beyond the mask
MAX_LEN = [0, 1, 2, 3, 7]
FEATURE_RASTERS = ["flwdir0", "synth_tiny_5x7"]
TRANSFORM = (0.25, 0.0, 5.0, 0.0, -0.5, 60.0)  # of the recorded features


def mask_of(kind, strahler, shape):
    """Flat boolean mask of one case (None for "none") from the flat Strahler order."""
    if kind == "none":
        return None
    if kind == "blob":
        return OC.region(shape, "blob").ravel()
    return np.asarray(strahler).ravel() >= int(kind[3:])


def key(raster, mask, max_len):
    return f"{raster}_{mask}_{max_len}"


def cases(raster):
    return [(key(raster, m, ml), m, ml) for m in MASKS for ml in MAX_LEN]


def flatten(segs, dtype):
    """(lengths int32[k], concatenated indices) of a list of segments — what a record holds."""
    lens = np.fromiter((len(s) for s in segs), np.int32, len(segs))
    flat = np.concatenate([np.asarray(s, dtype) for s in segs]) if len(segs) else np.empty(0, dtype)
    return lens, flat.astype(dtype, copy=False)


def unflatten(lens, flat):
    ends = np.cumsum(lens)
    return [flat[b - l:b] for l, b in zip(lens.tolist(), ends.tolist())]


def upstream_count(ds, mask, mv):
    """core.upstream_count (core.py:50-61) with numpy: upstream neighbours inside the mask; -9 on nodata."""
    ds = np.asarray(ds)
    n = ds.size
    idx = np.arange(n)
    src = (ds != mv) & (ds != idx)
    if mask is not None:
        src &= np.asarray(mask, bool)
    nup = np.bincount(ds[src].astype(np.int64), minlength=n).astype(np.int64)
    nup[ds == mv] = -9
    return nup


def _ref_streams(ds, seq, mask, max_len, mv=-1):
    """streams.streams (streams.py:154-188) on plain lists: list of lists of linear indices."""
    nup = upstream_count(ds, mask, mv).tolist()
    ds = np.asarray(ds).tolist()
    mask = None if mask is None else np.asarray(mask, bool).tolist()
    out = []
    done = [False] * len(ds)
    for idx0 in np.asarray(seq)[::-1].tolist():
        if done[idx0] or (mask is not None and not mask[idx0]):
            continue
        idxs = [idx0]
        while True:
            done[idx0] = True
            idx_ds = ds[idx0]
            pit = idx_ds == idx0
            if not pit:
                idxs.append(idx_ds)
            if nup[idx_ds] > 1 or pit:
                l = len(idxs)
                if l > max_len > 0:
                    n, k = l, 1
                    if (l / max_len) > 1.5:
                        k = round(l / max_len)
                        n = round(l / k)
                    for i in range(k):
                        out.append(idxs[i * n:] if i + 1 == k else idxs[i * n:n * (i + 1) + 1])
                else:
                    out.append(idxs)
                if pit:
                    out.append([idx_ds, idx_ds])
                break
            idx0 = idx_ds
    return out


def inputs(raster, O=None):
    """(idxs_ds, idxs_seq, flat Strahler order, shape) of a case raster without the reference and without a GPU: the
    recorded graph of a general case, else the CPU oracle ``O`` on the raster's D8 codes."""
    if raster in GENERAL:
        W = np.load(os.path.join(GOLD, "wide_general.npz"))
        shape = W["in_flwdir0_nextxy"].shape[1:]
        return W[f"out_{raster}_idxs_ds"], W[f"out_{raster}_idxs_seq"], W[f"out_{raster}_strahler"].ravel(), shape
    d8 = np.load(os.path.join(GOLD, raster + ".npz"))["d8"]
    ds, pits, _ = O.from_array(d8)
    seq = O.idxs_seq(ds, pits)
    return ds, seq, O.strahler_order(ds, seq).ravel(), d8.shape


def feature_record(feats, columns):
    """A list of geo-features as arrays: coordinates [M, 2] float64, points per feature, idx, idx_ds, pit, columns."""
    coords = np.array([c for f in feats for c in f["geometry"]["coordinates"]], np.float64).reshape(-1, 2)
    rec = dict(coords=coords, npts=np.array([len(f["geometry"]["coordinates"]) for f in feats], np.int32))
    for name in ("idx", "idx_ds", "pit") + tuple(columns):
        rec[name] = np.array([f["properties"][name] for f in feats])
    return rec


def feature_calls():
    """(tag, columns) of the recorded feature lists per raster of FEATURE_RASTERS."""
    return [("streams_sto2", ("strord", "uparea")), ("vectorize", ()), ("vectorize_up", ("strord",))]
