"""The restated loops of tests/subgrid_riv_cases.py against the reference's recorded outputs
(tests/golden/wide_subgrid_riv.npz, tools/gen_golden_subgrid_riv.py), bit for bit (NaNs count as equal when they sit in the
same positions), on inputs from the CPU oracle that the record's digests pin to what the reference derived itself — and that
the cases reach the edges the device code can get wrong.  No GPU."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subgrid_riv_cases as SC  # noqa: E402
from golden_util import digest  # noqa: E402

_graphs = {}


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(SC.GOLD, SC.RECORD))


def graph(G, oracle, raster, grid):
    """The raster of a case from the oracle, in the reference's index dtype, checked against the record's input digests."""
    from pyflwdir_amd import gis
    from pyflwdir_amd._affine import Affine

    if (raster, grid) not in _graphs:
        O = oracle
        d8 = SC.d8_of(raster)
        tr, latlon = SC.transform_of(raster, grid)
        mv = G[f"mv_{raster}"][()]
        ds, pits, _ = O.from_array(d8)
        seq = O.idxs_seq(ds, pits)
        upa = O.accuflux(ds, seq, np.ones(ds.size, np.int32), nodata=-9999)
        upa[ds == -1] = -9999
        us = O.main_upstream(ds, upa).astype(mv.dtype)
        distnc = O.stream_distance(ds, seq, d8.shape[1], real_length=True, latlon=latlon, transform=tr)
        dcell = O.stream_distance(ds, seq, d8.shape[1], real_length=False)
        rows = np.ascontiguousarray(gis.area_rows(Affine(*tr), d8.shape, latlon, unit="m2") / gis.AREA_FACTORS["m2"])
        assert digest(us) == str(G[f"usmain_{raster}"])
        assert digest(dcell.reshape(d8.shape)) == str(G[f"distcell_{raster}"])
        assert digest(distnc.reshape(d8.shape)) == str(G[f"distnc_{raster}_{grid}"])
        assert digest(rows) == str(G[f"area_{raster}_{grid}"])
        _graphs[raster, grid] = SC.Graph(ds.astype(mv.dtype), us, seq, mv, d8.shape, distnc, dcell, rows), ds
    return _graphs[raster, grid]


def recorded(G, raster, key, name, got):
    got = SC.canon(got)
    if raster in SC.FULL:
        exp = G[f"out_{key}_{name}"]
        return got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    return digest(got) == str(G[f"digest_{key}_{name}"])


def outlets_of(G, g, key, variant):
    return np.arange(g.n, dtype=np.intp).reshape(g.shape) if variant == "none" else G[f"outlets_{key}"]


@pytest.mark.parametrize("key,raster,grid,cellsize,variant", SC.configs())
def test_restated_loops_reproduce_the_record(G, oracle, key, raster, grid, cellsize, variant):
    g, _ = graph(G, oracle, raster, grid)
    idxs_out = outlets_of(G, g, key, variant)
    inp = SC.inputs(g.n)
    for name, method, kw in SC.calls(variant):
        res = SC.run(g, method, idxs_out, inp, kw)
        if method == "volume":
            assert recorded(G, raster, key, "ucatmap", res[0].astype(G[f"mv_{raster}"].dtype).reshape(g.shape)), (key, name, "map")
            res = res[1].reshape((res[1].shape[0], *idxs_out.shape))
        else:
            res = res.reshape(idxs_out.shape)
        assert recorded(G, raster, key, name, res), (key, name)
        assert int(np.count_nonzero(np.isnan(res))) == int(G[f"nan_{key}_{name}"])


def test_the_record_is_small():
    assert os.path.getsize(os.path.join(SC.GOLD, SC.RECORD)) < 1 << 20


def test_the_masked_slope_equals_the_unmasked_one(G):
    """The interpreted reference never honours the mask of its slope loops."""
    for key, raster, *_ in SC.configs():
        if f"nan_{key}_rivslp_both_1000_mask" not in G.files:
            continue
        pre = "out" if raster in SC.FULL else "digest"
        a, b = G[f"{pre}_{key}_rivslp_both_1000"], G[f"{pre}_{key}_rivslp_both_1000_mask"]
        assert a.tobytes() == b.tobytes()


def test_the_cases_reach_the_edges(G, oracle):
    seen = set()
    for key, raster, grid, cellsize, variant in SC.configs():
        g, ds = graph(G, oracle, raster, grid)
        idxs_out = outlets_of(G, g, key, variant)
        inp = SC.inputs(g.n)
        if int(G[f"nan_{key}_rivmed_up"]) > 0:
            seen.add("all-nodata median segment")
        cnt = SC.segment_median(g, idxs_out, "up", inp["data32"])[1]
        if np.any((cnt > 0) & (cnt % 2 == 0)) and np.any(cnt % 2 == 1):
            seen.add("even and odd median count")
        offs, cells, out = SC.walk_segments(g, idxs_out, "up")
        slp = SC.segment_slope(g, idxs_out, "up", inp["elev64"], g.distnc)
        one = np.flatnonzero(np.diff(offs) == 1)
        if one.size and np.all(slp[one] == 0.0):
            seen.add("one-cell segment, slope 0.0")
        st = {}
        SC.walk_segments(g, idxs_out, "down", inp["mask"], stats=st)
        SC.walk_segments(g, idxs_out, "up", None, onto=True, stats=st)
        for why in ("mask", "pit", "missing", "outlet"):
            if st[why]:
                seen.add("walk stopped by " + why)
        if st["longest"] > 64:
            seen.add("walk longer than 64 steps")
        if variant != "none":
            fs = {}
            SC.fixed_length_slope(g, idxs_out, inp["elev32"], g.distnc, 2000, fs)
            if fs["cut_pit"]:
                seen.add("fixed_length_slope cut short at a pit")
            if fs["cut_head"]:
                seen.add("fixed_length_slope cut short at a headwater")
        lab = SC.ucat_map(g, idxs_out, np.int64)[0]
        r, c = np.divmod(np.flatnonzero(lab > 0), g.shape[1])
        tiles = np.unique(np.stack([lab[lab > 0], (r // 64) * 4096 + c // 64], 1), axis=0)
        if np.any(np.bincount(tiles[:, 0]) > 1):
            seen.add("label over more than one 64 x 64 tile")
        valid = [c for c in out if c is not None]
        if np.any(ds[valid] == np.asarray(valid)):
            seen.add("outlet on a pit")
        if any(c is None for c in out) and len(set(valid)) < len(valid):
            seen.add("missing and repeated outlet")
    want = {"all-nodata median segment", "even and odd median count", "one-cell segment, slope 0.0", "walk stopped by mask",
            "walk stopped by pit", "walk stopped by missing", "walk stopped by outlet", "walk longer than 64 steps",
            "fixed_length_slope cut short at a pit", "fixed_length_slope cut short at a headwater",
            "label over more than one 64 x 64 tile", "outlet on a pit", "missing and repeated outlet"}
    assert want - seen == set()
