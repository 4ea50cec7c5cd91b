"""The restated loops of tests/window_cases.py against the reference's recorded outputs (tests/golden/wide_window.npz,
tools/gen_golden_window.py), bit for bit (NaNs count as equal when they sit in the same positions), on inputs from the CPU
oracle that the record's digests pin to what the reference derived itself — and that the cases reach the edges the device
code can get wrong.  No GPU."""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_cases as WC  # noqa: E402
from golden_util import digest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_graphs = {}


@pytest.fixture(scope="module", autouse=True)
def surface():
    """The four calls stand in every layer — header, binding, front end — before any case is looked at."""
    from pyflwdir_amd import _hip
    from pyflwdir_amd.raster import FlwdirRaster

    header = open(os.path.join(ROOT, "include", "pfd.h")).read()
    for sym in ("pfd_downstream", "pfd_moving_average", "pfd_moving_median", "pfd_path", "pfd_debug_window_wmax"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header) and sym in _hip.SYMBOLS, sym
    for method in ("downstream", "moving_average", "moving_median", "path"):
        assert callable(getattr(FlwdirRaster, method, None)), method


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(WC.GOLD, WC.RECORD))


def graph(G, oracle, raster, grid):
    """(Graph, Strahler order) of a case from the oracle, in the reference's index dtype, checked against the record's
    input digests; the step lengths of the grid in float64."""
    from pyflwdir_amd import gis
    from pyflwdir_amd._affine import Affine

    if (raster, grid) not in _graphs:
        O = oracle
        d8 = WC.d8_of(raster)
        tr, latlon = WC.transform_of(raster, grid)
        mv = G[f"mv_{raster}"][()]
        ds, pits, _ = O.from_array(d8)
        seq = O.idxs_seq(ds, pits)
        upa = O.accuflux(ds, seq, np.ones(ds.size, np.int32), nodata=-9999)
        upa[ds == -1] = -9999
        us = O.main_upstream(ds, upa).astype(mv.dtype)
        strord = O.strahler_order(ds, seq)
        assert digest(us) == str(G[f"usmain_{raster}"])
        assert digest(strord.reshape(d8.shape)) == str(G[f"strord_{raster}"])
        steps = gis.step_length_table(d8.shape[0], latlon, Affine(*tr), dtype=np.float64)
        _graphs[raster, grid] = WC.Graph(ds.astype(mv.dtype), us, mv, d8.shape, steps), strord
    return _graphs[raster, grid]


def recorded(G, raster, name, got):
    got = WC.canon(got)
    if raster in WC.FULL:
        exp = G[f"out_{name}"]
        return got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    return digest(got) == str(G[f"digest_{name}"])


@pytest.mark.parametrize("raster", WC.RASTERS)
def test_restated_window_loops_reproduce_the_record(G, oracle, raster):
    g, strord = graph(G, oracle, raster, "ll")
    inp = WC.inputs(g.n)
    for name, method, kw in WC.window_calls(raster):
        res = WC.run_window(g, method, inp, kw, strord).reshape(g.shape)
        assert recorded(G, raster, f"{raster}_{name}", res), (raster, name)
        if res.dtype.kind == "f":
            assert int(np.count_nonzero(np.isnan(res))) == int(G[f"nan_{raster}_{name}"])


@pytest.mark.parametrize("raster", WC.RASTERS)
@pytest.mark.parametrize("grid", WC.GRIDS)
def test_restated_path_loop_reproduces_the_record(G, oracle, raster, grid):
    g, _ = graph(G, oracle, raster, grid)
    inp = WC.inputs(g.n)
    starts = G[f"starts_{raster}"]
    assert np.array_equal(starts, WC.path_starts(g.ds, g.us, -1, inp["mask"]))
    for name, kw in WC.path_calls(raster, grid):
        kw = dict(kw)
        mask = inp[kw.pop("mask")] if "mask" in kw else None
        paths, dists = WC.path(g, starts, mask=mask, **kw)
        cells, lens = WC.flat_paths(paths, g.idx_dtype)
        pre = f"{raster}_{grid}_path_{name}"
        assert recorded(G, raster, pre + "_cells", cells), pre
        assert recorded(G, raster, pre + "_lens", lens), pre
        assert recorded(G, raster, pre + "_dists", dists), pre


def test_the_record_is_small():
    assert os.path.getsize(os.path.join(WC.GOLD, WC.RECORD)) < 1 << 20


def test_the_cases_reach_the_edges(G, oracle):
    seen = set()
    for raster in WC.RASTERS:
        g, strord = graph(G, oracle, raster, "ll")
        inp = WC.inputs(g.n)
        st, so = {}, {}
        WC.windows(g, 3, None, st)
        WC.windows(g, 3, strord, so)
        if st["pit"]:
            seen.add("window cut by a pit")
        if st["headwater"]:
            seen.add("window cut by a headwater")
        if so["strord"]:
            seen.add("window cut by the stream-order rule")
        nodata_cells = np.flatnonzero(g.ds < 0)
        win = WC.windows(g, 3)
        live = nodata_cells[inp["data32"][nodata_cells] != np.float32(WC.NODATA)]
        if live.size and np.all(np.count_nonzero(win[live] >= 0, axis=1) == 1):
            seen.add("window of one cell on a nodata flow cell")
        for name, method, kw in WC.window_calls(raster):
            if method == "downstream":
                continue
            s = {}
            res = WC.run_window(g, method, inp, kw, strord, s)
            nan_nd = np.isnan(kw.get("nodata", WC.NODATA))
            if method == "median" and s["empty"]:
                seen.add("all-nodata window: NaN median")
            if method == "median" and s["odd"] and s["even"]:
                seen.add("even and odd count")
            if method == "average" and s["w0"]:
                seen.add("w == 0")
                if "weights" not in kw and nan_nd:
                    seen.add("all-nodata window: nodata mean")
            del res
    for raster in WC.RASTERS:
        for grid in WC.GRIDS:
            g, _ = graph(G, oracle, raster, grid)
            starts = G[f"starts_{raster}"]
            for name, kw in WC.path_calls(raster, grid):
                if "max_length" not in kw or "mask" in kw:
                    continue
                s = {}
                cut = WC.path(g, starts, stats=s, **kw)[0]
                free = WC.path(g, starts, **{k: v for k, v in kw.items() if k != "max_length"})[0]
                if s["max_length"] and any(len(a) + 1 <= len(b) and np.array_equal(a, b[:len(a)]) for a, b in zip(cut, free)):
                    seen.add("max_length stops a path short (%s)" % kw.get("unit", "cell"))
    want = {"window cut by a pit", "window cut by a headwater", "window cut by the stream-order rule",
            "window of one cell on a nodata flow cell", "all-nodata window: NaN median", "all-nodata window: nodata mean",
            "even and odd count", "w == 0", "max_length stops a path short (cell)", "max_length stops a path short (m)"}
    assert want - seen == set()


def test_max_length_stops_one_step_short(G, oracle):
    """With max_length = 5 cells a path that would be longer holds exactly 6 cells and the distance 5.0: the step that
    would make the distance exceed max_length is not taken."""
    g, _ = graph(G, oracle, "flwdir_large", "ll")
    starts = G["starts_flwdir_large"]
    cut, dcut = WC.path(g, starts, max_length=5)
    free, _ = WC.path(g, starts)
    longer = [i for i in range(len(cut)) if len(free[i]) > 6]
    assert longer and all(len(cut[i]) == 6 and dcut[i] == 5.0 for i in longer)
    half, dhalf = WC.path(g, starts, direction="up", max_length=2.5)
    assert max(len(p) for p in half) == 3 and dhalf.max() == 2.0


def test_the_start_list_holds_the_special_cells(G, oracle):
    for raster in WC.RASTERS:
        g, _ = graph(G, oracle, raster, "ll")
        starts = G[f"starts_{raster}"]
        mask = WC.inputs(g.n)["mask"]
        idx = np.arange(g.n)
        assert np.any(g.ds[starts] == idx[starts]), "a pit"
        assert np.any((g.ds[starts] >= 0) & (g.us[starts] < 0)), "a headwater"
        assert np.any(g.ds[starts] < 0), "a nodata cell"
        assert np.any(mask[starts] & (g.ds[starts] >= 0)), "a masked cell"
        assert np.unique(starts).size < starts.size, "a repeated cell"


def test_the_library_exports_the_calls():
    """The built library holds the entry points the header declares, and the bound between the two median forms."""
    from pyflwdir_amd import _hip

    L = _hip.lib()
    for sym in ("pfd_downstream", "pfd_moving_average", "pfd_moving_median", "pfd_path"):
        assert hasattr(L, sym)
    assert _hip.window_wmax(np.float32) == 31 and _hip.window_wmax(np.float64) == 15
