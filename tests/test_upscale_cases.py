"""The restated serial loops of tests/upscale_cases.py against the reference's recorded outputs (tests/golden/
wide_upscale.npz, tools/gen_golden_upscale.py), the flow-error counts of the reference's own test, and the edges the
cases and the random rasters of tests/test_gpu_upscale.py must reach.  No GPU."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upscale_cases as UC  # noqa: E402
from golden_util import digest  # noqa: E402

_graphs, _areas, _results = {}, {}, {}


def graph(raster):
    if raster not in _graphs:
        tr, latlon = UC.transform_of(raster)
        _graphs[raster] = UC.HostGraph(UC.d8_of(raster), tr, latlon)
    return _graphs[raster]


def area(raster, kind):
    return UC.uparea_of(graph(raster), kind, _areas.setdefault(raster, {}))


def result(key, raster, kind, cellsize, method):
    """(coarse idxs_ds, idxs_out, error map, stats) of the restated loops, computed once."""
    k = (key, method)
    if k not in _results:
        g, stats = graph(raster), {}
        ds1, out = UC.upscale(g.idxs_ds, area(raster, kind), g.shape, cellsize, method, g.mv, stats)
        _results[k] = (ds1, out, UC.upscale_error(g.idxs_ds, out, ds1, g.mv), stats)
    return _results[k]


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(UC.GOLD, "wide_upscale.npz"))


def recorded(G, raster, name, got):
    got = np.asarray(got)
    if raster in UC.FULL:
        exp = G[f"out_{name}"]
        return got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    return digest(got) == str(G[f"digest_{name}"])


@pytest.mark.parametrize("key,raster,kind,cellsize", UC.keys())
def test_restated_loops_reproduce_the_record(G, key, raster, kind, cellsize):
    g = graph(raster)
    upa = area(raster, kind)
    assert digest(upa) == str(G[f"upa_{raster}_{kind}"])  # the area the reference was run with
    shape1 = UC.coarse_shape(g.shape, cellsize)
    for m in UC.METHODS:
        if f"raises_{key}_{m}" in G.files:  # (one coarse cell: no raster; the outlets below are still recorded)
            assert shape1 == (1, 1)
            continue
        ds1, out, err, _ = result(key, raster, kind, cellsize, m)
        assert UC.network_valid(ds1, g.mv)
        assert recorded(G, raster, f"{key}_{m}_ds", ds1), (key, m, "idxs_ds")
        assert recorded(G, raster, f"{key}_{m}_idxs", out.reshape(shape1)), (key, m, "idxs_out")
        assert recorded(G, raster, f"{key}_{m}_err", err.reshape(shape1)), (key, m, "upscale_error")
        assert int(G[f"nerr_{key}_{m}"]) == np.count_nonzero(err == 0)
        assert int(G[f"far_{key}_{m}"]) == UC.far_links(ds1, shape1, g.mv)
    for m in ("eam_plus", "dmm"):
        got = UC.ucat_outlets(g.idxs_ds, upa, g.shape, cellsize, m, g.mv).reshape(shape1)
        assert recorded(G, raster, f"{key}_{m}_ucat", got), (key, m, "ucat_outlets")


def test_flow_error_counts_of_the_reference_test(G):
    """The reference's own test (tests/test_upscale.py:20-24) expects 33 / 4 / 2 erroneous cells for dmm / eam / eam_plus
    on this raster at cellsize 20; the record and the restated loops agree with it."""
    for m, n in (("dmm", 33), ("eam", 4), ("eam_plus", 2)):
        assert int(G[f"nerr_flwdir_large_cell_20_{m}"]) == n
        assert np.count_nonzero(result("flwdir_large_cell_20", "flwdir_large", "cell", 20, m)[2] == 0) == n


def test_literal_scan_agrees_with_the_sort():
    """The arg-max by a sort is the serial scan (ascending index, strict >), on every small case and both selectors."""
    for key, raster, kind, cellsize in UC.keys():
        if raster in UC.FULL:
            g = graph(raster)
            grid = UC.Grid(g.idxs_ds, g.shape, cellsize, g.mv)
            for sel in ("edge", "effarea"):
                upa = area(raster, kind)
                assert np.array_equal(UC.rep_cells(grid, upa, sel), UC.rep_cells(grid, upa, sel, scan=True)), (key, sel)


def test_cases_reach_the_edges():
    """A partial last cell, an all-nodata coarse cell, a pit taken as representative outside the selector, a coarse link
    from the first effective area (the fallback of ihu_nextidx), a link outside the 8 neighbours, and the tie."""
    seen = dict(partial=0, empty=0, pit_outside=0, fallback=0, far=0)
    for key, raster, kind, cellsize in UC.keys():
        g = graph(raster)
        grid = UC.Grid(g.idxs_ds, g.shape, cellsize, g.mv)
        seen["partial"] += g.shape[0] % cellsize != 0 and g.shape[1] % cellsize != 0
        for sel in ("edge", "effarea"):
            rep = UC.rep_cells(grid, area(raster, kind), sel)
            seen["empty"] += int(np.count_nonzero(rep == g.mv))
            has = rep[rep != g.mv]
            seen["pit_outside"] += int(np.count_nonzero(grid.pit[has] & ~grid.selector(sel)[has]))
        if UC.coarse_shape(g.shape, cellsize) != (1, 1):
            ds1, _, _, stats = result(key, raster, kind, cellsize, "eam_plus")
            seen["fallback"] += len(stats.get("fallback", []))
            seen["far"] += sum(UC.far_links(result(key, raster, kind, cellsize, m)[0], grid.shape1, g.mv) for m in UC.METHODS)
    assert all(seen.values()), seen
    # an all-nodata coarse cell is missing in every output and 255 in the error map
    key, raster, kind, cellsize = [k for k in UC.keys() if k[1] == "synth_rough_nodata_384x512"][0]
    ds1, out, err, _ = result(key, raster, kind, cellsize, "eam_plus")
    g = graph(raster)
    grid = UC.Grid(g.idxs_ds, g.shape, cellsize, g.mv)
    empty = np.bincount(grid.coarse[grid.valid], minlength=grid.n1) == 0
    assert empty.any() and np.all(ds1[empty] == g.mv) and np.all(out[empty] == g.mv) and np.all(err[empty] == 255)


def test_tie_case_holds_a_tie():
    g = graph(UC.TIE)
    grid = UC.Grid(g.idxs_ds, g.shape, 4, g.mv)
    upa = area(UC.TIE, "cell")
    assert UC.tied_cells(grid, upa, "edge") >= 3 and UC.tied_cells(grid, upa, "effarea") >= 3
    # the smallest index among the equals: the channel along row 0, not the one along row 3
    assert list(UC.rep_cells(grid, upa, "edge")[:3]) == [3, 7, 11]


def test_cyclic_case_is_cyclic():
    assert not graph(UC.CYCLIC).acyclic


def test_random_rasters_complete():
    """At least three quarters of the random cases of tests/test_gpu_upscale.py give a valid coarse network for every
    method by the restated loops alone (the others expect a ValueError on the device), and they hold ties, NaN areas,
    empty coarse cells, pits next to nodata taken outside the selector, and both arg-max kernels' cell sizes."""
    from test_gpu_fuzz import random_d8

    done = total = ties = empty = pit_outside = nan = 0
    for shape, cellsize, seed in UC.fuzz_cases():
        d8, areas = UC.fuzz_raster(random_d8, shape, seed, cellsize)
        assert 0.15 < np.mean(d8 == 247) < 0.35
        g = UC.HostGraph(d8)
        assert g.acyclic
        upa = areas(g.upstream_area().ravel())
        nan += int(np.isnan(upa).any()) if upa.dtype.kind == "f" else 0
        grid = UC.Grid(g.idxs_ds, g.shape, cellsize, g.mv)
        for sel in ("edge", "effarea"):
            ties += UC.tied_cells(grid, upa, sel)
            rep = UC.rep_cells(grid, upa, sel)
            empty += int(np.count_nonzero(rep == g.mv))
            has = rep[rep != g.mv]
            pit_outside += int(np.count_nonzero(grid.pit[has] & ~grid.selector(sel)[has]))
        total += 1
        if grid.n1 > 1:
            done += all(UC.network_valid(UC.upscale(g.idxs_ds, upa, g.shape, cellsize, m, g.mv)[0], g.mv) for m in UC.METHODS)
    assert 4 * done >= 3 * total, (done, total)
    assert ties and empty and pit_outside and nan, (ties, empty, pit_outside, nan)


def test_loop_case_upscales_to_a_loop():
    """The raster tests/test_gpu_upscale.py expects the reference's "network is invalid" refusal for."""
    from test_gpu_fuzz import random_d8

    shape, cellsize, seed, method = UC.LOOP_CASE
    d8, areas = UC.fuzz_raster(random_d8, shape, seed)
    g = UC.HostGraph(d8)
    assert g.acyclic
    ds1, _ = UC.upscale(g.idxs_ds, areas(g.upstream_area().ravel()), shape, cellsize, method, g.mv)
    assert not UC.network_valid(ds1, g.mv)
