"""FlwdirRaster.ucat_volume, subgrid_rivlen, subgrid_rivslp, subgrid_rivavg, subgrid_rivmed and distnc (reference
pyflwdir/pyflwdir.py:1193-1454, :420-429; subgrid.py:96-559) on the device: dtype, shape and bytes against the reference's
recorded outputs (tests/golden/wide_subgrid_riv.npz, tools/gen_golden_subgrid_riv.py), one case per entry point through
the C-ABI with its inputs in device memory, random D8 rasters against the restated serial loops
(tests/subgrid_riv_cases.py, pinned to the record by tests/test_subgrid_riv_cases.py), and the refusals.  Every comparison
is exact; NaNs count as equal when they sit in the same positions."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subgrid_riv_cases as SC  # noqa: E402
from golden_util import digest  # noqa: E402
from test_gpu_fuzz import random_d8  # noqa: E402

pytestmark = pytest.mark.gpu

_flws = {}


def _same(a, b):
    a, b = SC.canon(a), SC.canon(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fine(raster, grid):
    """The device raster of a case (made once per raster and grid; cache=True: distnc and idxs_us_main are derived once)."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    if (raster, grid) not in _flws:
        tr, latlon = SC.transform_of(raster, grid)
        _flws[raster, grid] = pyflwdir.from_array(SC.d8_of(raster), ftype="d8", check_ftype=False, cache=True,
                                                  transform=Affine(*tr), latlon=latlon)
    return _flws[raster, grid]


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(SC.GOLD, SC.RECORD))


def recorded(G, raster, key, name, got):
    got = SC.canon(got)
    if raster in SC.FULL:
        return _same(got, G[f"out_{key}_{name}"])
    return digest(got) == str(G[f"digest_{key}_{name}"])


def call(flw, method, idxs_out, inp, kw):
    """One call of tests/subgrid_riv_cases.calls through the front end."""
    kw = dict(kw)
    for name in ("mask", "elevtn", "data", "weights", "hand"):
        if name in kw:
            kw[name] = inp[kw[name]].reshape(flw.shape) if name != "weights" else inp[kw[name]]
    if method == "rivlen":
        return flw.subgrid_rivlen(idxs_out, **kw)
    if method == "rivslp":
        return flw.subgrid_rivslp(idxs_out, method="mean", **kw)
    if method == "rivavg":
        return flw.subgrid_rivavg(idxs_out, **kw)
    if method == "rivmed":
        return flw.subgrid_rivmed(idxs_out, nodata=SC.NODATA, **kw)
    return flw.ucat_volume(idxs_out, kw["hand"], depths=SC.depths_of(kw["depths"]))


@pytest.mark.parametrize("key,raster,grid,cellsize,variant", SC.configs())
def test_subgrid_riv_golden(gpu_lib, G, key, raster, grid, cellsize, variant):
    flw = fine(raster, grid)
    assert digest(flw.idxs_us_main) == str(G[f"usmain_{raster}"])
    assert digest(flw.distnc) == str(G[f"distnc_{raster}_{grid}"])
    idxs_out = None if variant == "none" else G[f"outlets_{key}"]
    if variant == "":
        assert _same(flw.ucat_outlets(cellsize), idxs_out)
    shape = flw.shape if idxs_out is None else idxs_out.shape
    inp = SC.inputs(flw.size)
    for name, method, kw in SC.calls(variant):
        res = call(flw, method, idxs_out, inp, kw)
        if method == "volume":
            assert res[0].shape == flw.shape and recorded(G, raster, key, "ucatmap", res[0]), (key, name, "map")
            res = res[1]
            assert res.shape == (SC.depths_of(kw["depths"]).size, *shape) and res.dtype == SC.depths_of(kw["depths"]).dtype
        else:
            assert res.shape == shape
        assert recorded(G, raster, key, name, res), (key, name)
        assert int(np.count_nonzero(np.isnan(res))) == int(G[f"nan_{key}_{name}"])


def test_result_dtypes(gpu_lib, G):
    """int32 cells / float32 metres for the length; float32 for "both", the dtype of elevtn for "up" / "down"."""
    flw = fine("flwdir0", "ll")
    out = G["outlets_flwdir0_ll_3"]
    inp = SC.inputs(flw.size)
    assert flw.subgrid_rivlen(out).dtype == np.int32 and flw.subgrid_rivlen(out, unit="m").dtype == np.float32
    assert flw.subgrid_rivslp(out, inp["elev64"].reshape(flw.shape)).dtype == np.float32
    assert flw.subgrid_rivslp(out, inp["elev64"].reshape(flw.shape), direction="up").dtype == np.float64
    assert flw.subgrid_rivslp(out, inp["elev32"].reshape(flw.shape), direction="down").dtype == np.float32
    assert flw.subgrid_rivavg(out, inp["data64"].reshape(flw.shape)).dtype == np.float64
    # a missing outlet holds nodata in every result
    mv_out = np.array([flw._mv], flw.idxs_ds.dtype)
    assert flw.subgrid_rivlen(mv_out)[0] == -9999 and flw.subgrid_rivavg(mv_out, inp["data32"])[0] == -9999
    assert flw.subgrid_rivmed(mv_out, inp["data32"])[0] == -9999 and flw.subgrid_rivslp(mv_out, inp["elev32"])[0] == -9999
    assert np.all(flw.ucat_volume(mv_out, inp["hand32"])[1] == -9999)


def test_fixed_length_slope_from_an_outlet_on_a_nodata_cell(gpu_lib):
    """Deliberately not the reference's value: from an outlet on a nodata cell the reference steps to its missing value,
    which as an index is the raster's last cell, and walks on from there; here both walks stay on the cell and the slope
    is 0.0.  The outlets on valid cells are not affected by such an entry in the list."""
    flw = fine("flwdir0", "ll")
    inp = SC.inputs(flw.size)
    nodata = np.flatnonzero(flw.idxs_ds == flw._mv)
    valid = np.flatnonzero(flw.idxs_ds != flw._mv)[::7]
    assert nodata.size and valid.size
    elev = inp["elev32"].reshape(flw.shape)
    alone = flw.subgrid_rivslp(nodata.astype(flw.idxs_ds.dtype), elev, length=2000)
    assert alone.dtype == np.float32 and np.all(alone == 0.0)
    mixed = flw.subgrid_rivslp(np.concatenate([nodata, valid]).astype(flw.idxs_ds.dtype), elev, length=2000)
    assert np.all(mixed[:nodata.size] == 0.0)
    assert _same(mixed[nodata.size:], flw.subgrid_rivslp(valid.astype(flw.idxs_ds.dtype), elev, length=2000))
    every = flw.subgrid_rivslp(None, elev, length=2000)
    assert every.shape == flw.shape and np.all(every.ravel()[nodata] == 0.0)
    assert _same(every.ravel()[valid], mixed[nodata.size:])


def test_cabi_with_device_inputs(gpu_lib, G):
    """One case per entry point with the per-cell inputs and the result in device memory."""
    from pyflwdir_amd import _hip
    from pyflwdir_amd import gis

    key, raster, grid = "flwdir_large_ll_7", "flwdir_large", "ll"
    flw = fine(raster, grid)
    h, n = flw._h, flw.size
    inp = SC.inputs(n)
    out = G[f"outlets_{key}"]
    idx64 = np.where(out.ravel() == flw._mv, -1, out.ravel().astype(np.int64))
    k = idx64.size

    def dev(a):
        a = np.ascontiguousarray(a)
        return _hip.DeviceBuffer(a.nbytes).upload(a)

    us = flw.idxs_us_main
    d_us = (dev(us), us.dtype)
    d_mask = dev(inp["mask"].view(np.uint8))
    d_dist = dev(flw.distnc.ravel())
    res = _hip.DeviceBuffer(8 * 9 * k)
    h.segment_length(idx64, _hip.PFD_DOWN, None, d_mask, (d_dist, _hip.PFD_F32), out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, key, "rivlen_down_m_mask", res.download(np.float32, out.shape))
    h.segment_slope(idx64, _hip.PFD_BOTH, d_us, (dev(inp["elev64"]), _hip.PFD_F64), d_dist, 2000, out=res,
                    memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, key, "rivslp_both_2000", res.download(np.float32, out.shape))
    h.segment_slope(idx64, _hip.PFD_UP, d_us, (dev(inp["elev64"]), _hip.PFD_F64), d_dist, out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, key, "rivslp_up", res.download(np.float64, out.shape))
    h.segment_average(idx64, _hip.PFD_DOWN, None, None, (dev(inp["data64"]), _hip.PFD_F64), (dev(inp["w64"]), _hip.PFD_F64),
                      SC.NODATA, out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, key, "rivavg_f64_w64_down", res.download(np.float64, out.shape))
    h.segment_median(idx64, _hip.PFD_UP, d_us, None, (dev(inp["data32"]), _hip.PFD_F32), SC.NODATA, out=res,
                     memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, key, "rivmed_up", res.download(np.float32, out.shape))
    rows = np.ascontiguousarray(gis.area_rows(flw.transform, flw.shape, flw.latlon, unit="m2"))
    d_map = _hip.DeviceBuffer(4 * n)
    h.ucat_volume(idx64, flw.idxs_ds.dtype, (dev(inp["hand64"]), _hip.PFD_F64), rows, SC.DEPTHS_NINE, map_out=d_map,
                  vol_out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, key, "vol_h64_nine", res.download(np.float64, (9, *out.shape)))
    assert recorded(G, raster, key, "ucatmap", d_map.download(flw.idxs_ds.dtype, flw.shape))


@pytest.mark.parametrize("shape,count,seed", SC.fuzz_cases())
def test_random_rasters_against_the_restated_loops(gpu_lib, shape, count, seed):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import gis
    from pyflwdir_amd._affine import Affine

    rng = np.random.default_rng([SC.FUZZ_SEED_BASE, shape[0], shape[1], seed])
    d8 = random_d8(rng, shape, p_nodata=rng.choice([0.0, 0.1, 0.3]), p_pit=rng.choice([0.002, 0.02]), coherent=-1)
    tr, latlon = ((0.01, 0.0, 5.0, 0.0, -0.01, 50.0), True) if seed % 2 else (SC.PROJECTED, False)
    flw = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=True, transform=Affine(*tr), latlon=latlon)
    rows = np.ascontiguousarray(gis.area_rows(flw.transform, flw.shape, flw.latlon, unit="m2"))
    g = SC.Graph(flw.idxs_ds, flw.idxs_us_main, flw.idxs_seq, flw._mv, shape, flw.distnc.ravel(), flw.stream_distance().ravel(),
                 rows)
    valid = np.flatnonzero(flw.idxs_ds != flw._mv)
    idxs_out = SC.fuzz_outlets(rng, valid, count, flw._mv, flw.idxs_ds.dtype)
    inp = SC.inputs(flw.size, seed)
    for name, method, kw in SC.calls():
        got = call(flw, method, idxs_out, inp, kw)
        exp = SC.run(g, method, idxs_out, inp, kw)
        if method == "volume":
            assert _same(got[0].ravel(), exp[0].astype(got[0].dtype)), (name, "map")
            got, exp = got[1], exp[1]
        assert _same(got, exp), (shape, count, seed, name)


def test_refusals(gpu_lib, G):
    import pyflwdir_amd as pyflwdir

    flw = fine("flwdir0", "ll")
    out = G["outlets_flwdir0_ll_3"]
    inp = SC.inputs(flw.size)
    with pytest.raises(NotImplementedError, match="powf"):
        flw.subgrid_rivslp(out, inp["elev32"], method="lstsq")
    with pytest.raises(ValueError, match="Unknown flow direction"):
        flw.subgrid_rivlen(out, direction="both")
    with pytest.raises(ValueError, match="Unknown unit"):
        flw.subgrid_rivlen(out, unit="km")
    with pytest.raises(ValueError, match="Unknown flow direction"):
        flw.subgrid_rivslp(out, inp["elev32"], direction="sideways")
    with pytest.raises(ValueError, match="Unknown flow direction"):
        flw.subgrid_rivavg(out, inp["data32"], direction="both")
    with pytest.raises(ValueError, match="Unknown flow direction"):
        flw.subgrid_rivmed(out, inp["data32"], direction="both")
    ints = np.ones(flw.shape, np.int32)
    for f in (lambda: flw.subgrid_rivavg(out, ints), lambda: flw.subgrid_rivmed(out, ints),
              lambda: flw.subgrid_rivslp(out, ints), lambda: flw.ucat_volume(out, ints)):
        with pytest.raises(NotImplementedError, match="dtype"):
            f()
    loops = pyflwdir.from_array(np.load(os.path.join(SC.GOLD, "synth_loops_96x80.npz"))["d8"], ftype="d8", check_ftype=False)
    some = np.arange(0, loops.size, 97, dtype=loops.idxs_ds.dtype)
    one = np.ones(loops.shape, np.float32)
    for f in (lambda: loops.subgrid_rivlen(some, direction="down"), lambda: loops.subgrid_rivslp(some, one),
              lambda: loops.subgrid_rivavg(some, one), lambda: loops.subgrid_rivmed(some, one)):
        with pytest.raises(ValueError, match="loop"):
            f()


def test_rivmed_returns_where_the_reference_raises(gpu_lib, G):
    """The reference's subgrid_rivmed passes ``weights=`` to a function without that parameter (TypeError); here the call
    returns subgrid.segment_median, with and without weights."""
    flw = fine("flwdir0", "ll")
    out = G["outlets_flwdir0_ll_3"]
    inp = SC.inputs(flw.size)
    a = flw.subgrid_rivmed(out, inp["data32"])
    b = flw.subgrid_rivmed(out, inp["data32"], weights=inp["w64"])
    assert _same(a, b) and recorded(G, "flwdir0", "flwdir0_ll_3", "rivmed_up", a)


def test_distnc_is_stream_distance_and_cached_with_cache_only(gpu_lib):
    import pyflwdir_amd as pyflwdir

    d8 = SC.d8_of("flwdir0")
    for cache in (True, False):
        flw = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=cache, latlon=True)
        d = flw.distnc
        assert d.dtype == np.float32 and _same(d, flw.stream_distance(unit="m"))
        assert ("distnc" in flw._cached) == cache
        assert (flw.distnc is d) == cache
