"""FlwdirRaster.upscale (dmm, eam, eam_plus), upscale_error and ucat_outlets (reference pyflwdir/pyflwdir.py:1013-1157,
upscale.py, subgrid.py:13-48) on the device: dtype, shape and bytes against the reference's recorded outputs
(tests/golden/wide_upscale.npz, tools/gen_golden_upscale.py), random D8 rasters against the restated serial loops
(tests/upscale_cases.py, pinned to the record by tests/test_upscale_cases.py), and the refusals.

A coarse network with links outside the 8 neighbours: the reference produces one without raising for dmm at cellsize 1 on
flwdir_large (9875 such links in the record); it is part of the recorded cases and comes back through the general engine
(test_far_links_take_the_general_engine)."""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upscale_cases as UC  # noqa: E402
from golden_util import digest  # noqa: E402
from test_gpu_fuzz import random_d8  # noqa: E402  (the generator of test_gpu_fuzz_paths.py)

pytestmark = pytest.mark.gpu

_flws, _areas = {}, {}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fine(raster):
    """The device raster of a case (made once per raster)."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    if raster not in _flws:
        tr, latlon = UC.transform_of(raster)
        _flws[raster] = pyflwdir.from_array(UC.d8_of(raster), ftype="d8", check_ftype=False, cache=False,
                                            transform=Affine(*tr), latlon=latlon)
    return _flws[raster]


def area(raster, kind):
    return UC.uparea_of(fine(raster), kind, _areas.setdefault(raster, {}))


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(UC.GOLD, "wide_upscale.npz"))


def recorded(G, raster, name, got):
    got = np.asarray(got)
    return _same(got, G[f"out_{name}"]) if raster in UC.FULL else digest(got) == str(G[f"digest_{name}"])


def check_raster(flw, flw1, cellsize, shape1):
    """The upscaled raster's public face: shape, transform, latlon, ftype, index dtype, validity, and that it computes."""
    assert flw1.shape == shape1 and flw1.idxs_ds.dtype == flw.idxs_ds.dtype
    t, t1 = flw.transform, flw1.transform
    assert tuple(t1)[:6] == (t[0] * cellsize, t[1], t[2], t[3], t[4] * cellsize, t[5])
    assert flw1.latlon == flw.latlon and flw1.ftype == flw.ftype and flw1.isvalid
    upa1 = flw1.upstream_area()
    assert upa1.shape == shape1 and upa1.dtype == np.int32
    return upa1


@pytest.mark.parametrize("key,raster,kind,cellsize", UC.keys())
def test_upscale_golden(gpu_lib, G, key, raster, kind, cellsize):
    flw, upa = fine(raster), area(raster, kind)
    assert digest(upa) == str(G[f"upa_{raster}_{kind}"])
    shape1 = UC.coarse_shape(flw.shape, cellsize)
    for m in UC.METHODS:
        if f"raises_{key}_{m}" in G.files:
            with pytest.raises(ValueError):
                flw.upscale(cellsize, method=m, uparea=upa)
            continue
        flw1, idxs_out = flw.upscale(cellsize, method=m, uparea=upa)
        err = flw.upscale_error(flw1, idxs_out)
        assert idxs_out.shape == shape1 and idxs_out.dtype == flw.idxs_ds.dtype
        assert err.shape == shape1 and err.dtype == np.uint8
        assert recorded(G, raster, f"{key}_{m}_ds", flw1.idxs_ds), (key, m, "idxs_ds")
        assert recorded(G, raster, f"{key}_{m}_idxs", idxs_out), (key, m, "idxs_out")
        assert recorded(G, raster, f"{key}_{m}_err", err), (key, m, "upscale_error")
        assert np.count_nonzero(err == 0) == int(G[f"nerr_{key}_{m}"])
        upa1 = check_raster(flw, flw1, cellsize, shape1)
        assert upa1[idxs_out != flw._mv].min() >= 1 and np.all(upa1[idxs_out == flw._mv] == -9999)
    for m in ("eam_plus", "dmm"):
        got = flw.ucat_outlets(cellsize, uparea=upa, method=m)
        assert recorded(G, raster, f"{key}_{m}_ucat", got), (key, m, "ucat_outlets")


def test_flow_errors_and_pits_of_the_reference_test(gpu_lib):
    """The reference's own test (tests/test_upscale.py:20-24, :48-52) on flwdir_large at cellsize 20: 33 / 4 / 2 erroneous
    cells, and the pits of the coarse network map one-to-one to distinct fine outlet cells in distinct fine basins."""
    flw = fine("flwdir_large")
    bas = flw.basins().ravel()
    for m, n in (("dmm", 33), ("eam", 4), ("eam_plus", 2)):
        flw1, idxs_out = flw.upscale(20, method=m)
        assert (flw.upscale_error(flw1, idxs_out) == 0).sum() == n
        pits = idxs_out.ravel()[flw1.idxs_pit]
        assert np.unique(pits).size == flw1.idxs_pit.size
        assert np.unique(bas[pits]).size == pits.size
    assert _same(flw.ucat_outlets(20), flw.upscale(20, method="eam_plus")[1])


def test_uparea_none_is_upstream_area(gpu_lib):
    flw = fine("flwdir_large")
    upa = flw.upstream_area()
    for m in UC.METHODS:
        a, b = flw.upscale(7, method=m), flw.upscale(7, method=m, uparea=upa)
        assert _same(a[0].idxs_ds, b[0].idxs_ds) and _same(a[1], b[1])
    for m in ("eam_plus", "dmm"):
        assert _same(flw.ucat_outlets(7, method=m), flw.ucat_outlets(7, uparea=upa, method=m))


def test_far_links_take_the_general_engine(gpu_lib, G):
    """dmm at cellsize 1 links cells two apart: the reference accepts the network, and here it is a general graph."""
    assert int(G["far_flwdir_large_cell_1_dmm"]) > 0
    flw = fine("flwdir_large")
    flw1, idxs_out = flw.upscale(1, method="dmm")
    assert flw1._d8 is None and flw1.ftype == "d8"
    assert UC.far_links(flw1.idxs_ds, flw1.shape, flw._mv) == int(G["far_flwdir_large_cell_1_dmm"])
    assert _same(flw1.idxs_ds, G["out_flwdir_large_cell_1_dmm_ds"])
    # the D8 engine for a network inside the 8 neighbours
    assert flw.upscale(20, method="dmm")[0]._d8 is not None


_fuzz_done = {}


def run_fuzz_case(shape, cellsize, seed):
    """One random raster against the restated loops, once per session: True if every method ran through, False if the
    coarse network is refused (expected from both sides, and asserted)."""
    import pyflwdir_amd as pyflwdir

    if (shape, cellsize) in _fuzz_done:
        return _fuzz_done[shape, cellsize]
    d8, areas = UC.fuzz_raster(random_d8, shape, seed, cellsize)
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    upa = areas(flw.upstream_area().ravel()).reshape(shape)
    ds, mv = flw.idxs_ds, flw._mv
    shape1 = UC.coarse_shape(shape, cellsize)
    for m in ("eam_plus", "dmm"):
        assert _same(flw.ucat_outlets(cellsize, uparea=upa, method=m),
                     UC.ucat_outlets(ds, upa, shape, cellsize, m, mv).reshape(shape1)), m
    done = True
    for m in UC.METHODS:
        ok = shape1 != (1, 1)  # (a single coarse cell is no raster: ValueError from either constructor)
        if ok:
            ds1, out = UC.upscale(ds, upa, shape, cellsize, m, mv)
            ok = UC.network_valid(ds1, mv)  # (a loop in the coarse network)
        if not ok:
            with pytest.raises(ValueError):
                flw.upscale(cellsize, method=m, uparea=upa)
            done = False
            continue
        flw1, idxs_out = flw.upscale(cellsize, method=m, uparea=upa)
        assert _same(flw1.idxs_ds, ds1) and _same(idxs_out, out.reshape(shape1)), m
        assert _same(flw.upscale_error(flw1, idxs_out), UC.upscale_error(ds, out, ds1, mv).reshape(shape1)), m
        check_raster(flw, flw1, cellsize, shape1)
    _fuzz_done[shape, cellsize] = done
    return done


@pytest.mark.parametrize("shape,cellsize,seed", UC.fuzz_cases())
def test_random_rasters(gpu_lib, shape, cellsize, seed):
    """Random acyclic rasters (20-30 % nodata, areas with equal values and NaN) against the restated loops: every method,
    the error map and both ucat_outlets methods, bit for bit; a refused coarse network is refused on both sides."""
    run_fuzz_case(shape, cellsize, seed)


def test_random_rasters_mostly_complete(gpu_lib):
    """At least three quarters of the random cases run through every method (the others are refusals, asserted as such)."""
    cases = UC.fuzz_cases()
    assert 4 * sum(run_fuzz_case(*c) for c in cases) >= 3 * len(cases)


def test_invalid_coarse_network_is_refused(gpu_lib):
    """A coarse network with a loop (tests/test_upscale_cases.py::test_loop_case_upscales_to_a_loop): the reference's text."""
    import pyflwdir_amd as pyflwdir

    shape, cellsize, seed, method = UC.LOOP_CASE
    d8, areas = UC.fuzz_raster(random_d8, shape, seed)
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    with pytest.raises(ValueError, match="The upscaled flow direction network is invalid. Please provide a minimal"):
        flw.upscale(cellsize, method=method, uparea=areas(flw.upstream_area().ravel()))


def test_refusals(gpu_lib):
    import pyflwdir_amd as pyflwdir

    flw = fine("flwdir_large")
    with pytest.raises(NotImplementedError, match="eam_plus"):
        flw.upscale(20)  # (the reference's default method, ihu)
    with pytest.raises(NotImplementedError, match="eam_plus"), pytest.warns(DeprecationWarning):
        flw.upscale(20, method="com2")
    with pytest.warns(DeprecationWarning, match="com renamed to eam_plus"):
        a = flw.upscale(20, method="com")
    assert _same(a[1], flw.upscale(20, method="eam_plus")[1])
    with pytest.raises(ValueError, match="Unknown method: nearest, select from: 'ihu', 'eam_plus', 'com2', 'com', 'eam', 'dmm'"):
        flw.upscale(20, method="nearest")
    with pytest.raises(ValueError, match="Unknown method: eam, select from: 'eam_plus', 'dmm'"):
        flw.ucat_outlets(20, method="eam")
    with pytest.raises(ValueError, match="size does not match"):
        flw.upscale(20, method="eam", uparea=np.ones((3, 3)))
    # a fine raster of the general engine: NEXTXY, and a D8-typed raster whose links leave the 8 neighbours
    far = flw.upscale(1, method="dmm")[0]
    assert far._d8 is None
    nextxy = pyflwdir.FlwdirRaster(idxs_ds=flw.idxs_ds, shape=flw.shape, ftype="nextxy")
    for g in (far, nextxy):
        with pytest.raises(ValueError, match="only works for D8 or LDD"):
            g.upscale(2, method="eam")
        with pytest.raises(ValueError, match="only works for D8 or LDD"):
            g.ucat_outlets(2)


def test_cyclic_raster_is_refused_before_any_walk(gpu_lib, monkeypatch):
    """A fine raster with a loop raises ValueError from the front end; the library is not asked to walk."""
    from pyflwdir_amd import _hip

    import pyflwdir_amd as pyflwdir

    flw = pyflwdir.from_array(UC.d8_of(UC.CYCLIC), ftype="d8", check_ftype=False, cache=False)
    assert not flw.isvalid
    upa = flw.upstream_area()
    good = fine("flwdir_large")
    flw1, idxs_out = good.upscale(16, method="eam_plus")  # 10 x 13 coarse cells; the cyclic raster has 6 x 5 at 16

    def never(*a, **k):
        raise AssertionError("a walk kernel was started on a cyclic raster")

    monkeypatch.setattr(_hip.RasterHandle, "upscale", never)
    monkeypatch.setattr(_hip.RasterHandle, "upscale_error", never)
    for m in UC.METHODS:
        with pytest.raises(ValueError, match="loop"):
            flw.upscale(16, method=m, uparea=upa)
    with pytest.raises(ValueError, match="loop"):
        flw.ucat_outlets(16, uparea=upa)
    with pytest.raises(ValueError, match="loop"):
        flw.upscale_error(flw1, idxs_out)


def test_ldd_raster_keeps_its_type(gpu_lib):
    import pyflwdir_amd as pyflwdir

    flw = fine("flwdir_large")
    ldd = pyflwdir.from_array(flw.to_array("ldd"), ftype="ldd", cache=False)
    a, b = ldd.upscale(20, method="eam_plus"), flw.upscale(20, method="eam_plus")
    assert a[0].ftype == "ldd" and _same(a[0].idxs_ds, b[0].idxs_ds) and _same(a[1], b[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _same(ldd.upscale_error(*a), flw.upscale_error(*b))
