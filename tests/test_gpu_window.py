"""FlwdirRaster.downstream, moving_average, moving_median and path (reference pyflwdir/flwdir.py:394-410, :435-504;
pyflwdir/pyflwdir.py:443-500) on the device: dtype, shape and bytes against the reference's recorded outputs
(tests/golden/wide_window.npz, tools/gen_golden_window.py), one case per entry point through the C-ABI with its inputs and
outputs in device memory, random D8 rasters — with and without cycles — against the restated serial loops
(tests/window_cases.py, pinned to the record by tests/test_window_cases.py), and the refusals.  Every comparison is exact;
NaNs count as equal when they sit in the same positions."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_cases as WC  # noqa: E402
from golden_util import digest  # noqa: E402
from test_gpu_fuzz import random_d8  # noqa: E402

pytestmark = pytest.mark.gpu

_flws = {}


def _same(a, b):
    a, b = WC.canon(a), WC.canon(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fine(raster, grid):
    """The device raster of a case (made once per raster and grid; cache=True: idxs_us_main and the order are derived once)."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    if (raster, grid) not in _flws:
        tr, latlon = WC.transform_of(raster, grid)
        _flws[raster, grid] = pyflwdir.from_array(WC.d8_of(raster), ftype="d8", check_ftype=False, cache=True,
                                                  transform=Affine(*tr), latlon=latlon)
    return _flws[raster, grid]


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(WC.GOLD, WC.RECORD))


def recorded(G, raster, name, got):
    got = WC.canon(got)
    if raster in WC.FULL:
        return _same(got, G[f"out_{name}"])
    return digest(got) == str(G[f"digest_{name}"])


def window_call(flw, method, inp, kw, strord):
    """One call of tests/window_cases.window_calls through the front end."""
    kw = dict(kw)
    data = inp[kw.pop("data")].reshape(flw.shape)
    if method == "downstream":
        return flw.downstream(data)
    if "weights" in kw:
        kw["weights"] = inp[kw["weights"]].reshape(flw.shape)
    if kw.get("strord") == "given":
        kw["strord"] = strord
    return flw.moving_average(data, **kw) if method == "average" else flw.moving_median(data, **kw)


@pytest.mark.parametrize("raster", WC.RASTERS)
def test_window_golden(gpu_lib, G, raster):
    flw = fine(raster, "ll")
    assert digest(flw.idxs_us_main) == str(G[f"usmain_{raster}"])
    strord = flw.stream_order()
    assert digest(strord) == str(G[f"strord_{raster}"])
    inp = WC.inputs(flw.size)
    for name, method, kw in WC.window_calls(raster):
        res = window_call(flw, method, inp, kw, strord)
        assert res.shape == flw.shape and res.dtype == inp[kw["data"]].dtype
        assert recorded(G, raster, f"{raster}_{name}", res), (raster, name)
        if res.dtype.kind == "f":
            assert int(np.count_nonzero(np.isnan(res))) == int(G[f"nan_{raster}_{name}"])


@pytest.mark.parametrize("raster", WC.RASTERS)
@pytest.mark.parametrize("grid", WC.GRIDS)
def test_path_golden(gpu_lib, G, raster, grid):
    flw = fine(raster, grid)
    inp = WC.inputs(flw.size)
    starts = G[f"starts_{raster}"]
    for name, kw in WC.path_calls(raster, grid):
        kw = dict(kw)
        if "mask" in kw:
            kw["mask"] = inp[kw["mask"]].reshape(flw.shape)
        paths, dists = flw.path(idxs=starts, **kw)
        assert isinstance(paths, list) and len(paths) == starts.size and dists.dtype == np.float64
        assert all(p.dtype == flw.idxs_ds.dtype and p.ndim == 1 for p in paths)
        cells, lens = WC.flat_paths(paths, flw.idxs_ds.dtype)
        pre = f"{raster}_{grid}_path_{name}"
        assert recorded(G, raster, pre + "_cells", cells), pre
        assert recorded(G, raster, pre + "_lens", lens), pre
        assert recorded(G, raster, pre + "_dists", dists), pre


def test_path_from_xy_and_single_start(gpu_lib, G):
    flw = fine("flwdir0", "ll")
    starts = G["starts_flwdir0"][:5]
    a, da = flw.path(idxs=starts)
    b, db = flw.path(xy=flw.xy(starts))
    assert all(_same(p, q) for p, q in zip(a, b)) and _same(da, db)
    one, d1 = flw.path(idxs=int(starts[0]))
    assert len(one) == 1 and _same(one[0], a[0]) and d1.shape == (1,)
    nodata = int(np.flatnonzero(flw.idxs_ds == flw._mv)[0])
    p, d = flw.path(idxs=[nodata], direction="up")
    assert p[0].tolist() == [nodata] and d[0] == 0.0
    masked = np.ones(flw.shape, bool)
    p, d = flw.path(idxs=starts, mask=masked)
    assert [q.tolist() for q in p] == [[int(s)] for s in starts] and np.all(d == 0.0)


def test_path_longer_than_the_first_capacity(gpu_lib):
    """One path of 5000 cells (a row draining east into a pit in its last column) against the 4096 cells a first call
    with one start cell has room for: the binding repeats the call with room for all."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    res = {}
    for n in (100, 5000):
        d8 = np.full((1, n), 1, np.uint8)  # (1: east)
        d8[0, -1] = 0
        flw = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
        res[n] = flw._h.path(np.array([0]), _hip.PFD_DOWN, np.int32)
        cells, offsets, dists = res[n]
        assert cells.dtype == np.int32 and np.array_equal(cells, np.arange(n)) and offsets.tolist() == [0, n]
        assert dists.dtype == np.float64 and dists.shape == (1,)
    assert res[100][2][0] == 99.0 and res[5000][2][0] == res[100][2][0] / 99 * 4999  # (cells: one per step)


def test_cabi_with_device_inputs_and_outputs(gpu_lib, G):
    """One case per entry point with the per-cell inputs and the results in device memory."""
    from pyflwdir_amd import _hip
    from pyflwdir_amd import gis

    raster = "flwdir_large"
    flw = fine(raster, "ll")
    h, n = flw._h, flw.size
    inp = WC.inputs(n)

    def dev(a):
        a = np.ascontiguousarray(a)
        return _hip.DeviceBuffer(a.nbytes).upload(a)

    us = flw.idxs_us_main
    d_us = (dev(us), us.dtype)
    strord = np.ascontiguousarray(flw.stream_order().ravel())
    d_so = (dev(strord), _hip.STRORD_CODE[strord.dtype])
    res = _hip.DeviceBuffer(8 * n)
    h.downstream(dev(inp["i16"]), elem_bytes=2, out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, f"{raster}_ds_i16", res.download(np.int16, flw.shape))
    h.moving_average(3, d_us, (dev(inp["data64"]), _hip.PFD_F64), (dev(inp["w64"]), _hip.PFD_F64), d_so, out=res,
                     memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, f"{raster}_avg_f64_w64_given_n3", res.download(np.float64, flw.shape))
    h.moving_average(3, d_us, (dev(inp["data32"]), _hip.PFD_F32), out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, f"{raster}_avg_f32_n3", res.download(np.float32, flw.shape))
    h.moving_median(10, d_us, (dev(inp["data32"]), _hip.PFD_F32), d_so, out=res, memspace=_hip.PFD_DEVICE)
    assert recorded(G, raster, f"{raster}_med_f32_so_n10", res.download(np.float32, flw.shape))
    # path: a sizing call (cap 0, no lists), then the fetch into buffers of exactly that size
    starts = G[f"starts_{raster}"]
    d_mask = dev(inp["mask"].view(np.uint8))
    tab = gis.step_length_table(flw.shape[0], flw.latlon, flw.transform, dtype=np.float64)
    kw = dict(idxs_us_main=d_us, mask=d_mask, step_lengths=tab, max_length=2 * WC.max_length_m(raster, "ll"))
    m = h.path(starts, _hip.PFD_UP, us.dtype, memspace=_hip.PFD_DEVICE, **kw)
    assert m >= starts.size
    cells, offs, dists = _hip.DeviceBuffer(us.dtype.itemsize * m), _hip.DeviceBuffer(8 * (starts.size + 1)), _hip.DeviceBuffer(8 * starts.size)
    assert h.path(starts, _hip.PFD_UP, us.dtype, idxs_out=cells, offsets_out=offs, dist_out=dists, cap_idxs=m,
                  memspace=_hip.PFD_DEVICE, **kw) == m
    pre = f"{raster}_ll_path_up_m_max_mask"
    offsets = offs.download(np.int64, (starts.size + 1,))
    assert offsets[0] == 0 and offsets[-1] == m
    assert recorded(G, raster, pre + "_cells", cells.download(us.dtype, (m,)))
    assert recorded(G, raster, pre + "_lens", np.diff(offsets))
    assert recorded(G, raster, pre + "_dists", dists.download(np.float64, (starts.size,)))


def _random_raster(shape, seed, cyclic):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import gis
    from pyflwdir_amd._affine import Affine

    rng = np.random.default_rng([WC.FUZZ_SEED_BASE, shape[0], shape[1], seed, int(cyclic)])
    d8 = random_d8(rng, shape, p_nodata=rng.choice([0.0, 0.1, 0.3]), p_pit=rng.choice([0.002, 0.02]),
                   coherent=rng.choice([0, 1, 2, 4]) if cyclic else -1)
    tr, latlon = ((0.01, 0.0, 5.0, 0.0, -0.01, 50.0), True) if seed % 2 else (WC.PROJECTED, False)
    flw = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=True, transform=Affine(*tr), latlon=latlon)
    steps = gis.step_length_table(shape[0], latlon, flw.transform, dtype=np.float64)
    return rng, flw, WC.Graph(flw.idxs_ds, flw.idxs_us_main, flw._mv, shape, steps)


def _straddle(dtype):
    """n just below, at and just beyond the bound between the two median forms"""
    from pyflwdir_amd import _hip

    half = _hip.window_wmax(dtype) // 2
    return [half - 1, half, half + 1]


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("shape", WC.FUZZ_SHAPES)
def test_random_rasters_windows(gpu_lib, shape, cyclic):
    """downstream and the two window calls, on rasters with cycles as well: both median forms and the bound between them."""
    seed = WC.FUZZ_SHAPES.index(shape)
    rng, flw, g = _random_raster(shape, seed, cyclic)
    if cyclic and shape[0] > 1 and shape[1] > 1:
        assert flw._has_loop()
    inp = WC.inputs(flw.size, seed)
    for name in ("data32", "flag", "i64"):
        assert _same(flw.downstream(inp[name].reshape(shape)), WC.downstream(g, inp[name]).reshape(shape)), name
    strord = flw.stream_order()
    for dname, wnames in (("data32", [None, "w32", "w64"]), ("data64", ["w64", None, "w32"])):
        data = inp[dname].reshape(shape)
        for i, n in enumerate(_straddle(data.dtype)):
            so = strord if i == 1 else None
            nodata = float("nan") if i == 2 else WC.NODATA
            w = None if wnames[i] is None else inp[wnames[i]]
            got = flw.moving_average(data, n, weights=w, strord=so, nodata=nodata)
            assert _same(got, WC.moving_average(g, data, n, w, so, nodata).reshape(shape)), (shape, cyclic, dname, n, "average")
            got = flw.moving_median(data, n, strord=so, nodata=nodata)
            assert _same(got, WC.moving_median(g, data, n, so, nodata).reshape(shape)), (shape, cyclic, dname, n, "median")


def test_median_workspace_in_chunks(gpu_lib, monkeypatch):
    """A workspace smaller than the raster: the large-window median serves the cells in chunks."""
    shape = (257, 255)
    rng, flw, g = _random_raster(shape, 7, False)
    inp = WC.inputs(flw.size, 7)
    monkeypatch.setenv("PFD_WINDOW_WS_BYTES", str(1 << 20))
    for dname in ("data32", "data64"):
        data = inp[dname].reshape(shape)
        n = _straddle(data.dtype)[2] + 2
        lanes = (1 << 20) // ((2 * n + 1) * data.dtype.itemsize)
        assert 256 <= lanes < flw.size // 4
        assert _same(flw.moving_median(data, n), WC.moving_median(g, data, n).reshape(shape)), dname


@pytest.mark.parametrize("shape,count,seed", WC.fuzz_cases())
def test_random_rasters_paths(gpu_lib, shape, count, seed):
    rng, flw, g = _random_raster(shape, seed, False)
    inp = WC.inputs(flw.size, seed)
    starts = rng.integers(0, flw.size, count).astype(np.int64)
    mx = 3.5 * float(g.steps[0, 0])
    for kw in (dict(direction="down"), dict(direction="up", mask=inp["mask"]), dict(direction="down", max_length=4),
               dict(direction="up", unit="m"), dict(direction="down", unit="m", max_length=mx, mask=inp["mask"])):
        got, dgot = flw.path(idxs=starts, **{k: (v.reshape(shape) if k == "mask" else v) for k, v in kw.items()})
        exp, dexp = WC.path(g, starts, **kw)
        assert len(got) == count and _same(dgot, dexp), (shape, count, kw.get("direction"))
        assert _same(WC.flat_paths(got, flw.idxs_ds.dtype)[0], WC.flat_paths(exp, flw.idxs_ds.dtype)[0])
        assert [len(p) for p in got] == [len(p) for p in exp]


def test_refusals(gpu_lib, G):
    import pyflwdir_amd as pyflwdir

    flw = fine("flwdir0", "ll")
    inp = WC.inputs(flw.size)
    data = inp["data32"].reshape(flw.shape)
    for n in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="non-negative integer"):
            flw.moving_average(data, n)
        with pytest.raises(ValueError, match="non-negative integer"):
            flw.moving_median(data, n)
    assert _same(flw.moving_average(data, np.int64(3)), flw.moving_average(data, 3))
    ints = np.ones(flw.shape, np.int32)
    for f in (lambda: flw.moving_average(ints, 1), lambda: flw.moving_median(ints, 1),
              lambda: flw.moving_average(data, 1, weights=ints), lambda: flw.moving_average(data.astype(np.float16), 1),
              lambda: flw.moving_median(data, 1, strord=data), lambda: flw.downstream(np.zeros(flw.shape, "S3"))):
        with pytest.raises(NotImplementedError, match="dtype"):
            f()
    with pytest.raises(ValueError, match="size does not match"):
        flw.downstream(np.ones((3, 3)))
    with pytest.raises(ValueError, match=r'Unknown unit: km, select from \["m", "cell"\]'):
        flw.path(idxs=[0], unit="km")
    with pytest.raises(ValueError, match="Unknown flow direction"):
        flw.path(idxs=[0], direction="both")
    with pytest.raises(ValueError, match="Either idxs or xy"):
        flw.path()
    for bad in ([flw.size], [-1], [0, flw.size + 5]):
        with pytest.raises(IndexError):
            flw.path(idxs=bad)
    # a raster with a loop: no path, but downstream and the windows (bounded by n) are served
    loops = pyflwdir.from_array(np.load(os.path.join(WC.GOLD, "synth_loops_96x80.npz"))["d8"], ftype="d8", check_ftype=False)
    with pytest.raises(ValueError, match="loop"):
        loops.path(idxs=[0])
    assert loops.moving_median(np.ones(loops.shape, np.float32), 2).shape == loops.shape
    # a general idxs_ds graph: refused before any kernel
    general = pyflwdir.FlwdirRaster(idxs_ds=flw.idxs_ds, shape=flw.shape, ftype="nextxy")
    assert general._d8 is None
    for f in (lambda: general.downstream(data), lambda: general.moving_average(data, 1), lambda: general.moving_median(data, 1),
              lambda: general.path(idxs=[0])):
        with pytest.raises(NotImplementedError, match="general idxs_ds graph"):
            f()


def test_cabi_refusals(gpu_lib):
    """What the entry points themselves refuse: an idxs_us_main that is not the inverse of the downstream links, an index
    outside the raster, elements of 3 bytes."""
    from pyflwdir_amd import _hip

    flw = fine("flwdir0", "ll")
    h = flw._h
    data = WC.inputs(flw.size)["data32"]
    us = np.ascontiguousarray(flw.idxs_us_main).copy()
    valid = np.flatnonzero(flw.idxs_ds != flw._mv)
    pit = int(flw.idxs_pit[0])
    wrong = us.copy()
    wrong[pit] = [c for c in valid if flw.idxs_ds[c] != pit][0]
    with pytest.raises(ValueError, match="does not drain"):
        h.moving_average(2, wrong, data)
    outside = us.copy()
    outside[pit] = flw.size
    with pytest.raises(ValueError, match="outside the raster"):
        h.moving_median(2, outside, data)
    with pytest.raises(ValueError, match="outside the raster"):
        h.path(np.array([flw.size]), _hip.PFD_DOWN, us.dtype)
    with pytest.raises(NotImplementedError, match="1, 2, 4 or 8"):
        h.downstream(_hip.DeviceBuffer(3 * flw.size), elem_bytes=3, out=_hip.DeviceBuffer(3 * flw.size), memspace=_hip.PFD_DEVICE)
