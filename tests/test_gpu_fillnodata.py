"""FlwdirRaster.fillnodata (reference pyflwdir/flwdir.py:360-392; core.fillnodata_upstream / _downstream,
core.py:120-188) on the device: bit for bit against the reference's recorded outputs (tests/golden/wide_fillnodata.npz,
tools/gen_golden_fillnodata.py) through every engine, against a restatement of the two serial loops on larger rasters,
in row blocks, and through the C-ABI with device memory."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as FC  # noqa: E402
from golden_util import GOLD, digest  # noqa: E402
from serial_refs import _ref_down, _ref_up  # noqa: E402  (the reference's two serial loops, core.py:120-188)

pytestmark = pytest.mark.gpu

ENGINES = ["exact", "levels", "exact:PFD_TEST_FUSE_MIN=1048576"]


def _engine(monkeypatch, engine):
    if engine == "levels":
        monkeypatch.setenv("PFD_EXACT_LEVELS", "1")
    if ":" in engine:
        knob, _, val = engine.split(":")[1].partition("=")
        monkeypatch.setenv(knob, val or "1")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _rasters():
    import pyflwdir_amd as pyflwdir

    for name in FC.RASTERS:
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        yield name, pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
    W = np.load(os.path.join(GOLD, "wide_general.npz"))
    nxy = W["in_flwdir0_nextxy"]
    yield "flwdir0_nextxy", pyflwdir.from_array(nxy, ftype="nextxy", cache=False)
    yield "flwdir0_ds2", pyflwdir.FlwdirRaster(idxs_ds=W["in_flwdir0_ds2"], shape=nxy.shape[1:], ftype="d8", cache=False)


@pytest.mark.parametrize("engine", ENGINES)
def test_fillnodata_golden(gpu_lib, monkeypatch, engine):
    """Every recorded case (7 rasters incl. cycles and two general graphs; int8 ... float64; nodata -9999 / 0 / NaN;
    both directions, all three merge rules), dtype, shape and bytes."""
    _engine(monkeypatch, engine)
    G = np.load(os.path.join(GOLD, "wide_fillnodata.npz"))
    bad = []
    n = 0
    for name, flw in _rasters():
        for dt in FC.DTYPES:
            for ndname, nd in FC.NODATAS:
                data = FC.payload(flw.size, dt, nd).reshape(flw.shape)
                for direction, how in FC.CALLS:
                    k = FC.key(name, dt, ndname, direction, how)
                    got = flw.fillnodata(data, nd, direction=direction, how=how)
                    ok = _same(got, G["out_" + k]) if name in FC.FULL else digest(got) == str(G["digest_" + k])
                    n += 1
                    if not ok:
                        bad.append(k)
    assert n == 504 and not bad, bad[:20]


_EXPECTED = {}  # (raster, case) -> the serial loops' result, shared by the engines


@pytest.mark.parametrize("engine", ENGINES)
def test_fillnodata_large_rasters(gpu_lib, oracle, monkeypatch, engine):
    """1-1.5 Mcell rasters spanning hundreds of 64 x 64 tiles (a river raster and a rough one, nodata in the flow
    directions): float32 sum / max, int32 sum with nodata 0 and float64 up against the serial loops."""
    import warnings

    import pyflwdir_amd as pyflwdir

    O = oracle
    _engine(monkeypatch, engine)
    for shape, seed, kw in [((1200, 1000), 3, dict(tilt=1 << 26, white=2, nodata_pct=10)),
                            ((1024, 1024), 4, dict(tilt=3000, white=2, nodata_pct=25))]:
        d8 = O.synth_d8(shape[0], shape[1], seed=seed, **kw)
        idxs_ds, idxs_pit, _ = O.from_array(d8)
        seq = O.idxs_seq(idxs_ds, idxs_pit)
        flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
        n = d8.size
        f32 = FC.payload(n, "float32", -9999.0, salt=seed)
        i32 = FC.payload(n, "int32", 0, salt=seed)
        f64 = FC.payload(n, "float64", -9999.0, salt=seed + 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cases = [(f32, -9999.0, "down", "sum"), (f32, -9999.0, "down", "max"), (i32, 0, "down", "sum"),
                     (f64, -9999.0, "up", "max")]
            for c, (data, nd, direction, how) in enumerate(cases):
                if (seed, c) not in _EXPECTED:
                    _EXPECTED[seed, c] = (_ref_up(idxs_ds, seq, data, nd) if direction == "up"
                                          else _ref_down(idxs_ds, seq, data, nd, how))
                exp = _EXPECTED[seed, c]
                flw._h.set_profiling(True)
                got = flw.fillnodata(data.reshape(shape), nd, direction=direction, how=how).ravel()
                ran = [s["name"] for s in flw._h.last_timing()]
                flw._h.set_profiling(False)
                assert ("exact_fillnodata_" + direction in ran) == (engine != "levels"), ran
                assert _same(got, exp), (shape, data.dtype, direction, how)


def test_fillnodata_row_blocks(gpu_lib, oracle, monkeypatch):
    """A 1.65 Mcell raster cut into 5 row blocks (the path beyond 2**32 - 2 cells, threshold lowered): float32 sum and
    the up-fill equal the single-handle results bit for bit."""
    import pyflwdir_amd as pyflwdir

    O = oracle
    shape = (1500, 1100)
    d8 = O.synth_d8(shape[0], shape[1], seed=61, tilt=100000, white=2, nodata_pct=15)
    data = FC.payload(d8.size, "float32", -9999.0, salt=5).reshape(shape)
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    data8 = FC.payload(d8.size, "int8", 0, salt=5).reshape(shape)  # (int8 sums that wrap and meet 0)
    whole = [flw.fillnodata(data, -9999.0, direction="down", how="sum"), flw.fillnodata(data, -9999.0, direction="up"),
             flw.fillnodata(data8, 0, direction="down", how="sum")]
    monkeypatch.setenv("PFD_TEST_BIG_CELLS", "400000")
    blocked = pyflwdir.from_array(d8, ftype="d8", cache=False)
    assert blocked._row_blocks_needed() == 5
    got = [blocked.fillnodata(data, -9999.0, direction="down", how="sum"),
           blocked.fillnodata(data, -9999.0, direction="up"),
           blocked.fillnodata(data8, 0, direction="down", how="sum")]
    for g, w in zip(got, whole):
        assert _same(g, w)


def test_fillnodata_errors(gpu_lib):
    import pyflwdir_amd as pyflwdir

    d8 = np.load(os.path.join(GOLD, "flwdir0.npz"))["d8"]
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    data = np.ones(d8.shape, np.float32)
    with pytest.raises(ValueError, match="Unknown flow direction"):
        flw.fillnodata(data, -9999, direction="sideways")
    with pytest.raises(AssertionError):
        flw.fillnodata(data, -9999, direction="down", how="mean")
    flw.fillnodata(data, -9999, direction="up", how="mean")  # (how is not looked at upstream)
    with pytest.raises(ValueError, match="size does not match"):
        flw.fillnodata(np.ones(7, np.float32), -9999)
    with pytest.raises(NotImplementedError):
        flw.fillnodata(data.astype(np.complex64), -9999)
    assert _same(flw.fillnodata(data.astype(bool).astype(np.uint8), 0, direction="UP"),
                 data.astype(np.uint8))  # (case-insensitive like the reference; nothing to fill)


def test_fillnodata_device_memory(gpu_lib):
    """pfd_fillnodata with payload and result in device memory (PFD_DEVICE) gives the host call's bytes."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    d8 = np.load(os.path.join(GOLD, "synth_river_nodata_768x1024.npz"))["d8"]
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    data = FC.payload(d8.size, "float64", -9999.0, salt=9)
    for direction, how in ((_hip.PFD_DOWN, _hip.PFD_FILL_SUM), (_hip.PFD_UP, _hip.PFD_FILL_MAX)):
        host = flw._h.fillnodata(data, _hip.PFD_F64, nodata_f=-9999.0, direction=direction, how=how)
        din = _hip.DeviceBuffer(data.nbytes).upload(data)
        dout = _hip.DeviceBuffer(data.nbytes)
        try:
            flw._h.fillnodata(din, _hip.PFD_F64, nodata_f=-9999.0, direction=direction, how=how, out=dout,
                              memspace=_hip.PFD_DEVICE)
            dev = dout.download(np.float64, data.shape)
        finally:
            din.free()
            dout.free()
        assert _same(dev, host)
    # bad arguments through the C-ABI: direction, how, dtype code
    with pytest.raises(ValueError):
        flw._h.fillnodata(data, _hip.PFD_F64, direction=7)
    with pytest.raises(ValueError):
        flw._h.fillnodata(data, _hip.PFD_F64, direction=_hip.PFD_DOWN, how=9)
    with pytest.raises(NotImplementedError):
        flw._h.fillnodata(data, 42, direction=_hip.PFD_DOWN)
