"""FlwdirRaster.subbasins_area (reference pyflwdir/pyflwdir.py:665-692, basins.py:194-233) on the device.  Everything is
exact — dtype, shape and bytes of the uint32 map and of the outlet list: every recorded case of the reference (tests/
golden/wide_subbasins_area.npz, tools/gen_golden_subbasins_area.py) through the front end; device-resident arguments; the
sizing convention of the list; the pruned and the full mode; the bound on the rounds; random D8 rasters at the edges of the
64 x 64 tiles and the 256-lane workgroups against the restated serial loop (tests/subbasins_area_cases.py), with the device's
rounds, jobs and lane steps against the restated per-group form; and the refusals."""
from __future__ import annotations

import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basin_cases as BC  # noqa: E402
import subbasins_area_cases as SC  # noqa: E402
from golden_util import digest  # noqa: E402
from test_gpu_fuzz import random_d8  # noqa: E402  (the generator of the fuzz tests)

pytestmark = pytest.mark.gpu

# 1 x 1; the smallest shapes at which a neighbour gather crosses a tile edge; more than one workgroup of jobs in a round
FUZZ_SHAPES = [(1, 1), (63, 65), (64, 64), (130, 257)]
SEED_BASE = 9300


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _maker(d8, name=""):
    """make_flw(transform kind, cache) of SC.run, one FlwdirRaster per pair."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    made = {}

    def make_flw(kind, cache):
        if (kind, cache) not in made:
            kw = {}
            if name:
                tr, latlon = BC.transform_of(name, kind)
                kw.update(transform=Affine(*tr), latlon=latlon)
            made[kind, cache] = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=cache, **kw)
        return made[kind, cache]
    return make_flw


def _call(flw, A, area_min, usm=None, flags=0, cap=None, idx_dtype=None):
    """(map[n], outlets, stats) of the binding, the comparison form resolved as the front end resolves it; ``flw``: a
    FlwdirRaster, or a RasterHandle with ``idx_dtype``."""
    from pyflwdir_amd.raster import _PAYLOAD, _area_min_compare

    A = np.ascontiguousarray(np.asarray(A).ravel())
    am, form = _area_min_compare(A.dtype, area_min)
    us = None if usm is None else np.ascontiguousarray(usm, dtype=np.int64)
    h, idx_dtype = (flw, idx_dtype) if idx_dtype is not None else (flw._h, flw._idx_dtype)
    return h.subbasins_area(A, _PAYLOAD[A.dtype], am, form, us, idx_dtype, cap=cap, flags=flags)


@pytest.mark.parametrize("name", SC.RASTERS)
def test_subbasins_area_record(gpu_lib, name):
    """Every recorded case of one raster through the front end: lat/lon and projected transforms, int32 / float64 / float32
    areas (float64 km2 as the default of ``uparea``), 5-6 thresholds, and on three rasters equal areas, NaN areas, the
    Python-float / np.float64 pair that numpy's promotion decides, strong numpy thresholds and a cached idxs_us_main that
    another area chose."""
    G = np.load(os.path.join(BC.GOLD, "wide_subbasins_area.npz"))
    make_flw = _maker(BC.d8_of(name), name)
    src = SC.FromFlw({kind: make_flw(kind, False) for kind in ("own", "south")})
    bad, n = [], 0
    for key, spec in SC.keys(name):
        for i, got in enumerate(SC.run(make_flw, spec, src)):
            got = np.asarray(got)
            ok = _same(got, G[f"out_{key}_{i}"]) if name in SC.FULL else digest(got) == str(G[f"digest_{key}_{i}"])
            n += 1
            if not ok:
                bad.append(f"{key}_{i}")
    assert n >= 2 * 12 and not bad, bad[:20]


def test_subbasins_area_device_resident_and_sizing(gpu_lib):
    """Areas, main upstream cells, map and list in device memory give the host call's bytes; a ``cap`` too small reports
    k and leaves the list unwritten (the map is complete), and the binding then repeats the call with room."""
    from pyflwdir_amd import _hip

    flw = _maker(BC.d8_of("flwdir0"), "flwdir0")("own", False)
    A = flw.upstream_area("km2").astype(np.float32).ravel()
    am = SC.threshold(A, "mid")
    sub, idxs, _ = _call(flw, A, am)
    assert idxs.size > flw.idxs_pit.size + 3 and sub.dtype == np.uint32 and idxs.dtype == flw.idxs_ds.dtype
    us = flw.main_upstream().astype(np.int64)
    us[us == flw._mv] = -1
    dA, dU = _hip.DeviceBuffer(A.nbytes).upload(A), _hip.DeviceBuffer(us.nbytes).upload(us)
    dmap, didx = _hip.DeviceBuffer(sub.nbytes), _hip.DeviceBuffer(idxs.nbytes)
    try:
        _, _, k, stats = flw._h.subbasins_area(dA, _hip.PFD_F32, am, _hip.PFD_COMPARE_OWN, dU, idxs.dtype, cap=idxs.size,
                                               out=dmap, idxs_out=didx, memspace=_hip.PFD_DEVICE)
        assert k == idxs.size and stats[1] >= 1
        assert _same(dmap.download(np.uint32, sub.shape), sub) and _same(didx.download(idxs.dtype, idxs.shape), idxs)
    finally:
        dA.free(), dU.free(), dmap.free(), didx.free()
    # the sizing convention, on the entry point itself
    k = C.c_int64(-1)
    small = np.full(3, -7, idxs.dtype)
    out = np.zeros(flw.size, np.uint32)
    _hip.check(_hip.lib().pfd_subbasins_area(flw._h._h, _hip.PFD_F32, _hip.ptr(A), float(am), _hip.PFD_COMPARE_OWN, None,
                                             _hip.IDX_CODE[np.dtype(idxs.dtype)], _hip.ptr(small), 3, C.byref(k), _hip.ptr(out),
                                             None, 0, _hip.PFD_HOST))
    assert k.value == idxs.size and (small == -7).all() and _same(out, sub)
    k0 = C.c_int64(-1)
    _hip.check(_hip.lib().pfd_subbasins_area(flw._h._h, _hip.PFD_F32, _hip.ptr(A), float(am), _hip.PFD_COMPARE_OWN, None,
                                             _hip.IDX_CODE[np.dtype(idxs.dtype)], None, 0, C.byref(k0), _hip.ptr(out), None, 0,
                                             _hip.PFD_HOST))
    assert k0.value == idxs.size
    again = _call(flw, A, am, cap=1)
    assert _same(again[0], sub) and _same(again[1], idxs)


@pytest.mark.parametrize("name", ["flwdir0", "synth_river_256", "synth_loops_96x80", "rhine"])
def test_subbasins_area_modes_and_rounds(gpu_lib, name):
    """The default areas run in the pruned mode, random areas in the full mode — decided by the closure check, not by
    the caller —; with the flag the full mode gives the pruned mode's bytes on the same input and runs more lane steps;
    with the default main upstream cells the rounds stay within ceil(log2(n_seq)) + 1 in every mode."""
    from pyflwdir_amd import _hip

    flw = _maker(BC.d8_of(name), name)("own", False)
    bound = math.ceil(math.log2(max(flw.idxs_seq.size, 2))) + 1
    for A in (flw.upstream_area("km2").ravel(), flw.upstream_area().ravel()):
        for t in ("mid", "big", "zero"):
            am = SC.threshold(A, t)
            sub, idxs, st = _call(flw, A, am)
            fsub, fidxs, fst = _call(flw, A, am, flags=_hip.PFD_SUBAREA_FULL)
            assert st[0] == 0 and fst[0] == 1, (t, st, fst)
            assert _same(fsub, sub) and _same(fidxs, idxs), t
            assert 1 <= st[1] <= bound and 1 <= fst[1] <= bound, (st, fst, bound)
            assert fst[3] >= st[3] and fst[2] >= st[2] >= flw.idxs_pit.size
    A = SC.random_areas(flw.size, 3)
    sub, idxs, st = _call(flw, A, 6.0)
    assert st[0] == 1 and 1 <= st[1] <= bound
    front = flw.subbasins_area(6.0, uparea=A.reshape(flw.shape))
    assert _same(front[0], sub.reshape(flw.shape)) and _same(front[1], idxs)


def _fuzz_areas(kind, cells, n, seed):
    if kind == "cells":
        return cells
    if kind == "float":
        return (cells * np.float32(1.7)).astype(np.float32)
    if kind == "random":
        return SC.random_areas(n, seed)
    return np.full(n, 2.5, np.float64)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", FUZZ_SHAPES)
def test_subbasins_area_random_rasters(gpu_lib, oracle, shape, seed):
    """Random D8 rasters (cycles, nodata, many pits) against the restated serial loop: monotone areas (int32 cell counts
    and float32), random float32 areas with NaNs, equal areas; thresholds that leave the pits only, a few outlets and
    thousands.  The device's mode, rounds, jobs and lane steps are those of the restated per-group form."""
    from pyflwdir_amd import _hip

    O = oracle
    rng = np.random.default_rng([SEED_BASE, shape[0], shape[1], seed])
    d8 = random_d8(rng, shape, p_nodata=rng.choice([0.0, 0.1]), p_pit=rng.choice([0.002, 0.02]), coherent=[-1, 2][seed])
    ds, pits, _ = O.from_array(d8)
    seq = O.idxs_seq(ds, pits)
    n = d8.size
    cells = O.accuflux(ds, seq, np.ones(n, np.int32), nodata=-9999)
    cells[ds == -1] = -9999
    usm = O.main_upstream(ds, cells)
    # (the handle itself: like the reference, the front end takes no raster of one cell)
    h = _hip.RasterHandle(d8, shape[0], shape[1])
    assert _same(h.idxs_seq(ds.dtype), seq)
    counts = {}
    for kind in ("cells", "float", "random", "equal"):
        A = _fuzz_areas(kind, cells, n, seed)
        top = float(np.nanmax(A))
        for t, am in (("none", top * 2 + 1), ("few", top * 0.3), ("many", 0 if kind != "random" else 1.0), ("neg", -1.0)):
            want_sub, want_idxs = SC.ref_serial(ds, seq, usm, A, am)
            sub, idxs, st = _call(h, A, am, idx_dtype=ds.dtype)
            assert _same(sub, want_sub) and _same(idxs, np.array(want_idxs, ds.dtype)), (kind, t)
            info = SC.ref_groups(ds, seq, usm, A, am)[2]
            assert st.tolist() == [info["mode"], info["rounds"], info["jobs"], info["steps"]], (kind, t, st, info)
            counts[kind, t] = (idxs.size, max(info["round_jobs"][1:], default=0))
    assert all(counts[k, "none"][0] == pits.size for k in ("cells", "float", "random", "equal"))
    if shape == (130, 257):
        assert counts["cells", "many"][0] > 1000 and counts["random", "many"][0] > pits.size + 100, counts
        # more than 256 jobs queued in one round: the append crosses waves and workgroups
        assert counts["cells", "many"][1] > 256 and counts["random", "many"][1] > 256, counts
        assert pits.size < counts["cells", "few"][0] < pits.size + 10, counts


def test_subbasins_area_refusals(gpu_lib, oracle, monkeypatch):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    d8, ds, pits, _ = BC.graph("flwdir1", oracle)
    flw = _maker(d8, "flwdir1")("own", False)
    general = pyflwdir.FlwdirRaster(idxs_ds=ds.copy(), shape=d8.shape, ftype="nextxy", idxs_pit=pits, cache=False)
    assert general._d8 is None
    with pytest.raises(NotImplementedError, match="general idxs_ds graph"):
        general.subbasins_area(10.0)
    k = C.c_int64(0)
    out = np.zeros(d8.size, np.uint32)
    rc = _hip.lib().pfd_subbasins_area(general._h._h, _hip.PFD_I32, None, 3.0, _hip.PFD_COMPARE_F64, None, _hip.PFD_I32, None, 0,
                                       C.byref(k), _hip.ptr(out), None, 0, _hip.PFD_HOST)
    assert rc == -7  # PFD_EUNSUPPORTED
    for dt in (np.uint8, np.float16, np.uint32):
        with pytest.raises(NotImplementedError, match="uparea dtype"):
            flw.subbasins_area(3, uparea=np.ones(d8.shape, dt))
    with pytest.raises(ValueError, match='"uparea" size does not match.'):
        flw.subbasins_area(3.0, uparea=np.ones(7))
    # an idxs_us_main entry that does not drain into its cell; one outside the raster; a cell listed for itself
    A = flw.upstream_area().ravel()
    us = flw.main_upstream().astype(np.int64)
    us[us == flw._mv] = -1
    p = int(np.flatnonzero(us >= 0)[0])
    other = next(c for c in range(d8.size) if ds[c] != p and ds[c] >= 0)
    for wrong, msg in ((other, "does not drain"), (d8.size, "outside the raster"), (p, "does not drain")):
        bad = us.copy()
        bad[p] = wrong
        with pytest.raises(ValueError, match=msg):
            _call(flw, A, 3, usm=bad)
    # a tributary above the threshold joins a cell without a main upstream cell
    none = np.full(d8.size, -1, np.int64)
    with pytest.raises(ValueError, match="no main upstream cell"):
        _call(flw, A, 0, usm=none)
    # an integer comparison with a threshold that is no integer
    with pytest.raises(ValueError, match="no value of the integer"):
        flw._h.subbasins_area(A, _hip.PFD_I32, 2.5, _hip.PFD_COMPARE_OWN, None, flw._idx_dtype)
    assert _call(flw, A, 3)[1].size >= pits.size  # (the handle serves the next call)
    # beyond 2**32 - 2 cells (the threshold lowered): refused before any kernel
    monkeypatch.setenv("PFD_TEST_BIG_CELLS", "40")
    blocked = _maker(d8, "flwdir1")("own", False)
    assert blocked._row_blocks_needed() > 1
    with pytest.raises(NotImplementedError, match="2\\*\\*32 - 2 cells"):
        blocked.subbasins_area(3.0)
