"""FlwdirRaster.interbasin_mask / inflow_idxs / basin_bounds / subbasins_pfafstetter (reference pyflwdir/pyflwdir.py:
742-766, :804-818, :694-718, :631-663) on the device: dtype, shape and bytes against the reference's recorded outputs
(tests/golden/wide_basins.npz, tools/gen_golden_basins.py) through both engines, on a general graph and on random D8
rasters against the restated serial loops (tests/basin_cases.py), the paths beyond 2**32 - 2 cells with the thresholds
lowered, and the error paths."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basin_cases as BC  # noqa: E402
from golden_util import digest  # noqa: E402
from test_gpu_fuzz import random_d8  # noqa: E402  (the generator of test_gpu_fuzz_paths.py)

pytestmark = pytest.mark.gpu

# the smallest shapes that put walks and chains across 64 x 64 tile edges and the 256-thread grid edge
FUZZ_SHAPES = [(63, 65), (64, 64), (65, 129), (1, 257)]
FUZZ_SEEDS = [0, 1, 2]  # per shape; per depth at most half of the 12 rasters hold a Pfafstetter tie (test_basin_cases.py)
SEED_BASE = 9100
# area thresholds of the Pfafstetter fuzz: in uniformly random rasters three streams meet in one cell all over, and two
# tributaries that join the same cell have equal second sort keys; with a threshold only the larger streams take part
FUZZ_UPA_MIN = {1: 6.0, 2: 12.0, 3: 12.0}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _flw(d8, name="", kind="own", **kw):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    if name:
        tr, latlon = BC.transform_of(name, kind)
        kw.update(transform=Affine(*tr), latlon=latlon)
    return pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False, **kw)


@pytest.mark.parametrize("engine", ["exact", "levels"])
@pytest.mark.parametrize("name", BC.RASTERS)
def test_basins_ext_golden(gpu_lib, monkeypatch, name, engine):
    """Every recorded case of one raster (8 golden rasters incl. one with cycles and two strips, and the confluence
    raster): 4 regions x 2 stream masks, 4 regions, 2 basin maps x 2 transforms, and the tie-free ones of 3 depths x 2
    areas x 2 thresholds."""
    if engine == "levels":
        monkeypatch.setenv("PFD_EXACT_LEVELS", "1")
    G = np.load(os.path.join(BC.GOLD, "wide_basins.npz"))
    d8 = BC.d8_of(name)
    flws = {kind: _flw(d8, name, kind) for kind in BC.TRANSFORMS}
    cache, bad, n = {}, [], 0
    for key, call, args in BC.keys(name):
        if call == "pfaf" and bool(G[f"tie_{key}"]):
            continue
        outs = BC.run(flws[args[1]] if call == "bounds" else flws["own"], call, args, cache)
        for i, got in enumerate(outs):
            got = np.asarray(got)
            ok = _same(got, G[f"out_{key}_{i}"]) if name in BC.FULL else digest(got) == str(G[f"digest_{key}_{i}"])
            n += 1
            if not ok:
                bad.append(f"{key}_{i}")
    assert n >= 8 + 4 + 12 and not bad, bad[:20]


def fuzz_case(O, shape, seed):
    """The random raster of (shape, seed) with what the serial loops need: graph, sequence, a region, a stream mask, a
    label map, and areas without equal values (the upstream cell count plus a fraction)."""
    from types import SimpleNamespace

    rng = np.random.default_rng([SEED_BASE, shape[0], shape[1], seed])
    d8 = random_d8(rng, shape, p_nodata=rng.choice([0.0, 0.1]), p_pit=rng.choice([0.002, 0.02]), coherent=rng.choice([1, 2, 4, -1]))
    ds, pits, _ = O.from_array(d8)
    seq = O.idxs_seq(ds, pits)
    n = d8.size
    cells = O.accuflux(ds, seq, np.ones(n, np.int32), nodata=-9999)
    cells[ds == -1] = -9999
    upa = cells + rng.random(n) * 0.5
    region = BC.region(shape, "checker") ^ (rng.random(shape) < 0.1)
    labels = (rng.integers(0, 6, (-(-shape[0] // 5), -(-shape[1] // 7))).repeat(5, 0).repeat(7, 1)[:shape[0], :shape[1]]).astype(np.int32)
    return SimpleNamespace(d8=d8, shape=shape, ds=ds, pits=pits, seq=seq, cells=cells, upa=upa, region=region,
                           stream=rng.random(shape) < 0.02, labels=labels, us_main=O.main_upstream(ds, cells))


def fuzz_pfaf(c, depth):
    """(upa_min, expected map, expected outlets, ties) of a fuzz raster at one depth."""
    upa_min = FUZZ_UPA_MIN[depth]
    pf, idxs, info = BC._ref_pfafstetter(c.pits, c.ds, c.seq, c.us_main, c.upa, c.upa >= upa_min, depth)
    return upa_min, pf.reshape(c.shape), np.array(idxs, c.ds.dtype), info["ties"]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
@pytest.mark.parametrize("shape", FUZZ_SHAPES)
def test_basins_ext_random_rasters(gpu_lib, oracle, shape, seed):
    """Random D8 rasters (cycles, nodata, many pits) against the serial loops; Pfafstetter seeds with ties are left out."""
    c = fuzz_case(oracle, shape, seed)
    flw = _flw(c.d8)
    for stream in (None, c.stream):
        assert _same(flw.interbasin_mask(c.region, stream=stream),
                     BC._ref_interbasin(c.ds, c.seq, c.region, stream).reshape(shape)), stream is None
    assert _same(flw.inflow_idxs(c.region), np.array(BC._ref_inflow(c.ds, c.seq, c.region), c.ds.dtype))
    for got, want in zip(flw.basin_bounds(c.labels), BC._ref_bounds(c.labels, flw.transform)):
        assert _same(got, want)
    for depth in BC.DEPTHS:
        upa_min, pf, idxs, ties = fuzz_pfaf(c, depth)
        if ties:
            continue
        got = flw.subbasins_pfafstetter(depth=depth, uparea=c.upa.reshape(shape), upa_min=upa_min)
        assert _same(got[0], pf) and _same(got[1], idxs), depth


# (raster, area threshold at which its Pfafstetter cases hold no tie — checked on the CPU; None: ties at every threshold)
GENERAL = [("flwdir0", 8.0), ("flwdir1", 4.0), ("synth_loops_96x80", None), (BC.CORNER, 0.0)]


@pytest.mark.parametrize("name,upa_min", GENERAL)
def test_basins_ext_general_graph(gpu_lib, oracle, name, upa_min):
    """The same downstream links as a general idxs_ds graph (rank-sorted sequence): the four methods against the serial
    loops over the handle's own sequence; Pfafstetter on the upstream cell count plus a fraction."""
    import pyflwdir_amd as pyflwdir

    d8, ds, pits, _ = BC.graph(name, oracle)
    shape = d8.shape
    flw = pyflwdir.FlwdirRaster(idxs_ds=ds.copy(), shape=shape, ftype="nextxy", idxs_pit=pits, cache=False)
    assert flw._d8 is None
    seq = flw.idxs_seq
    stream = flw.upstream_area() > 5
    for kind in ("rect", "checker"):
        region = BC.region(shape, kind)
        for s in (None, stream):
            assert _same(flw.interbasin_mask(region, stream=s), BC._ref_interbasin(ds, seq, region, s).reshape(shape))
        assert _same(flw.inflow_idxs(region), np.array(BC._ref_inflow(ds, seq, region), ds.dtype))
    for got, want in zip(flw.basin_bounds(), BC._ref_bounds(flw.basins(), flw.transform)):
        assert _same(got, want)
    cells = flw.upstream_area().ravel()
    upa = cells + np.random.default_rng(5).random(cells.size) * 0.5
    us_main = oracle.main_upstream(ds, cells)
    for depth in (1, 2) if upa_min is not None else ():
        pf, idxs, info = BC._ref_pfafstetter(flw.idxs_pit, ds, seq, us_main, upa, upa >= upa_min, depth)
        got = flw.subbasins_pfafstetter(depth=depth, uparea=upa.reshape(shape), upa_min=upa_min)
        assert not info["ties"] and len(idxs) > flw.idxs_pit.size
        assert _same(got[0], pf.reshape(shape)) and _same(got[1], np.array(idxs, ds.dtype)), depth


def test_basins_ext_wide_and_row_blocks(gpu_lib, oracle, monkeypatch):
    """Beyond 2**32 - 2 cells with the thresholds lowered: the front end in row-block mode (PFD_TEST_BIG_CELLS) and the
    library's 64-bit sequence and links (PFD_TEST_ORDER64) give the single-handle bytes of interbasin_mask, inflow_idxs
    and basin_bounds; subbasins_pfafstetter names the primitives that have no one-handle form there."""
    shape = (300, 260)
    d8 = oracle.synth_d8(shape[0], shape[1], seed=61, tilt=100000, white=2, nodata_pct=15)
    region = BC.region(shape, "checker")

    def calls(flw):
        stream = flw.upstream_area() > 30
        return [flw.interbasin_mask(region), flw.interbasin_mask(region, stream=stream), flw.inflow_idxs(region),
                *flw.basin_bounds()]

    one = _flw(d8)
    whole = calls(one)
    ds, seq = one.idxs_ds, one.idxs_seq
    assert _same(whole[2], np.array(BC._ref_inflow(ds, seq, region), ds.dtype)) and whole[2].size > 50
    assert _same(whole[1], BC._ref_interbasin(ds, seq, region, one.upstream_area() > 30).reshape(shape))
    monkeypatch.setenv("PFD_TEST_BIG_CELLS", "20000")
    blocked = _flw(d8)
    assert blocked._row_blocks_needed() >= 4
    for g, w in zip(calls(blocked), whole):
        assert _same(g, w)
    with pytest.raises(NotImplementedError, match="pfd_main_upstream"):
        blocked.subbasins_pfafstetter()
    monkeypatch.setenv("PFD_TEST_ORDER64", "1")
    wide = _flw(d8)
    assert wide._wide()
    for g, w in zip(calls(wide), whole):
        assert _same(g, w)


def test_basins_ext_errors_and_dtypes(gpu_lib):
    d8 = BC.d8_of("flwdir1")
    flw = _flw(d8, "flwdir1")
    with pytest.raises(ValueError, match="No regions found in data"):
        flw.basin_bounds(np.zeros(d8.shape, np.int32))
    with pytest.raises(ValueError, match='"basins" shape does not match.'):
        flw.basin_bounds(np.ones(7, np.int32))
    with pytest.raises(ValueError, match='"region" size does not match.'):
        flw.interbasin_mask(np.ones(7, bool))
    with pytest.raises(ValueError, match='"stream" size does not match.'):
        flw.interbasin_mask(np.ones(d8.shape, bool), stream=np.ones(7, bool))
    with pytest.raises(ValueError, match='"region" size does not match.'):
        flw.inflow_idxs(np.ones(7, bool))
    with pytest.raises(ValueError, match='"uparea" size does not match.'):
        flw.subbasins_pfafstetter(uparea=np.ones(7))
    with pytest.raises(ValueError):
        flw.subbasins_pfafstetter(upa_min=None)
    with pytest.raises(ValueError):
        flw.subbasins_pfafstetter(depth=0)
    with pytest.raises(NotImplementedError):
        flw.basin_bounds(flw.basins().astype(np.float32))
    # every integer dtype of the labels gives the same boxes; the labels come back in the map's dtype
    sub = flw.subbasins_streamorder(min_sto=-1)[0]
    want = flw.basin_bounds(sub)
    for dt in (np.int8, np.uint8, np.int16, np.uint32, np.int64, np.uint64):
        got = flw.basin_bounds(sub.astype(dt))
        assert got[0].dtype == dt and np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[2])
    # negative labels are background; a list longer than the first call's room: the binding repeats the call
    neg = sub.copy()
    neg[sub == 1] = -3
    assert np.array_equal(flw.basin_bounds(neg)[0], want[0][want[0] != 1])
    lbs, rc = flw._h.basin_bounds(np.ascontiguousarray(sub).ravel(), 1, cap=1)
    assert _same(lbs, want[0]) and rc.shape == (4, lbs.size) and lbs.size > 1
    assert _same(flw._h.inflow_idxs(np.ascontiguousarray(BC.region(d8.shape, "checker")).ravel().view(np.uint8), np.int32, cap=1),
                 flw.inflow_idxs(BC.region(d8.shape, "checker")))
    # the cached main upstream cells are what the reference uses: the same answer as computing them on the device
    cached = _flw(d8, "flwdir1")
    cached.cache = True
    cached.main_upstream()
    assert "idxs_us_main" in cached._cached
    for a, b in zip(cached.subbasins_pfafstetter(depth=2), flw.subbasins_pfafstetter(depth=2)):
        assert _same(a, b)


def test_pfafstetter_second_lap(gpu_lib):
    """An outlet list longer than the first call's room (cap=1 on the 5 x 7 raster: 4 outlets): the binding repeats the
    call with room for all, and gives the default capacity's map and list."""
    from pyflwdir_amd import _hip

    flw = _flw(BC.d8_of("synth_tiny_5x7"))
    upa_min = BC.threshold(flw.upstream_area())
    sub, idxs = flw.subbasins_pfafstetter(depth=1, upa_min=upa_min)
    s2, i2 = flw._h.subbasins_pfafstetter(None, _hip.PFD_I32, upa_min, 1, None, flw.idxs_pit, idxs.dtype, cap=1)
    assert idxs.size >= 2 and _same(s2.reshape(sub.shape), sub) and _same(i2, idxs)
