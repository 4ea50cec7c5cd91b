"""The tiled engines (tile_fast.h, tiled.hip) and the exact-order engine (exact.hip, exact_sweep.h) on acyclic rasters whose
paths WIND (tests/winding_cases.py; tests/test_winding_cases.py checks on the CPU that they do): random trees in all eight
directions whose paths leave a tile, a supertile or a row block and come back, one 4096-cell path per tile, one path over
the whole raster, a river that crosses a tile / supertile / hypertile edge at every step, a spiral around a tile corner.  Every
other random acyclic raster of the suite flows E / SE / S / SW only.

Every operation is compared byte for byte (NaNs by position) with the C oracle or the serial loops of tests/serial_refs.py:
no tolerances.  ``tile_local`` and ``exact_*`` segments in the call's timing show that the fast engines, not the level
engine, produced the results.

* ``test_counts_and_labels`` / ``test_float_sweeps`` / ``test_fills_and_outlets`` / ``test_path_operations``: every case on
  the default engines (the operation list of test_gpu_fuzz.py::test_random_rasters and what rides the same engines).
* ``test_engine_matrix``: a subset under each switch that selects another kernel form, capacity or fall-back.  The level
  engine (PFD_BASINS_LEVELS + PFD_EXACT_LEVELS) costs a launch per one or two cells of the longest path and runs only on
  cases whose longest path is at most 30000 hops: that leaves out serp_rows_130x2100 (272999 hops).
* ``test_row_blocks`` / ``test_row_blocks_refuse_what_cannot_settle``: the row-block protocols against the WHOLE raster's
  result."""
import functools
import os
import sys
import warnings
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_cases as W  # noqa: E402
import winding_cases as WC  # noqa: E402
from serial_refs import (_ref_down, _ref_floodplains, _ref_outlets, _ref_snap, _ref_step_length_f64,  # noqa: E402
                         _ref_streamorder, _ref_ucat_area, _ref_up, _ref_upstream_sum)

pytestmark = pytest.mark.gpu

LL_TRANSFORM = (1 / 1200.0, 0.0, 5.0, 0.0, -1 / 1200.0, 52.0)  # lat/lon: every row has its own cell area and step length
LEVELS_MAX_HOPS = 30000
NOT_HUGE = [n for n in WC.NAMES if n != WC.HUGE_SPIRAL]
MATRIX_NAMES = WC.SUBSET + ["serp_rows_130x2100"]  # (one path, ~520 supertile-edge crossings: the exit graph's round budget)
LEVELS_LEFT_OUT = ["serp_rows_130x2100"]


def _rng(name, salt):
    return np.random.default_rng([zlib.crc32(name.encode()), salt])


@functools.lru_cache(maxsize=None)
def _graph(name):
    """The oracle's graph of a case and the results several tests share: computed once, left unchanged."""
    from oracle import oracle as O

    c = WC.case(name)
    idxs_ds, idxs_pit, nvalid = O.from_array(c.d8)
    seq = O.idxs_seq(idxs_ds, idxs_pit)
    assert seq.size == nvalid and idxs_pit.size  # acyclic
    upa = O.accuflux(idxs_ds, seq, np.ones(c.n, np.int32), nodata=-9999)
    upa[idxs_ds == -1] = -9999
    rank = O.rank(idxs_ds)[0]
    for a in (idxs_ds, idxs_pit, seq, upa, rank):
        a.setflags(write=False)
    return SimpleNamespace(name=name, d8=c.d8, shape=c.shape, n=c.n, idxs_ds=idxs_ds, idxs_pit=idxs_pit, seq=seq, upa=upa, rank=rank,
                           nodata=idxs_ds == -1)


def _raster(g, latlon=False, profiling=False):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    kw = dict(transform=Affine(*LL_TRANSFORM), latlon=True) if latlon else {}
    flw = pyflwdir.from_array(g.d8, ftype="d8", cache=False, **kw)
    if profiling:
        flw._h.set_profiling(True)
    return flw


def _segments(flw):
    return [s["name"] for s in flw._h.last_timing()]


def same(got, exp):
    """dtype, size and bytes (NaNs by position and payload)."""
    got, exp = np.asarray(got), np.asarray(exp)
    return got.dtype == exp.dtype and got.size == exp.size and got.tobytes() == exp.tobytes()


def _fixed_point(O, g, flw):
    """upstream_area("km2", exact=False): taken (the raster is acyclic), and the split-sum reference of wide_cases."""
    from pyflwdir_amd import gis

    rows = np.ascontiguousarray(gis.area_rows(flw.transform, flw.shape, True, unit="m2") / gis.AREA_FACTORS["km2"])
    flw._last_quantum = None
    got = flw.upstream_area("km2", exact=False)
    assert flw._last_quantum is not None, "the fixed-point form did not take an acyclic raster"
    exp, _ = W.expected(O, g.d8, rows, flw._last_quantum, (g.idxs_ds, g.seq))
    assert got.dtype == np.float64 and got.shape == g.shape and got.tobytes() == exp.tobytes()


# ---- default engines, every case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WC.NAMES)
def test_counts_and_labels(gpu_lib, oracle, name):
    """The integer operations of the tiled engines: the graph and its order, upstream cell counts (eager and deferred
    handle), int32 / int64 accuflux, basins, and the fixed-point upstream area.  The int32 accumulation must show the
    ``tile_local`` segment: a silent fall-back to the level engine would make this file prove nothing."""
    from pyflwdir_amd import _hip

    O, g = oracle, _graph(name)
    rng = _rng(name, 1)
    flw = _raster(g, latlon=True, profiling=True)
    assert np.array_equal(flw.rank.ravel(), g.rank)
    assert same(flw.upstream_area().ravel(), g.upa)
    for deferred in (True, False) if name == "serp_rows_130x2100" else (True,):
        h = _hip.RasterHandle(g.d8, g.shape[0], g.shape[1], deferred=deferred)
        h.set_profiling(True)
        assert same(h.upstream_area_cell(), g.upa)
        if name == "serp_rows_130x2100":
            # ~520 supertile-edge crossings on one path do NOT exhaust the flat forest's round budget: one exit-graph solve,
            # no redo without a knob (test_engine_matrix forces the redo)
            assert [s["name"] for s in h.last_timing()].count("exit_graph") == 1, h.last_timing()
        h.close()
    wi32 = rng.integers(0, 1000 if g.n < 1 << 20 else 100, g.n).astype(np.int32)  # (the whole payload sums to less than 2^31)
    assert same(flw.accuflux(wi32.reshape(g.shape)).ravel(), O.accuflux(g.idxs_ds, g.seq, wi32))
    assert "tile_local" in _segments(flw), _segments(flw)
    assert same(flw.basins().ravel(), O.basins(g.idxs_ds, g.idxs_pit, g.seq))
    _fixed_point(O, g, flw)
    if name == WC.HUGE_SPIRAL:
        return
    assert np.array_equal(flw.idxs_ds, g.idxs_ds) and np.array_equal(flw.idxs_pit, g.idxs_pit)
    assert np.array_equal(flw.idxs_seq, g.seq)
    wi64 = rng.integers(-5, 1000, g.n).astype(np.int64)
    assert same(flw.accuflux(wi64.reshape(g.shape), nodata=-3).ravel(), O.accuflux(g.idxs_ds, g.seq, wi64, nodata=-3))
    oidx = np.unique(rng.integers(0, g.n, 17))
    oids = (np.arange(oidx.size) + 5).astype(np.uint16)
    assert same(flw.basins(idxs=oidx, ids=oids).ravel(), O.basins(g.idxs_ds, oidx.astype(g.idxs_ds.dtype), g.seq, oids))


@pytest.mark.parametrize("name", NOT_HUGE)
def test_float_sweeps(gpu_lib, oracle, name):
    """The ordered sweeps of the exact engine: float accuflux up and down, upstream area in km2, both stream orders, HAND,
    stream distance.  The float32 accumulation must show its ``exact_accuflux_up`` segment."""
    from pyflwdir_amd import gis

    O, g = oracle, _graph(name)
    rng = _rng(name, 2)
    shape, n = g.shape, g.n
    flw = _raster(g, profiling=True)
    w = rng.random(n).astype(np.float32)
    w[rng.random(n) < 0.05] = -9999
    assert same(flw.accuflux(w.reshape(shape)).ravel(), O.accuflux(g.idxs_ds, g.seq, w))
    assert "exact_accuflux_up" in _segments(flw), _segments(flw)
    assert same(flw.accuflux(w.reshape(shape), direction="down").ravel(), O.accuflux(g.idxs_ds, g.seq, w, direction="down"))
    w64 = rng.random(n) * 3.25
    assert same(flw.accuflux(w64.reshape(shape)).ravel(), O.accuflux(g.idxs_ds, g.seq, w64))
    mask = rng.random(n) < 0.6
    assert same(flw.stream_order().ravel(), O.strahler_order(g.idxs_ds, g.seq))
    assert same(flw.stream_order(mask=mask.reshape(shape)).ravel(), O.strahler_order(g.idxs_ds, g.seq, mask))
    main = O.main_upstream(g.idxs_ds, g.upa)
    assert np.array_equal(flw.idxs_us_main, main)
    assert same(flw.stream_order(type="classic", mask=mask.reshape(shape)).ravel(), O.stream_order_classic(g.idxs_ds, g.seq, main, mask))
    elev = (rng.random(n) * 100).astype(np.float32)
    drain = rng.random(n) < 0.1
    assert same(flw.hand(drain.reshape(shape), elev.reshape(shape)).ravel(), O.height_above_nearest_drain(g.idxs_ds, g.seq, drain, elev))
    assert same(flw.stream_distance(mask=mask.reshape(shape)).ravel(),
                O.stream_distance(g.idxs_ds, g.seq, shape[1], mask=mask, real_length=False))
    assert same(flw.stream_distance(unit="m").ravel(),
                O.stream_distance(g.idxs_ds, g.seq, shape[1], latlon=False, transform=tuple(flw.transform)[:6]))
    ll = _raster(g, latlon=True)
    area = np.ascontiguousarray(gis.area_grid(ll.transform, shape, True, unit="m2").ravel() / gis.AREA_FACTORS["km2"])
    exp = O.accuflux(g.idxs_ds, g.seq, area, nodata=-9999)
    exp[g.nodata] = -9999
    assert exp.dtype == np.float64 and same(ll.upstream_area("km2").ravel(), exp)


@pytest.mark.parametrize("name", NOT_HUGE)
def test_fills_and_outlets(gpu_lib, oracle, name):
    """fillnodata in the three forms of the fuzz test, subbasins_streamorder and basin_outlets against the serial loops."""
    g = _graph(name)
    rng = _rng(name, 3)
    shape, n = g.shape, g.n
    flw = _raster(g)
    f32 = np.where(rng.random(n) < 0.3, np.float32(-9999), rng.integers(-8, 9, n).astype(np.float32) / 4)
    i32 = np.where(rng.random(n) < 0.3, 0, rng.integers(-5, 1000, n)).astype(np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for data, nd, direction, how in ((f32, -9999.0, "up", "max"), (f32, -9999.0, "down", "sum"), (i32, 0, "down", "max")):
            exp = _ref_up(g.idxs_ds, g.seq, data, nd) if direction == "up" else _ref_down(g.idxs_ds, g.seq, data, nd, how)
            got = flw.fillnodata(data.reshape(shape), nd, direction=direction, how=how)
            assert got.shape == shape and same(got, exp), (direction, how)
    dsl, sql = g.idxs_ds.tolist(), g.seq.tolist()
    strord = flw.stream_order()
    sub_o, out_o = _ref_streamorder(dsl, sql, strord.ravel().tolist(), -2)
    sub, out = flw.subbasins_streamorder(strord=strord, min_sto=-2)
    assert same(sub.ravel(), np.array(sub_o, np.int32)) and same(out, np.array(out_o, g.idxs_ds.dtype))
    bas = flw.basins()
    lbs_o, out_o = _ref_outlets(dsl, sql, bas.ravel().tolist())
    order = np.argsort(np.array(lbs_o, bas.dtype), kind="stable")
    lbs, out = flw.basin_outlets(bas)
    assert same(lbs, np.array(lbs_o, bas.dtype)[order]) and same(out, np.array(out_o, g.idxs_ds.dtype)[order])


@pytest.mark.parametrize("name", NOT_HUGE)
def test_path_operations(gpu_lib, oracle, name):
    """floodplains, snap in both directions, upstream_sum and ucat_area against the serial loops of tests/serial_refs.py."""
    from pyflwdir_amd import gis

    O, g = oracle, _graph(name)
    rng = _rng(name, 4)
    shape, n = g.shape, g.n
    flw = _raster(g, latlon=True)
    # floodplains: streams from a tenth of the cells (no accumulation: exact square roots), small integer elevations
    upa = rng.choice((1, 16, 81, 256, 625), n, p=(0.45, 0.25, 0.2, 0.06, 0.04)).astype(np.float32)
    upa[g.nodata] = -9999
    elev = rng.integers(0, 40, n).astype(np.float32)
    exp = _ref_floodplains(g.idxs_ds, g.seq, elev, upa, 256, 0.5)
    assert same(flw.floodplains(elev.reshape(shape), uparea=upa.reshape(shape), upa_min=256, b=0.5).ravel(), exp)
    # snap: downstream in cells to a mask of 5 % of the cells; upstream along the main upstream cells in metres, bounded
    starts = rng.integers(0, n, 64).astype(np.int64)
    starts[:2] = (0, n - 1)
    mask = rng.random(n) < 0.05
    exp_i, exp_d = _ref_snap(starts, g.idxs_ds, -1, mask.tolist(), None, lambda a, b: 1.0)
    got_i, got_d = flw.snap(idxs=starts, mask=mask.reshape(shape))
    assert same(got_i, exp_i) and same(got_d, exp_d)
    main = O.main_upstream(g.idxs_ds, g.upa)
    max_length = 37.5 * float(np.median(gis.step_length_table(shape[0], True, LL_TRANSFORM, dtype=np.float64)))
    step = functools.lru_cache(maxsize=None)(lambda a, b: _ref_step_length_f64(a, b, shape[1], True, LL_TRANSFORM))
    exp_i, exp_d = _ref_snap(starts, main, -1, None, max_length, step)
    got_i, got_d = flw.snap(idxs=starts, unit="m", direction="up", max_length=max_length)
    assert same(got_i, exp_i) and same(got_d, exp_d)
    # upstream_sum: float32 with full mantissas, a fifth of the cells missing
    data = (rng.standard_normal(n) * 1000).astype(np.float32)
    data[rng.random(n) < 0.2] = -9999
    assert same(flw.upstream_sum(data.reshape(shape), mv=-9999).ravel(), _ref_upstream_sum(g.idxs_ds, data, -9999, -1))
    # ucat_area: 40 outlets (a pit, a missing entry, a repeated one among them), in cells and in km2
    valid = np.flatnonzero(~g.nodata)
    outs = rng.choice(valid, 40).astype(g.idxs_ds.dtype)
    outs[3], outs[7], outs[11] = g.idxs_pit[0], -1, outs[0]
    for unit in ("cell", "km2"):
        area = np.ones(n, np.int32) if unit == "cell" else \
            np.ascontiguousarray(gis.area_grid(flw.transform, shape, True, unit="m2").ravel() / gis.AREA_FACTORS[unit])
        exp_m, exp_a = _ref_ucat_area(outs, g.idxs_ds, g.seq, area, -1)
        got_m, got_a = flw.ucat_area(outs, unit=unit)
        assert same(got_m.ravel(), exp_m) and same(got_a, exp_a), unit


# ---- the engine matrix -------------------------------------------------------------------------------------------------------------
KNOBS = {
    "tile_general": dict(PFD_TILE_GENERAL="1"),            # the frame kernel k_tile on every tile
    "hyper_small": dict(PFD_HYPER_SMALL="1"),              # hypertile solves instead of the flat forest
    "flat_l3": dict(PFD_FLAT_L3="1"),
    "rounds4": dict(PFD_TEST_ROUNDS4="1"),                 # too few rounds issued: the miss is noticed, the pass redone
    "scap0": dict(PFD_TEST_SCAP="0"),                      # the positional supertile kernel
    "hcap100": dict(PFD_TEST_HCAP="100", PFD_HYPER_SMALL="1"),
    "fuse_min": dict(PFD_TEST_FUSE_MIN="1048576"),         # production's lane-per-chain short path
    "scan_unfused": dict(PFD_SCAN_UNFUSED="1"),
    "dscan_global": dict(PFD_DSCAN_GLOBAL="1"),
    "wide_unfused": dict(PFD_WIDE_UNFUSED="1"),            # the fixed-point call's separate local pass
    "levels": dict(PFD_BASINS_LEVELS="1", PFD_EXACT_LEVELS="1"),
}
WITH_FIXED_POINT = ("tile_general", "hyper_small", "flat_l3", "rounds4", "hcap100", "wide_unfused")
MATRIX = [(k, n) for k in KNOBS for n in MATRIX_NAMES if not (k == "levels" and n in LEVELS_LEFT_OUT)]


@functools.lru_cache(maxsize=None)
def _matrix_refs(name):
    """Inputs and expected results of the matrix operations of a case: computed once, shared by every switch."""
    from oracle import oracle as O

    g = _graph(name)
    rng = _rng(name, 5)
    n = g.n
    wi32 = rng.integers(0, 1000, n).astype(np.int32)
    w = rng.random(n).astype(np.float32)
    w[rng.random(n) < 0.05] = -9999
    elev = (rng.random(n) * 100).astype(np.float32)
    drain = rng.random(n) < 0.1
    mask = rng.random(n) < 0.6
    return SimpleNamespace(
        wi32=wi32, w=w, elev=elev, drain=drain, mask=mask,
        acc_i32=O.accuflux(g.idxs_ds, g.seq, wi32), basins=O.basins(g.idxs_ds, g.idxs_pit, g.seq),
        acc_up=O.accuflux(g.idxs_ds, g.seq, w), acc_down=O.accuflux(g.idxs_ds, g.seq, w, direction="down"),
        strahler=O.strahler_order(g.idxs_ds, g.seq), hand=O.height_above_nearest_drain(g.idxs_ds, g.seq, drain, elev),
        dist=O.stream_distance(g.idxs_ds, g.seq, g.shape[1], mask=mask, real_length=False))


@pytest.mark.parametrize("knob,name", MATRIX)
def test_engine_matrix(gpu_lib, oracle, monkeypatch, knob, name):
    """upstream_area, int32 accuflux, basins, rank, float32 accuflux up and down, Strahler, HAND and stream_distance under
    each switch: the same bytes as on the default engines, which are the oracle's."""
    O, g, r = oracle, _graph(name), _matrix_refs(name)
    if knob == "levels":
        assert int(g.rank.max()) <= LEVELS_MAX_HOPS
    else:
        assert name not in LEVELS_LEFT_OUT or int(g.rank.max()) > LEVELS_MAX_HOPS
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    shape = g.shape
    flw = _raster(g, latlon=True, profiling=True)
    assert same(flw.upstream_area().ravel(), g.upa)
    if knob == "rounds4" and name in ("serp_rows_130x2100", "tree_130x2100_p1"):
        # the forced miss is noticed and the pass redone: a second exit-graph solve in the call's timing (without a knob the
        # budget suffices on both)
        assert _segments(flw).count("exit_graph") >= 2, _segments(flw)
    if knob == "hyper_small" and name == "serp_rows_130x2100":  # (the hypertile form falls short there by itself: one redo)
        assert _segments(flw).count("exit_graph") == 2, _segments(flw)
    assert same(flw.accuflux(r.wi32.reshape(shape)).ravel(), r.acc_i32)
    assert "tile_local" in _segments(flw), _segments(flw)
    assert same(flw.basins().ravel(), r.basins)
    assert np.array_equal(flw.rank.ravel(), g.rank)
    assert same(flw.accuflux(r.w.reshape(shape)).ravel(), r.acc_up)
    assert ("exact_accuflux_up" in _segments(flw)) == (knob != "levels"), _segments(flw)
    assert same(flw.accuflux(r.w.reshape(shape), direction="down").ravel(), r.acc_down)
    assert same(flw.stream_order().ravel(), r.strahler)
    assert same(flw.hand(r.drain.reshape(shape), r.elev.reshape(shape)).ravel(), r.hand)
    assert same(flw.stream_distance(mask=r.mask.reshape(shape)).ravel(), r.dist)
    if knob in WITH_FIXED_POINT:
        _fixed_point(O, g, flw)


# ---- row blocks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nb", [(n, nb) for n, nbs in WC.ROW_BLOCKS for nb in nbs])
def test_row_blocks(gpu_lib, oracle, name, nb):
    """The row-block protocols against the WHOLE raster's oracle / serial result; every own cell's local equation holds
    where the call can check it.  The fixpoint sweeps exchange boundary rows once per block-edge crossing of the longest
    path (tests/test_winding_cases.py counts them); where that is more than dist.MAX_ROUNDS — the river that crosses the edge
    between its two blocks 299 times, the column boustrophedon in three blocks — ``max_iter`` is raised to what the count says."""
    import verifier_cases as VC
    from pyflwdir_amd import _hip, dist

    O, g = oracle, _graph(name)
    rng = _rng(name, 6)
    d8, shape, n = g.d8, g.shape, g.n
    for deferred in (False, True):
        assert same(dist.upstream_area_blocks(d8, nb, deferred=deferred).ravel(), g.upa), deferred
    assert same(dist.basins_blocks(d8, nb, g.idxs_pit).ravel(), O.basins(g.idxs_ds, g.idxs_pit, g.seq))
    crossings = WC.ROW_BLOCK_CROSSINGS[name, nb]
    over = (name, nb) in WC.OVER_MAX_ROUNDS
    assert over == (crossings >= dist.MAX_ROUNDS)
    kw = dict(max_iter=crossings + 2) if over else {}
    elev = (rng.random(n) * 100).astype(np.float32)
    drain = rng.random(n) < 0.1
    got, iters = dist.hand_blocks(d8, nb, drain, elev)
    assert iters >= 1 and same(got.ravel(), O.height_above_nearest_drain(g.idxs_ds, g.seq, drain, elev))
    # (no nodata in the payload: a nodata cell is left out of the sums, which would cut the chain of dependencies along the
    #  winding path — every value is positive, so a sum is wrong until everything upstream of it has arrived, and the
    #  sweeps cannot settle in fewer exchanges than the longest path crosses block edges)
    w = (rng.random(n) * 3.7 + 1e-3).astype(np.float32)
    for direction in ("up", "down"):
        got, rounds, bad = dist.accuflux_blocks(d8, nb, w, (-9999, -9999.0, 1), verify=True, direction=direction, **kw)
        assert bad == 0 and rounds >= crossings, (direction, rounds, bad)
        assert same(got.ravel(), O.accuflux(g.idxs_ds, g.seq, w, nodata=-9999, direction=direction)), (direction, rounds)
    got, rounds, bad = dist.strahler_blocks(d8, nb, verify=True, **kw)
    assert bad == 0 and same(got.ravel(), O.strahler_order(g.idxs_ds, g.seq)), rounds
    mask = (rng.random(n) < 0.6).astype(np.uint8)
    got, rounds, bad = dist.stream_distance_blocks(d8, nb, mask, verify=True, **kw)
    assert bad == 0 and same(got.ravel(), O.stream_distance(g.idxs_ds, g.seq, shape[1], mask=mask, real_length=False)), rounds
    main = O.main_upstream(g.idxs_ds, g.upa)
    got, rounds, bad = dist.classic_blocks(d8, nb, g.upa.reshape(shape), mask, verify=True, **kw)
    assert bad == 0 and same(got.ravel(), O.stream_order_classic(g.idxs_ds, g.seq, main, mask)), rounds
    stream = (rng.random(n) < 0.1).astype(np.uint8)
    hs = np.where(stream, rng.integers(0, 25, n), 0).astype(np.float32)
    flood_elev = rng.integers(0, 40, n).astype(np.float32)
    got, rounds, bad = dist.floodplains_blocks(d8, nb, flood_elev.reshape(shape), stream.reshape(shape), hs.reshape(shape), verify=True, **kw)
    exp = VC.flood_state(g.idxs_ds, g.seq, flood_elev, stream, hs)["flag"].astype(np.int8)
    assert bad == 0 and same(got.ravel(), exp), rounds
    f32 = np.where(rng.random(n) < 0.3, np.float32(-9999), rng.integers(-8, 9, n).astype(np.float32) / 4)
    for direction, how, hw in (("down", "sum", _hip.PFD_FILL_SUM), ("up", "max", _hip.PFD_FILL_MAX)):
        exp = _ref_up(g.idxs_ds, g.seq, f32, -9999.0) if direction == "up" else _ref_down(g.idxs_ds, g.seq, f32, -9999.0, how)
        got, rounds, bad = dist.fillnodata_blocks(d8, nb, f32.reshape(shape), _hip.PFD_F32, (0, -9999.0, 1), direction=direction,
                                                  how=hw, verify=True, **kw)
        assert bad == 0 and same(got.ravel(), exp), (direction, rounds)


def test_row_blocks_refuse_what_cannot_settle(gpu_lib, oracle):
    """A river that crosses the edge between two row blocks 299 times needs 299 exchanges: with ``max_iter=8`` the call
    raises the documented error instead of returning a raster that has not settled."""
    from pyflwdir_amd import dist

    name, nb, max_iter = WC.REFUSED
    g = _graph(name)
    w = (_rng(name, 7).random(g.n) + 0.5).astype(np.float32)
    for direction in ("up", "down"):
        with pytest.raises(NotImplementedError, match="did not settle in 8 rounds"):
            dist.accuflux_blocks(g.d8, nb, w, (-9999, -9999.0, 1), max_iter=max_iter, direction=direction)
