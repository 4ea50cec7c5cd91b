"""Adversarial general ``idxs_ds`` graphs (tests/general_graphs.py) through the general engine (csrc/general.hip), every
operation bit for bit against the CPU oracle or the serial loops of tests/serial_refs.py: in-degrees up to 100, links
across the whole index range, one level to 3000 levels, trees hanging off cycles, node counts at the 256-thread grid
edges, the three index dtypes, and an installed ``sort`` order over long upstream lists (the float sums depend on it).
tests/test_general_graphs.py shows on the CPU that every case is inside the oracle's domain.

``stream_distance(unit="m")`` is not covered: the oracle's step table holds the lengths of neighbour steps and says
nothing about a link to a far cell.  ``snap``, ``ucat_area``, ``floodplains`` and ``upstream_sum`` refuse general graphs.

Two kinds of case can not be told from a D8 raster by their links (general_graphs.cannot_be_general: the 1 x 2 raster
and the graphs of pits alone); they are put on the general engine with ``ftype="nextxy"``, which never takes the D8
engines, and are walked breadth-first like the others."""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as FC  # noqa: E402
import general_graphs as GG  # noqa: E402
import outlet_cases as OC  # noqa: E402
from serial_refs import _ref_down, _ref_outflow, _ref_outlets, _ref_streamorder, _ref_up  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [GG.case_id(c) for c in GG.CASES]


class _Check:
    """Comparisons that name the case, the operation and the first differing cell."""

    def __init__(self, c, stage=""):
        self.c, self.stage = c, stage

    def __call__(self, what, got, exp, shape=None):
        got, exp = np.asarray(got), np.asarray(exp)
        tag = f"{GG.case_id(self.c)} {self.stage}{what}"
        assert got.dtype == exp.dtype, (tag, got.dtype, exp.dtype)
        if shape is not None:
            assert got.shape == tuple(shape), (tag, got.shape, shape)
            got = got.ravel()
        assert got.shape == exp.shape, (tag, got.shape, exp.shape)
        if not np.array_equal(got, exp, equal_nan=got.dtype.kind == "f"):
            diff = got != exp
            if got.dtype.kind == "f":
                diff &= ~(np.isnan(got) & np.isnan(exp))
            i = int(np.flatnonzero(diff)[0])
            raise AssertionError(f"{tag}: {int(diff.sum())} cells differ, first at {i}: got {got[i]!r}, expected {exp[i]!r}")

    def bytes(self, what, got, exp, shape=None):
        """The payloads of fill_cases hold NaN and -0.0: bytes, like tests/test_gpu_fillnodata.py."""
        got = np.asarray(got)
        self(what, got, exp, shape)
        assert got.tobytes() == exp.tobytes(), f"{GG.case_id(self.c)} {self.stage}{what}: equal values, other bytes"


def _build(c, ds):
    import pyflwdir_amd as pyflwdir

    if GG.cannot_be_general(c):
        flw = pyflwdir.FlwdirRaster(idxs_ds=ds, shape=c["shape"], ftype="nextxy", cache=False)
        flw.order_cells("walk")
    else:
        flw = pyflwdir.FlwdirRaster(idxs_ds=ds, shape=c["shape"], ftype="d8", cache=False)
    assert flw._d8 is None and flw._h.is_general
    return flw


def _sorted_seq(O, ds):
    rnk = O.rank(ds)[0]
    n = int(np.sum(rnk >= 0))
    return np.argsort(rnk)[-n:].astype(ds.dtype)  # (the expression of FlwdirRaster.order_cells("sort"))


def _payloads(c, n):
    rng = np.random.default_rng(7000 + c["seed"])
    P = {}
    P["w32"] = rng.random(n).astype(np.float32)
    P["w32nd"] = P["w32"].copy()
    P["w32nd"][rng.random(n) < 0.05] = -9999
    P["w64"] = rng.random(n)
    P["wi32"] = rng.integers(0, 1000, n).astype(np.int32)
    P["wi64"] = rng.integers(-5, 1000, n).astype(np.int64)
    P["ties"] = rng.integers(0, 4, n).astype(np.float32)  # many equal "areas" among the upstream cells of a cell
    P["mask"] = rng.random(n) < 0.6
    P["oidx"] = rng.integers(0, n, 17)
    P["oidx"][-1] = P["oidx"][0]  # a repeated outlet: the last id wins
    P["oids"] = (np.arange(17) + 5).astype(np.uint16)
    P["elev32"] = (rng.random(n) * 100).astype(np.float32)
    P["elev64"] = rng.random(n) * 100
    P["drain"] = rng.random(n) < 0.1
    P["f32"] = FC.payload(n, "float32", -9999.0, salt=c["seed"])
    P["i32"] = FC.payload(n, "int32", 0, salt=c["seed"])
    return P


def _accuflux_checks(O, eq, flw, ds, seq, P, shape, both_f64=False):
    first = flw.accuflux(P["w32"].reshape(shape))
    eq("accuflux f32 up", first, O.accuflux(ds, seq, P["w32"]), shape)
    eq("accuflux f32 nodata up", flw.accuflux(P["w32nd"].reshape(shape)), O.accuflux(ds, seq, P["w32nd"]), shape)
    eq("accuflux f32 nodata down", flw.accuflux(P["w32nd"].reshape(shape), direction="down"),
       O.accuflux(ds, seq, P["w32nd"], direction="down"), shape)
    eq("accuflux f64 down", flw.accuflux(P["w64"].reshape(shape), direction="down"),
       O.accuflux(ds, seq, P["w64"], direction="down"), shape)
    if both_f64:
        eq("accuflux f64 up", flw.accuflux(P["w64"].reshape(shape)), O.accuflux(ds, seq, P["w64"]), shape)
    return first


def _hand_checks(O, eq, flw, ds, seq, P, shape):
    for key in ("elev32", "elev64"):
        eq("hand " + key, flw.hand(P["drain"].reshape(shape), P[key].reshape(shape)),
           O.height_above_nearest_drain(ds, seq, P["drain"], P[key]), shape)


@pytest.mark.parametrize("c", GG.CASES, ids=IDS)
def test_general_graph(gpu_lib, oracle, c):
    O = oracle
    shape = c["shape"]
    n = shape[0] * shape[1]
    ds = GG.build(c)
    valid = ds != -1
    pits = np.flatnonzero(valid & (ds == np.arange(n))).astype(np.int32)
    seq = O.idxs_seq(ds, pits)
    rnk = O.rank(ds)[0]
    P = _payloads(c, n)
    flw = _build(c, ds)
    eq = _Check(c)

    # graph exports (idxs_ds: the front end's mirror and the device's copy)
    eq("idxs_ds", flw.idxs_ds, ds)
    eq("device idxs_ds", flw._h.idxs_ds(np.int32), ds)
    eq("idxs_pit", flw.idxs_pit, pits)
    eq("idxs_seq", flw.idxs_seq, seq)
    eq("rank", flw.rank, rnk, shape)
    eq("n_upstream", flw.n_upstream, O.upstream_count(ds), shape)
    upa_o = O.accuflux(ds, seq, np.ones(n, np.int32), nodata=-9999)
    upa_o[~valid] = -9999
    eq("upstream_area", flw.upstream_area(), upa_o, shape)

    # accuflux
    first = _accuflux_checks(O, eq, flw, ds, seq, P, shape)
    eq("accuflux i32 up", flw.accuflux(P["wi32"].reshape(shape)), O.accuflux(ds, seq, P["wi32"]), shape)
    eq("accuflux i64 nodata -3", flw.accuflux(P["wi64"].reshape(shape), nodata=-3),
       O.accuflux(ds, seq, P["wi64"], nodata=-3), shape)

    # stream orders and the main upstream cell
    mask2 = P["mask"].reshape(shape)
    strord = flw.stream_order()
    eq("strahler", strord, O.strahler_order(ds, seq), shape)
    eq("strahler mask", flw.stream_order(mask=mask2), O.strahler_order(ds, seq, P["mask"]), shape)
    main = O.main_upstream(ds, upa_o)
    eq("idxs_us_main", flw.idxs_us_main, main)
    eq("main_upstream ties", flw.main_upstream(uparea=P["ties"].reshape(shape)), O.main_upstream(ds, P["ties"]))
    eq("classic", flw.stream_order(type="classic"), O.stream_order_classic(ds, seq, main), shape)
    eq("classic mask", flw.stream_order(type="classic", mask=mask2), O.stream_order_classic(ds, seq, main, P["mask"]), shape)

    # basins, hand, stream distance in cells
    bas_o = O.basins(ds, pits, seq)
    eq("basins", flw.basins(), bas_o, shape)
    eq("basins idxs ids", flw.basins(idxs=P["oidx"], ids=P["oids"]), O.basins(ds, P["oidx"].astype(np.int32), seq, P["oids"]),
       shape)
    _hand_checks(O, eq, flw, ds, seq, P, shape)
    eq("stream_distance", flw.stream_distance(unit="cell"), O.stream_distance(ds, seq, shape[1], real_length=False), shape)
    eq("stream_distance mask", flw.stream_distance(mask=mask2, unit="cell"),
       O.stream_distance(ds, seq, shape[1], mask=P["mask"], real_length=False), shape)

    # fillnodata and the outlets against the serial loops
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for key, nd in (("f32", -9999.0), ("i32", 0)):
            eq.bytes(f"fillnodata up {key}", flw.fillnodata(P[key].reshape(shape), nd, direction="up"),
                     _ref_up(ds, seq, P[key], nd), shape)
            for how in ("max", "min", "sum"):
                eq.bytes(f"fillnodata down {how} {key}", flw.fillnodata(P[key].reshape(shape), nd, direction="down", how=how),
                         _ref_down(ds, seq, P[key], nd, how), shape)
    dsl, sql = ds.tolist(), seq.tolist()
    for m in (-2, 2):
        sub_o, idxs_o = _ref_streamorder(dsl, sql, strord.ravel().tolist(), m)
        sub, idxs = flw.subbasins_streamorder(strord=strord, min_sto=m)
        eq(f"subbasins_streamorder {m} map", sub, np.array(sub_o, np.int32), shape)
        eq(f"subbasins_streamorder {m} outlets", idxs, np.array(idxs_o, np.int32))
    blob = OC.region(shape, "blob")
    eq("outflow_idxs", flw.outflow_idxs(blob), np.array(_ref_outflow(dsl, sql, blob.ravel().tolist()), np.int32))

    def outlets_of(labels, sq):
        lbs, idxs = _ref_outlets(dsl, sq, labels.tolist())
        order = np.argsort(np.array(lbs, labels.dtype), kind="stable")
        return np.array(lbs, labels.dtype)[order], np.array(idxs, np.int32)[order]

    lbs, idxs = flw.basin_outlets(flw.basins())
    lbs_o, idxs_o = outlets_of(bas_o, sql)
    eq("basin_outlets labels", lbs, lbs_o)
    eq("basin_outlets outlets", idxs, idxs_o)

    # ---- 1. an installed sort order: the CSR lists the upstream cells by position, children combine in descending
    # position, and the expected values are the oracle's / the serial loops' over that sequence
    sseq = _sorted_seq(O, ds)
    flw.order_cells("sort")
    eq.stage = "sorted: "
    eq("idxs_seq", flw.idxs_seq, sseq)
    eq("device idxs_seq", flw._h.idxs_seq(np.int32), sseq)
    _accuflux_checks(O, eq, flw, ds, sseq, P, shape, both_f64=True)
    _hand_checks(O, eq, flw, ds, sseq, P, shape)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eq.bytes("fillnodata down sum f32", flw.fillnodata(P["f32"].reshape(shape), -9999.0, direction="down", how="sum"),
                 _ref_down(ds, sseq, P["f32"], -9999.0, "sum"), shape)
    eq("basins", flw.basins(), O.basins(ds, pits, sseq), shape)
    # (the upstream lists are no longer in ascending index: the smallest index among equal areas has to be looked for)
    eq("main_upstream ties", flw.main_upstream(uparea=P["ties"].reshape(shape)), O.main_upstream(ds, P["ties"]))
    eq("n_upstream", flw.n_upstream, O.upstream_count(ds), shape)
    flw.order_cells("walk")
    eq.stage = "walk again: "
    eq("idxs_seq", flw.idxs_seq, seq)
    eq("accuflux f32 up", flw.accuflux(P["w32"].reshape(shape)), first.ravel(), shape)

    # ---- 2. add_pits while the sort order is installed
    flw.order_cells("sort")
    rng = np.random.default_rng(9000 + c["seed"])
    inner = np.flatnonzero(rnk > 0)
    pick = (rng.choice(inner, size=min(3, inner.size), replace=False) if inner.size else pits[:3]).astype(np.int32)
    flw.add_pits(idxs=pick)
    ds2 = ds.copy()
    ds2[pick] = pick
    pits2 = np.flatnonzero(valid & (ds2 == np.arange(n))).astype(np.int32)
    seq2 = _sorted_seq(O, ds2) if flw.ftype == "nextxy" else O.idxs_seq(ds2, pits2)  # (NEXTXY rasters are re-sorted)
    eq.stage = "add_pits: "
    eq("idxs_ds", flw.idxs_ds, ds2)
    eq("device idxs_ds", flw._h.idxs_ds(np.int32), ds2)
    eq("idxs_pit", flw.idxs_pit, pits2)
    eq("device idxs_pit", flw._h.idxs_pit(np.int32), pits2)
    eq("idxs_seq", flw.idxs_seq, seq2)
    eq("rank", flw.rank, O.rank(ds2)[0], shape)
    upa2 = O.accuflux(ds2, seq2, np.ones(n, np.int32), nodata=-9999)
    upa2[~valid] = -9999
    eq("upstream_area", flw.upstream_area(), upa2, shape)
    eq("accuflux f32 up", flw.accuflux(P["w32"].reshape(shape)), O.accuflux(ds2, seq2, P["w32"]), shape)
    eq("basins", flw.basins(), O.basins(ds2, pits2, seq2), shape)


DTYPE_CASES = [c for c in GG.CASES if c["shape"] == (300, 211) and c["family"] in ("star", "recursive")]


@pytest.mark.parametrize("c", DTYPE_CASES, ids=[GG.case_id(c) for c in DTYPE_CASES])
def test_index_dtypes(gpu_lib, oracle, c):
    """int32, uint32 and int64 ``idxs_ds`` into pfd_raster_create_general (k_gen_import's three forms): every export comes
    back in the dtype asked for, with that dtype's missing value, and the graph behind it is the same."""
    from pyflwdir_amd import _hip

    shape = c["shape"]
    ref = GG.build(c, np.int32)
    pits = np.flatnonzero(ref == np.arange(ref.size)).astype(np.int32)
    seq = oracle.idxs_seq(ref, pits)
    upa_o = oracle.accuflux(ref, seq, np.ones(ref.size, np.int32), nodata=-9999)
    upa_o[ref == -1] = -9999
    eq = _Check(c)
    for dt_in in (np.int32, np.uint32, np.int64):
        ds = GG.build(c, dt_in)
        h = _hip.RasterHandle.general(ds, shape[0], shape[1])
        eq.stage = f"{np.dtype(dt_in).name} in: "
        eq("idxs_ds round trip", h.idxs_ds(dt_in), ds)
        for dt_out in (np.int32, np.uint32, np.int64):
            eq(f"idxs_ds as {np.dtype(dt_out).name}", h.idxs_ds(dt_out), GG.build(c, dt_out))
            eq(f"idxs_pit as {np.dtype(dt_out).name}", h.idxs_pit(dt_out), pits.astype(dt_out))
            eq(f"idxs_seq as {np.dtype(dt_out).name}", h.idxs_seq(dt_out), seq.astype(dt_out))
        eq("upstream_area_cell", h.upstream_area_cell(), upa_o)
        h.close()


NEXTXY_CASES = [c for c in GG.CASES if c["shape"] in ((16, 16), (300, 211)) and c["family"] in ("pref", "star")]


@pytest.mark.parametrize("c", NEXTXY_CASES, ids=[GG.case_id(c) for c in NEXTXY_CASES])
def test_nextxy_form(gpu_lib, oracle, c):
    """The same far-link graph as a NEXTXY raster (one-based next x / next y, pyflwdir_amd/nextxy.py's pit and nodata
    codes, one CaMa-style inland pit): from_array decodes it to the same ``idxs_ds``, installs the sort order like the
    reference's constructor, gives the float32 accuflux of that order, and ``to_array("nextxy")`` writes the river-mouth
    code on every pit."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import nextxy

    O = oracle
    shape = c["shape"]
    nrow, ncol = shape
    ds = GG.build(c)
    n = ds.size
    valid = ds != -1
    pit = valid & (ds == np.arange(n))
    nx = np.full(n, nextxy.MV, np.int32)
    ny = np.full(n, nextxy.MV, np.int32)
    link = valid & ~pit
    nx[link] = ds[link] % ncol + 1
    ny[link] = ds[link] // ncol + 1
    nx[pit] = ny[pit] = nextxy.PV[0]
    canonical = np.stack([nx.reshape(shape), ny.reshape(shape)])
    inland = int(np.flatnonzero(pit)[-1])
    nx[inland] = ny[inland] = nextxy.PV[1]
    data = np.stack([nx.reshape(shape), ny.reshape(shape)])
    assert nextxy.isvalid(data)
    flw = pyflwdir.from_array(data, ftype="nextxy", cache=False)
    eq = _Check(c, "nextxy: ")
    assert flw._d8 is None and flw.ftype == "nextxy"
    eq("idxs_ds", flw.idxs_ds, ds)
    eq("device idxs_ds", flw._h.idxs_ds(np.int32), ds)
    sseq = _sorted_seq(O, ds)
    eq("device idxs_seq", flw._h.idxs_seq(np.int32), sseq)  # (installed by the constructor, before any property asks)
    eq("idxs_seq", flw.idxs_seq, sseq)
    P = _payloads(c, n)
    eq("accuflux f32 up", flw.accuflux(P["w32"].reshape(shape)), O.accuflux(ds, sseq, P["w32"]), shape)
    # (to_array writes -9 on every pit, core_nextxy.to_array: the input but for the inland pit's code)
    eq("to_array", flw.to_array("nextxy"), canonical)
    back = flw.to_array("nextxy")
    back[:, inland // ncol, inland % ncol] = nextxy.PV[1]
    eq("to_array with the inland pit", back, data)


def test_refusals(gpu_lib):
    """What pfd_raster_create_general refuses, through the C-ABI: nothing beyond construction runs on the device."""
    from pyflwdir_amd import _hip

    c = next(c for c in GG.CASES if c["shape"] == (16, 16) and c["family"] == "recursive")
    ds = GG.build(c)
    n = ds.size
    nonpit = np.flatnonzero((ds != -1) & (ds != np.arange(n)))
    bad = ds.copy()
    bad[nonpit[0]] = n  # the first index past the raster
    with pytest.raises(ValueError, match="invalid idxs_ds"):
        _hip.RasterHandle.general(bad, 16, 16)
    bad = GG.build(c, np.int64)
    bad[nonpit[1]] = 1 << 40
    with pytest.raises(ValueError, match="invalid idxs_ds"):
        _hip.RasterHandle.general(bad, 16, 16)
    bad = ds.copy()
    if not (ds == -1).any():
        bad[np.flatnonzero(np.bincount(ds[nonpit], minlength=n) == 0)[0]] = -1  # (a headwater becomes nodata)
    bad[nonpit[-1] if bad[nonpit[-1]] != -1 else nonpit[-2]] = np.flatnonzero(bad == -1)[0]
    with pytest.raises(ValueError, match="invalid idxs_ds"):
        _hip.RasterHandle.general(bad, 16, 16)
    ring = np.roll(np.arange(n, dtype=np.int32), -7)  # one pure cycle over all cells (7 and 256 are coprime)
    with pytest.raises(ValueError, match="no pits found"):
        _hip.RasterHandle.general(ring, 16, 16)
    h = _hip.RasterHandle.general(ds, 16, 16)  # (the library is still usable)
    assert np.array_equal(h.idxs_ds(np.int32), ds)
    h.close()


def test_invalid_dtype_codes(gpu_lib):
    """A payload or index dtype code outside the C-ABI's set is PFD_EUNSUPPORTED (NotImplementedError) on every entry
    point alike, general graphs and D8 rasters; the handle stays usable."""
    import ctypes as C

    from pyflwdir_amd import _hip

    c = next(c for c in GG.CASES if c["shape"] == (16, 16) and c["family"] == "recursive")
    ds = GG.build(c)
    n = ds.size
    d8 = np.full((16, 16), 4, np.uint8)  # every cell drains south; the last row leaves the raster: pits
    w = np.ones(n, np.float32)
    for h in (_hip.RasterHandle.general(ds, 16, 16), _hip.RasterHandle(d8, 16, 16)):
        with pytest.raises(NotImplementedError, match="unsupported payload dtype code 99"):
            h.accuflux(w, 99, has_nodata=0)
        with pytest.raises(NotImplementedError, match="unsupported payload dtype code 99"):
            h.main_upstream(w, 99, np.int32)
        out = np.empty(n, np.int64)
        with pytest.raises(NotImplementedError, match="unsupported index dtype code 99"):
            _hip.check(_hip.lib().pfd_main_upstream(h._h, _hip.PFD_F32, _hip.ptr(w), C.c_double(0.0), 99, _hip.ptr(out),
                                                    _hip.PFD_HOST))
        # the handle is still usable
        upa = h.accuflux(w, _hip.PFD_F32, has_nodata=0)
        assert upa.min() == 1.0 and upa.sum() >= n
        main = h.main_upstream(upa, _hip.PFD_F32, np.int32)
        assert main.shape == (n,) and (main >= -1).all() and (main < n).all()
        h.close()
