"""FlwdirRaster.subbasins_streamorder / outflow_idxs / basin_outlets (reference pyflwdir/pyflwdir.py:601-629, :820-835,
:720-740; basins.py:67-103, core.py:501-514, regions.py:129-163) on the device: bytes against the reference's recorded
outputs (tests/golden/wide_outlets.npz, tools/gen_golden_outlets.py) through every engine, against a restatement of the
three serial loops on larger rasters, over the 64-bit sequence / in row blocks, identities that need no golden, and the
C-ABI with device memory."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlet_cases as OC  # noqa: E402
from golden_util import GOLD, digest  # noqa: E402
from serial_refs import _ref_outflow, _ref_outlets, _ref_streamorder  # noqa: E402  (the three serial loops)

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

    for name in OC.RASTERS:
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        yield name, pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
    W = np.load(os.path.join(GOLD, "wide_general.npz"))
    nxy = W["in_flwdir0_nextxy"]
    yield "flwdir0_nextxy", pyflwdir.from_array(nxy, ftype="nextxy", cache=False)
    yield "flwdir0_ds2", pyflwdir.FlwdirRaster(idxs_ds=W["in_flwdir0_ds2"], shape=nxy.shape[1:], ftype="d8", cache=False)


@pytest.mark.parametrize("engine", ENGINES)
def test_outlets_golden(gpu_lib, monkeypatch, engine):
    """Every recorded case (8 D8 rasters incl. one with cycles, a NEXTXY and a general graph; four min_sto values on the
    Strahler order and the classic order; two region masks; the outlets of basins() and of a sub-basin map): dtype,
    shape and bytes of every returned array."""
    _engine(monkeypatch, engine)
    G = np.load(os.path.join(GOLD, "wide_outlets.npz"))
    bad, n = [], 0
    for name, flw in _rasters():
        cache = {}
        for key, call, arg in OC.keys(name):
            outs = OC.run(flw, call, arg, cache)
            assert np.asarray(outs[-1]).size == int(G["count_" + key]), key
            for i, got in enumerate(outs):
                got = np.asarray(got)
                ok = _same(got, G[f"out_{key}_{i}"]) if name in OC.FULL else digest(got) == str(G[f"digest_{key}_{i}"])
                n += 1
                if not ok:
                    bad.append(f"{key}_{i}")
    assert n == 10 * (5 * 2 + 2 * 1 + 2 * 2) and not bad, bad[:20]


LARGE = [((1200, 1000), 3, dict(tilt=1 << 26, white=2, nodata_pct=10)),
         ((1024, 1024), 4, dict(tilt=3000, white=2, nodata_pct=25))]
_EXPECTED = {}  # seed -> the serial loops' results, shared by the engines


@pytest.mark.parametrize("engine", ENGINES)
def test_outlets_large_rasters(gpu_lib, oracle, monkeypatch, engine):
    """1-1.2 Mcell rasters spanning hundreds of 64 x 64 tiles (a river raster and a rough one, nodata in the flow
    directions) against the serial loops: integers, exact.  The label map handed to basin_outlets has regions with
    many outlets (8 x 8 blocks of labels): the order within a label (reversed sequence order) is part of the check."""
    import pyflwdir_amd as pyflwdir

    O = oracle
    _engine(monkeypatch, engine)
    for shape, seed, kw in LARGE:
        d8 = O.synth_d8(shape[0], shape[1], seed=seed, **kw)
        idxs_ds, idxs_pit, _ = O.from_array(d8)
        seq = O.idxs_seq(idxs_ds, idxs_pit)
        flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
        strord = flw.stream_order()
        blob = OC.region(shape, "blob")
        labels = OC.label_blocks(shape, seed)
        if seed not in _EXPECTED:
            ds, sq = idxs_ds.tolist(), seq.tolist()
            E = dict(out=np.array(_ref_outflow(ds, sq, blob.ravel().tolist()), idxs_ds.dtype))
            for m in (-2, 3):
                sub, idxs = _ref_streamorder(ds, sq, strord.ravel().tolist(), m)
                E["sto", m] = (np.array(sub, np.int32).reshape(shape), np.array(idxs, idxs_ds.dtype))
            lbs, idxs = _ref_outlets(ds, sq, labels.ravel().tolist())
            sort = np.argsort(np.array(lbs, labels.dtype), kind="stable")
            E["lab"] = (np.array(lbs, labels.dtype)[sort], np.array(idxs, idxs_ds.dtype)[sort])
            _EXPECTED[seed] = E
        E = _EXPECTED[seed]
        for m in (-2, 3):
            sub, idxs = flw.subbasins_streamorder(strord=strord, min_sto=m)
            assert _same(sub, E["sto", m][0]) and _same(idxs, E["sto", m][1]) and idxs.size > 10, (shape, m)
        assert _same(flw.outflow_idxs(blob), E["out"]) and E["out"].size > 100
        lbs, idxs = flw.basin_outlets(labels)
        assert _same(lbs, E["lab"][0]) and _same(idxs, E["lab"][1]) and np.unique(lbs).size < lbs.size


def test_outlets_wide_and_row_blocks(gpu_lib, oracle, monkeypatch):
    """The paths beyond 2**32 - 2 cells with the thresholds lowered: the front end's row blocks (PFD_TEST_BIG_CELLS: the
    Strahler order comes from 5 seeded blocks) and the library's 64-bit form (PFD_TEST_ORDER64: 64-bit sequence, 64-bit
    downstream links, the tiled label fill) give the single-handle bytes."""
    import pyflwdir_amd as pyflwdir

    shape = (1500, 1100)
    d8 = oracle.synth_d8(shape[0], shape[1], seed=61, tilt=100000, white=2, nodata_pct=15)
    region = OC.region(shape, "blob")

    def calls(flw):
        sub, idxs = flw.subbasins_streamorder(min_sto=3)
        sub2, idxs2 = flw.subbasins_streamorder()
        return [sub, idxs, sub2, idxs2, flw.outflow_idxs(region), *flw.basin_outlets(sub), *flw.basin_outlets(flw.basins())]

    whole = calls(pyflwdir.from_array(d8, ftype="d8", cache=False))
    assert whole[1].size > 100 and whole[4].size > 100
    monkeypatch.setenv("PFD_TEST_BIG_CELLS", "400000")
    blocked = pyflwdir.from_array(d8, ftype="d8", cache=False)
    assert blocked._row_blocks_needed() == 5
    for g, w in zip(calls(blocked), whole):
        assert _same(g, w)
    monkeypatch.setenv("PFD_TEST_ORDER64", "1")
    wide = pyflwdir.from_array(d8, ftype="d8", cache=False)
    assert wide._wide()
    for g, w in zip(calls(wide), whole):
        assert _same(g, w)


def test_outlets_identities(gpu_lib):
    """What must hold without any golden: the returned outlets, pushed through basins(), give the returned map; the
    outlets of basins() are the pits; every returned cell satisfies its mark rule."""
    import pyflwdir_amd as pyflwdir

    for name in ("rhine", "synth_loops_96x80", "synth_river_nodata_768x1024"):
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        flw = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
        ds, seq = flw.idxs_ds.astype(np.int64), flw.idxs_seq
        in_seq = np.zeros(flw.size, bool)
        in_seq[seq] = True
        strord = flw.stream_order().ravel()
        for min_sto in (-2, 2):
            sub, idxs = flw.subbasins_streamorder(strord=strord, min_sto=min_sto)
            k = idxs.size
            assert k > 0 and sub.dtype == np.int32 and idxs.dtype == flw.idxs_ds.dtype
            again = flw.basins(idxs=idxs, ids=np.arange(1, k + 1, dtype=np.int32))
            assert np.array_equal(again[sub != 0], sub[sub != 0]) and np.array_equal(again, sub)
            assert np.array_equal(sub.ravel()[idxs], np.arange(1, k + 1))
            m = int(strord.max()) + min_sto if min_sto < 0 else min_sto
            rule = (strord >= m) & ((ds == np.arange(flw.size)) | (strord[ds] != strord)) & in_seq
            assert np.array_equal(np.sort(idxs), np.flatnonzero(rule))
        lbs, outl = flw.basin_outlets(flw.basins())
        pits = flw.idxs_pit
        assert np.array_equal(np.sort(outl), pits[in_seq[pits]]) and np.array_equal(lbs, np.sort(lbs))
        assert lbs.dtype == np.uint32 and np.array_equal(flw.basins().ravel()[outl], lbs)
        region = OC.region(flw.shape, "blob").ravel()
        out = flw.outflow_idxs(region.reshape(flw.shape))
        cand = region & ((ds == np.arange(flw.size)) | ~region[ds]) & in_seq
        assert out.size and cand[out].all()
        pos = np.full(flw.size, -1, np.int64)
        pos[seq] = np.arange(seq.size)
        assert np.all(np.diff(pos[out]) > 0)  # (forward sequence order)
        # a candidate is returned iff no other candidate lies further down its flow path
        below = flw.basins(idxs=np.flatnonzero(cand), ids=np.ones(int(cand.sum()), np.uint8)).ravel()
        kept = cand & ((ds == np.arange(flw.size)) | (below[ds] == 0))
        assert np.array_equal(np.sort(out), np.flatnonzero(kept))


def test_outlets_errors_and_dtypes(gpu_lib):
    import pyflwdir_amd as pyflwdir

    d8 = np.load(os.path.join(GOLD, "flwdir0.npz"))["d8"]
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    with pytest.raises(ValueError, match='"strord" size does not match.'):
        flw.subbasins_streamorder(strord=np.ones(7, np.uint8))
    with pytest.raises(ValueError, match='"mask" size does not match.'):
        flw.subbasins_streamorder(mask=np.ones(7, bool))
    with pytest.raises(ValueError, match='"region" size does not match.'):
        flw.outflow_idxs(np.ones(7, bool))
    with pytest.raises(ValueError, match='"basins" size does not match.'):
        flw.basin_outlets(np.ones(7, np.int32))
    strord = flw.stream_order()
    with pytest.raises(NotImplementedError):
        flw.subbasins_streamorder(strord=strord.astype(np.float32))
    with pytest.raises(NotImplementedError):
        flw.basin_outlets(flw.basins().astype(np.float64))
    with pytest.raises(NotImplementedError):
        flw.outflow_idxs(np.ones(d8.shape, np.complex64))
    # an all-False mask changes nothing (the reference's `mask[idx0] is False` never holds); every integer dtype of the
    # stream order and of the labels gives the same outlets
    want = flw.subbasins_streamorder(strord=strord, min_sto=2)
    got = flw.subbasins_streamorder(strord=strord, mask=np.zeros(d8.shape, bool), min_sto=2)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and want[1].size
    for dt in (np.int8, np.int16, np.uint16, np.int32, np.uint32, np.int64):
        got = flw.subbasins_streamorder(strord=strord.astype(dt), min_sto=2)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), dt
    lbs, idxs = flw.basin_outlets(want[0])
    for dt in (np.int8, np.uint8, np.int16, np.uint32, np.int64, np.uint64):
        if want[0].max() > np.iinfo(dt).max:
            continue
        l2, i2 = flw.basin_outlets(want[0].astype(dt))
        assert l2.dtype == dt and np.array_equal(l2, lbs) and _same(i2, idxs), dt
    # a list longer than the first call's room: the binding repeats the call
    got = flw._h.subbasins_streamorder(strord.ravel(), pyflwdir._hip.PFD_U8, 1, np.int32, cap=3)
    assert _same(got[1], flw.subbasins_streamorder(strord=strord, min_sto=1)[1]) and got[1].size > 3


def test_outflow_and_basin_outlets_second_lap(gpu_lib):
    """Lists longer than the first call's room (cap=1 on the 5 x 7 raster: 4 outflow cells of the blob region, 4 basin
    outlets): the binding repeats the call with room for all, and gives the default capacity's arrays."""
    import pyflwdir_amd as pyflwdir

    _hip = pyflwdir._hip
    d8 = np.load(os.path.join(GOLD, "synth_tiny_5x7.npz"))["d8"]
    flw = pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
    blob = OC.region(d8.shape, "blob")
    want = flw.outflow_idxs(blob)
    got = flw._h.outflow_idxs(np.ascontiguousarray(blob).view(np.uint8), want.dtype, cap=1)
    assert want.size >= 2 and _same(got, want)
    basins = np.ascontiguousarray(flw.basins().astype(np.int32))
    lbs, idxs = flw.basin_outlets(basins)
    l2, i2 = flw._h.basin_outlets(basins, _hip.PFD_I32, idxs.dtype, cap=1)
    assert lbs.size >= 2 and _same(l2, lbs) and _same(i2, idxs)


def test_outlets_device_memory_and_transfers(gpu_lib):
    """pfd_subbasins_streamorder with stream order, map and list in device memory (PFD_DEVICE) gives the host call's
    bytes; a host call moves the stream order up and the map and the list down — never the sequence."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    d8 = np.load(os.path.join(GOLD, "synth_river_nodata_768x1024.npz"))["d8"]
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    strord = np.ascontiguousarray(flw.stream_order().ravel())
    _hip.transfer_stats(reset=True)
    sub, idxs = flw._h.subbasins_streamorder(strord, _hip.PFD_U8, 2, np.int32)
    t = _hip.transfer_stats(reset=True)
    assert t["h2d_bytes"] == strord.nbytes and t["d2h_bytes"] == sub.nbytes + idxs.nbytes and idxs.size
    region = np.ascontiguousarray(OC.region(d8.shape, "rect").ravel()).view(np.uint8)
    out = flw._h.outflow_idxs(region, np.int32)
    t = _hip.transfer_stats(reset=True)
    assert t["h2d_bytes"] == region.nbytes and t["d2h_bytes"] == out.nbytes and out.size
    din = _hip.DeviceBuffer(strord.nbytes).upload(strord)
    dmap, didx = _hip.DeviceBuffer(sub.nbytes), _hip.DeviceBuffer(4 * idxs.size)
    try:
        _, _, k = flw._h.subbasins_streamorder(din, _hip.PFD_U8, 2, np.int32, cap=idxs.size, out=dmap, idxs_out=didx,
                                               memspace=_hip.PFD_DEVICE)
        assert k == idxs.size
        assert _same(dmap.download(np.int32, sub.shape), sub) and _same(didx.download(np.int32, idxs.shape), idxs)
    finally:
        din.free(), dmap.free(), didx.free()
    with pytest.raises(NotImplementedError):  # a dtype code the entry point does not take
        flw._h.subbasins_streamorder(strord, _hip.PFD_F32, 2, np.int32)
