"""FlwdirRaster.stream_segments / streams / vectorize (reference pyflwdir/streams.py:132-188, pyflwdir.py:865-1009) on
the device: bytes against the reference's recorded outputs (tests/golden/wide_streams.npz, tools/gen_golden_streams.py)
through every engine, against the restatement of the serial loop on larger rasters, the recorded geo-features, identities
that need no golden, the C-ABI with device memory and the documented refusals."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlet_cases as OC  # noqa: E402
import stream_cases as SC  # noqa: E402
from golden_util import GOLD, digest  # noqa: E402
from test_gpu_outlets import ENGINES, _engine  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _raster(name, **kw):
    import pyflwdir_amd as pyflwdir

    if name in SC.GENERAL:
        W = np.load(os.path.join(GOLD, "wide_general.npz"))
        nxy = W["in_flwdir0_nextxy"]
        if name == "flwdir0_nextxy":
            return pyflwdir.from_array(nxy, ftype="nextxy", cache=False)
        return pyflwdir.FlwdirRaster(idxs_ds=W["in_flwdir0_ds2"], shape=nxy.shape[1:], ftype="d8", cache=False)
    d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
    return pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False, **kw)


@pytest.mark.parametrize("name", SC.RASTERS + SC.GENERAL)
@pytest.mark.parametrize("engine", ENGINES)
def test_stream_segments_golden(gpu_lib, monkeypatch, engine, name):
    """Every recorded case of one raster (four masks incl. one that is not closed downstream, five max_len): count,
    dtype, lengths and bytes of the returned list."""
    _engine(monkeypatch, engine)
    G = np.load(os.path.join(GOLD, "wide_streams.npz"))
    flw = _raster(name)
    strahler = flw.stream_order().ravel()
    bad = []
    for k, mkind, max_len in SC.cases(name):
        mask = SC.mask_of(mkind, strahler, flw.shape)
        segs = flw.stream_segments(mask=None if mask is None else mask.reshape(flw.shape), max_len=max_len)
        assert len(segs) == int(G[f"count_{k}"]), k
        assert all(s.dtype == flw.idxs_ds.dtype and s.ndim == 1 for s in segs[:50]), k
        lens, flat = SC.flatten(segs, flw.idxs_ds.dtype)
        if name in SC.FULL:
            ok = _same(lens, G[f"lens_{k}"]) and _same(flat, G[f"idxs_{k}"])
        else:
            ok = digest(lens) == str(G[f"digest_lens_{k}"]) and digest(flat) == str(G[f"digest_idxs_{k}"])
        if not ok:
            bad.append(k)
    assert not bad, bad


def _recorded(G, name, tag, columns):
    return {col: G[f"feat_{name}_{tag}_{col}"] for col in ("coords", "npts", "idx", "idx_ds", "pit") + tuple(columns)}


def _same_features(feats, want, columns):
    got = SC.feature_record(feats, columns)
    assert all(sorted(f) == ["geometry", "properties", "type"] and f["type"] == "Feature"
               and f["geometry"]["type"] == "LineString" for f in feats)
    for col, arr in want.items():
        assert _same(got[col], arr), col


@pytest.mark.parametrize("name", SC.FEATURE_RASTERS)
def test_streams_and_vectorize_features(gpu_lib, name):
    """streams(min_sto=2, strord=..., uparea=...) and vectorize() against the reference's recorded features: coordinates,
    idx, idx_ds, pit and the sampled columns; a missing strord is computed and added as a column."""
    G = np.load(os.path.join(GOLD, "wide_streams.npz"))
    flw = _raster(name, transform=SC.TRANSFORM)
    strord, uparea = flw.stream_order(), flw.upstream_area()
    want = _recorded(G, name, "streams_sto2", ("strord", "uparea"))
    _same_features(flw.streams(min_sto=2, strord=strord, uparea=uparea), want, ("strord", "uparea"))
    _same_features(flw.streams(min_sto=2, uparea=uparea), want, ("strord", "uparea"))
    _same_features(flw.streams(mask=strord >= 2, min_sto=5, strord=strord, uparea=uparea), want, ("strord", "uparea"))
    _same_features(flw.vectorize(), _recorded(G, name, "vectorize", ()), ())
    _same_features(flw.vectorize(mask=strord >= 2, direction="up", strord=strord),
                   _recorded(G, name, "vectorize_up", ("strord",)), ("strord",))
    # geofeatures on the segments themselves is what streams returns
    segs = flw.stream_segments(mask=strord >= 2)
    _same_features(flw.geofeatures(segs, strord=strord.ravel(), uparea=uparea.ravel()), want, ("strord", "uparea"))


LARGE = [((130, 70), 5, dict(tilt=3000, white=2, nodata_pct=10)),  # 3 x 2 tiles of 64 x 64, partial edge tiles
         ((1200, 1000), 3, dict(tilt=1 << 26, white=2, nodata_pct=10))]


@pytest.mark.parametrize("shape,seed,kw", LARGE, ids=["130x70", "1200x1000"])
def test_stream_segments_large_rasters(gpu_lib, oracle, shape, seed, kw):
    """Rasters of several / hundreds of tiles with nodata against the serial loop, exact: no mask, a threshold on the
    upstream area (closed downstream) and the blob mask (not closed: the W sweep runs)."""
    import pyflwdir_amd as pyflwdir

    O = oracle
    d8 = O.synth_d8(shape[0], shape[1], seed=seed, **kw)
    ds, pits, _ = O.from_array(d8)
    seq = O.idxs_seq(ds, pits)
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    upa = flw.upstream_area()
    small = shape[0] * shape[1] < 100000
    for mkind, mask in (("none", None), ("upa", upa >= (5 if small else 50)), ("blob", OC.region(shape, "blob"))):
        want = SC._ref_streams(ds, seq, None if mask is None else mask.ravel(), 0)
        whole = [s for s in want if not (len(s) == 2 and s[0] == s[1])]
        idxs, offsets, pit = flw.stream_segments(mask=mask, as_list=False)
        assert idxs.dtype == ds.dtype and offsets.dtype == np.int64 and pit.dtype == np.uint8
        lens, flat = SC.flatten(whole, ds.dtype)
        assert pit.size == len(whole) > 10 and np.array_equal(np.diff(offsets), lens) and offsets[0] == 0, mkind
        assert _same(idxs, flat), mkind
        assert int(pit.sum()) == len(want) - len(whole)
        for max_len in ((0, 1, 5) if small else (5,) if mkind == "upa" else ()):
            got = flw.stream_segments(mask=mask, max_len=max_len)
            want = SC._ref_streams(ds, seq, None if mask is None else mask.ravel(), max_len)
            gl, gf = SC.flatten(got, ds.dtype)
            wl, wf = SC.flatten(want, ds.dtype)
            assert _same(gl, wl) and _same(gf, wf), (mkind, max_len)


def test_stream_segments_one_long_chain(gpu_lib):
    """One segment of 5000 cells (a single row draining east into a pit): one thread walks the whole chain, and max_len
    cuts it into many pieces (k = 714 for max_len = 7), against the serial loop."""
    import pyflwdir_amd as pyflwdir

    d8 = np.full((1, 5000), 1, np.uint8)
    d8[0, -1] = 0
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    ds, seq = flw.idxs_ds, flw.idxs_seq
    assert np.array_equal(ds, np.minimum(np.arange(5000) + 1, 4999))
    idxs, offsets, pit = flw.stream_segments(as_list=False)
    assert np.array_equal(idxs, np.arange(5000)) and offsets.tolist() == [0, 5000] and pit.tolist() == [1]
    for max_len in (0, 2, 7, 64, 3000, 3334, 5000):
        got = flw.stream_segments(max_len=max_len)
        want = SC._ref_streams(ds, seq, None, max_len)
        assert len(got) == len(want) and all(g.tolist() == w for g, w in zip(got, want)), max_len
    assert len(flw.stream_segments(max_len=7)) == 714 + 1


def test_streams_cabi_device_memory(gpu_lib):
    """pfd_streams with the mask and the three lists in device memory: a sizing call (caps 0, NULL lists), then a
    fetch that gives the host call's bytes; caps one too small leave the lists unwritten and n_out correct."""
    from pyflwdir_amd import _hip

    flw = _raster("synth_river_256")
    mask = np.ascontiguousarray(OC.region(flw.shape, "blob").ravel()).view(np.uint8)
    idxs, offsets, pit = flw._h.streams(mask, np.int32)
    K, M = pit.size, idxs.size
    assert K > 10 and M > K and offsets[-1] == M
    dmask = _hip.DeviceBuffer(mask.nbytes).upload(mask)
    didx, doff, dpit = _hip.DeviceBuffer(4 * M), _hip.DeviceBuffer(8 * (K + 1)), _hip.DeviceBuffer(K)
    try:
        assert flw._h.streams(dmask, np.int32, memspace=_hip.PFD_DEVICE) == (K, M)
        assert flw._h.streams(dmask, np.int32, didx, doff, dpit, M, K, memspace=_hip.PFD_DEVICE) == (K, M)
        assert _same(didx.download(np.int32, (M,)), idxs) and _same(doff.download(np.int64, (K + 1,)), offsets)
        assert _same(dpit.download(np.uint8, (K,)), pit)
        for cap_idxs, cap_segs in ((M - 1, K), (M, K - 1)):
            didx.upload(np.full(M, -7, np.int32)), doff.upload(np.full(K + 1, -7, np.int64)), dpit.upload(np.full(K, 9, np.uint8))
            assert flw._h.streams(dmask, np.int32, didx, doff, dpit, cap_idxs, cap_segs, memspace=_hip.PFD_DEVICE) == (K, M)
            assert (didx.download(np.int32, (M,)) == -7).all() and (doff.download(np.int64, (K + 1,)) == -7).all()
            assert (dpit.download(np.uint8, (K,)) == 9).all()
        # int64 indices, no mask: the same cells as the front end's
        i64, o64, p64 = flw._h.streams(None, np.int64)
        i32, o32, p32 = flw.stream_segments(as_list=False)
        assert i64.dtype == np.int64 and np.array_equal(i64, i32) and _same(o64, o32) and _same(p64, p32)
    finally:
        dmask.free(), didx.free(), doff.free(), dpit.free()
    with pytest.raises(NotImplementedError):  # an index dtype code the entry point does not take
        _hip.check(gpu_lib.pfd_streams(flw._h._h, None, _hip.PFD_F32, None, 0, None, None, 0, (_hip.C.c_int64 * 2)(), 0))


@pytest.mark.parametrize("name", ["rhine", "synth_loops_96x80", "synth_river_nodata_768x1024", "flwdir0_ds2"])
def test_stream_segments_identities(gpu_lib, name):
    """What must hold without any golden for mask=None: every sequence cell is stepped from exactly once, and the starts
    are exactly the sequence cells whose upstream count is not 1."""
    flw = _raster(name)
    seq = flw.idxs_seq
    idxs, offsets, pit = flw.stream_segments(as_list=False)
    last = np.zeros(idxs.size, bool)
    last[offsets[1:][pit == 0] - 1] = True  # a segment's last cell is not stepped from — unless it is a pit
    stepped = idxs[~last]
    assert stepped.size == seq.size and np.array_equal(np.sort(stepped), np.sort(seq))
    nup = flw.n_upstream.ravel()
    in_seq = np.zeros(flw.size, bool)
    in_seq[seq] = True
    assert np.array_equal(np.sort(idxs[offsets[:-1]]), np.flatnonzero(in_seq & (nup != 1)))
    # reversed sequence order of the starts; every segment ends at a confluence or a pit
    pos = np.full(flw.size, -1, np.int64)
    pos[seq] = np.arange(seq.size)
    assert np.all(np.diff(pos[idxs[offsets[:-1]]]) < 0)
    ends = idxs[offsets[1:] - 1]
    ds = flw.idxs_ds
    assert np.all(ds[ends[pit == 1]] == ends[pit == 1]) and np.all(nup[ends[pit == 0]] > 1)


def test_streams_refusals(gpu_lib, oracle, monkeypatch):
    """idxs_out= is the subgrid family's; a row-block handle and a handle with 64-bit cell indices are refused with the
    documented errors; argument errors of the reference."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    d8 = np.load(os.path.join(GOLD, "flwdir0.npz"))["d8"]
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    with pytest.raises(NotImplementedError, match="idxs_out"):
        flw.streams(idxs_out=flw.idxs_pit)
    with pytest.raises(ValueError, match='"mask" size does not match.'):
        flw.streams(mask=np.ones(7, bool))
    with pytest.raises(ValueError, match='"strord" size does not match.'):
        flw.streams(min_sto=2, strord=np.ones(7, np.uint8))
    with pytest.raises(ValueError, match='Kwargs map "a" should be ndarrays of same size as coordinates'):
        flw.streams(a=np.ones(7))
    big = oracle.synth_d8(300, 200, seed=4, tilt=100000, white=2, nodata_pct=5).reshape(300, 200)
    h = _hip.RasterHandle(big[99:201], 100, 200, halo=(1, 1))
    with pytest.raises(NotImplementedError, match="streams is not available on a row-block handle"):
        h.streams(None, np.int32)
    h.close()
    monkeypatch.setenv("PFD_TEST_ORDER64", "1")
    wide = pyflwdir.from_array(d8, ftype="d8", cache=False)
    assert wide._wide()
    with pytest.raises(NotImplementedError, match=r"at most 4294967294 \(2\^32 - 2\) cells"):
        wide.stream_segments()
