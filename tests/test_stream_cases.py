"""Stream segments without a GPU: the restatement of the reference's serial loop (tests/stream_cases._ref_streams) gives
the recorded bytes of streams.streams on every case of tests/golden/wide_streams.npz (tools/gen_golden_streams.py), the
cases reach the corners of the closed form (csrc/streams.hip), and the host code that turns flow paths into geo-features
(pyflwdir_amd.gis.features, FlwdirRaster.geofeatures) gives the features the reference recorded."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as SC  # noqa: E402
from golden_util import GOLD, digest  # noqa: E402


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLD, "wide_streams.npz"))


@pytest.fixture(scope="module")
def graphs(oracle):
    """raster -> (idxs_ds, idxs_seq, Strahler order, shape), computed once."""
    return {name: SC.inputs(name, oracle) for name in SC.RASTERS + SC.GENERAL}


@pytest.fixture(scope="module")
def segments(graphs):
    """(raster, mask kind, max_len) -> the serial loop's list, computed once and shared by the tests."""
    out = {}
    for name, (ds, seq, strahler, shape) in graphs.items():
        for _, mkind, max_len in SC.cases(name):
            out[name, mkind, max_len] = SC._ref_streams(ds, seq, SC.mask_of(mkind, strahler, shape), max_len)
    return out


def test_golden_file_is_complete(G):
    assert os.path.getsize(os.path.join(GOLD, "wide_streams.npz")) < 1 << 20
    for name in SC.RASTERS + SC.GENERAL:
        for k, _, _ in SC.cases(name):
            assert f"count_{k}" in G.files
            want = (f"lens_{k}", f"idxs_{k}") if name in SC.FULL else (f"digest_lens_{k}", f"digest_idxs_{k}")
            assert all(w in G.files for w in want), k


def test_ref_streams_gives_golden(G, graphs, segments):
    n = 0
    for name, (ds, _, _, _) in graphs.items():
        for k, mkind, max_len in SC.cases(name):
            segs = segments[name, mkind, max_len]
            lens, flat = SC.flatten(segs, ds.dtype)
            assert len(segs) == int(G[f"count_{k}"]), k
            if name in SC.FULL:
                want_l, want_i = G[f"lens_{k}"], G[f"idxs_{k}"]
                assert lens.tobytes() == want_l.tobytes() and flat.dtype == want_i.dtype, k
                assert flat.tobytes() == want_i.tobytes(), k
            else:
                assert digest(lens) == str(G[f"digest_lens_{k}"]) and digest(flat) == str(G[f"digest_idxs_{k}"]), k
            n += 1
    assert n == 12 * len(SC.MASKS) * len(SC.MAX_LEN)


def test_cases_reach_the_corners(graphs, segments):
    """Each corner of the closed form occurs in the inputs at least once."""
    outside = twice = half = single = 0
    for name, (ds, seq, strahler, shape) in graphs.items():
        for mkind in SC.MASKS:
            mask = SC.mask_of(mkind, strahler, shape)
            whole = segments[name, mkind, 0]
            if mask is not None:  # a walk steps from a cell outside the mask (any element but a segment's last)
                outside += sum(1 for s in whole if not mask[s[:-1]].all())
            pits = [s[0] for s in whole if len(s) == 2 and s[0] == s[1]]
            twice += len(pits) != len(set(pits))
            lens = [len(s) for s in whole if not (len(s) == 2 and s[0] == s[1])]
            half += sum(1 for l in lens for ml in SC.MAX_LEN if ml and l / ml > 1.5 and (l / ml) % 1 == 0.5)
            single += sum(1 for ml in SC.MAX_LEN if ml for s in segments[name, mkind, ml] if len(s) == 1 and ml > 1)
    assert outside > 0 and twice > 0 and half > 0 and single > 0, (outside, twice, half, single)
    ds, seq, _, _ = graphs["synth_loops_96x80"]
    assert 0 < seq.size < np.count_nonzero(ds != -1)  # cells on or above a cycle are not in the sequence
    # the one-cell-wide strips hold segments long enough for max_len = 7 to cut them into several pieces
    for name in SC.STRIPS:
        assert max(len(s) for s in segments[name, "none", 0]) / 7 > 1.5
        assert len(segments[name, "none", 7]) > len(segments[name, "none", 0])


def _recorded(G, name, tag, columns):
    return {col: G[f"feat_{name}_{tag}_{col}"] for col in ("coords", "npts", "idx", "idx_ds", "pit") + tuple(columns)}


def _same_features(feats, want, columns):
    got = SC.feature_record(feats, columns)
    assert all(sorted(f) == ["geometry", "properties", "type"] and f["type"] == "Feature"
               and f["geometry"]["type"] == "LineString" for f in feats)
    for col, arr in want.items():
        assert got[col].shape == arr.shape and got[col].dtype == arr.dtype, col
        assert got[col].tobytes() == arr.tobytes(), col


def test_features_of_recorded_flow_paths(G, graphs):
    """gis.features and FlwdirRaster.geofeatures (host code) on the recorded segment lists / the flow direction pairs."""
    from pyflwdir_amd import gis
    from pyflwdir_amd.raster import FlwdirRaster

    for name in SC.FEATURE_RASTERS:
        ds, seq, strahler, shape = graphs[name]
        upa = np.ones(ds.size, np.int32)  # upstream cell count, -9999 on nodata (the reference's upstream_area)
        for x in seq[::-1].tolist():
            if ds[x] != x:
                upa[ds[x]] += upa[x]
        upa[ds == -1] = -9999
        paths = SC.unflatten(G[f"lens_{SC.key(name, 'sto2', 0)}"], G[f"idxs_{SC.key(name, 'sto2', 0)}"])
        kw = dict(strord=strahler.reshape(shape), uparea=upa.reshape(shape))
        feats = gis.features(paths, transform=gis.Affine(*SC.TRANSFORM), shape=shape, **kw)
        assert len(feats) == sum(1 for p in paths if len(p) > 1) > 0
        _same_features(feats, _recorded(G, name, "streams_sto2", ("strord", "uparea")), ("strord", "uparea"))
        keep = np.flatnonzero(ds != -1).astype(ds.dtype)
        pairs = list(np.stack([keep, ds[keep]], axis=1))
        flw = object.__new__(FlwdirRaster)  # (geofeatures reads the shape and the transform only: no device needed)
        flw.shape, flw.size = tuple(shape), ds.size
        flw.set_transform(SC.TRANSFORM)
        _same_features(flw.geofeatures(pairs), _recorded(G, name, "vectorize", ()), ())
        # coordinates sampled from xs / ys maps are the cell centres again
        xs, ys = gis.idxs_to_coords(np.arange(ds.size), flw.transform, shape)
        _same_features(flw.geofeatures(pairs, xs=xs.reshape(shape), ys=ys.reshape(shape)), _recorded(G, name, "vectorize", ()), ())


def test_features_errors():
    from pyflwdir_amd import gis

    paths = [np.array([0, 1]), np.array([3])]
    with pytest.raises(ValueError, match="transform and shape should be provided if xs and ys are None"):
        gis.features(paths)
    with pytest.raises(ValueError, match='Kwargs map "a" should be ndarrays of same size as coordinates'):
        gis.features(paths, transform=gis.IDENTITY, shape=(2, 2), a=np.ones(3))
    with pytest.raises(ValueError, match='Kwargs map "a" should be ndarrays of same size as coordinates'):
        gis.features(paths, transform=gis.IDENTITY, shape=(2, 2), a=[1, 2, 3, 4])
    feats = gis.features(paths, transform=gis.IDENTITY, shape=(2, 2), a=np.arange(4.0))
    assert len(feats) == 1 and feats[0]["properties"] == {"idx": 0, "idx_ds": 1, "pit": False, "a": 0.0}
    assert feats[0]["geometry"]["coordinates"] == [(0.5, -0.5), (1.5, -0.5)]
    assert gis.features([np.array([2])], transform=gis.IDENTITY, shape=(2, 2)) == []
    with pytest.raises(IndexError):
        gis.features([np.array([0, 4])], transform=gis.IDENTITY, shape=(2, 2))


def test_front_end_signatures_and_binding():
    import inspect
    import re

    from pyflwdir_amd import _hip
    from pyflwdir_amd.raster import FlwdirRaster

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pfd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pfd_streams\s*\(", header) and "pfd_streams" in _hip.SYMBOLS
    assert "#define PFD_ABI_VERSION 1" in header
    sig = inspect.signature(FlwdirRaster.streams)
    assert list(sig.parameters) == ["self", "mask", "min_sto", "xs", "ys", "idxs_out", "max_len", "direction", "kwargs"]
    assert [sig.parameters[p].default for p in ("mask", "min_sto", "idxs_out", "max_len", "direction")] == [None, 1, None, 0, "up"]
    sig = inspect.signature(FlwdirRaster.vectorize)
    assert list(sig.parameters) == ["self", "mask", "xs", "ys", "direction", "kwargs"] and sig.parameters["direction"].default == "down"
    assert list(inspect.signature(FlwdirRaster.geofeatures).parameters) == ["self", "flowpaths", "xs", "ys", "kwargs"]
    sig = inspect.signature(FlwdirRaster.stream_segments)
    assert [(p, sig.parameters[p].default) for p in list(sig.parameters)[1:]] == [("mask", None), ("max_len", 0), ("as_list", True)]
