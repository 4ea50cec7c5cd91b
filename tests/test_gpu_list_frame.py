"""What the shared frame of the walk and list calls (csrc/walks.h, csrc/lists.h) decides for every call that stands on it,
pinned at the C-ABI, where no front end looks at the input first: the error word (an index outside the raster, and the
handle's next call), the import rule of idxs_us_main per call, the step cap of the walks and the tail of the calls that
return ragged lists (pfd_path, pfd_streams).

The rasters are tests/golden/flwdir1.npz (15 x 10, with its recorded idxs_ds, idxs_us_main, upstream cells and distances
as inputs), synth_loops_96x80.npz for cycles and, for the two recorded ragged lists, flwdir0 (paths: wide_window.npz) and
flwdir1 (segments: wide_streams.npz).  A valid call is held against the restated serial loops of tests/*_cases.py, which
the CPU tests pin to the records — the records themselves hold none of these calls on flwdir1."""
from __future__ import annotations

import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as SC  # noqa: E402
import subbasins_area_cases as SA  # noqa: E402
import subgrid_riv_cases as RC  # noqa: E402
import upscale_cases as UC  # noqa: E402
import window_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1  # PFD_EINVAL


def _same(a, b):
    a, b = RC.canon(a), RC.canon(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def status(fn):
    """(C status, pfd_last_error() of a failure, result) of a call through a RasterHandle method."""
    from pyflwdir_amd import _hip

    seen, orig = [], _hip.check

    def spy(rc):
        seen.append(int(rc))
        orig(rc)

    _hip.check = spy
    try:
        try:
            return 0, "", fn()
        except (ValueError, NotImplementedError, RuntimeError, MemoryError) as e:
            return seen[-1], str(e), None
    finally:
        _hip.check = orig


class Raster:
    """A golden raster with its recorded graph, on a handle of its own."""

    def __init__(self, name):
        from pyflwdir_amd import _hip

        z = np.load(os.path.join(GOLD, name + ".npz"))
        self.d8 = np.ascontiguousarray(z["d8"])
        self.shape, self.n = self.d8.shape, self.d8.size
        self.ds = z["out_idxs_ds_int32"]
        self.seq = z["out_idxs_seq_int32"]
        self.us = np.ascontiguousarray(z["out_idxs_us_main"])
        self.upa = np.ascontiguousarray(z["out_uparea_cell"].ravel())
        self.distnc = np.ascontiguousarray(z["out_strdist_cell"].ravel())
        self.pits = z["out_idxs_pit_int32"]
        self.h = _hip.RasterHandle(self.d8, self.shape[0], self.shape[1])


@pytest.fixture(scope="module")
def F1(gpu_lib):
    r = Raster("flwdir1")
    assert r.shape == (15, 10) and r.us.dtype == np.int32 and r.distnc.dtype == np.int32 and r.upa.dtype == np.int32
    yield r
    r.h.close()


@pytest.fixture(scope="module")
def LOOPS(gpu_lib):
    r = Raster("synth_loops_96x80")
    yield r
    r.h.close()


def _outlets(r):
    """Some valid cells as an outlet list, with one missing value."""
    out = np.flatnonzero(r.ds >= 0)[::9].astype(np.int64)
    out[2] = -1
    return out


def _coarse(r):
    """A coarse network of flwdir1 (dmm, cellsize 3) as pfd_upscale_error takes it: (idxs_out, idxs_ds), int32."""
    ds1, out = r.h.upscale("dmm", 3, r.upa, None, np.int32)
    return out, ds1


def _calls(r):
    """name -> (call(lists) -> result, the index lists the call takes, expected(result) -> bool).  Each list maps to
    (its valid value, the first value outside its range)."""
    from pyflwdir_amd import _hip
    from pyflwdir_amd.raster import _area_min_compare

    inp = WC.inputs(r.n)
    data = inp["data32"]
    outlets = _outlets(r)
    starts = np.flatnonzero(r.ds >= 0)[::7].astype(np.int64)
    gw = WC.Graph(r.ds, r.us, -1, r.shape)
    gr = RC.Graph(r.ds, r.us, r.seq, -1, r.shape)
    us64 = r.us.astype(np.int64)
    am, form = _area_min_compare(r.upa.dtype, SA.threshold(r.upa, "mid"))
    c_out, c_ds = _coarse(r)

    def path_ok(res):
        cells, offsets, dists = res
        want, wdist = WC.path(gw, starts, "up")
        wc, wl = WC.flat_paths(want, np.int32)
        return _same(cells, wc) and _same(np.diff(offsets), wl) and _same(dists, wdist)

    def sa_ok(res):
        sub, idxs, _ = res
        wsub, widxs = SA.ref_serial(r.ds, r.seq, r.us, r.upa, SA.threshold(r.upa, "mid"))
        return _same(sub, wsub) and idxs.tolist() == list(widxs)

    return {
        "segment_length": (
            lambda L: r.h.segment_length(L["idxs_out"], _hip.PFD_UP, L["idxs_us_main"], None, r.distnc),
            {"idxs_out": (outlets, r.n), "idxs_us_main": (r.us, r.n)},
            lambda res: _same(res, RC.segment_length(gr, outlets, "up", r.distnc))),
        "segment_average": (
            lambda L: r.h.segment_average(L["idxs_out"], _hip.PFD_UP, L["idxs_us_main"], None, data),
            {"idxs_out": (outlets, r.n), "idxs_us_main": (r.us, r.n)},
            lambda res: _same(res, RC.segment_average(gr, outlets, "up", data))),
        "moving_average": (
            lambda L: r.h.moving_average(3, L["idxs_us_main"], data),
            {"idxs_us_main": (r.us, r.n)},
            lambda res: _same(res, WC.moving_average(gw, data, 3))),
        "path": (
            lambda L: r.h.path(L["idxs"], _hip.PFD_UP, np.int32, idxs_us_main=L["idxs_us_main"]),
            {"idxs": (starts, r.n), "idxs_us_main": (r.us, r.n)},
            path_ok),
        "subbasins_area": (
            lambda L: r.h.subbasins_area(r.upa, _hip.PFD_I32, am, form, L["idxs_us_main"], np.int32),
            {"idxs_us_main": (us64, r.n)},
            sa_ok),
        "upscale_error": (
            lambda L: r.h.upscale_error(L["idxs_out"], L["idxs_ds_coarse"]),
            {"idxs_out": (c_out, r.n), "idxs_ds_coarse": (c_ds, c_out.size)},
            lambda res: _same(res, UC.upscale_error(r.ds, c_out, c_ds, -1))),
    }


CALLS = ["segment_length", "segment_average", "moving_average", "path", "subbasins_area", "upscale_error"]


# ---- the error word --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CALLS)
def test_index_outside_the_raster(F1, name):
    """An entry outside its range in any index list of a call: PFD_EINVAL, "outside the raster" under the call's name —
    and the handle serves the next, valid call."""
    call, lists, expected = _calls(F1)[name]
    good = {k: v for k, (v, _) in lists.items()}
    for key, (valid, limit) in lists.items():
        bad = valid.copy()
        at = int(np.flatnonzero(bad >= 0)[1])
        bad[at] = limit
        rc, msg, _ = status(lambda: call(dict(good, **{key: bad})))
        print(name, key, rc, msg)
        assert rc == EINVAL and "outside the raster" in msg and name in msg, (name, key, rc, msg)
        rc, msg, res = status(lambda: call(good))
        assert rc == 0 and expected(res), (name, key, rc, msg)


# ---- the import rule of idxs_us_main, per call -----------------------------------------------------------------------
def _wrong_entry(r):
    """(p, other): p has a main upstream cell; other is a headwater that does not drain into p — followed upstream it ends
    at once, so a call that takes the entry ends too."""
    p = int(np.flatnonzero(r.us >= 0)[0])
    heads = np.flatnonzero((r.ds >= 0) & (r.us < 0) & (r.ds != p) & (np.arange(r.n) != p))
    return p, int(heads[0])


def test_entry_that_does_not_drain_into_its_cell(F1):
    """segment_* and path(up) follow idxs_us_main as it is given; the windows and subbasins_area refuse an entry that is
    no upstream cell of its cell."""
    from pyflwdir_amd import _hip

    r = F1
    p, other = _wrong_entry(r)
    bad, data = r.us.copy(), WC.inputs(r.n)["data32"]
    bad[p] = other
    outlets, starts = _outlets(r), np.flatnonzero(r.ds >= 0)[::7].astype(np.int64)
    accepted = {
        "segment_length": lambda: r.h.segment_length(outlets, _hip.PFD_UP, bad, None, r.distnc),
        "segment_average": lambda: r.h.segment_average(outlets, _hip.PFD_UP, bad, None, data),
        "segment_median": lambda: r.h.segment_median(outlets, _hip.PFD_UP, bad, None, data),
        "path": lambda: r.h.path(starts, _hip.PFD_UP, np.int32, idxs_us_main=bad),
    }
    for name, fn in accepted.items():
        rc, msg, _ = status(fn)
        print(name, rc, msg)
        assert rc == 0, (name, rc, msg)
    am = float(SA.threshold(r.upa, "mid"))
    refused = {
        "moving_average": lambda: r.h.moving_average(3, bad, data),
        "moving_median": lambda: r.h.moving_median(3, bad, data),
        "subbasins_area": lambda: r.h.subbasins_area(r.upa, _hip.PFD_I32, am, _hip.PFD_COMPARE_F64, bad.astype(np.int64), np.int32),
    }
    for name, fn in refused.items():
        rc, msg, _ = status(fn)
        print(name, rc, msg)
        assert rc == EINVAL and "does not drain" in msg and name in msg, (name, rc, msg)


def test_pit_listed_as_its_own_main_upstream_cell(F1):
    """subbasins_area wants ANOTHER cell; the windows only ask for down(entry) == cell, which a pit meets for itself.  Their
    walk (win_visit, csrc/window.hip) then steps n times up onto the pit and n times back down onto it: it ends, the window
    of the pit holds the pit 2n + 1 times and the call returns PFD_OK — the status observed before the calls shared their
    import kernel, recorded here as the literal 0."""
    from pyflwdir_amd import _hip

    r = F1
    pit = int(r.pits[0])
    bad, data = r.us.copy(), WC.inputs(r.n)["data32"]
    bad[pit] = pit
    am = float(SA.threshold(r.upa, "mid"))
    rc, msg, _ = status(lambda: r.h.subbasins_area(r.upa, _hip.PFD_I32, am, _hip.PFD_COMPARE_F64, bad.astype(np.int64), np.int32))
    print("subbasins_area", rc, msg)
    assert rc == EINVAL and "does not drain" in msg
    for name, fn in (("moving_average", lambda: r.h.moving_average(3, bad, data)),
                     ("moving_median", lambda: r.h.moving_median(3, bad, data))):
        rc, msg, res = status(fn)
        print(name, rc, msg)
        assert rc == 0 and msg == "", (name, rc, msg)
        # away from the pit's windows nothing changes (cells whose window of 3 steps down does not reach the pit)
        good = r.h.moving_average(3, r.us, data) if name == "moving_average" else r.h.moving_median(3, r.us, data)
        x = np.arange(r.n)
        far = np.ones(r.n, bool)
        for _ in range(4):
            far &= x != pit
            x = np.where(r.ds >= 0, r.ds[np.maximum(x, 0)], x)
        assert far.any() and _same(res[far], good[far])


# ---- the step cap ----------------------------------------------------------------------------------------------------
def _cycle_cells(r):
    """(a cell on a cycle, a cell that drains into a cycle without being on one)"""
    ds = np.where(r.ds >= 0, r.ds, np.arange(r.n)).astype(np.int64)
    far = ds.copy()
    for _ in range(int(r.n).bit_length() + 1):
        far = far[far]  # ds ** (2 ** k): beyond n steps every walk sits in its pit or on its cycle
    lost = (r.ds >= 0) & (ds[far] != far)
    on = np.zeros(r.n, bool)
    on[far[lost]] = True
    x = far[lost]
    for _ in range(r.n):  # (the cycles of this raster are a few cells long)
        x = ds[x]
        if on[x].all():
            break
        on[x] = True
    return int(np.flatnonzero(on)[0]), int(np.flatnonzero(lost & ~on)[0])


def test_walks_end_within_n_steps(LOOPS):
    """No mask, no max length, a start that never reaches a pit: the walks stop after n = 7680 steps and the calls say so.
    pfd_path starts ON a cycle.  pfd_segment_length starts on a cell that drains INTO one: its walk stops where it steps
    onto an outlet cell, and a start on the cycle itself is such a cell after one turn (that call returns PFD_OK)."""
    from pyflwdir_amd import _hip

    r = LOOPS
    assert r.n == 7680
    on, above = _cycle_cells(r)
    zeros = np.zeros(r.n, np.int32)
    rc, msg, _ = status(lambda: r.h.segment_length(np.array([above], np.int64), _hip.PFD_DOWN, None, None, zeros))
    print("segment_length", rc, msg)
    assert rc == EINVAL and "did not end within" in msg and "segment_length" in msg
    rc, msg, res = status(lambda: r.h.segment_length(np.array([on], np.int64), _hip.PFD_DOWN, None, None, zeros))
    print("segment_length, on the cycle", rc, msg)
    assert rc == 0 and res.tolist() == [0]
    for start in (on, above):
        rc, msg, _ = status(lambda: r.h.path(np.array([start], np.int64), _hip.PFD_DOWN, np.int32))
        print("path", start, rc, msg)
        assert rc == EINVAL and "did not end within" in msg and "path" in msg


# ---- the ragged tail -------------------------------------------------------------------------------------------------
class Lists:
    """The three output lists of a ragged call, in host or device memory, pre-filled with sentinels."""

    def __init__(self, space, idx_dtype, m, k, side_dtype):
        from pyflwdir_amd import _hip

        self.space, self._hip = space, _hip
        self.fill = [np.full(max(m, 1), -7, idx_dtype), np.full(k + 1, -7, np.int64), np.full(max(k, 1), 9, side_dtype)]
        if space == _hip.PFD_DEVICE:
            self.bufs = [_hip.DeviceBuffer(a.nbytes).upload(a) for a in self.fill]
        else:
            self.bufs = [a.copy() for a in self.fill]

    def ptrs(self):
        return [self._hip.ptr(b) for b in self.bufs]

    def get(self):
        if self.space == self._hip.PFD_DEVICE:
            return [b.download(a.dtype, a.shape) for a, b in zip(self.fill, self.bufs)]
        return self.bufs

    def untouched(self):
        return all(_same(a, b) for a, b in zip(self.fill, self.get()))

    def free(self):
        if self.space == self._hip.PFD_DEVICE:
            for b in self.bufs:
                b.free()


def _c_path(r, starts, idx_dtype, lists, cap):
    """pfd_path, direction down, cell units: (status, total)."""
    from pyflwdir_amd import _hip

    starts = np.ascontiguousarray(starts, dtype=np.int64)
    m = C.c_int64(-1)
    cells, offsets, dists = lists.ptrs() if lists else (None, None, None)
    rc = _hip.lib().pfd_path(r.h._h, _hip.ptr(starts), C.c_int64(starts.size), _hip.PFD_DOWN, _hip.IDX_CODE[np.dtype(idx_dtype)],
                             None, None, None, 0, C.c_double(0.0), cells, C.c_int64(cap), offsets, dists, C.byref(m),
                             lists.space if lists else _hip.PFD_HOST)
    return rc, int(m.value)


def _c_streams(r, mask, idx_dtype, lists, cap_idxs, cap_segs):
    """pfd_streams: (status, segments, cells); ``mask`` uint8 on the host or None."""
    from pyflwdir_amd import _hip

    space = lists.space if lists else _hip.PFD_HOST
    n_out = (C.c_int64 * 2)(-1, -1)
    dmask = mask
    if mask is not None and space == _hip.PFD_DEVICE:
        dmask = _hip.DeviceBuffer(mask.nbytes).upload(mask)
    idxs, offsets, pit = lists.ptrs() if lists else (None, None, None)
    try:
        rc = _hip.lib().pfd_streams(r.h._h, _hip.ptr(dmask), _hip.IDX_CODE[np.dtype(idx_dtype)], idxs, C.c_int64(cap_idxs), offsets,
                                    pit, C.c_int64(cap_segs), n_out, space)
    finally:
        if dmask is not mask:
            dmask.free()
    return rc, int(n_out[0]), int(n_out[1])


@pytest.fixture(scope="module")
def F0(gpu_lib):
    from pyflwdir_amd import _hip

    d8 = np.ascontiguousarray(np.load(os.path.join(GOLD, "flwdir0.npz"))["d8"])
    r = types.SimpleNamespace(h=_hip.RasterHandle(d8, d8.shape[0], d8.shape[1]))
    yield r
    r.h.close()


def _spaces():
    from pyflwdir_amd import _hip

    return {"host": _hip.PFD_HOST, "device": _hip.PFD_DEVICE}


@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
def test_path_tail(F0, idx_dtype, space):
    """pfd_path on flwdir0, the recorded start cells, direction down in cell units (wide_window.npz, "down"): no start cell,
    room for one cell less than the paths hold, room for exactly the paths.  (tests/test_gpu_window.py runs the sizing call
    and the exact fetch of the "up_m_max_mask" case of flwdir_large in device memory; the cases here are not among its.)"""
    space = _spaces()[space]
    G = np.load(os.path.join(GOLD, WC.RECORD))
    starts = G["starts_flwdir0"]
    want = G["out_flwdir0_ll_path_down_cells"]
    k, M = starts.size, want.size
    # no start cell: the offsets are the single 0
    L = Lists(space, idx_dtype, 4, 0, np.float64)
    try:
        rc, m = _c_path(F0, starts[:0], idx_dtype, L, 4)
        cells, offsets, dists = L.get()
        assert (rc, m) == (0, 0) and offsets.tolist() == [0] and (cells == -7).all() and (dists == 9).all()
    finally:
        L.free()
    rc, m = _c_path(F0, starts, idx_dtype, None, 0)  # (a sizing call: no lists)
    assert (rc, m) == (0, M)
    for cap in (M - 1, M):
        L = Lists(space, idx_dtype, M, k, np.float64)
        try:
            rc, m = _c_path(F0, starts, idx_dtype, L, cap)
            assert (rc, m) == (0, M)
            if cap < M:
                assert L.untouched()
                continue
            cells, offsets, dists = L.get()
            assert cells.dtype == np.dtype(idx_dtype) and np.array_equal(cells, want)
            assert offsets[0] == 0 and np.array_equal(np.diff(offsets), G["out_flwdir0_ll_path_down_lens"])
            assert _same(dists, G["out_flwdir0_ll_path_down_dists"])
        finally:
            L.free()


@pytest.mark.parametrize("idx_dtype,space", [(np.int32, "host"), (np.int64, "host"), (np.int64, "device")])
def test_streams_tail(F1, idx_dtype, space):
    """pfd_streams on flwdir1 without a mask (wide_streams.npz, "flwdir1_none_0"): a mask without a cell, room for one cell
    / one segment less than there are, room for exactly the lists.  (tests/test_gpu_streams.py::test_streams_cabi_device_memory
    has the short and the exact room for int32 indices in device memory on synth_river_256: that combination is left to it.)"""
    space = _spaces()[space]
    G = np.load(os.path.join(GOLD, "wide_streams.npz"))
    # no segment: the offsets are the single 0
    L = Lists(space, idx_dtype, 4, 0, np.uint8)
    try:
        rc, K, M = _c_streams(F1, np.zeros(F1.n, np.uint8), idx_dtype, L, 4, 0)
        idxs, offsets, pit = L.get()
        assert (rc, K, M) == (0, 0, 0) and offsets.tolist() == [0] and (idxs == -7).all() and (pit == 9).all()
    finally:
        L.free()
    rc, K, M = _c_streams(F1, None, idx_dtype, None, 0, 0)  # (a sizing call: no lists)
    assert rc == 0 and K > 1 and M > K
    for cap_idxs, cap_segs in ((M - 1, K), (M, K - 1), (M, K)):
        L = Lists(space, idx_dtype, M, K, np.uint8)
        try:
            assert _c_streams(F1, None, idx_dtype, L, cap_idxs, cap_segs) == (0, K, M)
            if (cap_idxs, cap_segs) != (M, K):
                assert L.untouched()
                continue
            idxs, offsets, pit = L.get()
            assert idxs.dtype == np.dtype(idx_dtype) and offsets[0] == 0 and offsets[-1] == M
            # the record holds the front end's list: a [p, p] entry follows a segment that ends in a pit
            segs = []
            for j in range(K):
                seg = idxs[offsets[j]:offsets[j + 1]]
                segs.append(seg)
                if pit[j]:
                    segs.append(np.array([seg[-1], seg[-1]], idxs.dtype))
            lens, flat = SC.flatten(segs, idxs.dtype)
            key = SC.key("flwdir1", "none", 0)
            assert int(G[f"count_{key}"]) == len(segs) and np.array_equal(lens, G[f"lens_{key}"])
            assert np.array_equal(flat, G[f"idxs_{key}"])
        finally:
            L.free()
