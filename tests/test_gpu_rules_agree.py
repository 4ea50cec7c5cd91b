"""Three engines, one answer, bit for bit: the exact-order engine, the level engine (PFD_EXACT_LEVELS=1) and the
general idxs_ds engine compute their cells through the same per-cell rules (csrc/rules.h).  Every operation below runs
on a handle of each engine, built from the same golden D8 raster, and the results are compared with tobytes() — which
tells -0.0 from 0.0 where == would not.  Where the golden manifest holds the result of an operation, the default
handle's answer is checked against it too: three engines agreeing on a wrong answer do not pass."""
import ctypes as C

import numpy as np
import pytest

from golden_util import Case, derived_inputs
from oracle import golden_inputs as GI

pytestmark = pytest.mark.gpu

# smaller than a tile / the quad and row-edge forms / 6 x 8 tiles with nodata and many short chains / cycles
ACYCLIC = ["synth_tiny_5x7", "synth_onerow_1x300", "synth_rough_nodata_384x512"]
CYCLIC = ["synth_loops_96x80"]


def _operations(case, a):
    """(name, call on a handle, golden key or None), inputs shared by the engines; `a`: the default handle."""
    from pyflwdir_amd import _hip

    n, shape = case.n, case.shape
    rng = np.random.default_rng(20240611)
    P = GI.payloads(shape)
    upa = a.upstream_area_cell()
    D = derived_inputs(case, upa.reshape(shape), a.idxs_pit(np.int32))
    u8 = lambda m: np.ascontiguousarray(np.asarray(m).ravel() != 0).view(np.uint8)  # noqa: E731

    w32 = rng.random(n, dtype=np.float32)
    w32[rng.random(n) < 0.05] = -1.0  # the nodata value, present in the payload
    wi32 = rng.integers(-50, 1000, n).astype(np.int32)
    wi32[rng.random(n) < 0.05] = -9999
    mask = u8(rng.random(n) < 0.6)
    drain = u8(rng.random(n) < 0.1)
    elev = np.ascontiguousarray(D["elevtn"].ravel(), dtype=np.float32)
    main = a.main_upstream(upa, _hip.PFD_I32, np.int32)
    valid = np.flatnonzero(upa != -9999)
    outlets = rng.choice(valid, size=min(5, valid.size), replace=False).astype(np.int64)
    ids = (np.arange(outlets.size, dtype=np.uint32) * 11 + 5).astype(np.uint32)
    gf32, gi32 = np.ascontiguousarray(P["wf32_nodata_m1"].ravel()), np.ascontiguousarray(P["wi32_nodata"].ravel())

    def acc(data, code, nodata, direction):
        return lambda h: h.accuflux(data, code, nodata_i=int(nodata), nodata_f=float(nodata), has_nodata=1, direction=direction)

    return [
        ("accuflux float32 up, nodata in the payload", acc(w32, _hip.PFD_F32, -1, _hip.PFD_UP), None),
        ("accuflux float32 up, golden payload", acc(gf32, _hip.PFD_F32, -1, _hip.PFD_UP), "accuflux_f32_nodata_m1"),
        ("accuflux int32 down", acc(wi32, _hip.PFD_I32, -9999, _hip.PFD_DOWN), None),
        ("accuflux int32 down, golden payload", acc(gi32, _hip.PFD_I32, -9999, _hip.PFD_DOWN), "accuflux_ds_i32_nodata"),
        ("strahler, random mask", lambda h: h.strahler(mask), None),
        ("strahler, golden mask", lambda h: h.strahler(u8(D["mask_rand"])), "strahler_mask_rand"),
        ("hand float32, random drain mask", lambda h: h.hand(drain, elev, _hip.PFD_F32), None),
        ("hand float32, golden drain mask", lambda h: h.hand(u8(D["drain"]), elev, _hip.PFD_F32), "hand_f32"),
        ("stream_distance in cells, random mask", lambda h: h.stream_distance(mask), None),
        ("stream_distance in cells, golden mask", lambda h: h.stream_distance(u8(D["mask_upa"])), "strdist_cell_mask"),
        ("stream_order_classic", lambda h: h.stream_order_classic(main), "strord_classic"),
        ("basins, 5 seeded outlets, uint32 ids", lambda h: h.basins(outlets, ids), None),
    ]


def _xplan_state(h):
    """1: the handle sweeps on the exact-order plan (builds the plan if the handle has none yet)."""
    from pyflwdir_amd import _hip

    L = _hip.lib()
    L.pfd_debug_xplan.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    info = (C.c_int64 * 8)()
    _hip.check(L.pfd_debug_xplan(h._h, info, None))
    return int(info[0])


def _run(case, monkeypatch, cyclic):
    from pyflwdir_amd import _hip

    nrow, ncol = case.shape
    a = _hip.RasterHandle(case.d8, nrow, ncol)
    ops = _operations(case, a)
    engines = {}
    if cyclic:  # the exact engine stands down on a raster with cycles: said here, not skipped silently
        assert _xplan_state(a) != 1, "the default handle of a cyclic raster must not hold an exact plan"
        st = case.entry["stats"]
        assert st["n_loop_cells"] > 0
    else:
        assert _xplan_state(a) == 1, "the default handle does not run the exact-order engine"
        engines["exact"] = a
    monkeypatch.setenv("PFD_EXACT_LEVELS", "1")
    monkeypatch.setenv("PFD_BASINS_LEVELS", "1")  # (basins: the level engine's label sweep, not the tiled path query)
    b = _hip.RasterHandle(case.d8, nrow, ncol)
    assert _xplan_state(b) != 1, "PFD_EXACT_LEVELS=1 did not select the level engine"
    engines["levels"] = b
    engines["general"] = _hip.RasterHandle.general(a.idxs_ds(np.int32), nrow, ncol)
    results = {e: [np.ascontiguousarray(f(h)) for _, f, _ in ops] for e, h in engines.items()}
    monkeypatch.delenv("PFD_EXACT_LEVELS")
    monkeypatch.delenv("PFD_BASINS_LEVELS")
    if cyclic:
        info = b.info()
        assert info["n_seq"] < info["n_valid"], "info(): a raster with cycles has cells outside the sequence"
    first = "levels" if cyclic else "exact"
    for i, (name, _, key) in enumerate(ops):
        ref = results[first][i]
        for e in engines:
            got = results[e][i]
            assert got.dtype == ref.dtype and got.shape == ref.shape, f"{case.name}: {name}: {e} vs {first}: dtype / shape"
            if got.tobytes() != ref.tobytes():
                bad = np.flatnonzero(got.view(np.uint8).reshape(got.size, -1) != ref.view(np.uint8).reshape(ref.size, -1))
                raise AssertionError(f"{case.name}: {name}: {e} differs from {first} in {bad.size} byte(s), first cell "
                                     f"{bad[0] // got.itemsize}: {got[bad[0] // got.itemsize]!r} vs {ref[bad[0] // got.itemsize]!r}")
        if key is not None and key in case.digests:
            case.check(key, ref.reshape(case.shape))
    for h in engines.values():
        h.close()
    if cyclic:
        a.close()


@pytest.mark.parametrize("name", ACYCLIC)
def test_three_engines_agree(gpu_lib, manifest, monkeypatch, name):
    _run(Case(name, manifest), monkeypatch, cyclic=False)


@pytest.mark.parametrize("name", CYCLIC)
def test_level_and_general_agree_on_cycles(gpu_lib, manifest, monkeypatch, name):
    _run(Case(name, manifest), monkeypatch, cyclic=True)
