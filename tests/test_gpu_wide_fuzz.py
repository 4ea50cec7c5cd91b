"""The fixed-point upstream area (csrc/wide.h, pfd_upstream_area_rows_fixed) on everything its 64-bit copy of the tiled
engine can get wrong, against the reference of tests/wide_cases.py: the exact sums of the quantised weights, accumulated
as two 32-bit halves and recombined as unbounded integers, so that a sum which reaches 2^64 shows instead of wrapping the
way the device would (tests/test_wide_cases.py pins that reference and the edges of the cases without a GPU).

* random acyclic rasters at every tile-edge shape, one row / one column, with and without an interior rectangle, two
  hypertiles, drain-all rasters where one cell holds the whole sum; eager and deferred handles; row values from lat/lon
  areas to equal rows, clamping fractions, 60 binary orders of dynamic range and totals near both ends of float64;
* the kernel forms (PFD_WIDE_UNFUSED: the separate local pass over every tile; PFD_TILE_GENERAL: no interior rectangle) and
  the forms and fall-backs of the exit graph (hypertile / flat level 3, overflow -> flat retry, short of rounds -> longer
  retry, a supertile beyond the LDS capacity -> not taken), and the production hypertile form at 65 hypertiles;
* the limits of the 64 bits: totals that round across a power of two (they wrapped before the scale kept a bit of headroom:
  the pit of ten rows of 0.1 x 64 columns came back as 3.6e-15 instead of 64), scales beyond float64, rows at and below
  the quantum;
* rasters with cycles are not taken; a device-resident result; what the call leaves on the handle for the next operation.

Nothing is compared with a second device run: every taken result is compared byte for byte with the reference, and with the
exact form within the bound wide.h states (upstream cells x quantum, plus the serial float64 sum's own rounding)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_cases as W  # noqa: E402

from pyflwdir_amd import gis  # noqa: E402
from pyflwdir_amd._affine import Affine  # noqa: E402

pytestmark = pytest.mark.gpu

ACYCLIC = W.acyclic_cases(gis.area_rows, Affine)
CYCLIC = W.cyclic_cases(gis.area_rows, Affine)
LIMITS = W.limit_cases()
BY_NAME = {c.name: c for c in ACYCLIC + CYCLIC + LIMITS}
_LATE = {}  # the cases that need the oracle's generator: built once


def exit_cases(O):
    if "exit" not in _LATE:
        _LATE["exit"] = {c.name: c for c in W.exit_graph_cases(O, gis.area_rows, Affine)}
    return _LATE["exit"]


EXIT_NAMES = [c.name for c in ACYCLIC if c.shape in W.EXIT_GRAPH_SHAPES and c.name.startswith("rand")] + \
    [f"synth_{W.SYNTH[0][0]}x{W.SYNTH[0][1]}"]


def handle(c, deferred=False):
    from pyflwdir_amd import _hip

    return _hip.RasterHandle(c.d8, c.shape[0], c.shape[1], deferred=deferred)


def exact_rows(h, rows):
    """The exact form on the same handle, as the front end calls it."""
    from pyflwdir_amd import _hip

    return h.accuflux_rows(rows, _hip.PFD_F64, nodata_i=-9999, nodata_f=-9999.0, has_nodata=1, direction=_hip.PFD_UP,
                           mask_invalid=1)


def check_taken(O, c, h, bound=True):
    """The call is taken, reports a power-of-two quantum — the one the host rule states — and returns the reference's bytes,
    twice; against the exact form: the bound of wide.h.  Returns the result."""
    out, quantum = h.upstream_area_rows_fixed(c.rows)
    assert out is not None, f"{c.name}: not taken"
    exp = c.expected(O, quantum)  # (a power-of-two quantum, and no sum of 2^64 or more, or this fails)
    nod = c.d8.ravel() == 247
    assert out.dtype == np.float64 and np.all(out[nod] == -9999.0)
    bad = np.flatnonzero(out != exp)
    assert out.tobytes() == exp.tobytes(), f"{c.name}: {bad.size} cells differ, first {bad[:4]}: {out[bad[:4]]} != {exp[bad[:4]]}"
    out2, quantum2 = h.upstream_area_rows_fixed(c.rows)
    assert quantum2 == quantum and out2.tobytes() == exp.tobytes(), f"{c.name}: the second call differs"
    s = W.quantum_exponent(quantum)
    assert s == W.scale_exponent(c.rows, c.shape[1]), f"{c.name}: quantum 2^{-s}, not the one the host rule states"
    if bound:
        exact = exact_rows(h, c.rows)
        nup = h.upstream_area_cell().astype(np.float64)
        v = ~nod
        assert np.all(exact[nod] == -9999.0) and np.all(nup[v] >= 1)
        lim = nup[v] * quantum + exact[v] * nup[v] * 2.0 ** -52
        assert np.all(np.abs(out[v] - exact[v]) <= lim), f"{c.name}: beyond upstream cells x quantum"
    return out


# ---- random parity, and the kernel forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
@pytest.mark.parametrize("name", [c.name for c in ACYCLIC])
def test_random_parity(gpu_lib, oracle, name, deferred):
    c = BY_NAME[name]
    h = handle(c, deferred)
    check_taken(oracle, c, h)
    h.close()


@pytest.mark.parametrize("knob", ["PFD_WIDE_UNFUSED", "PFD_TILE_GENERAL"])
@pytest.mark.parametrize("name", [c.name for c in ACYCLIC])
def test_kernel_forms(gpu_lib, oracle, monkeypatch, name, knob):
    """The separate local pass over every tile (k_wtile_local<false>) and the pass without an interior rectangle (every tile
    through the frame kernel): the same bytes as the default form, which are the reference's."""
    c = BY_NAME[name]
    monkeypatch.setenv(knob, "1")
    for deferred in (False, True):
        h = handle(c, deferred)
        h.set_profiling(True)
        check_taken(oracle, c, h, bound=False)
        names = [s["name"] for s in h.last_timing()]
        assert "wide_tile_local" in names and "wide_tile_final" in names, names
        if knob == "PFD_TILE_GENERAL":  # (no interior kernel, so no segment of its own for the frame)
            assert "tile_local_frame" not in names, names
        h.close()


def test_the_default_form_runs_the_fused_interior(gpu_lib, oracle):
    """With an interior rectangle the count pass's own local kernel produces the interior tiles' sums (a segment of its own
    in the timing), without one the frame kernel takes every tile."""
    for name, interior in (("rand9_200x511_range2", True), ("rand8_130x67_range1", False)):
        c = BY_NAME[name]
        assert W.has_interior(c.shape) == interior
        h = handle(c)
        h.set_profiling(True)
        assert h.upstream_area_rows_fixed(c.rows)[0] is not None
        names = [s["name"] for s in h.last_timing()]
        assert ("tile_local_frame" in names) == interior, names
        h.close()


# ---- the forms and fall-backs of the exit graph ----------------------------------------------------------------------------------
FORMS = {"hyper_small": dict(PFD_HYPER_SMALL="1"), "flat_l3": dict(PFD_FLAT_L3="1"),
         "hcap_overflow": dict(PFD_HYPER_SMALL="1", PFD_TEST_HCAP=str(W.HCAP_LOWERED)),
         "rounds4": dict(PFD_TEST_ROUNDS4="1"), "rounds4_hyper": dict(PFD_TEST_ROUNDS4="1", PFD_HYPER_SMALL="1")}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", EXIT_NAMES)
def test_exit_graph_forms(gpu_lib, oracle, monkeypatch, name, form):
    """Hypertile solves where production would take the flat forest, the flat level 3, a hypertile overflowing its (lowered)
    id range -> the flat retry, too few level-4 / flat-forest rounds -> the longer retry: all taken, all the reference."""
    c = exit_cases(oracle)[name]
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    # the fall-back fires where it must: a retry shows as a second structure pass in the call's timing.  Every hypertile of
    # these rasters holds more super-exits than the lowered capacity (tests/test_wide_cases.py); one round is too few for the
    # rivers of the synthetic raster (the random rasters' paths are short: one round saturates them, nothing to retry)
    retry = (form == "hcap_overflow" and W.n_hypertiles(c.shape) > 1) or (form.startswith("rounds4") and name.startswith("synth"))
    for deferred in (False, True):
        h = handle(c, deferred)
        h.set_profiling(True)
        check_taken(oracle, c, h, bound=False)
        names = [s["name"] for s in h.last_timing()]
        if retry or not form.startswith("rounds4"):
            assert names.count("exit_graph") == (2 if retry else 1), names
        h.close()


@pytest.mark.parametrize("name", EXIT_NAMES)
def test_supertile_beyond_capacity_is_not_taken(gpu_lib, oracle, monkeypatch, name):
    """PFD_TEST_SCAP=0: every supertile takes the positional kernel, which has no 64-bit form — not taken, and the front end
    answers with the exact form byte for byte."""
    import pyflwdir_amd as pyflwdir

    c = exit_cases(oracle)[name]
    h = handle(c)
    check_taken(oracle, c, h, bound=False)  # (taken without the knob)
    monkeypatch.setenv("PFD_TEST_SCAP", "0")
    assert h.upstream_area_rows_fixed(c.rows)[0] is None
    h.close()
    hd = handle(c, deferred=True)
    assert hd.upstream_area_rows_fixed(c.rows)[0] is None
    hd.close()
    res = 1.0 / 1200.0
    flw = pyflwdir.from_array(c.d8, ftype="d8", transform=Affine(res, 0.0, 5.0, 0.0, -res, 52.0), latlon=True, cache=False)
    got = flw.upstream_area("km2", exact=False)
    assert got.tobytes() == flw.upstream_area("km2", exact=True).tobytes()
    idxs_ds, seq = c.graph(oracle)
    rows = np.ascontiguousarray(gis.area_rows(flw.transform, flw.shape, True, unit="m2") / gis.AREA_FACTORS["km2"])
    exp = oracle.accuflux(idxs_ds, seq, np.repeat(rows, c.shape[1]), nodata=-9999.0)
    exp[c.d8.ravel() == 247] = -9999.0
    assert got.ravel().tobytes() == exp.tobytes()


def test_production_hypertile_form(gpu_lib, oracle, monkeypatch):
    """65 x 1 hypertiles, no knob: above 64 production keeps the per-hypertile level 3 (sa.hmode, n3 = nht * HCAP ids in the
    64-bit exit graph).  The 64-bit loop issues the same launches in either form, so the form is read off the structure
    pass before it: lists + records, 2 supertile solves up, link + hypertile solve, level 4 (link, its round budget, one
    check, push), hypertile solve down, 2 supertile solves down."""
    c = W.long_case(gis.area_rows, Affine)
    assert W.n_hypertiles(c.shape) > 64
    h = handle(c)
    h.set_profiling(True)
    check_taken(oracle, c, h, bound=False)
    segs = {s["name"]: s["launches"] for s in h.last_timing()}
    assert "wide_exit_graph" in segs and "exit_graph" in segs, segs
    ntr, ntc = -(-c.shape[0] // W.TS), -(-c.shape[1] // W.TS)
    budget = 5 + sum(1 for k in range(32) if (1 << k) < (ntr + ntc) // 32 + 2)
    assert segs["exit_graph"] == 12 + budget, segs
    h.close()
    monkeypatch.setenv("PFD_FLAT_L3", "1")  # the flat loop on the same raster: other launches, the same bytes
    h = handle(c)
    h.set_profiling(True)
    check_taken(oracle, c, h, bound=False)
    flat = {s["name"]: s["launches"] for s in h.last_timing()}
    assert flat["exit_graph"] != segs["exit_graph"], (flat, segs)
    h.close()


# ---- the limits of the 64 bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in LIMITS if c.taken])
def test_limits_taken(gpu_lib, oracle, name):
    """Totals that round across a power of two, rows 1 / 2 / 3 / 2^20 quanta, totals near 1e295, rows of 1e-280 and the
    largest finite scale: taken and exact; the pit of the drain-all raster holds the whole raster's sum."""
    c = BY_NAME[name]
    for deferred in (False, True):
        h = handle(c, deferred)
        out = check_taken(oracle, c, h)
        h.close()
        pit = int(np.flatnonzero(np.isin(c.d8.ravel(), [0, 255]))[0])
        s = W.scale_exponent(c.rows, c.shape[1])
        total = W.quantised_total(c.rows, c.shape[1], s)
        assert total < 1 << 64 and out[pit] == float(total) * math.ldexp(1.0, -s), (name, out[pit])
        real = float(sum(W.Fraction(v) for v in c.rows.tolist()) * c.shape[1])
        assert abs(out[pit] - real) <= c.n * math.ldexp(1.0, -s) + real * 2.0 ** -52, (name, out[pit], real)


@pytest.mark.parametrize("name", [c.name for c in LIMITS if not c.taken])
def test_limits_refused(gpu_lib, oracle, name):
    """A scale beyond float64 (totals below 2^-960) and a row below the quantum: not taken, before any conversion to an
    integer; the exact form on the same handle — what the front end then runs — is the serial float64 sum."""
    c = BY_NAME[name]
    idxs_ds, seq = c.graph(oracle)
    exp = oracle.accuflux(idxs_ds, seq, np.repeat(c.rows, c.shape[1]), nodata=-9999.0)
    for deferred in (False, True):
        h = handle(c, deferred)
        out, quantum = h.upstream_area_rows_fixed(c.rows)
        assert out is None and quantum == 0.0, name
        assert exact_rows(h, c.rows).tobytes() == exp.tobytes()
        h.close()


# ---- cycles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in CYCLIC])
def test_cycles_are_not_taken(gpu_lib, oracle, name):
    import pyflwdir_amd as pyflwdir

    c = BY_NAME[name]
    assert W.scale_exponent(c.rows, c.shape[1]) is not None  # (the row values are not the reason)
    for deferred in (False, True):
        h = handle(c, deferred)
        assert h.upstream_area_rows_fixed(c.rows)[0] is None, name
        assert h.upstream_area_rows_fixed(c.rows)[0] is None, name
        h.close()
    if min(c.shape) > 1 and c.name.startswith("cyclic"):  # the front end: lat/lon areas, the rows of the case
        flw = pyflwdir.from_array(c.d8, ftype="d8", transform=Affine(1 / 1200.0, 0.0, 5.0, 0.0, -1 / 1200.0, 0.5 * c.shape[0] / 1200.0),
                                  latlon=True, cache=False)
        rows = np.ascontiguousarray(gis.area_rows(flw.transform, flw.shape, True, unit="m2") / gis.AREA_FACTORS["km2"])
        assert np.array_equal(rows, c.rows)
        got = flw.upstream_area("km2", exact=False)
        assert got.dtype == np.float64 and got.tobytes() == flw.upstream_area("km2", exact=True).tobytes()


# ---- device memory, handle state ---------------------------------------------------------------------------------------------------
def test_device_resident_result(gpu_lib, oracle):
    from pyflwdir_amd import _hip

    for name in ("rand9_200x511_range2", "rand4_63x65_pole"):
        c = BY_NAME[name]
        h = handle(c)
        buf = _hip.DeviceBuffer(c.n * 8 + 64)
        buf.upload(np.full(c.n + 8, 7.5, np.float64))
        out, quantum = h.upstream_area_rows_fixed(c.rows, out=buf, memspace=_hip.PFD_DEVICE)
        assert out is buf and quantum > 0.0
        got = buf.download(np.float64, (c.n + 8,))
        assert got[: c.n].tobytes() == c.expected(oracle, quantum).tobytes()
        assert np.all(got[c.n:] == 7.5)  # (nothing past the raster)
        buf.free()
        h.close()


def _ops(O, c):
    idxs_ds, seq = c.graph(O)
    idxs_pit = O.from_array(c.d8)[1]
    w = O.synth_weights_f32(c.n, seed=3)
    upa = O.accuflux(idxs_ds, seq, np.ones(c.n, np.int32), nodata=-9999)
    upa[idxs_ds == -1] = -9999
    return {"cell": (lambda flw: flw.upstream_area().ravel(), upa),
            "accuflux_f32": (lambda flw: flw.accuflux(w.reshape(c.shape)).ravel(), O.accuflux(idxs_ds, seq, w)),
            "basins": (lambda flw: flw.basins().ravel(), O.basins(idxs_ds, idxs_pit, seq)),
            "stream_order": (lambda flw: flw.stream_order().ravel(), O.strahler_order(idxs_ds, seq))}


@pytest.mark.parametrize("op", ["cell", "accuflux_f32", "basins", "stream_order"])
@pytest.mark.parametrize("name", ["rand9_200x511_range2", "rand23_513x520_range2", "rand12_2100x200_e-280"])
def test_handle_state(gpu_lib, oracle, name, op):
    """The call leaves the handle as the next operation expects it (acyclic known, the control words, the buffers of the
    tiled run), and finds it so after another operation: both orders on one handle."""
    import pyflwdir_amd as pyflwdir

    c = BY_NAME[name]
    run, exp = _ops(oracle, c)[op]
    for wide_first in (True, False):
        flw = pyflwdir.from_array(c.d8, ftype="d8", cache=False)
        for step in range(4):
            if (step % 2 == 0) == wide_first:
                out, quantum = flw._h.upstream_area_rows_fixed(c.rows)
                assert out is not None and out.tobytes() == c.expected(oracle, quantum).tobytes(), (name, op, wide_first, step)
            else:
                got = run(flw)
                assert got.dtype == exp.dtype and np.array_equal(got, exp), (name, op, wide_first, step)


def test_deferred_handle_whose_first_operation_is_the_wide_call(gpu_lib, oracle):
    from pyflwdir_amd import _hip

    for name in ("rand22_200x511_range1", "rand25_2100x200_range_2p20"):
        c = BY_NAME[name]
        idxs_ds, seq = c.graph(oracle)
        upa, _, _ = oracle.upstream_area_cell(c.d8)
        w = oracle.synth_weights_f32(c.n, seed=5)
        h = handle(c, deferred=True)
        out, quantum = h.upstream_area_rows_fixed(c.rows)
        assert out is not None and out.tobytes() == c.expected(oracle, quantum).tobytes()
        assert np.array_equal(h.upstream_area_cell(), upa.ravel())
        assert np.array_equal(h.strahler(None), oracle.strahler_order(idxs_ds, seq))
        assert np.array_equal(h.accuflux(w, _hip.PFD_F32, nodata_f=-9999.0, has_nodata=1), oracle.accuflux(idxs_ds, seq, w))
        out, quantum = h.upstream_area_rows_fixed(c.rows)
        assert out is not None and out.tobytes() == c.expected(oracle, quantum).tobytes()
        info = h.info(counts=True)
        assert info["n_valid"] == np.count_nonzero(c.d8 != 247) and info["n_pits"] == np.count_nonzero(idxs_ds == np.arange(c.n))
        h.close()
