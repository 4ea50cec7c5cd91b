"""What can be said about subbasins_area without a GPU: the two restatements of the reference's loop (tests/
subbasins_area_cases.py: the loop over the sequence as it stands, and one short loop per parent cell with jobs in
rounds — the form the device runs) reproduce every output that tools/gen_golden_subbasins_area.py recorded from the
reference (tests/golden/wide_subbasins_area.npz), in the pruned and in the full mode; the cases reach the edges the
device code can get wrong; the C-ABI entry is declared and bound."""
from __future__ import annotations

import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basin_cases as BC  # noqa: E402
import subbasins_area_cases as SC  # noqa: E402
from golden_util import digest  # noqa: E402

_REACHED = {}  # raster -> what its cases reached (filled by test_restatements_reproduce_the_record)


def _golden():
    return np.load(os.path.join(BC.GOLD, "wide_subbasins_area.npz"))


def matches(G, name, key, outs):
    """The outputs of a case that differ from the record (dtype, shape, bytes)."""
    bad = []
    for i, o in enumerate(outs):
        o = np.asarray(o)
        if name in SC.FULL:
            w = G[f"out_{key}_{i}"]
            ok = o.dtype == w.dtype and o.shape == w.shape and o.tobytes() == w.tobytes()
        else:
            ok = digest(o) == str(G[f"digest_{key}_{i}"])
        if not ok:
            bad.append(f"{key}_{i}")
    return bad


@pytest.mark.parametrize("name", SC.RASTERS)
def test_restatements_reproduce_the_record(oracle, name):
    G = _golden()
    src = SC.FromOracle(name, oracle)
    shape = src.d8.shape
    reached = dict(trib_before_main=0, trib_after_main=0, two_tribs=0, kept=0, interbasin=0, nan=0, pruned=0, full=0,
                   pits_only=0, rounds=0)
    bad = []
    for key, spec in SC.keys(name):
        A, area_min, _ = SC.case(spec, src)
        usm = SC.usm_of(spec, src, oracle)
        sub, idxs = SC.ref_serial(src.ds, src.seq, usm, A, area_min)
        bad += matches(G, name, key, (sub.reshape(shape), np.array(idxs, src.ds.dtype)))
        gsub, gidxs, info = SC.ref_groups(src.ds, src.seq, usm, A, area_min)
        assert gidxs == idxs and np.array_equal(gsub, sub), key
        if info["mode"] == 0 and name not in SC.LARGE:  # the full mode on the same input: the same answer
            fsub, fidxs, finfo = SC.ref_groups(src.ds, src.seq, usm, A, area_min, force_full=True)
            assert finfo["mode"] == 1 and fidxs == idxs and np.array_equal(fsub, sub), key
        for k in ("trib_before_main", "trib_after_main", "two_tribs", "kept", "interbasin", "nan"):
            reached[k] += info[k]
        reached["full" if info["mode"] else "pruned"] += 1
        reached["pits_only"] += int(len(idxs) == src.pits.size)
        reached["rounds"] = max(reached["rounds"], info["rounds"])
        if spec[0] != "special" or spec[1] != "cached":
            # the main upstream cells by cell count: every queued child holds at most half of its parent's cells
            assert info["rounds"] <= math.ceil(math.log2(max(src.seq.size, 2))) + 1, (key, info)
    assert not bad, bad
    _REACHED[name] = reached


def test_cases_reach_the_edges():
    """Over all rasters (the previous test has run on each): a tributary above the threshold before and after the
    main-stem child in index order, a group with two of them, the main-stem step that keeps what a tributary wrote, an
    inter-basin outlet, NaN areas, both modes, and a threshold that leaves the pits only."""
    assert set(_REACHED) == set(SC.RASTERS)
    total = {k: sum(r[k] for r in _REACHED.values()) for k in next(iter(_REACHED.values()))}
    assert all(v > 0 for v in total.values()), total


def test_case_list_holds_the_thresholds_and_types():
    """area_min of 0, negative, larger than every area, fractional on int32 areas; equal areas; a cached idxs_us_main that
    another area chose; strong numpy thresholds."""
    specs = [s for _, s in SC.keys("flwdir1")]
    for t in ("zero", "neg", "huge"):
        assert ("own", "km2", t) in specs and ("own", "cell", t) in specs
    assert ("own", "cell", "frac") in specs and ("south", "km2f", "mid") in specs
    for s in ("equal", "nan", "nep50_weak", "nep50_strong", "cached", "np_int", "np_f32"):
        assert ("special", s) in specs
    assert SC.threshold(np.arange(9), "zero") == 0 and SC.threshold(np.arange(9), "neg") < 0
    assert SC.threshold(np.arange(9), "huge") > 8 and SC.threshold(np.arange(9), "frac") % 1 != 0
    assert SC.compare_form(np.float32, 2.5) == ("own", 2.5) and SC.compare_form(np.int32, 2.5) == ("f64", 2.5)
    assert SC.compare_form(np.int32, 3) == ("own", 3) and SC.compare_form(np.float32, np.float64(2.5)) == ("f64", 2.5)
    assert SC.compare_form(np.float64, np.float32(2.5)) == ("own", 2.5) and SC.compare_form(np.int32, np.float32(2.5))[0] == "f64"
    assert SC.compare_form(np.float32, np.int64(3))[0] == "f64"


@pytest.mark.parametrize("name", SC.SPECIAL_RASTERS)
def test_nep50_case_decides_an_outlet(oracle, name):
    """The Python float lies one float64 step below a float32 difference that the loop forms; rounded to float32 it is
    that difference, and the outlets differ from those of the same value as np.float64."""
    src = SC.FromOracle(name, oracle)
    A, am, _ = SC.case(("special", "nep50_weak"), src)
    assert A.dtype == np.float32 and isinstance(am, float) and float(np.float32(am)) != am
    trace = []
    weak = SC.ref_serial(src.ds, src.seq, src.usm, A, am, trace)[1]
    strong = SC.ref_serial(src.ds, src.seq, src.usm, A, np.float64(am))[1]
    step = float(np.nextafter(np.float64(am), np.inf))
    assert step == float(np.float32(am)) and any(rest == step for rest, _ in trace)
    assert weak != strong


def test_symbols_declared_and_bound():
    from pyflwdir_amd import _hip

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pfd_subbasins_area\s*\(", header)
    # (bound: tests/test_cabi.py holds every bound signature to the header's types)
    assert "pfd_subbasins_area" in _hip.SYMBOLS and _hip.lib().pfd_subbasins_area.argtypes
    for name in ("PFD_COMPARE_OWN", "PFD_COMPARE_F64", "PFD_SUBAREA_FULL"):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == getattr(_hip, name), name


def test_front_end_signature_and_comparison_form():
    from pyflwdir_amd import _hip
    from pyflwdir_amd.raster import FlwdirRaster, _area_min_compare

    sig = inspect.signature(FlwdirRaster.subbasins_area)
    assert list(sig.parameters) == ["self", "area_min", "uparea"] and sig.parameters["uparea"].default is None
    form = {"own": _hip.PFD_COMPARE_OWN, "f64": _hip.PFD_COMPARE_F64}
    for dt in (np.int32, np.int64, np.float32, np.float64):
        for am in (0, 3, -2, 2.5, float("nan"), np.float64(2.5), np.float32(2.5), np.int64(3), np.int16(3), np.array(2.5)):
            want = SC.compare_form(dt, am)
            got = _area_min_compare(dt, am)
            assert got[1] == form[want[0]] and (got[0] == want[1] or (got[0] != got[0] and want[1] != want[1])), (dt, am)
    with pytest.raises(ValueError):
        _area_min_compare(np.float32, [1.0, 2.0])


def test_golden_file_is_complete():
    G = _golden()
    assert os.path.getsize(os.path.join(BC.GOLD, "wide_subbasins_area.npz")) < 1 << 20
    n = 0
    for name in SC.RASTERS:
        for key, _ in SC.keys(name):
            for i in range(2):
                assert (f"out_{key}_{i}" if name in SC.FULL else f"digest_{key}_{i}") in G.files, key
                n += 1
    assert n == len(G.files)  # (no case is left out of the record, and the record holds nothing else)
