"""What can be said about subbasins_streamorder / outflow_idxs / basin_outlets without a GPU: the C-ABI entries are
declared in include/pfd.h and bound in pyflwdir_amd/_hip.py, the front end has the three methods with the reference's
signatures, and tests/golden/wide_outlets.npz holds every case with the outlet counts the reference is known to give."""
from __future__ import annotations

import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlet_cases as OC  # noqa: E402

NEW = ["pfd_subbasins_streamorder", "pfd_outflow_idxs", "pfd_basin_outlets"]


def test_symbols_declared_and_bound():
    from pyflwdir_amd import _hip

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _hip.SYMBOLS and getattr(_hip.lib(), name).argtypes, name  # (test_cabi.py: with the header's types)
    assert "#define PFD_ABI_VERSION 1" in header


def test_front_end_signatures():
    from pyflwdir_amd.raster import FlwdirRaster

    sig = inspect.signature(FlwdirRaster.subbasins_streamorder)
    assert list(sig.parameters) == ["self", "strord", "mask", "min_sto"]
    assert [sig.parameters[p].default for p in ("strord", "mask", "min_sto")] == [None, None, -2]
    assert list(inspect.signature(FlwdirRaster.outflow_idxs).parameters) == ["self", "region"]
    assert list(inspect.signature(FlwdirRaster.basin_outlets).parameters) == ["self", "basins"]


def test_golden_file_is_complete():
    G = np.load(os.path.join(ROOT, "tests", "golden", "wide_outlets.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "wide_outlets.npz")) < 1 << 20
    for name in OC.RASTERS + OC.GENERAL:
        for key, call, _ in OC.keys(name):
            nout = 1 if call == "outflow" else 2
            for i in range(nout):
                assert (f"out_{key}_{i}" if name in OC.FULL else f"digest_{key}_{i}") in G.files, key
            assert f"count_{key}" in G.files
    for name, counts in OC.KNOWN_COUNTS.items():
        for min_sto, k in counts.items():
            assert int(G[f"count_{name}_sto_strahler_{min_sto}"]) == k, (name, min_sto)
    # the empty case keeps dtype and shape: no outlets, an all-zero int32 map
    sub, idxs = G["out_flwdir1_sto_strahler_4_0"], G["out_flwdir1_sto_strahler_4_1"]
    assert sub.dtype == np.int32 and sub.shape == (15, 10) and not sub.any() and idxs.size == 0 and idxs.dtype == np.int32
    # outflow cells lie inside their region; outlet labels are sorted
    for name in sorted(OC.FULL & set(OC.RASTERS)):
        shape = G[f"out_{name}_sto_strahler_1_0"].shape
        for r in OC.REGIONS:
            assert OC.region(shape, r).ravel()[G[f"out_{name}_outflow_{r}_0"]].all()
        lbs = G[f"out_{name}_outlets_basins_0"]
        assert np.array_equal(lbs, np.sort(lbs)) and lbs.size
