"""What can be said about interbasin_mask / inflow_idxs / basin_bounds / subbasins_pfafstetter without a GPU: the plain
restatements of the four serial loops (tests/basin_cases.py) reproduce every output that tools/gen_golden_basins.py
recorded from the reference (tests/golden/wide_basins.npz), the cases reach the corners the device code can get wrong,
every depth keeps a tie-free Pfafstetter case, and the C-ABI entries are declared and bound."""
from __future__ import annotations

import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basin_cases as BC  # noqa: E402
from golden_util import digest  # noqa: E402
from serial_refs import _ref_streamorder  # noqa: E402

NEW = ["pfd_interbasin_mask", "pfd_inflow_idxs", "pfd_basin_bounds", "pfd_subbasins_pfafstetter"]
_REACHED = {}  # raster -> what its cases reached (filled by test_restatements_reproduce_the_records)


def _golden():
    return np.load(os.path.join(BC.GOLD, "wide_basins.npz"))


def _matches(G, name, key, outs):
    bad = []
    for i, o in enumerate(outs):
        o = np.asarray(o)
        if name in BC.FULL:
            w = G[f"out_{key}_{i}"]
            ok = o.dtype == w.dtype and o.shape == w.shape and o.tobytes() == w.tobytes()
        else:
            ok = digest(o) == str(G[f"digest_{key}_{i}"])
        if not ok:
            bad.append(f"{key}_{i}")
    return bad


@pytest.mark.parametrize("name", BC.RASTERS)
def test_restatements_reproduce_the_records(oracle, name):
    O = oracle
    G = _golden()
    d8, ds, pits, seq = BC.graph(name, O)
    shape, n = d8.shape, d8.size
    tr, latlon = BC.transform_of(name, "own")
    upa = BC.areas(O, ds, seq, shape, tr, latlon)
    us_main = O.main_upstream(ds, upa["cell"].ravel())
    stream = (upa["cell"] > BC.threshold(upa["cell"])).ravel()
    dsl, seql = ds.tolist(), seq.tolist()
    strahler = O.strahler_order(ds, seq).ravel().tolist()
    maps = dict(basins=O.basins(ds, pits, seq).reshape(shape),
                sub=np.array(_ref_streamorder(dsl, seql, strahler, -1)[0], np.int32).reshape(shape))
    pos = np.full(n, n, np.int64)
    pos[seq] = np.arange(seq.size)
    reached = dict(more_than_4=0, fewer_than_4=0, already_listed=0, stem_ends_at_order_0=0, entry_first_child=0,
                   entry_other_child=0, reentered=0, pit_without_stream=0, pfaf={d: 0 for d in BC.DEPTHS})
    bad = []
    for key, call, args in BC.keys(name):
        if call == "interbasin":
            reg = BC.region(shape, args[0]).ravel()
            out = BC._ref_interbasin(ds, seq, reg, stream if args[1] == "upa" else None).reshape(shape)
            bad += _matches(G, name, key, (out,))
            if args[1] == "none":
                reached["reentered"] += int((reg & ~out.ravel()).any())
            elif args[0] == "all":  # with the whole raster as region only a basin without a stream cell is cleared
                reached["pit_without_stream"] += int((~out.ravel()[pits]).any())
        elif call == "inflow":
            reg = BC.region(shape, args[0]).ravel()
            out = np.array(BC._ref_inflow(ds, seq, reg), ds.dtype)
            bad += _matches(G, name, key, (out,))
            # entry edges by the place of the entering cell among its parent's upstream cells
            x = seq[(ds[seq] != seq) & ~reg[seq] & reg[ds[seq]]]
            first = np.full(n, n, np.int64)
            np.minimum.at(first, ds[seq], pos[seq])
            reached["entry_first_child"] += int((first[ds[x]] == pos[x]).sum())
            reached["entry_other_child"] += int((first[ds[x]] != pos[x]).sum())
        elif call == "bounds":
            bad += _matches(G, name, key, BC._ref_bounds(maps[args[0]], BC.transform_of(name, args[1])[0]))
        else:
            assert bool(G[f"tie_{key}"]) == (f"{'out' if name in BC.FULL else 'digest'}_{key}_0" not in G.files)
            a = upa[args[1]].ravel()
            mask = a >= (0.0 if args[2] == "zero" else BC.threshold(a))
            pf, idxs, info = BC._ref_pfafstetter(pits, ds, seq, us_main, a, mask, args[0])
            assert info["ties"] == bool(G[f"tie_{key}"]), key  # (the reporter is the generator's)
            if info["ties"]:
                continue
            bad += _matches(G, name, key, (pf.reshape(shape), np.array(idxs, ds.dtype)))
            reached["pfaf"][args[0]] += 1
            for k in ("more_than_4", "fewer_than_4", "already_listed", "stem_ends_at_order_0"):
                reached[k] += info[k]
    assert not bad, bad
    _REACHED[name] = reached


def test_cases_reach_the_corners():
    """Over all rasters (the previous test has run on each): a label with more and with fewer than 4 candidate
    tributaries, an inter-basin outlet that is already listed, a main stem that ends where the capped stream order is 0,
    entry edges on and off a first-child chain, a river that re-enters its region, a pit without a stream cell in its
    basin — and per depth a Pfafstetter case without ties."""
    assert set(_REACHED) == set(BC.RASTERS)
    total = {k: sum(r[k] for r in _REACHED.values()) for k in next(iter(_REACHED.values())) if k != "pfaf"}
    assert all(v > 0 for v in total.values()), total
    for d in BC.DEPTHS:
        assert sum(r["pfaf"][d] for r in _REACHED.values()) >= 1, d


def test_fuzz_seeds_keep_half_of_the_pfafstetter_cases(oracle):
    """The fixed seed list of tests/test_gpu_basins_ext.py leaves, per depth, at least half of its random rasters without
    a tie, and the kept ones hold outlets beyond the pits."""
    import test_gpu_basins_ext as T

    for depth in BC.DEPTHS:
        ties, more = [], 0
        for shape in T.FUZZ_SHAPES:
            for seed in T.FUZZ_SEEDS:
                c = T.fuzz_case(oracle, shape, seed)
                _, _, idxs, tie = T.fuzz_pfaf(c, depth)
                ties.append(tie)
                more += 0 if tie else idxs.size - c.pits.size
        assert 2 * sum(ties) <= len(ties) and more > 100, (depth, ties, more)


def test_tie_reporter():
    """Two tributaries of equal area are a tie; distinct areas are none."""
    # 0 <- 1 <- 2 <- 5 is the main stem; 3 joins cell 1, 4 joins cell 2
    ds = np.array([0, 0, 1, 1, 2, 2], np.int32)
    seq = np.arange(6, dtype=np.int32)
    us_main = np.array([1, 2, 5, -1, -1, -1], np.int32)
    mask = np.ones(6, bool)
    assert BC.pfaf_ties([0], ds, seq, us_main, np.array([20, 15, 9, 2, 2, 5], np.int32), mask, 1)
    upa = np.array([20, 15, 9, 3, 2, 5], np.int32)
    assert not BC.pfaf_ties([0], ds, seq, us_main, upa, mask, 1)
    pf, idxs, _ = BC._ref_pfafstetter([0], ds, seq, us_main, upa, mask, 1)
    assert pf.tolist() == [1, 1, 3, 2, 4, 5] and idxs == [0, 3, 2, 4, 5]


def test_symbols_declared_and_bound():
    from pyflwdir_amd import _hip

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _hip.SYMBOLS and getattr(_hip.lib(), name).argtypes, name  # (test_cabi.py: with the header's types)
    assert "#define PFD_ABI_VERSION 1" in header


def test_front_end_signatures():
    from pyflwdir_amd.raster import FlwdirRaster

    sig = inspect.signature(FlwdirRaster.subbasins_pfafstetter)
    assert list(sig.parameters) == ["self", "depth", "uparea", "upa_min"]
    assert [sig.parameters[p].default for p in ("depth", "uparea", "upa_min")] == [1, None, 0.0]
    sig = inspect.signature(FlwdirRaster.interbasin_mask)
    assert list(sig.parameters) == ["self", "region", "stream"] and sig.parameters["stream"].default is None
    assert list(inspect.signature(FlwdirRaster.inflow_idxs).parameters) == ["self", "region"]
    sig = inspect.signature(FlwdirRaster.basin_bounds)
    assert list(sig.parameters) == ["self", "basins", "kwargs"] and sig.parameters["basins"].default is None


def test_golden_file_is_complete():
    G = _golden()
    assert os.path.getsize(os.path.join(BC.GOLD, "wide_basins.npz")) < 1 << 20
    for name in BC.RASTERS:
        for key, call, _ in BC.keys(name):
            if call == "pfaf" and bool(G[f"tie_{key}"]):
                continue
            nout = {"interbasin": 1, "inflow": 1, "bounds": 3, "pfaf": 2}[call]
            for i in range(nout):
                assert (f"out_{key}_{i}" if name in BC.FULL else f"digest_{key}_{i}") in G.files, key
