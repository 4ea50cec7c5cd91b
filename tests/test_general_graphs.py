"""The graphs of tests/general_graphs.py, on the CPU: every case that tests/test_gpu_general_fuzz.py runs on the device
meets the conditions under which the oracle (and the reference it restates) is defined — in-degree at most 100, no link
into a nodata cell, at least one pit and two valid cells, at least half of the valid cells on a path to a pit — the
oracle answers it with a sequence as long as its count of ranked cells, it is a graph the D8 engines refuse, and the
same arguments give the same bytes twice."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import general_graphs as GG  # noqa: E402

IDS = [GG.case_id(c) for c in GG.CASES]
_STATS = {}


def test_case_list_covers_the_regimes():
    fams = {c["family"] for c in GG.CASES}
    assert fams == set(GG.FAMILIES) and 35 <= len(GG.CASES) <= 50
    for fam in GG.FAMILIES:
        shapes = {c["shape"] for c in GG.CASES if c["family"] == fam}
        assert shapes == set(GG.SHAPES), fam
    assert len(set(IDS)) == len(IDS)


def _analyse(O, c):
    """Graph facts of one case, computed once: (ds, valid, pits, indeg, reach, seq, rank)."""
    key = GG.case_id(c)
    if key not in _STATS:
        ds = GG.build(c)
        n = ds.size
        valid = ds != -1
        idx = np.arange(n)
        # no link leaves the valid cells (checked here: the lines below index with the links)
        assert np.all((ds[valid] >= 0) & (ds[valid] < n)) and np.all(valid[ds[valid]]), key
        pits = np.flatnonzero(valid & (ds == idx)).astype(np.int32)
        indeg = np.bincount(ds[valid & (ds != idx)], minlength=n)
        reach = GG.reaches_pit(ds, -1)
        _STATS[key] = (ds, valid, pits, indeg, reach, O.idxs_seq(ds, pits), O.rank(ds)[0])
    return _STATS[key]


@pytest.mark.parametrize("c", GG.CASES, ids=IDS)
def test_case_conditions(oracle, c):
    from pyflwdir_amd import raster

    O = oracle
    ds, valid, pits, indeg, reach, seq, rnk = _analyse(O, c)
    n = c["shape"][0] * c["shape"][1]
    assert ds.dtype == np.int32 and ds.shape == (n,)
    assert GG.build(c).tobytes() == ds.tobytes()
    for dt in (np.uint32, np.int64):  # the same graph in the other index dtypes, with their missing value
        other = GG.build(c, dtype=dt)
        assert other.dtype == dt and np.array_equal(other == GG.missing_value(dt), ds == -1)
        assert np.array_equal(other[ds != -1].astype(np.int64), ds[ds != -1].astype(np.int64))
    assert valid.sum() >= 2 and pits.size >= 1
    assert indeg.max(initial=0) <= GG.MAX_INDEGREE
    assert 2 * reach.sum() >= valid.sum()
    assert seq.size == np.count_nonzero(rnk >= 0) == reach.sum()
    assert np.array_equal(np.sort(seq), np.flatnonzero(reach))
    assert np.array_equal(O.upstream_count(ds)[valid], indeg[valid].astype(np.int8))
    if c["family"] == "chain":
        assert rnk.max() < GG.MAX_CHAIN and valid.sum() <= GG.MAX_CHAIN
    if c["family"] == "allpits":
        assert np.array_equal(pits, np.flatnonzero(valid)) and rnk.max() == 0
    if GG.cannot_be_general(c):  # (two neighbouring cells / no links at all: see general_graphs.cannot_be_general)
        raster._d8_from_idxs_ds(ds, c["shape"], -1)
    else:
        with pytest.raises(ValueError, match="outside 8 neighbors"):
            raster._d8_from_idxs_ds(ds, c["shape"], -1)


def test_cases_reach_the_regimes(oracle):
    """Taken together the cases are what the general engine exists for (not a condition on one case): the in-degree cap
    is reached, the deepest chain has 3000 levels, and most cases that ask for cycles have cells off the sequence."""
    S = {GG.case_id(c): _analyse(oracle, c) for c in GG.CASES}
    indeg = {k: int(v[3].max(initial=0)) for k, v in S.items()}
    assert max(indeg.values()) == GG.MAX_INDEGREE
    assert max(indeg[GG.case_id(c)] for c in GG.CASES if c["family"] == "pref") >= 50
    assert max(int(v[6].max()) for v in S.values()) == GG.MAX_CHAIN - 1  # (ranks 0 .. 2999)
    want = [GG.case_id(c) for c in GG.CASES if c["n_cycles"] and not GG.cannot_be_general(c)]
    have = [k for k in want if S[k][4].sum() < S[k][1].sum()]
    assert len(have) >= 0.8 * len(want), sorted(set(want) - set(have))
