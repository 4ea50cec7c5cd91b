"""The round chain of the interior local tile pass (k_tile_local_fast): its first jump rounds run per wave, without
barrier or vote, and only then the voted loop takes over.  That may not change a result: everything here is the
oracle's, bit for bit, on an eager and on a deferred handle, through both tile passes.  The rasters are the smallest on
which these loops can go wrong — interior tiles need 3 x 3 tiles at least; 320 x 448 is 5 x 7 — and are built for what
the loops are sensitive to: the hand-over from free to voted rounds, waves of a tile that finish at different times and
read each other's pointers, paths that change wave every few hops, a cycle (never saturates), tiles with nothing to do.
(The supertile solves keep their voted rounds: nothing of them is tested here.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fuzz import random_d8  # noqa: E402  (the generator of the fuzz suite)

pytestmark = pytest.mark.gpu

SHAPE = (320, 448)  # 5 x 7 tiles, 3 x 5 of them interior
_REF = {}


def _ref(oracle, key, make):
    """raster + oracle answer, computed once per key and shared (never modified)."""
    if key not in _REF:
        d8 = np.ascontiguousarray(make(), dtype=np.uint8)
        d8.setflags(write=False)
        exp = oracle.upstream_area_cell(d8)[0]
        exp.setflags(write=False)
        _REF[key] = (d8, exp)
    return _REF[key]


def _both_handles(d8, exp):
    from pyflwdir_amd import _hip

    for deferred in (False, True):
        h = _hip.RasterHandle(d8, d8.shape[0], d8.shape[1], deferred=deferred)
        got = h.upstream_area_cell().reshape(d8.shape)
        h.close()
        assert np.array_equal(got, exp), f"deferred={deferred}"


def _tile_rounds(d8):
    """(result, round statistics) of a deferred handle with pfd_set_profiling(h, 2)"""
    from pyflwdir_amd import _hip

    h = _hip.RasterHandle(d8, d8.shape[0], d8.shape[1], deferred=True)
    h.set_profiling(2)
    upa = h.upstream_area_cell().reshape(d8.shape)
    st = h.graph_stats()["tile_rounds"]
    h.close()
    return upa, st


def _acyclic(oracle, d8):
    return not (oracle.rank(oracle.from_array(d8)[0])[0] == -1).any()


# ---- 1. hand-over from the free to the voted rounds ------------------------------------------------------------------
def serpentine(nrow, ncol):
    """every 64 x 64 tile one boustrophedon of 4096 cells that ends in a pit: the longest in-tile path there is"""
    t = np.empty((64, 64), np.uint8)
    t[0::2, :] = 1
    t[1::2, :] = 16
    t[0::2, 63] = 4
    t[1::2, 0] = 4
    t[63, 0] = 0
    return np.ascontiguousarray(np.tile(t, (-(-nrow // 64), -(-ncol // 64)))[:nrow, :ncol])


def test_free_to_voted_handover(gpu_lib, oracle):
    """No tile is done after the free rounds, every tile needs voted rounds behind them, and the final pass all 12 of
    its own.  The frame tiles (general kernel, one jump per round) report 12 local rounds; an interior tile reports its
    free rounds + its voted rounds and must stay at or below that."""
    d8, exp = _ref(oracle, "serpentine", lambda: serpentine(*SHAPE))
    assert exp.max() == 4096
    _both_handles(d8, exp)
    upa, st = _tile_rounds(d8)
    assert np.array_equal(upa, exp)
    nt, nframe = 5 * 7, 5 * 7 - 3 * 5
    interior_mean = (st["local_mean"] * nt - 12.0 * nframe) / (nt - nframe)
    print(f"tile_rounds {st}, interior local mean {interior_mean:.3f}")
    assert st["local_max"] <= 12 and st["final_max"] == 12 and st["final_mean"] == 12.0
    assert 1.0 < interior_mean <= 12.0


# ---- 2. waves that finish at different times ---------------------------------------------------------------------------
def _pit_rows(first):
    """Rows r with r % 16 in [first, first + 4) — the rows of ONE wave of a tile (thread t holds rows (t >> 4) + 16 j) —
    are pits: that wave is saturated before the first round.  The other rows are east / west runs that turn south at
    the side columns of their tile, 12 rows = 768 cells to the pit row below: the other waves need many rounds and end
    by gathering through the finished wave's cells."""
    r = np.arange(SHAPE[0])[:, None] + np.zeros(SHAPE, np.int64)
    c = np.arange(SHAPE[1])[None, :] + np.zeros(SHAPE, np.int64)
    east = (r % 2) == 0
    d8 = np.where(east, 1, 16).astype(np.uint8)
    d8[east & (c % 64 == 63)] = 4
    d8[~east & (c % 64 == 0)] = 4
    d8[((r % 16) >= first) & ((r % 16) < first + 4)] = 0
    return d8


@pytest.mark.parametrize("first", [0, 12])
def test_waves_finish_at_different_times(gpu_lib, oracle, first):
    d8, exp = _ref(oracle, ("pit_rows", first), lambda: _pit_rows(first))
    assert _acyclic(oracle, d8) and exp.max() >= 12 * 64  # a whole run of 12 rows drains into one pit
    _both_handles(d8, exp)


# ---- 3. paths that leave and re-enter a wave's rows --------------------------------------------------------------------
def _staircase(up):
    """rows of period 3: SE, S, SW (down) or NW, N, NE (up): a path zigzags through every row — hence through the
    rows of all four waves of a tile, in turn — from one end of the raster to the other"""
    codes = (32, 64, 128) if up else (2, 4, 8)
    d8 = np.empty(SHAPE, np.uint8)
    for k in range(3):
        d8[k::3, :] = codes[k]
    return d8


@pytest.mark.parametrize("up", [False, True])
def test_staircase_across_waves(gpu_lib, oracle, up):
    d8, exp = _ref(oracle, ("staircase", up), lambda: _staircase(up))
    assert _acyclic(oracle, d8) and exp.max() >= SHAPE[0] - 2  # paths run the height of the raster
    _both_handles(d8, exp)


# ---- 4. a cycle inside an interior tile ----------------------------------------------------------------------------------
def _cycle_raster():
    d8 = np.full(SHAPE, 4, np.uint8)  # south, off the raster
    d8[100, 60:100] = 1               # 40 cells east, into the loop ...
    d8[100, 100] = 1                  # ... (100, 100) <-> (100, 101), inside tile (1, 1)
    d8[100, 101] = 16
    return d8


def test_cycle_in_interior_tile(gpu_lib, oracle):
    """The cells on and above the loop never reach a root word, in the free rounds or in the voted ones: the pass counts
    them behind the voted loop as before and the raster is computed by the engine that handles cycles."""
    d8, exp = _ref(oracle, "cycle", _cycle_raster)
    on_cycle = oracle.rank(oracle.from_array(d8)[0])[0].reshape(SHAPE) == -1
    assert on_cycle[100, 100] and on_cycle[100, 101] and on_cycle[100, 60] and on_cycle[0, 60] and not on_cycle[101, 100]
    _both_handles(d8, exp)


# ---- 5. nothing to do ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 70), SHAPE])
def test_all_pits(gpu_lib, oracle, shape):
    """no wave is live in a free round and the one voted round says "nobody": 1 round, both passes"""
    d8, exp = _ref(oracle, ("pits", shape), lambda: np.zeros(shape, np.uint8))
    assert (exp == 1).all()
    _both_handles(d8, exp)
    upa, st = _tile_rounds(d8)
    assert (upa == 1).all()
    assert st["local_max"] == st["final_max"] == 1 and st["local_mean"] == st["final_mean"] == 1.0


# ---- 7. random acyclic rasters ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_random_acyclic(gpu_lib, oracle, seed):
    """200 x 260: 4 x 5 tiles, the inner ones interior; E / SE / S / SW only, with pits and nodata"""
    def make():
        rng = np.random.default_rng(7000 + seed)
        return random_d8(rng, (200, 260), p_nodata=rng.choice([0.0, 0.1, 0.4]), p_pit=rng.choice([0.002, 0.05]), coherent=-1)

    d8, exp = _ref(oracle, ("random", seed), make)
    assert _acyclic(oracle, d8)
    _both_handles(d8, exp)
