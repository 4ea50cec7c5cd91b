"""Acyclic rasters whose paths WIND, shared by tests/test_winding_cases.py (CPU: the rasters have the properties they are
built for) and tests/test_gpu_winding.py (GPU: the tiled and exact engines against the oracle on them).  numpy and the
standard library only; nothing here touches the library under test or the oracle.

Every other random acyclic raster of the suite is ``random_d8(..., coherent=-1)`` of tests/test_gpu_fuzz.py: only E / SE / S /
SW, so the row never decreases along a path.  Such a path never comes back to a band of tile rows, a supertile row or a row
block it has left, and no in-tile path is longer than 127 cells.  The rasters here are trees in all eight directions:

* ``invasion_tree``: invasion percolation from a few random pits, one uniform key per (cell, direction).  Paths are fractal:
  they leave a tile and come back several times, and all eight directions are equally frequent.
* ``serp_tiles``: every 64 x 64 tile is one path of 4096 cells — every doubling round of the tile passes runs.
* ``serp_whole``: one boustrophedon over the whole raster — one path crosses every tile (supertile) edge once per row.
* ``edge_river``: a river that crosses one line at every step, fed by straight tributaries from both sides.
* ``corner_spiral``: a square spiral around a tile corner — one path enters each of the four tiles ``laps`` times.
* ``with_nodata_holes``: nodata punched into any of them; edges are only removed, so the raster stays acyclic.

``case(name)`` builds a raster once per process; ``NAMES`` and the ``*_NAMES`` lists need no generation."""
from __future__ import annotations

import functools
import heapq
from types import SimpleNamespace

import numpy as np

TS, SUPER, HYPER = 64, 512, 2048  # tile, supertile and hypertile edges in cells (csrc/tiled.h)
NODATA = 247
PIT_CODES = (0, 255)
STEP = {1: (0, 1), 2: (1, 1), 4: (1, 0), 8: (1, -1), 16: (0, -1), 32: (-1, -1), 64: (-1, 0), 128: (-1, 1)}
D8_VALUES = np.array(sorted(STEP) + [0, 255, 247], np.uint8)
_TRANSPOSED = {1: 4, 2: 2, 4: 1, 8: 128, 16: 64, 32: 32, 64: 16, 128: 8, 0: 0, 255: 255, 247: 247}


# ---- the graph of a raster, in numpy ---------------------------------------------------------------------------------------------
def downstream(d8):
    """Flat int64 index of every cell's downstream cell: itself for a pit code, for flow off the raster and for flow into
    nodata; -1 on nodata (what the reference's ``from_array`` decodes)."""
    nrow, ncol = d8.shape
    flat = d8.ravel()
    idx = np.arange(d8.size, dtype=np.int64)
    r, c = np.divmod(idx, ncol)
    ds = np.where(flat == NODATA, -1, idx)
    for code, (dr, dc) in STEP.items():
        m = np.flatnonzero(flat == code)
        rr, cc = r[m] + dr, c[m] + dc
        ok = (rr >= 0) & (rr < nrow) & (cc >= 0) & (cc < ncol)
        tgt = np.where(ok, rr * ncol + cc, 0)
        ok &= flat[tgt] != NODATA
        ds[m] = np.where(ok, tgt, m)
    return ds


def path_sums(ds, w):
    """Per cell the sum of ``w`` over the links of its path to the pit (``w[x]`` belongs to the link x -> ds[x]), by pointer
    doubling; -1 where the path does not end (a cycle) and on nodata."""
    idx = np.arange(ds.size, dtype=np.int64)
    valid = ds >= 0
    nxt = np.where(valid, ds, idx)
    s = np.where(nxt != idx, np.asarray(w, np.int64), 0)
    for _ in range(64):
        n2 = nxt[nxt]
        s = s + s[nxt]
        if np.array_equal(n2, nxt):
            break
        nxt = n2
    out = np.where(valid & (nxt[nxt] == nxt) & (ds[nxt] == nxt), s, -1)
    return out


def hops(ds):
    """Links between every cell and its pit (the reference's ``rank``): -1 on nodata and on or behind a cycle."""
    return path_sums(ds, np.ones(ds.size, np.int64))


def path_from(ds, x):
    """The cells of the path from ``x`` to its pit, both included."""
    ds = ds.tolist()
    out = [int(x)]
    while ds[out[-1]] != out[-1]:
        out.append(ds[out[-1]])
        assert len(out) <= len(ds), "a cycle"
    return np.array(out, np.int64)


def _boxes(shape, edge, axis=None):
    """Per cell the id of its ``edge`` x ``edge`` box; ``axis`` 0 / 1: of its band of rows / columns."""
    nrow, ncol = shape
    r, c = np.divmod(np.arange(nrow * ncol, dtype=np.int64), ncol)
    if axis == 0:
        return r // edge
    if axis == 1:
        return c // edge
    return (r // edge) * -(-ncol // edge) + c // edge


def visits(path, shape, edge=TS, axis=None):
    """Walking ``path``: (box visits, distinct boxes, the most entries into one box)."""
    box = _boxes(shape, edge, axis)[path]
    starts = np.concatenate([[True], box[1:] != box[:-1]])
    _, counts = np.unique(box[starts], return_counts=True)
    return int(starts.sum()), int(counts.size), int(counts.max())


def crossings(path, shape, axis, line):
    """How often ``path`` steps between ``line`` and ``line + 1`` (rows for axis 0, columns for axis 1)."""
    pos = np.divmod(path, shape[1])[axis]
    lo, hi = np.minimum(pos[1:], pos[:-1]), np.maximum(pos[1:], pos[:-1])
    return int(((lo == line) & (hi == line + 1)).sum())


def most_entries(ds, shape, edge=TS, axis=None):
    """The most often ANY path of the raster enters one box (1: no path comes back to a box it has left; 0: no valid cell).
    Every cell that leaves its box starts a walk from box to box that counts the returns to the box it left."""
    idx = np.arange(ds.size, dtype=np.int64)
    valid = ds >= 0
    if not valid.any():
        return 0
    box = _boxes(shape, edge, axis)
    dsv = np.where(valid, ds, idx)
    leaves = valid & (box[dsv] != box)
    last = np.where(leaves, idx, dsv)  # the last cell of every cell's path inside its box: an exit or the pit
    for _ in range(64):
        n2 = last[last]
        if np.array_equal(n2, last):
            break
        last = n2
    start = np.flatnonzero(leaves)
    home, cur, count = box[start], dsv[start], np.ones(start.size, np.int64)
    best = 1
    for _ in range(ds.size):
        if cur.size == 0:
            break
        count = count + (box[cur] == home)
        best = max(best, int(count.max()))
        e = last[cur]
        live = leaves[e]
        home, cur, count = home[live], dsv[e[live]], count[live]
    assert cur.size == 0, "a cycle"
    return best


def longest_in_box_path(ds, shape, edge=TS):
    """The most links any path makes without leaving its box."""
    box = _boxes(shape, edge)
    idx = np.arange(ds.size, dtype=np.int64)
    dsv = np.where(ds >= 0, ds, idx)
    inside = np.where(box[dsv] == box, dsv, idx)
    inside[ds < 0] = -1
    return int(hops(inside).max())


def block_edge_crossings(ds, shape, rows):
    """The most links of one path that cross an edge between the row blocks ``rows`` ([r0, r1) each): the number of
    boundary-row exchanges the row-block sweeps need before that path's values are final."""
    ncol = shape[1]
    blk = np.zeros(shape[0], np.int64)
    for b, (r0, r1) in enumerate(rows):
        blk[r0:r1] = b
    cell = np.repeat(blk, ncol)
    idx = np.arange(ds.size, dtype=np.int64)
    dsv = np.where(ds >= 0, ds, idx)
    return int(path_sums(ds, cell[dsv] != cell).max())


def direction_shares(d8):
    """The share of each of the eight directions among the links (cells that hold a direction code)."""
    counts = np.array([(d8 == code).sum() for code in sorted(STEP)], np.float64)
    return counts / counts.sum()


# ---- generators --------------------------------------------------------------------------------------------------------------------
def transpose_d8(d8):
    """The raster mirrored at its main diagonal: rows become columns and every code the mirrored direction."""
    lut = np.zeros(256, np.uint8)
    for a, b in _TRANSPOSED.items():
        lut[a] = b
    return np.ascontiguousarray(lut[d8].T)


def invasion_tree(shape, seed, n_pits, p_nodata):
    """Invasion percolation: ``n_pits`` random valid cells are pits (codes 0 and 255 in turn); the cheapest frontier edge
    (a free cell x, a direction d into an attached cell) is popped from a heap and x attached with code d, until nothing is
    left.  One uniform random key per (cell, direction): with one key per cell, ties between a cell's eight edges fall to
    the smallest code and 85 % of the raster comes out E / SE / S / SW.  Nodata is marked up front with probability
    ``p_nodata``; of the valid cells that nodata cuts off from every pit, the first in index order becomes a pit and the
    invasion goes on from it."""
    rng = np.random.default_rng(seed)
    nrow, ncol = shape
    w = ncol + 2  # a frame of blocked cells, so that a neighbour is one addition away
    state = np.full((nrow + 2, w), 2, np.uint8)  # 0 free, 1 attached, 2 nodata / frame
    state[1:-1, 1:-1] = np.where(rng.random(shape) < p_nodata, 2, 0)
    free = np.flatnonzero(state.ravel() == 0)
    assert free.size >= n_pits and state.size * 8 < 1 << 23
    # a key holds its (cell, direction) in its low 23 bits: no ties, and the heap holds plain integers
    keys = ((rng.integers(0, 1 << 40, state.size * 8, dtype=np.int64) << 23) | np.arange(state.size * 8, dtype=np.int64)).tolist()
    codes = list(STEP)
    into = [(-(dr * w + dc), k) for k, (dr, dc) in enumerate(STEP.values())]  # x = y + offset flows into y with codes[k]
    st = state.ravel().tolist()
    out = [NODATA] * state.size
    heap = []
    push, pop = heapq.heappush, heapq.heappop
    roots = rng.choice(free, n_pits, replace=False).tolist()
    pending = iter(free.tolist())
    n_roots = 0
    while True:
        for y in roots:
            st[y], out[y] = 1, PIT_CODES[n_roots % 2]
            n_roots += 1
            for o, k in into:
                x = y + o
                if st[x] == 0:
                    push(heap, keys[x * 8 + k])
        while heap:
            xk = pop(heap) & 0x7FFFFF
            y = xk >> 3
            if st[y]:
                continue
            st[y], out[y] = 1, codes[xk & 7]
            for o, k in into:
                x = y + o
                if st[x] == 0:
                    push(heap, keys[x * 8 + k])
        y = next((x for x in pending if st[x] == 0), None)
        if y is None:
            break
        roots = [y]
    return np.ascontiguousarray(np.array(out, np.uint8).reshape(nrow + 2, w)[1:-1, 1:-1])


def serp_tiles(nrow, ncol):
    """Every 64 x 64 tile is one boustrophedon path of 4096 cells ending in a pit (even rows flow east, odd rows west, the
    row ends south): the longest in-tile path there is (bench.py's ``serpentine`` regime)."""
    t = np.empty((TS, TS), np.uint8)
    t[0::2, :] = 1
    t[1::2, :] = 16
    t[0::2, TS - 1] = 4
    t[1::2, 0] = 4
    t[TS - 1, 0] = 0
    return np.ascontiguousarray(np.tile(t, (-(-nrow // TS), -(-ncol // TS)))[:nrow, :ncol])


def serp_whole(nrow, ncol, axis):
    """One boustrophedon over the whole raster ending in a pit.  ``axis`` 1: along the rows (even rows east, odd rows west,
    the row ends south); ``axis`` 0: along the columns."""
    if axis == 0:
        return transpose_d8(serp_whole(ncol, nrow, 1))
    d8 = np.empty((nrow, ncol), np.uint8)
    d8[0::2, :] = 1
    d8[1::2, :] = 16
    d8[0::2, ncol - 1] = 4
    d8[1::2, 0] = 4
    d8[nrow - 1, (ncol - 1) if (nrow - 1) % 2 == 0 else 0] = 0
    return d8


def edge_river(shape, axis, line, tributaries=True):
    """A river that crosses the edge between ``line`` and ``line + 1`` at EVERY step (rows for ``axis`` 0: SE, NE, SE, ...;
    columns for ``axis`` 1) from index 0 to a pit at the far end; ``tributaries``: straight lines of cells that flow into
    every river cell from its own side, out to the raster's edge.  Everything else is nodata."""
    if axis == 1:
        return transpose_d8(edge_river(shape[::-1], 0, line, tributaries))
    nrow, ncol = shape
    assert 0 <= line and line + 1 < nrow
    d8 = np.full(shape, NODATA, np.uint8)
    d8[line, 0:ncol - 1:2] = 2  # SE -> (line + 1, c + 1)
    d8[line + 1, 1:ncol - 1:2] = 128  # NE -> (line, c + 1)
    d8[line + (ncol - 1) % 2, ncol - 1] = 0
    if tributaries:
        d8[:line, 0::2] = 4
        d8[line + 2:, 1::2] = 64
    return d8


def corner_spiral(shape, corner, laps, tributaries=True):
    """A square spiral that runs inward, clockwise, around the grid point between the cells (R - 1, C - 1) and (R, C),
    ``corner`` = (R, C): lap k is the ring of cells k steps from the point, walked from its north-west corner east, south,
    west and north again, then one step east onto lap k - 1; the innermost lap ends in a pit.  Every lap crosses all four
    edges that meet at the point.  ``tributaries``: a few straight lines that join the outermost lap from all four sides."""
    nrow, ncol = shape
    (R, C), L = corner, laps
    assert R - L >= 0 and C - L >= 0 and R + L <= nrow and C + L <= ncol
    d8 = np.full(shape, NODATA, np.uint8)
    for k in range(L, 0, -1):
        d8[R - k, C - k:C + k - 1] = 1
        d8[R - k:R + k - 1, C + k - 1] = 4
        d8[R + k - 1, C - k + 1:C + k] = 16
        d8[R - k + 2:R + k, C - k] = 64
        d8[R - k + 1, C - k] = 1
    d8[R, C - 1] = 0
    if tributaries:
        for o in (-L + 1, -L // 2, L // 3, L - 2):
            d8[:R - L, C + o] = 4
            d8[R + L:, C + o] = 64
            d8[R + o, :C - L] = 1
            d8[R + o, C + L:] = 16
    return d8


def with_nodata_holes(d8, rng, p):
    """Nodata punched into ``d8`` with probability ``p`` per cell: edges are only removed (a cell that now points into
    nodata is a pit), so an acyclic raster stays acyclic."""
    out = d8.copy()
    out[rng.random(d8.shape) < p] = NODATA
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (shape, seed, pits, share of nodata).  The seeds are pinned: tests/test_winding_cases.py asserts on every tree from (130, 67)
# up that the directions are balanced and that the longest path enters some tile 4 times or more (some supertile twice on
# the two 2100-long shapes)
TREES = [((64, 64), 11, 1, 0.1), ((64, 64), 12, 3, 0.3), ((64, 64), 13, 40, 0.0),
         ((63, 65), 21, 1, 0.1), ((63, 65), 22, 3, 0.3), ((63, 65), 23, 40, 0.0),
         ((65, 63), 31, 1, 0.1), ((65, 63), 32, 3, 0.3), ((65, 63), 33, 40, 0.0),
         ((130, 67), 49, 1, 0.1), ((130, 67), 42, 3, 0.3), ((130, 67), 40, 40, 0.0),
         ((200, 511), 51, 1, 0.1), ((200, 511), 52, 3, 0.3), ((200, 511), 53, 40, 0.0),
         ((513, 520), 60, 1, 0.1), ((130, 2100), 70, 1, 0.1), ((2100, 130), 80, 1, 0.1)]
SPIRAL_LAPS = 24
_SPECS = {}


def _spec(name, family, make, **facts):
    assert name not in _SPECS
    _SPECS[name] = (family, make, facts)


def _dims(shape):
    return f"{shape[0]}x{shape[1]}"


for _shape, _seed, _pits, _p in TREES:
    _spec(f"tree_{_dims(_shape)}_p{_pits}", "tree", functools.partial(invasion_tree, _shape, _seed, _pits, _p), pits=_pits,
          p_nodata=_p)
for _shape in ((130, 200), (64, 64)):
    _spec(f"serp_tiles_{_dims(_shape)}", "serp_tiles", functools.partial(serp_tiles, *_shape))
for _shape, _axis in (((130, 200), 1), ((130, 200), 0), ((200, 130), 1), ((200, 130), 0), ((130, 2100), 1), ((130, 2100), 0)):
    _spec(f"serp_{'rows' if _axis else 'cols'}_{_dims(_shape)}", "serp_whole", functools.partial(serp_whole, *_shape, _axis),
          axis=_axis)
# the line on a tile edge, on a supertile edge, on a hypertile edge, and on the last row / column before a partial tile;
# line 64 of 130 rows is the edge between two row blocks (dist.block_rows(130, 2))
for _shape, _line in (((130, 300), 63), ((600, 700), 511), ((2100, 300), 2047), ((130, 300), 127), ((130, 300), 64)):
    _spec(f"river_r{_line}_{_dims(_shape)}", "edge_river", functools.partial(edge_river, _shape, 0, _line), axis=0, line=_line)
    if _line != 64:
        _spec(f"river_c{_line}_{_dims(_shape[::-1])}", "edge_river", functools.partial(edge_river, _shape[::-1], 1, _line), axis=1,
              line=_line)
for _shape, _corner in (((130, 131), (64, 64)), ((600, 600), (512, 512)), ((2100, 2100), (2048, 2048))):
    _spec(f"spiral_{_corner[0]}_{_dims(_shape)}", "corner_spiral", functools.partial(corner_spiral, _shape, _corner, SPIRAL_LAPS),
          corner=_corner, laps=SPIRAL_LAPS)
HOLED = {"tree_200x511_p1": 0.02, "serp_tiles_130x200": 0.01, "serp_rows_130x200": 0.01, "river_r63_130x300": 0.02,
         "spiral_64_130x131": 0.02}
for _i, (_base, _p) in enumerate(HOLED.items()):
    _family, _make, _facts = _SPECS[_base]
    _spec("holes_" + _base, _family,
          (lambda make, seed, p: lambda: with_nodata_holes(make(), np.random.default_rng(seed), p))(_make, 900 + _i, _p),
          holes=_p, base=_base)

NAMES = list(_SPECS)
TREE_NAMES = [n for n in NAMES if n.startswith("tree_")]
HUGE_SPIRAL = "spiral_2048_2100x2100"  # nearly all nodata: the integer operations only
# one case per family plus the (200, 511) and (130, 2100) trees
SUBSET = ["tree_130x67_p3", "tree_200x511_p1", "tree_130x2100_p1", "serp_tiles_130x200", "serp_cols_130x200", "river_c63_300x130",
          "spiral_64_130x131", "holes_tree_200x511_p1"]
# (case, numbers of row blocks) whose fixpoint sweeps are expected to settle, and the one that must be refused: the river of
# river_r64_130x300 crosses the edge between the two blocks of dist.block_rows(130, 2) at every step
ROW_BLOCKS = [("tree_200x511_p1", (2, 3)), ("river_r63_130x300", (2, 3)), ("river_r64_130x300", (2, 3)),
              ("serp_cols_200x130", (2, 3))]
REFUSED = ("river_r64_130x300", 2, 8)  # (case, row blocks, max_iter): refused with that bound, settles with a sufficient one
# the most block-edge crossings of one path (block_edge_crossings over dist.block_rows; tests/test_winding_cases.py measures
# them again).  The sweeps exchange boundary rows once per crossing; dist.MAX_ROUNDS is 256, so the two combinations above it
# are run with ``max_iter`` raised
ROW_BLOCK_CROSSINGS = {("tree_200x511_p1", 2): 12, ("tree_200x511_p1", 3): 27, ("river_r63_130x300", 2): 1,
                       ("river_r63_130x300", 3): 1, ("river_r64_130x300", 2): 299, ("river_r64_130x300", 3): 1,
                       ("serp_cols_200x130", 2): 130, ("serp_cols_200x130", 3): 260}
OVER_MAX_ROUNDS = {("river_r64_130x300", 2), ("serp_cols_200x130", 3)}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case ``name``: name, family, shape, d8 (read-only) and the facts it was built with."""
    family, make, facts = _SPECS[name]
    d8 = np.ascontiguousarray(make(), dtype=np.uint8)
    d8.setflags(write=False)
    return SimpleNamespace(name=name, family=family, shape=d8.shape, n=d8.size, d8=d8, **facts)
