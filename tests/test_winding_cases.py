"""The rasters of tests/winding_cases.py have the properties tests/test_gpu_winding.py relies on — checked without a GPU, with
the C oracle (from_array, rank, idxs_seq) and numpy: acyclic, D8 codes only, a pit; the random trees use all eight directions
alike and their longest paths come back to tiles and supertiles they have left; every structured raster does the one thing it
is built for; and the row-block cases cross their block edges as often as the GPU test assumes.  These are conditions on
the inputs, on pinned seeds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import winding_cases as WC  # noqa: E402
from test_gpu_fuzz import SHAPES as OLD_SHAPES, random_d8  # noqa: E402


def graph(O, c):
    idxs_ds, idxs_pit, nvalid = O.from_array(c.d8)
    return idxs_ds, idxs_pit, nvalid, O.rank(idxs_ds)[0]


def longest_path(O, c):
    """The cells of the longest path, its head taken from the oracle's rank."""
    idxs_ds, _, _, rank = graph(O, c)
    return WC.path_from(idxs_ds.astype(np.int64), int(np.argmax(rank)))


@pytest.mark.parametrize("name", WC.NAMES)
def test_case_is_an_acyclic_d8_raster(oracle, name):
    c = WC.case(name)
    idxs_ds, idxs_pit, nvalid, rank = graph(oracle, c)
    assert c.d8.dtype == np.uint8 and np.isin(c.d8, WC.D8_VALUES).all()
    assert idxs_pit.size >= 1
    valid = idxs_ds != -1
    assert nvalid == valid.sum() == (c.d8 != WC.NODATA).sum()
    assert not (rank[valid] == -1).any()  # no cell on or behind a cycle
    assert oracle.idxs_seq(idxs_ds, idxs_pit).size == nvalid
    # the numpy restatements the other tests of this file measure with
    ds = WC.downstream(c.d8)
    assert np.array_equal(ds, idxs_ds)
    assert np.array_equal(WC.hops(ds)[valid], rank[valid])


@pytest.mark.parametrize("name", WC.TREE_NAMES)
def test_random_trees_wind(oracle, name):
    """All eight directions within 8 % .. 17 % of the links; the longest path enters some tile 4 times or more, and on the
    two 2100-long shapes some supertile twice.  (Measured: 489 hops and one tile entered 4 times at (130, 67) with one pit;
    1747 hops, 44 tile visits over 20 tiles at (200, 511); 3410 hops, 60 tile visits, one supertile entered twice at
    (130, 2100); 5894 hops, 159 tile visits, one tile entered 8 times, 13 supertile visits over 5 at (2100, 130).)"""
    c = WC.case(name)
    ds = WC.downstream(c.d8)
    pits = np.flatnonzero(ds == np.arange(c.n))
    assert pits.size >= c.pits and {0, 255} & set(c.d8.ravel()[pits].tolist())
    if c.pits > 1:
        assert {0, 255} <= set(c.d8.ravel()[pits].tolist())  # both pit codes
    assert ((c.d8 == WC.NODATA).mean() > 0) == (c.p_nodata > 0)
    if c.n < 130 * 67:
        return
    shares = WC.direction_shares(c.d8)
    assert shares.min() >= 0.08 and shares.max() <= 0.17, shares
    path = longest_path(oracle, c)
    assert WC.visits(path, c.shape, WC.TS)[2] >= 4, WC.visits(path, c.shape, WC.TS)
    if max(c.shape) == 2100:
        assert WC.visits(path, c.shape, WC.SUPER)[2] >= 2, WC.visits(path, c.shape, WC.SUPER)


@pytest.mark.parametrize("name", ["serp_tiles_130x200", "serp_tiles_64x64"])
def test_serp_tiles_has_the_longest_in_tile_path(oracle, name):
    c = WC.case(name)
    ds = WC.downstream(c.d8)
    assert WC.longest_in_box_path(ds, c.shape) == WC.TS * WC.TS - 1 == 4095
    assert graph(oracle, c)[3].max() == 4095
    assert WC.most_entries(ds, c.shape) == 1  # no path leaves its tile


@pytest.mark.parametrize("name", [n for n in WC.NAMES if n.startswith("serp_rows") or n.startswith("serp_cols")])
def test_serp_whole_is_one_path(oracle, name):
    c = WC.case(name)
    idxs_ds, idxs_pit, nvalid, rank = graph(oracle, c)
    assert idxs_pit.size == 1 and nvalid == c.n and rank.max() == c.n - 1
    path = longest_path(oracle, c)
    assert path.size == c.n and path[0] == 0
    # every edge across the path's direction is crossed once per row (column)
    nlines, length = (c.shape[0], c.shape[1]) if c.axis == 1 else (c.shape[1], c.shape[0])
    for edge in (WC.TS, WC.SUPER):
        for line in range(edge - 1, length - 1, edge):
            assert WC.crossings(path, c.shape, c.axis, line) == nlines
    if name == "serp_cols_130x2100":  # 2 horizontal tile edges x 2100 columns on one path
        assert WC.visits(path, c.shape, WC.TS, axis=0)[0] == 2 * 2100 + 1  # (visits to bands of tile rows)
    if name == "serp_rows_130x2100":  # 4 supertile edges x 130 rows on one path
        assert WC.visits(path, c.shape, WC.SUPER)[0] == 4 * 130 + 1


@pytest.mark.parametrize("name", [n for n in WC.NAMES if n.startswith("river_")])
def test_edge_river_crosses_its_line_at_every_step(oracle, name):
    c = WC.case(name)
    ds = WC.downstream(c.d8)
    length = c.shape[1 - c.axis]
    head = c.line * c.shape[1] if c.axis == 0 else c.line  # the river's first cell: index 0 along the line
    path = WC.path_from(ds, head)
    assert path.size == length and WC.crossings(path, c.shape, c.axis, c.line) == length - 1
    # the longest path is a tributary and then the river from where it joins
    long = longest_path(oracle, c)
    assert WC.crossings(long, c.shape, c.axis, c.line) >= length - 2


@pytest.mark.parametrize("name", [n for n in WC.NAMES if n.startswith("spiral_")])
def test_corner_spiral_enters_each_tile_once_per_lap(oracle, name):
    c = WC.case(name)
    ds = WC.downstream(c.d8)
    (R, C), L = c.corner, c.laps
    path = WC.path_from(ds, (R - L) * c.shape[1] + (C - L))  # from the outermost lap's first cell
    assert path.size == sum(8 * k - 4 for k in range(1, L + 1))
    edges = [e for e in (WC.TS, WC.SUPER, WC.HYPER) if R % e == 0 and C % e == 0]
    assert edges[0] == WC.TS
    for edge in edges:
        box = WC._boxes(c.shape, edge)[path]
        starts = np.concatenate([[True], box[1:] != box[:-1]])
        ids, counts = np.unique(box[starts], return_counts=True)
        assert ids.size == 4 and counts.tolist() == [L] * 4, (edge, counts)
        assert WC.most_entries(ds, c.shape, edge) == L
    # every entry into a tile goes through another perimeter slot
    box = WC._boxes(c.shape, WC.TS)[path]
    entries = path[1:][box[1:] != box[:-1]]
    assert np.unique(entries).size == entries.size == 4 * L - 1
    long = longest_path(oracle, c)  # a tributary, then every lap
    assert np.isin(path[1:], long).all()


def test_holes_only_remove_edges(oracle):
    for name, p in WC.HOLED.items():
        base, holed = WC.case(name), WC.case("holes_" + name)
        punched = (holed.d8 == WC.NODATA) & (base.d8 != WC.NODATA)
        assert 0.5 * p < punched.sum() / (base.d8 != WC.NODATA).sum() < 2 * p
        assert np.array_equal(holed.d8[~punched], base.d8[~punched])
        a, b = WC.downstream(base.d8), WC.downstream(holed.d8)
        kept = b >= 0
        assert np.all((b[kept] == a[kept]) | (b[kept] == np.flatnonzero(kept)))  # a link stays or becomes a pit
        assert (b == np.arange(b.size)).sum() > (a == np.arange(a.size)).sum()


def test_half_of_the_cases_come_back_to_a_tile(oracle):
    """Among the cases the exact-engine sweeps run on (all but the nearly empty (2100, 2100) spiral), at least half have a
    path that enters some tile more than once, and at least half a path that comes back to a BAND OF TILE ROWS it has left —
    what ``random_d8(..., coherent=-1)`` cannot have (the next test)."""
    names = [n for n in WC.NAMES if n != WC.HUGE_SPIRAL]
    tiles = bands = 0
    for name in names:
        c = WC.case(name)
        ds = WC.downstream(c.d8)
        tiles += WC.most_entries(ds, c.shape) > 1
        bands += WC.most_entries(ds, c.shape, axis=0) > 1
    assert 2 * tiles >= len(names), (tiles, len(names))
    assert 2 * bands >= len(names), (bands, len(names))


def test_the_old_acyclic_generator_never_comes_back_to_a_row_band():
    """``random_d8(..., coherent=-1)`` of tests/test_gpu_fuzz.py, the generator of every other random acyclic raster of the
    suite: the row never decreases along a path, so NO path comes back to a band of tile rows, a supertile row or a row block
    it has left, and no in-tile path is longer than 127 links.  It does come back to a TILE, across a vertical edge only (E out
    of the tile, SW back in one row further down: measured up to 9 entries at (1030, 90)) — each return costs the path a row,
    so a tile is entered 64 times at the most and always through its east or west side."""
    for i, shape in enumerate(OLD_SHAPES):
        for p_nodata, p_pit in ((0.0, 0.002), (0.1, 0.05), (0.4, 0.002)):
            d8 = random_d8(np.random.default_rng(5000 + i), shape, p_nodata, p_pit, -1)
            ds = WC.downstream(d8)
            assert (WC.hops(ds)[ds >= 0] >= 0).all()
            r = np.arange(d8.size) // shape[1]
            assert (r[ds[ds >= 0]] >= r[ds >= 0]).all()  # the row never decreases
            for edge in (WC.TS, WC.SUPER):
                assert WC.most_entries(ds, shape, edge, axis=0) == 1
            assert WC.longest_in_box_path(ds, shape) <= 2 * WC.TS - 1
            for nb in (2, 3):
                if shape[0] >= nb:
                    assert WC.block_edge_crossings(ds, shape, _block_rows(shape[0], nb)) <= nb - 1


def _block_rows(nrow, nb):
    from pyflwdir_amd import dist

    return dist.block_rows(nrow, nb)


def test_row_block_cases_cross_their_edges_as_often_as_assumed():
    """The float sweeps over row blocks exchange boundary rows once per block-edge crossing of the longest path: the cases
    expected to settle under the default stay below dist.MAX_ROUNDS — all but two, which the GPU test runs with ``max_iter``
    raised (stated here so that it does not find out): the column boustrophedon in three blocks crosses 2 edges x 130 columns
    = 260 times, and the river on the edge between two blocks crosses it 299 times — far above the ``max_iter`` of 8 it must
    be refused with."""
    from pyflwdir_amd import dist

    assert dist.MAX_ROUNDS == 256
    seen = {}
    for name, nbs in WC.ROW_BLOCKS:
        c = WC.case(name)
        ds = WC.downstream(c.d8)
        for nb in nbs:
            seen[name, nb] = k = WC.block_edge_crossings(ds, c.shape, dist.block_rows(c.shape[0], nb))
            assert k == WC.ROW_BLOCK_CROSSINGS[name, nb], (name, nb, k)
            assert (k >= dist.MAX_ROUNDS) == ((name, nb) in WC.OVER_MAX_ROUNDS), (name, nb, k)
    assert seen["serp_cols_200x130", 3] == 260 and seen["river_r64_130x300", 2] == 299
    name, nb, max_iter = WC.REFUSED
    c = WC.case(name)
    rows = dist.block_rows(c.shape[0], nb)
    assert rows[0][1] == c.line + 1  # the river's line IS the edge between the blocks
    assert WC.block_edge_crossings(WC.downstream(c.d8), c.shape, rows) == c.shape[1] - 1 == 299 > max_iter
    # the river of the settling case lies inside one block for either number of blocks
    c = WC.case("river_r63_130x300")
    for nb in (2, 3):
        assert all(not (r0 == c.line + 1) for r0, _ in dist.block_rows(c.shape[0], nb))
