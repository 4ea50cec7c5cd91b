"""The cases of FlwdirRaster.upscale / upscale_error / ucat_outlets (tests/golden/wide_upscale.npz, written by
tools/gen_golden_upscale.py) and plain restatements of the seven functions of the reference they stand for
(pyflwdir/upscale.py: dmm_exitcell, dmm_nextidx, eam_repcell, eam_nextidx, ihu_outlets, ihu_nextidx, upscale_error),
written from their documented behaviour — shared by the generator (which runs the reference), tests/test_upscale_cases.py
(CPU) and tests/test_gpu_upscale.py (device).

A coarse cell of ``cellsize`` x ``cellsize`` fine cells gets
* a representative cell: among its valid fine cells that are a pit or inside the method's selector (DMM: the cells on the
  edge of the coarse cell; EAM: the effective area, a cross along the centre lines widened towards the centre), the one
  with the largest upstream area > 0; the serial loop visits the cells in ascending index and replaces on a strict ``>``,
  so among equal areas the smallest index stays;
* (EAM+) an outlet cell: the last cell inside the coarse cell on the way down from the representative cell;
* a downstream coarse cell, found by a walk down the fine network from that cell (one rule per method).
"""
from __future__ import annotations

import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ["dmm", "eam", "eam_plus"]
TIE = "twin_channels_8x12"  # built here (twin_channels_d8), not a golden raster
# (raster, uparea kind, cellsizes): "cell" int32 upstream cell count, "km2" float64, "f32" the float32 of km2
CASES = [
    ("flwdir_large", "cell", [20, 7, 3, 2, 1]),
    ("flwdir_large", "f32", [20, 7]),
    ("rhine", "km2", [5, 16]),
    ("synth_river_nodata_768x1024", "cell", [16]),
    ("synth_rough_nodata_384x512", "cell", [10]),
    ("synth_tiny_5x7", "cell", [2, 3, 8]),
    ("synth_onerow_1x300", "cell", [4]),
    ("synth_onecol_300x1", "cell", [4]),
    (TIE, "cell", [4]),
]
FULL = {"flwdir_large", "synth_tiny_5x7", "synth_onerow_1x300", "synth_onecol_300x1", TIE}  # outputs in full; else digests
CYCLIC = "synth_loops_96x80"  # refused by the front end: the walks would never end

# random rasters of tests/test_gpu_upscale.py (the generator of tests/test_gpu_fuzz.py, acyclic form): shapes for the
# kernels' edges — one row, one column, around the 64-lane wave and the 256-thread workgroup — and cell sizes on both
# sides of the 256-column strip that separates the two arg-max kernels, one larger than every raster
FUZZ_SHAPES = [(1, 300), (300, 1), (63, 65), (64, 64), (129, 257)]
FUZZ_CELLSIZES = [1, 2, 3, 7, 64, 65, 256, 257, 400]
FUZZ_SEED_BASE = 4400
# a random raster (south-west links kept) whose coarse network holds a loop: (shape, cellsize, seed, method)
LOOP_CASE = ((63, 65), 2, 39, "eam")
FUZZ_FLOAT = (1, 2, 4, 6, 8)  # positions in FUZZ_CELLSIZES whose rasters get float32 areas with NaN (odd seeds)


def twin_channels_d8():
    """An 8 x 12 raster for the tie rule at cellsize 4: two one-cell-wide channels along rows 0 and 3 run east side by
    side through the three coarse cells of the upper coarse row to pits in column 11, so in each of those coarse cells two
    edge cells (and two cells of the effective area) hold the same, largest upstream area; a third channel along row 5
    runs west to a pit, and everything else is nodata."""
    d8 = np.full((8, 12), 247, np.uint8)
    d8[0, :11], d8[0, 11] = 1, 0
    d8[3, :11], d8[3, 11] = 1, 0
    d8[5, 1:], d8[5, 0] = 16, 0
    return d8


def d8_of(raster):
    return twin_channels_d8() if raster == TIE else np.load(os.path.join(GOLD, raster + ".npz"))["d8"]


def transform_of(raster):
    """(six affine coefficients, latlon)"""
    if raster == TIE:
        return (0.01, 0.0, 5.0, 0.0, -0.01, 50.0), True
    with open(os.path.join(GOLD, "manifest.json")) as f:
        ent = json.load(f)[raster]
    return tuple(ent["transform"]), bool(ent["latlon"])


def uparea_of(flw, kind, cache=None):
    """The upstream area of a case on ``flw`` (the reference's FlwdirRaster or the device's)."""
    cache = {} if cache is None else cache
    if kind not in cache:
        if kind == "cell":
            cache[kind] = flw.upstream_area()
        elif kind == "km2":
            cache[kind] = flw.upstream_area("km2")
        else:
            cache[kind] = uparea_of(flw, "km2", cache).astype(np.float32)
    return cache[kind]


def keys():
    """Every recorded call: (key, raster, uparea kind, cellsize)."""
    return [(f"{r}_{u}_{c}", r, u, c) for r, u, cs in CASES for c in cs]


# ---- the serial loops, restated ------------------------------------------------------------------------------------------
def coarse_shape(shape, cellsize):
    return (-(-shape[0] // cellsize), -(-shape[1] // cellsize))


def edge_mask(cellsize):
    """[cellsize, cellsize] bool: the fine cells on the edge of a coarse cell (DMM selector)."""
    m = np.zeros((cellsize, cellsize), bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


def effarea_mask(cellsize, r_ratio=0.5):
    """[cellsize, cellsize] bool: the effective area (EAM selector).  With the distances ri, ci of a fine cell to the
    centre of its coarse cell: sqrt(ri) + sqrt(ci) <= sqrt(cellsize * r_ratio), or within half a cell of a centre line;
    in float64, element by element with Python floats like the reference's scalar function."""
    off = cellsize / 2.0 - 0.5
    lim = (cellsize * r_ratio) ** 0.5
    m = np.zeros((cellsize, cellsize), bool)
    for i in range(cellsize):
        ri = abs(i - off)
        for j in range(cellsize):
            ci = abs(j - off)
            m[i, j] = (ri ** 0.5 + ci ** 0.5) <= lim or ri <= 0.5 or ci <= 0.5
    return m


class Grid:
    """The fine raster, the coarse grid over it and the per-cell selector values."""

    def __init__(self, ds, shape, cellsize, mv):
        self.ds, self.mv, self.cs = np.asarray(ds), mv, int(cellsize)
        self.nrow, self.ncol = shape
        self.shape1 = coarse_shape(shape, cellsize)
        self.n1 = self.shape1[0] * self.shape1[1]
        self.r, self.c = np.divmod(np.arange(self.ds.size, dtype=np.int64), self.ncol)
        self.coarse = (self.r // self.cs) * self.shape1[1] + self.c // self.cs
        self.valid = self.ds != mv
        self.pit = self.valid & (self.ds == np.arange(self.ds.size))
        self._sel = {}

    def selector(self, kind):
        if kind not in self._sel:
            m = edge_mask(self.cs) if kind == "edge" else effarea_mask(self.cs)
            self._sel[kind] = m[self.r % self.cs, self.c % self.cs]
        return self._sel[kind]

    def in_d8(self, i0, i1):
        n = self.shape1[1]
        return abs(i1 % n - i0 % n) <= 1 and abs(i1 // n - i0 // n) <= 1


def rep_cells(g, upa, kind, scan=False):
    """Representative (``kind`` "effarea") / exit (``kind`` "edge") cell per coarse cell, ``mv`` where there is none.
    ``scan``: the literal serial scan; else the same rule — largest area > 0, smallest index among equals — by a sort."""
    upa = np.asarray(upa).ravel()
    cand = g.valid & (g.pit | g.selector(kind))
    rep = np.full(g.n1, g.mv, g.ds.dtype)
    if scan:
        best = np.zeros(g.n1, upa.dtype)
        for i in np.flatnonzero(cand):
            k = g.coarse[i]
            if upa[i] > best[k]:
                best[k], rep[k] = upa[i], i
        return rep
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(cand & (upa > 0))
    order = np.lexsort((idx, -upa[idx].astype(np.float64), g.coarse[idx]))  # (float64 holds every int32 / float32 exactly)
    idx = idx[order]
    first = np.ones(idx.size, bool)
    first[1:] = g.coarse[idx[1:]] != g.coarse[idx[:-1]]
    rep[g.coarse[idx[first]]] = idx[first]
    return rep


def tied_cells(g, upa, kind):
    """Number of coarse cells in which two or more candidates share the largest upstream area."""
    upa = np.asarray(upa).ravel()
    rep = rep_cells(g, upa, kind)
    cand = np.flatnonzero(g.valid & (g.pit | g.selector(kind)))
    has = rep[g.coarse[cand]] != g.mv
    cand = cand[has]
    top = upa[rep[g.coarse[cand]]] == upa[cand]
    return int(np.count_nonzero(np.bincount(g.coarse[cand[top]], minlength=g.n1) > 1))


def ihu_outlets(g, rep):
    """From the representative cell downstream to the last cell inside the coarse cell (or a pit)."""
    out = np.full(g.n1, g.mv, g.ds.dtype)
    for i0 in np.flatnonzero(rep != g.mv):
        s = int(rep[i0])
        while True:
            s1 = int(g.ds[s])
            if s1 == s or g.coarse[s1] != i0:
                break
            s = s1
        out[i0] = s
    return out


def dmm_nextidx(g, rep):
    """The exit cell is followed until it is outside the coarse cell AND outside a window of one coarse cell's size
    that is shifted by half a cell towards the quadrant the exit cell lies in; the coarse cell of the last cell inside."""
    ds1 = np.full(g.n1, g.mv, g.ds.dtype)
    half = g.cs / 2
    for i0 in np.flatnonzero(rep != g.mv):
        s = int(rep[i0])
        i = i0
        dr = (int(g.r[s]) % g.cs) // half
        dc = (int(g.c[s]) % g.cs) // half
        r_mid = (i0 // g.shape1[1] + dr) * g.cs - 0.5
        c_mid = (i0 % g.shape1[1] + dc) * g.cs - 0.5
        while True:
            s1 = int(g.ds[s])
            if s1 == s:
                break
            if g.coarse[s1] != i0 and (abs(g.r[s] - r_mid) > half or abs(g.c[s] - c_mid) > half):
                break
            s, i = s1, int(g.coarse[s1])
        ds1[i0] = i
    return ds1


def eam_nextidx(g, rep):
    """To the first cell of another coarse cell's effective area, or to the pit: that cell's coarse cell."""
    ds1 = np.full(g.n1, g.mv, g.ds.dtype)
    ea = g.selector("effarea")
    for i0 in np.flatnonzero(rep != g.mv):
        s = int(rep[i0])
        while True:
            s1 = int(g.ds[s])
            if s1 == s or (g.coarse[s1] != i0 and ea[s1]):
                break
            s = s1
        ds1[i0] = g.coarse[s1]
    return ds1


def ihu_nextidx(g, out, stats=None):
    """To the next outlet cell (or pit) downstream: its coarse cell where that is one of the 8 neighbours (or the cell
    itself), else the coarse cell of the first effective area passed on the way (``stats["fallback"]`` lists those)."""
    ds1 = np.full(g.n1, g.mv, g.ds.dtype)
    ea = g.selector("effarea")
    for i0 in np.flatnonzero(out != g.mv):
        s, target = int(out[i0]), None
        while True:
            s1 = int(g.ds[s])
            i1 = int(g.coarse[s1])
            if out[i1] == s1 or s1 == s:
                if g.in_d8(i0, i1):
                    target = s1
                elif stats is not None:
                    stats.setdefault("fallback", []).append(int(i0))
                break
            if target is None and ea[s1]:
                target = s1
            s = s1
        if target is None:
            raise IndexError(f"coarse cell {i0}: no outlet within the 8 neighbours and no effective area downstream")
        ds1[i0] = g.coarse[target]
    return ds1


def upscale(ds, upa, shape, cellsize, method, mv, stats=None):
    """(coarse idxs_ds, fine idxs_out) of one method."""
    g = Grid(ds, shape, cellsize, mv)
    if method == "dmm":
        out = rep_cells(g, upa, "edge")
        return dmm_nextidx(g, out), out
    rep = rep_cells(g, upa, "effarea")
    if method == "eam":
        return eam_nextidx(g, rep), rep
    out = ihu_outlets(g, rep)
    return ihu_nextidx(g, out, stats), out


def ucat_outlets(ds, upa, shape, cellsize, method, mv):
    g = Grid(ds, shape, cellsize, mv)
    return rep_cells(g, upa, "edge") if method == "dmm" else ihu_outlets(g, rep_cells(g, upa, "effarea"))


def upscale_error(ds, out, ds1, mv):
    """uint8 per coarse cell: 1 where the first outlet cell (or pit) downstream of its outlet cell is the outlet cell of
    its downstream coarse cell, 0 where not, 255 where it has no outlet or no downstream cell."""
    flag = np.zeros(np.asarray(ds).size, bool)
    flag[out[out != mv]] = True
    res = np.full(out.size, 255, np.uint8)
    for i0 in np.flatnonzero((out != mv) & (ds1 != mv)):
        s = int(out[i0])
        while True:
            s1 = int(ds[s])
            if flag[s1] or s1 == s:
                res[i0] = 1 if s1 == out[ds1[i0]] else 0
                break
            s = s1
    return res


def network_valid(ds1, mv):
    """True if no cell of a coarse network is on or above a loop (pointer doubling: after round k a cell knows whether
    its path ends within 2**k steps).  A path may also end in a cell without data — a coarse cell none of whose candidates
    has an area > 0, NaN areas for instance, that another cell's walk ends in: the reference accepts such a network."""
    own = np.arange(ds1.size)
    p = np.where(ds1 == mv, own, ds1).astype(np.int64)
    ok = p == own
    for _ in range(max(1, int(ds1.size).bit_length())):
        ok = ok | ok[p]
        p = p[p]
    return bool(np.all(ok))


def far_links(ds1, shape1, mv):
    """Number of coarse links that leave the 8 neighbours."""
    i = np.flatnonzero(ds1 != mv)
    j = ds1[i].astype(np.int64)
    return int(np.count_nonzero((np.abs(j // shape1[1] - i // shape1[1]) > 1) | (np.abs(j % shape1[1] - i % shape1[1]) > 1)))


def fuzz_cases():
    """(shape, cellsize, seed) of the random rasters, one raster each: on every shape the cell sizes that leave more than
    one coarse cell, the one larger than every raster, and the one that is exactly the raster.  (A single coarse cell is no
    raster: the reference's constructor raises ValueError, and so does ours; ucat_outlets answers all the same.)"""
    out = []
    for i, s in enumerate(FUZZ_SHAPES):
        for j, c in enumerate(FUZZ_CELLSIZES):
            n1 = coarse_shape(s, c)[0] * coarse_shape(s, c)[1]
            if n1 > 1 or c == FUZZ_CELLSIZES[-1] or (c, c) == s:
                out.append((s, c, 2 * (i * len(FUZZ_CELLSIZES) + j) + (j in FUZZ_FLOAT)))
    return out


def fuzz_raster(random_d8, shape, seed, cellsize=None):
    """(d8, uparea maker): an acyclic random raster (links E / SE / S / SW) with 20-30 % nodata.  At cell sizes 2 and 3
    nearly every such raster upscales to a network with a loop — two coarse cells side by side whose cells drain into
    each other, east above and south-west below — and the call is refused like in the reference; so that the walks and not
    only the refusal are tested there, those rasters have SW turned into S (row and column never decrease along a path:
    no loop in any coarse network).  ``areas(cells)`` turns the upstream cell count into the case's area: thirds of the
    count (many equal values, ties at the maximum of a coarse cell included), int32 on even seeds, float32 with a sprinkle
    of NaN on odd ones — a coarse cell whose candidates all hold NaN has no data, and other cells may drain into it."""
    rng = np.random.default_rng([FUZZ_SEED_BASE, shape[0], shape[1], seed])
    d8 = random_d8(rng, shape, p_nodata=rng.choice([0.2, 0.25, 0.3]), p_pit=rng.choice([0.002, 0.02]), coherent=-1)
    if cellsize in (2, 3):
        d8[d8 == 8] = 4

    def areas(cells):
        upa = np.where(cells > 0, cells // 3 + 1, cells).astype(np.int32)
        if seed % 2:
            upa = upa.astype(np.float32)
            upa[np.random.default_rng([FUZZ_SEED_BASE, seed]).random(upa.size) < 0.03] = np.nan
        return upa

    return d8, areas


class HostGraph:
    """What the restated loops need of a raster, from the CPU oracle (no device): downstream links, missing value and
    ``upstream_area`` — the oracle's accumulation over the reference's cell order, in area units over the host's area grid
    (pinned to the reference by tests/test_host_logic.py); the digests in the record say that these are the areas the
    reference was run with."""

    def __init__(self, d8, transform=(1.0, 0.0, 0.0, 0.0, -1.0, 0.0), latlon=False):
        from oracle import oracle as O

        O.build()
        self.O, self.shape = O, d8.shape
        self.transform, self.latlon = transform, latlon
        self.idxs_ds, self.idxs_pit, _ = O.from_array(d8)
        self.mv = -1
        self.seq = O.idxs_seq(self.idxs_ds, self.idxs_pit)

    @property
    def acyclic(self):
        return self.seq.size == np.count_nonzero(self.idxs_ds != self.mv)

    def upstream_area(self, unit="cell"):
        from pyflwdir_amd import gis
        from pyflwdir_amd._affine import Affine

        if unit == "cell":
            w = np.ones(self.idxs_ds.size, np.int32)
        else:
            w = np.ascontiguousarray(gis.area_grid(Affine(*self.transform), self.shape, self.latlon, unit="m2").ravel()
                                     / gis.AREA_FACTORS[unit])
        out = self.O.accuflux(self.idxs_ds, self.seq, w, nodata=-9999)
        out[self.idxs_ds == self.mv] = -9999
        return out.reshape(self.shape)
