"""Rasters, correct results and mutations shared by tests/test_local_equations.py (CPU: the restatement sees every
mutation) and tests/test_gpu_verifiers.py (GPU: the device verifiers count what the restatement counts).

Mutation classes (one ``Mut`` each): M1 one cell at a named position, M2 a compensating pair on two tributaries of one
confluence, M3 a consistent shift (only the cell where the shift starts breaks its equation), M4 nodata cells, M5 float
bit patterns (-0.0, NaN payloads), M6 an input changed with the result left alone."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

import local_equations as LE
from serial_refs import _ref_down, _ref_up

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODES = np.array([1, 2, 4, 8, 16, 32, 64, 128, 0, 255, 247], np.uint8)

RASTERS = ["tiny_5x7", "onerow_1x300", "onecol_300x1", "synth_64x64", "synth_63x65", "synth_130x70", "rand_63x65",
           "rand_130x70", "tall_32771x70"]
_cache = {}


@dataclass
class Mut:
    cls: str
    label: str
    args: dict
    expect: object = None         # the exact set of valid cells that must be flagged (flat indices), where the class states one
    expect_nodata: object = None  # M4: the number of nodata cells that must be flagged, with no valid cell flagged
    at_least: int = 1             # the restatement's count is at least this (0 only where the contract says "equal")
    pit_sum_moves: bool = False
    expect_count: object = None   # row blocks: the exact count, where the class states one


class Solved:
    def __init__(self, O, d8):
        self.d8 = np.ascontiguousarray(d8, dtype=np.uint8)
        self.shape = self.d8.shape
        self.n = self.d8.size
        self.idxs_ds, self.idxs_pit, self.n_valid = O.from_array(self.d8)
        self.seq = O.idxs_seq(self.idxs_ds, self.idxs_pit)
        assert self.seq.size == self.n_valid, "the generated rasters are acyclic"
        self.g = LE.Graph(self.idxs_ds, self.shape)
        self.upa = O.upstream_area_cell(self.d8)[0].ravel()


class Cyclic:
    """A raster with cycles for restate_whole: the graph alone (the oracle's sequence leaves the cycles out)."""

    def __init__(self, d8, idxs_ds, shape):
        self.d8, self.shape, self.g = d8, tuple(shape), LE.Graph(idxs_ds, shape)


def random_acyclic_d8(rng, shape, p_nodata, p_pit):
    """The acyclic generator of tests/test_gpu_fuzz.py (``random_d8(..., coherent=-1)``): uniformly random codes with the
    four upward directions replaced by E / SE / S / SW, so that (row, column) strictly increases along a path."""
    n = shape[0] * shape[1]
    p_dir = (1.0 - p_nodata - p_pit) / 8
    d8 = rng.choice(CODES, size=n, p=[p_dir] * 8 + [p_pit / 2, p_pit / 2, p_nodata]).reshape(shape)
    dirs = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=n).reshape(shape)
    d8 = np.where(np.isin(d8, [16, 32, 64, 128]), dirs, d8)
    if not np.isin(d8, [0, 255]).any():
        d8.flat[rng.integers(0, n)] = 0
    return np.ascontiguousarray(d8, dtype=np.uint8)


def open_up(d8, seed, p_nodata=0.03):
    """oracle.synth_d8 ends every path at the border in a pit code and keeps its nodata in large patches: here every second
    border pit points off the raster instead, and single nodata cells are sprinkled in (the cells that drained into them
    now point into nodata).  Edges are only removed, so the raster stays acyclic."""
    d8 = d8.copy()
    nrow, ncol = d8.shape
    rng = np.random.default_rng(seed)
    d8[(rng.random(d8.shape) < p_nodata)] = 247
    for sl, code in (((0, slice(None)), 64), ((nrow - 1, slice(None)), 4), ((slice(None), 0), 16), ((slice(None), ncol - 1), 1)):
        edge = d8[sl]
        pits = np.flatnonzero(edge == 0)[::2]
        edge[pits] = code
    return d8


def raster(O, name) -> Solved:
    if name in _cache:
        return _cache[name]
    if name in ("tiny_5x7", "onerow_1x300", "onecol_300x1"):
        d8 = np.load(os.path.join(GOLD, "synth_" + name + ".npz"))["d8"]
    else:
        kind, dims = name.split("_")
        nrow, ncol = (int(v) for v in dims.split("x"))
        if kind == "rand":
            d8 = random_acyclic_d8(np.random.default_rng(nrow * 1000 + ncol), (nrow, ncol), 0.1, 0.02)
        else:  # all eight directions, interior pits, nodata
            d8 = open_up(O.synth_d8(nrow, ncol, seed=nrow + ncol, tilt=100000, white=2, nodata_pct=10 if kind == "synth" else 5),
                         nrow)
    _cache[name] = Solved(O, d8)
    return _cache[name]


def leaves_raster(d8):
    """(cells whose code points off the raster, cells whose code points into nodata)."""
    nrow, ncol = d8.shape
    r, c = np.divmod(np.arange(d8.size).reshape(d8.shape), ncol)
    off = np.zeros(d8.shape, bool)
    into = np.zeros(d8.shape, bool)
    for (dr, dc), code in LE.D8_CODE.items():
        rr, cc = r + dr, c + dc
        outside = (rr < 0) | (rr >= nrow) | (cc < 0) | (cc >= ncol)
        sel = d8 == code
        off |= sel & outside
        tgt = np.where(outside, 0, rr * ncol + cc)
        into |= sel & ~outside & (d8.ravel()[tgt] == 247)
    return off, into


def _prefer_late(R, cand):
    """Of the candidate cells the last one that lies in the partial column block (column >= 64) and — on a raster of more
    than 32768 rows — in the second or later stride iteration of the whole-raster verifiers; the last one otherwise."""
    cand = np.asarray(cand)
    if cand.size == 0:
        return None
    nrow, ncol = R.shape
    r, c = np.divmod(cand, ncol)
    for sel in ((c >= 64) & (r >= 32768), (r >= 32768), (c >= 64)):
        if sel.any():
            return int(cand[sel][-1])
    return int(cand[-1])


def named_cells(R) -> dict:
    """The positions of class M1 (None where the raster has no such cell)."""
    g = R.g
    nrow, ncol = R.shape
    mid_r, mid_c = nrow // 2, ncol // 2
    at = lambda r, c: r * ncol + c if 0 <= r < nrow and 0 <= c < ncol else None
    first = lambda sel: int(np.flatnonzero(sel)[0]) if sel.any() else None
    nup = g.n_upstream()
    names = dict(corner_nw=at(0, 0), corner_ne=at(0, ncol - 1), corner_sw=at(nrow - 1, 0), corner_se=at(nrow - 1, ncol - 1),
                 col63=at(mid_r, 63), col64=at(mid_r, 64), last_col=at(mid_r, ncol - 1), last_row=at(nrow - 1, mid_c),
                 row32767=at(32767, ncol - 2), row32768=at(32768, ncol - 3), tall_last_row=at(nrow - 1, ncol - 2) if nrow > 32768 else None,
                 pit=_prefer_late(R, np.flatnonzero(g.pit)), headwater=_prefer_late(R, np.flatnonzero(g.valid & ~g.pit & (nup == 0))),
                 confluence3=_prefer_late(R, np.flatnonzero(nup >= 3)))
    nodata2 = (~g.valid).reshape(R.shape)
    near = np.zeros(R.shape, bool)
    for dr, dc in LE.NEIGHBOURS:
        near |= LE._shifted(nodata2, dr, dc, False)
    names["next_to_nodata"] = first(near.ravel() & g.valid)
    step = g.ds - g.idx
    for (dr, dc), code in LE.D8_CODE.items():
        k = int(code).bit_length() - 1
        sel = g.valid & ~g.pit & (step == dr * ncol + dc) & (g.ds % ncol - g.idx % ncol == dc)
        names[f"drains_{k}"] = _prefer_late(R, np.flatnonzero(sel))
    return names


def _m1_cells(R):
    seen, out = set(), []
    for name, x in named_cells(R).items():
        if x is not None and x not in seen:
            seen.add(x)
            out.append((name, int(x)))
    return out


def _path_to_pit(R, x):
    ds = R.idxs_ds
    path = [int(x)]
    while int(ds[path[-1]]) != path[-1]:
        path.append(int(ds[path[-1]]))
    return np.array(path)


def _nodata_cells(R):
    nd = np.flatnonzero(~R.g.valid)
    return nd[np.unique(np.linspace(0, nd.size - 1, 3).astype(int))] if nd.size else nd


# ---------------------------------------------------------------------------------------------
# whole-raster verifiers: upa, labels, HAND
# ---------------------------------------------------------------------------------------------
def _label_inputs(O, R):
    """Seeds: every pit but one (its basin keeps 0) and a few interior cells (nested basins)."""
    g = R.g
    pits = R.idxs_pit.astype(np.int64)
    keep = pits if pits.size < 2 else np.delete(pits, pits.size // 2)
    inner = [x for x in (named_cells(R)["confluence3"], _prefer_late(R, np.flatnonzero(g.valid & ~g.pit & (R.upa >= 4))))
             if x is not None]
    outlets = np.unique(np.concatenate([keep, np.array(inner, np.int64)]))
    ids = (np.arange(outlets.size, dtype=np.uint32) * 3 + 2).astype(np.uint32)
    lab = O.basins(R.idxs_ds, outlets.astype(R.idxs_ds.dtype), R.seq, ids)
    return dict(outlets=outlets, ids=ids, lab=lab)


def _hand_inputs(O, R, dtype, integer=False, nan_at=None):
    rng = np.random.default_rng(R.n)
    if integer:
        elev = rng.integers(0, 60, R.n).astype(dtype)
    elif dtype == np.float32:
        elev = (rng.random(R.n) * 100).astype(np.float32)
    else:
        elev = rng.random(R.n) * 100  # (53-bit fractions: a difference taken in float32 would give other bits)
    if nan_at is not None:
        elev[nan_at] = np.nan
    thr = 3 if R.n > 200 else 2
    drain = (R.upa >= thr).astype(np.uint8)
    if nan_at is not None:
        drain[nan_at] = 0
    hand = O.height_above_nearest_drain(R.idxs_ds, R.seq, drain, elev)
    return dict(drain=drain, elev=elev, hand=hand)


def restate_whole_maps(R, op, a):
    if op == "upa":
        return LE.upa_cell(R.g, a["upa"])
    if op == "labels":
        return LE.labels(R.g, a["outlets"], a["ids"], a["lab"])
    return LE.hand(R.g, a["drain"], a["elev"], a["hand"])


def restate_whole(R, op, a):
    """What the device verifier of ``op`` must report for these arguments (the keys of _hip's verify_* results)."""
    if op == "upa":
        return LE.upa_cell_stats(R.g, a["upa"])
    if op == "labels":
        return LE.labels_stats(R.g, a["outlets"], a["ids"], a["lab"])
    return LE.hand_stats(R.g, a["drain"], a["elev"], a["hand"])


def _with(base, **changes):
    a = dict(base)
    a.update(changes)
    return a


def _set(arr, cells, values):
    out = arr.copy()
    out[cells] = values
    return out


def whole_raster_cases(O, R, op):
    key = (id(R), op)
    if key not in _cache:
        _cache[key] = {"upa": _upa_cases, "labels": _label_cases}.get(op, _hand_cases)(O, R, op)
    return _cache[key]


def _upa_cases(O, R, op):
    g, upa = R.g, R.upa
    base = dict(upa=upa)
    muts = []
    for name, x in _m1_cells(R):
        cand = _set(upa, x, upa[x] + 1)
        if g.valid[x]:
            muts.append(Mut("M1", name, dict(upa=cand), expect={x, int(g.down[x])}))
        else:
            muts.append(Mut("M1", name, dict(upa=cand), expect_nodata=1))
    nup = g.n_upstream()
    c = _prefer_late(R, np.flatnonzero(nup >= 2))
    if c is not None:
        t = np.flatnonzero(g.ds == c)
        t = t[t != c][:2]
        muts.append(Mut("M2", "pair", dict(upa=_set(upa, t, upa[t] + np.array([3, -3], np.int32))), expect=set(t.tolist())))
    h = named_cells(R)["headwater"]
    if h is not None:
        path = _path_to_pit(R, h)
        muts.append(Mut("M3", "path", dict(upa=_set(upa, path, upa[path] + 5)), expect={h}, pit_sum_moves=True))
    nd = _nodata_cells(R)
    if nd.size:
        muts.append(Mut("M4", "nodata", dict(upa=_set(upa, nd, np.arange(nd.size, dtype=np.int32))), expect_nodata=int(nd.size)))
    return base, muts


def _label_cases(O, R, op):
    g = R.g
    base = _label_inputs(O, R)
    lab, outlets, ids = base["lab"], base["outlets"], base["ids"]
    muts = []
    for name, x in _m1_cells(R):
        cand = _set(lab, x, lab[x] + 1)
        if g.valid[x]:
            muts.append(Mut("M1", name, _with(base, lab=cand)))
        else:
            muts.append(Mut("M1", name, _with(base, lab=cand), expect_nodata=1))
    # M3: a whole basin under another id: only its seed objects
    j = int(np.flatnonzero(outlets == _prefer_late(R, outlets))[0])
    muts.append(Mut("M3", "basin", _with(base, lab=np.where(lab == ids[j], np.uint32(ids.max() + 9), lab)), expect={int(outlets[j])}))
    unseeded = np.setdiff1d(R.idxs_pit.astype(np.int64), outlets)
    if unseeded.size:  # the basin that holds 0 under an id: only its pit objects
        muts.append(Mut("M3", "unseeded", _with(base, lab=np.where(g.valid & (lab == 0), np.uint32(ids[0]), lab)),
                        expect={int(unseeded[0])}))
    nd = _nodata_cells(R)
    if nd.size:
        muts.append(Mut("M4", "nodata", _with(base, lab=_set(lab, nd, 7)), expect_nodata=int(nd.size)))
    # M6: one seed's id changed, the labels left alone
    muts.append(Mut("M6", "seed_id", _with(base, ids=_set(ids, j, ids[j] + 1)), expect={int(outlets[j])}))
    return base, muts


def _hand_cases(O, R, op):
    g = R.g
    dtype = np.float32 if op == "hand_f32" else np.float64
    base = _hand_inputs(O, R, dtype)
    drain, hand = base["drain"], base["hand"]
    muts = []
    for name, x in _m1_cells(R):
        if g.valid[x]:
            muts.append(Mut("M1", name, _with(base, hand=_set(hand, x, np.nextafter(hand[x], np.inf)))))
        else:
            muts.append(Mut("M1", name, _with(base, hand=_set(hand, x, np.nextafter(hand[x], np.inf))), expect_nodata=1))
    # M3: integer-valued elevations (every sum exact); the cells that drain to one drain cell D without passing another
    # drain cell move up by 1.0: only the cells directly upstream of D object
    ib = _hand_inputs(O, R, dtype, integer=True)
    dcells = np.flatnonzero(ib["drain"] == 1)
    feeds = np.flatnonzero(g.valid & ~g.pit & (ib["drain"] == 0) & (ib["drain"][g.down] == 1))
    D = _prefer_late(R, np.unique(g.down[feeds]))
    if D is not None:
        near = O.basins(R.idxs_ds, dcells.astype(R.idxs_ds.dtype), R.seq, np.arange(1, dcells.size + 1, dtype=np.uint32))
        mine = np.flatnonzero(g.valid & (near == near[D]) & (g.idx != D))
        muts.append(Mut("M3", "subtree", _with(ib, hand=_set(ib["hand"], mine, ib["hand"][mine] + 1.0)),
                        expect=set(feeds[g.down[feeds] == D].tolist())))
    nd = _nodata_cells(R)
    if nd.size:
        muts.append(Mut("M4", "nodata", _with(base, hand=_set(hand, nd, 0.0)), expect_nodata=int(nd.size)))
    # M5: -0.0 on a drain cell; a NaN under another payload where a NaN belongs (equal by the contract of checks.hip)
    d0 = _prefer_late(R, np.flatnonzero(g.valid & ~g.pit & (drain == 1)))
    if d0 is not None:
        muts.append(Mut("M5", "minus_zero", _with(base, hand=_set(hand, d0, -0.0))))
        # M6: the drain flag dropped, or set to a value that is not 1, with the heights left alone
        muts.append(Mut("M6", "drain_flag", _with(base, drain=_set(drain, d0, 0))))
        muts.append(Mut("M6", "drain_flag_2", _with(base, drain=_set(drain, d0, 2))))
    c = named_cells(R)["headwater"]
    if c is not None:
        nb = _hand_inputs(O, R, dtype, nan_at=c)
        assert np.isnan(nb["hand"][c])
        other = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
        muts.append(Mut("M5", "nan_base", nb, at_least=0))
        muts.append(Mut("M5", "nan_payload", _with(nb, hand=_set(nb["hand"], c, other)), at_least=0))
        muts.append(Mut("M5", "nan_gone", _with(nb, hand=_set(nb["hand"], c, 1.0)), expect={c}))
        muts.append(Mut("M6", "elevation", _with(base, elev=_set(base["elev"], c, base["elev"][c] + dtype(1.0))), expect={c}))
    return base, muts


# ---------------------------------------------------------------------------------------------
# row blocks
# ---------------------------------------------------------------------------------------------
BLOCK_OPS = ["accu_up_f32_nd", "accu_up_f32", "accu_up_f64", "accu_up_f64_nd", "accu_up_i32_nd", "accu_up_i32", "accu_up_i64",
             "accu_up_i64_nd", "accu_up_f32_rows", "accu_up_f32_rows_nd", "accu_down_f32_nd", "accu_down_f64", "accu_down_i32_nd",
             "accu_down_i64", "fill_up_f32", "fill_down_max_f32", "fill_down_min_i32", "fill_down_sum_f32", "strahler",
             "strahler_mask", "dist_cells", "dist_cells_mask", "dist_m", "dist_m_mask", "classic", "classic_mask", "flood_f32", "flood_f64"]


def block_raster(O) -> Solved:
    if "blocks" not in _cache:
        d8 = open_up(O.synth_d8(500, 400, seed=91, tilt=20000, white=2, nodata_pct=5), 91, p_nodata=0.04)
        _cache["blocks"] = Solved(O, d8)
    return _cache["blocks"]


class Block:
    """Rows of block ``b`` of ``nblocks``: own rows [r0, r1), one halo row towards every neighbour, device rows [a, e)."""

    def __init__(self, B, nblocks, b):
        nrow, self.ncol = B.shape
        self.r0, self.r1 = (b * nrow) // nblocks, ((b + 1) * nrow) // nblocks
        self.halo = (1 if b > 0 else 0, 1 if b + 1 < nblocks else 0)
        self.a, self.e = self.r0 - self.halo[0], self.r1 + self.halo[1]
        self.own_rows = self.r1 - self.r0
        self.n_own = self.own_rows * self.ncol
        self.lo, self.hi = self.r0 * self.ncol, self.r1 * self.ncol      # own cells, whole-raster indices
        self.off = self.a * self.ncol                                    # whole-raster index of the block's first cell

    def rows(self, whole):
        """The block's device rows of a whole-raster array (a copy)."""
        w = np.asarray(whole)
        return np.ascontiguousarray(w.reshape(-1, self.ncol)[self.a:self.e]).ravel().copy()

    def seed_of(self, whole):
        """The halo seeds the neighbouring blocks' final rows give: [top halo row, bottom halo row], zeros where none."""
        w = np.asarray(whole).reshape(-1, self.ncol)
        s = np.zeros((2, self.ncol), w.dtype)
        if self.halo[0]:
            s[0] = w[self.a]
        if self.halo[1]:
            s[1] = w[self.e - 1]
        return s.ravel()


def flood_state(idxs_ds, seq, elevtn, is_stream, stream_h):
    """dem.floodplains (dem.py:333-379) keeping its three arrays: one FLOOD_STATE record per cell."""
    n = idxs_ds.size
    z = np.full(n, -9999.0, np.float32)
    h = np.full(n, -9999.0, np.float32)
    f = np.full(n, -1, np.int32)
    f[seq] = 0
    ds = idxs_ds.tolist()
    stream = np.asarray(is_stream).astype(bool).tolist()
    with np.errstate(invalid="ignore", over="ignore"):
        for x in seq.tolist():
            if stream[x]:
                h[x], z[x], f[x] = stream_h[x], elevtn[x], 1
            elif f[ds[x]] == 1:
                z0, h0 = z[ds[x]], h[ds[x]]
                if elevtn[x] - z0 <= h0:
                    f[x], z[x], h[x] = 1, z0, h0
    st = np.zeros(n, LE.FLOOD_STATE)
    st["z"], st["h"], st["flag"] = z, h, f
    return st


def _block_op(O, B, op):
    """(inputs: name -> whole-raster array, correct whole-raster result, restatement(g, inputs, out), by_row names)."""
    key = ("blockop", id(B), op)
    if key in _cache:
        return _cache[key]
    g, n = B.g, B.n
    nrow, ncol = B.shape
    rng = np.random.default_rng(len(op) * 7 + 1)
    mask = (rng.random(n) < 0.6).astype(np.uint8)
    kind = op.split("_")
    if kind[0] == "accu":
        dtype = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i64": np.int64}[kind[2]]
        nd = -9999 if "nd" in kind else None
        rows = "rows" in kind
        if rows:
            data = (rng.random(nrow) * 3).astype(dtype)
        elif np.dtype(dtype).kind == "f":
            data = rng.integers(0, 9, n).astype(dtype) / dtype(8) if dtype == np.float32 else rng.random(n)  # (zeros among them)
        else:
            data = rng.integers(-5, 1000, n).astype(dtype) * (1 if dtype == np.int32 else 100003 * 1000003)
        if nd is not None:
            data[rng.random(data.size) < 0.05] = nd
        if kind[2] == "f32" and nd is not None and not rows:  # NaN payloads on isolated pits: no sum reads them, so no NaN propagates
            lone = np.flatnonzero(g.valid & g.pit & (g.n_upstream() == 0))
            if lone.size:
                data[lone[np.unique(np.linspace(0, lone.size - 1, 12).astype(int))]] = np.nan
        cell = np.repeat(data, ncol) if rows else data
        down = kind[1] == "down"
        out = O.accuflux(B.idxs_ds, B.seq, cell, nodata=nd if nd is not None else np.nan if np.dtype(dtype).kind == "f" else 2**70,
                         direction="down" if down else "up")
        fn = LE.accuflux_down if down else LE.accuflux_up
        res = (dict(data=data), out, lambda g, i, o: fn(g, i["data"], o, nodata=nd, by_row=rows), ("data",) if rows else ())
    elif kind[0] == "fill":
        up = kind[1] == "up"
        how = "max" if up else kind[2]
        if kind[-1] == "f32":
            data, nd = np.where(rng.random(n) < 0.4, np.float32(-9999), rng.integers(-8, 9, n).astype(np.float32) / 4), -9999.0
        else:
            data, nd = np.where(rng.random(n) < 0.4, 0, rng.integers(-5, 1000, n)).astype(np.int32), 0
        out = _ref_up(B.idxs_ds, B.seq, data, nd) if up else _ref_down(B.idxs_ds, B.seq, data, nd, how)
        fn = (lambda g, i, o: LE.fillnodata_up(g, i["data"], o, nd)) if up else (lambda g, i, o: LE.fillnodata_down(g, i["data"], o, nd, how))
        res = (dict(data=data), out, fn, ())
    elif kind[0] == "strahler":
        m = mask if "mask" in kind else None
        out = O.strahler_order(B.idxs_ds, B.seq, m)
        res = (dict(mask=m), out, lambda g, i, o: LE.strahler(g, o, i["mask"]), ())
    elif kind[0] == "dist":
        m = mask if "mask" in kind else None
        real = kind[1] == "m"
        tr = (1 / 120.0, 0.0, 5.0, 0.0, -1 / 120.0, 50.0)
        tab = O.step_length_table(nrow, True, tr) if real else None
        out = O.stream_distance(B.idxs_ds, B.seq, ncol, mask=m, real_length=real, latlon=True, transform=tr)
        res = (dict(mask=m, steps=tab), out, lambda g, i, o: LE.stream_distance(g, o, i["mask"], i["steps"]), ())
    elif kind[0] == "classic":
        m = mask if "mask" in kind else None
        main = O.main_upstream(B.idxs_ds, B.upa)
        out = O.stream_order_classic(B.idxs_ds, B.seq, main, m)
        res = (dict(tinfo=LE.trib_info(g, main, m), mask=m), out, lambda g, i, o: LE.classic_order(g, i["tinfo"], o, i["mask"]), ())
    else:
        elev = (rng.random(n) * 20).astype(np.float32) if kind[1] == "f32" else rng.random(n) * 20
        stream = (B.upa >= 20).astype(np.uint8)
        h = (B.upa.clip(0).astype(np.float64) ** 0.3).astype(np.float32)
        out = flood_state(B.idxs_ds, B.seq, elev, stream, h)
        res = (dict(elev=elev, stream=stream, h=h), out, lambda g, i, o: LE.floodplains_state(g, i["elev"], i["stream"], i["h"], o), ())
    _cache[key] = res
    return res


def _bump(op, arr, x):
    """Class M1's new value: +1 on integers, the next float, another flag on a floodplain record."""
    out = arr.copy()
    if arr.dtype == LE.FLOOD_STATE:
        out["flag"][x] = 1 - out["flag"][x]
    elif arr.dtype.kind == "f":
        out[x] = arr.dtype.type(1) if np.isnan(arr[x]) else np.nextafter(arr[x], arr.dtype.type(np.inf))
    else:
        with np.errstate(over="ignore"):
            out[x] = arr[x] + arr.dtype.type(1)
    return out


def block_cases(O, B, blk, op):
    """(base, mutations): ``args`` = dict(out=..., seed=..., inputs={name: block rows or per-row values})."""
    inputs, W, _, by_row = _block_op(O, B, op)
    g = B.g
    ncol = blk.ncol

    def block_input(name, whole):
        if whole is None:
            return None
        if name == "steps":
            return np.ascontiguousarray(whole[2 * blk.a:2 * (blk.e - 1) + 1])
        if name in by_row:
            return np.ascontiguousarray(whole[blk.a:blk.e])
        return blk.rows(whole)

    base = dict(out=blk.rows(W), seed=blk.seed_of(W), inputs={k: block_input(k, v) for k, v in inputs.items()})
    own = np.zeros(B.n, bool)
    own[blk.lo:blk.hi] = True
    nup = g.n_upstream()
    loc = lambda x: int(x) - blk.off  # whole-raster index -> index into the block's rows
    pick = lambda sel: (int(np.flatnonzero(sel & own)[len(np.flatnonzero(sel & own)) // 2]) if (sel & own).any() else None)
    cells = dict(first_own=blk.lo, last_own=blk.hi - 1, pit=pick(g.pit), headwater=pick(g.valid & ~g.pit & (nup == 0)),
                 confluence=pick(nup >= 2), first_valid=pick(g.valid))
    muts = []
    for name, x in cells.items():
        if x is None:
            continue
        if g.valid[x]:
            muts.append(Mut("M1", name, _with(base, out=_bump(op, base["out"], loc(x)))))
        else:  # (the row-block verifiers do not look at nodata cells)
            muts.append(Mut("M1", name, _with(base, out=_bump(op, base["out"], loc(x))), at_least=0, expect_count=0))
    ndc = np.flatnonzero(~g.valid & own)
    if ndc.size:  # M4
        muts.append(Mut("M4", "nodata", _with(base, out=_bump(op, base["out"], loc(ndc[ndc.size // 2]))), at_least=0, expect_count=0))
    out = base["out"]
    if out.dtype.kind == "f":  # M5: the row-block verifiers compare bit patterns
        zero = pick(g.valid & (LE._bits(np.asarray(W)) == 0))
        if zero is not None:
            muts.append(Mut("M5", "minus_zero", _with(base, out=_set(out, loc(zero), out.dtype.type(-0.0)))))
        nan = pick(g.valid & np.isnan(np.asarray(W)))
        if nan is not None:  # (an isolated pit: no other cell reads it)
            other = np.array([0x7FC00123], np.uint32).view(np.float32)[0] if out.dtype == np.float32 else \
                np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
            muts.append(Mut("M5", "nan_payload", _with(base, out=_set(out, loc(nan), other)), expect_count=1))

    def first_seen(label, cands, make):
        """Class M6: of the candidate cells the first whose change the restatement sees in an own cell (a raster too small
        to have a candidate goes without)."""
        if len(cands) == 0 and blk.halo == (0, 0) and B.n < 10000:
            return
        for x in cands[:64]:
            a = make(int(x))
            if restate_block(B, blk, op, a) >= 1:
                muts.append(Mut("M6", label, a))
                return
        raise AssertionError(f"{op}: no {label} change is visible in block rows {blk.r0}:{blk.r1}")

    mid = lambda sel: np.roll(np.flatnonzero(sel & own), -(int((sel & own).sum()) // 2))
    heads = mid(g.valid & ~g.pit & (nup == 0))
    ins = base["inputs"]
    with_input = lambda name, arr: _with(base, inputs=_with(ins, **{name: arr}))
    if ins.get("data") is not None:
        if "data" in by_row:
            first_seen("payload", heads, lambda x: with_input("data", _bump(op, ins["data"], x // ncol - blk.a)))
        else:
            first_seen("payload", heads, lambda x: with_input("data", _bump(op, ins["data"], loc(x))))
    for name in ("mask", "stream"):
        if ins.get(name) is not None:
            cands = heads
            if op.startswith("strahler"):
                # only out of the mask: a headwater taken INTO the mask would hold 0 inside it, which no run of the
                # reference's loop leaves there — the equation of the cell below it is not defined for such a value
                cands = heads[ins[name][heads - blk.off] == 1]
            first_seen(name, cands, lambda x: with_input(name, _set(ins[name], loc(x), 1 - ins[name][loc(x)])))
    if ins.get("tinfo") is not None:
        first_seen("tinfo", mid(nup >= 2), lambda x: with_input("tinfo", _set(ins["tinfo"], loc(x), ins["tinfo"][loc(x)] ^ 0x10)))
    if ins.get("elev") is not None:
        first_seen("elev", mid(g.valid & (np.asarray(W)["flag"] == 1) & (inputs["stream"] == 0)),
                   lambda x: with_input("elev", _set(ins["elev"], loc(x), ins["elev"][loc(x)] + 1000)))
    # a halo seed that own cells read: an up-sweep reads the halo cells that drain into the block, a down-sweep the halo
    # cells the block drains into
    halo = np.zeros(B.n, bool)
    if blk.halo[0]:
        halo[blk.off:blk.off + ncol] = True
    if blk.halo[1]:
        halo[(blk.e - 1) * ncol:blk.e * ncol] = True
    reads_up = op.startswith(("accu_up", "fill_down", "strahler"))
    used = np.flatnonzero(halo & g.valid & own[g.down]) if reads_up else np.unique(g.down[np.flatnonzero(own & g.valid & halo[g.down])])

    def seed_changed(x):
        r, c = divmod(x, ncol)
        s = (0 if (r == blk.a and blk.halo[0]) else ncol) + c
        seed = base["seed"]
        if seed.dtype == LE.FLOOD_STATE:
            new = _bump(op, seed, s)
        elif seed.dtype.kind == "f":
            new = _set(seed, s, seed[s] * 2 + 1)
        else:
            new = _set(seed, s, seed[s] + seed.dtype.type(3))
        return _with(base, seed=new)

    if blk.halo != (0, 0):
        first_seen("halo_seed", np.roll(used, -(used.size // 2)), seed_changed)

    def first_exact(cls, label, cands, make, count):
        """Of the candidate cells the first for which the restatement flags exactly ``count`` own cells: the classes that
        state their count (a raster too small to have such a cell goes without)."""
        for x in cands[:64]:
            a = make(int(x))
            if a is not None and restate_block(B, blk, op, a) == count:
                muts.append(Mut(cls, label, a, at_least=count, expect_count=count))
                return
        if B.n >= 10000:
            raise AssertionError(f"{op}: no {cls} {label} case in block rows {blk.r0}:{blk.r1}")

    def shifted(cells, delta):
        """The whole result with ``cells`` moved by ``delta``; the block's rows and its halo seeds are cut from it."""
        w = np.asarray(W).copy()
        with np.errstate(over="ignore"):
            w[cells] = w[cells] + w.dtype.type(delta)
        return _with(base, out=blk.rows(w), seed=blk.seed_of(w))

    kind = op.split("_")
    integer = out.dtype.kind in "iu"
    if kind[0] == "accu" and kind[1] == "up" and integer:
        # M2: +3 / -3 on two own tributaries of one own confluence: its sum holds, the two cells object
        def pair(c):
            t = np.flatnonzero(g.ds == c)
            t = t[(t != c) & own[t]][:2]
            return shifted(t, 0) if t.size < 2 else _with(base, out=_set(base["out"], t - blk.off, base["out"][t - blk.off] + np.array([3, -3], out.dtype)))

        first_exact("M2", "pair", mid(nup >= 2), pair, 2)
        # M3: +5 from a headwater down its path to the pit: only the headwater objects
        first_exact("M3", "path", heads, lambda h: shifted(_path_to_pit(B, h), 5), 1)
    if integer and (kind[0] in ("dist", "classic") or (kind[0] == "accu" and kind[1] == "down")):
        # M3 of a down-sweep: a cell and everything upstream of it moved alike: only that cell objects
        def subtree(x):
            lab = O.basins(B.idxs_ds, np.array([x], B.idxs_ds.dtype), B.seq, np.array([1], np.uint32))
            return shifted(np.flatnonzero(lab == 1), 1 if kind[0] == "classic" else 5)

        first_exact("M3", "subtree", mid(g.valid & ~g.pit & (nup >= 1)), subtree, 1)
    if op.startswith("strahler") and ins.get("mask") is not None:
        # a headwater taken INTO the mask holds 0 where 1 belongs; with no own cell below it, only it objects
        alone = mid(g.valid & (nup == 0) & (np.asarray(inputs["mask"]) == 0) & (g.pit | ~own[g.down]))
        first_exact("M6", "mask_in", alone, lambda x: with_input("mask", _set(ins["mask"], loc(x), 1)), 1)
    if ins.get("steps") is not None:
        # M6: the table entry of one own cell's step
        def step_entry(x):
            r0, r1 = x // ncol, int(g.down[x]) // ncol
            k = 1 if r0 == r1 else (0 if x % ncol == int(g.down[x]) % ncol else 2)
            t = ins["steps"].copy()
            t[r0 + r1 - 2 * blk.a, k] *= np.float32(2)
            return with_input("steps", t)

        first_seen("steps", mid(g.valid & ~g.pit), step_entry)
    return base, muts


def restate_block(B, blk, op, a):
    """Own cells of the block whose local equation fails, on the whole raster with the block's rows, seeds and inputs in place."""
    inputs, W, fn, by_row = _cache[("blockop", id(B), op)]
    ncol = blk.ncol
    whole = np.asarray(W).copy()
    whole[blk.off:blk.off + a["out"].size] = a["out"]
    if blk.halo[0]:
        whole[blk.off:blk.off + ncol] = a["seed"][:ncol]
    if blk.halo[1]:
        whole[(blk.e - 1) * ncol:blk.e * ncol] = a["seed"][ncol:]
    ins = {}
    for k, v in inputs.items():
        if v is None:
            ins[k] = None
            continue
        w = np.asarray(v).copy()
        if k == "steps":
            w[2 * blk.a:2 * (blk.e - 1) + 1] = a["inputs"][k]
        elif k in by_row:
            w[blk.a:blk.e] = a["inputs"][k]
        else:
            w[blk.off:blk.off + a["inputs"][k].size] = a["inputs"][k]
        ins[k] = w
    bad, _ = fn(B.g, ins, whole)
    return int(bad[blk.lo:blk.hi].sum())
