"""Randomised parity of the operations test_gpu_fuzz.py leaves out: upstream_area in area units, upstream_sum, ucat_area,
floodplains and snap, on the same uniformly random D8 rasters (cycles, flow into nodata and off the raster, shapes around
the tile edges), each raster once on a lat/lon transform whose row areas differ and once on a projected one.  The
references are the serial restatements of tests/serial_refs.py (pinned to the reference's recorded outputs by
tests/test_serial_refs.py) and the oracle's accuflux.  Every comparison is on dtype, shape and bytes.

The generators (``gen_*`` / ``*_cases``) need no GPU: tests/test_serial_refs.py runs them with the serial references over all
seeds and asserts that the edges these kernels can get wrong really occur in the inputs.

snap on a cycle: the reference's walk never returns from a cycle when no mask cell and no ``max_length`` stops it; the
library answers such a walk after n + 1 hops.  That answer has no counterpart, so it is deliberately not asserted: starts
on or behind a cycle are drawn only for calls with a finite ``max_length``."""
import itertools
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from serial_refs import (_ref_floodplains, _ref_snap, _ref_step_length_f64, _ref_ucat_area,  # noqa: E402
                         _ref_upstream_sum)
from test_gpu_fuzz import SHAPES, random_d8  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = range(len(SHAPES) * 2)
SEED_BASE = 7022
LL_TRANSFORM = (0.05, 0.0, -20.0, 0.0, -0.05, 64.0)  # 1030 rows reach from 64N to 12.5N: every row has its own cell area
UCAT_K = (1, 63, 64, 65, 300)
UCAT_2D = {63: (7, 9), 64: (8, 8), 65: (5, 13), 300: (15, 20)}
SNAP_K = (1, 64, 65, 200)
UPA_VALUES, UPA_P, UPA_MIN = (1, 16, 81, 256, 625), (0.45, 0.25, 0.2, 0.06, 0.04), 256  # a tenth of the cells are streams


def transforms():
    from oracle import golden_inputs as GI

    return (("ll", LL_TRANSFORM, True), ("pr", GI.PROJ_TRANSFORM, False))


def raster_case(O, seed):
    """The random raster of a seed and its graph from the oracle."""
    rng = np.random.default_rng(SEED_BASE + seed)
    shape = SHAPES[seed % len(SHAPES)]
    d8 = random_d8(rng, shape, p_nodata=rng.choice([0.0, 0.1, 0.4]), p_pit=rng.choice([0.002, 0.05]),
                   coherent=rng.choice([0, 4, 2, 1, -1, -1]))
    idxs_ds, idxs_pit, _ = O.from_array(d8)
    assert idxs_pit.size  # (random_d8 always leaves a pit)
    seq = O.idxs_seq(idxs_ds, idxs_pit)
    nodata = idxs_ds == -1
    in_seq = np.zeros(d8.size, bool)
    in_seq[seq] = True
    assert np.array_equal(~in_seq & ~nodata, O.rank(idxs_ds)[0] == -1)  # (off the sequence: on or behind a cycle, or into nodata)
    return SimpleNamespace(seed=seed, shape=shape, n=d8.size, d8=d8, idxs_ds=idxs_ds, idxs_pit=idxs_pit, seq=seq, mv=-1,
                           nodata=nodata, in_seq=in_seq, offseq=~in_seq & ~nodata,
                           rng=lambda op: np.random.default_rng([SEED_BASE + seed, op]))


def area_flat(c, tag, unit):
    """The reference's area operand: ones for cells, else ``FlwdirRaster.area.ravel() / AREA_FACTORS[unit]`` (float64 on
    lat/lon grids, float32 on projected ones; the host grid is pinned by test_host_logic.py)."""
    from pyflwdir_amd import gis
    from pyflwdir_amd._affine import Affine

    if unit == "cell":
        return np.ones(c.n, np.int32)
    tr, latlon = {t: (a, ll) for t, a, ll in transforms()}[tag]
    with warnings.catch_warnings():  # (one row: the mean of no latitude steps is NaN, in the reference as well)
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.ascontiguousarray(gis.area_grid(Affine(*tr), c.shape, latlon, unit="m2").ravel() / gis.AREA_FACTORS[unit])


def upstream_area_expected(O, c, tag, unit):
    out = O.accuflux(c.idxs_ds, c.seq, area_flat(c, tag, unit), nodata=-9999)
    out[c.nodata] = -9999
    return out


# ---- upstream_sum ---------------------------------------------------------------------------------------------------------
def upstream_sum_cases(c):
    """(label, data, mv): five dtypes per seed; the missing value of each cycles over -9999, 0 and one that never compares
    equal (0.5 for integers, NaN for floats).  A fifth of the cells hold the missing value (or, where no element can hold
    it, an ordinary -9999 / 0).  The integers sit where two or three inflows leave the dtype's range; the floats have
    full mantissas, so the order of the adds shows in the bits."""
    rng = c.rng(1)
    out = []
    for j, dt in enumerate((np.int32, np.int64, np.uint32, np.float32, np.float64)):
        dt = np.dtype(dt)
        mv = (-9999, 0, 0.5 if dt.kind in "iu" else float("nan"))[(c.seed + j) % 3]
        if dt == np.int32:
            data = rng.integers(2**30 - 2**20, 2**30, c.n)
        elif dt == np.int64:
            data = rng.integers(2**62 - 2**40, 2**62, c.n)
        elif dt == np.uint32:
            data = rng.integers(2**31 - 2**20, 2**31 + 2**20, c.n)
        else:
            data = rng.standard_normal(c.n) * 1000
        data = data.astype(dt)
        holds = mv in (-9999, 0) and not (dt.kind == "u" and mv < 0)
        data[rng.random(c.n) < 0.2] = mv if holds else (0 if dt.kind == "u" else -9999)
        out.append((f"{dt.name}_mv{mv}", data, mv))
    return out


# ---- ucat_area ------------------------------------------------------------------------------------------------------------
def gen_outlets(c):
    """The outlet list of a seed (idxs_ds.dtype, ``mv`` for missing): k from UCAT_K clipped to the raster; random cells
    plus a missing entry, an outlet on a nodata cell, a pit, two outlets on one flow path with one directly upstream of the
    other, a cell off the sequence (where the raster has these), and a cell with upstream cells repeated at both ends."""
    rng = c.rng(2)
    k = min(UCAT_K[c.seed % len(UCAT_K)], c.n)
    out = rng.integers(0, c.n, k)
    specials = [[c.mv]]
    if c.nodata.any():
        specials.append([rng.choice(np.flatnonzero(c.nodata))])
    specials.append([rng.choice(c.idxs_pit)])
    links = c.seq[c.idxs_ds[c.seq] != c.seq]  # cells of the sequence with a downstream cell
    if links.size:
        u = rng.choice(links)
        specials.append([u, c.idxs_ds[u]])
    if c.offseq.any():
        specials.append([rng.choice(np.flatnonzero(c.offseq))])
    r = (c.seed // len(UCAT_K)) % len(specials)  # (a short list takes a different special first from seed to seed)
    flat = list(itertools.chain.from_iterable(specials[r:] + specials[:r]))
    inner = np.arange(1, k - 1) if k >= 3 else np.arange(k)
    pos = rng.permutation(inner)[:len(flat)]
    out[pos] = flat[:pos.size]
    if k >= 3:
        out[0] = out[k - 1] = rng.choice(c.idxs_ds[links]) if links.size else rng.integers(0, c.n)
    out = out.astype(c.idxs_ds.dtype)
    if k in UCAT_2D and c.seed % 2:
        out = out.reshape(UCAT_2D[k])
    return out


def ucat_cases(c):
    """(label, tag, unit, idxs_out): the seed's list in cells and in both float units, and a list of missing values."""
    io = gen_outlets(c)
    none = np.full(5, c.mv, c.idxs_ds.dtype)
    return [("cell", "ll", "cell", io), ("km2", "ll", "km2", io), ("ha", "pr", "ha", io), ("none_cell", "pr", "cell", none),
            ("none_km2", "ll", "km2", none)]


def ucat_expected(c, tag, unit, idxs_out):
    m, a = _ref_ucat_area(idxs_out.ravel(), c.idxs_ds, c.seq, area_flat(c, tag, unit), c.mv)
    return m.reshape(c.shape), a.reshape(idxs_out.shape)


# ---- floodplains ----------------------------------------------------------------------------------------------------------
def floodplain_cases(c):
    """(uparea, upa_min, [(label, elevtn, b)]).  ``uparea`` is no accumulation: random values whose square roots are exact,
    -9999 on nodata, streams (>= upa_min) anywhere, also upstream of cells that are none.  Elevations are small integers, so
    that dh == h0 occurs; as float32, as float64, and as float64 ``int * 1.000001`` (no float32 holds these) on a base of 0, 700
    or 1000: 16 steps up, dh is 16.000016 before the drain elevation is rounded, and near 700 and 1000 float32 rounds some
    elevations up by more than those 16e-6, so that the rounding alone admits the cell.  A few elevations are NaN."""
    rng = c.rng(3)
    upa = rng.choice(UPA_VALUES, c.n, p=UPA_P).astype(np.float32 if c.seed % 2 else np.float64)
    upa[c.nodata] = -9999
    ints = rng.integers(0, 40, c.n)
    nan = rng.random(c.n) < max(0.002, 1.5 / c.n)
    base = (0, 700, 1000)[c.seed % 3]

    def elev(a):
        a = a.copy()
        a[nan] = np.nan
        return a

    return upa, UPA_MIN, [("f32_b05", elev(ints.astype(np.float32)), 0.5), ("f64_b05", elev(ints.astype(np.float64)), 0.5),
                          ("f64x_b03", elev((ints + base) * 1.000001), 0.3), ("f64x_b05", elev((ints + base) * 1.000001), 0.5)]


# ---- snap -----------------------------------------------------------------------------------------------------------------
def main_upstream(O, c):
    upa = O.accuflux(c.idxs_ds, c.seq, np.ones(c.n, np.int32), nodata=-9999)
    upa[c.nodata] = -9999
    return O.main_upstream(c.idxs_ds, upa)


def snap_calls(c):
    """Every combination of unit and transform x direction x mask x max_length, as dicts.  k starts from SNAP_K: cell 0, the
    last cell, a pit, a nodata cell, a duplicate and random cells.  Without ``max_length`` the starts come from cells that
    reach a pit and from nodata cells only (everything upstream of such a cell reaches a pit as well, so the walks of both
    directions end); with a finite one from all cells, cycles included.  ``idxs`` is int64 in one call and idxs_ds.dtype in
    the next."""
    from pyflwdir_amd import gis

    rng = c.rng(4)
    k = SNAP_K[c.seed % len(SNAP_K)]
    safe = np.flatnonzero(c.in_seq | c.nodata)
    every = np.arange(c.n)
    fixed = [0, c.n - 1, int(rng.choice(c.idxs_pit))] + ([int(rng.choice(np.flatnonzero(c.nodata)))] if c.nodata.any() else [])
    rand5 = rng.random(c.n) < 0.05
    calls = []
    for unit, tag, tr, latlon in [("cell", "ll", LL_TRANSFORM, True)] + [("m", t, a, ll) for t, a, ll in transforms()]:
        if unit == "cell":
            lengths = [None, 0, 1, 2.5, 7]
        else:
            lengths = [None, 3.7 * float(np.median(gis.step_length_table(c.shape[0], latlon, tr, dtype=np.float64)))]
        for direction, mask_kind, max_length in itertools.product(("down", "up"), ("none", "rand5", "false", "starts"), lengths):
            pool = safe if max_length is None else every
            idxs = rng.choice(pool, k)
            mine = [x for x in fixed if max_length is not None or c.in_seq[x] or c.nodata[x]]
            r = len(calls) % len(mine)
            mine = mine[r:] + mine[:r]
            pos = rng.permutation(k)[:len(mine)]
            idxs[pos] = mine[:pos.size]
            if k >= 2:
                idxs[rng.integers(1, k)] = idxs[0]
            idxs = idxs.astype(np.int64 if len(calls) % 2 == 0 else c.idxs_ds.dtype)
            mask = {"none": None, "rand5": rand5, "false": np.zeros(c.n, bool)}.get(mask_kind)
            if mask_kind == "starts":
                mask = np.zeros(c.n, bool)
                mask[idxs] = True
            calls.append(dict(tag=tag, transform=tr, latlon=latlon, unit=unit, direction=direction, mask_kind=mask_kind,
                              mask=mask, max_length=max_length, idxs=idxs))
    return calls


def snap_expected(c, call, main, memo):
    nxt = c.idxs_ds if call["direction"] == "down" else main
    if call["unit"] == "cell":
        step = lambda a, b: 1.0  # noqa: E731
    else:
        lengths = memo.setdefault(call["tag"], {})
        ncol, latlon, tr = c.shape[1], call["latlon"], call["transform"]

        def step(a, b):
            if (a, b) not in lengths:
                lengths[(a, b)] = _ref_step_length_f64(a, b, ncol, latlon, tr)
            return lengths[(a, b)]

    mask = None if call["mask"] is None else call["mask"].tolist()
    return _ref_snap(call["idxs"], nxt, c.mv, mask, call["max_length"], step)


# ---- the device against them ----------------------------------------------------------------------------------------------
def same(got, exp):
    return got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


def rasters(c, **kw):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    return {tag: pyflwdir.from_array(c.d8, ftype="d8", transform=Affine(*tr), latlon=latlon, cache=False, **kw)
            for tag, tr, latlon in transforms()}


@pytest.mark.parametrize("seed", SEEDS)
def test_upstream_area_units(gpu_lib, oracle, seed):
    """km2 on the lat/lon grid (float64 sums) and ha on the projected one (float32 sums) against the oracle's accuflux of
    the area grid, -9999 on nodata."""
    c = raster_case(oracle, seed)
    flw = rasters(c)
    assert np.array_equal(flw["ll"].idxs_ds, c.idxs_ds) and np.array_equal(flw["ll"].idxs_seq, c.seq)
    for tag, unit, dt in (("ll", "km2", np.float64), ("pr", "ha", np.float32)):
        exp = upstream_area_expected(oracle, c, tag, unit).reshape(c.shape)
        assert exp.dtype == dt
        assert same(flw[tag].upstream_area(unit), exp), (tag, unit)


@pytest.mark.parametrize("seed", SEEDS)
def test_upstream_sum(gpu_lib, oracle, seed):
    c = raster_case(oracle, seed)
    flw = rasters(c)["ll"]
    for label, data, mv in upstream_sum_cases(c):
        exp = _ref_upstream_sum(c.idxs_ds, data, mv, c.mv).reshape(c.shape)
        got = flw.upstream_sum(data.reshape(c.shape), mv=mv)
        assert same(got, exp), (label, np.flatnonzero(got.ravel() != exp.ravel())[:5])


@pytest.mark.parametrize("seed", SEEDS)
def test_ucat_area(gpu_lib, oracle, monkeypatch, seed):
    c = raster_case(oracle, seed)
    cases = [(label, tag, unit, io) + ucat_expected(c, tag, unit, io) for label, tag, unit, io in ucat_cases(c)]
    for engine in ("exact", "levels"):
        if engine == "levels":
            monkeypatch.setenv("PFD_EXACT_LEVELS", "1")
        flw = rasters(c)
        for label, tag, unit, io, exp_map, exp_are in cases:
            if engine == "levels" and unit == "cell":
                continue  # (the float sums are what walks the engine's sequence)
            m, a = flw[tag].ucat_area(io, unit=unit)
            assert same(m, exp_map), (engine, label, np.flatnonzero(m.ravel() != exp_map.ravel())[:5])
            assert same(a, exp_are), (engine, label, np.flatnonzero(a.ravel() != exp_are.ravel())[:5])


@pytest.mark.parametrize("seed", SEEDS)
def test_floodplains(gpu_lib, oracle, monkeypatch, seed):
    c = raster_case(oracle, seed)
    upa, upa_min, variants = floodplain_cases(c)
    exps = [_ref_floodplains(c.idxs_ds, c.seq, elv, upa, upa_min, b).reshape(c.shape) for _, elv, b in variants]
    for engine in ("exact", "levels"):
        if engine == "levels":
            monkeypatch.setenv("PFD_EXACT_LEVELS", "1")
        flw = rasters(c)["ll"]
        for (label, elv, b), exp in zip(variants, exps):
            got = flw.floodplains(elv.reshape(c.shape), uparea=upa.reshape(c.shape), upa_min=upa_min, b=b)
            assert same(got, exp), (engine, label, np.flatnonzero(got.ravel() != exp.ravel())[:5])


@pytest.mark.parametrize("seed", SEEDS)
def test_snap(gpu_lib, oracle, seed):
    """See the module docstring for what is not asserted about cycles."""
    c = raster_case(oracle, seed)
    main = main_upstream(oracle, c)
    flw = rasters(c)
    assert np.array_equal(flw["ll"].idxs_us_main, main)
    memo = {}
    for call in snap_calls(c):
        exp_i, exp_d = snap_expected(c, call, main, memo)
        mask = None if call["mask"] is None else call["mask"].reshape(c.shape)
        got_i, got_d = flw[call["tag"]].snap(idxs=call["idxs"], mask=mask, max_length=call["max_length"], unit=call["unit"],
                                            direction=call["direction"])
        what = (call["tag"], call["unit"], call["direction"], call["mask_kind"], call["max_length"])
        assert got_i.dtype == call["idxs"].dtype and same(got_i, exp_i), (what, np.flatnonzero(got_i != exp_i)[:5])
        assert got_d.dtype == np.float32 and same(got_d, exp_d), (what, np.flatnonzero(got_d != exp_d)[:5])
