"""The golden cases of subbasins_area (tests/golden/wide_subbasins_area.npz, written by tools/
gen_golden_subbasins_area.py) and two restatements of the reference's loop (pyflwdir/basins.py:194-233) that import
nothing of the library: ``ref_serial``, the loop over the sequence as it stands, and ``ref_groups``, the form the device
runs — one short serial loop per parent cell, jobs in rounds.  Shared by the generator (which runs the reference),
tests/test_subbasins_area_cases.py (CPU) and tests/test_gpu_subbasins_area.py (device).

Both restatements compute on Python numbers: integer areas as ints, float64 areas as floats, float32 areas as floats that
hold float32 values, every difference rounded to float32 once (rounding the float64 difference of two float32 values to
float32 is the float32 difference: 53 >= 2 * 24 + 2 bits).  ``compare_form`` says where ``> area_min`` is evaluated, as
numpy >= 2 evaluates ``scalar > area_min``."""
from __future__ import annotations

import struct

import numpy as np

import basin_cases as BC

CORNER = BC.CORNER
RASTERS = ["synth_tiny_5x7", "synth_onerow_1x300", "synth_onecol_300x1", "flwdir0", "flwdir1", "synth_loops_96x80",
           "synth_river_256", "rhine", CORNER]
FULL = {"synth_tiny_5x7", "synth_onerow_1x300", "synth_onecol_300x1", "flwdir0", "flwdir1", CORNER}  # in full; else digests
LARGE = {"rhine", "synth_river_256"}  # fewer combinations: the serial loops of the CPU test are Python
# (transform, area): "own" is the raster's lat/lon transform, "south" a projected one; "cell" int32 cell counts, "km2"
# float64 (passed as uparea=None: the front end's default), "km2f" the same as float32
COMBOS = [("own", "cell"), ("own", "km2"), ("own", "km2f"), ("south", "km2"), ("south", "km2f")]
THRESHOLDS = ["zero", "neg", "huge", "big", "mid", "frac"]
SPECIAL_RASTERS = [CORNER, "flwdir1", "flwdir0"]
SPECIALS = ["equal", "nan", "nep50_weak", "nep50_strong", "cached", "np_int", "np_f32"]


def keys(raster):
    """Every record of one raster: (key, spec); spec = (transform, area, threshold) or ("special", name)."""
    out = []
    for tr, area in COMBOS:
        if raster in LARGE and tr == "south" and area == "km2f":
            continue
        for t in THRESHOLDS:
            if t == "frac" and area != "cell":  # a fractional threshold on integer areas
                continue
            if raster in LARGE and t in ("neg", "huge") and area != "cell":
                continue
            out.append((f"{raster}_{tr}_{area}_{t}", (tr, area, t)))
    if raster in SPECIAL_RASTERS:
        out += [(f"{raster}_special_{s}", ("special", s)) for s in SPECIALS]
    return out


# ---- numbers ---------------------------------------------------------------------------------------------------------
def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def compare_form(dtype, area_min):
    """("own" | "f64", area_min as a Python number): a Python number is weak (a float dtype compares in itself, an
    integer dtype with a float in float64), a numpy scalar is strong (the comparison is made in the common type)."""
    dtype = np.dtype(dtype)
    if not isinstance(area_min, (np.generic, np.ndarray)):
        if dtype.kind == "f" or isinstance(area_min, int):
            return "own", area_min
        return "f64", float(area_min)
    am = np.asarray(area_min)
    common = np.result_type(dtype, am.dtype)
    value = am.item()
    if common == dtype:
        return "own", value
    assert common == np.float64 or common.kind in "iu", common
    return "f64", value


def arith(dtype, area_min):
    """(sub, above): a - b rounded once in ``dtype``; x > area_min in the comparison type."""
    dtype = np.dtype(dtype)
    form, am = compare_form(dtype, area_min)
    if dtype.kind in "iu":
        bits = 8 * dtype.itemsize
        half = 1 << (bits - 1)

        def sub(a, b):
            return ((a - b + half) % (1 << bits)) - half  # (wraps like the dtype)
        return sub, (lambda x: x > am)  # (Python compares an int with a float exactly)
    if dtype == np.float64:
        am = float(am)
        return (lambda a, b: a - b), (lambda x: x > am)
    assert dtype == np.float32, dtype
    am = f32(float(am)) if form == "own" else float(am)
    return (lambda a, b: f32(a - b)), (lambda x: x > am)


def _fill(lab, dsl, seql):
    """core.fillnodata_upstream of the labels with nodata 0, as a uint32 array."""
    for x in seql:
        if lab[x] == 0:
            lab[x] = lab[dsl[x]]
    return np.array(lab, np.uint32)


# ---- the loop as it stands ---------------------------------------------------------------------------------------------
def ref_serial(ds, seq, usm, A, area_min, trace=None):
    """(uint32 map[n], outlet list) of the loop over the sequence.  ``trace`` (a list) receives (difference, area of the
    cell) of every non-pit cell."""
    A = np.asarray(A).ravel()
    sub, above = arith(A.dtype, area_min)
    a = A.tolist()
    carried = list(a)
    dsl, usl, seql = np.asarray(ds).tolist(), np.asarray(usm).tolist(), np.asarray(seq).tolist()
    lab, idxs = [0] * len(dsl), []
    for x in seql:
        y = dsl[x]
        if y == x:
            idxs.append(x)
            lab[x] = len(idxs)
            continue
        up, u = carried[y], a[x]
        rest = sub(up, u)
        if trace is not None:
            trace.append((rest, u))
        if above(rest) and above(u):
            tributary = usl[y] != x
            if tributary or not above(sub(a[y], u)):
                idxs.append(x)
                lab[x] = len(idxs)
                carried[x] = u
            if tributary:
                carried[y] = rest
                carried[usl[y]] = rest
        else:
            carried[x] = up
    return _fill(lab, dsl, seql), idxs


# ---- one group per parent, jobs in rounds ------------------------------------------------------------------------------
def children_csr(ds):
    """(offsets[n + 1], cells): the upstream cells of every cell in ascending linear index."""
    ds = np.asarray(ds).astype(np.int64)
    n = ds.size
    c = np.flatnonzero((ds >= 0) & (ds != np.arange(n)))
    c = c[np.argsort(ds[c], kind="stable")]
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, ds[c] + 1, 1)
    return np.cumsum(off).tolist(), c.tolist()


def ref_groups(ds, seq, usm, A, area_min, force_full=False):
    """(uint32 map[n], outlet list, info) of the per-group form.  info: mode (0 pruned / 1 full), rounds, jobs, steps,
    round_jobs (the jobs of every round), and what the groups met: trib_before_main, trib_after_main, two_tribs, kept,
    interbasin, nan."""
    A = np.asarray(A).ravel()
    sub, above = arith(A.dtype, area_min)
    a = A.tolist()
    dsl, usl, seql = np.asarray(ds).tolist(), np.asarray(usm).tolist(), np.asarray(seq).tolist()
    n = len(dsl)
    off, kids = children_csr(ds)
    inside = [above(v) for v in a]
    closed = all(not (inside[x] and not inside[dsl[x]]) for x in range(n) if dsl[x] >= 0 and dsl[x] != x)
    full = force_full or not closed
    flag = [False] * n
    info = dict(mode=int(full), rounds=0, jobs=0, steps=0, trib_before_main=0, trib_after_main=0, two_tribs=0, kept=0,
                interbasin=0, nan=0)
    jobs = [(x, a[x]) for x in seql if dsl[x] == x]
    for x, _ in jobs:
        flag[x] = True
    info["round_jobs"] = []
    while jobs:
        info["rounds"] += 1
        info["jobs"] += len(jobs)
        info["round_jobs"].append(len(jobs))
        assert info["rounds"] <= len(seql) + 1
        nxt = []
        for p, up in jobs:
            while True:
                info["steps"] += 1
                m = usl[p]
                main_val, main_set, saw_main, tribs = None, False, False, 0
                for c in kids[off[p]:off[p + 1]]:
                    u = a[c]
                    info["nan"] += int(u != u)
                    rest = sub(up, u)
                    cond = above(rest) and above(u)
                    if c == m:
                        saw_main = True
                        if cond:
                            if not above(sub(a[p], u)):
                                flag[c], main_val = True, u
                                info["interbasin"] += 1
                            elif main_set:
                                info["kept"] += 1
                            else:
                                main_val = u
                        else:
                            main_val = up
                        main_set = True
                    else:
                        val = up
                        if cond:
                            assert m >= 0, "a tributary fires at a cell without a main upstream cell"
                            flag[c], val = True, u
                            up = rest
                            main_val, main_set = up, True
                            tribs += 1
                            info["trib_after_main" if saw_main else "trib_before_main"] += 1
                        if full or inside[c]:
                            nxt.append((c, val))
                info["two_tribs"] += int(tribs >= 2)
                if saw_main and (full or inside[m]):
                    p, up = m, main_val
                else:
                    break
        jobs = nxt
    idxs = [x for x in seql if flag[x]]
    lab = [0] * n
    for i, x in enumerate(idxs):
        lab[x] = i + 1
    return _fill(lab, dsl, seql), idxs, info


# ---- inputs of a case --------------------------------------------------------------------------------------------------
def threshold(upa, name):
    """The threshold of a case as the Python number that is passed on."""
    flat = np.sort(np.asarray(upa).ravel())
    if name == "zero":
        return 0
    if name == "neg":
        return -1.5
    if name == "frac":
        return 2.5
    if name == "huge":
        return float(flat[-1]) * 2 + 1
    if name == "big":
        return float(flat[-min(flat.size, flat.size // 40 + 2)])
    assert name == "mid", name
    return float(flat[-min(flat.size, flat.size // 8 + 2)])


def random_areas(n, seed):
    """Non-monotone float32 areas with NaNs."""
    rng = np.random.default_rng([77, seed, n])
    a = (rng.random(n) * 40).astype(np.float32)
    a[rng.random(n) < 0.05] = np.nan
    return a


def other_areas(n):
    """Positive areas that choose other main upstream cells than the cell count does."""
    return 1.0 + np.random.default_rng([78, n]).random(n)


def nep50_area_min(ds, seq, usm, A):
    """A Python float one float64 step below a float32 difference that the loop forms on the float32 areas ``A`` and on
    which the outlets depend: rounded to float32 (the weak form) it IS that difference and the test ``>`` fails, as
    np.float64 (strong: compared in float64) it passes.  Found by trying the differences a first run forms."""
    A = np.asarray(A, np.float32).ravel()
    trace = []
    ref_serial(ds, seq, usm, A, threshold(A, "mid"), trace)
    for rest, u in sorted(set(t for t in trace if t[0] == t[0] and 0 < t[0] < t[1])):
        am = float(np.nextafter(np.float64(rest), -np.inf))
        formed = []
        weak = ref_serial(ds, seq, usm, A, am, formed)[1]
        if any(r == rest for r, _ in formed) and weak != ref_serial(ds, seq, usm, A, np.float64(am))[1]:
            return am
    raise AssertionError("no difference decides an outlet")


class FromFlw:
    """The inputs of a raster's cases from FlwdirRaster objects (the reference's or the device's), one per transform."""

    def __init__(self, flws):
        self.flws = flws
        self._areas = {}
        flw = flws["own"]
        self.ds, self.seq, self.usm = flw.idxs_ds, flw.idxs_seq, flw.main_upstream()

    def area(self, tr, unit):
        if (tr, unit) not in self._areas:
            self._areas[tr, unit] = np.asarray(self.flws[tr].upstream_area(unit)).ravel()
        return self._areas[tr, unit]


class FromOracle:
    """The same from the CPU oracle, without the reference and without a GPU."""

    def __init__(self, raster, O):
        self.O = O
        self.raster = raster
        self.d8, self.ds, self.pits, self.seq = BC.graph(raster, O)
        self._areas = {}
        self.usm = O.main_upstream(self.ds, self.area("own", "cell"))

    def area(self, tr, unit):
        if tr not in self._areas:
            t, latlon = BC.transform_of(self.raster, tr)
            self._areas[tr] = BC.areas(self.O, self.ds, self.seq, self.d8.shape, t, latlon)
        return self._areas[tr][unit].ravel()


def case(spec, src):
    """(areas[n], area_min, default): the flat areas of a case, the threshold as it is passed, and whether the call leaves
    ``uparea`` to its default.  The "cached" special also needs ``other_areas`` (see ``run``)."""
    if spec[0] != "special":
        tr, area, t = spec
        A = src.area(tr, "cell") if area == "cell" else src.area(tr, "km2")
        if area == "km2f":
            A = A.astype(np.float32)
        return A, threshold(A, t), area == "km2"
    name = spec[1]
    n = src.ds.size
    if name == "equal":
        return np.full(n, 3.0), 1.0, False
    if name == "nan":
        return random_areas(n, 0), 6.0, False
    if name in ("nep50_weak", "nep50_strong"):
        A = src.area("own", "km2").astype(np.float32)
        am = nep50_area_min(src.ds, src.seq, src.usm, A)
        return A, (am if name == "nep50_weak" else np.float64(am)), False
    if name == "np_int":  # a strong integer threshold on float32 areas: compared in float64
        A = (src.area("own", "cell") * np.float32(1.1)).astype(np.float32)
        return A, np.int64(round(threshold(A, "mid"))), False
    if name == "np_f32":  # a strong float32 threshold on integer areas: compared in float64
        A = src.area("own", "cell")
        return A, np.float32(threshold(A, "mid") + 0.5), False
    assert name == "cached", name
    A = src.area("own", "km2")
    return A, threshold(A, "mid"), False


def run(make_flw, spec, src):
    """One case through a front end: ``make_flw(transform, cache)`` makes a FlwdirRaster.  (map, outlets)."""
    A, area_min, default = case(spec, src)
    if spec[0] == "special" and spec[1] == "cached":
        flw = make_flw("own", True)
        flw.main_upstream(other_areas(A.size).reshape(flw.shape))  # (cached: what the call then follows)
    else:
        flw = make_flw("own" if spec[0] == "special" else spec[0], False)
    return flw.subbasins_area(area_min, uparea=None if default else A.reshape(flw.shape))


def usm_of(spec, src, O):
    """The main upstream cells a case follows."""
    if spec[0] == "special" and spec[1] == "cached":
        return O.main_upstream(src.ds, other_areas(src.ds.size))
    return src.usm
