"""Cases and the reference for the fixed-point upstream area (csrc/wide.h, pfd_upstream_area_rows_fixed), shared by
tests/test_wide_cases.py (CPU: the reference against itself and the goldens, the cases against their edges) and
tests/test_gpu_wide_fuzz.py (the device against the reference).  Nothing here touches the library under test: the oracle
and ``gis.area_rows`` are handed in by the callers.

THE REFERENCE cannot wrap.  A cell's weight is what wide.h states — floor(row * 2^s) plus the cell's Bresenham share
((c + 1) f >> 32) - (c f >> 32) of the row's fraction f — split into its high and low 32 bits; either half is accumulated on
its own (a half's sum stays below 2^63 on any raster of fewer than 2^31 cells) and the halves are recombined as unbounded
integers.  A sum that reaches 2^64 is reported, never reduced.  ``serial_sums`` says the same in one loop over unbounded
Python integers, without the split; the two check each other on every small case.

THE SCALE is wide.h's host rule restated: s = 63 - ex with ``tot = f * 2^ex`` the float64 total summed row by row (rule
"headroom"); ``rule="tight"`` is the earlier s = 64 - ex, kept to show on the CPU which inputs wrap under it."""
import math
from fractions import Fraction

import numpy as np

M32 = (1 << 32) - 1
TS, SUPER, HYPER = 64, 512, 2048  # tile, supertile and hypertile edges in cells (csrc/tiled.h)
SMALL = 70000  # cells up to which the unbounded-integer loop runs as well
HCAP_LOWERED = 100  # the PFD_TEST_HCAP of the overflow runs: fewer than the super-exits of a hypertile of the cases below
CODES = np.array([1, 2, 4, 8, 16, 32, 64, 128, 0, 255, 247], np.uint8)
DR = {1: 0, 2: 1, 4: 1, 8: 1, 16: 0, 32: -1, 64: -1, 128: -1}
DC = {1: 1, 2: 1, 4: 0, 8: -1, 16: -1, 32: -1, 64: 0, 128: 1}


# ---- the host rule -------------------------------------------------------------------------------------------------------------
def float_total(rows, ncol):
    """The float64 total as the host computes it: the rows added in order, then times the number of columns."""
    tot = 0.0
    for v in np.asarray(rows, np.float64).tolist():
        tot += v
    return tot * float(ncol)


def scale_exponent(rows, ncol, rule="headroom"):
    """s of the fixed-point scale 2^s, or None where the host refuses the call (a value that is not finite and positive,
    a scale that is no normal float64, a row below one quantum)."""
    vals = np.asarray(rows, np.float64).tolist()
    if not all(v > 0.0 and v < 1e300 for v in vals):
        return None
    tot = float_total(rows, ncol)
    if not (tot > 0.0 and tot < 1e300):
        return None
    ex = math.frexp(tot)[1]
    s = (63 if rule == "headroom" else 64) - ex
    if s > 1023 or s < -1022:
        return None
    if any(Fraction(v) * Fraction(2) ** s < 1 for v in vals):
        return None
    return s


def quantise(rows, s):
    """Per row the integer part floor(row * 2^s) and the fraction as 32-bit fixed point (clamped), in Python integers."""
    q, f = [], []
    for v in np.asarray(rows, np.float64).tolist():
        x = Fraction(v) * Fraction(2) ** s  # (exact: a power-of-two scale)
        fl = x.numerator // x.denominator
        q.append(fl)
        f.append(min(int((x - fl) * (1 << 32)), M32))
    return q, f


def quantum_exponent(quantum):
    """s of a quantum 2^-s; asserts that it is a power of two."""
    m, e = math.frexp(quantum)
    assert quantum > 0.0 and m == 0.5, f"quantum {quantum!r} is no power of two"
    return 1 - e


def cell_weights(rows, ncol, s):
    """[nrow, ncol] uint64 weights (every weight is below 2^63 wherever scale_exponent allows s)."""
    q, f = quantise(rows, s)
    assert max(q) < 1 << 63
    c = np.arange(ncol, dtype=np.uint64)[None, :]
    fa = np.array(f, np.uint64)[:, None]
    return np.array(q, np.uint64)[:, None] + ((((c + np.uint64(1)) * fa) >> np.uint64(32)) - ((c * fa) >> np.uint64(32)))


def quantised_total(rows, ncol, s):
    """The exact sum of every cell's weight, as an unbounded integer (a row sums to ncol q + (ncol f >> 32))."""
    q, f = quantise(rows, s)
    return sum(ncol * a + ((ncol * b) >> 32) for a, b in zip(q, f))


# ---- the sums --------------------------------------------------------------------------------------------------------------------
def graph(O, d8):
    idxs_ds, idxs_pit, _ = O.from_array(d8)
    return idxs_ds, O.idxs_seq(idxs_ds, idxs_pit)


def split_sums(O, idxs_ds, seq, w):
    """Upstream sums of the uint64 weights ``w``: (hi, lo) int64 sums of the high and low 32-bit halves (the oracle's int64
    accuflux on each; neither can wrap below 2^31 cells)."""
    assert w.dtype == np.uint64 and w.size < 1 << 31
    w = np.ascontiguousarray(w).ravel()
    hi = O.accuflux(idxs_ds, seq, (w >> np.uint64(32)).astype(np.int64), nodata=-1)
    lo = O.accuflux(idxs_ds, seq, (w & np.uint64(M32)).astype(np.int64), nodata=-1)
    return hi, lo


def recombine(hi, lo):
    """hi * 2^32 + lo as unbounded Python integers (an object array)."""
    return hi.astype(object) * (1 << 32) + lo.astype(object)


def recombine_u64(hi, lo):
    """The same without object arrays, for the large rasters: (uint64 sums, the cells whose sum is >= 2^64)."""
    top = hi + (lo >> 32)  # (below 2^63: hi < 2^63 - 2^31)
    wrapped = top > M32
    return (top.astype(np.uint64) << np.uint64(32)) | (lo & M32).astype(np.uint64), wrapped


def serial_sums(idxs_ds, seq, w):
    """The upstream sums in one loop over ``seq`` from upstream to downstream, in unbounded Python integers."""
    tot = [int(v) for v in np.ascontiguousarray(w).ravel().tolist()]
    ds = idxs_ds.tolist()
    for x in reversed(seq.tolist()):
        d = ds[x]
        if d != x:
            tot[d] += tot[x]
    return tot


def expected(O, d8, rows, quantum, graph_=None):
    """What the device must return bit for bit on an acyclic raster for the quantum it reports: float(sum) * quantum, one
    rounding at integer -> float64, -9999 on nodata.  Returns (float64 [n], the largest sum as an unbounded integer); a sum
    of 2^64 or more fails here."""
    s = quantum_exponent(quantum)
    w = cell_weights(rows, d8.shape[1], s)
    idxs_ds, seq = graph_ or graph(O, d8)
    hi, lo = split_sums(O, idxs_ds, seq, w)
    if d8.size <= SMALL:
        sums = recombine(hi, lo)
        largest = max(sums.tolist())
        assert largest < 1 << 64, f"a sum of the quantised weights reaches 2^64: {largest}"
        u = sums.astype(np.uint64)
        assert np.array_equal(u, recombine_u64(hi, lo)[0])
    else:
        u, wrapped = recombine_u64(hi, lo)
        assert not wrapped.any(), "a sum of the quantised weights reaches 2^64"
        largest = int(u.max())
    exp = u.astype(np.float64) * quantum  # (uint64 -> float64 rounds to nearest even, as the device's conversion does)
    exp[d8.ravel() == 247] = -9999.0
    return exp, largest


# ---- rasters ---------------------------------------------------------------------------------------------------------------------
def random_d8(rng, shape, p_nodata, p_pit, acyclic):
    """Uniformly random codes with both pit codes and nodata; ``acyclic``: only E / SE / S / SW, so that (row, column)
    strictly increases along a path (tests/test_gpu_fuzz.py random_d8, coherent = -1 / 0)."""
    n = shape[0] * shape[1]
    p_dir = (1.0 - p_nodata - p_pit) / 8
    d8 = rng.choice(CODES, size=n, p=[p_dir] * 8 + [p_pit / 2, p_pit / 2, p_nodata]).reshape(shape)
    if acyclic:
        dirs = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=n).reshape(shape)
        d8 = np.where(np.isin(d8, [16, 32, 64, 128]), dirs, d8)
    if not np.isin(d8, [0, 255]).any():
        d8.flat[rng.integers(0, n)] = 0
    return np.ascontiguousarray(d8, dtype=np.uint8)


def drain_all_d8(shape, pit=0):
    """Column 0 flows south, every other cell west, one pit in the last row: that cell holds the whole raster's sum."""
    d8 = np.full(shape, 16, np.uint8)
    d8[:, 0] = 4
    d8[-1, 0] = pit
    return d8


def with_border_cycles(d8):
    """Adds loops that cross tile borders: a 2-cycle over the column border at 63 | 64 (or the row border), and a 4-cycle
    around the tile corner where the raster has one."""
    d8 = d8.copy()
    nrow, ncol = d8.shape
    if ncol > TS:
        r = min(5, nrow - 1)
        d8[r, TS - 1], d8[r, TS] = 1, 16
    elif nrow > TS:
        d8[TS - 1, 0], d8[TS, 0] = 4, 64
    else:
        d8[0, 0], d8[0, 1] = 1, 16
    if nrow > TS and ncol > TS:
        d8[TS - 1, TS - 1], d8[TS - 1, TS], d8[TS, TS], d8[TS, TS - 1] = 1, 4, 16, 64
    return d8


def has_interior(shape):
    """The count pass runs its fast interior kernel on a rectangle of tiles (csrc/tiled.hip, TiledRun::init: tiles whose
    ring and 4 staging columns lie inside the raster, first row excluded), the frame kernel on the rest."""
    nrow, ncol = shape
    tr_lo, tr_hi = 1, (nrow - 1) // TS if nrow - 1 >= TS else 0
    tc_lo, tc_hi = 1, (ncol - 4) // TS if ncol >= TS + 4 else 0
    return tr_hi > tr_lo and tc_hi > tc_lo


def n_hypertiles(shape):
    return -(-shape[0] // HYPER) * -(-shape[1] // HYPER)


def super_exits_per_hypertile(d8):
    """Per hypertile the cells whose downstream cell lies in another supertile or off the raster."""
    nrow, ncol = d8.shape
    r, c = np.indices(d8.shape)
    cnt = np.zeros(n_hypertiles(d8.shape), np.int64)
    nhc = -(-ncol // HYPER)
    for code in DR:
        m = d8 == code
        r1, c1 = r[m] + DR[code], c[m] + DC[code]
        off = (r1 < 0) | (r1 >= nrow) | (c1 < 0) | (c1 >= ncol)
        leaves = off | (r1 // SUPER != r[m] // SUPER) | (c1 // SUPER != c[m] // SUPER)
        np.add.at(cnt, ((r[m] // HYPER) * nhc + c[m] // HYPER)[leaves], 1)
    return cnt


# ---- row values ------------------------------------------------------------------------------------------------------------------
def _in_quanta(values_in_quanta, shift):
    """Rows given in units of the quantum they are built for, scaled by an exact power of two."""
    return np.array([math.ldexp(v, shift) for v in values_in_quanta], np.float64)


def _dominated(nrow, ncol, small):
    """Row 0 carries 1.5 x 2^62 / ncol quanta, so that the scale (s = 0 before the shift) does not depend on the other
    rows; ``small``: the values of rows 1 .. in quanta (far below row 0)."""
    big = float(3 << 61) / ncol
    vals = [big] + list(small)
    assert len(vals) == nrow and 1 << 62 <= float_total(vals, ncol) < 1 << 63
    return vals


def rows_latlon(area_rows, affine, shape, lat_top):
    res = 1.0 / 1200.0
    rows = np.ascontiguousarray(area_rows(affine(res, 0.0, 5.0, 0.0, -res, lat_top), shape, True, unit="m2") / 1e6)
    assert rows.dtype == np.float64
    return rows


def rows_equal(nrow, value):
    return np.full(nrow, value, np.float64)


def rows_clamp(rng, nrow, ncol, shift=-40):
    """Rows 1 .. are m + 1 - 2^-36 quanta: the fraction lies within 2^-33 of 1 and its 32-bit form clamps to 2^32 - 1."""
    small = [float(int(m)) + 1.0 - 2.0 ** -36 for m in rng.integers(1, 1 << 15, nrow - 1)]
    return _in_quanta(_dominated(nrow, ncol, small), shift)


def rows_range(rng, nrow, ncol, smallest, shift=17):
    """A dynamic range of ~60 binary orders: row 0 dominates, one row is ``smallest`` quanta, the others lie between."""
    small = [math.floor(2.0 ** e * 8) / 8 + 4.0 + 2.0 * smallest for e in rng.uniform(0, 40, nrow - 1)]
    small[int(rng.integers(0, nrow - 1))] = float(smallest)
    return _in_quanta(_dominated(nrow, ncol, small), shift)


def straddle_search(seed=20260, want=10):
    """Row vectors whose float64 total lies below a power of two 2^ex while the exact sum of the weights quantised with the
    tight rule s = 64 - ex reaches 2^64: found by a seeded search with exact rationals, not tabulated.  The candidates are
    what a regular grid produces: rows in small whole-number proportions a_i that share 2^k out between them, each rounded
    to float64 (ten rows of 0.1 are a_i = 1, k = 0).  Returns a list of (rows, ncol)."""
    rng = np.random.default_rng(seed)
    hits = []
    for _ in range(5000):
        if len(hits) == want:
            break
        ncol = int(rng.choice([1, 2, 3, 5, 8, 64, 67]))
        nrow = int(rng.integers(2, 25))
        k = int(rng.integers(-30, 40))
        a = rng.integers(1, 10, nrow).tolist()
        rows = [math.ldexp(float(x), k) / (sum(a) * ncol) for x in a]
        tot = float_total(rows, ncol)
        ex = math.frexp(tot)[1]
        exact = sum(Fraction(v) for v in rows) * ncol
        if exact >= Fraction(2) ** ex > tot and quantised_total(rows, ncol, 64 - ex) >= 1 << 64:
            hits.append((np.array(rows, np.float64), ncol))
    assert len(hits) == want, f"the search found {len(hits)} of {want} straddles"
    return hits


def straddles():
    """(name, rows, ncol): the three named straddles and the generated family."""
    out = [("tenths_1col", np.array([0.1] * 10), 1), ("tenths_64col", np.array([0.1] * 10), 64),
           ("one_minus_ulp_1col", np.array([1 - 2.0 ** -53] + [2.0 ** -55] * 8), 1)]
    return out + [(f"searched{i}", rows, ncol) for i, (rows, ncol) in enumerate(straddle_search())]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2), (1, 700), (700, 1), (7, 5), (63, 65), (64, 64), (65, 63), (64, 129), (130, 67), (200, 511), (513, 520),
          (1030, 90), (2100, 200)]
DRAIN_SHAPES = [(1, 700), (700, 1), (64, 64), (130, 67), (200, 511), (513, 520), (2100, 200)]  # one per shape class
EXIT_GRAPH_SHAPES = [(513, 520), (2100, 200)]
SYNTH = ((2300, 2600), dict(seed=8, tilt=100000, white=2, nodata_pct=10))  # 2 x 2 hypertiles (tests/test_gpu_large.py)
LONG = (131073, 8)  # 65 x 1 hypertiles: above the 64 up to which production takes the flat forest
KINDS = ["equator", "pole", "tenth", "third", "one", "pow_m40", "pow_37", "clamp", "range1", "range2", "range3", "range_2p20",
         "e-280", "e295"]


class WideCase:
    """One raster with one vector of row values.  ``taken``: the fixed-point form must take it."""

    def __init__(self, name, d8, rows, taken=True, kind=""):
        self.name, self.d8, self.rows, self.taken, self.kind = name, d8, np.ascontiguousarray(rows, np.float64), taken, kind
        self.shape, self.n = d8.shape, d8.size
        self._graph = self._exp = None

    def graph(self, O):
        if self._graph is None:
            self._graph = graph(O, self.d8)
        return self._graph

    def expected(self, O, quantum):
        """The reference for ``quantum``, computed once per case and left unchanged."""
        if self._exp is None or self._exp[0] != quantum:
            exp, largest = expected(O, self.d8, self.rows, quantum, self.graph(O))
            exp.setflags(write=False)
            self._exp = (quantum, exp, largest)
        return self._exp[1]

    def __repr__(self):
        return self.name


def row_values(kind, rng, shape, area_rows, affine):
    nrow, ncol = shape
    if kind == "equator":
        return rows_latlon(area_rows, affine, shape, 0.5 * nrow / 1200.0)
    if kind == "pole":
        return rows_latlon(area_rows, affine, shape, 89.9)
    if kind in ("tenth", "third", "one", "pow_m40", "pow_37"):
        return rows_equal(nrow, dict(tenth=0.1, third=1 / 3, one=1.0, pow_m40=2.0 ** -40, pow_37=2.0 ** 37)[kind])
    if kind == "clamp":
        return rows_clamp(rng, nrow, ncol)
    if kind.startswith("range"):
        return rows_range(rng, nrow, ncol, dict(range1=1.0, range2=2.0, range3=3.5, range_2p20=2.0 ** 20 + 1.25)[kind])
    if kind == "e-280":
        return rows_equal(nrow, 1e-280) * (1.0 + rng.integers(0, 8, nrow) / 8.0)
    if kind == "e295":
        return rows_equal(nrow, 1e295 / (nrow * ncol)) * (1.0 + rng.integers(0, 8, nrow) / 16.0) / 1.5
    raise ValueError(kind)


def kinds_for(shape):
    """Lat/lon areas need two rows and two columns (the cell size is a difference of coordinates); the rows built around a
    dominating row 0 need a second row."""
    nrow, ncol = shape
    return [k for k in KINDS if not ((k in ("equator", "pole") and min(shape) < 2)
                                     or ((k == "clamp" or k.startswith("range")) and nrow < 2))]


def acyclic_cases(area_rows, affine):
    """Two random rasters per shape and one drain-all raster per shape class; the row kinds go round, so that every kind
    meets several shapes."""
    cases, pending = [], []
    for i, shape in enumerate(SHAPES * 2 + DRAIN_SHAPES):
        rng = np.random.default_rng(7000 + i)
        drain = i >= 2 * len(SHAPES)
        if drain:
            d8 = drain_all_d8(shape, pit=(0, 255)[i % 2])
        else:
            d8 = random_d8(rng, shape, p_nodata=(0.0, 0.1, 0.4)[i % 3], p_pit=(0.002, 0.05)[(i // 3) % 2], acyclic=True)
        allowed = kinds_for(shape)
        if not any(k in allowed for k in pending):
            pending += KINDS
        kind = next(k for k in pending if k in allowed)  # (a kind this shape cannot take waits for the next shape)
        pending.remove(kind)
        name = f"{'drain' if drain else 'rand'}{i}_{shape[0]}x{shape[1]}_{kind}"
        cases.append(WideCase(name, d8, row_values(kind, rng, shape, area_rows, affine), kind=kind))
    return cases


def cyclic_cases(area_rows, affine):
    """The unrestricted random codes (full of short loops), plus loops laid over tile borders."""
    cases = []
    for i, shape in enumerate([(7, 5), (63, 65), (64, 129), (130, 67), (200, 511), (513, 520), (700, 1), (1, 700)]):
        rng = np.random.default_rng(7500 + i)
        d8 = random_d8(rng, shape, p_nodata=(0.0, 0.1, 0.4)[i % 3], p_pit=0.05, acyclic=False)
        if min(shape) > 1:
            d8 = with_border_cycles(d8)
            rows = row_values("equator", rng, shape, area_rows, affine)
        elif shape[0] == 1:
            d8[0, TS - 1], d8[0, TS] = 1, 16
            rows = rows_equal(1, 1.0)
        else:
            d8[TS - 1, 0], d8[TS, 0] = 4, 64
            rows = rows_equal(shape[0], 0.1)
        cases.append(WideCase(f"cyclic{i}_{shape[0]}x{shape[1]}", d8, rows, taken=False))
    # an acyclic raster with nothing but one loop across a tile corner
    d8 = with_border_cycles(random_d8(np.random.default_rng(7600), (130, 131), 0.1, 0.01, acyclic=True))
    cases.append(WideCase("one_corner_loop_130x131", d8, rows_equal(130, 1 / 3), taken=False))
    return cases


def limit_cases():
    """The limits of the 64 bits, each on a drain-all raster (the pit holds the whole raster's sum)."""
    cases = []
    for name, rows, ncol in straddles():
        cases.append(WideCase(f"straddle_{name}", drain_all_d8((rows.size, ncol)), rows, kind="straddle"))
    rng = np.random.default_rng(7700)
    shape = (67, 66)
    for smallest, tag in ((1.0, "1"), (2.0, "2"), (3.0, "3"), (2.0 ** 20, "2p20")):
        cases.append(WideCase(f"smallest_{tag}_quanta", drain_all_d8(shape), rows_range(rng, *shape, smallest), kind="quanta"))
    cases.append(WideCase("smallest_below_quantum", drain_all_d8(shape), rows_range(rng, *shape, 1.0 - 2.0 ** -30), taken=False,
                          kind="below"))
    cases.append(WideCase("total_1e295", drain_all_d8(shape), row_values("e295", rng, shape, None, None), kind="huge"))
    cases.append(WideCase("rows_1e-280", drain_all_d8(shape), row_values("e-280", rng, shape, None, None), kind="tiny_taken"))
    # 2^s is the largest finite power of two (s = 1023), and one step beyond it
    cases.append(WideCase("scale_2p1023", drain_all_d8((7, 5)), rows_equal(7, 1.3 * 2.0 ** -961 / 35), kind="tiny_taken"))
    cases.append(WideCase("scale_2p1024", drain_all_d8((7, 5)), rows_equal(7, 1.3 * 2.0 ** -962 / 35), taken=False, kind="tiny"))
    cases.append(WideCase("rows_1e-300", drain_all_d8(shape), rows_equal(67, 1e-300), taken=False, kind="tiny"))
    cases.append(WideCase("rows_2p-1000", drain_all_d8((10, 64)), rows_equal(10, 2.0 ** -1000), taken=False, kind="tiny"))
    return cases


def exit_graph_cases(O, area_rows, affine):
    """The rasters of the exit-graph forms: the (513, 520) and (2100, 200) random cases and one synthetic river raster of
    2 x 2 hypertiles."""
    cases = [c for c in acyclic_cases(area_rows, affine) if c.shape in EXIT_GRAPH_SHAPES and c.name.startswith("rand")]
    shape, kw = SYNTH
    d8 = O.synth_d8(shape[0], shape[1], **kw)
    cases.append(WideCase(f"synth_{shape[0]}x{shape[1]}", d8, rows_latlon(area_rows, affine, shape, 52.0), kind="equator"))
    return cases


def long_case(area_rows, affine):
    rng = np.random.default_rng(7800)
    d8 = random_d8(rng, LONG, p_nodata=0.1, p_pit=0.002, acyclic=True)
    return WideCase(f"long_{LONG[0]}x{LONG[1]}", d8, rows_latlon(area_rows, affine, LONG, 0.5 * LONG[0] / 1200.0), kind="equator")
