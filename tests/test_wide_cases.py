"""Pin the reference and the cases of tests/wide_cases.py, which judge the fixed-point upstream area (csrc/wide.h) in
tests/test_gpu_wide_fuzz.py, without a GPU.

The reference against itself: the split-sum form (two int64 sums of the 32-bit halves, recombined as unbounded integers)
and one loop over unbounded Python integers agree on every small case.  Against what tests/test_gpu_wide.py already pins on
the lat/lon goldens: the oracle path of its ``_quantised_sums`` bit for bit, and the recorded ``uparea_km2_latlon`` within
its REL = 1e-9.

The cases against their edges: the straddles wrap under the tight rule s = 64 - ex and not under s = 63 - ex, the clamp
rows produce f = 2^32 - 1, the row below the quantum is one row, acyclic rasters are acyclic and cyclic ones hold a loop,
the shapes with / without an interior rectangle and with several hypertiles are what csrc/tiled.hip says, and a hypertile
holds more super-exits than the lowered PFD_TEST_HCAP of the overflow runs."""
import math
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_wide as TW  # noqa: E402  (its _quantised_sums and REL; the GPU tests in it keep their own mark)
import wide_cases as W  # noqa: E402
from conftest import case_names  # noqa: E402
from golden_util import Case  # noqa: E402

from pyflwdir_amd import gis  # noqa: E402
from pyflwdir_amd._affine import Affine  # noqa: E402


@pytest.fixture(scope="module")
def acyclic():
    return W.acyclic_cases(gis.area_rows, Affine)


@pytest.fixture(scope="module")
def cyclic():
    return W.cyclic_cases(gis.area_rows, Affine)


@pytest.fixture(scope="module")
def limits():
    return W.limit_cases()


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_split_sums_agree_with_the_unbounded_loop(oracle, acyclic, limits):
    small = [c for c in acyclic + limits if c.taken and c.n <= W.SMALL]
    assert len(small) >= 30
    for c in small:
        s = W.scale_exponent(c.rows, c.shape[1])
        assert s is not None, c.name
        w = W.cell_weights(c.rows, c.shape[1], s)
        idxs_ds, seq = c.graph(oracle)
        hi, lo = W.split_sums(oracle, idxs_ds, seq, w)
        sums = W.recombine(hi, lo).tolist()
        assert sums == W.serial_sums(idxs_ds, seq, w), c.name
        assert max(sums) < 1 << 64, c.name
        u, wrapped = W.recombine_u64(hi, lo)
        assert not wrapped.any() and u.tolist() == sums, c.name
        # the weights themselves, cell by cell in Python integers
        q, f = W.quantise(c.rows, s)
        for r in {0, c.shape[0] // 2, c.shape[0] - 1}:
            assert w[r].tolist() == [q[r] + (((k + 1) * f[r]) >> 32) - ((k * f[r]) >> 32) for k in range(c.shape[1])]
            assert sum(w[r].tolist()) == c.shape[1] * q[r] + ((c.shape[1] * f[r]) >> 32)


def test_recombination_reports_a_sum_of_two_to_the_64():
    hi, lo = np.array([M := (1 << 32) - 1, M, 5], np.int64), np.array([M, M + 1, 7 << 32], np.int64)
    assert W.recombine(hi, lo).tolist() == [(1 << 64) - 1, 1 << 64, (12 << 32)]
    u, wrapped = W.recombine_u64(hi, lo)
    assert wrapped.tolist() == [False, True, False] and u[[0, 2]].tolist() == [(1 << 64) - 1, 12 << 32]


@pytest.mark.parametrize("name", case_names())
def test_reference_on_the_latlon_goldens(oracle, manifest, name):
    case = Case(name, manifest)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the mean of no coordinate differences, on one row / one column)
        rows = np.ascontiguousarray(gis.area_rows(Affine(*case.transform), case.shape, case.latlon, unit="m2")
                                    / gis.AREA_FACTORS["km2"])
    s = W.scale_exponent(rows, case.shape[1])
    if not np.all(np.isfinite(rows)):
        assert min(case.shape) == 1 and s is None  # (the cell size of one row / one column is NaN in the reference too)
        return
    assert case.latlon and rows.dtype == np.float64 and s is not None
    if case.entry["stats"]["n_loop_cells"]:
        return  # (cells on and above a loop are not in the sequence: the device does not take such a raster)
    quantum = math.ldexp(1.0, -s)
    exp, largest = W.expected(oracle, case.d8, rows, quantum)
    assert largest < 1 << 63
    old, nseq = TW._quantised_sums(oracle, case.d8, rows, quantum)
    assert exp.tobytes() == old.tobytes()
    if "uparea_km2_latlon" in case.full:
        rec = case.full["uparea_km2_latlon"].ravel()
        v = case.d8.ravel() != 247
        assert np.all(exp[~v] == -9999.0) and np.all(rec[~v] == -9999.0)
        assert np.max(np.abs(exp[v] - rec[v]) / np.abs(rec[v])) <= TW.REL


# ---- the cases reach their edges -----------------------------------------------------------------------------------------------
def test_straddles_wrap_under_the_tight_rule_only(limits):
    strad = [c for c in limits if c.kind == "straddle"]
    assert len(strad) >= 3 + 8
    for c in strad:
        ncol = c.shape[1]
        tot = W.float_total(c.rows, ncol)
        ex = math.frexp(tot)[1]
        exact = sum(Fraction(v) for v in c.rows.tolist()) * ncol
        assert tot < Fraction(2) ** ex <= exact, c.name  # the float total and the real one lie either side of 2^ex
        assert W.scale_exponent(c.rows, ncol, "tight") == 64 - ex and W.scale_exponent(c.rows, ncol) == 63 - ex
        assert W.quantised_total(c.rows, ncol, 64 - ex) >= 1 << 64, c.name
        assert 1 << 63 <= W.quantised_total(c.rows, ncol, 63 - ex) < 1 << 64, c.name
        assert c.d8.shape == (c.rows.size, ncol) and np.isin(c.d8, [0, 255]).sum() == 1  # drain-all: one cell holds the total
    assert W.quantised_total(np.array([0.1] * 10), 64, 58) == 18446744073709552640  # (2^64 + 1024)


def test_clamp_rows_clamp(acyclic):
    hit = 0
    for c in acyclic:
        if c.kind != "clamp":
            continue
        q, f = W.quantise(c.rows, W.scale_exponent(c.rows, c.shape[1]))
        assert f[0] == 0 and all(v == 4294967295 for v in f[1:]), c.name
        for v, fl in zip(c.rows[1:].tolist(), q[1:]):
            x = Fraction(v) * Fraction(2) ** W.scale_exponent(c.rows, c.shape[1])
            assert 0 < 1 - (x - fl) <= Fraction(1, 1 << 33)
        hit += 1
    assert hit >= 2


def test_rows_at_and_below_the_quantum(limits):
    by = {c.name: c for c in limits}
    for tag, smallest in (("1", 1), ("2", 2), ("3", 3), ("2p20", 1 << 20)):
        c = by[f"smallest_{tag}_quanta"]
        q, _ = W.quantise(c.rows, W.scale_exponent(c.rows, c.shape[1]))
        assert min(q) == smallest and c.taken
    c = by["smallest_below_quantum"]
    assert not c.taken and W.scale_exponent(c.rows, c.shape[1]) is None
    s = 63 - math.frexp(W.float_total(c.rows, c.shape[1]))[1]
    q, _ = W.quantise(c.rows, s)
    assert sorted(q)[:2][0] == 0 and sorted(q)[1] >= 1  # floor(x) == 0 in exactly one row


def test_magnitude_limits(limits):
    by = {c.name: c for c in limits}
    assert 1e294 < W.float_total(by["total_1e295"].rows, 66) < 1e296 and W.scale_exponent(by["total_1e295"].rows, 66) < -900
    assert W.scale_exponent(by["rows_1e-280"].rows, 66) > 900
    assert W.scale_exponent(by["scale_2p1023"].rows, 5) == 1023
    for name in ("scale_2p1024", "rows_1e-300", "rows_2p-1000"):  # s beyond 1023: 2^s is no finite float64
        c = by[name]
        assert not c.taken and W.scale_exponent(c.rows, c.shape[1]) is None
        assert 63 - math.frexp(W.float_total(c.rows, c.shape[1]))[1] > 1023
    for c in limits:
        assert c.taken == (W.scale_exponent(c.rows, c.shape[1]) is not None), c.name


def test_acyclic_rasters_are_acyclic(oracle, acyclic, limits):
    assert len(acyclic) == 2 * len(W.SHAPES) + len(W.DRAIN_SHAPES)
    assert {c.shape for c in acyclic} == set(W.SHAPES)
    assert {c.kind for c in acyclic} == set(W.KINDS)
    long = W.long_case(gis.area_rows, Affine)
    for c in acyclic + limits + W.exit_graph_cases(oracle, gis.area_rows, Affine) + [long]:
        idxs_ds, seq = c.graph(oracle)
        rank = oracle.rank(idxs_ds)[0]
        assert not (rank[c.d8.ravel() != 247] == -1).any(), c.name
        assert seq.size == np.count_nonzero(c.d8 != 247), c.name
        if c.taken:
            assert W.scale_exponent(c.rows, c.shape[1]) is not None, c.name
    assert any((c.d8 == 247).mean() > 0.3 for c in acyclic) and any(not (c.d8 == 247).any() for c in acyclic)
    assert any((c.d8 == 0).any() for c in acyclic) and any((c.d8 == 255).any() for c in acyclic)
    drains = [c for c in acyclic if c.name.startswith("drain")]
    for c in drains:  # one cell holds the whole raster
        idxs_ds, seq = c.graph(oracle)
        assert np.count_nonzero(idxs_ds == np.arange(c.n)) == 1 and seq.size == c.n


def test_cyclic_rasters_hold_a_loop(oracle, cyclic):
    crossing = 0
    for c in cyclic:
        idxs_ds, _ = c.graph(oracle)
        rank = oracle.rank(idxs_ds)[0]
        loop = (rank == -1) & (c.d8.ravel() != 247)
        assert loop.any() and not c.taken, c.name
        x = np.flatnonzero(loop)
        d = idxs_ds[x]
        ncol = c.shape[1]
        crossing += int(np.any(((x // ncol) // W.TS != (d // ncol) // W.TS) | ((x % ncol) // W.TS != (d % ncol) // W.TS)))
    assert crossing >= 6  # loops (or their tributaries) that cross a tile border


def test_shape_classes():
    f = W.has_interior
    assert [s for s in W.SHAPES if f(s)] == [(200, 511), (513, 520), (2100, 200)]
    assert not f((130, 67)) and not f((128, 511)) and f((129, 132)) and not f((129, 131)) and not f((1030, 90))
    assert W.n_hypertiles((2100, 200)) == 2 and W.n_hypertiles((513, 520)) == 1 and W.n_hypertiles(W.SYNTH[0]) == 4
    assert W.n_hypertiles(W.LONG) == 65  # above FLAT_MAX_HT = 64: production keeps the hypertile form of level 3
    assert -(-513 // W.SUPER) * -(-520 // W.SUPER) == 4  # 2 x 2 supertiles


def test_hypertile_cases_overflow_the_lowered_capacity(oracle):
    cases = [c for c in W.exit_graph_cases(oracle, gis.area_rows, Affine) if W.n_hypertiles(c.shape) > 1]
    assert len(cases) >= 3
    for c in cases:
        assert W.super_exits_per_hypertile(c.d8).max() > W.HCAP_LOWERED, c.name
