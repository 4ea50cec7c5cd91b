"""Pin the serial restatements of tests/serial_refs.py that judge the device in tests/test_gpu_fuzz_paths.py
(_ref_upstream_sum, _ref_ucat_area, _ref_floodplains, _ref_snap with _ref_step_length_f64) to the reference: on the graph
the oracle builds from a golden raster, each must reproduce bit for bit, dtype included, what the reference recorded in
tests/golden/wide_arith.npz, wide_snap.npz, wide_snap2.npz and wide_subgrid.npz.

No golden raster is left out: the sixteen Python loops over the largest one (rhine, 680 000 cells) take a few seconds.

The second half runs the input generators of test_gpu_fuzz_paths.py with the serial references over all its seeds, without a
GPU, and asserts that the edges those kernels can get wrong occur in what the device is compared with."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_fuzz_paths as P  # noqa: E402  (its generators; the GPU tests in it keep their own mark)
from serial_refs import (_ref_floodplains, _ref_snap, _ref_step_length_f64, _ref_ucat_area,  # noqa: E402
                         _ref_upstream_sum)

from oracle import golden_inputs as GI  # noqa: E402
from pyflwdir_amd import gis  # noqa: E402
from pyflwdir_amd._affine import Affine  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(got, exp):
    return got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


def graph(O, manifest, name):
    d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
    idxs_ds, idxs_pit, _ = O.from_array(d8)
    seq = O.idxs_seq(idxs_ds, idxs_pit)
    return d8, idxs_ds, seq, manifest[name]


def accumulated(O, idxs_ds, seq, weights):
    out = O.accuflux(idxs_ds, seq, np.ascontiguousarray(weights), nodata=-9999)
    out[idxs_ds == -1] = -9999
    return out


# ---- the restatements against the reference's recorded outputs ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["flwdir0", "flwdir1", "synth_loops_96x80", "synth_tiny_5x7", "synth_onerow_1x300"])
def test_upstream_sum_recorded(oracle, manifest, name):
    W = np.load(os.path.join(GOLD, "wide_arith.npz"))
    d8, idxs_ds, _, _ = graph(oracle, manifest, name)
    keys = [k[3:] for k in W.files if k.startswith(f"in_{name}_")]
    assert len(keys) >= 2
    for key in keys:
        got = _ref_upstream_sum(idxs_ds, W["in_" + key].ravel(), -9999, -1).reshape(d8.shape)
        assert same(got, W["out_" + key]), key
    got = _ref_upstream_sum(idxs_ds, np.ones(d8.size, np.float64), np.nan, -1).reshape(d8.shape)
    assert same(got, W[f"out_{name}_ones_nan"])


@pytest.mark.parametrize("name", ["flwdir0", "flwdir_large", "synth_rough_nodata_384x512", "rhine"])
def test_snap_recorded(oracle, manifest, name):
    """All eleven recorded snap calls: downstream and along the main upstream cells, in cells and in metres."""
    W, W2 = np.load(os.path.join(GOLD, "wide_snap.npz")), np.load(os.path.join(GOLD, "wide_snap2.npz"))
    d8, idxs_ds, seq, ent = graph(oracle, manifest, name)
    main = oracle.main_upstream(idxs_ds, accumulated(oracle, idxs_ds, seq, np.ones(d8.size, np.int32)))
    idxs = W[f"in_{name}_idxs"]
    streams, heads = W[f"in_{name}_streams"].ravel().tolist(), W2[f"in_{name}_heads"].ravel().tolist()
    lengths = {}

    def metres(a, b):
        if (a, b) not in lengths:
            lengths[(a, b)] = _ref_step_length_f64(a, b, d8.shape[1], ent["latlon"], ent["transform"])
        return lengths[(a, b)]

    cells = lambda a, b: 1.0  # noqa: E731
    calls = dict(snap=(W, idxs_ds, streams, None, cells), snap5=(W, idxs_ds, streams, 5, cells),
                 snap_nomask=(W, idxs_ds, None, None, cells), down_m=(W2, idxs_ds, streams, None, metres),
                 down_m_max=(W2, idxs_ds, streams, 2500.0, metres), down_m_nomask=(W2, idxs_ds, None, None, metres),
                 up_cell=(W2, main, None, None, cells), up_cell_mask=(W2, main, heads, None, cells),
                 up_cell_max=(W2, main, None, 7, cells), up_m=(W2, main, None, None, metres),
                 up_m_max=(W2, main, heads, 4000.0, metres))
    for key, (rec, nxt, mask, max_length, step) in calls.items():
        got_i, got_d = _ref_snap(idxs, nxt, -1, mask, max_length, step)
        assert same(got_i, rec[f"out_{name}_{key}_idxs"]), key
        assert same(got_d, rec[f"out_{name}_{key}_dist"]), (key, np.flatnonzero(got_d != rec[f"out_{name}_{key}_dist"])[:5])


@pytest.mark.parametrize("name", ["flwdir0", "flwdir_large", "flwdir1", "synth_loops_96x80", "rhine", "synth_rough_nodata_384x512"])
def test_subgrid_recorded(oracle, manifest, name):
    """ucat_area for both transforms, both outlet lists and three units; both recorded floodplain variants."""
    W = np.load(os.path.join(GOLD, "wide_subgrid.npz"))
    d8, idxs_ds, seq, ent = graph(oracle, manifest, name)
    for tag, tr, latlon in (("ll", ent["transform"], ent["latlon"]), ("pr", GI.PROJ_TRANSFORM, False)):
        area = gis.area_grid(Affine(*tr), d8.shape, latlon, unit="m2").ravel()
        for key_io in ("idxs_out", "idxs_out_dup"):
            io = W[f"in_{name}_{key_io}"]
            for unit in ("cell", "km2", "ha"):
                a = np.ones(d8.size, np.int32) if unit == "cell" else area / gis.AREA_FACTORS[unit]
                m, are = _ref_ucat_area(io.ravel(), idxs_ds, seq, a, -1)
                assert same(m.reshape(d8.shape), W[f"out_{name}_{tag}_{key_io}_{unit}_map"]), (tag, key_io, unit)
                assert same(are.reshape(io.shape), W[f"out_{name}_{tag}_{key_io}_{unit}_are"]), (tag, key_io, unit)
        elv = W[f"in_{name}_elevtn"].ravel()
        thr = float(W[f"in_{name}_{tag}_upa_min"])
        upa = accumulated(oracle, idxs_ds, seq, area / gis.AREA_FACTORS["km2"])
        got = _ref_floodplains(idxs_ds, seq, elv, upa, thr, 0.3).reshape(d8.shape)
        assert same(got, W[f"out_{name}_{tag}_fld"]), tag
        got = _ref_floodplains(idxs_ds, seq, elv.astype(np.float64) * 1.000001, upa, thr * 0.5, 0.5).reshape(d8.shape)
        assert same(got, W[f"out_{name}_{tag}_fld_b05_f64"]), tag


def test_step_length_is_the_library_table():
    """The scalar restatement agrees with the float64 table the library hands to the device (the median of that table sets a
    ``max_length`` in test_gpu_fuzz_paths.py)."""
    for nrow, ncol, tr, latlon in ((7, 5, P.LL_TRANSFORM, True), (7, 5, GI.PROJ_TRANSFORM, False), (1, 9, P.LL_TRANSFORM, True)):
        tab = gis.step_length_table(nrow, latlon, tr, dtype=np.float64)
        for r0 in range(nrow):
            for dr, dc, kind in ((1, 0, 0), (0, 1, 1), (1, 1, 2), (1, -1, 2), (-1, 1, 2), (-1, 0, 0)):
                r1, c0 = r0 + dr, 2
                if not 0 <= r1 < nrow:
                    continue
                got = _ref_step_length_f64(r0 * ncol + c0, r1 * ncol + c0 + dc, ncol, latlon, tr)
                assert isinstance(got, float) and got == tab[r0 + r1, kind]


# ---- the inputs of test_gpu_fuzz_paths.py reach the edges ----------------------------------------------------------------------
EDGES = ["flood_admitted_dh_equals_h0", "flood_rejected_within_one_f32_ulp_of_z0", "flood_decided_by_the_f32_drain_elevation",
         "flood_stream_restarts_above_a_rejected_cell", "sum_i32_wrapped", "sum_own_event_between_three_inflows",
         "sum_order_of_float_adds_shows", "ucat_outlet_off_the_sequence", "ucat_first_of_a_repeated_outlet_keeps_own_area",
         "ucat_outlet_directly_upstream_of_an_outlet", "snap_stopped_by_max_length", "snap_stopped_exactly_at_max_length",
         "snap_ended_on_nodata", "snap_up_ended_on_the_missing_main_upstream_cell", "snap_f32_sum_of_steps_differs"]


def flood_edges(c, found):
    upa, upa_min, variants = P.floodplain_cases(c)
    ds, seq = c.idxs_ds, c.seq
    stream = upa >= upa_min
    for label, elv, b in variants:
        fld = _ref_floodplains(ds, seq, elv, upa, upa_min, b)
        assert fld.dtype == np.int8 and np.all(fld[~c.in_seq] == -1) and np.all(fld[stream & c.in_seq] == 1)
        src = [-1] * c.n  # the stream cell whose (z, h) a floodplain cell carries
        dsl, fl, st = ds.tolist(), fld.tolist(), stream.tolist()
        for x in seq.tolist():
            src[x] = x if st[x] else (src[dsl[x]] if fl[x] == 1 else -1)
        x = seq[~stream[seq] & (fld[ds[seq]] == 1)]  # the cells that were judged
        s = np.array(src)[ds[x]]
        with np.errstate(invalid="ignore"):
            z0, h0 = elv[s].astype(np.float32), (upa[s] ** b).astype(np.float32)
            dh = elv[x] - z0
            assert dh.dtype == elv.dtype and np.array_equal(dh <= h0, fld[x] == 1)  # (the loop, said once more in whole arrays)
            found["flood_admitted_dh_equals_h0"] += int(np.sum(dh == h0))
            found["flood_rejected_within_one_f32_ulp_of_z0"] += int(np.sum((dh > h0) & (dh - h0 < np.spacing(np.abs(z0)))))
            found["flood_decided_by_the_f32_drain_elevation"] += int(np.sum((elv[x] - elv[s] <= h0) != (dh <= h0)))
        found["flood_stream_restarts_above_a_rejected_cell"] += int(np.sum(stream[seq] & (fld[ds[seq]] == 0)))


def sum_edges(c, found):
    ds, idx = c.idxs_ds, np.arange(c.n)
    link = (ds != c.mv) & (ds != idx)
    for label, data, mv in P.upstream_sum_cases(c):
        out = _ref_upstream_sum(ds, data, mv, c.mv)
        assert out.dtype == data.dtype
        nd = data == mv
        dsafe = np.where(link, ds, 0)
        flows = link & ~nd & ~nd[dsafe]  # the links that add
        below = np.bincount(ds[flows & (idx < ds)], minlength=c.n)
        above = np.bincount(ds[flows & (idx > ds)], minlength=c.n)
        event = link & ~nd & nd[dsafe]  # the cell's own write of the missing value, its own value being valid
        found["sum_own_event_between_three_inflows"] += int(np.sum(event & (below >= 1) & (above >= 1) & (below + above >= 3)))
        if data.dtype == np.int32:
            wide = _ref_upstream_sum(ds, data.astype(np.int64), mv, c.mv)
            assert np.array_equal(wide.astype(np.int32), out)  # (the same sums modulo 2**32)
            found["sum_i32_wrapped"] += int(np.sum(wide != out))
        if data.dtype.kind == "f":
            rev = np.zeros(c.n, data.dtype)  # the same operands added in descending cell index
            src = np.flatnonzero(flows)[::-1]
            np.add.at(rev, ds[src], data[src])
            plain = ~(link & (nd | nd[dsafe]))  # cells without an own event
            found["sum_order_of_float_adds_shows"] += int(np.sum(plain & (rev != out)))


def ucat_edges(c, found):
    for label, tag, unit, io in P.ucat_cases(c):
        m, a = P.ucat_expected(c, tag, unit, io)
        area = P.area_flat(c, tag, unit)
        assert m.dtype == c.idxs_ds.dtype and a.dtype == area.dtype and a.shape == io.shape
        flat, are = io.ravel(), a.ravel()
        assert np.all(are[flat == c.mv] == -9999)
        last = {int(x): i for i, x in enumerate(flat)}
        for i, x in enumerate(flat.tolist()):
            if x == c.mv:
                continue
            assert m.ravel()[x] == last[x] + 1  # an outlet keeps its label, wherever it lies
            if not c.in_seq[x]:
                assert are[i:i + 1].tobytes() == area[x:x + 1].tobytes()  # (bytes: a raster of one row has NaN lat/lon areas)
                found["ucat_outlet_off_the_sequence"] += int(c.offseq[x])
            elif last[x] != i and are[i] == area[x] and are[last[x]] != area[x]:
                found["ucat_first_of_a_repeated_outlet_keeps_own_area"] += 1
            d = int(c.idxs_ds[x])
            if c.in_seq[x] and d != x and d in last:
                found["ucat_outlet_directly_upstream_of_an_outlet"] += 1


def snap_edges(O, c, found):
    main = P.main_upstream(O, c)
    memo = {}
    for call in P.snap_calls(c):
        out, dist = P.snap_expected(c, call, main, memo)
        assert out.dtype == call["idxs"].dtype and dist.dtype == np.float32
        nxt = c.idxs_ds if call["direction"] == "down" else main
        moved = out != call["idxs"]
        on_mask = np.zeros(out.size, bool) if call["mask"] is None else call["mask"][out]
        open_end = ~on_mask & (nxt[out] != c.mv) & (nxt[out] != out)  # a next cell existed: only max_length ends such a walk
        assert call["max_length"] is not None or not open_end.any()
        found["snap_stopped_by_max_length"] += int(open_end.sum())
        if call["max_length"] is not None:
            found["snap_stopped_exactly_at_max_length"] += int(np.sum(open_end & (dist == np.float32(call["max_length"])) & moved))
        if call["direction"] == "down":  # (no cell flows into nodata in a decoded D8 raster: such a walk starts there)
            found["snap_ended_on_nodata"] += int(np.sum(~on_mask & c.nodata[out]))
        else:
            found["snap_up_ended_on_the_missing_main_upstream_cell"] += int(np.sum(moved & ~on_mask & (main[out] == c.mv)))
        if call["unit"] == "m":
            nxt_l, mask_l = nxt.tolist(), None if call["mask"] is None else call["mask"].tolist()
            step = lambda a, b: memo[call["tag"]][(a, b)]  # noqa: E731  (snap_expected has walked these links)
            single = _walk_float32(call["idxs"], nxt_l, c.mv, mask_l, call["max_length"], step, out)
            found["snap_f32_sum_of_steps_differs"] += int(np.sum(single.view(np.uint32) != dist.view(np.uint32)))


def _walk_float32(idxs0, nxt, mv, mask, max_length, step, ends):
    """The distances of the walks that end in ``ends``, with the running sum rounded to float32 after every step."""
    dists = np.zeros(idxs0.size, np.float32)
    for i, (x, end) in enumerate(zip(idxs0.tolist(), ends.tolist())):
        dist = np.float32(0)
        while x != end:
            dist = np.float32(float(dist) + step(x, nxt[x]))
            x = nxt[x]
        dists[i] = dist
    return dists


@pytest.fixture(scope="module")
def edges_found(oracle):
    found = Counter()
    for seed in P.SEEDS:
        c = P.raster_case(oracle, seed)
        flood_edges(c, found)
        sum_edges(c, found)
        ucat_edges(c, found)
        snap_edges(oracle, c, found)
    return found


@pytest.mark.parametrize("edge", EDGES)
def test_fuzz_inputs_reach_the_edge(edges_found, edge):
    assert edges_found[edge] > 0, dict(edges_found)
