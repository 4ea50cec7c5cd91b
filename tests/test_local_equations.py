"""Pins tests/local_equations.py — the numpy restatement of the sweeps' local equations that the device verifiers are
compared with (tests/test_gpu_verifiers.py) — before anything trusts it: it accepts every result the reference recorded
(tests/golden) and every result of the oracle on the rasters the GPU test uses, it objects to the reference's own result
on the raster with cycles, and every mutation the GPU test applies makes it flag at least one cell — exactly the stated
set where the class states one — so that no device count is compared with a vacuous zero."""
import numpy as np
import pytest

import local_equations as LE
import verifier_cases as VC
from conftest import case_names
from golden_util import Case, derived_inputs
from oracle import golden_inputs as GI
from serial_refs import _ref_down, _ref_floodplains, _ref_up

CASES = case_names()


def _n(maps):
    return int(maps[0].sum()), int(maps[1].sum())


@pytest.fixture(scope="module", params=CASES)
def solved(request, manifest, oracle):
    case = Case(request.param, manifest)
    idxs_ds, idxs_pit, _ = oracle.from_array(case.d8)
    seq = oracle.idxs_seq(idxs_ds, idxs_pit)
    return case, idxs_ds, idxs_pit, seq, LE.Graph(idxs_ds, case.shape)


def test_graph_of_d8_is_the_reference_decode(solved):
    case, idxs_ds, idxs_pit, seq, g = solved
    assert np.array_equal(LE.graph_of_d8(case.d8), idxs_ds.astype(np.int64))
    assert np.array_equal(np.flatnonzero(g.pit), idxs_pit)


def test_restatement_accepts_the_recorded_results(solved, oracle):
    """Zero flagged cells on the reference's outputs (the recorded arrays where tests/golden holds them, else the oracle's,
    which tests/test_oracle_golden.py pins to the recorded digests).  Cells off the sequence — the cycles of
    synth_loops_96x80 — are left out here: the reference never visits them (see the next test)."""
    O = oracle
    case, idxs_ds, idxs_pit, seq, g = solved
    shape = case.shape
    on_seq = np.zeros(g.n, bool)
    on_seq[seq] = True

    def ok(maps, what):
        bad, bad_nodata = maps
        assert int((bad & on_seq).sum()) == 0 and int(bad_nodata.sum()) == 0, (case.name, what)

    def rec(key, compute):
        return (case.full[key] if key in case.full else compute()).ravel()

    acc = lambda w, **kw: O.accuflux(idxs_ds, seq, np.ascontiguousarray(w.ravel()), **kw)
    upa = rec("uparea_cell", lambda: O.upstream_area_cell(case.d8)[0])
    ok(LE.upa_cell(g, upa), "upa")
    st = LE.upa_cell_stats(g, upa)
    assert st["n_valid"] == case.entry["stats"]["n_valid"] and st["n_pits"] == idxs_pit.size
    if seq.size == st["n_valid"]:
        assert st["pit_sum"] == st["n_valid"]  # (reference tests/test_streams_basins.py:24-27)
    P = GI.payloads(shape)
    for key, w, nd, down in (("accuflux_f32", "w32", -9999, False), ("accuflux_f64", "w64", -9999, False),
                             ("accuflux_ds_f32", "w32", -9999, True), ("accuflux_i32_nodata", "wi32_nodata", -9999, False),
                             ("accuflux_ds_i32_nodata", "wi32_nodata", -9999, True),
                             ("accuflux_f32_nodata_m1", "wf32_nodata_m1", -1, False), ("accuflux_i64", "wi64", -9999, False)):
        out = rec(key, lambda: acc(P[w], nodata=nd, direction="down" if down else "up"))
        ok((LE.accuflux_down if down else LE.accuflux_up)(g, P[w], out, nodata=nd), key)
    D = derived_inputs(case, upa.reshape(shape), idxs_pit)
    for key, mask in (("strahler", None), ("strahler_mask_upa", D["mask_upa"]), ("strahler_mask_rand", D["mask_rand"])):
        m = None if mask is None else mask.ravel()
        ok(LE.strahler(g, rec(key, lambda: O.strahler_order(idxs_ds, seq, m)), m), key)
    ids = np.arange(1, idxs_pit.size + 1, dtype=np.uint32)
    ok(LE.labels(g, idxs_pit, ids, rec("basins", lambda: O.basins(idxs_ds, idxs_pit, seq))), "basins")
    sub = rec("basins_sub_i16", lambda: O.basins(idxs_ds, D["basins_idxs"], seq, D["basins_ids"]))
    ok(LE.labels(g, D["basins_idxs"], D["basins_ids"].astype(np.uint32), sub.astype(np.uint32)), "basins_sub")
    e32 = D["elevtn"].ravel()
    e64 = (D["elevtn"].astype(np.float64) * 1.000001).ravel()
    drain = D["drain"].ravel()
    ok(LE.hand(g, drain, e32, rec("hand_f32", lambda: O.height_above_nearest_drain(idxs_ds, seq, drain, e32))), "hand_f32")
    ok(LE.hand(g, drain, e64, rec("hand_f64", lambda: O.height_above_nearest_drain(idxs_ds, seq, drain, e64))), "hand_f64")
    main = rec("idxs_us_main", lambda: O.main_upstream(idxs_ds, upa))
    for key, mask in (("strord_classic", None), ("strord_classic_mask", D["mask_upa"])):
        m = None if mask is None else mask.ravel()
        out = rec(key, lambda: O.stream_order_classic(idxs_ds, seq, main, m))
        ok(LE.classic_order(g, LE.trib_info(g, main, m), out, m), key)
    for key, mask in (("strdist_cell", None), ("strdist_cell_mask", D["mask_upa"])):
        m = None if mask is None else mask.ravel()
        out = rec(key, lambda: O.stream_distance(idxs_ds, seq, shape[1], mask=m, real_length=False))
        ok(LE.stream_distance(g, out, m), key)
    for key, mask, latlon, tr in (("strdist_m_latlon", None, case.latlon, case.transform),
                                  ("strdist_m_proj", None, False, GI.PROJ_TRANSFORM),
                                  ("strdist_m_mask", D["mask_rand"], case.latlon, case.transform)):
        if key not in case.digests:
            continue
        m = None if mask is None else mask.ravel()
        out = rec(key, lambda: O.stream_distance(idxs_ds, seq, shape[1], mask=m, latlon=latlon, transform=tr))
        ok(LE.stream_distance(g, out, m, O.step_length_table(shape[0], latlon, tr)), key)


def test_restatement_accepts_the_serial_loops_of_fillnodata_and_floodplains(solved, oracle):
    """fillnodata and floodplains have no recorded arrays per golden case: their serial loops (tests/serial_refs.py, pinned
    by tests/test_serial_refs.py) give the results the restatement must accept."""
    case, idxs_ds, idxs_pit, seq, g = solved
    if g.n > 40000:
        return  # (serial Python loops: the row-block raster of the last test is the large case)
    on_seq = np.zeros(g.n, bool)
    on_seq[seq] = True
    rng = np.random.default_rng(5)
    f32 = np.where(rng.random(g.n) < 0.4, np.float32(-9999), rng.integers(-8, 9, g.n).astype(np.float32) / 4)
    i32 = np.where(rng.random(g.n) < 0.4, 0, rng.integers(-5, 1000, g.n)).astype(np.int32)
    for data, nd in ((f32, -9999.0), (i32, 0)):
        bad, bn = LE.fillnodata_up(g, data, _ref_up(idxs_ds, seq, data, nd), nd)
        assert not (bad & on_seq).any() and not bn.any()
        for how in ("max", "min", "sum"):
            bad, bn = LE.fillnodata_down(g, data, _ref_down(idxs_ds, seq, data, nd, how), nd, how)
            assert not (bad & on_seq).any() and not bn.any(), how
    upa = oracle.upstream_area_cell(case.d8)[0].ravel().astype(np.float64)
    for elev in (rng.random(g.n).astype(np.float32) * 20, rng.random(g.n) * 20):
        stream, h = upa >= 5.0, (upa.clip(0) ** 0.3).astype(np.float32)
        st = VC.flood_state(idxs_ds, seq, elev, stream, h)
        flags = np.where(on_seq, st["flag"], -1)
        assert np.array_equal(flags, _ref_floodplains(idxs_ds, seq, elev, upa, 5.0, 0.3))
        bad, bn = LE.floodplains_state(g, elev, stream, h, st)
        assert not (bad & on_seq).any() and not bn.any()


def test_restatement_objects_to_the_cycles(manifest, oracle):
    """The reference never visits the cells of a cycle (they are on no pit's sequence): its own results break the local
    equations there, and the restatement says so."""
    case = Case("synth_loops_96x80", manifest)
    idxs_ds, idxs_pit, _ = oracle.from_array(case.d8)
    g = LE.Graph(idxs_ds, case.shape)
    assert _n(LE.upa_cell(g, case.full["uparea_cell"]))[0] > 0
    ids = np.arange(1, idxs_pit.size + 1, dtype=np.uint32)
    assert _n(LE.labels(g, idxs_pit, ids, case.full["basins"]))[0] == 0  # (0 round a cycle satisfies "my downstream cell's")
    assert _n(LE.accuflux_up(g, GI.payloads(case.shape)["w32"], case.full["accuflux_f32"], nodata=-9999))[0] > 0
    assert _n(LE.accuflux_down(g, GI.payloads(case.shape)["w32"], case.full["accuflux_ds_f32"], nodata=-9999))[0] > 0


# ---------------------------------------------------------------------------------------------
# the rasters and mutations of tests/test_gpu_verifiers.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.RASTERS)
def test_generated_rasters_have_the_stated_features(oracle, name):
    R = VC.raster(oracle, name)
    nrow, ncol = R.shape
    assert np.array_equal(LE.graph_of_d8(R.d8), R.idxs_ds.astype(np.int64))
    if name.startswith(("synth", "rand", "tall")):
        off, into = VC.leaves_raster(R.d8)
        assert off.any() and into.any(), "flow off the raster edge and into nodata"
    if name.startswith("tall"):
        assert nrow > 32768 + 2 and ncol % 64 != 0
        for k in range(8):
            assert VC.named_cells(R)[f"drains_{k}"] is not None
    if name == "synth_130x70":
        assert ncol - 64 == 6


@pytest.mark.parametrize("name", VC.RASTERS)
@pytest.mark.parametrize("op", ["upa", "labels", "hand_f32", "hand_f64"])
def test_whole_raster_mutations_are_seen(oracle, name, op):
    R = VC.raster(oracle, name)
    base, muts = VC.whole_raster_cases(oracle, R, op)
    b0 = VC.restate_whole(R, op, base)
    assert b0["bad_cells"] == 0 and b0["bad_nodata"] == 0
    assert len(muts) >= 5
    classes = set()
    for m in muts:
        st = VC.restate_whole(R, op, m.args)
        classes.add(m.cls)
        assert st["bad_cells"] + st["bad_nodata"] >= m.at_least, (name, op, m.label, st)
        if m.expect is not None:
            bad, bad_nodata = VC.restate_whole_maps(R, op, m.args)
            assert set(np.flatnonzero(bad).tolist()) == set(m.expect), (name, op, m.label)
        if m.expect_nodata is not None:
            assert st["bad_nodata"] == m.expect_nodata and st["bad_cells"] == 0, (name, op, m.label)
        if m.pit_sum_moves:
            assert st["pit_sum"] != st["n_valid"], (name, op, m.label)
    assert "M1" in classes and "M3" in classes
    if name in ("tall_32771x70", "synth_130x70", "rand_130x70"):  # (these have nodata, confluences and drain cells)
        want = {"upa": {"M1", "M2", "M3", "M4"}, "labels": {"M1", "M3", "M4", "M6"}}.get(op, {"M1", "M3", "M4", "M5", "M6"})
        assert classes == want, (name, op, classes)
        if op.startswith("hand"):
            assert {"minus_zero", "nan_payload", "nan_gone", "drain_flag", "elevation"} <= {m.label for m in muts}
    if name.startswith("tall") or name == "synth_130x70":
        # the single-count-in-millions case sits in the partial column block, and on the tall raster in a later stride
        # iteration of the whole-raster kernels
        late = [divmod(x, R.shape[1]) for m in muts if m.cls == "M3" and m.expect for x in m.expect]
        assert any(c >= 64 and (r >= 32768 or not name.startswith("tall")) for r, c in late), late


@pytest.mark.parametrize("nblocks,name", [(2, None), (3, None), (1, "tiny_5x7"), (1, "onerow_1x300"), (1, "onecol_300x1"),
                                          (1, "rand_63x65"), (1, "synth_130x70")])
@pytest.mark.parametrize("op", VC.BLOCK_OPS)
def test_block_mutations_are_seen(oracle, op, nblocks, name):
    B = VC.block_raster(oracle) if name is None else VC.raster(oracle, name)
    for b in range(nblocks):
        blk = VC.Block(B, nblocks, b)
        assert name is not None or (blk.n_own % 64 != 0 and blk.n_own % 256 != 0)
        base, muts = VC.block_cases(oracle, B, blk, op)
        assert VC.restate_block(B, blk, op, base) == 0, (op, b)
        assert len(muts) >= 3
        if name is None:  # the 500 x 400 raster: every class that applies to the operation is there
            labels = {f"{m.cls}:{m.label}" for m in muts}
            kind = op.split("_")
            integer = base["out"].dtype.kind in "iu"
            want = {"M1:first_own", "M1:last_own", "M4:nodata", "M6:halo_seed"}
            if kind[0] == "accu" and kind[1] == "up" and integer:
                want |= {"M2:pair", "M3:path"}
            if integer and (kind[0] in ("dist", "classic") or kind[:2] == ["accu", "down"]):
                want |= {"M3:subtree"}
            if op in ("accu_up_f32_nd", "accu_down_f32_nd"):
                want |= {"M5:minus_zero", "M5:nan_payload"}
            if kind[0] in ("accu", "fill"):
                want |= {"M6:payload"}
            if "mask" in kind:
                want |= {"M6:mask"}
            if op == "strahler_mask":
                want |= {"M6:mask_in"}
            if kind[:2] == ["dist", "m"]:
                want |= {"M6:steps"}
            if kind[0] == "classic":
                want |= {"M6:tinfo"}
            if kind[0] == "flood":
                want |= {"M6:stream", "M6:elev"}
            assert want <= labels, (op, b, want - labels)
        for m in muts:
            n = VC.restate_block(B, blk, op, m.args)
            assert n >= m.at_least, (op, b, m.label, n)
            if m.expect_count is not None:
                assert n == m.expect_count, (op, b, m.label, n)
    assert nblocks == 2 or VC.Block(B, 3, 1).halo == (1, 1)
