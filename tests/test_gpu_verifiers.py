"""The oracle-free verifiers — pfd_verify_upstream_area_cell / _basins / _hand (csrc/checks.hip), the verify mode of every
pfd_*_block sweep (k_verify_up / k_verify_down, csrc/sweeps.hip) and pfd_checksum_i32 — against the independent numpy
restatement of the local equations (tests/local_equations.py, pinned by tests/test_local_equations.py).  These kernels are
the only all-cell evidence for results beyond the sizes the oracle reaches, and the block verifiers compute their
expected values through the rules the engines use: what pins them is that, for the correct result and for every mutated
one (tests/verifier_cases.py), EVERY count the device reports equals the restatement's, exactly — candidate in host
memory and in device memory."""
import numpy as np
import pytest

import local_equations as LE
import verifier_cases as VC
from golden_util import Case, derived_inputs

pytestmark = pytest.mark.gpu

MEMSPACES = ("host", "device")


class _Dev:
    """Arrays uploaded for one call with memspace PFD_DEVICE (released afterwards)."""

    def __init__(self, hip, on_device):
        self.hip, self.on, self.bufs = hip, on_device, []

    def __call__(self, arr):
        if arr is None or not self.on:
            return arr
        arr = np.ascontiguousarray(arr)
        buf = self.hip.DeviceBuffer(max(arr.nbytes, 8)).upload(arr)
        self.bufs.append(buf)
        return buf

    def free(self):
        for b in self.bufs:
            b.free()


def _verify_whole(hip, h, op, a, where):
    dev = _Dev(hip, where == "device")
    ms = hip.PFD_DEVICE if where == "device" else hip.PFD_HOST
    try:
        if op == "upa":
            return h.verify_upstream_area_cell(dev(a["upa"]), ms)
        if op == "labels":
            return h.verify_basins(a["outlets"], a["ids"], dev(np.ascontiguousarray(a["lab"], dtype=np.uint32)), ms)
        return h.verify_hand(dev(a["drain"]), dev(a["elev"]), hip._PAYLOAD_CODE[a["elev"].dtype], dev(a["hand"]), ms)
    finally:
        dev.free()


@pytest.mark.parametrize("op", ["upa", "labels", "hand_f32", "hand_f64"])
@pytest.mark.parametrize("name", VC.RASTERS)
def test_whole_raster_verifiers_count_what_the_restatement_counts(gpu_lib, oracle, name, op):
    """Rasters from 5 x 7 to 32771 x 70: the last makes the grid-stride loop of the three kernels take a second and a
    partial last iteration (rows from 32768 on), with a column block of 6 live lanes; the mutations sit there."""
    from pyflwdir_amd import _hip

    R = VC.raster(oracle, name)
    base, muts = VC.whole_raster_cases(oracle, R, op)
    h = _hip.RasterHandle(R.d8, R.shape[0], R.shape[1])
    try:
        for label, args in [("unmutated", base)] + [(f"{m.cls}:{m.label}", m.args) for m in muts]:
            exp = VC.restate_whole(R, op, args)
            for where in MEMSPACES:
                got = _verify_whole(_hip, h, op, args, where)
                print(name, op, label, where, got, exp)
                assert got == exp, (name, op, label, where)
    finally:
        h.close()


def test_whole_raster_verifiers_on_cycles(gpu_lib, oracle, manifest):
    """synth_loops_96x80 with the reference's own results: the cells of the cycles break their equations (the reference
    never visits them), and the device counts exactly those."""
    from pyflwdir_amd import _hip

    case = Case("synth_loops_96x80", manifest)
    idxs_ds, idxs_pit, _ = oracle.from_array(case.d8)
    R = VC.Cyclic(case.d8, idxs_ds, case.shape)
    g = R.g
    upa = case.full["uparea_cell"].ravel()
    D = derived_inputs(case, upa.reshape(case.shape), idxs_pit)
    ids = np.arange(1, idxs_pit.size + 1, dtype=np.uint32)
    lab = np.ascontiguousarray(case.full["basins"].ravel(), dtype=np.uint32)
    # a cycle's cells hold 0, each the label of its downstream cell; one of them relabelled breaks that round the cycle
    lab2 = lab.copy()
    lab2[np.flatnonzero(g.valid & (lab == 0))[0]] = 9
    cases = [("upa", dict(upa=upa), True), ("labels", dict(outlets=idxs_pit, ids=ids, lab=lab), False),
             ("labels", dict(outlets=idxs_pit, ids=ids, lab=lab2), True),
             ("hand_f32", dict(drain=D["drain"].ravel().astype(np.uint8), elev=D["elevtn"].ravel(),
                               hand=case.full["hand_f32"].ravel()), True)]
    h = _hip.RasterHandle(case.d8, case.shape[0], case.shape[1])
    try:
        for op, args, positive in cases:
            exp = VC.restate_whole(R, op, args)
            assert (exp["bad_cells"] > 0) == positive, (op, exp)
            for where in MEMSPACES:
                assert _verify_whole(_hip, h, op, args, where) == exp, (op, where)
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------
# row-block verifiers
# ---------------------------------------------------------------------------------------------
def _verify_block(hip, h, op, a, where):
    """The device's count of own cells failing their local equation."""
    dev = _Dev(hip, where == "device")
    ms = hip.PFD_DEVICE if where == "device" else hip.PFD_HOST
    i, seed = a["inputs"], a["seed"]
    kind = op.split("_")
    try:
        out = dev(a["out"].copy())  # (the call writes the seeds into the halo rows of a device-resident candidate)
        if kind[0] == "accu":
            nd = "nd" in kind
            rows = "rows" in kind
            return h.accuflux_block(i["data"] if rows else dev(i["data"]), hip._PAYLOAD_CODE[a["out"].dtype], seed, out, -9999, -9999.0,
                                    1 if nd else 0, by_row=rows, verify=True, memspace=ms,
                                    direction=hip.PFD_DOWN if kind[1] == "down" else hip.PFD_UP)[1]
        if kind[0] == "fill":
            f32 = a["out"].dtype == np.float32
            how = {"max": hip.PFD_FILL_MAX, "min": hip.PFD_FILL_MIN, "sum": hip.PFD_FILL_SUM}["max" if kind[1] == "up" else kind[2]]
            return h.fillnodata_block(dev(i["data"]), hip._PAYLOAD_CODE[a["out"].dtype], seed, out, 0 if not f32 else -9999,
                                      -9999.0 if f32 else 0.0, 1, direction=hip.PFD_UP if kind[1] == "up" else hip.PFD_DOWN,
                                      how=how, verify=True, memspace=ms)[1]
        if kind[0] == "strahler":
            return h.strahler_block(dev(i["mask"]), seed, out, verify=True, memspace=ms)[1]
        if kind[0] == "dist":
            return h.stream_distance_block(dev(i["mask"]), i["steps"], seed, out, verify=True, memspace=ms)[1]
        if kind[0] == "classic":
            return h.stream_order_classic_block(dev(i["tinfo"]), dev(i["mask"]), seed, out, verify=True, memspace=ms)[1]
        return h.floodplains_block(dev(i["elev"]), hip._PAYLOAD_CODE[i["elev"].dtype], dev(i["stream"]), dev(i["h"]), seed, out,
                                   verify=True, memspace=ms)[1]
    finally:
        dev.free()


def _run_block_cases(hip, oracle, B, nblocks, op):
    for b in range(nblocks):
        blk = VC.Block(B, nblocks, b)
        base, muts = VC.block_cases(oracle, B, blk, op)
        h = hip.RasterHandle(B.d8[blk.a:blk.e], blk.own_rows, blk.ncol, halo=blk.halo)
        try:
            for label, args in [("unmutated", base)] + [(f"{m.cls}:{m.label}", m.args) for m in muts]:
                exp = VC.restate_block(B, blk, op, args)
                for where in MEMSPACES:
                    got = _verify_block(hip, h, op, args, where)
                    print(op, nblocks, b, label, where, got, exp)
                    assert got == exp, (op, nblocks, b, label, where)
        finally:
            h.close()


@pytest.mark.parametrize("nblocks", [2, 3])
@pytest.mark.parametrize("op", VC.BLOCK_OPS)
def test_block_verifiers_count_what_the_restatement_counts(gpu_lib, oracle, op, nblocks):
    """500 x 400 with nodata, cut into 2 and 3 row blocks (the middle one of three has both halos; no block's own cells
    are a multiple of 64 or 256): every verify mode against the restatement — the first and the last own cell, cells
    whose upstream or downstream cell is a halo seed, nodata cells (never counted), -0.0 and NaN payloads (bitwise)."""
    from pyflwdir_amd import _hip

    _run_block_cases(_hip, oracle, VC.block_raster(oracle), nblocks, op)


def test_block_verifiers_on_cycles(gpu_lib, oracle, manifest):
    """k_verify_up and k_verify_down on synth_loops_96x80 (a whole-raster handle, the level structure: a raster with cycles
    has no plan) with the reference's accuflux results: the cells of the cycles, which the reference never visits, are
    counted as the restatement counts them."""
    from pyflwdir_amd import _hip
    from oracle import golden_inputs as GI

    case = Case("synth_loops_96x80", manifest)
    idxs_ds, _, _ = oracle.from_array(case.d8)
    g = LE.Graph(idxs_ds, case.shape)
    data = np.ascontiguousarray(GI.payloads(case.shape)["w32"].ravel())
    h = _hip.RasterHandle(case.d8, case.shape[0], case.shape[1])
    try:
        for op, key, fn in (("accu_up_f32_nd", "accuflux_f32", LE.accuflux_up), ("accu_down_f32_nd", "accuflux_ds_f32", LE.accuflux_down)):
            out = np.ascontiguousarray(case.full[key].ravel())
            exp = int(fn(g, data, out, nodata=-9999)[0].sum())
            assert exp > 0
            args = dict(out=out, seed=np.zeros(2 * case.shape[1], np.float32), inputs=dict(data=data))
            for where in MEMSPACES:
                assert _verify_block(_hip, h, op, args, where) == exp, (op, where)
    finally:
        h.close()


@pytest.mark.parametrize("op", ["accu_up_f32_nd", "fill_down_sum_f32", "strahler_mask"])
def test_up_block_verifiers_on_the_level_structure(gpu_lib, oracle, monkeypatch, op):
    """k_verify_up reads the upstream masks of the block's plan; under PFD_BLOCK_LEVELS those of the level structure."""
    from pyflwdir_amd import _hip

    monkeypatch.setenv("PFD_BLOCK_LEVELS", "1")
    _run_block_cases(_hip, oracle, VC.block_raster(oracle), 3, op)


@pytest.mark.parametrize("name", ["tiny_5x7", "onerow_1x300", "onecol_300x1", "rand_63x65", "synth_130x70"])
def test_block_verifiers_on_whole_raster_handles(gpu_lib, oracle, name):
    """A whole-raster handle is a block without halos: the small shapes, every operation."""
    from pyflwdir_amd import _hip

    for op in VC.BLOCK_OPS:
        _run_block_cases(_hip, oracle, VC.raster(oracle, name), 1, op)


# ---------------------------------------------------------------------------------------------
# pfd_checksum_i32
# ---------------------------------------------------------------------------------------------
def test_checksum_i32_is_numpys_sum(gpu_lib):
    from pyflwdir_amd import _hip

    rng = np.random.default_rng(11)
    nmax = 4096 * 256 + 1
    odd = 333  # one row of odd length: the pointer is no longer 8- or 16-byte aligned
    v = rng.integers(-2**31, 2**31, nmax + odd, dtype=np.int64).astype(np.int32)
    buf = _hip.DeviceBuffer(v.nbytes).upload(v)
    try:
        for n in (0, 1, 255, 256, 257, nmax):
            assert _hip.checksum_i32(buf, n) == int(v[:n].sum(dtype=np.int64)), n
            assert _hip.checksum_i32(buf.addr + 4 * odd, n) == int(v[odd:odd + n].sum(dtype=np.int64)), n
        neg = np.full(70000, -2**31, np.int32)  # (the sum leaves 32 bits: -2^31 * 70000)
        buf.upload(neg)
        assert _hip.checksum_i32(buf, neg.size) == -2**31 * 70000
    finally:
        buf.free()
