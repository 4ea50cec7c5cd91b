"""``resident=True`` and ``DeviceArray`` arguments on the sweeps of ``FlwdirRaster``: every call of the list gives, once
downloaded, the bytes of the numpy path (and of the recorded golden where there is one), whether its inputs are device
arrays, numpy arrays or a mix; a chain of calls moves nothing per-cell over PCIe; calls of both kinds can follow each
other at once; and the numpy path of the same handle is what it was."""
import numpy as np
import pytest

from golden_util import Case, derived_inputs
from oracle import golden_inputs as GI

pytestmark = pytest.mark.gpu

CASES = ["rhine", "synth_river_256", "synth_loops_96x80", "synth_rough_nodata_384x512", "synth_onerow_1x300"]
# result key -> key of the recorded golden of the same call with the same inputs
GOLDEN = {"uparea_cell": "uparea_cell", "uparea_km2": "uparea_km2_latlon", "accuflux_f32": "accuflux_f32",
          "accuflux_f64": "accuflux_f64", "accuflux_ds_i32": "accuflux_ds_i32_nodata", "accuflux_i64": "accuflux_i64",
          "strahler": "strahler", "strahler_mask": "strahler_mask_upa", "strdist_cell": "strdist_cell",
          "strdist_cell_mask": "strdist_cell_mask", "strdist_m_mask": "strdist_m_mask", "basins": "basins",
          "hand_f32": "hand_f32", "hand_f64": "hand_f64"}


def same_bytes(got, want, what=""):
    """Byte equality (so NaNs are compared by position and payload), with dtype and shape."""
    assert isinstance(got, np.ndarray), (what, type(got))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.ravel() != want.ravel())
        raise AssertionError(f"{what}: {bad.size} cells differ, first {bad[:5]}: got {got.ravel()[bad[:5]]} "
                             f"expected {want.ravel()[bad[:5]]}")


def make_flw(case, cache=False):
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd._affine import Affine

    return pyflwdir.from_array(case.d8, ftype="d8", transform=Affine(*case.transform), latlon=case.latlon, cache=cache)


def inputs_of(case, flw):
    upa = flw.upstream_area()
    D = derived_inputs(case, upa, flw.idxs_pit)
    P = GI.payloads(case.shape)
    rng = np.random.default_rng(5)
    fill_f32 = P["w32"].copy()
    fill_f32[rng.random(case.shape) < 0.7] = -9999.0
    fill_i32 = (P["w32"] * 1000).astype(np.int32)
    fill_i32[rng.random(case.shape) < 0.7] = -1
    I = dict(w32=P["w32"], w64=P["w64"], wi32_nodata=P["wi32_nodata"], wi64=P["wi64"], wu32=P["wi32_nodata"].view(np.uint32),
             fill_f32=fill_f32, fill_i32=fill_i32, mask_upa=D["mask_upa"], mask_rand_f32=D["mask_rand"].astype(np.float32) * 2.5,
             drain=D["drain"], drain_i32=D["drain"].astype(np.int32) * 1 + (upa > 3 * D["thr"]),  # (holds 0, 1 and 2)
             elevtn=D["elevtn"], elevtn_f64=D["elevtn"].astype(np.float64) * 1.000001,
             elevtn_i32=(D["elevtn"] * 10).astype(np.int32), elevtn_u8=(D["elevtn"] % 200).astype(np.uint8),
             strord_u8=(upa % 5).astype(np.uint8))
    for a in I.values():
        a.setflags(write=False)
    I["_basins"] = (D["basins_idxs"], D["basins_ids"].astype(np.int32))
    return I


def run_calls(flw, A, resident):
    """Every call of the list, with its per-cell inputs taken from ``A`` (numpy or device arrays)."""
    kw = dict(resident=True) if resident else {}
    idxs, ids = A["_basins"]
    out = {}
    out["uparea_cell"] = flw.upstream_area(**kw)
    out["uparea_km2"] = flw.upstream_area("km2", **kw)
    out["uparea_km2_fixed"] = flw.upstream_area("km2", exact=False, **kw)
    out["accuflux_f32"] = flw.accuflux(A["w32"], **kw)
    out["accuflux_f64"] = flw.accuflux(A["w64"], **kw)
    out["accuflux_ds_i32"] = flw.accuflux(A["wi32_nodata"], nodata=-9999, direction="down", **kw)
    out["accuflux_i64"] = flw.accuflux(A["wi64"], **kw)
    out["accuflux_u32"] = flw.accuflux(A["wu32"], nodata=7, **kw)
    out["fill_down_max"] = flw.fillnodata(A["fill_f32"], -9999.0, direction="down", how="max", **kw)
    out["fill_down_sum"] = flw.fillnodata(A["fill_i32"], -1, direction="down", how="sum", **kw)
    out["fill_up"] = flw.fillnodata(A["fill_f32"], -9999.0, direction="up", **kw)
    out["upstream_sum_f32"] = flw.upstream_sum(A["w32"], **kw)
    out["upstream_sum_i32"] = flw.upstream_sum(A["wi32_nodata"], mv=-9999, **kw)
    out["strahler"] = flw.stream_order(**kw)
    out["strahler_mask"] = flw.stream_order(mask=A["mask_upa"], **kw)
    out["strahler_mask_f32"] = flw.stream_order(mask=A["mask_rand_f32"], **kw)
    out["strdist_cell"] = flw.stream_distance(**kw)
    out["strdist_cell_mask"] = flw.stream_distance(mask=A["mask_upa"], **kw)
    out["strdist_m_mask"] = flw.stream_distance(mask=A["mask_rand_f32"], unit="m", **kw)
    out["basins"] = flw.basins(**kw)
    out["basins_sub_i32"] = flw.basins(idxs=idxs, ids=ids, **kw)
    out["hand_f32"] = flw.hand(A["drain"], A["elevtn"], **kw)
    out["hand_f64"] = flw.hand(A["drain"], A["elevtn_f64"], **kw)
    out["hand_i32_drain_i32_elev"] = flw.hand(A["drain_i32"], A["elevtn_i32"], **kw)
    out["hand_u8_elev"] = flw.hand(A["drain"], A["elevtn_u8"], **kw)
    out["downstream_f64"] = flw.downstream(A["w64"], **kw)
    out["downstream_u8"] = flw.downstream(A["strord_u8"], **kw)
    out["downstream_bool"] = flw.downstream(A["mask_upa"], **kw)
    return out


@pytest.fixture(scope="module", params=CASES)
def setup(request, manifest, gpu_lib):
    """(case, raster, numpy inputs, the numpy path's results) — computed once per golden and left unchanged."""
    case = Case(request.param, manifest)
    flw = make_flw(case)
    I = inputs_of(case, flw)
    ref = run_calls(flw, I, resident=False)
    for k, v in ref.items():
        assert isinstance(v, np.ndarray), k
        v.setflags(write=False)
    return case, flw, I, ref


def as_device(I, names, device=0):
    from pyflwdir_amd import to_device

    return {k: (to_device(v, device) if k in names else v) for k, v in I.items()}


FORMS = {"device": lambda I: {k for k in I if not k.startswith("_")}, "numpy": lambda I: set(),
         "mixed": lambda I: {"drain", "drain_i32", "mask_upa", "w32", "fill_i32", "elevtn_f64", "strord_u8"}}


def test_numpy_path_is_the_golden(setup):
    """What the resident results are compared with is itself the recorded reference wherever ``tests/golden`` has it."""
    case, flw, I, ref = setup
    checked = 0
    for key, gold in GOLDEN.items():
        if gold in case.digests:
            case.check(gold, ref[key])
            checked += 1
    assert checked >= 10


@pytest.mark.parametrize("form", list(FORMS))
def test_resident_calls_equal_the_numpy_path(setup, form):
    from pyflwdir_amd import DeviceArray

    case, flw, I, ref = setup
    A = as_device(I, FORMS[form](I))
    got = run_calls(flw, A, resident=True)
    assert set(got) == set(ref)
    for key, dev in got.items():
        assert isinstance(dev, DeviceArray) and dev.device == 0, key
        same_bytes(dev.numpy(), ref[key], f"{case.name}:{key}:{form}")
        if GOLDEN.get(key) in case.digests:
            case.check(GOLDEN[key], dev.numpy())


def test_device_arguments_without_resident_return_numpy(setup):
    """Independently of ``resident``: a DeviceArray argument is taken wherever an array is, the result comes back as numpy."""
    case, flw, I, ref = setup
    A = as_device(I, FORMS["mixed"](I))
    got = run_calls(flw, A, resident=False)
    for key, arr in got.items():
        same_bytes(arr, ref[key], f"{case.name}:{key}")


# ---- the chain -----------------------------------------------------------------------------------------------------------
UPA_MIN, STO_MIN = 20, 2


def chain_numpy(flw, elevtn):
    upa = flw.upstream_area("cell")
    sto = flw.stream_order(mask=upa > UPA_MIN)
    return flw.hand(sto >= STO_MIN, elevtn)


def chain_resident(flw, elevtn_dev, between=None):
    upa = flw.upstream_area("cell", resident=True)
    between and between()
    mask = upa > UPA_MIN
    between and between()
    sto = flw.stream_order(mask=mask, resident=True)
    between and between()
    drain = sto >= STO_MIN
    between and between()
    return flw.hand(drain, elevtn_dev, resident=True)


@pytest.fixture(scope="module")
def river(manifest, gpu_lib):
    case = Case("synth_river_256", manifest)
    flw = make_flw(case)
    elevtn = GI.elevation(case.elevtn_in, flw.upstream_area())
    want = chain_numpy(flw, elevtn)
    want.setflags(write=False)
    assert np.count_nonzero(want == 0) > 100 and np.count_nonzero(want > 0) > 1000  # (a chain with drains and hillslopes)
    return case, flw, elevtn, want


def test_chain_stays_on_the_device(river):
    from pyflwdir_amd import _hip, to_device

    case, flw, elevtn, want = river
    n = case.n
    n_pits = flw.idxs_pit.size
    assert n_pits == case.entry["stats"]["n_pits"] == 69  # few pits: the outlet lists are far below a byte per cell
    elevtn_dev = to_device(elevtn)
    # two accounts together are ALL host <-> device traffic: the staging copies inside the library's calls
    # (pfd_transfer_stats) and the copies DeviceArray itself makes in to_device / .numpy() (buffer_transfer_stats)
    _hip.buffer_transfer_stats(reset=True)
    assert _hip.buffer_transfer_stats(reset=False) == dict(h2d_bytes=0, h2d_copies=0, h2d_ms=0, d2h_bytes=0, d2h_copies=0, d2h_ms=0)
    to_device(np.zeros(3, np.int32)).numpy()  # (the second account sees what it is there for)
    seen = _hip.buffer_transfer_stats(reset=True)
    assert (seen["h2d_bytes"], seen["h2d_copies"], seen["d2h_bytes"], seen["d2h_copies"]) == (12, 1, 12, 1)
    _hip.transfer_stats(reset=True)  # the inputs are on the device
    hand = chain_resident(flw, elevtn_dev)
    st, sb = _hip.transfer_stats(reset=True), _hip.buffer_transfer_stats(reset=True)
    print("resident chain transfers:", st, sb)
    assert st["d2h_bytes"] == 0 and st["host_results"] == 0 and sb["d2h_bytes"] == 0 and sb["d2h_copies"] == 0
    assert sb["h2d_bytes"] == 0 and sb["h2d_copies"] == 0  # no DeviceArray went through the host on its way
    assert st["h2d_bytes"] < n  # less than one one-byte per-cell array
    bas = flw.basins(resident=True)  # (outlet lists) and
    dist = flw.stream_distance(mask=hand == 0, unit="m", resident=True)  # (a row table) may cross, nothing per-cell
    upa_km2 = flw.upstream_area("km2", resident=True)  # (one value per row)
    st, sb = _hip.transfer_stats(reset=True), _hip.buffer_transfer_stats(reset=True)
    print("more resident calls:", st, sb)
    assert st["d2h_bytes"] == 0 and st["host_results"] == 0 and sb["d2h_bytes"] == 0 and sb["h2d_bytes"] == 0
    assert 0 < st["h2d_bytes"] < n
    got = hand.numpy()  # the one download: the float64 HAND and nothing else
    st, sb = _hip.transfer_stats(reset=True), _hip.buffer_transfer_stats(reset=True)
    assert (sb["d2h_bytes"], sb["d2h_copies"], sb["h2d_bytes"]) == (n * 8, 1, 0) and st["d2h_bytes"] == 0 and st["h2d_bytes"] == 0
    same_bytes(got, want, "chain")
    same_bytes(bas.numpy(), flw.basins(), "basins")
    same_bytes(dist.numpy(), flw.stream_distance(mask=want == 0, unit="m"), "stream_distance")
    same_bytes(upa_km2.numpy(), flw.upstream_area("km2"), "upstream_area km2")
    # the numpy form of the same chain moves every link both ways
    _hip.transfer_stats(reset=True)
    _hip.buffer_transfer_stats(reset=True)
    chain_numpy(flw, elevtn)
    st, sb = _hip.transfer_stats(reset=True), _hip.buffer_transfer_stats(reset=True)
    assert st["d2h_bytes"] >= n * (4 + 1 + 8) and st["h2d_bytes"] >= n * (1 + 1 + 4)
    assert sb["d2h_bytes"] == 0 and sb["h2d_bytes"] == 0
    # mixed arguments: the numpy ones are uploaded (once each, as they are), the device ones never come down
    drain_dev = to_device(want == 0)
    _hip.transfer_stats(reset=True)
    _hip.buffer_transfer_stats(reset=True)
    mixed = flw.hand(drain_dev, elevtn, resident=True)
    st, sb = _hip.transfer_stats(reset=True), _hip.buffer_transfer_stats(reset=True)
    assert (sb["h2d_bytes"], sb["h2d_copies"], sb["d2h_bytes"]) == (n * 4, 1, 0) and st["d2h_bytes"] == 0 and st["h2d_bytes"] < n
    same_bytes(mixed.numpy(), want, "mixed hand")


def test_ordering_sweeps_and_elementwise_calls_follow_each_other(river):
    """The rule of include/pfd.h: a result is complete when its call returns, whichever stream computed it.  The chain
    alternates sweeps (the handle's stream) and elementwise calls (the null stream) twenty times on one handle, with an
    unrelated device array rewritten between the links by elementwise calls and never read."""
    from pyflwdir_amd import device_array as D

    case, flw, elevtn, want = river
    elevtn_dev = D.to_device(elevtn)
    other = D.to_device(np.arange(case.n, dtype=np.int64).reshape(case.shape))
    junk = []

    def between():
        k = len(junk)
        junk.append(D.where(other > 1000 * k, other, k))  # a different value every time; never read
        if len(junk) > 3:
            junk.pop(0)

    first = None
    for it in range(20):
        got = chain_resident(flw, elevtn_dev, between).numpy()
        if first is None:
            first = got
            same_bytes(first, want, "first iteration")
        assert got.tobytes() == first.tobytes(), f"iteration {it} differs from the first"


def test_default_path_is_unchanged_after_resident_calls(manifest, gpu_lib):
    case = Case("synth_river_256", manifest)
    flw = make_flw(case, cache=True)
    upa = flw.upstream_area(resident=True)
    sto_masked = flw.stream_order(mask=upa > UPA_MIN, resident=True)
    assert "strord" not in flw._cached  # a resident call does not write the cache
    flw.hand(sto_masked >= STO_MIN, GI.elevation(case.elevtn_in, upa.numpy()), resident=True)
    flw.basins(resident=True)
    # the plain numpy calls on the same handle still return the goldens
    upa_np = flw.upstream_area()
    case.check("uparea_cell", upa_np)
    Dv = derived_inputs(case, upa_np, flw.idxs_pit)
    sto = flw.stream_order()
    case.check("strahler", sto)
    assert flw._cached["strord"] is not None and np.array_equal(flw._cached["strord"].reshape(case.shape), sto)
    # ... a resident call does not read the cache either (the numpy call, like the reference, returns the cached order)
    same_bytes(flw.stream_order(mask=Dv["mask_upa"], resident=True).numpy(), case.full["strahler_mask_upa"]
               if "strahler_mask_upa" in case.full else make_flw(case).stream_order(mask=Dv["mask_upa"]), "masked")
    assert flw.stream_order(mask=Dv["mask_upa"]) is not None and np.array_equal(flw.stream_order(mask=Dv["mask_upa"]), sto)
    case.check("basins", flw.basins())
    case.check("hand_f32", flw.hand(Dv["drain"], Dv["elevtn"]))
    case.check("strdist_cell", flw.stream_distance())
    case.check("accuflux_f32", flw.accuflux(GI.payloads(case.shape)["w32"]))


def test_refusals(manifest, gpu_lib, monkeypatch):
    from pyflwdir_amd import to_device

    case = Case("synth_loops_96x80", manifest)
    flw = make_flw(case)
    n = case.n
    w32 = GI.payloads(case.shape)["w32"]
    # narrow-integer payloads: the host path widens and range-checks them with numpy
    for narrow in (np.int8, np.uint8, np.int16, np.uint16):
        with pytest.raises(NotImplementedError, match="without resident=True"):
            flw.accuflux(np.ones(case.shape, narrow), resident=True)
        with pytest.raises(NotImplementedError, match="without resident=True"):
            flw.fillnodata(np.ones(case.shape, narrow), 0, resident=True)
    with pytest.raises(NotImplementedError, match="without resident=True"):
        flw.accuflux(to_device(np.ones(case.shape, np.uint8)))
    with pytest.raises(NotImplementedError, match="without resident=True"):
        flw.fillnodata(to_device(np.ones(case.shape, np.int8)), 0)
    # a device array of the wrong size, and a freed one
    small = to_device(w32.ravel()[: n - 1])
    for call in (lambda a: flw.accuflux(a), lambda a: flw.fillnodata(a, -9999.0), lambda a: flw.upstream_sum(a),
                 lambda a: flw.stream_order(mask=a), lambda a: flw.stream_distance(mask=a), lambda a: flw.hand(a, w32),
                 lambda a: flw.hand(w32 > 0.5, a), lambda a: flw.downstream(a)):
        with pytest.raises(ValueError, match="size does not match"):
            call(small)
        gone = to_device(w32)
        gone.free()
        with pytest.raises(ValueError, match="freed"):
            call(gone)
    # what the device conversions do not offer, and the calls outside the list
    with pytest.raises(NotImplementedError, match="int64"):
        flw.hand(w32 > 0.5, to_device(np.ones(case.shape, np.int64)))
    with pytest.raises(NotImplementedError, match="classic"):
        flw.stream_order(type="classic", resident=True)
    with pytest.raises(ValueError, match="Unknown stream order type"):
        flw.stream_order(type="horton", resident=True)
    with pytest.raises(TypeError, match=r"\.numpy\(\)"):
        flw.main_upstream(uparea=to_device(w32))
    with pytest.raises(NotImplementedError, match="not supported"):
        flw.basins(ids=np.arange(1, flw.idxs_pit.size + 1, dtype=np.int16), resident=True)
    # a raster that needs row blocks
    monkeypatch.setenv("PFD_TEST_BIG_CELLS", str(n // 3))
    assert flw._row_blocks_needed() > 1
    dev = to_device(w32)
    for call in (lambda: flw.upstream_area(resident=True), lambda: flw.upstream_area("km2", resident=True),
                 lambda: flw.accuflux(w32, resident=True), lambda: flw.accuflux(dev), lambda: flw.fillnodata(dev, -9999.0),
                 lambda: flw.upstream_sum(dev), lambda: flw.stream_order(resident=True), lambda: flw.stream_distance(mask=dev),
                 lambda: flw.basins(resident=True), lambda: flw.hand(dev, w32), lambda: flw.downstream(dev)):
        with pytest.raises(NotImplementedError, match="without resident=True|beyond 2\\*\\*32"):
            call()
    monkeypatch.delenv("PFD_TEST_BIG_CELLS")
    assert flw._row_blocks_needed() == 1
    same_bytes(flw.accuflux(dev, resident=True).numpy(), flw.accuflux(w32), "after the refusals")
