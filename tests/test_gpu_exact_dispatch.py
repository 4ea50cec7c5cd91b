"""Every sweep of the exact-order engine on the dispatch production takes, bit for bit against the CPU references
(tests/exact_dispatch.py: rasters, payloads, references, launch counts and where each kernel choice runs under test).

Forms (PFD_TEST_FUSE_MIN, set before the handle is created): `production` 2**20 — no round of these rasters reaches it,
as on a user's raster; `suite` 1 — every round takes the workgroup-per-256-chains kernels; `straddle` — the chains of
the raster's largest round, so that one round is fused and the others are not.  TAIL splits its last two rounds onto the
second stream (xplan_tail_split) in every form, with no knob.  With profiling on, every test also proves
that it ran the form it names: the operation's exact_* segment with the launches that form issues."""
import pytest

import exact_dispatch as X

pytestmark = pytest.mark.gpu

WHOLE = ([("production", n) for n in X.SMALL + ("TAIL",)] + [("suite", "TAIL")]
         + [("straddle", n) for n in ("TAIL",) + X.STRADDLE_SMALL])
BLOCK_CALLS = ("accuflux_block", "fillnodata_block", "stream_distance_block", "stream_order_classic_block",
               "floodplains_block", "strahler_block", "hand_block")
BLOCK_UPDATES = ("exact_up_block_update", "hand_block_update")  # later sweeps of a block that redo a part only


def plan_of(r):
    """xplan_info of the whole raster (the plan does not depend on the form), once per session."""
    from pyflwdir_amd import _hip

    if r.plan is None:
        h = _hip.RasterHandle(r.d8, r.shape[0], r.shape[1])
        r.plan = X.xplan_info(h)
        h.close()
    return r.plan


def sweep_segments(timing):
    return [s for s in timing if s["name"].startswith("exact_") and s["name"] != "exact_plan"]


def check_launches(seg, info, sweep, fewer, what):
    """``seg``: the sweep's profiling segment; ``fewer``: an up-sweep of a FUSE_UP operation in a form that fuses at least
    one round without chains of XLONG slots."""
    plain = X.up_launches(info) if sweep == "up" else X.down_launches(info)
    print(f"{what}: {seg['name']} launches {seg['launches']}, unfused {plain}, plan {info}")
    if fewer:
        assert seg["launches"] < plain, (what, seg, info)
    else:
        assert seg["launches"] == plain, (what, seg, info)


def test_tail_plan_splits(gpu_lib):
    """TAIL's plan forks its last two rounds onto the second stream without any knob.  Seen on the MI355X:
    TAIL (18000 x 896): 11 rounds, tail_split 30, longest chain 27590 slots, 4528372 slots in 207105 chains, largest round
    60609 chains.
    The plans of the row blocks of TAIL_BLOCKS, built the way dist._block_handle builds them, hold a chain of more than
    XTAIL_LONG slots each but do not split (exact_dispatch.py says why and what was seen); they are reported here."""
    from pyflwdir_amd import dist

    info = plan_of(X.raster("TAIL"))
    print("TAIL", info)
    assert info["state"] == 1 and info["tail_split"] >= 0 and info["longest_chain"] >= X.XTAIL_LONG, info
    rb = X.raster("TAIL_BLOCKS")
    for b in range(rb.nblocks):
        h = dist._block_handle(rb.d8, rb.nblocks, b, [0] * rb.nblocks)
        info = X.xplan_info(h)
        h.close()
        print("TAIL_BLOCKS", b, info)
        assert info["state"] == 1 and info["rounds"] >= 4 and info["longest_chain"] >= X.XTAIL_LONG, (b, info)


@pytest.mark.parametrize("name", X.SMALL)
def test_small_plans(gpu_lib, name):
    """The SMALL rasters sweep on the exact-order plan, none of them with a two-stream tail; those of the `straddle` form
    have at least two rounds, the two left out have fewer."""
    info = plan_of(X.raster(name))
    print(name, info)
    assert info["state"] == 1 and info["tail_split"] == -1, info
    assert (info["rounds"] >= 2) == (name in X.STRADDLE_SMALL), info


@pytest.mark.parametrize("op", [o.name for o in X.OPS])
@pytest.mark.parametrize("form,name", WHOLE)
def test_whole_raster(gpu_lib, monkeypatch, form, name, op):
    import pyflwdir_amd as pyflwdir

    r, o = X.raster(name), X.OP[op]
    exp = o.expected(r)
    info = plan_of(r)
    monkeypatch.setenv("PFD_TEST_FUSE_MIN", str(X.fuse_min(form, info)))
    flw = pyflwdir.from_array(r.d8, ftype="d8", cache=False)
    flw._h.set_profiling(True)
    first = None
    # TAIL: three runs on one handle — an unordered pair of streams shows up as a difference between runs
    for k in range(3 if name == "TAIL" else 1):
        got = o.run(flw, r)
        what = f"{name} {form} {op} run {k}"
        if first is None:
            diff = X.same_bytes(got, exp, r.shape)
            assert diff is None, f"{what}: {diff}; plan {info}"
            first = got.tobytes()
        else:
            assert got.tobytes() == first, f"{what}: differs from run 0"
        segs = sweep_segments(flw._h.last_timing())
        assert [s["name"] for s in segs] == [o.segment], (what, segs)
        fewer = o.sweep == "up" and o.fuses and form != "production" and info["slots"] > 0
        if form == "straddle" and name in X.WIDEST_HAS_LONG:
            fewer = False  # (the one fused round holds long chains: two launches, like the pair it replaces)
        check_launches(segs[0], info, o.sweep, fewer, what)


@pytest.mark.parametrize("op", list(X.BLOCK_OPS))
@pytest.mark.parametrize("form", ["production", "suite"])
def test_row_blocks(gpu_lib, monkeypatch, form, op):
    """The dist.*_blocks calls on TAIL_BLOCKS in 2 row blocks against the WHOLE raster's reference; every block handle
    sweeps on an exact-order plan and its full sweeps make the launches that plan's shape gives."""
    from pyflwdir_amd import dist

    r = X.raster("TAIL_BLOCKS")
    whole, sweep, segment, fuses = X.BLOCK_OPS[op]
    exp = X.OP[whole].expected(r)
    monkeypatch.setenv("PFD_TEST_FUSE_MIN", str(X.fuse_min(form, None)))
    log, make = [], dist._block_handle

    def traced(d8, nblocks, b, devices):
        h = make(d8, nblocks, b, devices)
        h.set_profiling(True)
        info = X.xplan_info(h)

        def after(call):
            def wrapped(*a, **kw):
                out = call(*a, **kw)
                log.append((b, info, h.last_timing()))
                return out
            return wrapped

        for name in BLOCK_CALLS:
            setattr(h, name, after(getattr(h, name)))
        return h

    monkeypatch.setattr(dist, "_block_handle", traced)
    got = X.run_block_op(op, r)
    diff = X.same_bytes(got, exp, r.shape)
    assert diff is None, f"TAIL_BLOCKS {form} {op}: {diff}"
    full = {b: 0 for b in range(r.nblocks)}
    for b, info, timing in log:
        assert info["state"] == 1, (b, info)
        segs = [s for s in sweep_segments(timing) if s["name"] not in BLOCK_UPDATES]
        assert all(s["name"] == segment for s in segs), (b, segs)
        for s in segs:
            full[b] += 1
            check_launches(s, info, sweep, sweep == "up" and fuses and form == "suite", f"TAIL_BLOCKS {form} {op} block {b}")
    assert all(full.values()), f"a block never ran {segment}: {full}"


def test_plan_bytes_of_a_whole_raster(gpu_lib):
    """bytes_held grows when the plan is built, by the same amount on every handle of the raster."""
    from pyflwdir_amd import _hip

    r = X.raster("fuzz_130x67")
    held = []
    for _ in range(2):
        h = _hip.RasterHandle(r.d8, r.shape[0], r.shape[1])
        before = h.info()["bytes_held"]
        info = X.xplan_info(h)
        held.append(h.info()["bytes_held"])
        h.close()
        print("fuzz_130x67", info, "bytes_held", before, "->", held[-1])
        assert info["state"] == 1 and held[-1] > before, (info, before, held)
    assert held[0] == held[1], held


@pytest.mark.parametrize("b", [0, 1])
def test_kept_block_sweep_bytes_do_not_drift(gpu_lib, b):
    """fuzz_513x520 in two row blocks: a kept up-sweep (pfd_set_block_update 1) holds at least its element and value
    arrays — 8 bytes per slot — more than the handle does after pfd_set_block_update(0), a second keep / release cycle
    ends on the same bytes_held as the first, and both kept sweeps give the plain sweep's bits."""
    import numpy as np

    from pyflwdir_amd import _hip, dist

    r, nb = X.raster("fuzz_513x520"), 2
    a, e = dist.block_slice(r.shape[0], nb, b)
    ncol = r.shape[1]
    h = dist._block_handle(r.d8, nb, b, [0] * nb)
    bufs = []
    try:
        info = X.xplan_info(h)
        assert info["state"] == 1 and info["slots"] > 0, info
        payload = np.ascontiguousarray(r.payloads["f32"].reshape(r.shape)[a:e])
        data = _hip.DeviceBuffer(payload.nbytes, h.device).upload(payload)
        out = _hip.DeviceBuffer(payload.nbytes, h.device)
        bufs += [data, out]
        seed = np.random.default_rng(513 + b).random(2 * ncol, dtype=np.float32)

        def sweep():
            h.accuflux_block(data, _hip.PFD_F32, seed, out, nodata_f=X.NODATA["f32"], has_nodata=1, memspace=_hip.PFD_DEVICE)
            return out.download(np.float32, (e - a, ncol)).tobytes()

        h.set_block_update(0)
        plain = sweep()
        released = []
        for cycle in range(2):
            h.set_block_update(1)
            got = sweep()
            kept = h.info()["bytes_held"]
            h.set_block_update(0)
            released.append(h.info()["bytes_held"])
            print(f"block {b} cycle {cycle}: slots {info['slots']}, bytes_held kept {kept}, released {released[-1]}")
            assert got == plain, f"block {b} cycle {cycle}: the kept sweep differs from the plain one"
            assert kept - released[-1] >= 8 * info["slots"], (kept, released, info)
        assert released[0] == released[1], released
    finally:
        for buf in bufs:
            buf.free()
        h.close()


def test_abandoned_plan_leaves_a_readable_record(gpu_lib):
    """A raster with cycles gets no plan: the first order-sensitive call records a closed exact_plan segment, then runs on
    the level engine; the handle remembers (state -1) and the next call does not try again."""
    import math
    import os

    import numpy as np

    from pyflwdir_amd import _hip

    d8 = np.ascontiguousarray(np.load(os.path.join(X.GOLD, "synth_loops_96x80.npz"))["d8"], dtype=np.uint8)
    data = np.random.default_rng(96).random(d8.size, dtype=np.float32)
    h = _hip.RasterHandle(d8, d8.shape[0], d8.shape[1])
    try:
        h.set_profiling(True)
        first = h.accuflux(data, _hip.PFD_F32, nodata_f=-9999.0)
        timing = h.last_timing()
        print("first call", timing)
        names = [s["name"] for s in timing]
        assert names.count("exact_plan") == 1 and "sweep_accuflux_up" in names, names
        plan = timing[names.index("exact_plan")]
        assert math.isfinite(plan["ms"]) and plan["ms"] >= 0.0, plan
        assert names.index("sweep_accuflux_up") > names.index("exact_plan"), names
        assert X.xplan_info(h)["state"] == -1
        second = h.accuflux(data, _hip.PFD_F32, nodata_f=-9999.0)
        names = [s["name"] for s in h.last_timing()]
        print("second call", names)
        assert "exact_plan" not in names and "sweep_accuflux_up" in names, names
        assert second.tobytes() == first.tobytes()
    finally:
        h.close()
