"""Rasters, payloads, references and launch counts for the tests of the exact-order engine's DISPATCH
(tests/test_exact_dispatch_cases.py on the CPU, tests/test_gpu_exact_dispatch.py on the device).

run_exact_up / run_exact_down (csrc/exact_sweep.h) choose their kernels by two size rules:

 1. a round of at least xfuse_min_chains() chains — 2**20 in production — takes k_xtrunk_prescan (up) or
    k_xtrunk_dscan_lds (down, HAND only); a smaller round takes k_xtrunk_pre + k_xtrunk_scan, or k_xtrunk_dscan;
 2. a plan whose last two rounds hold a chain of XTAIL_LONG = 16384 slots and at most an eighth of the slots
    (xplan_tail_split, csrc/exact.h) forks the raster-order pass onto the handle's second stream.

Where each choice runs under test (tests/conftest.py sets PFD_TEST_FUSE_MIN=1 for the whole suite, so every exact-engine
test NOT named here runs the workgroup-per-256-chains kernels in every round and, its rasters being less than 16384 cells
high, never the two-stream tail):

 * the production threshold (no round of a raster below ~10**8 cells reaches it: every round takes the lane-per-chain
   kernels, as on a user's raster): the `production` form of test_gpu_exact_dispatch.py, every operation of the engine on
   SMALL, TAIL and TAIL_BLOCKS; test_gpu_large.py::test_exact_engine_accuflux, test_gpu_fillnodata.py and
   test_gpu_outlets.py in one parametrisation each;
 * rounds on both sides of the threshold within one sweep: the `straddle` form here (the threshold is set to the chains
   of the raster's largest round, so that round alone is fused) and test_gpu_fullsize.py's 30000 x 30000 raster;
 * the two-stream tail, up and down: TAIL here, in every form and with no knob — its plan splits because it holds a
   river of 18000 cells AND is wide enough for its last two rounds to hold less than an eighth of the slots; before, only
   float32 accuflux and the Strahler order of the 30000 x 30000 raster took the up branch and nothing took the down
   branch.  No row-block plan splits under test: see TAIL_BLOCKS below.

Launches of one sweep, as profiling reports them (`launches` of the exact_* segment), with nb rounds and no round fused:

    up    1 tile pass (exact_sweep.h, k_xtile_up) + 2 per round (k_xtrunk_pre, k_xtrunk_scan: `launches += 2`)
          + 1 raster-order pass (k_xtrunk_unscatter_list)                                   = 2 + 2 nb
          with the tail split: that pass runs on the second stream at round bsplit (`++launches`) and k_xtrunk_scatter
          follows the last round (`++launches`)                                             = 3 + 2 nb
    down  1 tile pass (k_xtile_down) + 1 gather (k_xtrunk_demit_list) + 1 per round (k_xtrunk_dscan or
          k_xtrunk_dscan_lds: `++launches` in either branch)                                = 2 + nb
          with the tail split: k_xtrunk_demit_list<Op, true> on the second stream and k_xtrunk_dpre on the first
          (`launches += 2`)                                                                 = 3 + nb

A plan without trunk cells (nslot == 0: a raster smaller than a tile) launches the tile pass alone.  An up-sweep of a
FUSE_UP operation (AccuUp, Strahler, FillDown) replaces the 2 launches of a fused round by 1 — k_xtrunk_prescan, plus
k_xtrunk_pre_long where the round holds chains of XLONG slots — so a sweep with a fused round WITHOUT such chains makes
strictly fewer launches, and one whose fused rounds all hold such chains makes as many as the unfused sweep (the
`straddle` form of WIDEST_HAS_LONG: its count proves nothing, its results pin it); a block sweep that is kept for
incremental updates (accuflux up, Strahler) never fuses.  A
down-sweep launches one kernel per round in both chain forms and both read the same xfuse_min_chains(): its count cannot
tell them apart, and no probe is invented for it — the `suite` / `straddle` forms of a down-sweep are pinned by their
results alone.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden_util import GOLD  # noqa: E402
from serial_refs import _ref_down, _ref_floodplains, _ref_up  # noqa: E402

FUSE_PRODUCTION = 1 << 20  # xfuse_min_chains() without PFD_TEST_FUSE_MIN
XTAIL_LONG = 16384         # csrc/exact.h
FORMS = ("production", "suite", "straddle")

INFO_KEYS = ("state", "trunk_cells", "chains", "slots", "rounds", "tail_split", "longest_chain", "widest_round")


def xplan_info(handle) -> dict:
    """pfd_debug_xplan of a RasterHandle (builds the plan if the handle has none; a row-block handle reports the plan its
    *_block sweeps run on).  state 1: the handle sweeps on the exact-order plan; tail_split -1: no two-stream tail;
    longest_chain 0: no chain of XLONG = 512 slots or more; widest_round: chains of the largest round."""
    return xplan_debug(handle)[0]


def xplan_debug(handle, lh=None):
    """(info dict, lh): as xplan_info; ``lh`` (uint8, one byte per cell of the device raster) receives the leaf steps."""
    from pyflwdir_amd import _hip

    L = _hip.lib()
    L.pfd_debug_xplan.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    L.pfd_debug_xplan.restype = C.c_int
    info = (C.c_int64 * 8)()
    _hip.check(L.pfd_debug_xplan(handle._h, info, None if lh is None else lh.ctypes.data_as(C.c_void_p)))
    return dict(zip(INFO_KEYS, (int(v) for v in info))), lh


def up_launches(info) -> int:
    """Launches of an up-sweep with no round fused (module docstring)."""
    if info["slots"] == 0:
        return 1
    return 2 + 2 * info["rounds"] + (info["tail_split"] >= 0)


def down_launches(info) -> int:
    """Launches of a down-sweep, in either chain form (module docstring)."""
    if info["slots"] == 0:
        return 1
    return 2 + info["rounds"] + (info["tail_split"] >= 0)


def fuse_min(form, info) -> int:
    """PFD_TEST_FUSE_MIN of a dispatch form; `straddle`: the chains of the largest round, which alone reaches it."""
    if form == "straddle":
        return info["widest_round"]
    return {"production": FUSE_PRODUCTION, "suite": 1}[form]


# ---- rasters -------------------------------------------------------------------------------------------------------
RIVER = dict(tilt=1 << 26, white=2, nodata_pct=0)
# TAIL.  A river strip splits its plan only when it is wide enough: the last two rounds are the main stems and the chains
# that join them directly, and their share of the trunk shrinks slowly with the width.  Measured on the device, with the
# plan's own rule restated on the CPU for the widths not run there (trunk cells per round; slots follow them closely):
#   18000 x 256   rounds 9, tail_split -1, longest chain 26742 slots; last two rounds 18.9 % of the trunk cells
#   20000 x 384   14.4 %      18000 x 512   12.2 %      18000 x 640   11.8 %      18000 x 768   10.9 %
#   18000 x 896    9.3 %  <- taken: clear of the eighth (12.5 %) whatever the post slots of the stems add
TAIL_SHAPE = (18000, 896)
# TAIL_BLOCKS.  Either half plus its halo row holds a stem of 18001 cells, but at 128 columns the block plans do not split
# (seen on the device: block 0 rounds 8, tail_split -1, longest chain 28743 slots; block 1 rounds 9, -1, 28274), and by the
# figures above neither would 192 or 256 columns: a block would have to be as wide as TAIL, 32 M cells for two of them,
# more than the plain-Python references of floodplains and fillnodata can take.  The row-block tests therefore cover the
# production threshold, the sweeps with nothing kept and the whole-raster reference, not the tail branch.
TAIL_BLOCKS_SHAPE, TAIL_NBLOCKS = (36000, 128), 2
# name -> (shape, seed, synth_d8 arguments): the rasters of test_gpu_large.py::test_exact_engine_accuflux
SYNTH_SMALL = {
    "river_1500x2100": ((1500, 2100), 3, dict(tilt=1 << 26, white=2, nodata_pct=0)),
    "rough_1024x1024": ((1024, 1024), 4, dict(tilt=100000, white=2, nodata_pct=30)),
    "hills_700x900": ((700, 900), 5, dict(tilt=3000, white=2, nodata_pct=3)),
}
GOLDEN_SMALL = ("synth_tiny_5x7", "synth_onerow_1x300", "synth_rough_nodata_384x512")
FUZZ_SMALL = {"fuzz_130x67": ((130, 67), 7101, 0.1, 0.05), "fuzz_513x520": ((513, 520), 7102, 0.1, 0.002)}  # shape, seed, p_nodata, p_pit
SMALL = tuple(SYNTH_SMALL) + GOLDEN_SMALL + tuple(FUZZ_SMALL)
# the SMALL rasters whose plans have at least two rounds, as the `straddle` form needs (test_small_plans asserts the split)
STRADDLE_SMALL = tuple(n for n in SMALL if n not in ("synth_tiny_5x7", "synth_onerow_1x300"))
# rasters whose LARGEST round holds chains of XLONG slots: fused, that round costs k_xtrunk_pre_long + k_xtrunk_prescan, as
# many launches as the k_xtrunk_pre + k_xtrunk_scan it replaces
WIDEST_HAS_LONG = ("TAIL", "river_1500x2100")


def _oracle():
    from oracle import oracle as O

    O.build()
    return O


def tail_d8(headwaters=True):
    """TAIL: a river raster 18000 rows high — one main stem of 18000 cells — with both pit codes and, after the
    ``headwaters`` step, nodata: 30 % of the cells without upstream cells are removed, which breaks no path."""
    O = _oracle()
    d8 = O.synth_d8(TAIL_SHAPE[0], TAIL_SHAPE[1], seed=3, **RIVER)
    pits = np.flatnonzero(d8.ravel() == 0)
    d8.flat[pits[1::2]] = 255
    if headwaters:
        upa = O.upstream_area_cell(d8)[0]
        head = np.flatnonzero(upa.ravel() == 1)
        rng = np.random.default_rng(18000)
        d8.flat[head[rng.random(head.size) < 0.3]] = 247
    return d8


class Raster:
    """One test raster with what the CPU knows about it, its payloads and the references of the operations, each computed
    on first use and kept (read-only) for the session."""

    def __init__(self, name, d8, nblocks=1):
        self.name, self.nblocks = name, nblocks
        self.d8 = np.ascontiguousarray(d8, dtype=np.uint8)
        self.d8.setflags(write=False)
        self.shape, self.n = self.d8.shape, self.d8.size
        self._refs = {}
        self.plan = None  # xplan_info of the whole raster's handle (the GPU tests fill it in)

    @functools.cached_property
    def graph(self):
        O = _oracle()
        idxs_ds, idxs_pit, _ = O.from_array(self.d8)
        seq = O.idxs_seq(idxs_ds, idxs_pit)
        return idxs_ds, idxs_pit, seq

    @functools.cached_property
    def upa(self):
        """int32 upstream cells, -9999 on nodata."""
        upa = _oracle().upstream_area_cell(self.d8)[0].ravel()
        upa.setflags(write=False)
        return upa

    def stem(self):
        """Cells of the main stem: from the largest sink along oracle.main_upstream to a headwater."""
        idxs_ds, idxs_pit, _ = self.graph
        main = _oracle().main_upstream(idxs_ds, self.upa)
        x, k = int(idxs_pit[np.argmax(self.upa[idxs_pit])]), 1
        while main[x] >= 0 and main[x] != x:
            x, k = int(main[x]), k + 1
        return k

    @functools.cached_property
    def transforms(self):
        """(lat/lon, projected): at most 60 degrees of latitude from 55 N down; 90 m cells (0.81 ha: float32 sums round)."""
        from pyflwdir_amd._affine import Affine

        res = min(0.01, 60.0 / self.shape[0])
        return Affine(res, 0.0, 3.0, 0.0, -res, 55.0), Affine(90.0, 0.0, 0.0, 0.0, -90.0, 0.0)

    @functools.cached_property
    def payloads(self):
        """Inputs of the operations; every payload with a nodata value holds it INSIDE the domain (NODATA)."""
        n, valid = self.n, self.d8.ravel() != 247
        rng = np.random.default_rng([self.shape[0], self.shape[1], 20240611])
        P = {}
        P["f32"] = rng.random(n, dtype=np.float32)
        P["f32"][rng.random(n) < 0.05] = -1.0
        P["f64"] = rng.random(n) * 3.25
        P["f64"][rng.random(n) < 0.05] = -9999.0
        P["i32"] = rng.integers(-50, 1000, n).astype(np.int32)  # negative values: the exact engine, not the tiled one
        P["i32"][rng.random(n) < 0.05] = -9999
        P["i64"] = P["i32"].astype(np.int64) * 100000
        P["i64"][P["i32"] == -9999] = -9999
        P["mask"] = rng.random(n) < 0.6
        P["drain"] = rng.random(n) < 0.01
        P["elev32"] = (rng.random(n) * 100).astype(np.float32)
        P["elev64"] = P["elev32"].astype(np.float64) * 1.000001  # (no float32 holds these)
        # floodplains: areas whose square roots are exact in every pow() (b = 0.5), small integer elevations (dh == h0 occurs)
        root = np.floor(np.sqrt(np.maximum(self.upa, 0).astype(np.float64)))
        P["flood_upa"] = np.where(valid, root * root, -9999).astype(np.float32)
        P["flood_elev"] = rng.integers(0, 40, n).astype(np.float32)
        P["fill_f32"] = np.where(rng.random(n) < 0.3, np.float32(-9999), rng.integers(-8, 9, n).astype(np.float32) / 4)
        P["fill_i32"] = np.where(rng.random(n) < 0.3, 0, rng.integers(-5, 1000, n)).astype(np.int32)
        for name, nd in NODATA.items():  # (tiny rasters: make sure the value is there, on a valid cell)
            if not (P[name][valid] == nd).any():
                P[name][np.flatnonzero(valid)[-1]] = nd
        for a in P.values():
            a.setflags(write=False)
        return P

    def ref(self, key, compute):
        if key not in self._refs:
            r = np.ascontiguousarray(compute())
            r.setflags(write=False)
            self._refs[key] = r
        return self._refs[key]


NODATA = {"f32": -1.0, "f64": -9999.0, "i32": -9999, "i64": -9999, "fill_f32": -9999.0, "fill_i32": 0}
FLOOD_UPA_MIN, FLOOD_B = 49.0, 0.5


@functools.lru_cache(maxsize=None)
def raster(name) -> Raster:
    """The raster ``name`` (SMALL, "TAIL", "TAIL_BLOCKS"), built once per session."""
    O = _oracle()
    if name == "TAIL":
        return Raster(name, tail_d8())
    if name == "TAIL_BLOCKS":
        return Raster(name, O.synth_d8(TAIL_BLOCKS_SHAPE[0], TAIL_BLOCKS_SHAPE[1], seed=3, **RIVER), nblocks=TAIL_NBLOCKS)
    if name in SYNTH_SMALL:
        shape, seed, kw = SYNTH_SMALL[name]
        return Raster(name, O.synth_d8(shape[0], shape[1], seed=seed, **kw))
    if name in GOLDEN_SMALL:
        return Raster(name, np.load(os.path.join(GOLD, name + ".npz"))["d8"])
    from test_gpu_fuzz import random_d8

    shape, seed, p_nodata, p_pit = FUZZ_SMALL[name]
    return Raster(name, random_d8(np.random.default_rng(seed), shape, p_nodata=p_nodata, p_pit=p_pit, coherent=-1))


# ---- operations ------------------------------------------------------------------------------------------------------
class Op:
    """One operation of the engine: ``sweep`` "up" / "down", the profiling segment it must run in, whether its up-sweep
    fuses (FUSE_UP), the call on a FlwdirRaster and the reference on a Raster."""

    def __init__(self, name, sweep, segment, run, ref, fuses=False):
        self.name, self.sweep, self.segment, self.run, self.ref, self.fuses = name, sweep, segment, run, ref, fuses

    def expected(self, r: Raster):
        return r.ref(self.name, lambda: self.ref(r))


def _accuflux(key, direction):
    def run(flw, r):
        return flw.accuflux(r.payloads[key].reshape(r.shape), nodata=NODATA[key], direction=direction)

    def ref(r):
        idxs_ds, _, seq = r.graph
        return _oracle().accuflux(idxs_ds, seq, r.payloads[key], nodata=NODATA[key], direction=direction)

    return Op(f"accuflux_{key}_{direction}", direction, f"exact_accuflux_{direction}", run, ref, fuses=direction == "up")


def _area(unit, which):
    def rows_of(r):
        from pyflwdir_amd import gis

        tr = r.transforms[which]
        return np.ascontiguousarray(gis.area_rows(tr, r.shape, which == 0, unit="m2") / gis.AREA_FACTORS[unit])

    def run(flw, r):
        flw.set_transform(r.transforms[which], latlon=which == 0)
        return flw.upstream_area(unit)

    def ref(r):  # oracle.accuflux of the row areas repeated per cell; -9999 on nodata
        idxs_ds, _, seq = r.graph
        exp = _oracle().accuflux(idxs_ds, seq, np.repeat(rows_of(r), r.shape[1]), nodata=-9999)
        exp[r.d8.ravel() == 247] = -9999
        return exp

    return Op(f"upstream_area_{unit}", "up", "exact_accuflux_up", run, ref, fuses=True)


def _strahler(masked):
    def run(flw, r):
        return flw.stream_order(mask=r.payloads["mask"].reshape(r.shape) if masked else None)

    def ref(r):
        idxs_ds, _, seq = r.graph
        return _oracle().strahler_order(idxs_ds, seq, r.payloads["mask"] if masked else None)

    return Op("strahler_masked" if masked else "strahler", "up", "exact_strahler", run, ref, fuses=True)


def _classic():
    def run(flw, r):
        return flw.stream_order(type="classic", mask=r.payloads["mask"].reshape(r.shape))

    def ref(r):
        idxs_ds, _, seq = r.graph
        O = _oracle()
        return O.stream_order_classic(idxs_ds, seq, O.main_upstream(idxs_ds, r.upa), r.payloads["mask"])

    return Op("classic_masked", "down", "exact_classic_order", run, ref)


def _hand(key):
    def run(flw, r):
        return flw.hand(r.payloads["drain"].reshape(r.shape), r.payloads[key].reshape(r.shape))

    def ref(r):
        idxs_ds, _, seq = r.graph
        return _oracle().height_above_nearest_drain(idxs_ds, seq, r.payloads["drain"], r.payloads[key])

    return Op(f"hand_{key}", "down", "exact_hand", run, ref)


def _distance(metres):
    def run(flw, r):
        if metres:
            flw.set_transform(r.transforms[0], latlon=True)
            return flw.stream_distance(unit="m")
        return flw.stream_distance(mask=r.payloads["mask"].reshape(r.shape))

    def ref(r):
        idxs_ds, _, seq = r.graph
        if metres:
            return _oracle().stream_distance(idxs_ds, seq, r.shape[1], latlon=True, transform=tuple(r.transforms[0])[:6])
        return _oracle().stream_distance(idxs_ds, seq, r.shape[1], mask=r.payloads["mask"], real_length=False)

    return Op("stream_distance_m" if metres else "stream_distance_cells_masked", "down", "exact_stream_distance", run, ref)


def _floodplains():
    def run(flw, r):
        P = r.payloads
        return flw.floodplains(P["flood_elev"].reshape(r.shape), uparea=P["flood_upa"].reshape(r.shape),
                               upa_min=FLOOD_UPA_MIN, b=FLOOD_B)

    def ref(r):
        idxs_ds, _, seq = r.graph
        P = r.payloads
        return _ref_floodplains(idxs_ds, seq, P["flood_elev"], P["flood_upa"], FLOOD_UPA_MIN, FLOOD_B)

    return Op("floodplains", "down", "exact_floodplains", run, ref)


def _fillnodata(key, direction, how):
    def run(flw, r):
        return flw.fillnodata(r.payloads[key].reshape(r.shape), NODATA[key], direction=direction, how=how)

    def ref(r):
        idxs_ds, _, seq = r.graph
        if direction == "up":
            return _ref_up(idxs_ds, seq, r.payloads[key], NODATA[key])
        return _ref_down(idxs_ds, seq, r.payloads[key], NODATA[key], how)

    # (direction "down" merges upstream values into a cell: an up-sweep, FillDown; "up" is a down-sweep)
    return Op(f"fillnodata_{direction}" + ("" if direction == "up" else f"_{how}"), "down" if direction == "up" else "up",
              f"exact_fillnodata_{direction}", run, ref, fuses=direction == "down")


OPS = [
    _accuflux("f32", "up"), _accuflux("f64", "up"), _accuflux("i32", "up"), _accuflux("i64", "up"),
    _accuflux("f32", "down"), _accuflux("i32", "down"),
    _area("km2", 0), _area("ha", 1),
    _strahler(False), _strahler(True), _classic(),
    _hand("elev32"), _hand("elev64"),
    _distance(False), _distance(True),
    _floodplains(),
    _fillnodata("fill_f32", "up", "max"), _fillnodata("fill_i32", "down", "max"), _fillnodata("fill_f32", "down", "sum"),
]
OP = {op.name: op for op in OPS}

# The dist.*_blocks counterparts on TAIL_BLOCKS: name -> (whole-raster operation whose reference they must equal, sweep,
# segment of the block sweep, fuses).  accuflux up and Strahler keep their first sweep for incremental updates
# (pfd_set_block_update), which never fuses; fillnodata "down" is the row-block up-sweep with nothing kept.
BLOCK_OPS = {
    "accuflux_up": ("accuflux_f32_up", "up", "exact_up_block", False),
    "accuflux_down": ("accuflux_f32_down", "down", "exact_down_block", False),
    "strahler": ("strahler", "up", "exact_up_block", False),
    "hand": ("hand_elev32", "down", "exact_hand_block", False),
    "stream_distance": ("stream_distance_cells_masked", "down", "exact_down_block", False),
    "classic": ("classic_masked", "down", "exact_down_block", False),
    "floodplains": ("floodplains", "down", "exact_down_block", False),
    "fillnodata": ("fillnodata_down_sum", "up", "exact_up_block", True),
}


def run_block_op(name, r: Raster):
    """The dist.*_blocks call of BLOCK_OPS[name] on the whole host raster of ``r``, in ``r.nblocks`` row blocks."""
    from pyflwdir_amd import _hip, dist

    P, nb, shape = r.payloads, r.nblocks, r.shape
    u8 = lambda m: np.ascontiguousarray(m).view(np.uint8).reshape(shape)  # noqa: E731
    if name.startswith("accuflux"):
        return dist.accuflux_blocks(r.d8, nb, P["f32"].reshape(shape), (0, NODATA["f32"], 1), direction=name.split("_")[1])[0]
    if name == "strahler":
        return dist.strahler_blocks(r.d8, nb)[0]
    if name == "hand":
        return dist.hand_blocks(r.d8, nb, u8(P["drain"]), P["elev32"].reshape(shape))[0]
    if name == "stream_distance":
        return dist.stream_distance_blocks(r.d8, nb, u8(P["mask"]))[0]
    if name == "classic":
        return dist.classic_blocks(r.d8, nb, r.upa.reshape(shape), u8(P["mask"]))[0]
    if name == "floodplains":
        upa = P["flood_upa"]
        stream = (upa >= FLOOD_UPA_MIN).astype(np.uint8)
        hs = np.where(stream, np.sqrt(np.maximum(upa, 0)), 0).astype(np.float32)  # (exact roots: == upa ** 0.5)
        return dist.floodplains_blocks(r.d8, nb, P["flood_elev"].reshape(shape), stream.reshape(shape), hs.reshape(shape))[0]
    assert name == "fillnodata"
    return dist.fillnodata_blocks(r.d8, nb, P["fill_f32"].reshape(shape), _hip.PFD_F32, (0, NODATA["fill_f32"], 1),
                                  direction="down", how=_hip.PFD_FILL_SUM)[0]


def same_bytes(got, exp, shape):
    """None, or what differs: dtype, shape or the first differing cells.  ``exp``: the flat reference of a raster of
    ``shape``.  Bytes are compared, so -0.0 differs from 0.0 and a NaN equals only a NaN of the same bits in its place."""
    got = np.asarray(got)
    if got.dtype != exp.dtype:
        return f"dtype {got.dtype} != {exp.dtype}"
    if got.shape != tuple(shape) or got.size != exp.size:
        return f"shape {got.shape} != {tuple(shape)}"
    g, e = np.ascontiguousarray(got).ravel(), exp.ravel()
    if g.tobytes() == e.tobytes():
        return None
    bad = np.flatnonzero(g.view(f"u{g.itemsize}") != e.view(f"u{e.itemsize}"))
    return f"{bad.size} cells differ, first {bad[:5].tolist()}: got {g[bad[:5]].tolist()} expected {e[bad[:5]].tolist()}"
