"""ctypes binding of libpfd_hip.so — the C-ABI declared in include/pfd.h.

There is deliberately NO fallback: if the shared library is missing, or no MI355X/HIP device
is visible, every entry point raises.  The CPU oracle under oracle/ is test infrastructure and
is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpfd_hip.so")

PFD_HOST, PFD_DEVICE = 0, 1
PFD_I32, PFD_U32, PFD_I64, PFD_F32, PFD_F64 = 1, 2, 3, 4, 5
_PAYLOAD_CODE = {np.dtype(np.int32): PFD_I32, np.dtype(np.int64): PFD_I64, np.dtype(np.float32): PFD_F32,
                 np.dtype(np.float64): PFD_F64}
PFD_UP, PFD_DOWN, PFD_BOTH = 0, 1, 2  # (PFD_BOTH: pfd_segment_slope only)
# fillnodata payload codes beyond the five above (narrow integers travel widened in int32 lanes) and merge rules
PFD_U64, PFD_I8, PFD_U8, PFD_I16, PFD_U16 = 6, 7, 8, 9, 10
PFD_FILL_MAX, PFD_FILL_MIN, PFD_FILL_SUM = 0, 1, 2
UPSCALE_METHOD = {"dmm": 0, "eam": 1, "eam_plus": 2}  # PFD_UPSCALE_*
PFD_COMPARE_OWN, PFD_COMPARE_F64 = 0, 1  # pfd_subbasins_area: where `> area_min` is evaluated
PFD_SUBAREA_FULL = 1  # pfd_subbasins_area flag: follow every cell (tests)
# the elementwise calls (csrc/elementwise.hip): outcomes a relation accepts, logic ops, reductions
PFD_EW_LT, PFD_EW_EQ, PFD_EW_GT, PFD_EW_UNORDERED = 1, 2, 4, 8
PFD_EW_AND, PFD_EW_OR, PFD_EW_XOR, PFD_EW_NOT = 0, 1, 2, 3
PFD_EW_COUNT, PFD_EW_MIN, PFD_EW_MAX = 0, 1, 2

_FLOAT_CODE = {np.dtype(np.float32): PFD_F32, np.dtype(np.float64): PFD_F64}

IDX_CODE = {np.dtype(np.int32): PFD_I32, np.dtype(np.uint32): PFD_U32, np.dtype(np.int64): PFD_I64}
# the stream order of the window calls (pfd_moving_average / pfd_moving_median)
STRORD_CODE = {np.dtype(np.uint8): PFD_U8, np.dtype(np.int32): PFD_I32, np.dtype(np.uint32): PFD_U32, np.dtype(np.int64): PFD_I64}

# status code -> Python exception (messages come from pfd_last_error()).  PFD_ENOPITS and
# PFD_EBADCODE map to the ValueErrors the reference raises for the same conditions
# (reference pyflwdir/flwdir.py:126-127, pyflwdir/pyflwdir.py:181-182).
_ERRORS = {-1: ValueError, -2: RuntimeError, -3: RuntimeError, -4: MemoryError, -5: ValueError,
           -6: ValueError, -7: NotImplementedError, -8: RuntimeError}

def _signatures():
    """(return type, [argument types]) of every function include/pfd.h declares, one row per prototype and in the
    header's order (tests/test_cabi.py holds every row to the header).  Untyped (`void *`), uint8 / int8 / int32 /
    uint32 / float and handle pointers are ``p``; the typed pointers below are the ones the wrappers pass ctypes
    arrays or ``byref`` values for."""
    i, i32, i64, u64, sz, f64 = C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_double
    p, s, pp = C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)
    pi, pi64, pf64 = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    synth = [i, u64, i64, i64, i64, i64, i32, i64, i64, p]
    return {
        "pfd_abi_version": (i, []),
        "pfd_last_error": (s, []),
        "pfd_device_count": (i, [pi]),
        "pfd_malloc": (i, [i, sz, pp]),
        "pfd_free": (i, [i, p]),
        "pfd_malloc_pooled": (i, [i, sz, pp]),
        "pfd_free_pooled": (i, [i, p]),
        "pfd_memcpy_h2d": (i, [i, p, p, sz]),
        "pfd_memcpy_d2h": (i, [i, p, p, sz]),
        "pfd_device_synchronize": (i, [i]),
        "pfd_trim": (i, [i]),
        "pfd_reserve": (i, [i, sz]),
        "pfd_alloc_stats": (i, [pi64]),
        "pfd_mem_info": (i, [i, pi64]),
        "pfd_transfer_stats": (i, [pf64, i]),
        "pfd_raster_create": (i, [p, i64, i64, i, i, pp]),
        "pfd_raster_destroy": (i, [p]),
        "pfd_raster_create_general": (i, [p, i, i64, i64, i, i, pp]),
        "pfd_raster_create_block": (i, [p, i64, i64, i, i, i, i, pp]),
        "pfd_raster_create_deferred": (i, [p, i64, i64, i, i, i, i, pp]),
        "pfd_raster_validate": (i, [p]),
        "pfd_raster_info": (i, [p, pi64]),
        "pfd_add_pits": (i, [p, p, i64]),
        "pfd_idxs_ds": (i, [p, i, p, i]),
        "pfd_idxs_pit": (i, [p, i, p, i]),
        "pfd_upstream_count": (i, [p, p, p, i]),
        "pfd_order_cells": (i, [p]),
        "pfd_idxs_seq": (i, [p, i, p, i]),
        "pfd_set_idxs_seq": (i, [p, i, p, i64]),
        "pfd_rank": (i, [p, p, i]),
        "pfd_upstream_area_cell": (i, [p, p, i]),
        "pfd_upstream_area_cell_levels": (i, [p, p, i]),
        "pfd_accuflux": (i, [p, i, p, i64, f64, i, i, i, p, i]),
        "pfd_accuflux_rows": (i, [p, i, p, i64, f64, i, i, i, p, i]),
        "pfd_fillnodata": (i, [p, i, p, i64, f64, i, i, i, p, i]),
        "pfd_upstream_area_rows_fixed": (i, [p, p, p, i, pi, pf64]),
        "pfd_strahler": (i, [p, p, p, i]),
        "pfd_basins": (i, [p, p, p, i64, i, p, i]),
        "pfd_hand": (i, [p, p, i, p, p, i]),
        "pfd_main_upstream": (i, [p, i, p, f64, i, p, i]),
        "pfd_upstream_sum": (i, [p, i, p, i64, f64, i, p, i]),
        "pfd_stream_order_classic": (i, [p, i, p, p, p, i]),
        "pfd_stream_distance": (i, [p, p, i, p, p, i]),
        "pfd_upstream_area_cell_blocks": (i, [pp, i, pp, i]),
        "pfd_comm_unique_id": (i, [p, sz]),
        "pfd_comm_create": (i, [p, sz, i, i, i, pp]),
        "pfd_comm_destroy": (i, [p]),
        "pfd_comm_info": (i, [p, pi, pi, pi]),
        "pfd_upstream_area_cell_dist": (i, [p, p, p, i]),
        "pfd_comm_exchange_rows": (i, [p, p, p, i, p, p]),
        "pfd_comm_allgather_host": (i, [p, p, p, sz, p]),
        "pfd_set_block_io": (i, [p, i]),
        "pfd_upstream_area_cell_begin": (i, [p, p, i, p]),
        "pfd_upstream_area_cell_finish": (i, [p, p, i, i, pi]),
        "pfd_hand_block": (i, [p, p, i, p, p, i, p, i, p, pi64]),
        "pfd_set_block_update": (i, [p, i]),
        "pfd_accuflux_block": (i, [p, i, p, i, i64, f64, i, i, p, i, p, i, p, pi64]),
        "pfd_strahler_block": (i, [p, p, p, i, p, i, p, pi64]),
        "pfd_fillnodata_block": (i, [p, i, p, i64, f64, i, i, i, p, i, p, i, p, pi64]),
        "pfd_stream_distance_block": (i, [p, p, i, p, p, i, p, i, p, pi64]),
        "pfd_floodplains_block": (i, [p, i, p, p, p, p, i, p, i, p, pi64]),
        "pfd_floodplains_block_flags": (i, [p, p, p, i]),
        "pfd_trib_info_block": (i, [p, i, p, f64, p, p, i]),
        "pfd_stream_order_classic_block": (i, [p, p, p, p, i, p, i, p, pi64]),
        "pfd_basins_begin": (i, [p, p, p, i64, i, p, i, p]),
        "pfd_basins_finish": (i, [p, p, i, i, pi]),
        "pfd_fill_depressions": (i, [i, p, i64, i64, f64, f64, i, i, f64, p, i64, i, p, p]),
        "pfd_ucat_area": (i, [p, p, i64, i, p, i, i, p, p]),
        "pfd_ucat_volume": (i, [p, p, i64, i, p, i, p, i, p, i, p, i64, p, i]),
        "pfd_segment_length": (i, [p, p, i64, i, i, p, p, i, p, p, i]),
        "pfd_segment_slope": (i, [p, p, i64, i, i, p, i, p, p, f64, p, i]),
        "pfd_segment_average": (i, [p, p, i64, i, i, p, p, i, p, i, p, f64, p, i]),
        "pfd_segment_median": (i, [p, p, i64, i, i, p, p, i, p, f64, p, i]),
        "pfd_subbasins_streamorder": (i, [p, i, p, i64, i, p, i64, pi64, p, i]),
        "pfd_outflow_idxs": (i, [p, p, i, p, i64, pi64, i]),
        "pfd_basin_outlets": (i, [p, i, p, i, p, p, i64, pi64, i]),
        "pfd_interbasin_mask": (i, [p, p, p, p, i]),
        "pfd_inflow_idxs": (i, [p, p, i, p, i64, pi64, i]),
        "pfd_basin_bounds": (i, [p, i, p, p, p, i64, pi64, i]),
        "pfd_subbasins_pfafstetter": (i, [p, i, p, f64, i, p, p, i64, i, p, i64, pi64, p, i]),
        "pfd_subbasins_area": (i, [p, i, p, f64, i, p, i, p, i64, pi64, p, p, i, i]),
        "pfd_streams": (i, [p, p, i, p, i64, p, p, i64, pi64, i]),
        "pfd_upscale": (i, [p, i, i64, i, p, p, i, p, p, i]),
        "pfd_upscale_outlets": (i, [p, i, i64, i, p, p, i, p, i]),
        "pfd_upscale_error": (i, [p, i, p, p, i64, p, i]),
        "pfd_downstream": (i, [p, i, p, p, i]),
        "pfd_moving_average": (i, [p, i64, i, p, i, p, i, p, i, p, f64, p, i]),
        "pfd_moving_median": (i, [p, i64, i, p, i, p, i, p, f64, p, i]),
        "pfd_path": (i, [p, p, i64, i, i, p, p, p, i, f64, p, i64, p, p, pi64, i]),
        "pfd_debug_window_wmax": (i, [i, pi]),
        "pfd_floodplains": (i, [p, i, p, p, p, p, i]),
        "pfd_snap_downstream": (i, [p, p, i64, p, i, i64, p, p]),
        "pfd_snap": (i, [p, p, i64, p, p, p, i, f64, p, p]),
        "pfd_set_profiling": (i, [p, i]),
        "pfd_last_timing": (i, [p, i, p, p, s, sz, pi]),
        "pfd_graph_stats": (i, [p, pi64]),
        "pfd_verify_upstream_area_cell": (i, [p, p, i, pi64]),
        "pfd_verify_basins": (i, [p, p, p, i64, p, i, pi64]),
        "pfd_verify_hand": (i, [p, p, i, p, p, i, pi64]),
        "pfd_checksum_i32": (i, [i, p, i64, pi64]),
        "pfd_count_nonfinite": (i, [i, i, p, i64, pi64]),
        "pfd_ew_compare": (i, [i, i, i, p, i, i64, f64, p, i64]),
        "pfd_ew_logic": (i, [i, i, p, p, p, i64]),
        "pfd_ew_where": (i, [i, i, p, p, p, i64, f64, p, i64]),
        "pfd_ew_convert": (i, [i, i, p, i, p, i64]),
        "pfd_ew_reduce": (i, [i, i, i, p, i64, pi64, pf64, pi]),
        "pfd_synth_d8": (i, synth),
        "pfd_synth_elev_f32": (i, synth),
        "pfd_synth_mosaic": (i, [i, p, i64, i64, i64, i64, p]),
        "pfd_calib_traffic": (i, [i, p, sz, i, i]),
        "pfd_synth_weights_f32": (i, [i, u64, i64, i64, p]),
    }


SIGNATURES = _signatures()
SYMBOLS = list(SIGNATURES)  # every symbol include/pfd.h declares

_lib = None


class HipLibraryMissing(ImportError):
    pass


def lib() -> C.CDLL:
    """Load libpfd_hip.so (once).  Raises HipLibraryMissing when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build the HIP extension first (python -m pyflwdir_amd.build, "
                "needs hipcc/ROCm).  pyflwdir_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().pfd_last_error().decode("utf-8", "replace")
        raise _ERRORS.get(rc, RuntimeError)(msg)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().pfd_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def ptr(a):
    """void* of a numpy array (None -> NULL) or pass-through for raw device addresses."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, DeviceBuffer):
        return C.c_void_p(a.addr)
    return C.c_void_p(int(a))


def _list_call(cap, alloc, call):
    """The protocol of the list calls (csrc/lists.h): the C call reports the count and leaves the lists unwritten when
    they do not fit ``cap`` entries; it is then made once more with room for exactly the count.  ``alloc(cap)`` returns
    the output arrays for a capacity, ``call(cap, arrays)`` makes the C call and returns the reported count.  Returns
    (arrays, count)."""
    arrays = alloc(cap)
    k = call(cap, arrays)
    if k > cap:
        cap, arrays = k, alloc(k)
        k = call(cap, arrays)
        if k > cap:
            raise RuntimeError(f"a list call reported {cap} entries, then {k}")
    return arrays, k


def _payload_pair(a):
    """(array or DeviceBuffer, dtype code) of a per-cell payload: a C-contiguous numpy array, or a ``(DeviceBuffer, code)``
    pair passed through."""
    if isinstance(a, tuple):
        return a
    a = np.ascontiguousarray(a)
    return a, _PAYLOAD_CODE[a.dtype]


# state record of the row-block floodplains (csrc/sweeps.hip FloodV): elevation / height threshold of the stream cell that
# started the floodplain, flag (1 floodplain, 0 not, -1 nodata), padding
FLOOD_STATE = np.dtype([("z", np.float32), ("h", np.float32), ("flag", np.int32), ("pad", np.int32)])


_explicit_reserve = False  # the caller sized an arena itself: the default one stands down
_auto_reserved = {}        # device -> bytes of the default arenas of this process
AUTO_RESERVE_MIN = 64 << 20
AUTO_RESERVE_BYTES_PER_CELL = 48


def reserve(nbytes: int, device: int = 0):
    """Reserve ``nbytes`` of HBM as one arena for the library's working buffers (``pfd_reserve``): afterwards a steady
    state never calls hipMalloc, whose latency for multi-GiB blocks is unpredictable (0.2 ms or seconds).  ``nbytes=0``
    releases the arenas that hold no live block.  A process that calls this sizes its arenas itself: the default arena
    of ``ensure_reserved`` is not added."""
    global _explicit_reserve
    check(lib().pfd_reserve(int(device), C.c_size_t(int(nbytes))))
    if nbytes:
        _explicit_reserve = True
    else:
        _auto_reserved.pop(int(device), None)


def mem_info(device: int = 0) -> dict:
    """Free and total HBM of ``device`` in bytes (``pfd_mem_info``)."""
    a = (C.c_int64 * 2)()
    check(lib().pfd_mem_info(int(device), a))
    return dict(free=int(a[0]), total=int(a[1]))


def ensure_reserved(n_cells: int, device: int = 0):
    """The default arena: the first handle of a process reserves
    ``min(0.5 x free HBM, 48 B x n_cells)`` — what the working buffers of the operations on a raster of ``n_cells`` need —
    so that the path a ``FlwdirRaster`` user takes is the path ``bench.py`` times; a later, larger raster adds the
    difference.  ``PFD_RESERVE_GIB`` overrides the size (``0``: no default arena); an explicit ``reserve()`` switches this
    off; arenas stay below half of the device's HBM in total and are released by ``reserve(0)``.  Failure to reserve is
    not an error: the class cache and hipMalloc remain."""
    if _explicit_reserve:
        return
    env = os.environ.get("PFD_RESERVE_GIB")
    have = _auto_reserved.get(int(device), 0)
    try:
        if env is not None:
            want = int(float(env) * 2**30)
            if want <= 0 or have:
                return
        else:
            want = AUTO_RESERVE_BYTES_PER_CELL * int(n_cells)
            if want - have < AUTO_RESERVE_MIN:
                return
            mi = mem_info(device)
            want = min(want - have, mi["free"] // 2, max(0, mi["total"] // 2 - have))
            if want < AUTO_RESERVE_MIN:
                return
        check(lib().pfd_reserve(int(device), C.c_size_t(int(want))))
        _auto_reserved[int(device)] = have + int(want)
    except (RuntimeError, MemoryError, ValueError):
        pass


def window_wmax(dtype) -> int:
    """The largest window (2n + 1 cells) ``moving_median`` sorts in LDS for float32 / float64 data; larger windows take
    the global workspace (``pfd_debug_window_wmax``)."""
    w = C.c_int(0)
    check(lib().pfd_debug_window_wmax(_FLOAT_CODE[np.dtype(dtype)], C.byref(w)))
    return int(w.value)


def transfer_stats(reset: bool = True) -> dict:
    """Host <-> device traffic of this thread's API calls since the last reset (``pfd_transfer_stats``)."""
    a = (C.c_double * 6)()
    check(lib().pfd_transfer_stats(a, 1 if reset else 0))
    keys = ("h2d_bytes", "h2d_ms", "d2h_bytes", "d2h_ms", "prefault_ms", "host_results")
    return {k: float(v) for k, v in zip(keys, a)}


def alloc_stats() -> dict:
    """Allocator counters since the process started (``pfd_alloc_stats``)."""
    a = (C.c_int64 * 8)()
    check(lib().pfd_alloc_stats(a))
    keys = ("hipmalloc_calls", "cache_hits", "near_fit_hits", "arena_blocks", "idle_bytes", "reserved_bytes", "reserved_free", "live_blocks")
    return {k: int(v) for k, v in zip(keys, a)}


# Bytes the Python side itself moves with DeviceBuffer.upload / download (pfd_memcpy_h2d / pfd_memcpy_d2h): those copies
# are no staging copies of an API call, so pfd_transfer_stats does not see them — DeviceArray's to_device and .numpy() are
# counted here, and a caller that wants ALL host <-> device traffic of a stretch of code reads both accounts.
_buffer_traffic = dict(h2d_bytes=0, h2d_copies=0, h2d_ms=0.0, d2h_bytes=0, d2h_copies=0, d2h_ms=0.0)


def buffer_transfer_stats(reset: bool = True) -> dict:
    """Host <-> device traffic of ``DeviceBuffer.upload`` / ``download`` in this process since the last reset: bytes, number
    of copies and wall milliseconds per direction.  The complement of ``transfer_stats`` (the staging copies inside the
    library's calls), which never counts these."""
    out = dict(_buffer_traffic)
    if reset:
        for k in _buffer_traffic:
            _buffer_traffic[k] = 0.0 if k.endswith("_ms") else 0
    return out


class DeviceBuffer:
    """A plain HBM allocation owned by Python (no torch): bench.py keeps the D8 raster and the
    result resident with these and passes them with memspace=PFD_DEVICE."""

    def __init__(self, nbytes: int, device: int = 0, pooled: bool = False):
        """``pooled``: from the library's caching allocator (``pfd_malloc_pooled``: the reserved arena, then cached blocks)
        instead of a ``hipMalloc`` of its own — for buffers that come and go with every call (``DeviceArray``)."""
        self.device, self.nbytes, self.pooled = device, int(nbytes), bool(pooled)
        p = C.c_void_p()
        alloc = lib().pfd_malloc_pooled if self.pooled else lib().pfd_malloc
        check(alloc(device, C.c_size_t(self.nbytes), C.byref(p)))
        self.addr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        t0 = time.perf_counter()
        check(lib().pfd_memcpy_h2d(self.device, C.c_void_p(self.addr), ptr(arr), C.c_size_t(arr.nbytes)))
        _buffer_traffic["h2d_bytes"] += arr.nbytes
        _buffer_traffic["h2d_copies"] += 1
        _buffer_traffic["h2d_ms"] += (time.perf_counter() - t0) * 1e3
        return self

    def download(self, dtype, shape, offset_bytes: int = 0, out=None) -> np.ndarray:
        """``out``: a C-contiguous array of that dtype and size to fill (e.g. a block's rows of the whole result)."""
        if out is None:
            out = np.empty(shape, dtype)
        assert out.dtype == np.dtype(dtype) and out.flags.c_contiguous and out.size == int(np.prod(shape))
        assert out.nbytes + offset_bytes <= self.nbytes
        t0 = time.perf_counter()
        check(lib().pfd_memcpy_d2h(self.device, ptr(out), C.c_void_p(self.addr + offset_bytes), C.c_size_t(out.nbytes)))
        _buffer_traffic["d2h_bytes"] += out.nbytes
        _buffer_traffic["d2h_copies"] += 1
        _buffer_traffic["d2h_ms"] += (time.perf_counter() - t0) * 1e3
        return out

    def free(self):
        if self.addr:
            release = lib().pfd_free_pooled if self.pooled else lib().pfd_free
            check(release(self.device, C.c_void_p(self.addr)))
            self.addr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RasterHandle:
    """Owner of one ``pfd_raster`` (device-side graph of one raster on one GPU)."""

    def __init__(self, d8, nrow: int, ncol: int, device: int = 0, memspace: int = PFD_HOST, halo=(0, 0),
                 deferred: bool = False):
        """``nrow`` counts the OWNED rows; with ``halo=(top, bottom)`` (row block of a multi-GPU job) ``d8``
        holds top + nrow + bottom rows.  ``deferred``: decode/validate inside the first operation
        (``pfd_raster_create_deferred``); a device buffer ``d8`` is then referenced until that operation."""
        self._h = C.c_void_p()
        self.nrow, self.ncol, self.n = int(nrow), int(ncol), int(nrow) * int(ncol)
        self.device = device
        self.halo = (int(halo[0]), int(halo[1]))
        self.is_general = False
        if isinstance(d8, np.ndarray):
            d8 = np.ascontiguousarray(d8, dtype=np.uint8)
            assert d8.size == (self.nrow + sum(self.halo)) * self.ncol
        self._d8_ref = d8 if deferred else None  # keep a referenced device buffer alive
        ensure_reserved((self.nrow + sum(self.halo)) * self.ncol, device)
        if deferred:
            check(lib().pfd_raster_create_deferred(ptr(d8), self.nrow, self.ncol, self.halo[0], self.halo[1],
                                                   memspace, device, C.byref(self._h)))
        elif self.halo == (0, 0):
            check(lib().pfd_raster_create(ptr(d8), self.nrow, self.ncol, memspace, device, C.byref(self._h)))
        else:
            check(lib().pfd_raster_create_block(ptr(d8), self.nrow, self.ncol, self.halo[0], self.halo[1], memspace,
                                                device, C.byref(self._h)))

    @classmethod
    def general(cls, idxs_ds: np.ndarray, nrow: int, ncol: int, device: int = 0):
        """Handle of a general ``idxs_ds`` graph (links outside the 8 neighbours; pfd_raster_create_general)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.nrow, self.ncol, self.n = int(nrow), int(ncol), int(nrow) * int(ncol)
        self.device, self.halo, self._d8_ref, self.is_general = device, (0, 0), None, True
        idxs_ds = np.ascontiguousarray(idxs_ds).ravel()
        assert idxs_ds.size == self.n
        ensure_reserved(self.n, device)
        check(lib().pfd_raster_create_general(ptr(idxs_ds), IDX_CODE[idxs_ds.dtype], self.nrow, self.ncol, PFD_HOST, device,
                                              C.byref(self._h)))
        return self

    def close(self):
        if self._h:
            lib().pfd_raster_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- info -------------------------------------------------------------------------------
    def validate(self):
        """Normalise + validate a deferred handle now (counts become available)."""
        check(lib().pfd_raster_validate(self._h))

    def info(self, counts: bool = False) -> dict:
        if counts:
            self.validate()
        a = (C.c_int64 * 8)()
        check(lib().pfd_raster_info(self._h, a))
        keys = ["nrow", "ncol", "n_valid", "n_pits", "n_seq", "n_levels", "device", "bytes_held"]
        return dict(zip(keys, [int(v) for v in a]))

    def graph_stats(self) -> dict:
        """n_valid, n_pits, max_rank (longest flow path; -1 with cycles, -2 unknown: beyond the tiled query) and the in-degree histogram."""
        a = (C.c_int64 * 16)()
        check(lib().pfd_graph_stats(self._h, a))
        ntiles = max(1, -(-self.nrow // 64) * -(-self.ncol // 64))
        return dict(n_valid=int(a[0]), n_pits=int(a[1]), max_rank=int(a[2]), indegree_hist=[int(a[3 + k]) for k in range(9)],
                    tile_rounds=dict(local_max=int(a[12]), local_mean=round(int(a[13]) / ntiles, 2), final_max=int(a[14]),
                                     final_mean=round(int(a[15]) / ntiles, 2)))

    def verify_upstream_area_cell(self, upa, memspace=PFD_HOST) -> dict:
        """Local-equation check of an upstream_area("cell") result (see include/pfd.h)."""
        a = (C.c_int64 * 8)()
        check(lib().pfd_verify_upstream_area_cell(self._h, ptr(upa), memspace, a))
        return dict(bad_cells=int(a[0]), bad_nodata=int(a[1]), pit_sum=int(a[2]), n_pits=int(a[3]), checksum=int(a[4]),
                    n_valid=int(a[5]))

    def set_block_io(self, seed_memspace):
        """Where the ``*_block`` sweeps read their halo seeds from (PFD_HOST / PFD_DEVICE)."""
        check(lib().pfd_set_block_io(self._h, int(seed_memspace)))

    def set_block_update(self, mode):
        """What the next up-sweep of this block keeps / reuses (include/pfd.h pfd_set_block_update): 0 nothing, 1 keep
        the sweep, 2 update the kept sweep's result for the halo seeds that changed."""
        check(lib().pfd_set_block_update(self._h, int(mode)))

    def set_profiling(self, on=True):  # (2: also count the doubling rounds of the tile passes, see graph_stats)
        check(lib().pfd_set_profiling(self._h, int(on)))

    def last_timing(self):
        ms = (C.c_double * 16)()
        ln = (C.c_int64 * 16)()
        names = C.create_string_buffer(512)
        k = C.c_int(0)
        check(lib().pfd_last_timing(self._h, 16, ms, ln, names, 512, C.byref(k)))
        nm = names.value.decode().split(";") if k.value else []
        return [dict(name=nm[i], ms=ms[i], launches=int(ln[i])) for i in range(k.value)]

    # -- graph exports ----------------------------------------------------------------------
    def idxs_ds(self, dtype) -> np.ndarray:
        out = np.empty(self.n, dtype)
        check(lib().pfd_idxs_ds(self._h, IDX_CODE[np.dtype(dtype)], ptr(out), PFD_HOST))
        return out

    def idxs_pit(self, dtype) -> np.ndarray:
        out = np.empty(self.info(counts=True)["n_pits"], dtype)
        check(lib().pfd_idxs_pit(self._h, IDX_CODE[np.dtype(dtype)], ptr(out), PFD_HOST))
        return out

    def order_cells(self):
        check(lib().pfd_order_cells(self._h))

    def wide_cells(self) -> bool:
        """The handle's cells need 64-bit indices (csrc/order64.hip: rank and idxs_seq without the level engine)."""
        return self.n > 4294967294 or (os.environ.get("PFD_ENABLE_KNOBS") == "1" and bool(os.environ.get("PFD_TEST_ORDER64")))

    def idxs_seq(self, dtype) -> np.ndarray:
        if self.wide_cells() and not self.is_general:
            out = np.empty(self.info(counts=True)["n_valid"], np.int64)  # (room for every valid cell; cells that never
            check(lib().pfd_idxs_seq(self._h, PFD_I64, ptr(out), PFD_HOST))  # reach a pit are left out: n_seq entries)
            return out[: self.info()["n_seq"]].astype(dtype, copy=False)
        self.order_cells()
        out = np.empty(self.info()["n_seq"], dtype)
        check(lib().pfd_idxs_seq(self._h, IDX_CODE[np.dtype(dtype)], ptr(out), PFD_HOST))
        return out

    def set_idxs_seq(self, seq: np.ndarray):
        """General graphs: install the host's cell sequence (order_cells("sort")) as the order of the sweeps."""
        seq = np.ascontiguousarray(seq)
        check(lib().pfd_set_idxs_seq(self._h, IDX_CODE[seq.dtype], ptr(seq), seq.size))

    def clear_idxs_seq(self):
        """General graphs: forget an installed sequence (back to the breadth-first order of core.idxs_seq)."""
        check(lib().pfd_set_idxs_seq(self._h, PFD_I32, None, 0))

    def rank(self) -> np.ndarray:
        out = np.empty(self.n, np.int32)
        check(lib().pfd_rank(self._h, ptr(out), PFD_HOST))
        return out

    def upstream_count(self, mask=None) -> np.ndarray:
        out = np.empty(self.n, np.int8)
        m = None if mask is None else np.ascontiguousarray(mask).astype(np.uint8, copy=False).ravel()
        check(lib().pfd_upstream_count(self._h, ptr(m), ptr(out), PFD_HOST))
        return out

    def add_pits(self, idxs):
        idxs = np.ascontiguousarray(idxs, dtype=np.int64).ravel()
        check(lib().pfd_add_pits(self._h, ptr(idxs), idxs.size))

    # -- sweeps -----------------------------------------------------------------------------
    def upstream_area_cell(self, out=None, memspace=PFD_HOST, engine="auto"):
        f = lib().pfd_upstream_area_cell if engine == "auto" else lib().pfd_upstream_area_cell_levels
        if memspace == PFD_HOST:
            out = np.empty(self.n, np.int32)
        check(f(self._h, ptr(out), memspace))
        return out

    def accuflux(self, data, dtype_code, nodata_i=0, nodata_f=0.0, has_nodata=1, direction=PFD_UP,
                 mask_invalid=0, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty_like(data)
        check(lib().pfd_accuflux(self._h, dtype_code, ptr(data), int(nodata_i), float(nodata_f), int(has_nodata),
                                 direction, int(mask_invalid), ptr(out), memspace))
        return out

    def accuflux_rows(self, row_values, dtype_code, nodata_i=0, nodata_f=0.0, has_nodata=1, direction=PFD_UP,
                      mask_invalid=0, out=None, memspace=PFD_HOST):
        """accuflux of a payload that is constant along raster rows (``row_values``: nrow host values)."""
        row_values = np.ascontiguousarray(row_values)
        assert row_values.size == self.nrow
        if memspace == PFD_HOST:
            out = np.empty(self.n, row_values.dtype)
        check(lib().pfd_accuflux_rows(self._h, dtype_code, ptr(row_values), int(nodata_i), float(nodata_f),
                                      int(has_nodata), direction, int(mask_invalid), ptr(out), memspace))
        return out

    def upstream_area_rows_fixed(self, row_values, out=None, memspace=PFD_HOST):
        """Order-free upstream sums of one float64 value per row in 64-bit fixed point (pfd_upstream_area_rows_fixed).
        Returns (out, quantum), or (None, 0.0) when the library did not take the call (the caller runs accuflux_rows)."""
        row_values = np.ascontiguousarray(row_values, dtype=np.float64)
        assert row_values.size == self.nrow
        if memspace == PFD_HOST:
            out = np.empty(self.n, np.float64)
        used, quantum = C.c_int(0), C.c_double(0.0)
        check(lib().pfd_upstream_area_rows_fixed(self._h, ptr(row_values), ptr(out), memspace, C.byref(used),
                                                 C.byref(quantum)))
        return (out, quantum.value) if used.value else (None, 0.0)

    def strahler(self, mask=None, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty(self.n, np.uint8)
        check(lib().pfd_strahler(self._h, ptr(mask), ptr(out), memspace))
        return out

    def basins(self, outlets, ids, out=None, memspace=PFD_HOST):
        outlets = np.ascontiguousarray(outlets, dtype=np.int64).ravel()
        ids = np.ascontiguousarray(ids).ravel()
        if memspace == PFD_HOST:
            out = np.empty(self.n, ids.dtype)
        check(lib().pfd_basins(self._h, ptr(outlets), ptr(ids), outlets.size, ids.dtype.itemsize, ptr(out), memspace))
        return out

    def hand(self, drain, elevtn, elev_code, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty(self.n, np.float64)
        check(lib().pfd_hand(self._h, ptr(drain), elev_code, ptr(elevtn), ptr(out), memspace))
        return out

    def hand_block(self, drain, elevtn, elev_code, halo_seed, out=None, memspace=PFD_HOST, update=False):
        """HAND of a row block whose halo cells take their height from ``halo_seed`` (2 * ncol float64, host); drain,
        elevtn and the result cover the block's device raster (own + halo rows).  ``update``: ``out`` holds an earlier
        result, only its unknown (-inf) cells are recomputed.  Returns (out, boundary rows [2, ncol], unknown own cells)."""
        brows = None
        if not isinstance(halo_seed, DeviceBuffer):  # (a DeviceBuffer: pfd_set_block_io(PFD_DEVICE), rows stay on the device)
            halo_seed = np.ascontiguousarray(halo_seed, dtype=np.float64)
            assert halo_seed.size == 2 * self.ncol
            brows = np.empty((2, self.ncol), np.float64)
        if memspace == PFD_HOST and out is None:
            assert not update
            out = np.empty((self.nrow + sum(self.halo)) * self.ncol, np.float64)
        unk = C.c_int64(0)
        check(lib().pfd_hand_block(self._h, ptr(drain), elev_code, ptr(elevtn), ptr(halo_seed), 1 if update else 0, ptr(out),
                                   memspace, ptr(brows), C.byref(unk)))
        return out, brows, int(unk.value)

    def _block_sweep(self, halo_seed, dtype, call, code=None):
        """The frame of the pfd_*_block sweeps: ``halo_seed`` is 2 * ncol host values (``dtype``: None keeps the array's;
        ``code``: the payload code they must have) or a DeviceBuffer (pfd_set_block_io(PFD_DEVICE): the boundary rows stay
        on the device); ``call(seed, brows, bad)`` makes the C call.  Returns (boundary rows [2, ncol] or None, own cells
        failing their local equation — verify only)."""
        brows = None
        if not isinstance(halo_seed, DeviceBuffer):
            halo_seed = np.ascontiguousarray(halo_seed, dtype=dtype)
            assert halo_seed.size == 2 * self.ncol and (code is None or _PAYLOAD_CODE[halo_seed.dtype] == code)
            brows = np.empty((2, self.ncol), halo_seed.dtype)
        bad = C.c_int64(0)
        check(call(ptr(halo_seed), ptr(brows), C.byref(bad)))
        return brows, int(bad.value)

    def accuflux_block(self, data, dtype_code, halo_seed, out, nodata_i=0, nodata_f=0.0, has_nodata=0, by_row=False,
                       verify=False, memspace=PFD_HOST, direction=PFD_UP):
        """accuflux (either direction) of a row block whose halo cells hold ``halo_seed`` (2 * ncol values of the result
        type, host); data and ``out`` cover the block's device raster (own + halo rows), ``by_row``: one host value per
        device row.  Returns (boundary rows [2, ncol], own cells failing their local equation — verify only)."""
        return self._block_sweep(halo_seed, None, lambda seed, brows, bad: lib().pfd_accuflux_block(
            self._h, dtype_code, ptr(data), 1 if by_row else 0, int(nodata_i), float(nodata_f), int(has_nodata),
            int(direction), seed, 1 if verify else 0, ptr(out), memspace, brows, bad), code=dtype_code)

    def fillnodata(self, data, dtype_code, nodata_i=0, nodata_f=0.0, has_nodata=1, direction=PFD_DOWN, how=PFD_FILL_MAX,
                   out=None, memspace=PFD_HOST):
        """fillnodata (pfd_fillnodata): ``data`` in the lane type of ``dtype_code`` (int32 lanes for the narrow codes)."""
        if memspace == PFD_HOST:
            out = np.empty_like(data)
        check(lib().pfd_fillnodata(self._h, dtype_code, ptr(data), int(nodata_i), float(nodata_f), int(has_nodata),
                                   int(direction), int(how), ptr(out), memspace))
        return out

    def fillnodata_block(self, data, dtype_code, halo_seed, out, nodata_i=0, nodata_f=0.0, has_nodata=0,
                         direction=PFD_DOWN, how=PFD_FILL_MAX, verify=False, memspace=PFD_HOST):
        """fillnodata of a row block whose halo cells hold ``halo_seed`` (2 * ncol values of the lane type, host); data
        and ``out`` cover the block's device raster.  Returns (boundary rows [2, ncol], failing own cells — verify only)."""
        return self._block_sweep(halo_seed, None, lambda seed, brows, bad: lib().pfd_fillnodata_block(
            self._h, dtype_code, ptr(data), int(nodata_i), float(nodata_f), int(has_nodata), int(direction), int(how), seed,
            1 if verify else 0, ptr(out), memspace, brows, bad))

    def stream_distance_block(self, mask, step_lengths, halo_seed, out, verify=False, memspace=PFD_HOST):
        """stream_distance of a row block whose halo cells hold ``halo_seed`` (2 * ncol int32, or float32 with
        ``step_lengths``: the table rows of the block's device raster).  Returns (boundary rows, failing own cells)."""
        real = step_lengths is not None
        if real:
            step_lengths = np.ascontiguousarray(step_lengths, dtype=np.float32)
            assert step_lengths.size == 3 * (2 * (self.nrow + sum(self.halo)) - 1)
        return self._block_sweep(halo_seed, np.float32 if real else np.int32, lambda seed, brows, bad:
                                 lib().pfd_stream_distance_block(self._h, ptr(mask), int(real), ptr(step_lengths), seed,
                                                                 1 if verify else 0, ptr(out), memspace, brows, bad))

    def trib_info_block(self, uparea, dtype_code, mask=None, upa_min=0.0, out=None, memspace=PFD_HOST):
        """One byte per cell of the block's device raster: slot of the main upstream cell | (more than one upstream cell
        inside the mask) << 4 (include/pfd.h pfd_trib_info_block); the halo rows are the caller's to fill in."""
        if memspace == PFD_HOST:
            out = np.empty((self.nrow + sum(self.halo)) * self.ncol, np.uint8)
        check(lib().pfd_trib_info_block(self._h, int(dtype_code), ptr(uparea), float(upa_min), ptr(mask), ptr(out), memspace))
        return out

    def stream_order_classic_block(self, tinfo, mask, halo_seed, out, verify=False, memspace=PFD_HOST):
        """Classic stream order of a row block whose halo cells hold ``halo_seed`` (2 * ncol uint8).  Returns (boundary
        rows [2, ncol], own cells failing their local equation — verify only)."""
        return self._block_sweep(halo_seed, np.uint8, lambda seed, brows, bad: lib().pfd_stream_order_classic_block(
            self._h, ptr(tinfo), ptr(mask), seed, 1 if verify else 0, ptr(out), memspace, brows, bad))

    def floodplains_block(self, elevtn, elev_code, is_stream, stream_h, halo_seed, state, verify=False, memspace=PFD_HOST):
        """dem.floodplains of a row block whose halo cells hold the floodplain state ``halo_seed`` (2 * ncol records of
        FLOOD_STATE, host, or a DeviceBuffer after set_block_io); ``state`` covers the block's device raster.  Returns
        (boundary rows [2, ncol] of FLOOD_STATE, own cells failing their local equation — verify only)."""
        return self._block_sweep(halo_seed, FLOOD_STATE, lambda seed, brows, bad: lib().pfd_floodplains_block(
            self._h, int(elev_code), ptr(elevtn), ptr(is_stream), ptr(stream_h), seed, 1 if verify else 0, ptr(state),
            memspace, brows, bad))

    def floodplains_block_flags(self, state: "DeviceBuffer", out=None) -> np.ndarray:
        """int8 flags of the block's own rows from its device-resident floodplain state (pfd_floodplains_block_flags);
        ``out``: a C-contiguous int8 array of own_rows * ncol cells to fill (e.g. the block's rows of the whole result)."""
        if out is None:
            out = np.empty((self.nrow, self.ncol), np.int8)
        assert out.dtype == np.int8 and out.flags.c_contiguous and out.size == self.nrow * self.ncol
        check(lib().pfd_floodplains_block_flags(self._h, ptr(state), ptr(out), PFD_HOST))
        return out

    def strahler_block(self, mask, halo_seed, out, verify=False, memspace=PFD_HOST):
        """Strahler order of a row block whose halo cells hold ``halo_seed`` (2 * ncol uint8, host).  Returns
        (boundary rows [2, ncol], own cells failing their local equation — verify only)."""
        return self._block_sweep(halo_seed, np.uint8, lambda seed, brows, bad: lib().pfd_strahler_block(
            self._h, ptr(mask), seed, 1 if verify else 0, ptr(out), memspace, brows, bad))

    def verify_basins(self, outlets, ids, labels, memspace=PFD_HOST) -> dict:
        """Local-equation check of a basins() result with uint32 ids (see include/pfd.h)."""
        outlets = np.ascontiguousarray(outlets, dtype=np.int64).ravel()
        ids = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        a = (C.c_int64 * 4)()
        check(lib().pfd_verify_basins(self._h, ptr(outlets), ptr(ids), outlets.size, ptr(labels), memspace, a))
        return dict(bad_cells=int(a[0]), bad_nodata=int(a[1]), checksum=int(a[2]), n_labelled=int(a[3]))

    def verify_hand(self, drain, elevtn, elev_code, hand, memspace=PFD_HOST) -> dict:
        """Local-equation check of a HAND result, bit for bit (see include/pfd.h)."""
        a = (C.c_int64 * 4)()
        check(lib().pfd_verify_hand(self._h, ptr(drain), elev_code, ptr(elevtn), ptr(hand), memspace, a))
        return dict(bad_cells=int(a[0]), bad_nodata=int(a[1]), checksum=int(a[2]), n_drain=int(a[3]))

    def ucat_area(self, idxs_out, map_dtype, area_rows=None):
        """(map[n] of map_dtype, area[k]); area_rows None: int32 cell counts, else nrow float32/float64 row areas."""
        idxs_out = np.ascontiguousarray(idxs_out, dtype=np.int64).ravel()
        ucmap = np.empty(self.n, map_dtype)
        if area_rows is None:
            code, are = PFD_I32, np.empty(idxs_out.size, np.int32)
        else:
            area_rows = np.ascontiguousarray(area_rows)
            assert area_rows.size == self.nrow and area_rows.dtype in (np.float32, np.float64)
            code, are = (PFD_F32 if area_rows.dtype == np.float32 else PFD_F64), np.empty(idxs_out.size, area_rows.dtype)
        check(lib().pfd_ucat_area(self._h, ptr(idxs_out), idxs_out.size, IDX_CODE[np.dtype(map_dtype)], ptr(ucmap), PFD_HOST,
                                  code, ptr(area_rows), ptr(are)))
        return ucmap, are

    def ucat_volume(self, idxs_out, map_dtype, hand, area_rows, depths, map_out=None, vol_out=None, memspace=PFD_HOST):
        """(map[n] of map_dtype, volume[depths.size, k] in the dtype of ``depths``) of pfd_ucat_volume; ``hand`` float32 /
        float64 per cell, ``area_rows`` nrow float32 / float64 row areas.  PFD_DEVICE: ``hand`` (pass its dtype code as a
        ``(DeviceBuffer, code)`` pair), ``map_out`` and ``vol_out`` are DeviceBuffers and are returned as given."""
        idxs_out = np.ascontiguousarray(idxs_out, dtype=np.int64).ravel()
        area_rows, depths = np.ascontiguousarray(area_rows), np.ascontiguousarray(depths)
        assert area_rows.size == self.nrow
        hand, hcode = _payload_pair(hand)
        if memspace == PFD_HOST:
            map_out, vol_out = np.empty(self.n, map_dtype), np.empty((depths.size, idxs_out.size), depths.dtype)
        check(lib().pfd_ucat_volume(self._h, ptr(idxs_out), idxs_out.size, IDX_CODE[np.dtype(map_dtype)], ptr(map_out), hcode,
                                    ptr(hand), _FLOAT_CODE[area_rows.dtype], ptr(area_rows), _FLOAT_CODE[depths.dtype],
                                    ptr(depths), depths.size, ptr(vol_out), memspace))
        return map_out, vol_out

    # -- river segments between unit-catchment outlets (csrc/subgrid.hip).  ``idxs_out``: int64, < 0 = missing.  PFD_HOST:
    #    per-cell arguments are numpy arrays and the result is a new array; PFD_DEVICE: they are DeviceBuffers — payloads as
    #    ``(DeviceBuffer, dtype code)`` pairs, ``idxs_us_main`` as ``(DeviceBuffer, numpy dtype)`` — and ``out`` is returned.
    def _segment_args(self, idxs_out, idxs_us_main):
        idxs_out = np.ascontiguousarray(idxs_out, dtype=np.int64).ravel()
        if idxs_us_main is None:
            return idxs_out, None, PFD_I64
        if isinstance(idxs_us_main, tuple):
            return idxs_out, idxs_us_main[0], IDX_CODE[np.dtype(idxs_us_main[1])]
        idxs_us_main = np.ascontiguousarray(idxs_us_main).ravel()
        assert idxs_us_main.size == self.n
        return idxs_out, idxs_us_main, IDX_CODE[idxs_us_main.dtype]

    def segment_length(self, idxs_out, direction, idxs_us_main, mask, distnc, out=None, memspace=PFD_HOST):
        idxs_out, us, icode = self._segment_args(idxs_out, idxs_us_main)
        distnc, dcode = _payload_pair(distnc)
        if memspace == PFD_HOST:
            out = np.empty(idxs_out.size, distnc.dtype)
        check(lib().pfd_segment_length(self._h, ptr(idxs_out), idxs_out.size, int(direction), icode, ptr(us), ptr(mask), dcode,
                                       ptr(distnc), ptr(out), memspace))
        return out

    def segment_slope(self, idxs_out, direction, idxs_us_main, elevtn, distnc, length=1000, out=None, memspace=PFD_HOST):
        idxs_out, us, icode = self._segment_args(idxs_out, idxs_us_main)
        elevtn, ecode = _payload_pair(elevtn)
        if memspace == PFD_HOST:
            assert distnc.dtype == np.float32
            out = np.empty(idxs_out.size, np.float32 if direction == PFD_BOTH else elevtn.dtype)
        check(lib().pfd_segment_slope(self._h, ptr(idxs_out), idxs_out.size, int(direction), icode, ptr(us), ecode, ptr(elevtn),
                                      ptr(distnc), float(length), ptr(out), memspace))
        return out

    def segment_average(self, idxs_out, direction, idxs_us_main, mask, data, weights=None, nodata=-9999.0, out=None,
                        memspace=PFD_HOST):
        """``weights`` None: float32 ones (the reference's default)."""
        idxs_out, us, icode = self._segment_args(idxs_out, idxs_us_main)
        data, dcode = _payload_pair(data)
        weights, wcode = (None, PFD_F32) if weights is None else _payload_pair(weights)
        if memspace == PFD_HOST:
            out = np.empty(idxs_out.size, data.dtype)
        check(lib().pfd_segment_average(self._h, ptr(idxs_out), idxs_out.size, int(direction), icode, ptr(us), ptr(mask), dcode,
                                        ptr(data), wcode, ptr(weights), float(nodata), ptr(out), memspace))
        return out

    def segment_median(self, idxs_out, direction, idxs_us_main, mask, data, nodata=-9999.0, out=None, memspace=PFD_HOST):
        idxs_out, us, icode = self._segment_args(idxs_out, idxs_us_main)
        data, dcode = _payload_pair(data)
        if memspace == PFD_HOST:
            out = np.empty(idxs_out.size, data.dtype)
        check(lib().pfd_segment_median(self._h, ptr(idxs_out), idxs_out.size, int(direction), icode, ptr(us), ptr(mask), dcode,
                                       ptr(data), float(nodata), ptr(out), memspace))
        return out

    # -- windows along the flow path (csrc/window.hip).  PFD_HOST: per-cell arguments are numpy arrays and the result is a
    #    new array; PFD_DEVICE: they are DeviceBuffers — payloads as ``(DeviceBuffer, dtype code)`` pairs, ``idxs_us_main``
    #    as ``(DeviceBuffer, numpy dtype)``, ``strord`` as ``(DeviceBuffer, STRORD code)`` — and ``out`` is returned.
    def downstream(self, data, elem_bytes=None, out=None, memspace=PFD_HOST):
        """data[idxs_ds] on valid cells, data elsewhere; elements of 1, 2, 4 or 8 bytes of any dtype."""
        if memspace == PFD_HOST:
            data = np.ascontiguousarray(data).ravel()
            assert data.size == self.n
            elem_bytes, out = data.dtype.itemsize, np.empty_like(data)
        check(lib().pfd_downstream(self._h, int(elem_bytes), ptr(data), ptr(out), memspace))
        return out

    def _window_args(self, idxs_us_main, strord):
        _, us, icode = self._segment_args((), idxs_us_main)
        if strord is None:
            return us, icode, None, 0
        if isinstance(strord, tuple):
            return us, icode, strord[0], int(strord[1])
        strord = np.ascontiguousarray(strord).ravel()
        assert strord.size == self.n
        return us, icode, strord, STRORD_CODE[strord.dtype]

    def moving_average(self, n, idxs_us_main, data, weights=None, strord=None, nodata=-9999.0, out=None, memspace=PFD_HOST):
        """``weights`` None: float64 ones (the reference's default); ``strord`` uint8 / int32 / uint32 / int64 or None."""
        us, icode, so, scode = self._window_args(idxs_us_main, strord)
        data, dcode = _payload_pair(data)
        weights, wcode = (None, PFD_F64) if weights is None else _payload_pair(weights)
        if memspace == PFD_HOST:
            out = np.empty(self.n, data.dtype)
        check(lib().pfd_moving_average(self._h, int(n), icode, ptr(us), scode, ptr(so), dcode, ptr(data), wcode, ptr(weights),
                                       float(nodata), ptr(out), memspace))
        return out

    def moving_median(self, n, idxs_us_main, data, strord=None, nodata=-9999.0, out=None, memspace=PFD_HOST):
        us, icode, so, scode = self._window_args(idxs_us_main, strord)
        data, dcode = _payload_pair(data)
        if memspace == PFD_HOST:
            out = np.empty(self.n, data.dtype)
        check(lib().pfd_moving_median(self._h, int(n), icode, ptr(us), scode, ptr(so), dcode, ptr(data), float(nodata),
                                      ptr(out), memspace))
        return out

    def path(self, idxs, direction, idx_dtype, idxs_us_main=None, mask=None, step_lengths=None, max_length=None,
             idxs_out=None, offsets_out=None, dist_out=None, cap_idxs=None, memspace=PFD_HOST):
        """The paths of pfd_path as a CSR pair plus distances: (cells[M] of ``idx_dtype``, offsets[k + 1] int64, float64
        dists[k]).  PFD_DEVICE: ``idxs_us_main``, ``mask`` and the three lists (``cap_idxs`` cells; None with a cap of 0: a
        sizing call) are DeviceBuffers; returns M, the lists are written when they fit."""
        idxs = np.ascontiguousarray(idxs, dtype=np.int64).ravel()
        k, m = idxs.size, C.c_int64(0)
        code = IDX_CODE[np.dtype(idx_dtype)]
        tab = None if step_lengths is None else np.ascontiguousarray(step_lengths, dtype=np.float64)
        has_max, mx = (0, 0.0) if max_length is None else (1, float(max_length))
        if isinstance(idxs_us_main, tuple):
            idxs_us_main = idxs_us_main[0]

        def run(cells, cap, offsets, dists, space):
            check(lib().pfd_path(self._h, ptr(idxs), k, int(direction), code, ptr(idxs_us_main), ptr(mask), ptr(tab), has_max,
                                 C.c_double(mx), ptr(cells), int(cap), ptr(offsets), ptr(dists), C.byref(m), space))
            return int(m.value)
        if memspace != PFD_HOST:
            return run(idxs_out, cap_idxs or 0, offsets_out, dist_out, memspace)
        (cells, offsets, dists), n = _list_call(
            max(4096, 64 * k), lambda cap: (np.empty(cap, idx_dtype), np.zeros(k + 1, np.int64), np.zeros(k, np.float64)),
            lambda cap, a: run(a[0], cap, a[1], a[2], PFD_HOST))
        return cells[:n].copy(), offsets, dists

    # -- outlets derived from the network (csrc/outlets.hip) ------------------------------------------------------
    def _outlet_cap(self):
        """Room for the outlet list of a first call: the C entry points report the count and leave the list unwritten when
        it does not fit; the call is then repeated with room for all of them."""
        return max(4096, self.n // 16)

    def subbasins_streamorder(self, strord, dtype_code, min_sto, idx_dtype, cap=None, out=None, idxs_out=None,
                              memspace=PFD_HOST):
        """(int32 map[n], outlet cells[k]) of pfd_subbasins_streamorder.  PFD_DEVICE: ``strord``, ``out`` and ``idxs_out``
        (``cap`` entries) are DeviceBuffers; returns (out, idxs_out, k)."""
        k = C.c_int64(0)

        def run(cap, idxs, space):
            check(lib().pfd_subbasins_streamorder(self._h, int(dtype_code), ptr(strord), int(min_sto),
                                                  IDX_CODE[np.dtype(idx_dtype)], ptr(idxs), int(cap), C.byref(k), ptr(out), space))
            return int(k.value)
        if memspace != PFD_HOST:
            return out, idxs_out, run(cap, idxs_out, memspace)
        out = np.empty(self.n, np.int32)
        idxs, n = _list_call(self._outlet_cap() if cap is None else int(cap), lambda cap: np.empty(cap, idx_dtype),
                             lambda cap, idxs: run(cap, idxs, PFD_HOST))
        return out, idxs[:n].copy()

    def outflow_idxs(self, region, idx_dtype, cap=None):
        """Outflow cells of a uint8 region mask in forward sequence order (pfd_outflow_idxs)."""
        k = C.c_int64(0)

        def run(cap, idxs):
            check(lib().pfd_outflow_idxs(self._h, ptr(region), IDX_CODE[np.dtype(idx_dtype)], ptr(idxs), cap, C.byref(k),
                                         PFD_HOST))
            return int(k.value)
        idxs, n = _list_call(self._outlet_cap() if cap is None else int(cap), lambda cap: np.empty(cap, idx_dtype), run)
        return idxs[:n].copy()

    def basin_outlets(self, regions, dtype_code, idx_dtype, cap=None):
        """(labels[k] in the dtype of ``regions``, outlet cells[k]) sorted by label (pfd_basin_outlets)."""
        k = C.c_int64(0)

        def run(cap, a):
            check(lib().pfd_basin_outlets(self._h, int(dtype_code), ptr(regions), IDX_CODE[np.dtype(idx_dtype)], ptr(a[0]),
                                          ptr(a[1]), cap, C.byref(k), PFD_HOST))
            return int(k.value)
        (idxs, lbs), n = _list_call(self._outlet_cap() if cap is None else int(cap),
                                    lambda cap: (np.empty(cap, idx_dtype), np.empty(cap, regions.dtype)), run)
        return lbs[:n].copy(), idxs[:n].copy()

    # -- the rest of the BASINS section (csrc/basins_ext.hip) ---------------------------------------------------------
    def interbasin_mask(self, region, stream):
        """uint8 mask[n] of pfd_interbasin_mask; ``region`` uint8, ``stream`` uint8 or None."""
        out = np.empty(self.n, np.uint8)
        check(lib().pfd_interbasin_mask(self._h, ptr(region), ptr(stream), ptr(out), PFD_HOST))
        return out

    def inflow_idxs(self, region, idx_dtype, cap=None):
        """Inflow cells of a uint8 region mask in reversed sequence order (pfd_inflow_idxs)."""
        k = C.c_int64(0)

        def run(cap, idxs):
            check(lib().pfd_inflow_idxs(self._h, ptr(region), IDX_CODE[np.dtype(idx_dtype)], ptr(idxs), cap, C.byref(k),
                                        PFD_HOST))
            return int(k.value)
        idxs, n = _list_call(self._outlet_cap() if cap is None else int(cap), lambda cap: np.empty(cap, idx_dtype), run)
        return idxs[:n].copy()

    def basin_bounds(self, labels, dtype_code, cap=None):
        """(sorted unique labels[k] > 0, int64 [4, k] = row_min, row_max, col_min, col_max) of pfd_basin_bounds."""
        k = C.c_int64(0)

        def run(cap, a):
            check(lib().pfd_basin_bounds(self._h, int(dtype_code), ptr(labels), ptr(a[0]), ptr(a[1]), cap, C.byref(k), PFD_HOST))
            return int(k.value)
        (lbs, bounds), n = _list_call(4096 if cap is None else int(cap),
                                      lambda cap: (np.empty(cap, labels.dtype), np.empty(4 * cap, np.int64)), run)
        return lbs[:n].copy(), bounds[:4 * n].reshape(4, n).copy()

    def subbasins_pfafstetter(self, uparea, dtype_code, upa_min, depth, idxs_us_main, idxs_pit, idx_dtype, cap=None):
        """(int32 map[n], outlet cells[k]) of pfd_subbasins_pfafstetter; ``uparea`` / ``idxs_us_main`` (int64) may be None."""
        k = C.c_int64(0)
        out = np.empty(self.n, np.int32)
        idxs_pit = np.ascontiguousarray(idxs_pit, dtype=np.int64)

        def run(cap, idxs):
            check(lib().pfd_subbasins_pfafstetter(self._h, int(dtype_code), ptr(uparea), float(upa_min), int(depth),
                                                  ptr(idxs_us_main), ptr(idxs_pit), idxs_pit.size, IDX_CODE[np.dtype(idx_dtype)],
                                                  ptr(idxs), cap, C.byref(k), ptr(out), PFD_HOST))
            return int(k.value)
        idxs, n = _list_call(idxs_pit.size + max(1 << 16, 16 * idxs_pit.size) if cap is None else int(cap),
                             lambda cap: np.empty(cap, idx_dtype), run)
        return out, idxs[:n].copy()

    def subbasins_area(self, uparea, dtype_code, area_min, compare, idxs_us_main, idx_dtype, cap=None, flags=0, out=None,
                       idxs_out=None, memspace=PFD_HOST):
        """(uint32 map[n], outlet cells[k], int64 stats[4] = mode, rounds, jobs, lane steps) of pfd_subbasins_area;
        ``uparea`` / ``idxs_us_main`` (int64) may be None.  PFD_DEVICE: ``uparea``, ``idxs_us_main``, ``out`` and ``idxs_out``
        (``cap`` entries) are DeviceBuffers; returns (out, idxs_out, k, stats)."""
        k = C.c_int64(0)
        stats = np.zeros(4, np.int64)
        icode = IDX_CODE[np.dtype(idx_dtype)]

        def run(cap, idxs, space):
            check(lib().pfd_subbasins_area(self._h, int(dtype_code), ptr(uparea), float(area_min), int(compare),
                                           ptr(idxs_us_main), icode, ptr(idxs), int(cap), C.byref(k), ptr(out), ptr(stats),
                                           int(flags), space))
            return int(k.value)
        if memspace != PFD_HOST:
            return out, idxs_out, run(cap, idxs_out, memspace), stats
        out = np.empty(self.n, np.uint32)
        idxs, n = _list_call(self._outlet_cap() if cap is None else int(cap), lambda cap: np.empty(cap, idx_dtype),
                             lambda cap, idxs: run(cap, idxs, PFD_HOST))
        return out, idxs[:n].copy(), stats

    # -- upscaling (csrc/upscale.hip) ------------------------------------------------------------------------------------
    def upscale(self, method, cellsize, uparea, effarea, idx_dtype, outlets_only=False):
        """(coarse idxs_ds[n1], fine idxs_out[n1]) of pfd_upscale, or idxs_out alone (pfd_upscale_outlets); ``method`` a key
        of UPSCALE_METHOD, ``uparea`` int32 / float32 / float64, ``effarea`` the uint8 effective-area mask or None (dmm)."""
        cellsize = int(cellsize)
        n1 = -(-self.nrow // cellsize) * -(-self.ncol // cellsize)
        code, icode = _PAYLOAD_CODE[uparea.dtype], IDX_CODE[np.dtype(idx_dtype)]
        idxs_out = np.empty(n1, idx_dtype)
        if outlets_only:
            check(lib().pfd_upscale_outlets(self._h, UPSCALE_METHOD[method], cellsize, code, ptr(uparea), ptr(effarea), icode,
                                            ptr(idxs_out), PFD_HOST))
            return idxs_out
        idxs_ds = np.empty(n1, idx_dtype)
        check(lib().pfd_upscale(self._h, UPSCALE_METHOD[method], cellsize, code, ptr(uparea), ptr(effarea), icode, ptr(idxs_ds),
                                ptr(idxs_out), PFD_HOST))
        return idxs_ds, idxs_out

    def upscale_error(self, idxs_out, idxs_ds_coarse):
        """uint8[k] of pfd_upscale_error on the FINE handle: 1 connected, 0 not, 255 missing."""
        assert idxs_out.dtype == idxs_ds_coarse.dtype and idxs_out.size == idxs_ds_coarse.size
        out = np.empty(idxs_out.size, np.uint8)
        check(lib().pfd_upscale_error(self._h, IDX_CODE[idxs_out.dtype], ptr(idxs_out), ptr(idxs_ds_coarse), idxs_out.size,
                                      ptr(out), PFD_HOST))
        return out

    # -- stream segments (csrc/streams.hip) ------------------------------------------------------------------------
    def streams(self, mask, idx_dtype, idxs_out=None, offsets_out=None, pit_out=None, cap_idxs=None, cap_segs=None,
                memspace=PFD_HOST):
        """The unsplit stream segments of pfd_streams as a CSR triple: (idxs[M] of ``idx_dtype``, offsets[K + 1] int64,
        pit[K] uint8); ``mask`` uint8 or None.  PFD_HOST: a sizing call, then the fetch with room for exactly K and M.
        PFD_DEVICE: ``mask`` and the three lists (``cap_idxs`` / ``cap_segs`` entries; None with caps of 0: a sizing
        call) are DeviceBuffers; returns (K, M), the lists are written when they fit."""
        n_out = (C.c_int64 * 2)()
        code = IDX_CODE[np.dtype(idx_dtype)]
        if memspace != PFD_HOST:
            check(lib().pfd_streams(self._h, ptr(mask), code, ptr(idxs_out), int(cap_idxs or 0), ptr(offsets_out),
                                    ptr(pit_out), int(cap_segs or 0), n_out, memspace))
            return int(n_out[0]), int(n_out[1])
        # a sizing call in device memory first: the lists have no useful upper bound short of the raster's size
        dmask = None if mask is None else DeviceBuffer(mask.nbytes, self.device).upload(mask)
        try:
            check(lib().pfd_streams(self._h, ptr(dmask), code, None, 0, None, None, 0, n_out, PFD_DEVICE))
        finally:
            if dmask is not None:
                dmask.free()
        k, m = int(n_out[0]), int(n_out[1])
        idxs, offsets, pit = np.empty(m, idx_dtype), np.zeros(k + 1, np.int64), np.empty(k, np.uint8)
        if k:
            check(lib().pfd_streams(self._h, ptr(mask), code, ptr(idxs), m, ptr(offsets), ptr(pit), k, n_out, PFD_HOST))
        return idxs, offsets, pit

    def floodplains(self, elevtn, elev_code, is_stream, stream_h):
        out = np.empty(self.n, np.int8)
        check(lib().pfd_floodplains(self._h, elev_code, ptr(elevtn), ptr(is_stream), ptr(stream_h), ptr(out), PFD_HOST))
        return out

    def snap_downstream(self, idxs, mask, max_hops=-1):
        idxs = np.ascontiguousarray(idxs, dtype=np.int64).ravel()
        out, dist = np.empty(idxs.size, np.int64), np.empty(idxs.size, np.float32)
        check(lib().pfd_snap_downstream(self._h, ptr(idxs), idxs.size, ptr(mask), PFD_HOST, int(max_hops), ptr(out), ptr(dist)))
        return out, dist

    def snap(self, idxs, mask=None, idxs_us_main=None, step_lengths=None, max_length=None):
        """core.snap: downstream, or upstream along ``idxs_us_main`` (int64, negative = none); cells, or metres from
        the float64 ``step_lengths`` table; returns (idxs int64, dists float32)."""
        idxs = np.ascontiguousarray(idxs, dtype=np.int64).ravel()
        out, dist = np.empty(idxs.size, np.int64), np.empty(idxs.size, np.float32)
        up = None if idxs_us_main is None else np.ascontiguousarray(idxs_us_main, dtype=np.int64).ravel()
        tab = None if step_lengths is None else np.ascontiguousarray(step_lengths, dtype=np.float64)
        check(lib().pfd_snap(self._h, ptr(idxs), idxs.size, ptr(mask), ptr(up), ptr(tab), 0 if max_length is None else 1,
                             C.c_double(0.0 if max_length is None else float(max_length)), ptr(out), ptr(dist)))
        return out, dist

    def main_upstream(self, uparea, dtype_code, idx_dtype, upa_min=0.0, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty(self.n, idx_dtype)
        check(lib().pfd_main_upstream(self._h, dtype_code, ptr(uparea), float(upa_min), IDX_CODE[np.dtype(idx_dtype)],
                                      ptr(out), memspace))
        return out

    def upstream_sum(self, data, dtype_code, nodata_i=0, nodata_f=0.0, has_nodata=1, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty_like(data)
        check(lib().pfd_upstream_sum(self._h, dtype_code, ptr(data), int(nodata_i), float(nodata_f), int(has_nodata),
                                     ptr(out), memspace))
        return out

    def stream_order_classic(self, idxs_us_main, mask=None, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty(self.n, np.uint8)
        check(lib().pfd_stream_order_classic(self._h, IDX_CODE[np.dtype(idxs_us_main.dtype)], ptr(idxs_us_main),
                                             ptr(mask), ptr(out), memspace))
        return out

    def stream_distance(self, mask=None, step_lengths=None, out=None, memspace=PFD_HOST, per_cell=False):
        """``step_lengths`` None: int32 cell counts; else float32 with the host table [2*nrow-1, 3] (D8 rasters)
        or one value per cell (``per_cell``: general idxs_ds graphs)."""
        real = step_lengths is not None
        if memspace == PFD_HOST:
            out = np.empty(self.n, np.float32 if real else np.int32)
        if real:
            step_lengths = np.ascontiguousarray(step_lengths, dtype=np.float32)
            assert step_lengths.size == (self.n if per_cell else 3 * (2 * self.nrow - 1))
        check(lib().pfd_stream_distance(self._h, ptr(mask), int(real), ptr(step_lengths), ptr(out), memspace))
        return out


def upstream_area_cell_blocks(handles, outs=None, memspace=PFD_HOST):
    """upstream_area("cell") of a raster held as row blocks by the handles of THIS process."""
    k = len(handles)
    if memspace == PFD_HOST:
        outs = [np.empty(h.n, np.int32) for h in handles]
    hs = (C.c_void_p * k)(*[h._h for h in handles])
    ps = (C.c_void_p * k)(*[ptr(o) for o in outs])
    check(lib().pfd_upstream_area_cell_blocks(hs, k, ps, memspace))
    return outs


def upstream_area_cell_begin(handle, out=None, memspace=PFD_HOST):
    """Local phase of a multi-block pass; returns (out, record) with record = 4*ncol uint32."""
    if memspace == PFD_HOST:
        out = np.empty(handle.n, np.int32)
    rec = np.empty(4 * handle.ncol, np.uint32)
    check(lib().pfd_upstream_area_cell_begin(handle._h, ptr(out), memspace, ptr(rec)))
    return out, rec


def upstream_area_cell_finish(handle, all_records: np.ndarray, nblocks: int, block: int) -> bool:
    """Completes the pass with the records of all blocks (shape [nblocks, 4*ncol]); True if acyclic."""
    all_records = np.ascontiguousarray(all_records, dtype=np.uint32)
    assert all_records.size == nblocks * 4 * handle.ncol
    ok = C.c_int(0)
    check(lib().pfd_upstream_area_cell_finish(handle._h, ptr(all_records), nblocks, block, C.byref(ok)))
    return bool(ok.value)


def basins_begin(handle, outlets, ids, out=None, memspace=PFD_HOST):
    """Local phase of a multi-block basins query; ``outlets`` index the block's own rows.  Returns
    (out, record) with record = 6*ncol uint32."""
    outlets = np.ascontiguousarray(outlets, dtype=np.int64).ravel()
    ids = np.ascontiguousarray(ids).ravel()
    if memspace == PFD_HOST:
        out = np.empty(handle.n, ids.dtype)
    rec = np.empty(6 * handle.ncol, np.uint32)
    check(lib().pfd_basins_begin(handle._h, ptr(outlets), ptr(ids), outlets.size, ids.dtype.itemsize, ptr(out), memspace,
                                 ptr(rec)))
    handle._basins_out = out  # (the library writes it in finish: keep it alive)
    return out, rec


def basins_finish(handle, all_records: np.ndarray, nblocks: int, block: int) -> bool:
    all_records = np.ascontiguousarray(all_records, dtype=np.uint32)
    assert all_records.size == nblocks * 6 * handle.ncol
    ok = C.c_int(0)
    check(lib().pfd_basins_finish(handle._h, ptr(all_records), nblocks, block, C.byref(ok)))
    return bool(ok.value)


class Communicator:
    """RCCL communicator (one rank per GPU/process).  ``uid`` = 128 bytes from ``unique_id()`` of rank 0."""

    UID_BYTES = 128

    def __init__(self, uid: bytes, rank: int, world: int, device: int):
        self._c = C.c_void_p()
        buf = C.create_string_buffer(bytes(uid), self.UID_BYTES)
        check(lib().pfd_comm_create(buf, self.UID_BYTES, rank, world, device, C.byref(self._c)))
        self.rank, self.world, self.device = rank, world, device

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Communicator.UID_BYTES)
        check(lib().pfd_comm_unique_id(buf, Communicator.UID_BYTES))
        return buf.raw

    def info(self) -> dict:
        """World size / rank / device as RCCL reports them for this communicator."""
        n, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().pfd_comm_info(self._c, C.byref(n), C.byref(r), C.byref(d)))
        return dict(nranks=n.value, rank=r.value, device=d.value)

    def upstream_area_cell(self, handle, out=None, memspace=PFD_HOST):
        if memspace == PFD_HOST:
            out = np.empty(handle.n, np.int32)
        check(lib().pfd_upstream_area_cell_dist(handle._h, self._c, ptr(out), memspace))
        return out

    def exchange_rows(self, handle, result_buf, itemsize: int, seed_buf, c0: int = 0, c1: int = 0):
        """Neighbour exchange of the block's boundary rows, device to device (pfd_comm_exchange_rows): returns
        (sum of c0 over the ranks, sum of c1, my halo values changed, ranks whose halo values changed)."""
        a = (C.c_int64 * 4)(int(c0), int(c1), 0, 0)
        check(lib().pfd_comm_exchange_rows(self._c, handle._h, ptr(result_buf), int(itemsize), ptr(seed_buf), a))
        return int(a[0]), int(a[1]), bool(a[2]), int(a[3])

    def allgather_host(self, handle, data: bytes) -> list:
        """All-gather of equally sized host byte strings through the device and RCCL."""
        n = len(data)
        src = np.frombuffer(data, np.uint8)
        out = np.empty(n * self.world, np.uint8)
        check(lib().pfd_comm_allgather_host(self._c, handle._h, ptr(np.ascontiguousarray(src)), n, ptr(out)))
        return [out[i * n:(i + 1) * n].tobytes() for i in range(self.world)]

    def close(self):
        if self._c:
            lib().pfd_comm_destroy(self._c)
            self._c = C.c_void_p()


def count_nonfinite(buf, n: int, dtype_code: int, device: int = 0) -> int:
    """NaN / +-inf values among the first n float32 / float64 values of a device buffer."""
    out = C.c_int64(0)
    check(lib().pfd_count_nonfinite(device, int(dtype_code), ptr(buf), int(n), C.byref(out)))
    return int(out.value)


def checksum_i32(buf, n: int, device: int = 0) -> int:
    """Sum (64-bit two's complement) of n int32 values in a device buffer."""
    out = C.c_int64(0)
    check(lib().pfd_checksum_i32(device, ptr(buf), int(n), C.byref(out)))
    return int(out.value)


# -- elementwise calls on device buffers (csrc/elementwise.hip; pyflwdir_amd/device_array.py is their front end) --------
def ew_compare(a, code, rel, compare_code, scalar_i, scalar_f, out, n, device=0):
    check(lib().pfd_ew_compare(int(device), int(rel), int(code), ptr(a), int(compare_code), int(scalar_i), float(scalar_f),
                               ptr(out), int(n)))
    return out


def ew_logic(op, a, b, out, n, device=0):
    check(lib().pfd_ew_logic(int(device), int(op), ptr(a), ptr(b), ptr(out), int(n)))
    return out


def ew_where(mask, code, a, b, scalar_i, scalar_f, out, n, device=0):
    """``b`` None: the scalar takes its place."""
    check(lib().pfd_ew_where(int(device), int(code), ptr(mask), ptr(a), ptr(b), int(scalar_i), float(scalar_f), ptr(out),
                             int(n)))
    return out


def ew_convert(a, src_code, dst_code, out, n, device=0):
    check(lib().pfd_ew_convert(int(device), int(src_code), ptr(a), int(dst_code), ptr(out), int(n)))
    return out


def ew_reduce(op, a, code, n, device=0):
    """(int result, float result, a NaN was seen) of pfd_ew_reduce."""
    ri, rf, nan = C.c_int64(0), C.c_double(0.0), C.c_int(0)
    check(lib().pfd_ew_reduce(int(device), int(op), int(code), ptr(a), int(n), C.byref(ri), C.byref(rf), C.byref(nan)))
    return int(ri.value), float(rf.value), bool(nan.value)


# -- synthetic rasters generated in HBM ---------------------------------------------------------
def synth_d8_device(nrow, ncol, seed=0, tilt=1 << 26, white=2, nodata_pct=0, row0=0, nrows=None, device=0):
    nrows = nrow - row0 if nrows is None else nrows
    buf = DeviceBuffer(nrows * ncol, device)
    check(lib().pfd_synth_d8(device, seed, nrow, ncol, tilt, white, nodata_pct, row0, nrows, C.c_void_p(buf.addr)))
    return buf


def synth_mosaic_device(base: np.ndarray, nrow, ncol, device=0):
    """A host base raster tiled over nrow x ncol cells in HBM (nodata frame per copy): pfd_synth_mosaic."""
    base = np.ascontiguousarray(base, dtype=np.uint8)
    buf = DeviceBuffer(int(nrow) * int(ncol), device)
    check(lib().pfd_synth_mosaic(device, ptr(base), base.shape[0], base.shape[1], int(nrow), int(ncol), C.c_void_p(buf.addr)))
    return buf


def synth_elev_device(nrow, ncol, seed=0, tilt=1 << 26, white=2, nodata_pct=0, row0=0, nrows=None, device=0):
    nrows = nrow - row0 if nrows is None else nrows
    buf = DeviceBuffer(nrows * ncol * 4, device)
    check(lib().pfd_synth_elev_f32(device, seed, nrow, ncol, tilt, white, nodata_pct, row0, nrows, C.c_void_p(buf.addr)))
    return buf


def synth_weights_device(n, seed=1, i0=0, device=0):
    buf = DeviceBuffer(n * 4, device)
    check(lib().pfd_synth_weights_f32(device, seed, i0, n, C.c_void_p(buf.addr)))
    return buf
