"""``DeviceArray``: a per-cell array that stays in the HBM of one GPU between two calls.

    upa = flw.upstream_area(resident=True)            # DeviceArray, nothing per-cell crosses PCIe
    sto = flw.stream_order(mask=upa > 100, resident=True)
    hand = flw.hand(sto >= 3, elevtn_dev, resident=True).numpy()

It owns one ``_hip.DeviceBuffer``, is C-contiguous, has no views and no strides, and offers exactly the small expressions
the front end computes with numpy between two sweeps — comparisons with a scalar, logic on masks, ``where``, the
conversions that are exact for every value, and the reductions no execution order can change — each as a HIP kernel
(csrc/elementwise.hip) that returns a new ``DeviceArray``.  No arithmetic and no float sums: a float sum has an order, and
this library does not return sums whose order it cannot state.  ``.numpy()`` is the only way out; ``np.asarray`` raises.

Ordering (include/pfd.h, "memory spaces"): every call of the library returns only after its result is complete in HBM, so
an array returned by a sweep can go into an elementwise call at once, and the other way round.
"""
from __future__ import annotations

import numpy as np

from . import _hip

__all__ = ["DeviceArray", "to_device", "where", "compare_rule", "astype_rule"]

_BOOL = np.dtype(np.bool_)
_F64 = np.dtype(np.float64)
# supported dtypes -> element code of the elementwise calls (bool travels as bytes 0 / 1)
_CODES = {_BOOL: _hip.PFD_U8, np.dtype(np.uint8): _hip.PFD_U8, np.dtype(np.int8): _hip.PFD_I8,
          np.dtype(np.int32): _hip.PFD_I32, np.dtype(np.uint32): _hip.PFD_U32, np.dtype(np.int64): _hip.PFD_I64,
          np.dtype(np.float32): _hip.PFD_F32, _F64: _hip.PFD_F64}
DTYPES = tuple(_CODES)
# new arrays take their buffer from the library's caching allocator (pfd_malloc_pooled); False: a hipMalloc of their own
# (pfd_malloc) — kept switchable so that tools/probe_resident_chain.py --hipmalloc can show what that costs
POOLED = True

_LT, _EQ, _GT, _UN = _hip.PFD_EW_LT, _hip.PFD_EW_EQ, _hip.PFD_EW_GT, _hip.PFD_EW_UNORDERED
# operator name -> the outcomes of "element ? scalar" it accepts (a NaN on either side is "unordered")
RELATIONS = {"lt": _LT, "le": _LT | _EQ, "gt": _GT, "ge": _GT | _EQ, "eq": _EQ, "ne": _LT | _GT | _UN}


def _check_dtype(dtype, what):
    dtype = np.dtype(dtype)
    if dtype not in _CODES:
        raise NotImplementedError(f"{what}: dtype {dtype} is not supported on the device (supported: "
                                  f"{', '.join(str(d) for d in DTYPES)}); convert on the host first")
    return dtype


def compare_rule(dtype, scalar, op):
    """How ``array of dtype <op> scalar`` is evaluated so that it equals numpy's answer: ``(compare dtype, scalar cast to
    it, op)`` with ``op`` one of "lt", "le", "gt", "ge", "eq", "ne".  The compare dtype is ``np.result_type(dtype,
    scalar)`` — the array's own dtype, or float64 (every element is then converted to float64 first, as numpy does); any
    other outcome raises NotImplementedError.  A Python int outside the range of an integer dtype, which numpy compares by
    value, becomes the comparison with the dtype's smallest value that has the same answer for every element.  Pure host
    code: no device is touched."""
    dtype = _check_dtype(dtype, "compare")
    if op not in RELATIONS:
        raise ValueError(f"unknown comparison {op!r}")
    if isinstance(scalar, np.ndarray) and scalar.ndim == 0:
        scalar = scalar[()]
    if not isinstance(scalar, (bool, int, float, np.bool_, np.integer, np.floating)):
        raise TypeError(f"a DeviceArray is compared with a real scalar, not with {type(scalar).__name__}")
    common = np.result_type(dtype, scalar)
    if common != dtype and common != _F64:
        raise NotImplementedError(f"comparing a {dtype} array with a {type(scalar).__name__} scalar takes place in {common}: "
                                  f"only the array's own dtype and float64 are compared on the device; pass the scalar as "
                                  f"a Python number or as numpy.float64")
    if common.kind in "iu" and isinstance(scalar, int) and not isinstance(scalar, bool):
        info = np.iinfo(common)
        if scalar < info.min or scalar > info.max:
            # numpy compares such a Python int by value: every element lies on one side of it
            truth = RELATIONS[op] & (_LT if scalar > info.max else _GT)
            return common, common.type(info.min), "ge" if truth else "lt"
    with np.errstate(over="ignore"):  # (a Python float beyond float32 compares as inf, as in numpy)
        cast = common.type(scalar)
    return common, cast, op


# astype: the conversions that are exact for every value
_ONE_BYTE = (_BOOL, np.dtype(np.uint8), np.dtype(np.int8))
_WIDEN = {(np.dtype(np.uint8), np.dtype(np.int32)), (np.dtype(np.int8), np.dtype(np.int32)), (_BOOL, np.dtype(np.int32)),
          (np.dtype(np.int32), np.dtype(np.int64)), (np.dtype(np.int32), _F64), (np.dtype(np.uint32), np.dtype(np.int64)),
          (np.dtype(np.uint32), _F64), (np.dtype(np.float32), _F64)}


def astype_rule(src, dst):
    """How ``astype`` converts ``src`` to ``dst``: "same" (the identity), "bytes" (one-byte types among each other: the
    bytes are kept — int8 <-> uint8 wrap as numpy's cast does, bool reads as 0 / 1), "nonzero" (uint8 / int8 -> bool:
    ``!= 0``, numpy's cast), "widen" (a conversion kernel).  Any other pair raises NotImplementedError: it is not exact
    for every value."""
    src, dst = _check_dtype(src, "astype"), _check_dtype(dst, "astype")
    if src == dst:
        return "same"
    if src in _ONE_BYTE and dst in _ONE_BYTE:
        return "nonzero" if dst == _BOOL else "bytes"
    if (src, dst) in _WIDEN:
        return "widen"
    raise NotImplementedError(f"astype: {src} -> {dst} is not exact for every value; supported are one-byte types among "
                              "each other, bool / uint8 / int8 -> int32, int32 / uint32 -> int64 / float64 and float32 -> "
                              "float64 — download with .numpy() for anything else")


def _scalar_pair(dtype, value):
    """(scalar_i, scalar_f) of a numpy scalar of ``dtype`` for the C calls."""
    if dtype.kind == "f":
        return 0, float(value)
    return int(value), 0.0


class DeviceArray:
    """A C-contiguous array in the HBM of one GPU (see the module docstring)."""

    __array_ufunc__ = None  # numpy defers to the reflected operators below instead of converting
    __hash__ = None

    def __init__(self, buf, shape, dtype):
        """Wraps a ``_hip.DeviceBuffer`` that holds ``prod(shape)`` elements of ``dtype`` (use ``to_device`` / ``empty``)."""
        self._buf = buf
        self.shape = tuple(int(s) for s in shape)
        self.dtype = _check_dtype(dtype, "DeviceArray")
        assert buf.nbytes >= self.nbytes

    @classmethod
    def empty(cls, shape, dtype, device=0):
        """An uninitialised array (the ``out`` of a sweep or of an elementwise call)."""
        dtype = _check_dtype(dtype, "DeviceArray")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        if any(s < 0 for s in shape):
            raise ValueError("negative dimensions are not allowed")
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        # (from the library's caching allocator: a chain of calls makes and drops multi-GiB arrays without a hipMalloc)
        return cls(_hip.DeviceBuffer(n * dtype.itemsize, device, pooled=POOLED), shape, dtype)

    # -- attributes ------------------------------------------------------------------------------------------------
    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def device(self):
        return self._buf.device

    def __len__(self):
        if not self.shape:
            raise TypeError("len() of unsized object")
        return self.shape[0]

    def __repr__(self):
        state = "freed" if self._buf.addr is None else f"device={self.device}"
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype}, {state})"

    def __bool__(self):
        raise ValueError("the truth value of a DeviceArray is ambiguous; use .any() or .all()")

    # -- lifetime and the way out ----------------------------------------------------------------------------------
    def _live(self):
        """The buffer, or ValueError after ``free()``."""
        if self._buf.addr is None:
            raise ValueError("this DeviceArray was freed")
        return self._buf

    def free(self):
        """Release the HBM now (also for every array that shares the buffer); any later use raises ValueError."""
        self._buf.free()

    def numpy(self, out=None):
        """Download into a new numpy array, or into ``out`` (C-contiguous, same dtype and size)."""
        buf = self._live()
        if out is None:
            out = np.empty(self.shape, self.dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == self.dtype and out.size == self.size and out.flags.c_contiguous):
            raise ValueError(f"out must be a C-contiguous {self.dtype} array of {self.size} elements")
        if self.size:
            buf.download(self.dtype, out.shape, out=out)
        return out

    def __array__(self, *args, **kwargs):
        raise TypeError("a DeviceArray lives in GPU memory and is not converted implicitly: download it with .numpy(), or "
                        "pass it to a method that takes device arrays")

    def reshape(self, *shape):
        """The same buffer under another shape of the same size (one -1 allowed); both arrays keep it alive."""
        self._live()
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        shape = [int(s) for s in shape]
        if shape.count(-1) > 1 or any(s < -1 for s in shape):
            raise ValueError("can only specify one unknown dimension")
        if -1 in shape:
            known = int(np.prod([s for s in shape if s != -1], dtype=np.int64))
            if known == 0 or self.size % known:
                raise ValueError(f"cannot reshape array of size {self.size} into shape {tuple(shape)}")
            shape[shape.index(-1)] = self.size // known
        if int(np.prod(shape, dtype=np.int64)) != self.size:
            raise ValueError(f"cannot reshape array of size {self.size} into shape {tuple(shape)}")
        return DeviceArray(self._buf, shape, self.dtype)

    def ravel(self):
        return self.reshape(self.size)

    def _new(self, dtype, shape=None):
        return DeviceArray.empty(self.shape if shape is None else shape, dtype, self.device)

    # -- comparisons with a scalar ---------------------------------------------------------------------------------
    def _compare(self, scalar, op):
        if isinstance(scalar, DeviceArray):
            raise NotImplementedError("a DeviceArray is compared with a scalar; two arrays are not compared on the device")
        try:
            common, cast, op = compare_rule(self.dtype, scalar, op)
        except TypeError:
            return NotImplemented
        buf = self._live()
        out = self._new(_BOOL)
        si, sf = _scalar_pair(common, cast)
        _hip.ew_compare(buf, _CODES[self.dtype], RELATIONS[op], _CODES[common], si, sf, out._buf, self.size, self.device)
        return out

    def __lt__(self, s):
        return self._compare(s, "lt")

    def __le__(self, s):
        return self._compare(s, "le")

    def __gt__(self, s):
        return self._compare(s, "gt")

    def __ge__(self, s):
        return self._compare(s, "ge")

    def __eq__(self, s):
        return self._compare(s, "eq")

    def __ne__(self, s):
        return self._compare(s, "ne")

    # -- logic on bool arrays --------------------------------------------------------------------------------------
    def _logic(self, other, op):
        if not isinstance(other, DeviceArray):
            return NotImplemented
        if self.dtype != _BOOL or other.dtype != _BOOL:
            raise NotImplementedError("&, |, ^ and ~ are offered for bool DeviceArrays (compare first)")
        if other.size != self.size:
            raise ValueError(f"operands of {self.size} and {other.size} elements")
        if other.device != self.device:
            raise ValueError("operands live on different devices")
        a, b = self._live(), other._live()
        out = self._new(_BOOL)
        _hip.ew_logic(op, a, b, out._buf, self.size, self.device)
        return out

    def __and__(self, o):
        return self._logic(o, _hip.PFD_EW_AND)

    def __or__(self, o):
        return self._logic(o, _hip.PFD_EW_OR)

    def __xor__(self, o):
        return self._logic(o, _hip.PFD_EW_XOR)

    __rand__, __ror__, __rxor__ = __and__, __or__, __xor__

    def __invert__(self):
        if self.dtype != _BOOL:
            raise NotImplementedError("~ is offered for bool DeviceArrays (compare first)")
        a = self._live()
        out = self._new(_BOOL)
        _hip.ew_logic(_hip.PFD_EW_NOT, a, None, out._buf, self.size, self.device)
        return out

    # -- conversion ------------------------------------------------------------------------------------------------
    def astype(self, dtype):
        """The conversions that are exact for every value (``astype_rule``); a new DeviceArray — which shares the buffer
        where no byte changes (arrays are never written after they are made)."""
        dtype = np.dtype(dtype)
        how = astype_rule(self.dtype, dtype)
        buf = self._live()
        if how in ("same", "bytes"):
            return DeviceArray(buf, self.shape, dtype)
        if how == "nonzero":
            return self != 0
        out = self._new(dtype)
        _hip.ew_convert(buf, _CODES[self.dtype], _CODES[dtype], out._buf, self.size, self.device)
        return out

    # -- reductions that no execution order can change -------------------------------------------------------------
    def count_nonzero(self):
        return _hip.ew_reduce(_hip.PFD_EW_COUNT, self._live(), _CODES[self.dtype], self.size, self.device)[0]

    def any(self):
        return self.count_nonzero() > 0

    def all(self):
        return self.count_nonzero() == self.size

    def _extreme(self, op, name):
        buf = self._live()
        if self.size == 0:
            raise ValueError(f"zero-size array to reduction operation {name} which has no identity")
        ri, rf, nan = _hip.ew_reduce(op, buf, _CODES[self.dtype], self.size, self.device)
        if self.dtype.kind == "f":
            return float("nan") if nan else rf
        return bool(ri) if self.dtype == _BOOL else ri

    def min(self):
        """The smallest element as a Python scalar; NaN when any element is NaN, like ``np.min``."""
        return self._extreme(_hip.PFD_EW_MIN, "minimum")

    def max(self):
        """The largest element as a Python scalar; NaN when any element is NaN, like ``np.max``."""
        return self._extreme(_hip.PFD_EW_MAX, "maximum")


def to_device(arr, device=0):
    """Upload a numpy array (any layout: it is made C-contiguous) as a ``DeviceArray`` on GPU ``device``.  A ``DeviceArray``
    that already lives there is returned as it is; one on another GPU raises ``ValueError``."""
    if isinstance(arr, DeviceArray):
        if arr.device != int(device):
            raise ValueError(f"the DeviceArray lives on GPU {arr.device}, not on GPU {device}; download it with .numpy() and "
                             "upload it there")
        return arr
    arr = np.asarray(arr)
    _check_dtype(arr.dtype, "to_device")
    arr = np.ascontiguousarray(arr)
    out = DeviceArray.empty(arr.shape, arr.dtype, device)
    if arr.size:
        out._buf.upload(arr)
    return out


def where(mask, a, b):
    """``mask ? a : b`` element by element: ``mask`` a bool DeviceArray, ``a`` a DeviceArray, ``b`` a DeviceArray of the same
    dtype and size or a scalar, which is cast to ``a.dtype``.  A new DeviceArray of ``a``'s dtype and shape."""
    if not isinstance(mask, DeviceArray) or not isinstance(a, DeviceArray):
        raise TypeError("where: mask and a are DeviceArrays")
    if mask.dtype != _BOOL:
        raise NotImplementedError("where: mask is a bool DeviceArray (compare first)")
    if mask.size != a.size:
        raise ValueError(f"where: mask of {mask.size} and a of {a.size} elements")
    si, sf, bbuf = 0, 0.0, None
    if isinstance(b, DeviceArray):
        if b.dtype != a.dtype or b.size != a.size:
            raise ValueError(f"where: b ({b.dtype}, {b.size} elements) must have the dtype and size of a ({a.dtype}, {a.size})")
        bbuf = b._live()
        devices = {mask.device, a.device, b.device}
    else:
        if not isinstance(b, (bool, int, float, np.bool_, np.integer, np.floating)):
            raise TypeError(f"where: b is a DeviceArray or a real scalar, not {type(b).__name__}")
        si, sf = _scalar_pair(a.dtype, np.array(b).astype(a.dtype)[()])
        devices = {mask.device, a.device}
    if len(devices) != 1:
        raise ValueError("where: operands live on different devices")
    mbuf, abuf = mask._live(), a._live()
    out = a._new(a.dtype)
    _hip.ew_where(mbuf, _CODES[a.dtype], abuf, bbuf, si, sf, out._buf, a.size, a.device)
    return out
