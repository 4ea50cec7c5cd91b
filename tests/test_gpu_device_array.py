"""The elementwise kernels (csrc/elementwise.hip) alone, through ``DeviceArray``: every dtype and every operator, on sizes
that sit on the edges of the 16-byte vector, the wave, the workgroup and the grid, byte for byte against numpy on the host
copy."""
import operator
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4099, 2**20 + 5]
DTYPES = [np.dtype(t) for t in (np.bool_, np.uint8, np.int8, np.int32, np.uint32, np.int64, np.float32, np.float64)]
OPS = {"lt": operator.lt, "le": operator.le, "gt": operator.gt, "ge": operator.ge, "eq": operator.eq, "ne": operator.ne}


@pytest.fixture(scope="module")
def D(gpu_lib):
    from pyflwdir_amd import device_array

    return device_array


def specials(dtype):
    if dtype == np.bool_:
        return [True, False]
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return [info.min, info.max, 0, 1, info.max - 1, info.min + 1]
    info = np.finfo(dtype)
    return [np.nan, 0.0, -0.0, np.inf, -np.inf, info.max, info.min, info.tiny, 1.5, -1.5]


_PAYLOADS = {}


def payload(dtype, n):
    """n elements of ``dtype`` (computed once per pair): small random values around the scalars the tests compare with,
    and the specials — NaN, +-0.0, +-inf, the extremes — at the first and last positions and around the wave edge."""
    key = (dtype, n)
    if key not in _PAYLOADS:
        rng = np.random.default_rng(1000 + n)
        if dtype == np.bool_:
            a = rng.integers(0, 2, n).astype(np.bool_)
        elif dtype.kind in "iu":
            a = rng.integers(-4 if dtype.kind == "i" else 0, 8, n).astype(dtype)
        else:
            a = (rng.integers(-6, 7, n) / 2).astype(dtype)
        sp = specials(dtype)
        for k, pos in enumerate([0, n - 1, 62, 63, 64, 65, n // 2, 255, 256, n - 2, n - 17, 1]):
            if 0 <= pos < n:
                a[pos] = sp[k % len(sp)]
        a.setflags(write=False)
        _PAYLOADS[key] = a
    return _PAYLOADS[key]


def same_bytes(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.ravel().view(np.uint8) != want.ravel().view(np.uint8)) // got.dtype.itemsize
        raise AssertionError(f"{bad.size} bytes differ, first elements {bad[:5]}: got {got.ravel()[bad[:5]]} "
                             f"expected {want.ravel()[bad[:5]]}")


def scalars(dtype):
    if dtype == np.bool_:
        return [True, False, np.bool_(True)]
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return [1, 0, 1.5, float("nan"), np.float64(2.0), info.max, info.max + 1, info.min - 1, float("inf")]
    return [1.5, 0, -0.0, float("nan"), float("inf"), np.float64(0.1), 0.1, np.float32(1.5), 1e300, -1]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_compare_every_size(D, dtype):
    for n in SIZES:
        a = payload(dtype, n)
        d = D.to_device(a)
        for s in scalars(dtype):
            if np.result_type(dtype, s) not in (dtype, np.float64):
                continue
            for name, fn in OPS.items():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    want = fn(a, s)
                same_bytes(fn(d, s).numpy(), want)
        # the scalar on the left: numpy defers to the reflected operator
        if dtype != np.bool_:
            same_bytes((np.float64(1.0) < d).numpy(), np.float64(1.0) < a)
            same_bytes((1 >= d).numpy(), 1 >= a)


def test_compare_refuses_other_dtypes_and_arrays(D):
    d = D.to_device(np.arange(5, dtype=np.uint8))
    with pytest.raises(NotImplementedError, match="float64"):
        d < np.float32(2)  # (numpy compares in float32)
    with pytest.raises(NotImplementedError, match="float64"):
        D.to_device(np.arange(5, dtype=np.int32)) == np.int64(2)
    with pytest.raises(NotImplementedError):
        d == d
    with pytest.raises(TypeError):
        d < "3"
    with pytest.raises(ValueError, match="ambiguous"):
        bool(d > 1)


@pytest.mark.parametrize("n", SIZES)
def test_logic(D, n):
    a, b = payload(np.dtype(np.bool_), n), np.random.default_rng(n).integers(0, 2, n).astype(np.bool_)
    da, db = D.to_device(a), D.to_device(b)
    same_bytes((da & db).numpy(), a & b)
    same_bytes((da | db).numpy(), a | b)
    same_bytes((da ^ db).numpy(), a ^ b)
    same_bytes((~da).numpy(), ~a)
    same_bytes((~(da ^ db) | (da & ~db)).numpy(), ~(a ^ b) | (a & ~b))
    with pytest.raises(NotImplementedError):
        D.to_device(a.view(np.uint8)) & db
    if n > 1:
        with pytest.raises(ValueError):
            da & D.to_device(b[:-1])
    with pytest.raises(TypeError):
        da & True


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_where(D, dtype):
    for n in SIZES:
        a = payload(dtype, n)
        b = a[::-1].copy()
        m = np.random.default_rng(7 * n).integers(0, 2, n).astype(np.bool_)
        da, db, dm = D.to_device(a), D.to_device(b), D.to_device(m)
        same_bytes(D.where(dm, da, db).numpy(), np.where(m, a, b))
        for s in ([True] if dtype == np.bool_ else [-9999, 3] if dtype.kind == "i" else [200] if dtype.kind == "u" else
                  [-9999.0, float("nan"), 0.1, -0.0]):
            if dtype.kind in "iu" and not np.iinfo(dtype).min <= s <= np.iinfo(dtype).max:
                continue
            same_bytes(D.where(dm, da, s).numpy(), np.where(m, a, np.array(s).astype(dtype)))
    with pytest.raises(NotImplementedError):
        D.where(D.to_device(m.view(np.uint8)), da, db)
    with pytest.raises(ValueError):  # (b of another dtype)
        D.where(dm, da, D.to_device(np.zeros(b.shape, np.float64 if dtype != np.float64 else np.float32)))


@pytest.mark.parametrize("src", DTYPES, ids=str)
def test_astype(D, src):
    from pyflwdir_amd.device_array import astype_rule

    for dst in DTYPES:
        try:
            astype_rule(src, dst)
        except NotImplementedError:
            with pytest.raises(NotImplementedError, match="not exact"):
                D.to_device(payload(src, 17)).astype(dst)
            continue
        for n in SIZES:
            a = payload(src, n)
            same_bytes(D.to_device(a).astype(dst).numpy(), a.astype(dst))


def py_scalar_equal(got, want):
    """A reduction's Python scalar against numpy's: the same value (NaN for NaN) and a plain Python type."""
    assert type(got) in (bool, int, float), type(got)
    if isinstance(want, (float, np.floating)) and np.isnan(want):
        assert isinstance(got, float) and got != got
    else:
        assert got == want  # (zeros of both signs are equal: numpy's pick among them depends on its order)


def check_reductions(D, a):
    d = D.to_device(a)
    assert d.count_nonzero() == int(np.count_nonzero(a)) and type(d.count_nonzero()) is int
    assert d.any() is bool(a.any()) and d.all() is bool(a.all())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        py_scalar_equal(d.min(), a.min())
        py_scalar_equal(d.max(), a.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_reductions(D, dtype):
    sp = specials(dtype)
    for n in SIZES:
        check_reductions(D, payload(dtype, n))
        # all-equal arrays, and a single other value — an extreme, a NaN — at the first, the last and a wave-edge position
        for base in (sp[2 % len(sp)], sp[-1], sp[0] if dtype.kind != "f" else 0.0):
            a = np.full(n, base, dtype)
            check_reductions(D, a)
            for pos in {0, n - 1, min(63, n - 1), min(64, n - 1), n // 2}:
                for v in sp[:6]:
                    b = a.copy()
                    b[pos] = v
                    check_reductions(D, b)
            if n > 4099:
                break  # (the large size: one base value)
    if dtype.kind == "f":  # zeros of both signs: one answer whatever the order, and equal to numpy's as a number
        d = D.to_device(np.array([0.0, -0.0, 0.0], dtype))
        assert d.min() == 0 and np.signbit(d.min()) and d.max() == 0 and not np.signbit(d.max())
        only_nan = D.to_device(np.full(70, np.nan, dtype))
        assert only_nan.min() != only_nan.min() and only_nan.count_nonzero() == 70


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_empty_arrays(D, dtype):
    for shape in ((0,), (0, 5), (3, 0)):
        a = np.empty(shape, dtype)
        d = D.to_device(a)
        assert d.shape == shape and d.size == 0 and d.nbytes == 0
        assert d.count_nonzero() == 0 and d.any() is False and d.all() is True
        with pytest.raises(ValueError, match="zero-size"):
            d.min()
        with pytest.raises(ValueError, match="zero-size"):
            d.max()
        same_bytes(d.numpy(), a)
        zero = dtype.type(0)
        same_bytes((d != zero).numpy(), a != zero)
        if dtype == np.bool_:
            same_bytes((~d & d).numpy(), ~a & a)
        same_bytes(D.where(d != zero, d, d).numpy(), a)


def test_attributes_reshape_and_lifetime(D):
    a = np.arange(24, dtype=np.float32).reshape(4, 6)
    d = D.to_device(a[:, ::2])  # (any layout goes up: made contiguous)
    assert d.shape == (4, 3) and d.dtype == np.float32 and d.size == 12 and d.nbytes == 48 and d.device == 0 and d.ndim == 2
    assert len(d) == 4 and "float32" in repr(d)
    same_bytes(d.numpy(), np.ascontiguousarray(a[:, ::2]))
    out = np.empty((3, 4), np.float32)
    assert d.numpy(out=out) is out and np.array_equal(out.ravel(), a[:, ::2].ravel())
    for bad in (np.empty(12, np.float64), np.empty(11, np.float32), np.empty((4, 6), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            d.numpy(out=bad)
    assert D.to_device(d) is d
    # reshape shares the buffer; both keep it alive
    r = d.reshape(3, -1)
    assert r.shape == (3, 4) and r._buf is d._buf and d.reshape((12,)).shape == (12,) and d.ravel().shape == (12,)
    with pytest.raises(ValueError):
        d.reshape(5, 2)
    with pytest.raises(ValueError):
        d.reshape(-1, -1)
    addr = d._buf.addr
    del d
    same_bytes(r.numpy().ravel(), np.ascontiguousarray(a[:, ::2]).ravel())  # the last one alive still holds it
    assert r._buf.addr == addr
    # __array__ raises and names the way out
    for convert in (np.asarray, np.array, np.atleast_1d, np.ascontiguousarray):
        with pytest.raises(TypeError, match=r"\.numpy\(\)"):
            convert(r)
    # free(): any use afterwards raises, for every array that shares the buffer
    s = r.reshape(12)
    r.free()
    for use in (lambda: r.numpy(), lambda: s.numpy(), lambda: r > 1, lambda: s.min(), lambda: r.astype(np.float64),
                lambda: r.reshape(12), lambda: s.count_nonzero(), lambda: D.where(s > 0, s, 0.0)):
        with pytest.raises(ValueError, match="freed"):
            use()
    r.free()  # (twice is fine)
    assert "freed" in repr(r)


def test_to_device_checks_the_device_of_a_device_array(D):
    d = D.to_device(np.arange(4, dtype=np.int32))
    assert D.to_device(d, device=0) is d
    with pytest.raises(ValueError, match="GPU 0"):
        D.to_device(d, device=1)


@pytest.mark.parametrize("n", [1, 5, 63, 64, 257, 4099])
def test_unaligned_pointers_take_the_scalar_loops(D, n):
    """The C entry points with addresses that are NOT 16-byte aligned (one element into a block: what only a C caller can
    pass — every DeviceArray starts at an allocator's alignment): each kernel then runs its scalar loop over everything."""
    from pyflwdir_amd import _hip

    def off(dev, k=1):  # the address of element k
        return dev._buf.addr + k * dev.dtype.itemsize

    f = payload(np.dtype(np.float32), n + 1)
    i = payload(np.dtype(np.int32), n + 1)
    b = payload(np.dtype(np.bool_), n + 1)
    df, di, db = D.to_device(f), D.to_device(i), D.to_device(b)
    assert off(df) % 16 == 4 and off(db) % 16 == 1
    # compare: float32 own dtype and int32 in float64, the result written one byte into its block
    out = D.DeviceArray.empty(n + 1, np.bool_)
    _hip.ew_compare(off(df), _hip.PFD_F32, D.RELATIONS["ne"], _hip.PFD_F32, 0, 1.5, off(out), n)
    same_bytes(out.numpy()[1:], f[1:] != np.float32(1.5))
    _hip.ew_compare(off(di), _hip.PFD_I32, D.RELATIONS["le"], _hip.PFD_F64, 0, 1.5, off(out), n)
    same_bytes(out.numpy()[1:], i[1:] <= 1.5)
    # logic
    _hip.ew_logic(_hip.PFD_EW_XOR, off(db), db._buf.addr, off(out), n)
    same_bytes(out.numpy()[1:], b[1:] ^ b[:-1])
    _hip.ew_logic(_hip.PFD_EW_NOT, off(db), None, off(out), n)
    same_bytes(out.numpy()[1:], ~b[1:])
    # where: array and scalar second operand
    outf = D.DeviceArray.empty(n + 1, np.float32)
    _hip.ew_where(off(db), _hip.PFD_F32, off(df), df._buf.addr, 0, 0.0, off(outf), n)
    same_bytes(outf.numpy()[1:], np.where(b[1:], f[1:], f[:-1]))
    _hip.ew_where(off(db), _hip.PFD_F32, off(df), None, 0, -9999.0, off(outf), n)
    same_bytes(outf.numpy()[1:], np.where(b[1:], f[1:], np.float32(-9999.0)))
    # convert
    outd = D.DeviceArray.empty(n + 1, np.float64)
    _hip.ew_convert(off(di), _hip.PFD_I32, _hip.PFD_F64, off(outd), n)
    same_bytes(outd.numpy()[1:], i[1:].astype(np.float64))
    # reduce
    assert _hip.ew_reduce(_hip.PFD_EW_COUNT, off(di), _hip.PFD_I32, n)[0] == int(np.count_nonzero(i[1:]))
    assert _hip.ew_reduce(_hip.PFD_EW_MAX, off(di), _hip.PFD_I32, n)[0] == int(i[1:].max())
    ri, rf, nan = _hip.ew_reduce(_hip.PFD_EW_MIN, off(df), _hip.PFD_F32, n)
    assert nan == bool(np.isnan(f[1:]).any()) and (nan or rf == float(f[1:].min()))


def test_unsupported_dtypes(D):
    for dt in (np.float16, np.int16, np.uint16, np.uint64, np.complex64):
        with pytest.raises(NotImplementedError, match="not supported"):
            D.to_device(np.zeros(4, dt))
    with pytest.raises(NotImplementedError, match="not supported"):
        D.to_device(np.array(["a"]))
    with pytest.raises(NotImplementedError, match="not supported"):
        D.DeviceArray.empty((2, 2), np.int16)


def test_public_names(D):
    import pyflwdir_amd

    assert pyflwdir_amd.DeviceArray is D.DeviceArray and pyflwdir_amd.to_device is D.to_device
