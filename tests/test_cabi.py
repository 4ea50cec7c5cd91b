"""The C-ABI library loads and exports every symbol include/pfd.h declares (no compute calls:
this runs without a GPU)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "pfd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pfd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    from pyflwdir_amd import _hip

    lib = _hip.lib()
    names = _declared()
    assert len(names) >= 25
    for name in names:
        assert hasattr(lib, name), f"libpfd_hip.so does not export {name}"
    # the binding's list is the header's list
    assert sorted(_hip.SYMBOLS) == names


_C_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
              "double": C.c_double}
_C_RETURNS = {"int": C.c_int, "const char *": C.c_char_p}
_PROTOTYPE = re.compile(r"\b(int|const char \*)\s*(pfd_\w+)\s*\(([^)]*)\)\s*;")
_PARAMETER = re.compile(r"(?:const\s+)?(\w+)\s*(\*{0,2})\s*\w+\s*(\[\d*\])?")


def _tname(t):
    return f"POINTER({t._type_.__name__})" if issubclass(t, C._Pointer) else t.__name__


def _parameter_complaint(decl, bound):
    """What is wrong with binding the C parameter ``decl`` to the ctypes type ``bound`` ("" when nothing is)."""
    m = _PARAMETER.fullmatch(decl)
    if not m:
        return f"cannot parse parameter '{decl}'"
    base, stars, array = m.groups()
    if not stars and not array:
        want = _C_SCALARS.get(base)
        if want is None:
            return f"'{decl}' has a scalar type the check does not know"
        return "" if bound is want else f"'{decl}' is bound to {_tname(bound)}, not {_tname(want)}"
    if bound is C.c_void_p:
        return ""
    if bound is C.c_char_p:
        return "" if base == "char" and stars == "*" else f"'{decl}' is bound to c_char_p"
    if not issubclass(bound, C._Pointer):
        return f"pointer '{decl}' is bound to {_tname(bound)}"
    want = C.c_void_p if stars == "**" else _C_SCALARS.get(base)  # (a handle out-parameter points at a void *)
    return "" if bound._type_ is want else f"'{decl}' is bound to {_tname(bound)}" + (f", not POINTER({want.__name__})" if want else "")


def _prototypes(header):
    """(return type, name, [parameter declarations]) of every prototype of the header text."""
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for ret, name, params in _PROTOTYPE.findall(src):
        decls = [" ".join(p.split()) for p in params.split(",")]
        yield ret, name, [] if decls in (["void"], [""]) else decls


def header_complaints(header, table):
    """Everything in which ``table`` ({name: (return type, [argument types])}) disagrees with the prototypes of the
    header text: a list with one line per complaint, each starting with the function's name."""
    out, seen = [], set()
    for ret, name, decls in _prototypes(header):
        seen.add(name)
        if name not in table:
            out.append(f"{name}: declared in the header, missing from the table")
            continue
        restype, argtypes = table[name]
        if restype is not _C_RETURNS[ret]:
            out.append(f"{name}: returns '{ret}', bound to {_tname(restype)}")
        if len(decls) != len(argtypes):
            out.append(f"{name}: {len(decls)} parameters in the header, {len(argtypes)} in the table")
            continue
        for k, (decl, bound) in enumerate(zip(decls, argtypes)):
            why = _parameter_complaint(decl, bound)
            if why:
                out.append(f"{name}: parameter {k} {why}")
    out += [f"{name}: in the table, not declared in the header" for name in table if name not in seen]
    return out


def _header():
    return open(os.path.join(ROOT, "include", "pfd.h")).read()


def test_signature_table_matches_header():
    from pyflwdir_amd import _hip

    assert header_complaints(_header(), _hip.SIGNATURES) == []
    parsed = [name for _, name, _ in _prototypes(_header())]
    # no prototype escapes the parser, and the table, SYMBOLS and the loaded library are that same list
    assert sorted(parsed) == _declared() == sorted(_hip.SIGNATURES) and _hip.SYMBOLS == list(_hip.SIGNATURES)
    lib = _hip.lib()
    for name, (restype, argtypes) in _hip.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name


def _doctored(table, name, edit):
    restype, argtypes = table[name]
    return {**table, name: (restype, edit(list(argtypes)))}


def _swap(old, new):
    def edit(argtypes):
        k = argtypes.index(old)
        return argtypes[:k] + [new] + argtypes[k + 1:]
    return edit


@pytest.mark.parametrize("case, name, edit", [
    ("c_int64 -> c_int", "pfd_set_idxs_seq", _swap(C.c_int64, C.c_int)),
    ("parameter dropped", "pfd_path", lambda argtypes: argtypes[:-1]),
    ("POINTER(c_int64) -> POINTER(c_int)", "pfd_outflow_idxs", _swap(C.POINTER(C.c_int64), C.POINTER(C.c_int))),
    ("function removed", "pfd_synth_mosaic", None),
])
def test_header_check_can_fail(case, name, edit):
    """The comparison complains, naming the function, about a table doctored in one place — and about nothing else."""
    from pyflwdir_amd import _hip

    table = dict(_hip.SIGNATURES)
    if edit is None:
        del table[name]
    else:
        table = _doctored(table, name, edit)
        assert table[name] != _hip.SIGNATURES[name]
    complaints = header_complaints(_header(), table)
    print(case, "->", complaints)
    assert len(complaints) == 1 and complaints[0].startswith(name + ":"), complaints


def test_header_check_rejects_unknown_scalar_and_extra_row():
    from pyflwdir_amd import _hip

    text = "int pfd_x(float v, int64_t n[2], pfd_raster **out); // int pfd_gone(void);\n"
    table = {"pfd_x": (C.c_int, [C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]), "pfd_y": _hip.SIGNATURES["pfd_trim"]}
    complaints = header_complaints(text, table)
    assert [name for _, name, _ in _prototypes(text)] == ["pfd_x"] and len(complaints) == 2
    assert complaints[0].startswith("pfd_x: parameter 0") and "does not know" in complaints[0]
    assert complaints[1].startswith("pfd_y:")


_CODES = ["PFD_HOST", "PFD_DEVICE", "PFD_I32", "PFD_U32", "PFD_I64", "PFD_F32", "PFD_F64", "PFD_U64", "PFD_I8", "PFD_U8",
          "PFD_I16", "PFD_U16", "PFD_UP", "PFD_DOWN", "PFD_BOTH", "PFD_FILL_MAX", "PFD_FILL_MIN", "PFD_FILL_SUM",
          "PFD_COMPARE_OWN", "PFD_COMPARE_F64", "PFD_SUBAREA_FULL"]


def test_constants_match_header():
    from pyflwdir_amd import _hip

    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"#define\s+(PFD_\w+)\s+\(?(-?\d+)\)?\s*$", header, flags=re.M)}
    assert defines["PFD_ABI_VERSION"] == 1 == _hip.lib().pfd_abi_version()
    for name in _CODES:
        assert name in defines and hasattr(_hip, name), name
    for name, value in defines.items():
        if hasattr(_hip, name):
            assert getattr(_hip, name) == value, name
    upscale = {n[len("PFD_UPSCALE_"):].lower(): v for n, v in defines.items() if n.startswith("PFD_UPSCALE_")}
    assert upscale == _hip.UPSCALE_METHOD and len(upscale) == 3
    statuses = {n: v for n, v in defines.items() if re.match(r"PFD_E[A-Z]+$", n)}
    assert len(statuses) == 8 and all(v < 0 and v in _hip._ERRORS for v in statuses.values()), statuses
    assert set(_hip._ERRORS) == set(statuses.values())


class _FakeListCall:
    """A C list call that holds ``count`` entries: writes them when they fit, reports the count either way."""

    def __init__(self, count):
        self.count, self.caps, self.allocs = count, [], []

    def alloc(self, cap):
        self.allocs.append(cap)
        return [None] * cap

    def call(self, cap, out):
        assert len(out) == cap
        self.caps.append(cap)
        if self.count <= cap:
            out[:self.count] = range(self.count)
        return self.count


@pytest.mark.parametrize("count, cap, caps", [(3, 8, [8]), (9, 8, [8, 9]), (0, 8, [8]), (8, 8, [8]), (5, 1, [1, 5]),
                                              (0, 0, [0]), (1, 0, [0, 1])])
def test_list_call_protocol(count, cap, caps):
    """One C call when the list fits the first capacity, else exactly one more with room for exactly the count."""
    from pyflwdir_amd import _hip

    fake = _FakeListCall(count)
    out, k = _hip._list_call(cap, fake.alloc, fake.call)
    assert fake.caps == caps == fake.allocs and k == count
    assert len(out) == caps[-1] and out[:k] == list(range(count))


def test_list_call_refuses_a_count_that_grows():
    from pyflwdir_amd import _hip

    counts = iter([5, 6])
    with pytest.raises(RuntimeError):
        _hip._list_call(2, lambda cap: None, lambda cap, out: next(counts))


def test_abi_version_and_error_string():
    from pyflwdir_amd import _hip

    lib = _hip.lib()
    assert lib.pfd_abi_version() == 1
    assert isinstance(lib.pfd_last_error(), bytes)


def test_no_silent_fallback_without_device():
    """On a box without a GPU the product path must raise, never fall back to a CPU path."""
    import numpy as np

    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    if _hip.device_count() > 0:
        pytest.skip("a device is visible")
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        pyflwdir.from_array(np.array([[1, 4], [0, 0]], dtype=np.uint8), ftype="d8")


def test_product_does_not_import_oracle():
    """Nothing under pyflwdir_amd/ may import or load the oracle."""
    pkg = os.path.join(ROOT, "pyflwdir_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "liboracle" not in txt and "import oracle" not in txt and "from oracle" not in txt, f
