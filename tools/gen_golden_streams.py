"""Record tests/golden/wide_streams.npz from the reference's streams.streams (pyflwdir/streams.py:132-188) and its
FlwdirRaster.streams / vectorize (pyflwdir/pyflwdir.py:865-974, gis_utils.py:490-549), imported as
tools/gen_golden_outlets.py does (the oracle's shim, no numba JIT).  The cases are tests/stream_cases.py; per case the
segment count, the lengths and the concatenated indices — in full for the small rasters, as digests
(tests/golden_util.digest) for the others.

    python tools/gen_golden_streams.py /path/to/the/reference
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PYFLWDIR_REFERENCE", "")
sys.path[:] = [q for q in sys.path if os.path.abspath(q or ".") != HERE]
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["NUMBA_DISABLE_JIT"] = "1"

import pyflwdir  # noqa: E402  (the reference)
from pyflwdir import streams as ref_streams  # noqa: E402

import stream_cases as SC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def digest(a):  # (tests/golden_util.digest)
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(str(a.dtype.str).encode())
    h.update(str(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def rasters():
    for name in SC.RASTERS:
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        yield name, pyflwdir.from_array(d8, ftype="d8", check_ftype=False, cache=False)
    W = np.load(os.path.join(GOLD, "wide_general.npz"))
    nxy = W["in_flwdir0_nextxy"]
    yield "flwdir0_nextxy", pyflwdir.from_array(nxy, ftype="nextxy", cache=False)
    yield "flwdir0_ds2", pyflwdir.FlwdirRaster(idxs_ds=W["in_flwdir0_ds2"], shape=nxy.shape[1:], ftype="d8", cache=False)


def main():
    store = {}
    for name, flw in rasters():
        ds, seq = flw.idxs_ds, flw.idxs_seq
        strahler = flw.stream_order().ravel()
        for k, mkind, max_len in SC.cases(name):
            mask = SC.mask_of(mkind, strahler, flw.shape)
            segs = ref_streams.streams(ds, seq, mask=mask, max_len=max_len, mv=flw._mv)
            assert all(s.dtype == ds.dtype for s in segs), k
            lens, flat = SC.flatten(segs, ds.dtype)
            # the restatement the tests run elsewhere agrees with the reference here
            mine = SC._ref_streams(ds, seq, mask, max_len)
            assert len(mine) == len(segs) and all(a == b.tolist() for a, b in zip(mine, segs)), k
            store[f"count_{k}"] = np.array(len(segs), np.int64)
            if name in SC.FULL:
                store[f"lens_{k}"], store[f"idxs_{k}"] = lens, flat
            else:
                store[f"digest_lens_{k}"], store[f"digest_idxs_{k}"] = np.array(digest(lens)), np.array(digest(flat))
        print(name, "done", flush=True)
    for name in SC.FEATURE_RASTERS:
        d8 = np.load(os.path.join(GOLD, name + ".npz"))["d8"]
        flw = pyflwdir.from_array(d8, ftype="d8", transform=SC.TRANSFORM, cache=False)
        strord, uparea = flw.stream_order(), flw.upstream_area()
        feats = dict(streams_sto2=flw.streams(min_sto=2, strord=strord, uparea=uparea), vectorize=flw.vectorize(),
                     vectorize_up=flw.vectorize(mask=strord >= 2, direction="up", strord=strord))
        for tag, columns in SC.feature_calls():
            assert all(sorted(f) == ["geometry", "properties", "type"] and f["type"] == "Feature"
                       and f["geometry"]["type"] == "LineString" for f in feats[tag]), tag
            for col, arr in SC.feature_record(feats[tag], columns).items():
                store[f"feat_{name}_{tag}_{col}"] = arr
    fn = os.path.join(GOLD, "wide_streams.npz")
    np.savez_compressed(fn, **store)
    print(fn, len(store), "arrays", os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) < 1 << 20


if __name__ == "__main__":
    main()
