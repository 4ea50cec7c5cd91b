"""The memory phases of the final tile pass (k_tile_final_fast) and of the supertile solves (super_solve) issue their
loads in batches: candidates of a perimeter slot worked out in registers, a nodata mask instead of live codes, one
16-byte store per quad chosen by the host, list entries / boundary pulls loaded ahead of their use and unpredicated.
Every result here must be the oracle's, bit for bit; the rasters are chosen for the paths those changes touch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_DR = (0, 1, 1, 1, 0, -1, -1, -1)  # E, SE, S, SW, W, NW, N, NE  (code 1 << k)
_DC = (1, 1, 0, -1, -1, -1, 0, 1)
_REF = {}


def _ref(oracle, key, make):
    """raster + oracle answer, computed once per key and shared (never modified)."""
    if key not in _REF:
        d8 = make()
        d8.setflags(write=False)
        exp = oracle.upstream_area_cell(d8)[0]
        exp.setflags(write=False)
        _REF[key] = (d8, exp)
    return _REF[key]


def _both_handles(d8, exp):
    from pyflwdir_amd import _hip

    for deferred in (False, True):
        h = _hip.RasterHandle(d8, d8.shape[0], d8.shape[1], deferred=deferred)
        got = h.upstream_area_cell().reshape(d8.shape)
        h.close()
        assert np.array_equal(got, exp), f"deferred={deferred}"


def exit_counts(d8):
    """Exits per supertile (512 x 512 cells), derived from the codes: a cell whose step leaves its 64 x 64 tile and lands
    on a cell of the raster that is not nodata."""
    nrow, ncol = d8.shape
    r, c = np.mgrid[0:nrow, 0:ncol]
    ex = np.zeros(d8.shape, bool)
    for k in range(8):
        rr, cc = r + _DR[k], c + _DC[k]
        inside = (rr >= 0) & (rr < nrow) & (cc >= 0) & (cc < ncol)
        ok = np.zeros(d8.shape, bool)
        ok[inside] = d8[rr[inside], cc[inside]] != 247
        ex |= (d8 == (1 << k)) & ok & (((rr >> 6) != (r >> 6)) | ((cc >> 6) != (c >> 6)))
    cnt = np.zeros(((nrow + 511) // 512, (ncol + 511) // 512), np.int64)
    np.add.at(cnt, (r[ex] >> 9, c[ex] >> 9), 1)
    return cnt


# ---- final pass, prologue: the candidates of a perimeter slot ---------------------------------------------------------
def _mixed_directions():
    """the eight directions in 64 x 64 blocks offset by 32 cells against the tiles: every tile edge is crossed inside a
    block and along a block boundary.  (The assignment of directions to blocks is one that leaves no cycle.)"""
    perm = (0, 1, 2, 3, 6, 5, 4, 7)
    d8 = np.empty((256, 256), np.uint8)
    for r in range(256):
        br = (r + 32) // 64
        for bc in range(5):
            d8[r, max(0, bc * 64 - 32):min(256, bc * 64 + 32)] = 1 << perm[(br * 3 + bc * 5) % 8]
    return d8


@pytest.mark.parametrize("k", list(range(8)) + ["mixed"])
def test_final_prologue_candidates(gpu_lib, oracle, k):
    """256 x 256 = 4 x 4 tiles, the inner 2 x 2 take the interior kernels.  One direction everywhere: every entry cell of
    a tile is fed through exactly the candidate opposite to k (an edge slot's 3 and a corner slot's 5 are all met over
    the eight rasters); the mixed raster feeds several candidates of one slot at once."""
    if k == "mixed":
        d8, exp = _ref(oracle, "mixed", _mixed_directions)
        assert not (oracle.rank(oracle.from_array(d8)[0])[0] == -1).any()  # no cycle: the tiled engine's result counts
    else:
        d8, exp = _ref(oracle, ("dir", k), lambda: np.full((256, 256), 1 << k, np.uint8))
    _both_handles(d8, exp)


# ---- final pass, epilogue: nodata mask, aligned / unaligned stores, WEIGHTS -------------------------------------------
def _synth_both_pits(oracle, shape, **kw):
    d8 = oracle.synth_d8(shape[0], shape[1], **kw)
    d8[d8 == 0] = np.where(np.arange((d8 == 0).sum()) % 2 == 0, 0, 255).astype(np.uint8)  # both pit codes
    return d8


@pytest.mark.parametrize("nodata_pct", [0, 30])
@pytest.mark.parametrize("tilt", [1 << 26, 100000, 3000])
@pytest.mark.parametrize("shape", [(320, 320), (320, 323), (321, 322)])
def test_final_epilogue(gpu_lib, oracle, shape, tilt, nodata_pct):
    """5 x 5 (6 x 6) tiles.  320 columns: rows of 16-byte aligned quads (the ALIGNED instantiation); 323 / 322: the
    four-dword one.  30 % nodata: -9999 comes from the nodata mask.  Counts, and integer accuflux (WEIGHTS) on the tiled
    engine."""
    import pyflwdir_amd as pyflwdir

    d8, exp = _ref(oracle, ("epi", shape, tilt, nodata_pct),
                   lambda: _synth_both_pits(oracle, shape, seed=11, tilt=tilt, white=2, nodata_pct=nodata_pct))
    if nodata_pct:  # (the mask of seed 11 cuts through the interior tiles: quads with some, all and no nodata)
        inner = exp[64:256, 64:256]
        assert (inner == -9999).any() and (inner > 0).any()
    _both_handles(d8, exp)
    idxs_ds, idxs_pit, _ = oracle.from_array(d8)
    seq = oracle.idxs_seq(idxs_ds, idxs_pit)
    wi = (np.arange(d8.size, dtype=np.int64) * 2654435761 % 7).astype(np.int32)  # small, non-negative
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    flw._h.set_profiling(True)
    got = flw.accuflux(wi.reshape(shape))
    assert any(s["name"] == "tile_local" for s in flw._h.last_timing())  # the tiled engine ran it
    flw._h.set_profiling(False)
    assert np.array_equal(got.ravel(), oracle.accuflux(idxs_ds, seq, wi))


# ---- supertile solves: list batches, boundary pulls ------------------------------------------------------------------
_SUPER = [("south", 4), ("south_east", 2), ("east", 1)] + [
    (f"tilt{t}_nd{nd}", (t, nd)) for t in (1 << 26, 100000, 3000) for nd in (0, 30)]


def _super_raster(oracle, spec):
    if isinstance(spec, int):
        return np.full((1100, 1100), spec, np.uint8)
    return oracle.synth_d8(1100, 1100, seed=21, tilt=spec[0], white=2, nodata_pct=spec[1])


def test_super_exit_counts(oracle):
    """What the rasters below put into the list phase (16 entries per thread, 512 per step of a workgroup), derived
    from the codes on the CPU.  1100 x 1100 is 3 x 3 supertiles, the outer ones 76 cells wide / high:
      south       4096 4096 608 | 4096 4096 608 | 512 512 76    (full supertiles: a batch ends exactly at the count)
      south-east  8128 8128 1104 | 8128 8128 1104 | 1104 1104 149   (just under the 8192 kept in LDS; last batch part filled)
      east        4096 4096 512 | 4096 4096 512 | 608 608 76
      synthetic   tilt 2^26: 6875 7002 1213 6769 7225 1063 913 926 135, with 30 % nodata 4019 5744 1213 4658 5873 904 703 686 0;
                  tilt 100000: 6726 6498 1164 6496 7125 1060 912 924 128 / 3937 5280 1164 4443 5800 904 705 685 0;
                  tilt 3000: 5774 6012 1077 6004 6350 953 886 946 131 / 3419 5092 1077 4096 5019 834 631 700 0
    so that with the capacity lowered to 5000 every raster but south / east has supertiles on both sides of it, and
    counts below 512 (and 0) occur."""
    c = {name: exit_counts(_super_raster(oracle, spec)) for name, spec in _SUPER[:4]}
    assert c["south"].tolist() == [[4096, 4096, 608], [4096, 4096, 608], [512, 512, 76]]
    assert c["south_east"].tolist() == [[8128, 8128, 1104], [8128, 8128, 1104], [1104, 1104, 149]]
    assert c["east"].tolist() == [[4096, 4096, 512], [4096, 4096, 512], [608, 608, 76]]
    s = c[_SUPER[3][0]]
    assert s.max() < 8192 and s.max() > 5000 and s.min() < 512


@pytest.mark.parametrize("scap", [None, "5000"])
@pytest.mark.parametrize("name,spec", _SUPER)
def test_super_solve_batches(gpu_lib, oracle, monkeypatch, name, spec, scap):
    """Both supertile solves (roots, then totals) in the regular form and, with the capacity lowered, in the flagged form
    for the fuller supertiles; single handle, deferred handle, and three row blocks (the first solve of a block only
    produces the totals of its edge supertile rows)."""
    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip, dist

    d8, exp = _ref(oracle, ("super", name), lambda: _super_raster(oracle, spec))
    if scap is not None:
        monkeypatch.setenv("PFD_TEST_SCAP", scap)
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    assert np.array_equal(flw.upstream_area(), exp)
    h = _hip.RasterHandle(d8, d8.shape[0], d8.shape[1], deferred=True)
    got = h.upstream_area_cell().reshape(d8.shape)
    h.close()
    assert np.array_equal(got, exp)
    assert np.array_equal(dist.upstream_area_blocks(d8, 3), exp)
