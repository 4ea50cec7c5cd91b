"""What can be checked without a device about the rasters and payloads of tests/exact_dispatch.py: the GPU tests of the
exact-order engine's dispatch (tests/test_gpu_exact_dispatch.py) rely on these rasters being acyclic, on TAIL and
TAIL_BLOCKS holding a river long enough for the two-stream tail (a chain of XTAIL_LONG = 16384 slots needs a river of as
many cells), and on every nodata rule being exercised."""
import numpy as np
import pytest

import exact_dispatch as X

ALL = X.SMALL + ("TAIL", "TAIL_BLOCKS")


@pytest.mark.parametrize("name", ALL)
def test_raster_is_acyclic_and_drains(oracle, name):
    r = X.raster(name)
    idxs_ds, idxs_pit, seq = r.graph
    valid = r.d8.ravel() != 247
    rank = oracle.rank(idxs_ds)[0]
    assert idxs_pit.size > 0 and not (rank[valid] == -1).any()
    assert seq.size == int(valid.sum())  # every valid cell reaches a pit


def test_tail_stem_and_codes(oracle):
    """TAIL: one main stem of 18000 cells before and after the headwater step (max rank 17999), both pit codes, nodata on
    30 % of the former headwaters and nowhere else."""
    before, r = X.Raster("TAIL before the headwater step", X.tail_d8(headwaters=False)), X.raster("TAIL")
    assert r.shape == X.TAIL_SHAPE
    assert before.stem() == 18000 and int(oracle.rank(before.graph[0])[0].max()) == 17999
    assert r.stem() >= 17999 and r.stem() >= X.XTAIL_LONG
    assert (r.d8 == 0).any() and (r.d8 == 255).any() and (r.d8 == 247).any()
    removed = r.d8 != before.d8
    assert np.array_equal(removed, r.d8 == 247) and (before.upa.reshape(r.shape)[removed] == 1).all()
    heads = int((before.upa == 1).sum())
    assert 0.28 * heads < int(removed.sum()) < 0.32 * heads
    # the stem's basin is most of the raster (12.0 M of its 14.5 M valid cells)
    assert int(r.upa.max()) > 0.8 * int((r.d8 != 247).sum())


def test_tail_blocks_stems(oracle):
    """TAIL_BLOCKS: either half plus its halo row, as dist._block_handle cuts it, holds a stem of 18001 cells."""
    from pyflwdir_amd import dist

    r = X.raster("TAIL_BLOCKS")
    assert r.shape == X.TAIL_BLOCKS_SHAPE and r.nblocks == 2 and r.stem() == 36000
    for b in range(r.nblocks):
        a, e = dist.block_slice(r.shape[0], r.nblocks, b)
        assert e - a == 18001
        assert X.Raster(f"block {b}", r.d8[a:e]).stem() == 18001


@pytest.mark.parametrize("name", ALL)
def test_payloads_hold_their_nodata(name):
    r = X.raster(name)
    valid = r.d8.ravel() != 247
    for key, nd in X.NODATA.items():
        p = r.payloads[key]
        assert p.size == r.n and (p[valid] == nd).any() and (p[valid] != nd).any(), (name, key)
    if r.n > 1000:
        assert r.payloads["i32"][valid].min() < 0  # (negative values: the exact engine takes int32 accuflux, not the tiled one)
        assert r.payloads["mask"].any() and not r.payloads["mask"].all() and r.payloads["drain"].any()
        assert (r.payloads["flood_upa"][valid] >= X.FLOOD_UPA_MIN).any()


def test_launch_formulas():
    plan = dict(slots=100, rounds=5, tail_split=-1)
    assert X.up_launches(plan) == 12 and X.down_launches(plan) == 7
    plan["tail_split"] = 29
    assert X.up_launches(plan) == 13 and X.down_launches(plan) == 8
    assert X.up_launches(dict(slots=0, rounds=0, tail_split=-1)) == 1 == X.down_launches(dict(slots=0, rounds=0, tail_split=-1))
    assert X.fuse_min("production", None) == 1 << 20 and X.fuse_min("suite", None) == 1
    assert X.fuse_min("straddle", dict(widest_round=777)) == 777


def test_every_operation_has_a_reference_of_the_rasters_size():
    r = X.raster("synth_rough_nodata_384x512")
    for op in X.OPS:
        exp = op.expected(r)
        assert exp.size == r.n and not exp.flags.writeable, op.name
    assert {v[0] for v in X.BLOCK_OPS.values()} <= set(X.OP)
