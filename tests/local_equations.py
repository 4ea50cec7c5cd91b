"""The local equations of the sweeps' results, restated in plain numpy from the reference's serial loops
(pyflwdir/streams.py, dem.py, basins.py, core.py) and the contracts of include/pfd.h — the independent side of
tests/test_gpu_verifiers.py.  Nothing here imports the library or follows csrc/rules.h: the device verifiers
(csrc/checks.hip, the verify mode of the row-block sweeps) are compared with these counts, cell for cell.

Every function takes the flow graph as ``idxs_ds`` (flat, the downstream cell's linear index, the cell itself at a
pit, negative on nodata — core_d8.from_array) with the raster's ``shape``, the operation's inputs and a candidate
result, and returns two boolean maps: the valid cells whose local equation fails, and the nodata cells that do not
hold the value the reference leaves there.  Arithmetic is done in the result's own dtype (numpy array arithmetic:
float32 adds round to float32, integer adds wrap) and values are compared by their bit patterns unless stated.

A serial loop of the reference that runs "up- to downstream" over ``seq[::-1]`` adds the upstream cells of a cell in
DESCENDING linear index (core.idxs_seq appends them in ascending index per level): ``NEIGHBOURS`` is in that order."""
import numpy as np

# (dr, dc) of the eight neighbours of a cell, in descending linear index
NEIGHBOURS = ((1, 1), (1, 0), (1, -1), (0, 1), (0, -1), (-1, 1), (-1, 0), (-1, -1))
# core_d8._ds: the D8 code of a step (dr, dc)
D8_CODE = {(0, 1): 1, (1, 1): 2, (1, 0): 4, (1, -1): 8, (0, -1): 16, (-1, -1): 32, (-1, 0): 64, (-1, 1): 128}
D8_NODATA = 247


def graph_of_d8(d8):
    """core_d8.from_array: idxs_ds (int64; -1 on nodata) of a D8 raster; a cell that points off the raster or into
    nodata is a pit like the codes 0 and 255."""
    d8 = np.asarray(d8, np.uint8)
    nrow, ncol = d8.shape
    idx = np.arange(d8.size, dtype=np.int64).reshape(d8.shape)
    r, c = np.divmod(idx, ncol)
    ds = idx.copy()
    for (dr, dc), code in D8_CODE.items():
        rr, cc = r + dr, c + dc
        inside = (d8 == code) & (rr >= 0) & (rr < nrow) & (cc >= 0) & (cc < ncol)
        tgt = np.where(inside, rr * ncol + cc, 0)
        ok = inside & (d8.ravel()[tgt] != D8_NODATA)
        ds[ok] = tgt[ok]
    ds[d8 == D8_NODATA] = -1
    return ds.ravel()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def differ(a, b):
    """Cells whose bit patterns differ (-0.0 is not 0.0, a NaN equals only the NaN with the same payload)."""
    return _bits(a) != _bits(b)


def _shifted(a2, dr, dc, fill=0):
    """out[r, c] = a2[r + dr, c + dc], ``fill`` outside the raster."""
    nrow, ncol = a2.shape
    out = np.full_like(a2, fill)
    r0, r1 = max(0, -dr), min(nrow, nrow - dr)
    c0, c1 = max(0, -dc), min(ncol, ncol - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = a2[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


class Graph:
    """idxs_ds with the maps every equation needs."""

    def __init__(self, idxs_ds, shape):
        self.shape = tuple(shape)
        self.ds = np.asarray(idxs_ds).astype(np.int64).ravel()
        self.n = self.ds.size
        assert self.n == shape[0] * shape[1]
        self.idx = np.arange(self.n, dtype=np.int64)
        self.valid = self.ds >= 0
        self.pit = self.ds == self.idx
        self.down = np.where(self.valid, self.ds, self.idx)  # (a pit and a nodata cell: the cell itself)
        ds2 = self.ds.reshape(self.shape)
        idx2 = self.idx.reshape(self.shape)
        # per neighbour, in descending linear index: does it drain into this cell?
        self.inflow = [(_shifted(ds2, dr, dc, -1) == idx2).ravel() & self.valid for dr, dc in NEIGHBOURS]

    def neighbour(self, values, k):
        """The neighbour's value per cell (anything where there is no such neighbour)."""
        dr, dc = NEIGHBOURS[k]
        return _shifted(np.asarray(values).reshape(self.shape), dr, dc).ravel()

    def n_upstream(self):
        return np.sum(self.inflow, axis=0)


def _split(g, wrong, nodata_wrong):
    return wrong & g.valid, nodata_wrong & ~g.valid


# ---------------------------------------------------------------------------------------------
# upstream_area("cell"), basins labels, HAND: the whole-raster verifiers of csrc/checks.hip
# ---------------------------------------------------------------------------------------------
def upa_cell(g, upa):
    """streams.accuflux over ones (streams.py:15-41) with -9999 on nodata (pyflwdir.py:770-801): int32, wrapping."""
    upa = np.asarray(upa, np.int32).ravel()
    acc = np.ones(g.n, np.int32)
    with np.errstate(over="ignore"):
        for k in range(8):
            acc = np.where(g.inflow[k], acc + g.neighbour(upa, k), acc)
    return _split(g, acc != upa, upa != -9999)


def upa_cell_stats(g, upa):
    """What pfd_verify_upstream_area_cell reports (include/pfd.h)."""
    upa = np.asarray(upa, np.int32).ravel()
    bad, bad_nodata = upa_cell(g, upa)
    return dict(bad_cells=int(bad.sum()), bad_nodata=int(bad_nodata.sum()),
                pit_sum=int(upa[g.pit].view(np.uint32).sum(dtype=np.uint64)), n_pits=int(g.pit.sum()),
                checksum=int(upa.sum(dtype=np.int64)), n_valid=int(g.valid.sum()))


def labels(g, outlets, ids, lab):
    """basins.basins + core.fillnodata_upstream with nodata 0 (basins.py:12-18, core.py:120-146): a seeded cell holds its
    id, any other cell the label of its downstream cell, an unseeded pit and a nodata cell hold 0."""
    lab = np.asarray(lab, np.uint32).ravel()
    seed = np.zeros(g.n, np.uint32)
    seed[np.asarray(outlets, np.int64)] = np.asarray(ids, np.uint32)
    exp = np.where(seed != 0, seed, np.where(g.pit, np.uint32(0), lab[g.down]))
    return _split(g, exp != lab, lab != 0)


def labels_stats(g, outlets, ids, lab):
    lab = np.asarray(lab, np.uint32).ravel()
    bad, bad_nodata = labels(g, outlets, ids, lab)
    return dict(bad_cells=int(bad.sum()), bad_nodata=int(bad_nodata.sum()), checksum=int(lab.sum(dtype=np.uint64)),
                n_labelled=int((g.valid & (lab != 0)).sum()))


def hand(g, drain, elevtn, hnd):
    """dem.height_above_nearest_drain (dem.py:299-330): 0.0 on a drain cell (drain == 1), else the downstream cell's height
    (0.0 at a pit: the loop reads the initial value) plus the elevation difference, taken in the elevation dtype and
    widened; -9999.0 on nodata.  Bitwise, except that any NaN equals any NaN (the contract of csrc/checks.hip)."""
    hnd = np.asarray(hnd, np.float64).ravel()
    elevtn = np.asarray(elevtn).ravel()
    assert elevtn.dtype in (np.float32, np.float64)
    is_drain = np.asarray(drain).ravel().view(np.uint8) == 1
    with np.errstate(invalid="ignore", over="ignore"):
        dz = elevtn - elevtn[g.down]
        assert dz.dtype == elevtn.dtype
        exp = np.where(g.pit, np.float64(0.0), hnd[g.down]) + dz.astype(np.float64)
    exp = np.where(is_drain, np.float64(0.0), exp)
    wrong = differ(exp, hnd) & ~(np.isnan(exp) & np.isnan(hnd))
    return _split(g, wrong, hnd != -9999.0)


def hand_stats(g, drain, elevtn, hnd):
    hnd = np.asarray(hnd, np.float64).ravel()
    bad, bad_nodata = hand(g, drain, elevtn, hnd)
    is_drain = np.asarray(drain).ravel().view(np.uint8) == 1
    with np.errstate(over="ignore"):
        csum = hnd.view(np.uint64).sum(dtype=np.uint64)
    return dict(bad_cells=int(bad.sum()), bad_nodata=int(bad_nodata.sum()), checksum=int(np.array(csum).view(np.int64)),
                n_drain=int((g.valid & is_drain).sum()))


# ---------------------------------------------------------------------------------------------
# the sweeps the row-block verifiers cover
# ---------------------------------------------------------------------------------------------
def _payload(g, data, by_row):
    data = np.asarray(data)
    if by_row:
        assert data.size == g.shape[0]
        return np.repeat(data, g.shape[1])
    return data.ravel()


def accuflux_up(g, data, out, nodata=None, by_row=False):
    """streams.accuflux (streams.py:15-41): ``accu = data.copy()``, then every upstream cell, in descending linear index,
    is added unless the running sum or the upstream cell's (final) value is nodata.  Nodata cells keep their payload."""
    out = np.asarray(out).ravel()
    data = _payload(g, data, by_row).astype(out.dtype, copy=False)
    acc = data.copy()
    with np.errstate(all="ignore"):
        for k in range(8):
            u = g.neighbour(out, k)
            add = g.inflow[k].copy()
            if nodata is not None:
                add &= (acc != out.dtype.type(nodata)) & (u != out.dtype.type(nodata))
            acc = np.where(add, acc + u, acc)
    assert acc.dtype == out.dtype
    return _split(g, differ(acc, out), differ(data, out))


def accuflux_down(g, data, out, nodata=None, by_row=False):
    """streams.accuflux_ds (streams.py:44-70): ``accu[idx0] += accu[idx_ds]`` unless the cell is a pit or either value is
    nodata; the downstream cell's value is final when the loop reads it."""
    out = np.asarray(out).ravel()
    data = _payload(g, data, by_row).astype(out.dtype, copy=False)
    d = out[g.down]
    add = ~g.pit
    if nodata is not None:
        add = add & (d != out.dtype.type(nodata)) & (data != out.dtype.type(nodata))
    with np.errstate(all="ignore"):
        exp = np.where(add, data + d, data)
    assert exp.dtype == out.dtype
    return _split(g, differ(exp, out), differ(data, out))


def strahler(g, out, mask=None):
    """streams.strahler_order (streams.py:228-269), uint8.  The loop keeps, per cell, the running order and the largest
    order among the tributaries seen so far; replayed here over the (at most eight) upstream cells of every cell at once,
    in the loop's order.  A cell outside the mask is skipped by the loop: it passes nothing on, and is no headwater.
    (An upstream cell inside the mask holds at least 1 in every run of the loop; the equation of the cell below a
    candidate that holds 0 there is not defined, and tests/verifier_cases.py builds no such candidate.)"""
    out = np.asarray(out, np.uint8).ravel()
    inside = g.valid if mask is None else g.valid & (np.asarray(mask).ravel() != 0)
    strord = np.zeros(g.n, np.uint8)
    strmax = np.zeros(g.n, np.uint8)
    for k in range(8):
        sto = g.neighbour(out, k)
        # the upstream cell runs its own iteration only inside the mask; its value is final by then
        act = g.inflow[k] & g.neighbour(inside, k).astype(bool)
        lower = act & (strord < sto)
        inc = act & ~lower & (sto == strord) & (strmax == sto)
        new = np.where(lower, sto, np.where(inc, strord + np.uint8(1), strord)).astype(np.uint8)
        strmax = np.where(act & (strmax < sto), sto, strmax)
        strord = new
    # a headwater cell inside the mask starts at 1; a cell outside the mask keeps what its tributaries left there
    exp = np.where(inside & (strord == 0), np.uint8(1), strord)
    return _split(g, exp != out, out != 0)


def stream_distance(g, out, mask=None, steps=None):
    """streams.stream_distance (streams.py:272-315): 0 at a pit and inside the mask, else the downstream cell's distance plus
    one cell (int32) or plus the step's length (float32; ``steps``: the float32 table [2 * nrow - 1, 3] over the row sum
    and the kind of step — vertical, horizontal, diagonal — that gis_utils.distance gives); -9999 on nodata."""
    real = steps is not None
    out = np.asarray(out, np.float32 if real else np.int32).ravel()
    ncol = g.shape[1]
    reset = g.pit.copy()
    if mask is not None:
        reset |= np.asarray(mask).ravel() != 0
    if real:
        r0, c0 = np.divmod(g.idx, ncol)
        r1, c1 = np.divmod(g.down, ncol)
        kind = np.where(r0 == r1, 1, np.where(c0 == c1, 0, 2))
        d = np.asarray(steps, np.float32).reshape(-1, 3)[r0 + r1, kind]
        exp = np.where(reset, np.float32(0), out[g.down] + d)
    else:
        with np.errstate(over="ignore"):
            exp = np.where(reset, np.int32(0), out[g.down] + np.int32(1))
    assert exp.dtype == out.dtype
    return _split(g, differ(exp, out), out != out.dtype.type(-9999))


def fillnodata_up(g, data, out, nodata):
    """core.fillnodata_upstream (core.py:120-146): a cell that holds nodata takes its downstream cell's (final) value when
    that is not nodata; every other cell, a pit and a raster-nodata cell keep their payload."""
    out = np.asarray(out).ravel()
    data = np.asarray(data).ravel()
    nd = out.dtype.type(nodata)
    d = out[g.down]
    exp = np.where(~g.pit & (data == nd) & (d != nd), d, data)  # (a pit reads itself: still nodata)
    return _split(g, differ(exp, out), differ(data, out))


def fillnodata_down(g, data, out, nodata, how="max"):
    """core.fillnodata_downstream (core.py:149-188): a cell whose payload is nodata gathers its upstream cells' (final)
    values that are not nodata, in descending linear index: the first replaces the nodata, the others are merged with
    ``max`` / ``min`` / ``+=`` (upstream value first, as the loop writes ``max(data_out[idx0], data_out[idx_ds])``)."""
    out = np.asarray(out).ravel()
    data = np.asarray(data).ravel()
    nd = out.dtype.type(nodata)
    acc = data.copy()
    open_ = data == nd
    with np.errstate(all="ignore"):
        for k in range(8):
            u = g.neighbour(out, k)
            take = g.inflow[k] & open_ & (u != nd)
            first = take & (acc == nd)
            if how == "max":
                merged = np.where(acc > u, acc, u)  # Python's max(u, acc): acc only when it is larger
            elif how == "min":
                merged = np.where(acc < u, acc, u)
            else:
                merged = acc + u
            acc = np.where(first, u, np.where(take, merged, acc))
    assert acc.dtype == out.dtype
    return _split(g, differ(acc, out), differ(data, out))


def trib_info(g, idxs_us_main, mask=None):
    """The byte include/pfd.h documents for pfd_trib_info_block, from core.main_upstream's result and core.upstream_count:
    low four bits the D8 slot (code == 1 << slot) of the step from the cell to its main upstream cell, 15 if it has none;
    bit 4 set when more than one upstream cell lies inside the mask."""
    main = np.asarray(idxs_us_main).astype(np.int64).ravel()
    ncol = g.shape[1]
    slot = np.full(g.n, 15, np.uint8)
    has = g.valid & (main >= 0)
    dr = main // ncol - g.idx // ncol
    dc = main % ncol - g.idx % ncol
    for (r, c), code in D8_CODE.items():
        slot[has & (dr == r) & (dc == c)] = int(code).bit_length() - 1
    inside = np.ones(g.n, bool) if mask is None else np.asarray(mask).ravel() != 0
    nup = np.zeros(g.n, np.int32)
    for k in range(8):
        nup += g.inflow[k] & g.neighbour(inside, k).astype(bool)
    return (slot | np.where(g.valid & (nup > 1), 0x10, 0)).astype(np.uint8)


def classic_order(g, tinfo, out, mask=None):
    """streams.stream_order (streams.py:191-225), uint8: 0 outside the mask (the loop skips the cell), 1 at a pit, else the
    downstream cell's order, plus one when that cell has more than one upstream cell inside the mask and this cell is not
    its main upstream cell — both read from the downstream cell's ``tinfo`` byte."""
    out = np.asarray(out, np.uint8).ravel()
    tinfo = np.asarray(tinfo, np.uint8).ravel()
    ncol = g.shape[1]
    inside = np.ones(g.n, bool) if mask is None else np.asarray(mask).ravel() != 0
    # the D8 slot of the step from the downstream cell back to this cell
    dr = g.idx // ncol - g.down // ncol
    dc = g.idx % ncol - g.down % ncol
    back = np.full(g.n, 15, np.uint8)
    for (r, c), code in D8_CODE.items():
        back[(dr == r) & (dc == c)] = int(code).bit_length() - 1
    t = tinfo[g.down]
    trib = ((t & 0x10) != 0) & ((t & 0x0F) != back)
    exp = np.where(g.pit, np.uint8(1), out[g.down] + trib.astype(np.uint8)).astype(np.uint8)
    exp = np.where(inside, exp, np.uint8(0))
    return _split(g, exp != out, out != 0)


FLOOD_STATE = np.dtype([("z", np.float32), ("h", np.float32), ("flag", np.int32), ("pad", np.int32)])


def floodplains_state(g, elevtn, is_stream, stream_h, state):
    """dem.floodplains (dem.py:333-379) with its three arrays as one record per cell (include/pfd.h pfd_floodplains_block:
    z = drainz, h = drainh, flag = fldpln): a stream cell (``uparea >= upa_min``; ``stream_h`` = ``uparea ** b`` as float32)
    holds (float32(elevtn), h, 1); another cell whose downstream cell is floodplain and lies no more than that cell's h
    above its z (difference in the dtype of ``elevtn - float32``) holds the downstream cell's (z, h, 1); every other
    valid cell — a pit that is no stream cell reads its own initial flag 0 — holds (-9999, -9999, 0), a nodata cell
    (-9999, -9999, -1).  The padding word is not compared."""
    st = np.asarray(state).ravel().view(FLOOD_STATE) if np.asarray(state).dtype != FLOOD_STATE else np.asarray(state).ravel()
    elevtn = np.asarray(elevtn).ravel()
    assert elevtn.dtype in (np.float32, np.float64)
    stream = np.asarray(is_stream).ravel().view(np.uint8) == 1
    h_in = np.asarray(stream_h, np.float32).ravel()
    dn = st[g.down]
    with np.errstate(invalid="ignore", over="ignore"):
        dh = elevtn - dn["z"]
        assert dh.dtype == elevtn.dtype
        inherit = ~g.pit & (dn["flag"] == 1) & (dh <= dn["h"])
        ez = np.where(stream, elevtn.astype(np.float32), np.where(inherit, dn["z"], np.float32(-9999.0)))
    eh = np.where(stream, h_in, np.where(inherit, dn["h"], np.float32(-9999.0)))
    ef = np.where(stream | inherit, 1, 0).astype(np.int32)
    wrong = differ(ez, st["z"]) | differ(eh, st["h"]) | (ef != st["flag"])
    nd_wrong = differ(np.full(g.n, -9999.0, np.float32), st["z"]) | differ(np.full(g.n, -9999.0, np.float32), st["h"]) | \
        (st["flag"] != -1)
    return _split(g, wrong, nd_wrong)
