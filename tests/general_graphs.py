"""Deterministic general ``idxs_ds`` graphs for the general engine (csrc/general.hip): trees and forests whose links go
anywhere in the raster (the node labels are a random permutation of the valid cells), with in-degrees far above the 8 of
a D8 raster, depths from one level to thousands, and rho-shaped cycles with trees hanging off them.  Pure numpy; shared
by tests/test_general_graphs.py (the conditions every case meets, on the CPU) and tests/test_gpu_general_fuzz.py."""
from __future__ import annotations

import numpy as np

FAMILIES = ["chain", "star", "recursive", "pref", "binary", "allpits"]
# the smallest shapes that hit the edges: two cells, the 256-thread grid edge in one row / one column, one block, 248
# blocks with a ragged last one, exactly 2**16 cells
SHAPES = [(1, 2), (1, 255), (1, 256), (1, 257), (16, 16), (255, 1), (300, 211), (64, 1024)]
MAX_INDEGREE = 100  # (the reference counts upstream cells in int8 and indexes its upstream matrix with the count)
MAX_CHAIN = 3000  # most nodes of a chain graph = its depth: one launch per level on the device


def missing_value(dtype):
    dtype = np.dtype(dtype)
    return dtype.type(np.iinfo(dtype).max) if dtype.kind == "u" else dtype.type(-1)


def _parents(rng, family, m, n_pits):
    """Parent of every node 0 .. m-1 in node space (nodes 0 .. n_pits-1 are the pits: own parent); a parent always has
    a smaller number than its child."""
    par = np.arange(m, dtype=np.int64)
    p = n_pits
    k = np.arange(p, m, dtype=np.int64)
    if family == "allpits" or m == p:
        return par
    if family == "chain":  # every node drains into the previous one; the pits sit at random places of the line
        cut = np.zeros(m, bool)
        cut[0] = True
        if p > 1:
            cut[rng.choice(np.arange(1, m), size=p - 1, replace=False)] = True
        par = np.where(cut, par, par - 1)
    elif family == "star":  # hub j takes the next cap[j] nodes, the first hubs are the pits
        cap = rng.integers(40, MAX_INDEGREE + 1, size=m)
        par[p:] = np.searchsorted(np.cumsum(cap), k - p, side="right")
    elif family == "binary":
        par[p:] = (k - p) // 2
    elif family == "recursive":
        par[p:] = (rng.random(m - p) * k).astype(np.int64)
    elif family == "pref":
        early = (rng.random(m - p) * k).astype(np.int64).tolist()
        copy = (rng.random(m - p) < 0.8).tolist()
        pl = par.tolist()
        cnt = [0] * m
        for i, x in enumerate(range(p, m)):
            j = early[i]
            q = pl[j] if copy[i] else j
            if cnt[q] >= MAX_INDEGREE:
                q = j
            while cnt[q] >= MAX_INDEGREE:  # (a parent that is full: the node before it)
                q = q - 1 if q > 0 else x - 1
            pl[x] = q
            cnt[q] += 1
        par = np.array(pl, np.int64)
    else:
        raise ValueError(f"unknown family {family}")
    # the in-degree cap for the families that do not keep it by construction
    for _ in range(64):
        deg = np.bincount(par[p:], minlength=m)
        full = np.flatnonzero(deg > MAX_INDEGREE)
        if full.size == 0:
            break
        for q in full:
            kids = p + np.flatnonzero(par[p:] == q)
            move = kids[MAX_INDEGREE:]
            par[move] = (rng.random(move.size) * move).astype(np.int64)
    return par


def _children(par):
    """CSR of the children in node space."""
    m = par.size
    nonpit = np.flatnonzero(par != np.arange(m))
    order = nonpit[np.argsort(par[nonpit], kind="stable")]
    off = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(par[nonpit], minlength=m), out=off[1:])
    return off, order


def _subtree(off, kids, v):
    out, todo = [], [int(v)]
    while todo:
        x = todo.pop()
        out.append(x)
        todo.extend(kids[off[x]:off[x + 1]].tolist())
    return np.array(out, np.int64)


def reaches_pit(ds, mv):
    """Boolean per cell: valid and on a path that ends in a pit (pointer doubling on the host)."""
    n = ds.size
    idx = np.arange(n, dtype=np.int64)
    valid = ds != mv
    hop = np.where(valid, ds.astype(np.int64), idx)
    for _ in range(max(1, int(np.ceil(np.log2(max(n, 2)))) + 1)):
        hop = hop[hop]
    return valid & (ds.astype(np.int64)[hop] == hop)


def make(seed, shape, family, p_nodata, n_pits, n_cycles, dtype=np.int32):
    """Flat ``idxs_ds`` of ``shape``: own index on pits, the dtype's missing value on nodata cells.  ``n_cycles`` (at
    most 3) non-pit nodes are re-pointed to one of their own descendants: the node and its subtree leave the sequence,
    as a cycle with the rest of the subtree hanging off it.  A node is only re-pointed while at least half of the valid
    cells still reach a pit; fewer cycles are made where no node allows it."""
    nrow, ncol = shape
    n = nrow * ncol
    rng = np.random.default_rng([int(seed), FAMILIES.index(family), nrow, ncol])
    valid = rng.random(n) >= p_nodata
    if valid.sum() < 2:
        valid[rng.choice(n, size=2, replace=False)] = True
    cells = rng.permutation(np.flatnonzero(valid))
    m = cells.size
    if family == "chain" and m > MAX_CHAIN:  # (the depth cap: the other cells of a large raster are nodata)
        cells = cells[:MAX_CHAIN]
        m = MAX_CHAIN
    n_pits = m if family == "allpits" else max(1, min(int(n_pits), m - 1))
    par = _parents(rng, family, m, n_pits)
    # cycles
    budget = m - (m + 1) // 2  # nodes that may leave the sequence
    if n_cycles > 0 and budget >= 2 and family != "allpits":
        size = np.ones(m, np.int64)
        pl = par.tolist()
        sz = size.tolist()
        for x in range(m - 1, 0, -1):
            if pl[x] != x:
                sz[pl[x]] += sz[x]
        size = np.array(sz, np.int64)
        off, kids = _children(par)
        gone = np.zeros(m, bool)
        for _ in range(min(int(n_cycles), 3)):
            left = budget - int(gone.sum())
            free = ~gone & (par != np.arange(m))
            cand = np.empty(0, np.int64)
            for lo, hi in ((3, left // 2), (3, left), (2, left)):  # (leave room for the next cycle where that works)
                cand = np.flatnonzero((size >= lo) & (size <= hi) & free)
                if cand.size:
                    break
            if cand.size == 0:
                break
            # (the larger subtrees: a cycle of some length with something hanging off it)
            v = int(cand[np.argsort(size[cand], kind="stable")][-1 - int(rng.integers(0, min(8, cand.size)))])
            sub = _subtree(off, kids, v)
            deg = np.bincount(par[par != np.arange(m)], minlength=m)
            below = sub[(sub != v) & (deg[sub] < MAX_INDEGREE)]
            if below.size == 0:
                break
            par[v] = int(below[int(rng.integers(0, below.size))])
            gone[sub] = True
    ds = np.full(n, -1, np.int64)
    ds[cells] = cells[par]
    mv = missing_value(dtype)
    out = ds.astype(dtype)
    out[ds < 0] = mv
    return out


def _case_list():
    cases = []
    i = 0
    for family in FAMILIES:
        for shape in SHAPES:
            p_nodata = 0.0 if shape == (1, 2) else [0.0, 0.1, 0.3][i % 3]
            c = dict(family=family, shape=shape, seed=100 + i, p_nodata=p_nodata, n_pits=[1, 3, 7][(i // 3) % 3],
                     n_cycles=[3, 1, 2, 0][i % 4])
            if family == "chain" and shape == (300, 211):  # the deepest case: one line of MAX_CHAIN cells
                c.update(n_pits=1, n_cycles=0)
            cases.append(c)
            i += 1
    return cases


CASES = _case_list()


def case_id(c):
    return f"{c['family']}-{c['shape'][0]}x{c['shape'][1]}-s{c['seed']}"


def build(c, dtype=np.int32):
    return make(c["seed"], c["shape"], c["family"], c["p_nodata"], c["n_pits"], c["n_cycles"], dtype=dtype)


def cannot_be_general(c):
    """The two kinds of case whose links can not leave the 8 neighbours whatever the labels: the two cells of a 1 x 2
    raster are neighbours, and a graph of pits alone has no links.  The GPU tests put them on the general engine with
    ``ftype="nextxy"``, which never takes the D8 engines."""
    return c["shape"] == (1, 2) or c["family"] == "allpits"
