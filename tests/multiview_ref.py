"""include/gpn.h section MV restated in plain numpy: the reference of tests/test_multiview_cpu.py and tests/test_gpu_multiview*.py.
Per-pixel arithmetic is written element by element in the contract's order (numpy evaluates every ufunc call on its own, so
nothing is contracted); everything that is an algorithm - the distinct (voxel, part) set, the pair table, the merge, the gather -
is a loop over Python sets, dicts and ``Fraction``.  ``merge`` has two forms: the literal repeated arg-max (small tables) and the
one pass over the sorted candidates the contract says it equals; ``tables_fast`` is the vectorised form for the larger shapes."""
from fractions import Fraction

import numpy as np

GRID = 1024
DEAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def counts_and_base(n_parts, GT):
    n = [min(max(int(x), 0), GT) for x in n_parts]
    base = [0]
    for x in n:
        base.append(base[-1] + x)
    return n, base


def part_of(inst, valid, n_parts, GT):
    """[V,H,W] i32: the global part of every pixel, or -1"""
    V = inst.shape[0]
    n, base = counts_and_base(n_parts, GT)
    out = np.full(inst.shape, -1, np.int32)
    for v in range(V):
        q = inst[v].astype(np.int64)
        m = (valid[v] != 0) & (q >= 0) & (q < n[v]) & (base[v] + q < GT)
        out[v][m] = (base[v] + q[m]).astype(np.int32)
    return out


def world_rows(rows, pof, R, t):
    """[V*H*W,3] f32, NaN for a non-member pixel"""
    V = pof.shape[0]
    HW = pof[0].size
    out = np.full((V * HW, 3), np.nan, np.float32)
    R, t = np.asarray(R, np.float64).reshape(V, 3, 3), np.asarray(t, np.float64).reshape(V, 3)
    for v in range(V):
        m = np.flatnonzero(pof[v].reshape(-1) >= 0) + v * HW
        x, y, z = (rows[m, k].astype(np.float64) for k in range(3))
        for k in range(3):
            a = x * R[v, k, 0]
            b = y * R[v, k, 1]
            c = z * R[v, k, 2]
            with np.errstate(all="ignore"):
                out[m, k] = (((a + b) + c) + t[v, k]).astype(np.float32)
    return out


def _image(col):
    """the order-preserving integer image of float32 values, as Python-sized ints"""
    u = col.view(np.uint32).astype(np.int64)
    return np.where(u >> 31, (~u) & 0xFFFFFFFF, u | 0x80000000)


def lower_bound(wrows, pof):
    """[3] f64: the smallest stored float32 per axis over the member pixels by the integer image (-0.0 < +0.0, NaN is the largest
    positive image), 0.0 without members"""
    m = pof.reshape(-1) >= 0
    lo = np.zeros(3, np.float64)
    if m.any():
        for k in range(3):
            col = np.ascontiguousarray(wrows[m, k])
            lo[k] = np.float64(col[int(np.argmin(_image(col)))])
    return lo


def area(pof, GT):
    out = np.zeros(GT, np.int32)
    for g in pof.reshape(-1):
        if g >= 0:
            out[g] += 1
    return out


def keys(wrows, pof, lo, cell, GT):
    """-> (keys [V,H,W] u64, dropped [V] i32)"""
    V = pof.shape[0]
    g = pof.reshape(-1).astype(np.int64)
    member = (g >= 0) & (g < GT)
    idx = np.zeros((g.shape[0], 3), np.int64)
    ok = np.ones(g.shape[0], bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            d = wrows[:, k].astype(np.float64) - np.float64(lo[k])
            q = np.floor(d / np.float64(cell))
            good = (q >= 0) & (q < GRID)
            ok &= good
            idx[:, k] = np.where(good, q, 0).astype(np.int64)
    vox = (idx[:, 0] << 20) | (idx[:, 1] << 10) | idx[:, 2]
    out = np.full(g.shape[0], DEAD, np.uint64)
    live = member & ok
    out[live] = ((vox[live] << 9) | g[live]).astype(np.uint64)
    dropped = np.array([int((member & ~ok).reshape(V, -1)[v].sum()) for v in range(V)], np.int32)
    return out.reshape(pof.shape), dropped


def tables(ks, GT):
    """vol [GT], inter [GT,GT] i32 from the set of distinct (vox, g): plain loops"""
    cells = {}
    for k in set(int(x) for x in ks.reshape(-1) if x != DEAD):
        cells.setdefault(k >> 9, set()).add(k & 511)
    vol, inter = np.zeros(GT, np.int32), np.zeros((GT, GT), np.int32)
    for parts in cells.values():
        for g in parts:
            vol[g] += 1
            for h in parts:
                if h != g:
                    inter[g, h] += 1
    return vol, inter


def tables_fast(ks, GT):
    """the same through a dense boolean occupancy over the distinct voxels (for the larger shapes)"""
    u = np.unique(ks.reshape(-1))
    u = u[u != DEAD].astype(np.int64)
    vox, g = np.unique(u >> 9, return_inverse=True)[1], u & 511
    occ = np.zeros((int(vox.max()) + 1 if vox.size else 0, GT), np.int64)
    occ[vox, g] = 1
    inter = occ.T @ occ
    vol = np.diag(inter).astype(np.int32).copy()
    np.fill_diagonal(inter, 0)
    return vol, inter.astype(np.int32)


def _candidates(inter, vol, cls, view_of, min_inter, min_overlap):
    GT = vol.shape[0]
    out = []
    for g in range(GT):
        for h in range(g + 1, GT):
            c = int(inter[g, h])
            if view_of[g] < 0 or view_of[h] < 0 or vol[g] <= 0 or vol[h] <= 0:
                continue
            m = int(min(vol[g], vol[h]))
            if cls[g] == cls[h] and c >= max(int(min_inter), 1) and float(c) >= float(min_overlap) * float(m):
                out.append((Fraction(c, m), g, h, c))
    return out


def merge(inter, vol, cls, n_parts, min_inter, min_overlap, literal=False):
    """the outputs of gpn_views_merge as a dict of host arrays"""
    GT, V = int(vol.shape[0]), len(n_parts)
    _, base = counts_and_base(n_parts, GT)
    base = [min(b, GT) for b in base]
    view_of = [-1] * GT
    for v in range(V):
        for g in range(base[v], base[v + 1]):
            view_of[g] = v
    vol = np.array([int(vol[g]) if view_of[g] >= 0 and vol[g] > 0 else 0 for g in range(GT)], np.int64)
    cls = [0] * GT if cls is None else [int(c) for c in cls]
    cand = _candidates(inter, vol, cls, view_of, min_inter, min_overlap)
    cluster = list(range(GT))
    views = {g: ({view_of[g]} if view_of[g] >= 0 else set()) for g in range(GT)}
    links = []

    def eligible(c):
        a, b = cluster[c[1]], cluster[c[2]]
        return a != b and not (views[a] & views[b])

    def unite(c):
        a, b = cluster[c[1]], cluster[c[2]]
        keep, gone = min(a, b), max(a, b)
        for g in range(GT):
            if cluster[g] == gone:
                cluster[g] = keep
        views[keep] |= views[gone]
        links.append((c[1], c[2], c[3]))

    order = lambda c: (-c[0], c[1], c[2])  # noqa: E731
    if literal:
        while True:
            live = [c for c in cand if eligible(c)]
            if not live:
                break
            unite(min(live, key=order))
    else:
        for c in sorted(cand, key=order):
            if eligible(c):
                unite(c)
    reps = sorted({cluster[g] for g in range(GT) if vol[g] > 0})
    F = len(reps)
    out = dict(fused_of=np.array([reps.index(cluster[g]) if vol[g] > 0 else -1 for g in range(GT)], np.int32).reshape(GT),
               n_fused=np.array([F], np.int32), fused_views=np.zeros(GT, np.uint64), fused_class=np.full(GT, -1, np.int32),
               fused_vol=np.zeros(GT, np.int32), fused_parts=np.full((GT, V), -1, np.int32), links=np.zeros((GT, 3), np.int32),
               n_links=np.array([len(links)], np.int32))
    out["links"][:, :2] = -1
    for i, l in enumerate(links):
        out["links"][i] = l
    for f, r in enumerate(reps):
        members = [g for g in range(GT) if cluster[g] == r]
        out["fused_views"][f] = np.uint64(sum(1 << view_of[g] for g in members))
        out["fused_class"][f] = cls[r]
        out["fused_vol"][f] = sum(int(vol[g]) for g in members)
        for g in members:
            out["fused_parts"][f, view_of[g]] = g - base[view_of[g]]
    return out


def relabel(pof, fused_of):
    GT = fused_of.shape[0]
    out = np.full(pof.shape, -1, np.int32)
    m = (pof >= 0) & (pof < GT)
    out[m] = fused_of[pof[m]]
    return out


def gather(wrows, npcs, fused_inst, seg_start, n_total, fill):
    """-> (xyz [M,3] f64, npcs_out [M,3] f64, src [M] i64); rows no segment covers hold ``fill``"""
    xyz, out_npcs = np.full((n_total, 3), fill, np.float64), np.full((n_total, 3), fill, np.float64)
    src = np.full(n_total, int(fill), np.int64)
    flat = fused_inst.reshape(-1)
    for f, s0 in enumerate(seg_start):
        if s0 < 0:
            continue
        rows = np.flatnonzero(flat == f)  # ascending (view, pixel)
        rows = rows[:max(n_total - int(s0), 0)]
        at = slice(int(s0), int(s0) + rows.shape[0])
        xyz[at], src[at] = wrows[rows].astype(np.float64), rows
        if npcs is not None:
            out_npcs[at] = npcs.reshape(-1, 3)[rows].astype(np.float64)
    return xyz, out_npcs, src


def fuse(rows, valid, inst, n_parts, cls, R, t, cell, min_inter, min_overlap, npcs=None, fast=False):
    """the whole contract -> dict: every table, fused_inst, and the clouds of all fused parts back to back"""
    GT = int(sum(n_parts))
    pof = part_of(inst, valid, n_parts, GT)
    wrows = world_rows(rows, pof, R, t)
    lo = lower_bound(wrows, pof)
    ks, dropped = keys(wrows, pof, lo, cell, GT)
    vol, inter = (tables_fast if fast else tables)(ks, GT)
    m = merge(inter, vol, cls, n_parts, min_inter, min_overlap)
    fused_inst = relabel(pof, m["fused_of"])
    F = int(m["n_fused"][0])
    ar = area(pof, GT)
    n_points = np.array([int(ar[m["fused_of"] == f].sum()) for f in range(F)], np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_points)]).astype(np.int64)
    xyz, npcs_out, src = gather(wrows, npcs, fused_inst, offsets[:-1], int(offsets[-1]), -1.0)
    out = dict(m, part_of=pof, wrows=wrows, lo=lo, keys=ks, dropped=dropped, vol=vol, inter=inter, area=ar, fused_inst=fused_inst,
               n_points=n_points, offsets=offsets, xyz=xyz, npcs=npcs_out, src=src)
    return out
