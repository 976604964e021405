"""Reference for the proposal stage (csrc/proposals.hip) and its post-processing (csrc/postprocess.hip): plain numpy, no torch,
no project kernel.  Everything but the per-proposal frame is integer work; the frame is transcribed one np.float32 operation
per line from the comment above prop_stats_kernel / segmented_voxelize in network/grouping_utils.py, so the voxel cells can be
compared without a tolerance.

build() returns a dict with the keys of hip_ops.proposals_build (counts Q, M, P, V, dropped, coarse; the tables sliced to
their sizes) or None when no proposal survives.  Keys that start with "_" (the frame itself) are extras that
assert_tables_equal does not compare.

`coarse` counts the rows of the proposal grid's stride-2 level as the rulebook builders do: distinct
(proposal, x // 2, y // 2, z // 2) rows whose coarse cell lies inside the coarse grid of floor(fullscale / 2)^3 cells.  For an
even fullscale that is every distinct row; for an odd one the cells x == fullscale - 1 have no coarse cell and do not count."""
import numpy as np

F = np.float32
BUILD_COUNTS = ("Q", "M", "P", "V", "dropped", "coarse")
BUILD_TABLES = ("valid_mask", "valid_indices", "sorted_indices", "point_indices", "proposal_indices", "batch_indices", "pt_xyz",
                "sem_preds", "instance_labels", "sizes", "proposal_offsets", "member_slot", "voxel_coords", "pc_voxel_id",
                "point_order", "voxel_point_start")
POST_TABLES = ("kept_ids", "new_offsets", "src_row")


# ------------------------------------------------------------------------------------------------ clustering
def neighbours(coords, scene, cls, valid, radius, K):
    """truncated edge lists of the label-aware ball query, brute force: (query, hit) index pairs with hit among the first K
    points (ascending index) of the query's scene and class with d2 < r * r, d2 = (dx*dx + dy*dy) + dz*dz in float32"""
    coords = np.ascontiguousarray(coords, F)
    r2 = F(radius) * F(radius)
    src, dst = [], []
    ids = np.flatnonzero(valid)
    if ids.size == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    group_key = scene[ids].astype(np.int64) * (int(cls.max()) + 1) + cls[ids].astype(np.int64)
    for key in np.unique(group_key):
        g = ids[group_key == key]  # ascending point index
        pts = coords[g]
        for a in range(0, g.size, 512):
            q = pts[a:a + 512]
            dx = q[:, None, 0] - pts[None, :, 0]
            dy = q[:, None, 1] - pts[None, :, 1]
            dz = q[:, None, 2] - pts[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            hit = d2 < r2
            hit &= np.cumsum(hit, axis=1) <= K  # the first K in ascending point index
            qi, hj = np.nonzero(hit)
            src.append(g[a + qi])
            dst.append(g[hj])
    return np.concatenate(src), np.concatenate(dst)


def components(n, src, dst):
    """union-find over the edges; label of a point = minimum point index of its component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in zip(src.tolist(), dst.tolist()):
        a, b = find(i), find(j)
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    return np.array([find(i) for i in range(n)], np.int64)


def cluster_sets(points, offset_preds, sem_preds, instance_labels, batch_indices, radius, K1, K2):
    """-> (valid [N] bool, labels_A [N], labels_B [N]); labels of invalid points are meaningless"""
    xyz = np.ascontiguousarray(np.asarray(points)[:, :3], F)
    shifted = xyz + np.asarray(offset_preds, F)  # one fp32 add
    assert shifted.dtype == F
    sem = np.asarray(sem_preds).astype(np.int64)
    valid = sem > 0
    if instance_labels is not None:
        valid &= np.asarray(instance_labels) >= 0
    scene = np.asarray(batch_indices).astype(np.int64)
    N = xyz.shape[0]
    la = components(N, *neighbours(xyz, scene, sem, valid, radius, K1))
    lb = components(N, *neighbours(shifted, scene, sem, valid, radius, K2))
    return valid, la, lb


# ------------------------------------------------------------------------------------------------ the per-proposal frame
def frame(pts, fullscale, max_scale, jitter, div="mul"):
    """mean, scale, shift and scaled coordinates of one proposal's points [n, 3] float32 (ascending point order)"""
    full = F(fullscale)
    ra, rb = np.asarray(jitter[0], F).reshape(3), np.asarray(jitter[1], F).reshape(3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        total = np.cumsum(pts, axis=0, dtype=F)[-1]  # ordered fp32 sum, ascending point
        mean = total / F(pts.shape[0])
        centred = pts - mean
        lo = centred.min(0)
        hi = centred.max(0)
        width = hi - lo
        if div == "mul":
            inv_full = F(1) / full
            cells = width * inv_full
        else:
            cells = width / full
        widest = cells.max()
        scale = F(1) / widest
        scale = scale - F(0.01)
        scale = np.minimum(scale, F(max_scale))
        lo_s = lo * scale
        hi_s = hi * scale
        ext = hi_s - lo_s
        room = full - ext
        room_a = np.maximum(room - F(0.001), F(0))
        room_b = np.minimum(room + F(0.001), F(0))
        shift = -lo_s + room_a * ra
        shift = shift + room_b * rb
        scaled = centred * scale
        scaled = scaled + shift
    for a in (mean, scale, shift, scaled):
        assert np.asarray(a).dtype == F
    return mean, scale, shift, scaled


def frame64(pts, fullscale, max_scale, jitter):
    """the frame in float64 (for the distance of a point to its nearest cell face)"""
    p = np.asarray(pts, np.float64)
    ra, rb = np.asarray(jitter[0], np.float64).reshape(3), np.asarray(jitter[1], np.float64).reshape(3)
    full = float(fullscale)
    c = p - p.mean(0)
    lo, hi = c.min(0), c.max(0)
    with np.errstate(divide="ignore"):
        scale = min(1.0 / ((hi - lo) / full).max() - 0.01, float(max_scale))
    ext = hi * scale - lo * scale
    shift = -lo * scale + np.maximum(full - ext - 0.001, 0) * ra + np.minimum(full - ext + 0.001, 0) * rb
    return c * scale + shift


def coarse_rows(voxel_coords, fullscale):
    vc = np.asarray(voxel_coords).reshape(-1, 4)
    half = vc[:, 1:] // 2
    inside = (half < int(fullscale) // 2).all(1)
    rows = np.concatenate([vc[inside, :1], half[inside]], axis=1)
    return int(np.unique(rows, axis=0).shape[0])


# ------------------------------------------------------------------------------------------------ build
def build(points, offset_preds, sem_preds, instance_labels, batch_indices, batch_size, radius, K1, K2, min_points, fullscale,
          max_scale, jitter, div="mul"):
    xyz = np.ascontiguousarray(np.asarray(points)[:, :3], F)
    N = xyz.shape[0]
    sem = np.asarray(sem_preds).astype(np.int64)
    scene = np.asarray(batch_indices).astype(np.int64)
    assert (np.diff(scene) >= 0).all() and (scene >= 0).all() and (scene < batch_size).all()
    valid, la, lb = cluster_sets(points, offset_preds, sem, instance_labels, scene, radius, K1, K2)
    valid_indices = np.flatnonzero(valid).astype(np.int64)
    Q = int(valid_indices.size)
    rank = np.cumsum(valid) - valid  # index among the valid points

    rows_pt, rows_prop, sizes = [], [], []
    member_slot = np.full((2 * N,), -1, np.int32)
    m = 0
    for which, labels in enumerate((la, lb)):
        ids = valid_indices[np.argsort(labels[valid_indices], kind="stable")]  # by label, members ascending
        lab = labels[ids]
        starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]) if ids.size else np.zeros((0,), np.int64)
        ends = np.r_[starts[1:], ids.size]
        for b, e in zip(starts.tolist(), ends.tolist()):
            if e - b < min_points:
                continue
            rows_pt.append(ids[b:e])
            rows_prop.append(np.full((e - b,), len(sizes), np.int64))
            member_slot[which * N + ids[b:e]] = np.arange(m, m + e - b, dtype=np.int32)
            sizes.append(e - b)
            m += e - b
    P, M = len(sizes), m
    if M == 0:
        return None
    point_indices = np.concatenate(rows_pt).astype(np.int64)
    proposal_indices = np.concatenate(rows_prop)
    sizes = np.asarray(sizes, np.int64)
    proposal_offsets = np.r_[0, np.cumsum(sizes)].astype(np.int32)
    pt_xyz = xyz[point_indices]

    scaled = np.zeros((M, 3), F)
    means, scales, shifts = np.zeros((P, 3), F), np.zeros((P,), F), np.zeros((P, 3), F)
    for p in range(P):
        b, e = int(proposal_offsets[p]), int(proposal_offsets[p + 1])
        means[p], scales[p], shifts[p], scaled[b:e] = frame(pt_xyz[b:e], fullscale, max_scale, jitter, div)
    cell = np.floor(scaled)
    kept = ((scaled >= F(0)) & (scaled < F(fullscale))).all(1)
    cell = np.where(kept[:, None], cell, 0).astype(np.int64)
    rows = np.concatenate([proposal_indices[:, None], cell], axis=1)
    voxel_coords, inverse = np.unique(rows[kept], axis=0, return_inverse=True)
    V = int(voxel_coords.shape[0])
    pc_voxel_id = np.full((M,), -1, np.int32)
    pc_voxel_id[kept] = inverse.reshape(-1).astype(np.int32)
    kept_rows = np.flatnonzero(kept)
    order_kept = kept_rows[np.argsort(pc_voxel_id[kept_rows], kind="stable")]
    point_order = np.r_[order_kept, np.flatnonzero(~kept)].astype(np.int32)
    voxel_point_start = np.r_[0, np.cumsum(np.bincount(pc_voxel_id[kept_rows], minlength=V))].astype(np.int32)
    inst = None if instance_labels is None else np.asarray(instance_labels).astype(np.int32)[point_indices]
    return dict(Q=Q, M=M, P=P, V=V, dropped=int((~kept).sum()), coarse=coarse_rows(voxel_coords, fullscale),
                valid_mask=valid, valid_indices=valid_indices, sorted_indices=rank[point_indices].astype(np.int64),
                point_indices=point_indices, proposal_indices=proposal_indices, batch_indices=scene[point_indices].astype(np.int32),
                pt_xyz=pt_xyz, sem_preds=sem[point_indices].astype(np.int32), instance_labels=inst, sizes=sizes,
                proposal_offsets=proposal_offsets, member_slot=member_slot, voxel_coords=voxel_coords.astype(np.int32),
                pc_voxel_id=pc_voxel_id, point_order=point_order, voxel_point_start=voxel_point_start,
                _mean=means, _scale=scales, _shift=shifts, _scaled=scaled, _labels=(la, lb))


# ------------------------------------------------------------------------------------------------ post-processing
def iou32(inter, size_a, size_b):
    """inter / ((|a| + |b|) - inter + 1e-8f) in float32"""
    union = (F(size_a) + F(size_b)) - F(inter)
    return F(inter) / (union + F(1e-8))


def intersections(proposal_offsets, point_indices, ids):
    """exact intersection sizes between the proposals `ids`, from their point lists: {(a, b): n} with a < b"""
    owners, inter = {}, {}
    for p in ids:
        for i in point_indices[proposal_offsets[p]:proposal_offsets[p + 1]].tolist():
            owners.setdefault(i, []).append(p)
    for ps in owners.values():
        for x in range(len(ps)):
            for y in range(x + 1, len(ps)):
                key = (min(ps[x], ps[y]), max(ps[x], ps[y]))
                inter[key] = inter.get(key, 0) + 1
    return inter


def postprocess(score, sizes, proposal_offsets, point_indices, proposal_indices, score_thr, min_points, iou_thr, live=None):
    """score filter (strict), greedy NMS in (-score, id) order on exact point-set IoU (strict), compaction tables.
    `live`: only the first `live` proposals exist (the rows behind them hold anything)."""
    score = np.asarray(score, F)
    P = score.shape[0] if live is None else int(live)
    sizes = np.asarray(sizes).astype(np.int64)
    proposal_offsets = np.asarray(proposal_offsets).astype(np.int64)
    point_indices = np.asarray(point_indices)
    thr = F(score_thr)
    survivors = [p for p in range(P) if score[p] > thr and sizes[p] > min_points]
    inter = intersections(proposal_offsets, point_indices, survivors)
    nbrs = {p: [] for p in survivors}
    for (a, b), n in inter.items():
        if iou32(n, sizes[a], sizes[b]) > F(iou_thr):
            nbrs[a].append(b)
            nbrs[b].append(a)
    kept = set()
    for p in sorted(survivors, key=lambda q: (-float(score[q]), q)):
        if not any(q in kept for q in nbrs[p]):
            kept.add(p)
    kept_ids = np.array(sorted(kept), np.int32)
    new_offsets = np.r_[0, np.cumsum(sizes[kept_ids])].astype(np.int32)
    src = [np.arange(proposal_offsets[p], proposal_offsets[p] + sizes[p]) for p in kept_ids.tolist()]
    src_row = np.concatenate(src).astype(np.int64) if src else np.zeros((0,), np.int64)
    return dict(kept_ids=kept_ids, new_offsets=new_offsets, src_row=src_row,
                _max_neighbours=max([len(v) for v in nbrs.values()], default=0))


def sharers(proposal_offsets, point_indices, proposal_indices, member_slot, p):
    """distinct proposals (filtered or not) that share a point with proposal p: what one wave's table has to hold"""
    N = member_slot.shape[0] // 2
    out = set()
    for r in range(int(proposal_offsets[p]), int(proposal_offsets[p + 1])):
        i = int(point_indices[r])
        s0, s1 = int(member_slot[i]), int(member_slot[N + i])
        r2 = s1 if s0 == r else s0
        if r2 >= 0:
            out.add(int(proposal_indices[r2]))
    return out


# ------------------------------------------------------------------------------------------------ voxel means
def voxel_mean64(feats, point_indices, point_order, voxel_point_start):
    """[V, C] float64 mean of feats[point_indices[m]] over every voxel's points, and the same of |feats|"""
    x = np.asarray(feats, np.float64)
    V = voxel_point_start.shape[0] - 1
    out, mag = np.zeros((V, x.shape[1])), np.zeros((V, x.shape[1]))
    for v in range(V):
        rows = point_indices[point_order[voxel_point_start[v]:voxel_point_start[v + 1]]]
        out[v] = x[rows].mean(0)
        mag[v] = np.abs(x[rows]).mean(0)
    return out, mag


def voxel_mean_bwd64(dout, member_slot, pc_voxel_id, voxel_point_start, N):
    """[N, C] float64 gradient of the voxel mean w.r.t. the point features, and the sum of the terms' magnitudes"""
    g = np.asarray(dout, np.float64)
    cnt = np.diff(voxel_point_start).astype(np.float64)
    out, mag = np.zeros((N, g.shape[1])), np.zeros((N, g.shape[1]))
    for which in range(2):
        m = member_slot[which * N:(which + 1) * N]
        has = m >= 0
        v = np.where(has, pc_voxel_id[np.maximum(m, 0)], -1)
        has &= v >= 0
        term = g[v[has]] / cnt[v[has]][:, None]
        out[has] += term
        mag[has] += np.abs(term)
    return out, mag


# ------------------------------------------------------------------------------------------------ comparison
def _same(name, got, want):
    if isinstance(want, (int, np.integer)) and not isinstance(want, (bool, np.bool_)):
        if int(got) != int(want):
            raise AssertionError(f"{name}: {int(got)} != {int(want)}")
        return
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError(f"{name}: shape {got.shape} != {want.shape}")
    if want.dtype.kind == "f":
        diff = got.view(np.uint32) != want.astype(F).view(np.uint32) if got.dtype == F else got != want  # bits: no tolerance
    else:
        diff = got != want
    if diff.any():
        width = int(np.prod(want.shape[1:])) if want.ndim > 1 else 1
        bad = np.flatnonzero(diff.reshape(-1))
        raise AssertionError(f"{name}: {bad.size} of {got.size} entries differ, first in row {int(bad[0]) // width} "
                             f"(flat index {int(bad[0])}): {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}")


def assert_tables_equal(got, want):
    """every table and count of `want` (keys not starting with "_") equals `got`'s; the error names the first differing table
    and row.  None (no proposal / a designed overflow) only equals None."""
    if want is None or got is None:
        if got is not want:
            raise AssertionError(f"result: {'None' if got is None else 'tables'} != {'None' if want is None else 'tables'}")
        return
    for name in want:
        if name.startswith("_"):
            continue
        if name not in got:
            raise AssertionError(f"{name}: missing")
        if want[name] is None or got[name] is None:
            if got[name] is not want[name]:
                raise AssertionError(f"{name}: one side is None")
            continue
        _same(name, got[name], want[name])
