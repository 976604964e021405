"""Edge inputs for the grouping / PointNet++ operators, each with an INDEPENDENT numpy statement of the result.

Shared by tests/test_oracle_pins_edges.py (oracle == these references, no GPU) and tests/test_gpu_op_edges.py (HIP kernels ==
oracle on the very same inputs), so that oracle equality on the GPU means something: the oracle functions of family F are
line-by-line twins of the kernels, the references here are not (argsort, fancy indexing, scipy, per-segment loops).
Every case is built once per process (lru_cache) and must be treated as read-only."""
import functools

import numpy as np

f32, i32 = np.float32, np.int32


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def dist2(a, b):
    """[b, n, m] float32 (dx*dx + dy*dy) + dz*dz between a [b, n, 3] and b [b, m, 3] (no contraction: numpy does not fuse)"""
    d = a[:, :, None, :].astype(f32) - b[:, None, :, :].astype(f32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ------------------------------------------------------------------------------------------------ three_nn / knn
KNN_SHAPES = [(70, 1, 3), (70, 2, 5), (300, 257, 5), (65, 300, 200), (5, 7, 200)]  # (n unknown, m known, k)


@functools.lru_cache(maxsize=None)
def knn_case(n, m, k):
    """lattice points (many duplicates, exact distance ties) -> (unknown, known, dist [b, n, k], idx [b, n, k],
    dist3 [b, n, 3], idx3 [b, n, 3]): neighbours ranked by a STABLE argsort (the first index wins a tie), slots past
    min(k, m) hold index 0 and distance inf"""
    rng = np.random.default_rng(1000 * n + m)
    unknown = (rng.integers(0, 4, (2, n, 3)) * 0.25).astype(f32)
    known = (rng.integers(0, 4, (2, m, 3)) * 0.25).astype(f32)
    d2 = dist2(unknown, known)
    order = np.argsort(d2, axis=-1, kind="stable")

    def ranked(kk):
        live = min(kk, m)
        idx = np.zeros((2, n, kk), i32)
        dist = np.full((2, n, kk), np.inf, f32)
        idx[..., :live] = order[..., :live]
        dist[..., :live] = np.take_along_axis(d2, order[..., :live], -1)
        return dist, idx
    dist, idx = ranked(k)
    dist3, idx3 = ranked(3)
    return _frozen(unknown, known, dist, idx, dist3, idx3)


# ------------------------------------------------------------------------------------------------ pn2 ball query
PN2_BALL_SHAPES = [(1, 1, 4), (255, 3, 8), (256, 257, 1), (257, 256, 64), (700, 300, 16)]  # (n, m, nsample)
PN2_BALL_RADIUS = 0.15


@functools.lru_cache(maxsize=None)
def pn2_ball_case(n, m, nsample):
    """points on a 0.1 lattice (radius 0.15 takes the 19 cells at squared distance <= 0.02; 0.03 is out - both far from
    0.0225 in float32), every fourth query far outside the cloud -> (xyz, new_xyz, idx [b, m, nsample]): hits in ascending
    index truncated at nsample, a row with hits padded with its first hit, a row without any all zero"""
    rng = np.random.default_rng(77 * n + m)
    xyz = (rng.integers(0, 6, (2, n, 3)) * 0.1).astype(f32)
    pick = rng.integers(0, n, (2, m))
    new_xyz = np.take_along_axis(xyz, pick[:, :, None], 1).copy()
    new_xyz[:, 3::4] += f32(5.0)
    hit = dist2(new_xyz, xyz) < f32(PN2_BALL_RADIUS) * f32(PN2_BALL_RADIUS)
    idx = np.zeros((2, m, nsample), i32)
    for b in range(2):
        for j in range(m):
            h = np.flatnonzero(hit[b, j])[:nsample]
            if h.size:
                idx[b, j, :] = h[0]
                idx[b, j, :h.size] = h
    return _frozen(xyz, new_xyz, idx)


# ------------------------------------------------------------------------------------------------ FPS
FPS_SIZES = [1, 2, 3, 5, 63, 64, 65, 513, 1023, 1024, 1025, 2049, 3000]


def fps_closed_form(xyz, m):
    """furthest point sampling in closed form: start at 0; the next sample has the highest running distance, ties go to
    the smallest bit-reversed (k mod B), then to the smallest k, B = min(1024, 2 ** floor(log2 n))"""
    b, n, _ = xyz.shape
    bits = min(10, n.bit_length() - 1)
    B = 1 << bits
    t = np.arange(n) % B
    rev = np.zeros(n, np.int64)
    for s in range(bits):
        rev |= ((t >> s) & 1) << (bits - 1 - s)
    out = np.zeros((b, m), i32)
    for bs in range(b):
        run = np.full(n, 1e10, f32)
        old = 0
        for j in range(1, m):
            d = xyz[bs] - xyz[bs, old]
            run = np.minimum(run, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            cand = np.flatnonzero(run == run.max())
            old = int(cand[np.lexsort((cand, rev[cand]))[0]])
            out[bs, j] = old
    return out


@functools.lru_cache(maxsize=None)
def fps_case(n):
    """integer lattice of 27 cells (ties everywhere); m = min(n + 3, 48): m > n forces repeated picks"""
    rng = np.random.default_rng(n)
    xyz = rng.integers(0, 3, (2, n, 3)).astype(f32)
    m = min(n + 3, 48)
    return _frozen(xyz, fps_closed_form(xyz, m)) + (m,)


# ------------------------------------------------------------------------------------------------ CCL
CCL_CASES = ["permuted_path", "star_hub_last", "two_paths_bridge_junk", "no_edges"]


def _csr(Q, rows):
    """rows: list of target lists per vertex -> (begin_end [2Q] i32, edges i32)"""
    cnt = np.array([len(r) for r in rows], np.int64)
    begin = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if Q else np.zeros(0, np.int64)
    be = np.stack([begin, begin + cnt], 1).reshape(-1).astype(i32)
    edges = np.array([u for r in rows for u in r], i32)
    return be, edges


@functools.lru_cache(maxsize=None)
def ccl_case(name):
    """-> (begin_end, edges, labels, compact): labels = smallest vertex of the component (scipy connected_components over
    the valid edges, undirected), compact = np.unique(labels, return_inverse)"""
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    rng = np.random.default_rng(CCL_CASES.index(name))
    if name == "permuted_path":  # every edge listed on one side only: vertex perm[i] names perm[i + 1]
        Q = 2500
        perm = rng.permutation(Q)
        rows = [[] for _ in range(Q)]
        for a, b in zip(perm[:-1], perm[1:]):
            rows[a].append(int(b))
    elif name == "star_hub_last":  # 2499 edges in the single row of the highest vertex
        Q = 2500
        rows = [[] for _ in range(Q)]
        rows[Q - 1] = [int(v) for v in rng.permutation(Q - 1)]
    elif name == "two_paths_bridge_junk":
        Q = 2100
        perm = rng.permutation(Q)
        rows = [[] for _ in range(Q)]
        for path in (perm[:1000], perm[1000:2000]):  # perm[2000:] stay isolated
            for a, b in zip(path[:-1], path[1:]):
                rows[a].append(int(b))
        rows[perm[1500]].append(int(perm[500]))  # one-sided bridge between the two paths
        for v in rng.choice(Q, 300, replace=False):  # entries outside [0, Q) are ignored
            rows[v].insert(int(rng.integers(0, len(rows[v]) + 1)), int(rng.choice([-1, Q, Q + 5, 2 ** 31 - 1])))
    else:
        Q = 1025
        rows = [[] for _ in range(Q)]
    be, edges = _csr(Q, rows)
    src = np.repeat(np.arange(Q), [len(r) for r in rows])
    ok = (edges >= 0) & (edges < Q)
    graph = sp.coo_matrix((np.ones(int(ok.sum())), (src[ok], edges[ok])), shape=(Q, Q))
    _, comp = csgraph.connected_components(graph, directed=False)
    first = np.full(comp.max() + 1, Q)
    np.minimum.at(first, comp, np.arange(Q))
    labels = first[comp].astype(i32)
    compact = np.unique(labels, return_inverse=True)[1].astype(i32)
    return _frozen(be, edges, labels, compact)


# ------------------------------------------------------------------------------------------------ NMS
NMS_SIZES = [1, 63, 64, 65, 129]
NMS_KINDS = ["asymmetric", "at_threshold", "chain", "chain_transposed", "all_overlap", "no_overlap"]
NMS_THR = 0.3


def nms_loop(ious, scores, thr):
    """the plain greedy loop of tests/test_oracle_pins.py: ROW = the kept proposal, strict >"""
    P = scores.shape[0]
    order = np.argsort(-scores, kind="stable")
    keep, dead = [], np.zeros(P, bool)
    for a in order:
        if dead[a]:
            continue
        keep.append(int(a))
        dead |= ious[a] > f32(thr)
        dead[a] = True
    return np.array(keep, np.int64)


@functools.lru_cache(maxsize=None)
def nms_case(P, kind):
    rng = np.random.default_rng(10 * P + NMS_KINDS.index(kind))
    scores = rng.uniform(size=P).astype(f32)
    if P > 20:
        scores[5] = scores[17]  # a score tie: the lower index first
    order = np.argsort(-scores, kind="stable")
    ious = np.zeros((P, P), f32)
    if kind == "asymmetric":  # ious[i, j] != ious[j, i]: only the row of the kept proposal counts
        ious = (rng.uniform(size=(P, P)) * (rng.uniform(size=(P, P)) < 0.1)).astype(f32)
    elif kind == "at_threshold":  # exactly the threshold everywhere: strict > suppresses nothing
        ious[:] = f32(NMS_THR)
    elif kind == "chain":  # a -> b -> c ...: b is suppressed, so c survives (every other proposal is kept)
        ious[order[:-1], order[1:]] = 0.9
    elif kind == "chain_transposed":  # the same entries on the other side: the lower-scored row never suppresses upwards
        ious[order[1:], order[:-1]] = 0.9
    elif kind == "all_overlap":
        ious[:] = 0.9
    keep = nms_loop(ious, scores, NMS_THR)
    want = {"at_threshold": P, "chain": (P + 1) // 2, "chain_transposed": P, "all_overlap": 1, "no_overlap": P}
    assert kind == "asymmetric" or len(keep) == want[kind]
    return _frozen(ious, scores, keep)


# ------------------------------------------------------------------------------------------------ segmented ops
SEG_CHANNELS = [1, 3, 48, 100, 256]
SEG_SIZES = [0, 1, 700, 12, 0, 40, 9, 0]  # empty first / middle / last, one row, 700 rows


@functools.lru_cache(maxsize=None)
def segment_case(C):
    """-> (values [M, C], begin, end, {mode: reduced}, pooled, argmax): per-segment numpy loops; sums run in row order in
    float32; an empty segment gives 0 (and argmax -1); the first occurrence of the maximum wins"""
    rng = np.random.default_rng(C)
    offs = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(i32)
    begin, end = offs[:-1].copy(), offs[1:].copy()
    M = int(offs[-1])
    vals = rng.normal(size=(M, C)).astype(f32)
    vals[begin[3]:end[3]] = vals[begin[3]]                   # a segment of one repeated row
    vals[begin[5] + 10:begin[5] + 20] = vals[begin[5] + 10]  # repeated rows inside a segment
    vals[begin[5] + 30] = vals[begin[5]:end[5]].max(0)       # a late copy of every channel's maximum
    vals[begin[6]:end[6]] = -np.inf                          # a segment made entirely of -inf
    P = len(SEG_SIZES)
    red = {mode: np.zeros((P, C), f32) for mode in ("sum", "min", "max")}
    pooled, arg = np.zeros((P, C), f32), np.full((P, C), -1, i32)
    for p in range(P):
        seg = vals[begin[p]:end[p]]
        if seg.shape[0] == 0:
            continue
        acc = seg[0].copy()
        for r in range(1, seg.shape[0]):
            acc = acc + seg[r]
        red["sum"][p], red["min"][p], red["max"][p] = acc, seg.min(0), seg.max(0)
        pooled[p], arg[p] = seg.max(0), begin[p] + np.argmax(seg, 0)
    return _frozen(vals, begin, end) + (red,) + _frozen(pooled, arg)


# ------------------------------------------------------------------------------------------------ instance IoU
IOU_INSTANCES = [1, 129, 300]


@functools.lru_cache(maxsize=None)
def iou_case(I):
    """-> (offsets, instance_labels, batch_indices, num_points_per_instance, ious): one-hot product; labels -1 and >= I count
    for nothing; an empty proposal (batch 0 by convention) and one of more than 128 points"""
    rng = np.random.default_rng(I)
    B, P = 3, 40
    sizes = rng.integers(1, 60, P)
    sizes[7], sizes[11] = 0, 200
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(i32)
    M = int(offs[-1])
    pb = np.sort(rng.integers(0, B, P)).astype(i32)
    bi = np.repeat(pb, sizes).astype(i32)
    il = rng.integers(-1, I + 2, M).astype(i32)
    npi = rng.integers(1, 300, (B, I)).astype(i32)
    npi[:, -1] = 0
    ok = (il >= 0) & (il < I)
    onehot = np.zeros((M, I), np.int64)
    onehot[np.arange(M)[ok], il[ok]] = 1
    member = np.zeros((P, M), np.int64)
    member[np.repeat(np.arange(P), sizes), np.arange(M)] = 1
    inter = member @ onehot
    pb_eff = np.where(sizes > 0, pb, 0)
    union = sizes[:, None] + npi[pb_eff] - inter
    want = np.where((npi[pb_eff] > 0) & (union > 0), inter.astype(f32) / np.maximum(union, 1).astype(f32), f32(0)).astype(f32)
    return _frozen(offs, il, bi, npi, want)


# ------------------------------------------------------------------------------------------------ group / gather / interpolate
@functools.lru_cache(maxsize=None)
def gather_case():
    """-> dict: forward results by numpy fancy indexing; three_interpolate = (w0 p0 + w1 p1) + w2 p2 in float32"""
    rng = np.random.default_rng(31)
    b, c, n, npts, ns, m = 2, 5, 300, 37, 8, 257
    feats = rng.normal(size=(b, c, n)).astype(f32)
    gidx = rng.integers(0, n, (b, npts, ns)).astype(i32)
    gidx[0, 0] = n - 1
    sidx = rng.integers(0, n, (b, m)).astype(i32)
    grouped = np.stack([feats[i][:, gidx[i]] for i in range(b)])       # [b, c, npts, ns]
    gathered = np.stack([feats[i][:, sidx[i]] for i in range(b)])      # [b, c, m]
    known = rng.normal(size=(b, c, m)).astype(f32)
    idx3 = rng.integers(0, m, (b, n, 3)).astype(i32)
    idx3[1, :10] = idx3[1, :10, :1]  # the same neighbour three times
    w = rng.uniform(size=(b, n, 3)).astype(f32)
    p = np.stack([known[i][:, idx3[i]] for i in range(b)])             # [b, c, n, 3]
    interp = (w[:, None, :, 0] * p[..., 0] + w[:, None, :, 1] * p[..., 1]) + w[:, None, :, 2] * p[..., 2]
    out = dict(feats=feats, gidx=gidx, sidx=sidx, grouped=grouped, gathered=gathered, known=known, idx3=idx3, w=w,
               interp=interp.astype(f32))
    _frozen(*out.values())
    return out


# ------------------------------------------------------------------------------------------------ gradient kernels (atomics)
GRAD_KINDS = ["random", "contended", "sparse"]


def _grad_idx(rng, kind, shape, n):
    if kind == "contended":  # every index names the same point
        return np.full(shape, 5, i32)
    if kind == "sparse":     # most points receive nothing
        return rng.choice(np.array([0, 1, n // 2, n - 1], i32), size=shape).astype(i32)
    return rng.integers(0, n, shape).astype(i32)


def _scatter64(shape, where, addends):
    """float64 sums of the float32 addends, the sum of their magnitudes and their number, per destination element"""
    s, a, k = np.zeros(shape, np.float64), np.zeros(shape, np.float64), np.zeros(shape, np.int64)
    np.add.at(s, where, addends.astype(np.float64))
    np.add.at(a, where, np.abs(addends.astype(np.float64)))
    np.add.at(k, where, 1)
    return s, a, k


@functools.lru_cache(maxsize=None)
def grad_case(op, kind):
    """-> (kernel arguments as a tuple, ref64, bound): the order of an atomic sum is not fixed, so the check is elementwise
    against a float64 accumulation of the same float32 addends with the bound (k + 1) 2^-24 sum|addend|, k = the number of
    addends landing on the element (k - 1 roundings of at most 2^-24 of a partial sum each, partial sums <= sum|addend|;
    no addend at all: exactly zero).  `contended` puts 256 x 8 = 2048 addends on one element per (batch, channel)."""
    rng = np.random.default_rng(100 * GRAD_KINDS.index(kind) + len(op))
    b, c, n = 2, 3, 64
    bb, cc = np.arange(b)[:, None, None], np.arange(c)[None, :, None]
    if op == "group_points":
        npts, ns = 256, 8
        idx = _grad_idx(rng, kind, (b, npts, ns), n)
        g = rng.normal(size=(b, c, npts, ns)).astype(f32)
        where = (bb[..., None], cc[..., None], idx[:, None, :, :])
        s, a, k = _scatter64((b, c, n), tuple(np.broadcast_arrays(*where)), g)
        args = (g, idx, n)
    elif op == "gather_points":
        m = 2048
        idx = _grad_idx(rng, kind, (b, m), n)
        g = rng.normal(size=(b, c, m)).astype(f32)
        s, a, k = _scatter64((b, c, n), tuple(np.broadcast_arrays(bb, cc, idx[:, None, :])), g)
        args = (g, idx, n)
    else:
        assert op == "three_interpolate"
        npt = 2048  # unknown points; the destination has n = 64 known points
        idx = _grad_idx(rng, kind, (b, npt, 3), n)
        if kind == "contended":
            idx = idx.copy()
            idx[..., 1], idx[..., 2] = 1, 2  # 2048 addends on each of the points 5, 1 and 2
        g = rng.normal(size=(b, c, npt)).astype(f32)
        w = rng.uniform(size=(b, npt, 3)).astype(f32)
        addends = g[..., None] * w[:, None, :, :]  # float32 products [b, c, npt, 3]
        where = tuple(np.broadcast_arrays(bb[..., None], cc[..., None], idx[:, None, :, :]))
        s, a, k = _scatter64((b, c, n), where, addends)
        args = (g, idx, w, n)
    bound = (k + 1) * 2.0 ** -24 * a
    if kind == "contended":
        assert k.max() == 2048
    if kind == "sparse":
        assert (k == 0).mean() > 0.9
    return (_frozen(*args), s, bound)
