"""Deterministic small inputs for csrc/proposals.hip and csrc/postprocess.hip, each named for the seam it sits on.
numpy only.  tests/test_proposal_cases_cpu.py recomputes the property every case is named for; tests/test_gpu_proposal_seams.py
runs them through the kernels.

Build cases: cluster points sit on a planar lattice of pitch 0.6 r, perturbed by at most 3 % of the pitch per axis, so lattice
neighbours (0.6 r, 0.85 r) are hits and everything else (>= 1.2 r) is not, with every same-scene same-class distance at least
1 % away from r in both cluster sets (asserted on the CPU, not assumed).  Clusters are placed 6 r apart.  r = 2^-5, so the one
deliberate exception (`exact_radius_pair`) can put pairs at d2 == r * r exactly.

Post-processing cases are built directly from two partitions of N points (set A's proposals first, then set B's)."""
import functools

import numpy as np

F = np.float32
RADIUS = 0.03125  # 2^-5: r * r is exact in float32
PITCH = 0.6 * RADIUS
GAP = 6 * RADIUS
JITTER = (np.array([0.3, 0.6, 0.1], F), np.array([0.5, 0.2, 0.9], F))
MAX_SCALE = 50.0
K1, K2 = 16, 12  # above the 9 hits a lattice point can have: no truncation unless a case asks for it


def _frozen(a):
    a.setflags(write=False)
    return a


class Scene:
    """accumulates clusters; every cluster gets its own stretch of the x axis"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.x = 0.0
        self.xyz, self.off, self.sem, self.inst, self.scene = [], [], [], [], []

    def block(self, n, width, cls=1, scene=0, inst=0, flat=False, advance=True):
        """n lattice points, `width` per column-major run, perturbed; -> slice of their rows"""
        k = np.arange(n)
        p = np.stack([self.x + (k // width) * PITCH, (k % width) * PITCH, np.zeros(n)], axis=1)
        noise = self.rng.uniform(-0.03 * PITCH, 0.03 * PITCH, size=p.shape)
        if flat:
            noise[:, 2] = 0.0
        return self.raw(p + noise, cls, scene, inst, advance, extent=((n - 1) // width + 1) * PITCH)

    def raw(self, p, cls=1, scene=0, inst=0, advance=True, extent=0.0):
        n = p.shape[0]
        first = sum(a.shape[0] for a in self.xyz)
        self.xyz.append(np.asarray(p, np.float64).astype(F))
        self.off.append(np.zeros((n, 3), F))
        self.sem.append(np.full((n,), cls, np.int64))
        self.inst.append(np.full((n,), inst, np.int32))
        self.scene.append(np.full((n,), scene, np.int32))
        if advance:
            self.x += extent + GAP
        return slice(first, first + n)

    def case(self, batch_size=None, with_inst=True, min_points=5, fullscale=28, K1=K1, K2=K2, offsets=None, **extra):
        xyz, off = np.concatenate(self.xyz), np.concatenate(self.off)
        if offsets is not None:
            for rows, d in offsets:
                off[rows] = np.asarray(d, F)
        scene = np.concatenate(self.scene)
        assert (np.diff(scene) >= 0).all(), "scenes in order"
        B = int(batch_size if batch_size is not None else scene.max() + 1)
        return dict(points=_frozen(xyz), offset_preds=_frozen(off), sem_preds=_frozen(np.concatenate(self.sem)),
                    instance_labels=_frozen(np.concatenate(self.inst)) if with_inst else None, batch_indices=_frozen(scene),
                    batch_size=B, radius=RADIUS, K1=K1, K2=K2, min_points=min_points, fullscale=fullscale, max_scale=MAX_SCALE,
                    jitter=JITTER, **extra)


def build_args(case):
    """the arguments of proposal_ref.build / hip_ops.proposals_build, in order"""
    return tuple(case[k] for k in ("points", "offset_preds", "sem_preds", "instance_labels", "batch_indices", "batch_size", "radius",
                                   "K1", "K2", "min_points", "fullscale", "max_scale", "jitter"))


UP = np.array([0.0, 0.0, 10 * RADIUS])  # a rigid move out of the lattice plane: a set-B cluster of its own


def min_points_edges():
    s = Scene(1)
    for n in (4, 5, 6):  # set A (and, unmoved, set B): min_points - 1, min_points, min_points + 1
        s.block(n, 2)
    moved = []
    for head in (4, 5, 6):  # set B: heads of 4, 5, 6 points stay, the tails of 5 leave
        rows = s.block(head + 5, 1)
        moved.append((slice(rows.start + head, rows.stop), UP))
    return s.case(min_points=5, offsets=moved, sizes_A=[5, 6, 9, 10, 11], sizes_B=[5, 6, 5, 5, 5, 6, 5])


def merge_and_split():
    s = Scene(2)
    a = s.block(6, 2)
    b = s.block(6, 2)
    c = s.block(12, 2)
    step = float(s.xyz[1][0, 0] - s.xyz[0][0, 0])
    pull = np.array([-(round(step / PITCH) - 3) * PITCH, 0.0, 0.0])  # b continues a's lattice: one cluster of 12 in set B
    return s.case(offsets=[(b, pull), (slice(c.start + 6, c.stop), UP)], sizes_A=[6, 6, 12], sizes_B=[12, 6, 6], rows=(a, b, c))


def collapsed_blob():
    k2 = 84
    n = 3 * k2 + 5  # 257: more than K2 and more than the ball query's 256-entry hit list
    s = Scene(3)
    blob = s.block(n, 16)
    other_class = s.block(7, 2, cls=2)
    other_cluster = s.block(9, 3)
    xyz = np.concatenate(s.xyz).astype(np.float64)
    target = xyz[blob][0]
    off = [(blob, target - xyz[blob]), (other_class, target - xyz[other_class])]
    return s.case(K2=k2, offsets=off, blob=n, sizes_A=[n, 7, 9], sizes_B=[n, 7, 9])


def same_place_other_class():
    s = Scene(4)
    a = s.block(8, 2, cls=1)
    s.raw(s.xyz[0].copy(), cls=2)
    return s.case(sizes_A=[8, 8], sizes_B=[8, 8], rows=a)


def same_place_other_scene():
    s = Scene(5)
    a = s.block(8, 2, scene=0)
    s.raw(s.xyz[0].copy(), scene=1)
    return s.case(sizes_A=[8, 8], sizes_B=[8, 8], rows=a)


def _invalid_mix(with_inst):
    s = Scene(6)
    for n in (12, 9, 7):
        s.block(n, 3)
    c = s.case(with_inst=with_inst)
    sem, inst = c["sem_preds"].copy(), np.concatenate(s.inst)
    sem[[1, 13, 14, 22]] = 0
    inst[[4, 5, 6, 7, 23]] = -1  # (with labels: rows 4..7 cut the first cluster's lattice in two)
    inst[[0, 2]] = 7
    c["sem_preds"] = _frozen(sem)
    c["instance_labels"] = _frozen(inst) if with_inst else None
    return c


def scenes():
    s = Scene(7)
    s.block(9, 3, scene=0)
    s.block(6, 2, scene=1, cls=0)  # a scene whose points are all invalid, between two that have valid ones
    s.block(7, 2, scene=2)
    s.block(5, 1, scene=2, cls=3)
    s.block(8, 2, scene=4)  # (no point carries scene 3; scene 5, the last, is empty)
    return s.case(batch_size=6, sizes_A=[9, 7, 5, 8], sizes_B=[9, 7, 5, 8])


def scenes_b4():
    s = Scene(8)
    s.block(9, 3, scene=0)
    s.block(11, 2, scene=1, inst=-1)
    s.block(7, 2, scene=2)
    s.block(6, 3, scene=3)
    return s.case(batch_size=4, sizes_A=[9, 7, 6], sizes_B=[9, 7, 6])


def _n_points(n, valid=True):
    s = Scene(100 + n)
    left, sizes = n, []
    while left > 0:
        m = min(left, 37)
        s.block(m, 4, cls=1 if valid else 0)
        sizes.append(m)
        left -= m
    return s.case(min_points=1, sizes_A=sizes if valid else [], sizes_B=sizes if valid else [])


def one_giant():
    s = Scene(9)
    s.block(600, 20)
    return s.case(sizes_A=[600], sizes_B=[600])


SEAM_SIZES = (63, 64, 65, 128, 129, 257, 513)


def _seam_sizes(fullscale=28):
    s = Scene(10)
    for n in SEAM_SIZES:
        s.block(n, 7)
    return s.case(fullscale=fullscale, sizes_A=list(SEAM_SIZES), sizes_B=list(SEAM_SIZES))


def proposals_1100():
    s = Scene(11)
    pairs = 550
    k = np.arange(pairs)
    first = np.stack([(k // 25) * GAP, (k % 25) * GAP, np.zeros(pairs)], axis=1)
    p = np.repeat(first, 2, axis=0)
    p[1::2, 1] += PITCH
    p += s.rng.uniform(-0.03 * PITCH, 0.03 * PITCH, size=p.shape)
    s.raw(p)
    return s.case(min_points=2, sizes_A=[2] * pairs, sizes_B=[2] * pairs)


def degenerate_extent():
    s = Scene(12)
    s.raw(np.tile(np.array([[0.3, 0.7, 0.2]]), (6, 1)), extent=0.0)  # coincident: extent 0 on every axis, 1 / 0, scale = max_scale
    s.x = 1.0
    s.block(12, 3, flat=True)  # z == 0 exactly: flat along an axis
    s.block(5, 1, flat=True)   # flat along two axes but for the perturbation of x
    return s.case(sizes_A=[6, 12, 5], sizes_B=[6, 12, 5])


def strided(contiguous=False):
    c = _seam_sizes()
    wide = np.zeros((c["points"].shape[0], 6), F)
    wide[:, :3] = c["points"]
    wide[:, 3:] = 7.5  # colours: never read
    c["points"] = np.ascontiguousarray(wide[:, :3]) if contiguous else wide[:, :3]
    assert c["points"].flags.c_contiguous == contiguous
    return c


def exact_radius_pair():
    """two clusters of three points on exactly representable coordinates, half a radius apart; the last point of the first and
    the first of the second are exactly one radius apart (d2 == r * r: not a hit), and so are the ends of each cluster"""
    s = Scene(13)
    h = RADIUS / 2
    one = np.array([[1 - 2 * h, 1, 1], [1 - h, 1, 1], [1, 1, 1]])
    two = np.array([[1 + RADIUS, 1, 1], [1 + RADIUS + h, 1, 1], [1 + RADIUS + 2 * h, 1, 1]])
    s.raw(one)
    s.raw(two)
    return s.case(min_points=2, sizes_A=[3, 3], sizes_B=[3, 3], exact_pairs=True)


def all_invalid():
    s = Scene(14)
    s.block(9, 3, cls=0)
    s.block(9, 3, inst=-1)
    return s.case(sizes_A=[], sizes_B=[])


BUILD_CASES = {
    "min_points_edges": min_points_edges,
    "merge_and_split": merge_and_split,
    "collapsed_blob": collapsed_blob,
    "same_place_other_class": same_place_other_class,
    "same_place_other_scene": same_place_other_scene,
    "invalid_mix": functools.partial(_invalid_mix, True),
    "invalid_mix_no_labels": functools.partial(_invalid_mix, False),
    "scenes": scenes,
    "scenes_b4": scenes_b4,
    "n_1_valid": functools.partial(_n_points, 1),
    "n_1_invalid": functools.partial(_n_points, 1, False),
    "n_255": functools.partial(_n_points, 255),
    "n_256": functools.partial(_n_points, 256),
    "n_257": functools.partial(_n_points, 257),
    "all_invalid": all_invalid,
    "one_giant": one_giant,
    "sizes_63_64_65_128_129_257_513": _seam_sizes,
    "proposals_1100": proposals_1100,
    "degenerate_extent": degenerate_extent,
    "strided": strided,
    "strided_contiguous": functools.partial(strided, True),
    "exact_radius_pair": exact_radius_pair,
    "fullscale_7": functools.partial(_seam_sizes, 7),
    "fullscale_28": functools.partial(_seam_sizes, 28),
    "fullscale_30": functools.partial(_seam_sizes, 30),
    "fullscale_31": functools.partial(_seam_sizes, 31),
    "fullscale_32": functools.partial(_seam_sizes, 32),
}
NONE_CASES = ("n_1_invalid", "all_invalid")
BUILD_CASES = {k: functools.lru_cache(maxsize=None)(v) for k, v in BUILD_CASES.items()}
REVOX_MAX_CELLS = 32768  # kRevoxMaxCells: (fullscale + 1)^3 cells up to this take the sort-free re-voxeliser


# ------------------------------------------------------------------------------------------------ post-processing
def tables(part_a, part_b, n_points):
    """the proposal tables of two partitions (lists of ascending point lists; a point in at most one list of each)"""
    sizes = [len(p) for p in part_a] + [len(p) for p in part_b]
    member_slot = np.full((2 * n_points,), -1, np.int32)
    point_indices, proposal_indices, m = [], [], 0
    for which, part in enumerate((part_a, part_b)):
        for pts in part:
            pts = np.asarray(pts, np.int64)
            assert pts.size and (np.diff(pts) > 0).all() and pts[0] >= 0 and pts[-1] < n_points
            assert (member_slot[which * n_points + pts] == -1).all(), "a point sits in one proposal of a set"
            member_slot[which * n_points + pts] = np.arange(m, m + pts.size, dtype=np.int32)
            point_indices.append(pts)
            proposal_indices.append(np.full((pts.size,), len(proposal_indices), np.int64))
            m += pts.size
    return dict(sizes=np.asarray(sizes, np.int64), proposal_offsets=np.r_[0, np.cumsum(sizes)].astype(np.int32),
                point_indices=np.concatenate(point_indices), proposal_indices=np.concatenate(proposal_indices),
                member_slot=member_slot, N=n_points)


def _post(part_a, part_b, n_points, score, score_thr=0.09, min_points=1, iou_thr=0.3, expect="equal", **extra):
    t = tables(part_a, part_b, n_points)
    score = np.asarray(score, F)
    assert score.shape == t["sizes"].shape
    return dict(t, score=score, score_thr=float(F(score_thr)), min_points=int(min_points), iou_thr=float(F(iou_thr)), live=None,
                expect=expect, **extra)


def _seg(first, n):
    return list(range(first, first + n))


def strict_score():
    thr = F(0.09)
    score = [thr, np.nextafter(thr, F(1)), np.nextafter(thr, F(0))]
    return _post([_seg(0, 4), _seg(4, 4), _seg(8, 4)], [], 12, score, score_thr=thr, want_kept=[1])


def strict_size():
    return _post([_seg(0, 5), _seg(5, 6), _seg(11, 4)], [], 15, [0.5, 0.6, 0.7], min_points=5, want_kept=[1])


def _iou32(inter, a, b):
    return F(inter) / ((F(a) + F(b)) - F(inter) + F(1e-8))


def strict_iou(below):
    """a pair of 10-point proposals sharing 5 points: IoU = fl(5 / 15)"""
    thr = _iou32(5, 10, 10)
    if below:
        thr = np.nextafter(thr, F(0))
    return _post([_seg(0, 10)], [_seg(5, 10)], 15, [0.9, 0.8], iou_thr=thr, want_kept=[0] if below else [0, 1])


def ties():
    """equal scores along a chain of overlaps: the lower id is visited first"""
    a = [_seg(8 * j, 8) for j in range(4)]
    b = [_seg(8 * j + 4, 8) for j in range(4)]
    return _post(a, b, 36, [0.5] * 8, want_kept=[0, 1, 2, 3])


def chain_40():
    """A_0 B_0 A_1 B_1 ... : each overlaps the next with IoU 4 / 12, scores descending along the chain"""
    n = 40
    a = [_seg(8 * j, 8) for j in range(n)]
    b = [_seg(8 * j + 4, 8) for j in range(n)]
    score = np.zeros(2 * n, F)
    score[:n] = 0.9 - 0.01 * (2 * np.arange(n))
    score[n:] = 0.9 - 0.01 * (2 * np.arange(n) + 1)
    return _post(a, b, 8 * n + 4, score, score_thr=0.05, want_kept=list(range(n)))


def one_set_only():
    a = [_seg(0, 6), _seg(6, 6), _seg(20, 5)]
    b = [_seg(3, 6)]  # points 12 .. 19 and 25 .. 29 are in no proposal, 0 .. 2 / 9 .. 11 / 20 .. 24 only in set A
    return _post(a, b, 30, [0.5, 0.6, 0.7, 0.8], want_kept=[2, 3])


def neighbours(n):
    """proposal 0 overlaps n proposals of the other set; iou_thr = 0 makes every one a neighbour"""
    a = [_seg(0, 2 * n)] + [_seg(2 * n + 3 * j, 3) for j in range(5)]
    b = [_seg(2 * j, 2) for j in range(n)]
    score = np.r_[0.2, [0.3] * 5, 0.5 + 0.001 * np.arange(n)]
    return _post(a, b, 2 * n + 15, score, iou_thr=0.0, expect="equal" if n <= 32 else "none", hub=0, degree=n)


def sharers(n, filtered=False):
    """proposal 0 shares one point with each of n proposals of the other set whose ids fall on 4 residues modulo 64; the IoUs
    (1 / (n + 2)) stay below the threshold, so only the sharers' table is loaded"""
    fillers, per = 4, 17  # ids: 1 hub + 4 fillers of set A, then set B; sharers at B ids 64 j + c, c < 4
    n_b = 64 * per
    pick = [64 * j + c for c in range(4) for j in range(per)][:n]
    hub = [2 * q for q in sorted(pick)]
    a = [hub] + [_seg(2 * n_b + 3 * j, 3) for j in range(fillers)]
    b = [_seg(2 * q, 2) for q in range(n_b)]
    rng = np.random.default_rng(n)
    score = rng.uniform(0.2, 0.9, size=1 + fillers + n_b).astype(F)
    if filtered:
        for q in sorted(pick)[::3]:
            score[1 + fillers + q] = 0.01
    ids = [1 + fillers + q for q in pick]
    assert len({i % 64 for i in ids}) == 4
    return _post(a, b, 2 * n_b + 3 * fillers, score, iou_thr=0.5,
                 expect="either" if filtered else ("equal" if n <= 64 else "none"), hub=0, sharers=n)


def none_survive():
    return _post([_seg(0, 4), _seg(4, 4)], [_seg(2, 4)], 8, [0.01, 0.05, 0.089], want_kept=[])


def random_p(P, seed=0):
    """P proposals: consecutive segments of 2 .. 7 points in each set, boundaries unrelated, scores from a few values (ties)"""
    rng = np.random.default_rng(1000 * seed + P)
    n_a = (P + 1) // 2
    n_b = P - n_a

    def segments(count, first):
        out = []
        for _ in range(count):
            n = int(rng.integers(2, 8))
            out.append(_seg(first, n))
            first += n + int(rng.integers(0, 2))
        return out, first
    a, end_a = segments(n_a, 0)
    b, end_b = segments(n_b, 1)
    score = rng.choice(np.linspace(0.05, 0.95, 19).astype(F), size=P)
    return _post(a, b, max(end_a, end_b) + 1, score, min_points=2)


def live_lt_bound():
    """37 live proposals in tables sized for 50: NaN scores, huge sizes and closing offsets behind them"""
    c = random_p(37, seed=1)
    pad = 13
    c["score"] = np.r_[c["score"], np.full(pad, np.nan, F)]
    c["sizes"] = np.r_[c["sizes"], np.full(pad, 1 << 40, np.int64)]
    c["proposal_offsets"] = np.r_[c["proposal_offsets"], np.full(pad, c["proposal_offsets"][-1], np.int32)]
    c["live"] = 37
    return c


POST_CASES = {
    "strict_score": strict_score,
    "strict_size": strict_size,
    "strict_iou_at": functools.partial(strict_iou, False),
    "strict_iou_below": functools.partial(strict_iou, True),
    "ties": ties,
    "chain_40": chain_40,
    "one_set_only": one_set_only,
    "neighbours_32": functools.partial(neighbours, 32),
    "neighbours_33": functools.partial(neighbours, 33),
    "sharers_64": functools.partial(sharers, 64),
    "sharers_65": functools.partial(sharers, 65),
    "sharers_65_filtered": functools.partial(sharers, 65, True),
    "none_survive": none_survive,
    "live_lt_bound": live_lt_bound,
}
for _p in (1, 3, 4, 5, 1023, 1024, 1025):
    POST_CASES[f"p_{_p}"] = functools.partial(random_p, _p)
POST_CASES = {k: functools.lru_cache(maxsize=None)(v) for k, v in POST_CASES.items()}
MAX_NBR, TABLE = 32, 64  # kMaxNbr, kTable of csrc/postprocess.hip
