"""TEST INFRASTRUCTURE - the inputs the pose-evaluation tests share (tests/test_pose_eval_cpu.py on the host formulations,
tests/test_gpu_pose_eval*.py on the kernels): boxes, instances with known poses, pairs of every symmetry type, the evaluator's
closed-form batch, and the comparisons with the restatement (tests/pose_eval_ref.py)."""
import numpy as np
import torch

from gapartnet_amd.misc.info import SYMMETRY_MATRIX
from gapartnet_amd.structure.instances import Instances
from gapartnet_amd.structure.point_cloud import PointCloudBatch
from tests import pose_eval_ref as ref

I3 = np.eye(3)


def rot(axis, deg):
    """rotation matrix about `axis` by `deg` (Rodrigues), acting on columns"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return I3 + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, [1, 0, 2]]


def box(centre, half, frame=I3):
    return ref.box_corners(1.0, frame, np.asarray(centre, np.float64), np.asarray(half, np.float64))


def exact_cases():
    """name -> (a, b, IoU): the cases whose value the tie rule decides"""
    A = box([0, 0, 0], [0.5, 0.5, 0.5])
    return {"itself": (A, A, 1.0),
            "relabelled axes": (A, box([0, 0, 0], [0.5, 0.5, 0.5], np.array([[0, 1, 0], [0, 0, 1], [1.0, 0, 0]])), 1.0),
            "flipped by 180 degrees": (A, box([0, 0, 0], [0.5, 0.5, 0.5], np.diag([-1.0, -1.0, 1.0])), 1.0),
            "half-shifted": (A, box([0.5, 0, 0], [0.5, 0.5, 0.5]), 1.0 / 3.0),
            "half-sized concentric": (A, box([0, 0, 0], [0.25, 0.25, 0.25]), 1.0 / 8.0),
            "half box sharing a face": (A, box([0.25, 0, 0], [0.25, 0.5, 0.5]), 0.5),
            "touching": (A, box([1.0, 0, 0], [0.5, 0.5, 0.5]), 0.0),
            "disjoint": (A, box([2.0, 0, 0], [0.5, 0.5, 0.5]), 0.0)}


def coplanar_rotations():
    """the same box turned by 30, 60, 90 degrees about z: top and bottom stay coplanar"""
    A = box([0.125, -0.25, 0.5], [0.5, 0.25, 0.375])
    return [(A, box([0.125, -0.25, 0.5], [0.5, 0.25, 0.375], rot([0, 0, 1], deg).T)) for deg in (30.0, 60.0, 90.0)]


def turned_self_pairs(n=40, seed=2):
    """boxes in general orientation against themselves (even i) and against the same pose rebuilt with a scale that differs in
    the last bit (odd i)"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        R, h, t, s = random_rotation(rng), rng.uniform(0.1, 0.5, 3), rng.uniform(-0.3, 0.3, 3), rng.uniform(0.3, 1.2)
        a = ref.box_corners(s, R, t, h)
        pairs.append((a, a if i % 2 == 0 else ref.box_corners(np.nextafter(s, 2.0), R, t, h)))
    return pairs


def random_box_pairs(n, seed, max_aspect=None):
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        if max_aspect is None:
            h = rng.uniform(0.05, 0.5, (2, 3))
        else:  # one long axis each: aspect ratios up to max_aspect
            h = rng.uniform(0.05, 0.1, (2, 3))
            h[0, rng.integers(3)] *= rng.uniform(1.0, max_aspect) * 0.5
            h[1, rng.integers(3)] *= rng.uniform(1.0, max_aspect) * 0.5
        Ra = random_rotation(rng)
        Rb = rot(rng.normal(size=3), rng.uniform(0, 0.5)) @ Ra if i % 5 == 0 else random_rotation(rng)  # one in five nearly aligned
        pairs.append((ref.box_corners(1.0, Ra, rng.uniform(-0.2, 0.2, 3), h[0]), ref.box_corners(1.0, Rb, rng.uniform(-0.2, 0.2, 3), h[1])))
    return pairs


def make_instances(seed, sizes, W, kinds=None, dtype=np.float32):
    """scenes of instances with known poses: -> xyz, npcs [N,3] f32 (shuffled inside each scene), labels [N], offsets, poses"""
    rng = np.random.default_rng(seed)
    xyz, npcs, lab, off, poses = [], [], [], [0], []
    for s, scene_sizes in enumerate(sizes):
        px, pn, pl = [rng.normal(size=(17, 3))], [np.zeros((17, 3))], [np.full(17, -1)]      # rows of no instance
        for w, n in enumerate(scene_sizes):
            kind = (kinds or {}).get((s, w), "solid")
            q = rng.uniform(-0.4, 0.4, (n, 3))
            if kind == "planar":
                q[:, 2] = 0.25
            if kind == "collinear":
                q = 0.1 + np.outer(np.linspace(-0.3, 0.3, n), [0.5, -0.25, 1.0])
            q = q.astype(dtype).astype(np.float64)
            s_, R, t = rng.uniform(0.2, 1.5), random_rotation(rng), rng.uniform(-0.5, 0.5, 3)
            poses.append((s, w, s_, R, t))
            px.append(q @ (s_ * R) + t), pn.append(q), pl.append(np.full(n, w))
        px, pn, pl = np.concatenate(px), np.concatenate(pn), np.concatenate(pl)
        order = rng.permutation(len(pl))
        xyz.append(px[order]), npcs.append(pn[order]), lab.append(pl[order]), off.append(off[-1] + len(pl))
    return np.concatenate(xyz).astype(dtype), np.concatenate(npcs).astype(dtype), np.concatenate(lab).astype(np.int64), np.array(off), poses


def slots_of(lab, off, W):
    scene = np.searchsorted(off[1:], np.arange(len(lab)), side="right")
    return np.where((lab >= 0) & (lab < W), scene * W + lab, -1)


def assert_fit_equals_ref(got, want, tol):
    """got: dict of tensors per slot; want: list of (count, dict or None) from the restatement"""
    for g, (n, w) in enumerate(want):
        assert int(got["count"][g]) == n, g
        assert bool(got["valid"][g]) == (w is not None), g
        for k in ("scale", "rotation", "translation", "half", "bbox"):
            v = got[k][g].cpu().numpy()
            if w is None:
                assert np.isnan(v).all(), (g, k)
            else:
                assert np.abs(v - w[k]).max() <= tol, (g, k, np.abs(v - w[k]).max())


FIT_SIZES = [[1, 2, 3, 63, 64, 0, 65], [257, 40, 30, 0, 0, 0, 12]]
FIT_KINDS = {(1, 1): "planar", (1, 2): "collinear"}


def random_pairs(seed, n):
    """pairs of every symmetry type: a ground truth and a prediction a few degrees / per cent off a random candidate"""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("ps", "pR", "pt", "ph", "gs", "gR", "gt", "gh", "ty")}
    for i in range(n):
        ty = i % len(SYMMETRY_MATRIX)
        Rg, sg, tg, hg = random_rotation(rng), rng.uniform(0.3, 1.2), rng.uniform(-0.3, 0.3, 3), rng.uniform(0.1, 0.5, 3)
        Sk = np.array(SYMMETRY_MATRIX[ty][rng.integers(len(SYMMETRY_MATRIX[ty]))])
        Rp = rot(rng.normal(size=3), rng.uniform(0.5, 12.0)) @ Sk @ Rg
        for k, v in zip(out, (sg * rng.uniform(0.9, 1.1), Rp, tg + rng.normal(size=3) * 0.03, hg * rng.uniform(0.9, 1.1, 3), sg, Rg, tg, hg, ty)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def first_extremum_case(seed=31):
    """a candidate table of its own (the table is an argument of the entry point) on which the winning candidate is not a matter
    of round-off, unlike SYMMETRY_MATRIX, whose groups turn a box onto itself: turns Z(d) about z of a box with three different
    extents.  Type 0 = [Z0, Z40, Z80], type 1 = [Z80, Z0, Z40], type 2 = [Z40, Z40, Z0, Z0] (duplicates: bit-exact ties, the first
    must win), type 3 = [I, I].  Every pair's prediction is one degree off one candidate of its type.
    -> (d as random_pairs gives it, (table, start, count) tensors, per pair the restatement's result, per pair the type)"""
    rng = np.random.default_rng(seed)
    Z = lambda deg: rot([0, 0, 1], deg)
    groups = [[Z(0), Z(40), Z(80)], [Z(80), Z(0), Z(40)], [Z(40), Z(40), Z(0), Z(0)], [I3, I3]]
    counts = [len(g) for g in groups]
    table = (torch.from_numpy(np.array([m for g in groups for m in g])), torch.tensor(np.concatenate([[0], np.cumsum(counts)[:-1]]), dtype=torch.int32),
             torch.tensor(counts, dtype=torch.int32))
    out = {k: [] for k in ("ps", "pR", "pt", "ph", "gs", "gR", "gt", "gh", "ty")}
    want = []
    for ty, group in enumerate(groups):
        for j in range(len(group)):
            Rg, sg, tg, hg = random_rotation(rng), rng.uniform(0.5, 1.0), rng.uniform(-0.3, 0.3, 3), np.array([0.4, 0.15, 0.25])
            vals = (sg * 1.02, rot(rng.normal(size=3), 1.0) @ group[j] @ Rg, tg + 0.01, hg * 1.01, sg, Rg, tg, hg, ty)
            for k, v in zip(out, vals):
                out[k].append(v)
            want.append(ref.pair_errors(vals[:4], vals[4:8], np.array(group)))
    return {k: np.array(v) for k, v in out.items()}, table, want


def assert_first_extrema(got, d, want):
    """k_re and k_iou equal the restatement's first extremum on every pair of first_extremum_case; where the type has no duplicate
    the winner leads by far more than GAP (asserted), where it has, the tie is bit-exact and the first index is the answer"""
    clear = [0, 0]
    for i, w in enumerate(want):
        ty = int(d["ty"][i])
        assert int(got["k_re"][i]) == w["k_re"] and int(got["k_iou"][i]) == w["k_iou"], (i, ty, int(got["k_re"][i]), int(got["k_iou"][i]), w["k_re"], w["k_iou"])
        if ty < 2:
            assert clear_winner(w["all_re"], w["k_re"], False) and clear_winner(w["all_iou"], w["k_iou"], True), i
            clear[0], clear[1] = clear[0] + 1, clear[1] + 1
        if ty == 3:
            assert w["k_re"] == 0 and w["k_iou"] == 0
    assert clear == [6, 6]
    # the winners cover every position of the table, the last one included, and both copies' first index for the duplicates
    assert sorted({(int(d["ty"][i]), w["k_iou"]) for i, w in enumerate(want)}) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 2), (3, 0)]


def pair_dicts(d, device="cpu"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    pred = {"scale": t(d["ps"]), "rotation": t(d["pR"]), "translation": t(d["pt"]), "half": t(d["ph"])}
    gt = {"scale": t(d["gs"]), "rotation": t(d["gR"]), "translation": t(d["gt"]), "half": t(d["gh"])}
    return pred, gt, t(d["ty"]).to(torch.int32)


def ref_pair_errors(d):
    return [ref.pair_errors((d["ps"][i], d["pR"][i], d["pt"][i], d["ph"][i]), (d["gs"][i], d["gR"][i], d["gt"][i], d["gh"][i]),
                            np.array(SYMMETRY_MATRIX[int(d["ty"][i])])) for i in range(len(d["ty"]))]


GAP = 1e-9  # the extremum must beat every other candidate by this much (degrees, IoU) for its index to be compared


def clear_winner(values, k, largest):
    """is candidate k ahead of all others by more than GAP?  (A box turned by 180 degrees about one of its axes is the same box, so
    in every group but the trivial one the IoUs of the candidates tie in pairs up to round-off: there the index the code returns
    must be one of the tied ones, which is all that can be asked.)"""
    others = np.delete(values, k)
    return others.size == 0 or (values[k] - others.max() > GAP if largest else others.min() - values[k] > GAP)


def assert_pair_errors_equal_ref(got, want, tol):
    compared = [0, 0]
    for i, w in enumerate(want):
        for k in ("re_deg", "te", "se", "iou"):
            assert abs(float(got[k][i]) - w[k]) <= tol, (i, k, float(got[k][i]), w[k])
        if clear_winner(w["all_re"], w["k_re"], False):
            assert int(got["k_re"][i]) == w["k_re"], i
            compared[0] += 1
        assert w["all_iou"][int(got["k_iou"][i])] >= w["iou"] - GAP and w["all_re"][int(got["k_re"][i])] <= w["re_deg"] + GAP, i
        if clear_winner(w["all_iou"], w["k_iou"], True):
            assert int(got["k_iou"][i]) == w["k_iou"], i
            compared[1] += 1
    return compared


SYM_OF_CLASS = [0, 1, 3, 3, 2, 0, 3, 2, 4, 1]


def evaluator_case(device="cpu"):
    """two scenes whose proposals are the ground-truth instances with the NPCS perturbed by a known rotation Q (3 degrees about a
    generic axis), shift b and scale a: pred = (npcs @ Q) a + b, so s' = s / a, R' = Q^T R, t' = t - (b Q^T)(s R) / a and the
    errors are re = 3 degrees (every other candidate is at least 27 away), te = (s / a) |b|, se = s |1 / a - 1|, and the IoU that of
    the box of that pose with the perturbed NPCS' extent against the ground truth's.  Class 5 (no
    symmetry) is shifted only, with the box corners among its points: IoU = h / (h + b) along the shifted axis.  Class 7 has a
    proposal without a single predicted point (no pose), class 4's instance is collinear (no ground-truth pose), class 9 has an
    instance and no proposal, class 3 an instance whose proposal is of class 2 (no pair)."""
    rng = np.random.default_rng(8)
    Q, a, b = rot([1.0, 2.0, 3.0], 3.0), 1.25, np.array([0.02, -0.01, 0.015])
    W = 4
    spec = [[(1, "solid"), (5, "shift"), (7, "nomask"), (4, "collinear")], [(8, "solid"), (1, "solid"), (9, "none"), (3, "wrong")]]
    pts, npcs_gt, lab, bidx, p_xyz, p_npcs, p_mask, p_off, p_cls, p_b, ious, labels = [], [], [], [], [], [], [], [0], [], [], [], []
    expect = {}
    for s, scene in enumerate(spec):
        labels.append([c for c, _ in scene])
        for w, (c, kind) in enumerate(scene):
            n = 150
            h = np.array([0.3, 0.2, 0.25])
            q = rng.uniform(-1, 1, (n, 3)) * h
            if kind == "shift":
                q[:8] = ref.SIGNS * h
            if kind == "collinear":
                q = np.outer(np.linspace(-0.3, 0.3, n), [0.5, -0.25, 1.0])
            q = q.astype(np.float32).astype(np.float64)
            sc, R, t = rng.uniform(0.4, 0.9), random_rotation(rng), rng.uniform(-0.3, 0.3, 3)
            x = (q @ (sc * R) + t).astype(np.float32)
            pts.append(x), npcs_gt.append(q), lab.append(np.full(n, w)), bidx.append(np.full(n, s))
            if kind == "none":
                continue
            shift = np.array([0.05, 0.0, 0.0])
            pred = q + shift if kind == "shift" else (q @ Q) * a + b
            p_xyz.append(x), p_npcs.append(pred + 0.5), p_mask.append(np.full(n, kind != "nomask")), p_off.append(p_off[-1] + n)
            p_cls.append(2 if kind == "wrong" else c), p_b.append(np.full(n, s))
            row = np.zeros(W)
            row[w] = 1.0
            ious.append(row)
            if kind == "solid":
                # the IoU of the closed-form predicted box (s', R', t', the perturbed NPCS' own extent) and the ground truth's, by
                # the restatement over the class's candidates: independent of the code under test
                p32 = (pred + 0.5).astype(np.float32).astype(np.float64) - 0.5
                closed = ref.pair_errors((sc / a, Q.T @ R, t - (b @ Q.T) @ (sc * R) / a, np.abs(p32).max(0)), (sc, R, t, np.abs(q).max(0)),
                                         np.array(SYMMETRY_MATRIX[SYM_OF_CLASS[c]]))
                expect.setdefault(c, []).append((3.0, sc / a * np.linalg.norm(b), sc * abs(1 / a - 1), closed["iou"]))
            if kind == "shift":
                expect.setdefault(c, []).append((0.0, sc * 0.05, 0.0, 0.3 / 0.35))
    mask = np.concatenate(p_mask)
    f32 = lambda v: torch.from_numpy(np.asarray(v, np.float32)).to(device)
    i64 = lambda v: torch.from_numpy(np.asarray(v, np.int64)).to(device)
    kept = Instances(pt_xyz=f32(np.concatenate(p_xyz)), score_preds=f32(np.linspace(0.9, 0.5, len(p_cls))), pt_sem_classes=i64(p_cls),
                     batch_indices=i64(np.concatenate(p_b)), proposal_offsets=i64(p_off), instance_sem_labels=i64(labels).int(),
                     ious=f32(np.stack(ious)), npcs_preds=f32(np.concatenate(p_npcs)[mask]),
                     npcs_valid_mask=torch.from_numpy(mask).to(device))
    xyz = np.concatenate(pts)
    batch = PointCloudBatch(pc_ids=["a", "b"], points=f32(np.concatenate([xyz, np.zeros_like(xyz)], 1)), batch_indices=i64(np.concatenate(bidx)),
                            batch_size=2, instance_labels=i64(np.concatenate(lab)), instance_sem_labels=i64(labels).int(),
                            gt_npcs=f32(np.concatenate(npcs_gt)))
    picks = lambda sizes: torch.from_numpy(np.stack([np.random.RandomState(5).randint(int(n), size=(20, 5)) for n in sizes]))
    return kept, batch, picks, expect
