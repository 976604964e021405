"""Is an estimated part pose right?  Rotation, translation and scale error and oriented-box IoU of the predicted part poses
against the ground truth, under the part's symmetry group: R_e, T_e, S_e, 3D mIoU and the 5 deg / 5 cm and 10 deg / 10 cm accuracies the
GAPartNet paper reports for its second task.  The reference cannot produce them (its ``on_test_epoch_end`` ends at a commented-out
``# pose estimation``).  On GPU tensors the three building blocks are HIP entry points (csrc/poseeval.hip, include/gpn.h section
PE); on CPU tensors the torch float64 formulations below compute the same contract and document it.

``gt_part_poses``      the exact similarity ``xyz ~ npcs @ (s R) + t`` (row vectors, as ``pose_fitting_batched._umeyama``) of every
                       ground-truth instance: plain Umeyama over ALL its points - means first, then centred moments -, no RANSAC.
                       ``half`` = max |npcs| per axis over the instance's points (the observed extent, which is what
                       ``gpn_pose_fit`` builds the predicted box from), ``bbox`` = (signs * half * s) @ R + t.  No pose (valid =
                       False, NaN) for fewer than 3 points and for collinear points: second singular value of the NPCS covariance
                       below 1e-9 x the first.  A planar instance (a door seen as one face) is rank 2 and valid.
``oriented_box_iou``   exact IoU of two oriented boxes given as 8 corners (``_CORNER_SIGNS`` order).  Centre = mean of the corners,
                       axes and half extents from the edges corner 1, 2, 3 - corner 0.  Each of the 12 faces (6 of a, 6 of b) is
                       clipped by the 6 half-spaces of the other box (Sutherland-Hodgman: a polygon never exceeds 10 vertices) and
                       contributes the cone volume area * height / 3 from a's centre, the height signed along the face's outward
                       normal; their sum is the intersection.  Tie rule: a vertex ON a clipping plane is inside only while a's
                       faces are clipped by b and only if the face's outward normal and the plane's normal have a positive dot
                       product; otherwise it is outside.  (With <= in both passes identical boxes would score twice their volume,
                       with < in one pass touching boxes would keep one uncancelled face.)  ON = a signed distance within 2^-26 x
                       the largest half extent of the two boxes, taken as 0: with an exact test the sign of a rounding error
                       decides whether a coincident face of a turned box counts (a box against itself: 0.1 .. 15).  Round-off
                       accuracy in general position, eps / angle where faces meet at a small angle, about 1e-8 at worst.  NaN for
                       a non-finite corner or a zero extent.
``pose_pair_errors``   per matched pair, with F_k = S_k R_gt over the candidates S_k of the part's symmetry type (``misc/info.py``
                       SYMMETRY_MATRIX, flattened by ``symmetry_table``): re_deg = min_k angle(R_pred, F_k) computed as
                       atan2(|v|, (tr M - 1) / 2), M = R_pred F_k^T, v = vee of the antisymmetric part of M (acos loses eight digits
                       at 0); te = |t_pred - t_gt|; se = |s_pred - s_gt| (in GAPartNet's NPCS the similarity scale IS the box
                       diagonal: the size error, invariant under every group); iou = max_k IoU(predicted box, ground-truth box
                       re-framed by S_k with the same centre and half extents); k_re / k_iou = the first extremum.  The groups are
                       proper rotations and closed under inverse, so the side S_k multiplies on does not change either extremum.
``match_pairs``        (prediction, ground truth) pairs = exactly the true positives of ``compute_ap_multi`` at the threshold.
``PoseEvaluator``      accumulates the pairs of an epoch on the device, one host read in ``compute()``.
"""
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from ..structure.instances import Instances
from .info import SYMMETRY_MATRIX
from .pose_fitting_batched import _CORNER_SIGNS, draw_picks, estimate_pose_from_npcs_batched

# corners of face 2 * axis + (0: the -axis side, 1: the +axis side), in cyclic order (csrc/poseeval.hip: kFaceCorner)
_FACE_CORNER = [[0, 2, 6, 3], [1, 4, 7, 5], [0, 1, 5, 3], [2, 4, 7, 6], [0, 1, 4, 2], [3, 5, 7, 6]]
_POLY_MAX = 10
_SNAP = 2.0 ** -26
_SYM_CACHE = {}


def symmetry_table(device=None):
    """SYMMETRY_MATRIX flattened: (table [K,3,3] f64, start [T] i32, count [T] i32) - type t owns table[start[t]:start[t]+count[t]]"""
    key = str(device)
    if key not in _SYM_CACHE:
        counts = [len(g) for g in SYMMETRY_MATRIX]
        table = torch.tensor([m for g in SYMMETRY_MATRIX for m in g], dtype=torch.float64)
        start = torch.tensor(np.concatenate([[0], np.cumsum(counts)[:-1]]), dtype=torch.int32)
        _SYM_CACHE[key] = tuple(t.to(device) if device is not None else t for t in (table, start, torch.tensor(counts, dtype=torch.int32)))
    return _SYM_CACHE[key]


def _hip():
    from .. import backend
    ops = backend.raw()
    if ops.name != "hip":
        raise RuntimeError("pose metrics on a GPU tensor need the HIP library as the operator backend")
    return ops


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ------------------------------------------------------------------------------------------------ ground-truth poses
@torch.no_grad()
def gt_part_poses(xyz: torch.Tensor, gt_npcs: torch.Tensor, instance_labels: torch.Tensor, scene_offsets, W: int,
                  force_torch: bool = False) -> Dict[str, torch.Tensor]:
    """xyz, gt_npcs [N,3] (float32 is what the kernel reads), instance_labels [N] = the point's instance id in its scene (outside
    0 .. W-1 = none), scene_offsets [S+1] = the scenes' rows -> per slot scene * W + id, [S*W]: count i64, valid bool, scale,
    rotation [.,3,3], translation [.,3], half [.,3], bbox [.,8,3] float64 (module docstring).  ``force_torch``: the torch formulation
    on GPU tensors too (the baseline of tools/pose_eval_bench.py); the same switch exists on the other two functions."""
    dev, f64 = xyz.device, torch.float64
    off = torch.as_tensor(scene_offsets, dtype=torch.int64).to(dev)
    S, N, W = int(off.numel()) - 1, int(xyz.shape[0]), int(W)
    scene = torch.bucketize(torch.arange(N, device=dev), off[1:], right=True)
    ids = instance_labels.to(dev).long()
    slot = torch.where((ids >= 0) & (ids < W) & (scene < S), scene * W + ids, torch.full_like(ids, -1))
    xyz32, npcs32 = xyz.to(torch.float32), gt_npcs.to(dev).to(torch.float32)
    if xyz.is_cuda and not force_torch:
        out = _hip().pose_gt_fit(xyz32, npcs32, slot.to(torch.int32), off, W)
        out["valid"] = out["valid"].bool()
        return out
    return _gt_part_poses_torch(xyz32, npcs32, slot, S * W)


def _gt_part_poses_torch(xyz32, npcs32, slot, G):
    dev, f64 = xyz32.device, torch.float64
    rows = torch.nonzero(slot >= 0).squeeze(1)
    g, src, dst = slot[rows], npcs32[rows].to(f64), xyz32[rows].to(f64)
    count = torch.bincount(g, minlength=G)
    n = count.to(f64)
    mu_s = torch.zeros(G, 3, dtype=f64, device=dev).index_add_(0, g, src) / n[:, None]
    mu_d = torch.zeros(G, 3, dtype=f64, device=dev).index_add_(0, g, dst) / n[:, None]
    cs, cd = src - mu_s[g], dst - mu_d[g]
    cov = torch.zeros(G, 9, dtype=f64, device=dev).index_add_(0, g, (cd[:, :, None] * cs[:, None, :]).reshape(-1, 9)).reshape(G, 3, 3) / n[:, None, None]
    css = torch.zeros(G, 9, dtype=f64, device=dev).index_add_(0, g, (cs[:, :, None] * cs[:, None, :]).reshape(-1, 9)).reshape(G, 3, 3) / n[:, None, None]
    half = torch.zeros(G, 3, dtype=f64, device=dev).scatter_reduce_(0, g[:, None].expand(-1, 3), src.abs(), "amax")
    finite = torch.isfinite(cov).all(-1).all(-1) & torch.isfinite(css).all(-1).all(-1)
    zero = torch.zeros_like(cov)
    sv = torch.linalg.svdvals(torch.where(finite[:, None, None], css, zero))
    U, Sg, Vh = torch.linalg.svd(torch.where(finite[:, None, None], cov, zero))
    sign = torch.ones_like(Sg)
    sign[:, 2] = torch.where(torch.linalg.det(U) * torch.linalg.det(Vh) < 0.0, -1.0, 1.0).to(f64)
    Sg, U = Sg * sign, U * sign[:, None, :]
    var = css[:, 0, 0] + css[:, 1, 1] + css[:, 2, 2]
    scale = Sg.sum(-1) / var
    rotation = (U @ Vh).transpose(1, 2)
    translation = mu_d - torch.einsum("bi,bij->bj", mu_s, scale[:, None, None] * rotation)
    valid = finite & (count >= 3) & (sv[:, 1] >= 1e-9 * sv[:, 0]) & (sv[:, 0] > 0) & torch.isfinite(scale)
    signs = torch.tensor(_CORNER_SIGNS, dtype=f64, device=dev)
    bbox = torch.einsum("pki,pij->pkj", signs[None] * half[:, None, :] * scale[:, None, None], rotation) + translation[:, None, :]
    nan, bad = float("nan"), ~valid
    return {"count": count, "valid": valid, "scale": scale.masked_fill(bad, nan), "rotation": rotation.masked_fill(bad[:, None, None], nan),
            "translation": translation.masked_fill(bad[:, None], nan), "half": half.masked_fill(bad[:, None], nan),
            "bbox": bbox.masked_fill(bad[:, None, None], nan)}


# ------------------------------------------------------------------------------------------------ box IoU
def _box_frame(corners):
    """[B,8,3] -> centre [B,3], unit axes [B,3,3], half extents [B,3], volume [B] (NaN: non-finite corner or zero extent)"""
    c = corners.sum(1) / 8.0
    e = (corners[:, 1:4] - corners[:, :1]) / 2.0
    h = torch.sqrt(_dot3(e, e))
    vol = 8.0 * h[:, 0] * h[:, 1] * h[:, 2]
    ok = torch.isfinite(corners).all(-1).all(-1) & (vol > 0) & torch.isfinite(vol)
    return c, e / h[..., None], h, torch.where(ok, vol, torch.full_like(vol, float("nan")))


def _clipped_cones(xc, xu, yc, yu, yh, a_by_b: bool, apex, snap):
    """the six faces of the boxes X (corners xc [B,8,3], axes xu) clipped by the boxes Y (centre yc, axes yu, half extents yh):
    their cone volumes from ``apex`` [B,3] -> [B,6]"""
    B, dev, dt = xc.shape[0], xc.device, xc.dtype
    sgn = torch.tensor([-1.0, 1.0] * 3, dtype=dt, device=dev)
    normal = xu[:, [0, 0, 1, 1, 2, 2]] * sgn[None, :, None]                              # [B,6,3] outward normals of the faces
    poly = torch.zeros(B, 6, _POLY_MAX + 1, 3, dtype=dt, device=dev)                      # (slot 10 takes what is not emitted)
    poly[:, :, :4] = xc[:, torch.tensor(_FACE_CORNER, device=dev)]
    n = torch.full((B, 6), 4, dtype=torch.int64, device=dev)
    idx = torch.arange(_POLY_MAX, device=dev)[None, None, :]
    for pl in range(6):
        pn = yu[:, pl >> 1] * (1.0 if pl & 1 else -1.0)                                   # [B,3]
        p = poly[:, :, :_POLY_MAX]
        d = _dot3(p - yc[:, None, None, :], pn[:, None, None, :]) - yh[:, pl >> 1][:, None, None]
        d = torch.where(d.abs() <= snap[:, None, None], torch.zeros_like(d), d)
        nxt = torch.where(idx + 1 == n[..., None], torch.zeros_like(idx), idx + 1).clamp(max=_POLY_MAX - 1)
        q, dq = p.gather(2, nxt[..., None].expand(-1, -1, -1, 3)), d.gather(2, nxt)
        tie = (_dot3(normal, pn[:, None, :]) > 0)[..., None] if a_by_b else torch.zeros(B, 6, 1, dtype=torch.bool, device=dev)
        live = idx < n[..., None]
        in_p, in_q = (d < 0) | ((d == 0) & tie), (dq < 0) | ((dq == 0) & tie)
        e1, e2 = live & in_p, live & (in_p != in_q)
        cross = p + (d / (d - dq))[..., None] * (q - p)
        cnt = e1.long() + e2.long()
        before = cnt.cumsum(-1) - cnt
        pos1 = torch.where(e1, before, torch.full_like(before, _POLY_MAX)).clamp(max=_POLY_MAX)
        pos2 = torch.where(e2, before + e1.long(), torch.full_like(before, _POLY_MAX)).clamp(max=_POLY_MAX)
        new = torch.zeros_like(poly)
        new.scatter_(2, pos1[..., None].expand(-1, -1, -1, 3), p)
        new.scatter_(2, pos2[..., None].expand(-1, -1, -1, 3), torch.where(e2[..., None], cross, torch.zeros_like(cross)))
        poly, n = new, cnt.sum(-1).clamp(max=_POLY_MAX)
    v0 = poly[:, :, 0]
    s = torch.zeros(B, 6, 3, dtype=dt, device=dev)
    for i in range(1, _POLY_MAX - 1):
        a, b = poly[:, :, i] - v0, poly[:, :, i + 1] - v0
        s = s + torch.where((i + 1 < n)[..., None], torch.cross(a, b, dim=-1), torch.zeros_like(a))
    area = 0.5 * _dot3(s, normal).abs()
    height = _dot3(v0 - apex[:, None, :], normal)
    return torch.where(n >= 3, area * height / 3.0, torch.zeros_like(area))


def _box_iou_torch(a, b):
    ca, ua, ha, va = _box_frame(a)
    cb, ub, hb, vb = _box_frame(b)
    ok = ~(torch.isnan(va) | torch.isnan(vb))
    snap = _SNAP * torch.maximum(ha.max(1)[0], hb.max(1)[0])
    cones = torch.cat([_clipped_cones(a, ua, cb, ub, hb, True, ca, snap), _clipped_cones(b, ub, ca, ua, ha, False, ca, snap)], dim=1)
    inter = torch.zeros_like(va)
    for f in range(12):  # in face order, as the kernel adds them
        inter = inter + torch.where(ok, cones[:, f], torch.zeros_like(va))
    return inter / (va + vb - inter)


@torch.no_grad()
def oriented_box_iou(a: torch.Tensor, b: torch.Tensor, force_torch: bool = False) -> torch.Tensor:
    """a, b [P,8,3] corners (``_CORNER_SIGNS`` order) -> IoU [P] float64 (module docstring: clipping, cone volumes, tie rule)"""
    a, b = a.to(torch.float64), b.to(torch.float64)
    if a.is_cuda and not force_torch:
        return _hip().box_iou_3d(a, b)
    if a.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float64, device=a.device)
    return _box_iou_torch(a, b)


# ------------------------------------------------------------------------------------------------ pair errors
def _pose_box(scale, frame, translation, half):
    signs = torch.tensor(_CORNER_SIGNS, dtype=torch.float64, device=scale.device)
    ext = signs[None] * half[:, None, :] * scale[:, None, None]                           # [P,8,3]
    return ((ext[..., 0, None] * frame[:, None, 0] + ext[..., 1, None] * frame[:, None, 1]) + ext[..., 2, None] * frame[:, None, 2]) \
        + translation[:, None, :]


def _side(pose):
    return [pose[k].to(torch.float64) for k in ("scale", "rotation", "translation", "half")]


@torch.no_grad()
def pose_pair_errors(pred: Dict[str, torch.Tensor], gt: Dict[str, torch.Tensor], sym_type: torch.Tensor, table=None,
                     force_torch: bool = False) -> Dict[str, torch.Tensor]:
    """pred, gt: dicts with scale [P], rotation [P,3,3], translation [P,3], half [P,3]; sym_type [P] = the pair's symmetry type ->
    re_deg, te, se, iou [P] float64, k_re, k_iou [P] int32 (module docstring).  Non-finite poses give NaN; a type outside the
    table gives NaN and k = -1.  ``table`` = (matrices [K,3,3], start [T], count [T]) replaces ``symmetry_table()``."""
    dev = sym_type.device
    table, start, count = symmetry_table(dev) if table is None else (t.to(dev) for t in table)
    p, g = _side(pred), _side(gt)
    if sym_type.is_cuda and not force_torch:
        return _hip().pose_pair_errors(p, g, sym_type, table, start, count)
    return _pose_pair_errors_torch(p, g, sym_type, table, start, count)


def _pose_pair_errors_torch(p, g, sym_type, table, start, count):
    dev = sym_type.device
    P, T = int(sym_type.numel()), int(start.numel())
    ty = sym_type.long()
    known = (ty >= 0) & (ty < T)
    tyc = ty.clamp(0, T - 1)
    first, cnt = start.long()[tyc], count.long()[tyc]
    box_p = _pose_box(*[p[i] for i in (0, 1, 2, 3)])
    nan = torch.full((P,), float("nan"), dtype=torch.float64, device=dev)
    best_re, best_iou = nan.clone(), nan.clone()
    k_re, k_iou = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    for k in range(int(cnt.max()) if P else 0):
        live = k < cnt
        F = table[first + torch.where(live, torch.full_like(cnt, k), torch.zeros_like(cnt))] @ g[1]
        M = p[1] @ F.transpose(1, 2)
        v = torch.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], dim=1) / 2.0
        tr = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
        re = torch.rad2deg(torch.atan2(torch.sqrt(_dot3(v, v)), (tr - 1.0) / 2.0))
        iou = _box_iou_torch(box_p, _pose_box(g[0], F, g[2], g[3]))
        if k == 0:
            best_re, best_iou = re, iou
            continue
        take = live & (re < best_re)                                                      # strict: the first extremum stays
        best_re, k_re = torch.where(take, re, best_re), torch.where(take, torch.full_like(k_re, k), k_re)
        take = live & (iou > best_iou)
        best_iou, k_iou = torch.where(take, iou, best_iou), torch.where(take, torch.full_like(k_iou, k), k_iou)
    d = p[2] - g[2]
    minus = torch.full_like(k_re, -1)
    return {"re_deg": torch.where(known, best_re, nan), "k_re": torch.where(known, k_re, minus),
            "te": torch.where(known, torch.sqrt(_dot3(d, d)), nan), "se": torch.where(known, (p[0] - g[0]).abs(), nan),
            "iou": torch.where(known, best_iou, nan), "k_iou": torch.where(known, k_iou, minus)}


# ------------------------------------------------------------------------------------------------ matching
@torch.no_grad()
def match_pairs(proposals: Union[Instances, Sequence[Instances]], iou_threshold: float = 0.5) -> Dict[str, torch.Tensor]:
    """The true positives of ``compute_ap_multi`` at ``iou_threshold``, restated (tests compare the two through the sequential walk):
    a proposal's candidate is the ground-truth instance of its own class and scene with the highest IoU (the first maximum); it
    counts if that IoU, compared in double, is > the threshold; of the proposals that count for the same instance the first in
    descending confidence (the order of one ``torch.argsort`` over all sets, as there) is the pair.
    -> set, proposal (index in its set), scene, instance (id in the scene), cls: int64 [Q], by set and proposal index."""
    sets: List[Instances] = [proposals] if isinstance(proposals, Instances) else list(proposals)
    dev = sets[0].score_preds.device if sets else torch.device("cpu")
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    n_total = sum(int(p.score_preds.shape[0]) for p in sets)
    if n_total == 0:
        return {k: empty for k in ("set", "proposal", "scene", "instance", "cls")}
    conf = torch.cat([p.score_preds for p in sets]).detach().float()
    order = torch.argsort(conf, descending=True)
    best, key, set_of, local, scene_of, inst_of, cls_of = [], [], [], [], [], [], []
    key_base = 0
    for i, p in enumerate(sets):
        n = int(p.score_preds.shape[0])
        labels = p.instance_sem_labels.to(dev)
        width = int(labels.shape[1]) if labels.dim() == 2 else 0
        cls = p.pt_sem_classes.long()
        if n and width:
            sample = p.batch_indices[p.proposal_offsets[:-1].long()].long()
            row = torch.where(labels[sample].long() == cls[:, None], p.ious.detach().float(), p.ious.new_zeros(()).float())
            top, arg = row.max(dim=1)
        else:
            sample = torch.zeros(n, dtype=torch.int64, device=dev)
            top, arg = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        best.append(top), key.append(key_base + sample * max(width, 1) + arg)
        set_of.append(torch.full((n,), i, dtype=torch.int64, device=dev)), local.append(torch.arange(n, device=dev))
        scene_of.append(sample), inst_of.append(arg), cls_of.append(cls)
        key_base += int(labels.shape[0]) * max(width, 1)
    best, key = torch.cat(best), torch.cat(key)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(n_total, device=dev)
    cand = best.double() > float(iou_threshold)
    first = torch.full((max(key_base, 1),), n_total, dtype=torch.int64, device=dev)
    first = first.scatter_reduce(0, key, torch.where(cand, rank, torch.full_like(rank, n_total)), "amin")
    rows = torch.nonzero(cand & (first[key] == rank)).squeeze(1)
    return {"set": torch.cat(set_of)[rows], "proposal": torch.cat(local)[rows], "scene": torch.cat(scene_of)[rows],
            "instance": torch.cat(inst_of)[rows], "cls": torch.cat(cls_of)[rows]}


# ------------------------------------------------------------------------------------------------ the evaluator
class PoseEvaluator:
    """Pose metrics of an epoch.  ``update(kept, batch)`` takes what ``test_step`` keeps of one batch (an ``Instances`` with
    score_preds, pt_sem_classes, batch_indices, proposal_offsets, instance_sem_labels, ious, pt_xyz, npcs_preds, npcs_valid_mask)
    and the batch it came from (points, batch_indices, batch_size, instance_labels, gt_npcs), on their device:
    match (``match_pairs``); ONE ``gpn_pose_fit`` over the matched proposals' points that carry a prediction (npcs_valid_mask),
    predicted NPCS - 0.5 as everywhere; ONE ``gpn_pose_gt_fit``; ONE ``gpn_pose_pair_errors``; append.  The predicted half extents
    are read off the fitted box (|corner i+1 - corner 0| / (2 s)).  ``picks(sizes) -> [Q,H,5]`` draws the RANSAC samples.
    In a test step ``npcs_valid_mask`` is the reference's: points whose predicted class is right and whose ground-truth NPCS is not
    zero, so the predicted pose is fitted on correctly classified points only - the ground truth chooses the points, not their
    values; the numbers are not a blind pose error.
    ``compute()`` makes one host read and returns, per class 1 .. num_classes-1 (arrays) and under "mean" over the classes that have
    pairs: Re [deg], Te, Se, mIoU, and A<deg> per threshold pair (the share of a class's pairs with re <= deg and te <= the
    distance); a class without pairs is NaN and left out of the mean.  Counts per class: "pairs" (both poses exist: what the
    metrics average over), "gt_instances", "dropped_no_pose" (matched, the prediction got no pose), "dropped_degenerate_gt"
    (matched, the ground truth has no pose).  ``scene_scale`` [scenes of a batch] multiplies te and se (the meta file's
    max_radius gives metres); default 1: the network's ball frame.  It can also be given per ``update``."""

    def __init__(self, num_classes: int, symmetry_indices, picks: Callable = draw_picks, scene_scale=None,
                 thresholds=((5, 0.05), (10, 0.10)), iou_threshold: float = 0.5, force_torch: bool = False):
        self.num_classes = int(num_classes)
        self.force_torch = bool(force_torch)    # the torch formulation of the three new stages on GPU tensors too
        self.symmetry_indices = torch.as_tensor(symmetry_indices, dtype=torch.int64)
        self.picks, self.scene_scale = picks, scene_scale
        self.thresholds = tuple((float(a), float(d)) for a, d in thresholds)
        self.iou_threshold = float(iou_threshold)
        self._rows: List[torch.Tensor] = []     # per update [Q,7] f64: cls, re, te, se, iou, pred valid, gt valid
        self._gt_counts: List[torch.Tensor] = []
        self.num_scenes = 0                     # scenes seen by update

    @torch.no_grad()
    def update(self, kept: Optional[Instances], batch, scene_scale=None) -> None:
        dev, f64 = batch.points.device, torch.float64
        labels = batch.instance_sem_labels if getattr(batch, "instance_sem_labels", None) is not None else kept.instance_sem_labels
        labels = labels.to(dev).long()
        S, W = int(labels.shape[0]), int(labels.shape[1]) if labels.dim() == 2 else 0
        self.num_scenes += S
        cls_ids = torch.arange(1, self.num_classes, device=dev)
        self._gt_counts.append((labels.reshape(-1)[None, :] == cls_ids[:, None]).sum(1).to(f64))
        if kept is None or kept.score_preds is None or kept.score_preds.shape[0] == 0 or W == 0:
            return
        m = match_pairs(kept, self.iou_threshold)
        Q = int(m["proposal"].shape[0])
        if Q == 0:
            return
        # ---- the matched proposals' points that carry a prediction ----
        po = kept.proposal_offsets.to(dev).long()
        P, M = int(po.shape[0]) - 1, int(kept.pt_xyz.shape[0])
        mask = kept.npcs_valid_mask.to(dev).bool() if kept.npcs_valid_mask is not None else torch.ones(M, dtype=torch.bool, device=dev)
        npcs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
        if kept.npcs_preds is not None:
            npcs[mask] = kept.npcs_preds.to(dev).float()
        pair_of_proposal = torch.full((P,), -1, dtype=torch.int64, device=dev)
        pair_of_proposal[m["proposal"]] = torch.arange(Q, device=dev)
        pair_of_point = pair_of_proposal[torch.bucketize(torch.arange(M, device=dev), po[1:], right=True).clamp(max=max(P - 1, 0))]
        rows = torch.nonzero(mask & (pair_of_point >= 0)).squeeze(1)   # (proposal by proposal, so pair by pair: m is by proposal)
        sizes = torch.bincount(pair_of_point[rows], minlength=Q)
        fitted = torch.nonzero(sizes > 0).squeeze(1)
        nan = float("nan")
        pred = {"scale": torch.full((Q,), nan, dtype=f64, device=dev), "rotation": torch.full((Q, 3, 3), nan, dtype=f64, device=dev),
                "translation": torch.full((Q, 3), nan, dtype=f64, device=dev), "half": torch.full((Q, 3), nan, dtype=f64, device=dev)}
        pred_valid = torch.zeros(Q, dtype=torch.bool, device=dev)
        if fitted.numel():
            live = sizes[fitted]
            offsets = torch.zeros(int(fitted.numel()) + 1, dtype=torch.int64, device=dev)
            offsets[1:] = live.cumsum(0)
            picks = self.picks(live.tolist())
            fit = estimate_pose_from_npcs_batched(kept.pt_xyz.to(dev)[rows].contiguous(), (npcs[rows] - 0.5).contiguous(), offsets,
                                                  picks=picks)
            box = fit["bbox"]
            edge = box[:, 1:4] - box[:, :1]
            pred["scale"][fitted], pred["rotation"][fitted], pred["translation"][fitted] = fit["scale"], fit["rotation"], fit["translation"]
            pred["half"][fitted] = torch.sqrt(_dot3(edge, edge)) / (2.0 * fit["scale"][:, None])
            pred_valid[fitted] = fit["valid"]
        # ---- ground truth, errors ----
        off = torch.searchsorted(batch.batch_indices.to(dev).long().contiguous(), torch.arange(S + 1, device=dev))
        gt_all = gt_part_poses(batch.points[:, :3], batch.gt_npcs, batch.instance_labels, off, W, force_torch=self.force_torch)
        slot = m["scene"] * W + m["instance"]
        gt = {k: gt_all[k][slot] for k in ("scale", "rotation", "translation", "half")}
        err = pose_pair_errors(pred, gt, self.symmetry_indices.to(dev)[m["cls"]].to(torch.int32), force_torch=self.force_torch)
        scale = scene_scale if scene_scale is not None else self.scene_scale
        unit = torch.ones(Q, dtype=f64, device=dev) if scale is None else torch.as_tensor(scale, dtype=f64).to(dev)[m["scene"]]
        self._rows.append(torch.stack([m["cls"].to(f64), err["re_deg"], err["te"] * unit, err["se"] * unit, err["iou"],
                                       pred_valid.to(f64), gt_all["valid"][slot].to(f64)], dim=1))

    def compute(self) -> Dict[str, object]:
        C = self.num_classes - 1
        dev = self._gt_counts[0].device if self._gt_counts else torch.device("cpu")
        gt_counts = torch.stack(self._gt_counts).sum(0) if self._gt_counts else torch.zeros(C, dtype=torch.float64, device=dev)
        rows = torch.cat(self._rows) if self._rows else torch.zeros(0, 7, dtype=torch.float64, device=dev)
        host = torch.cat([gt_counts.reshape(-1), rows.reshape(-1)]).cpu().numpy()          # the one host read
        gt_counts, rows = host[:C], host[C:].reshape(-1, 7)
        cls, ok_p, ok_g = rows[:, 0].astype(np.int64), rows[:, 5] > 0, rows[:, 6] > 0
        names = ["Re", "Te", "Se", "mIoU"] + [f"A{a:g}" for a, _ in self.thresholds]
        out: Dict[str, object] = {k: np.full(C, np.nan) for k in names}
        for k in ("pairs", "dropped_no_pose", "dropped_degenerate_gt"):
            out[k] = np.zeros(C, dtype=np.int64)
        out["gt_instances"] = gt_counts.astype(np.int64)
        out["classes"] = list(range(1, self.num_classes))
        for c in range(1, self.num_classes):
            of = cls == c
            out["dropped_no_pose"][c - 1] = int((of & ~ok_p).sum())
            out["dropped_degenerate_gt"][c - 1] = int((of & ~ok_g).sum())
            r = rows[of & ok_p & ok_g]
            out["pairs"][c - 1] = r.shape[0]
            if r.shape[0] == 0:
                continue
            for j, k in enumerate(("Re", "Te", "Se", "mIoU")):
                out[k][c - 1] = r[:, 1 + j].mean()
            for a, d in self.thresholds:
                out[f"A{a:g}"][c - 1] = ((r[:, 1] <= a) & (r[:, 2] <= d)).mean()
        have = out["pairs"] > 0
        out["mean"] = {k: float(out[k][have].mean()) if have.any() else float("nan") for k in names}
        out["total_pairs"] = int(out["pairs"].sum())
        return out
