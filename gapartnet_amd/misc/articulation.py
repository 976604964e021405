"""Articulation from two frames: which parts moved, about which axis, by how much (include/gpn.h section AR).

Two RGB-D frames of one object, before and after something moved, give two sets of parts with unrelated numbering
(``PartPredictor.predict_frames``).  ``estimate_joints`` (section JE) takes ONE part and asks for its points in each frame, as the
reference's ``estimate_joint_angle`` does ("only part, please segment first", structure/gapartnet.py:829).  This module is what lies
between: the parts of frame A are associated with the parts of frame B, every matched part's pixels are cut out of both frames, and
ONE joint pass runs over all matched pairs of all frame pairs.

  match_parts              instance maps + classes of both frames -> the matched (i, j), their 2D IoU, the unmatched parts
  articulation_from_maps   depth + instance maps + classes of both frames -> a joint per matched pair
  articulation_from_frames the same from a ``PartPredictor`` and the raw frames
  draw_articulation        the joints of one frame pair drawn on frame A

The association is GREEDY one-to-one matching by exact 2D mask IoU (the contract is in include/gpn.h): pairs of equal class with
``inter >= min_iou * union``, the largest IoU first, ties to the smaller i, then the smaller j.  Not the optimal assignment, on
purpose: it is the rule the AP matching of this project uses, it is a total order and it needs no floating-point cost.  A part
that moved across the image, so that its two masks do not overlap, is not matched; a STATIC CAMERA is assumed throughout, as in the
reference, whose joint is expressed in the one camera frame both observations share.

On GPU tensors the maps never leave the device: ``gpn_parts_overlap`` and ``gpn_parts_match`` produce the small tables, which are
read in ONE copy (they size the clouds and draw the picks, as ``estimate_joints`` needs the sizes on the host), ``gpn_parts_gather``
writes both sides' ragged clouds, and ``estimate_joints_packed`` runs once.  On CPU tensors the same contract runs in numpy.

The joint type comes from the part class (``JOINT_TYPE_OF_CLASS``): sliders are prismatic, hinges and the revolute handle are
revolute, fixed handles and ``others`` are fixed - their joint is NaN, but their rigid transform is still reported, because it
tells the caller whether the whole object moved.
"""
import argparse
import functools
import os
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import info
from .joint_fitting import JointLeg, _lists, _maps, _need_hip, draw_joint, estimate_joints_packed, joint_from_rigid

PARTS_MAX = 64  # GPN_PARTS_MAX
FIXED, REVOLUTE, PRISMATIC = "fixed", "revolute", "prismatic"
_TYPE_OF_NAME = {"others": FIXED, "line_fixed_handle": FIXED, "round_fixed_handle": FIXED, "slider_button": PRISMATIC,
                 "hinge_door": REVOLUTE, "slider_drawer": PRISMATIC, "slider_lid": PRISMATIC, "hinge_lid": REVOLUTE,
                 "hinge_knob": REVOLUTE, "revolute_handle": REVOLUTE}
JOINT_TYPE_OF_CLASS = {info.PART_NAME2ID[name]: kind for name, kind in _TYPE_OF_NAME.items()}


@dataclass
class PartMatches:
    """per frame pair v (host arrays): ``pairs[v]`` [M,2] i64 = the matched (i, j) in ascending i; ``inter[v]``, ``union[v]`` [M] i64
    pixels; ``iou[v]`` [M] f64 = inter / union; ``unmatched_a[v]``, ``unmatched_b[v]`` i64; ``area_a[v]`` [n_a], ``area_b[v]`` [n_b] i64"""
    pairs: List[np.ndarray]
    inter: List[np.ndarray]
    union: List[np.ndarray]
    iou: List[np.ndarray]
    unmatched_a: List[np.ndarray]
    unmatched_b: List[np.ndarray]
    area_a: List[np.ndarray]
    area_b: List[np.ndarray]


@dataclass
class Articulation:
    """the G matched pairs of the whole batch in (frame, i) order.  Host arrays: ``frame``, ``part_a`` (i), ``part_b`` (j),
    ``part_class`` [G] i64, ``joint_type`` (G strings: "revolute" / "prismatic" / "fixed"), ``iou2d`` [G] f64, ``n_points_a``,
    ``n_points_b`` [G] i64.  On the frames' device: ``cpd`` and ``ransac`` (``JointLeg``: axis [G,3], pivot [G,3], angle [G] - the
    displacement of a prismatic pair, NaN for a fixed one - and the rigid transform of every pair, fixed ones included),
    ``iterations`` [G] i32, ``norm`` [G,4] = (S, Mx, My, Mz).  ``matches``: the ``PartMatches`` behind them."""
    frame: np.ndarray
    part_a: np.ndarray
    part_b: np.ndarray
    part_class: np.ndarray
    joint_type: List[str]
    iou2d: np.ndarray
    n_points_a: np.ndarray
    n_points_b: np.ndarray
    cpd: JointLeg
    ransac: JointLeg
    iterations: torch.Tensor
    norm: torch.Tensor
    matches: PartMatches

    def to_numpy(self) -> dict:
        out = {f: getattr(self, f) for f in ("frame", "part_a", "part_b", "part_class", "iou2d", "n_points_a", "n_points_b")}
        out["joint_type"] = np.array(self.joint_type, dtype="U9")
        out["iterations"], out["norm"] = self.iterations.cpu().numpy(), self.norm.cpu().numpy()
        for name, leg in (("cpd", self.cpd), ("ransac", self.ransac)):
            for f in ("axis", "pivot", "angle", "scale", "rotation", "translation"):
                out[f"{name}_{f}"] = getattr(leg, f).cpu().numpy()
        return out


# ------------------------------------------------------------------------------------------------------------ inputs
def _class_table(classes: list, P: int, dev) -> torch.Tensor:
    """[V,P] i32 on ``dev``, -1 beyond a list's end; device lists are padded on the device (no host read)"""
    table = torch.full((len(classes), P), -1, dtype=torch.int32, device=dev)
    for v, c in enumerate(classes):
        if int(c.shape[0]):
            table[v, :int(c.shape[0])] = c.to(dev, non_blocking=True).to(torch.int32)
    return table


# ------------------------------------------------------------------------------------------------------------ the CPU path
def _keys_numpy(inst: np.ndarray, valid: np.ndarray, n: int) -> np.ndarray:
    """the membership rule: the part of every pixel, or -1"""
    inst = inst.astype(np.int64)
    return np.where((valid != 0) & (inst >= 0) & (inst < n), inst, -1)


def _overlap_numpy(inst_a, valid_a, n_a, inst_b, valid_b, n_b, PA: int, PB: int):
    V = inst_a.shape[0]
    inter, area_a, area_b = np.zeros((V, PA, PB), np.int32), np.zeros((V, PA), np.int32), np.zeros((V, PB), np.int32)
    for v in range(V):
        ka = _keys_numpy(inst_a[v].reshape(-1), valid_a[v].reshape(-1), n_a[v])
        kb = _keys_numpy(inst_b[v].reshape(-1), valid_b[v].reshape(-1), n_b[v])
        area_a[v] = np.bincount(ka[ka >= 0], minlength=PA)[:PA]
        area_b[v] = np.bincount(kb[kb >= 0], minlength=PB)[:PB]
        both = (ka >= 0) & (kb >= 0)
        inter[v] = np.bincount(ka[both] * PB + kb[both], minlength=PA * PB).reshape(PA, PB)
    return inter, area_a, area_b


def _before(p, q) -> int:
    """the order of the greedy matching on (inter, union, i, j): the larger IoU first, exactly, then the smaller i, then j"""
    l, r = p[0] * q[1], q[0] * p[1]
    if l != r:
        return -1 if l > r else 1
    return -1 if p[2:] < q[2:] else (1 if p[2:] > q[2:] else 0)


def _match_numpy(inter, area_a, area_b, n_a, n_b, cls_a, cls_b, min_iou: float):
    V, PA, PB = inter.shape
    match_ab, match_ba = np.full((V, PA), -1, np.int32), np.full((V, PB), -1, np.int32)
    m_inter, m_union = np.zeros((V, PA), np.int32), np.zeros((V, PA), np.int32)
    for v in range(V):
        cand = []
        for i in range(min(int(n_a[v]), PA)):
            for j in range(min(int(n_b[v]), PB)):
                c = int(inter[v, i, j])
                u = int(area_a[v, i]) + int(area_b[v, j]) - c
                if cls_a[v, i] == cls_b[v, j] and c > 0 and float(c) >= float(min_iou) * float(u):
                    cand.append((c, u, i, j))
        # (the order is total and does not depend on what is matched: walking the sorted list IS the repeated arg-max)
        for c, u, i, j in sorted(cand, key=functools.cmp_to_key(_before)):
            if match_ab[v, i] < 0 and match_ba[v, j] < 0:
                match_ab[v, i], match_ba[v, j], m_inter[v, i], m_union[v, i] = j, i, c, u
    return match_ab, match_ba, m_inter, m_union


# ------------------------------------------------------------------------------------------------------------ matching
def _match_tables(inst_a, valid_a, cls_a: list, inst_b, valid_b, cls_b: list, min_iou: float):
    """-> host arrays (match_ab [V,PA], m_inter [V,PA], m_union [V,PA], area_a [V,PA], area_b [V,PB], ca [V,PA], cb [V,PB]); on the GPU
    the ONE host read of the call"""
    dev = inst_a.device
    V = int(inst_a.shape[0])
    n_a, n_b = [int(c.shape[0]) for c in cls_a], [int(c.shape[0]) for c in cls_b]
    PA, PB = max(n_a, default=0), max(n_b, default=0)
    ca, cb = _class_table(cls_a, PA, dev), _class_table(cls_b, PB, dev)
    if dev.type == "cuda":
        hip = _need_hip("match_parts")
        inter, area_a, area_b = hip.parts_overlap(inst_a, valid_a, n_a, inst_b, valid_b, n_b, PA, PB)
        m = hip.parts_match(inter, area_a, area_b, n_a, n_b, ca, cb, min_iou)
        flat = torch.cat([t.reshape(-1) for t in (m["match_ab"], m["inter"], m["union"], area_a, ca, area_b, cb)]).cpu().numpy()
        a, b = flat[:5 * V * PA].reshape(5, V, PA), flat[5 * V * PA:].reshape(2, V, PB)
        return a[0], a[1], a[2], a[3], b[0], a[4], b[1]
    ca, cb = ca.numpy(), cb.numpy()
    inter, area_a, area_b = _overlap_numpy(inst_a.numpy(), valid_a.numpy(), n_a, inst_b.numpy(), valid_b.numpy(), n_b, PA, PB)
    match_ab, _, m_inter, m_union = _match_numpy(inter, area_a, area_b, n_a, n_b, ca, cb, min_iou)
    return match_ab, m_inter, m_union, area_a, area_b, ca, cb


def _part_matches(match_ab, m_inter, m_union, area_a, area_b, n_a, n_b) -> PartMatches:
    out = PartMatches([], [], [], [], [], [], [], [])
    for v in range(match_ab.shape[0]):
        i = np.flatnonzero(match_ab[v, :n_a[v]] >= 0).astype(np.int64)
        j = match_ab[v, i].astype(np.int64)
        out.pairs.append(np.stack([i, j], 1))
        out.inter.append(m_inter[v, i].astype(np.int64))
        out.union.append(m_union[v, i].astype(np.int64))
        out.iou.append(out.inter[-1].astype(np.float64) / out.union[-1].astype(np.float64))
        out.unmatched_a.append(np.flatnonzero(match_ab[v, :n_a[v]] < 0).astype(np.int64))
        out.unmatched_b.append(np.setdiff1d(np.arange(n_b[v], dtype=np.int64), j))
        out.area_a.append(area_a[v, :n_a[v]].astype(np.int64))
        out.area_b.append(area_b[v, :n_b[v]].astype(np.int64))
    return out


def _checked_maps(inst_a, inst_b, classes_a, classes_b, valid_a, valid_b):
    inst_a, inst_b = _maps(inst_a, "inst_a"), _maps(inst_b, "inst_b")
    if inst_a.shape != inst_b.shape or inst_a.device != inst_b.device:
        raise ValueError("both frames of a pair have one size and live on one device")
    V = int(inst_a.shape[0])
    cls_a, cls_b = _lists(classes_a, V, "classes_a", PARTS_MAX), _lists(classes_b, V, "classes_b", PARTS_MAX)
    valid = []
    for inst, val in ((inst_a, valid_a), (inst_b, valid_b)):
        val = (inst >= 0) if val is None else torch.as_tensor(val).reshape(inst.shape).to(inst.device)
        valid.append(val.to(torch.uint8))
    return inst_a, inst_b, cls_a, cls_b, valid[0], valid[1]


@torch.no_grad()
def match_parts(inst_a, inst_b, classes_a, classes_b, valid_a=None, valid_b=None, min_iou: float = 0.1) -> PartMatches:
    """``inst`` [V,H,W] (or [H,W]) integer maps - pixel -> the part's position in the frame's class list, anything else: no part -
    and one class list per frame and side (``FramePrediction.instance`` / ``.proposal_classes``); ``valid`` [V,H,W] defaults to
    ``inst >= 0``.  -> ``PartMatches``: greedy one-to-one matching by exact 2D mask IoU among pairs of equal class with
    ``inter >= min_iou * union`` (include/gpn.h section AR).  ``min_iou`` = 0.1 is a convention, like the evaluator's thresholds.
    GPU maps: two launches and one host read; CPU maps: numpy."""
    inst_a, inst_b, cls_a, cls_b, valid_a, valid_b = _checked_maps(inst_a, inst_b, classes_a, classes_b, valid_a, valid_b)
    match_ab, m_inter, m_union, area_a, area_b, _, _ = _match_tables(inst_a, valid_a, cls_a, inst_b, valid_b, cls_b, float(min_iou))
    return _part_matches(match_ab, m_inter, m_union, area_a, area_b, [int(c.shape[0]) for c in cls_a], [int(c.shape[0]) for c in cls_b])


# ------------------------------------------------------------------------------------------------------------ joints
def _empty_articulation(matches: PartMatches, dev) -> Articulation:
    f64 = torch.float64
    z = lambda *s: torch.zeros(s, dtype=f64, device=dev)  # noqa: E731
    leg = lambda: JointLeg(z(0, 3), z(0, 3), z(0), z(0), z(0, 3, 3), z(0, 3))  # noqa: E731
    e = np.zeros(0, np.int64)
    return Articulation(e, e.copy(), e.copy(), e.copy(), [], np.zeros(0, np.float64), e.copy(), e.copy(), leg(), leg(),
                        torch.zeros(0, dtype=torch.int32, device=dev), z(0, 4), matches)


@torch.no_grad()
def articulation_from_maps(depth_a, depth_b, K, inst_a, inst_b, classes_a, classes_b, depth_scale: float = 1.0, flip: bool = False,
                           min_iou: float = 0.1, sample_number: int = 500, picks=None, ransac_picks=None, **cpd_kwargs) -> Articulation:
    """two depth frames [H,W] (or V frame pairs [V,H,W]) of one STATIC camera ``K``, with each frame's instance map and class list
    (``match_parts``) -> the joint of every matched pair.  Both frames are back-projected (section FR; a pixel without depth
    belongs to no part), the parts are matched, the matched parts' pixels become the ragged clouds of ONE ``estimate_joints_packed``
    pass over the G pairs of the whole batch in (frame, i) order; ``picks`` / ``ransac_picks`` are that pass's (drawn when None,
    ``sample_number`` rows a side), ``cpd_kwargs`` its ``max_iterations``, ``tolerance`` and ``w``.  The joint type follows the part
    class (``JOINT_TYPE_OF_CLASS``; a class outside the table is fixed).  As in ``estimate_joints`` the registration moves the second
    observation onto the first (TY = s Y R + t with Y from frame B): a prismatic axis points from the part's place in B to its
    place in A.  On the GPU: ONE host read (the match and area tables) in
    front of the joint pass."""
    from .. import inference
    (da, _, Kc, _), (db, _, _, _) = (inference._check_frames(d, None, K, None) for d in (depth_a, depth_b))
    inst_a, inst_b = _maps(inst_a, "inst_a"), _maps(inst_b, "inst_b")
    if not (da.shape == db.shape == inst_a.shape == inst_b.shape) or len({t.device for t in (da, db, inst_a, inst_b)}) != 1:
        raise ValueError("the depth frames and instance maps of both sides have one shape and live on one device")
    V, H, W = (int(v) for v in da.shape)
    dev = da.device
    cls_a, cls_b = _lists(classes_a, V, "classes_a", PARTS_MAX), _lists(classes_b, V, "classes_b", PARTS_MAX)
    n_a, n_b = [int(c.shape[0]) for c in cls_a], [int(c.shape[0]) for c in cls_b]
    # ---- 1. back-projection ----
    hip = _need_hip("articulation_from_maps") if dev.type == "cuda" else None
    (rows_a, valid_a, _), (rows_b, valid_b, _) = (inference.backproject_frames(d, None, Kc, None, depth_scale, flip) for d in (da, db))
    # ---- 2 + 3. overlap, match, the one host read ----
    match_ab, m_inter, m_union, area_a, area_b, ca, _ = _match_tables(inst_a, valid_a, cls_a, inst_b, valid_b, cls_b, float(min_iou))
    matches = _part_matches(match_ab, m_inter, m_union, area_a, area_b, n_a, n_b)
    # ---- 4. the pairs of the batch in (frame, i) order; their segments are consecutive ----
    frame = np.concatenate([np.full(len(p), v, np.int64) for v, p in enumerate(matches.pairs)]) if V else np.zeros(0, np.int64)
    G = int(frame.shape[0])
    if G == 0:
        return _empty_articulation(matches, dev)
    pairs = np.concatenate(matches.pairs)
    part_a, part_b = pairs[:, 0], pairs[:, 1]
    sizes1, sizes2 = area_a[frame, part_a].astype(np.int64), area_b[frame, part_b].astype(np.int64)
    off1, off2 = np.concatenate([[0], np.cumsum(sizes1)]), np.concatenate([[0], np.cumsum(sizes2)])
    seg_a, seg_b = np.full((V, max(n_a)), -1, np.int64), np.full((V, max(n_b)), -1, np.int64)
    seg_a[frame, part_a], seg_b[frame, part_b] = off1[:-1], off2[:-1]
    # ---- 5. gather ----
    if dev.type == "cuda":
        pc1 = hip.parts_gather(rows_a, inst_a, valid_a, n_a, torch.from_numpy(seg_a), int(off1[-1]))
        pc2 = hip.parts_gather(rows_b, inst_b, valid_b, n_b, torch.from_numpy(seg_b), int(off2[-1]))
    else:
        clouds = []
        for rows, inst, valid, n, parts in ((rows_a, inst_a, valid_a, n_a, part_a), (rows_b, inst_b, valid_b, n_b, part_b)):
            xyz = rows.numpy()[:, :3].reshape(V, H * W, 3)
            keys = [_keys_numpy(inst[v].numpy().reshape(-1), valid[v].numpy().reshape(-1), n[v]) for v in range(V)]
            clouds.append(torch.from_numpy(np.concatenate([xyz[v][keys[v] == p] for v, p in zip(frame, parts)]).astype(np.float64)))
        pc1, pc2 = clouds
    # ---- 6. one joint pass ----
    est = estimate_joints_packed(pc1, pc2, sizes1.tolist(), sizes2.tolist(), sample_number, picks, ransac_picks, REVOLUTE, **cpd_kwargs)
    part_class = ca[frame, part_a].astype(np.int64)
    kinds = [JOINT_TYPE_OF_CLASS.get(int(c), FIXED) for c in part_class]
    pris = torch.tensor([k == PRISMATIC for k in kinds]).to(dev, non_blocking=True)
    fixed = torch.tensor([k == FIXED for k in kinds]).to(dev, non_blocking=True)
    legs = []
    for leg in (est.cpd, est.ransac):
        axis, pivot, angle = leg.axis, leg.pivot, leg.angle
        if PRISMATIC in kinds:
            p_axis, p_pivot, p_angle = joint_from_rigid(leg.rotation, leg.translation, est.norm, PRISMATIC)
            axis, pivot = torch.where(pris[:, None], p_axis, axis), torch.where(pris[:, None], p_pivot, pivot)
            angle = torch.where(pris, p_angle, angle)
        nan = torch.full_like(angle, float("nan"))
        legs.append(JointLeg(torch.where(fixed[:, None], nan[:, None], axis), torch.where(fixed[:, None], nan[:, None], pivot),
                             torch.where(fixed, nan, angle), leg.scale, leg.rotation, leg.translation))
    return Articulation(frame, part_a, part_b, part_class, kinds, np.concatenate(matches.iou), sizes1, sizes2, legs[0], legs[1],
                        est.iterations, est.norm, matches)


@torch.no_grad()
def articulation_from_frames(predictor, depth_a, rgb_a, depth_b, rgb_b, K, presample: int = 4, seed=0, isolate=None,
                             sampler: Optional[str] = None, frame_picks=None, depth_scale: float = 1.0, flip: bool = False, **kw):
    """``predictor.predict_frames`` on both frames (``presample``, ``seed``, ``isolate``, ``depth_scale``, ``flip`` and ``frame_picks``
    - its ``picks`` - go to it; ``sampler``: another sampler than the predictor's), then ``articulation_from_maps`` on their
    ``instance`` maps and ``proposal_classes`` (``kw``).  -> (frames_a, frames_b, articulation)"""
    predictor = predictor.with_sampler(sampler)
    shared = dict(picks=frame_picks, presample=presample, seed=seed, depth_scale=depth_scale, flip=flip, isolate=isolate)
    frames_a = predictor.predict_frames(depth_a, rgb_a, K, **shared)
    frames_b = predictor.predict_frames(depth_b, rgb_b, K, **shared)
    art = articulation_from_maps(depth_a, depth_b, K, torch.stack([f.instance for f in frames_a]), torch.stack([f.instance for f in frames_b]),
                                 [f.proposal_classes for f in frames_a], [f.proposal_classes for f in frames_b], depth_scale=depth_scale,
                                 flip=flip, **kw)
    return frames_a, frames_b, art


def draw_articulation(rgb, K, articulation: Articulation, frame: int = 0) -> np.ndarray:
    """a copy of frame A's ``rgb`` [H,W,3] u8 with the CPD axis of every non-fixed pair of frame pair ``frame`` drawn by ``draw_joint``
    (a joint that is not finite draws nothing)"""
    img = np.array(torch.as_tensor(rgb).detach().cpu().numpy(), dtype=np.uint8, copy=True)
    axis, pivot = articulation.cpd.axis.cpu().numpy(), articulation.cpd.pivot.cpu().numpy()
    for g in np.flatnonzero(articulation.frame == frame):
        if articulation.joint_type[g] != FIXED and np.isfinite(axis[g]).all() and np.isfinite(pivot[g]).all():
            img = draw_joint(img, K, axis[g], pivot[g])
    return img


# ------------------------------------------------------------------------------------------------------------ command line
def main(argv: Optional[Sequence[str]] = None) -> int:
    from .. import inference
    ap = argparse.ArgumentParser(prog="python -m gapartnet_amd.misc.articulation",
                                 description="which parts moved between two RGB-D frames of one static camera, about which axis, by how much")
    ap.add_argument("--depth", nargs=2, required=True, help="the two depth maps (.png 16-bit / .npy), before and after")
    ap.add_argument("--rgb", nargs=2, help="the two images (needed with --ckpt; the first is drawn into)")
    ap.add_argument("--intrinsics", required=True, help="3x3 camera matrix as text or .npy")
    ap.add_argument("--ckpt", help="checkpoint: the parts are predicted")
    ap.add_argument("--instances", nargs=2, help="instead of --ckpt: the two [H,W] integer instance maps (.npy)")
    ap.add_argument("--classes", nargs=2, help="with --instances: the two class lists (.npy)")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--depth_scale", type=float, default=1.0)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--min_iou", type=float, default=0.1)
    ap.add_argument("--sample_number", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--presample", type=int, default=4)
    ap.add_argument("--sampler", default="fps", choices=("fps", "grid"))
    ap.add_argument("--isolate", action="store_true", help="with --ckpt: cut the object out of the raw frames first")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args(argv)
    if (args.ckpt is None) == (args.instances is None):
        ap.error("give --ckpt, or --instances with --classes")
    if args.instances is not None and args.classes is None:
        ap.error("--instances needs --classes")
    if args.ckpt is not None and args.rgb is None:
        ap.error("--ckpt needs --rgb")
    random.seed(args.seed)
    np.random.seed(args.seed)
    dev = torch.device(args.device)
    depth = [inference._read_depth(p) for p in args.depth]
    if depth[0].shape != depth[1].shape or depth[0].dtype != depth[1].dtype:
        ap.error("the two depth maps have one size and type")
    K = (np.load(args.intrinsics) if args.intrinsics.endswith(".npy") else np.loadtxt(args.intrinsics)).astype(np.float64).reshape(3, 3)
    rgb = None if args.rgb is None else [np.ascontiguousarray(inference._read_image(p)[..., :3]).astype(np.uint8) for p in args.rgb]
    da, db = (torch.from_numpy(d[None]).to(dev) for d in depth)
    kw = dict(depth_scale=args.depth_scale, flip=args.flip, min_iou=args.min_iou, sample_number=args.sample_number)
    if args.ckpt is not None:
        model = inference.load_model(args.ckpt, dev)
        predictor = inference.PartPredictor(model, num_points=args.num_points, sampler=args.sampler)
        ca, cb = (torch.from_numpy(c[None]).to(dev) for c in rgb)
        _, _, art = articulation_from_frames(predictor, da, ca, db, cb, K, presample=args.presample, seed=args.seed,
                                             isolate=inference.IsolateConfig() if args.isolate else None, **kw)
    else:
        inst = [torch.from_numpy(np.load(p).astype(np.int64)[None]).to(dev) for p in args.instances]
        cls = [[np.load(p).astype(np.int64).reshape(-1)] for p in args.classes]
        art = articulation_from_maps(da, db, K, inst[0], inst[1], cls[0], cls[1], **kw)
    os.makedirs(args.out, exist_ok=True)
    name = os.path.splitext(os.path.basename(args.depth[0]))[0]
    path = os.path.join(args.out, f"{name}_articulation.npz")
    cpd = art.to_numpy()
    np.savez(path, **cpd)
    print(path)
    for g in range(len(art.joint_type)):
        print(f"part {int(art.part_a[g])} -> {int(art.part_b[g])} ({info.PART_ID2NAME.get(int(art.part_class[g]), '?')}, IoU {art.iou2d[g]:.3f}): "
              f"{art.joint_type[g]}, axis {cpd['cpd_axis'][g].tolist()}, pivot {cpd['cpd_pivot'][g].tolist()}, angle {float(cpd['cpd_angle'][g]):.6f}")
    if rgb is None:  # (no image given: the joints are drawn on the depth map, as grey levels)
        d = depth[0].astype(np.float64)
        top = d.max() if d.max() > 0 else 1.0
        rgb = [np.repeat(np.rint(d / top * 255.0).astype(np.uint8)[..., None], 3, 2)]
    from PIL import Image
    path = os.path.join(args.out, f"{name}_articulation.png")
    Image.fromarray(draw_articulation(rgb[0], K, art, 0)).save(path)
    print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
