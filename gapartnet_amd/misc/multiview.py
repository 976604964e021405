"""Parts of one object from several posed RGB-D views (include/gpn.h section MV).

``predict_frames`` gives per-pixel parts and camera-frame boxes for each frame on its own: K posed views of one object give K
unrelated part lists, whose numbers do not correspond and whose boxes are fitted on the one side of the part the view saw.  This
module fuses them: ONE list of the object's parts in the world frame, every part knowing its mask in every view, its box fitted once
on the points of all views (NPCS is canonical per part, so the union cloud is a valid input to the existing fit).

  fuse_parts    depth + instance maps + class lists + poses of V views -> ``FusedParts``
  fuse_frames   the same from a ``PartPredictor`` and the raw frames
  draw_fused    the fused boxes projected into one view

Poses are the renderer's (``camera_frame`` in dataset/render_assets.py; ``world2camera_rotation`` and ``camera2world_translation``
of ``write_view``): a camera point is ``(world - t) @ R``, so ``world = cam @ R^T + t``.

The association is GREEDY SINGLE LINKAGE over voxel occupancy (the contract is in include/gpn.h): every member pixel goes to the
world frame and into a grid of 1024 cells of edge ``cell`` an axis, anchored at the minimum of all member points; two parts of equal
class are a candidate pair when they share at least ``min_inter`` voxels and at least ``min_overlap`` of the SMALLER part's voxels
(two views see different faces of one part); candidates are united in the order of that ratio, exactly, ties to the smaller global
part number - unless the two clusters already hold a part of one and the same view.  Not an optimal assignment, on purpose.
LIMITS: at most 64 views, at most 512 parts over all views, one object per call; a member pixel beyond the 1024th cell of an axis is
left out of the occupancy (it stays a member of its part) and counted in ``dropped``.  The defaults of ``cell``, ``min_inter`` and
``min_overlap`` are NOT tuned on real data.

On GPU tensors the maps never leave the device: four entry points produce the small tables, which are read in ONE copy (they size
the clouds and draw the picks), ``gpn_views_gather`` writes the fused parts' clouds and one ``estimate_pose_from_npcs_batched`` pass
fits all boxes.  On CPU tensors the same contract runs in numpy.
"""
import argparse
import functools
import json
import os
import random
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .joint_fitting import _lists, _maps, _need_hip
from .pose_fitting_batched import draw_picks, estimate_pose_from_npcs_batched

VIEWS_MAX = 64        # GPN_VIEWS_MAX
FUSE_PARTS_MAX = 512  # GPN_FUSE_PARTS_MAX
GRID_CELLS = 1024
DEAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


@dataclass
class FusedParts:
    """the F fused parts of one object.  On the views' device: ``fused_inst`` [V,H,W] i32 (the fused part of every pixel, -1 where
    none: ids are consistent across views), ``score`` [F] f32 (the maximum of the members' scores, NaN without scores), ``valid`` [F]
    bool, ``bbox`` [F,8,3], ``scale`` [F], ``rotation`` [F,3,3], ``translation`` [F,3] f64 - the similarity world ~ (npcs - 0.5) @
    (s R) + t and its box in the WORLD frame, NaN where not valid (fewer than 5 points, no fit, or no ``npcs`` given) -
    ``member_xyz`` [M,3] f64 (world), ``member_npcs`` [M,3] f64 or None, ``member_src`` [M] i64 (= view * H * W + pixel), fused part f
    = rows ``member_offsets[f]:member_offsets[f + 1]`` in ascending (view, pixel) order.  Host arrays: ``part_class`` [F] i64,
    ``n_views`` [F] i64, ``parts`` [F,V] i64 (the view's local part, -1 where the view does not see it), ``n_points`` [F] i64,
    ``vol`` [F] i64 (voxels, the sum over the members), ``links`` [L,3] i64 = (g, h, shared voxels) of every union in the order taken
    (g, h: global part numbers = the view's first number + the local one), ``dropped`` [V] i64, ``member_offsets`` [F+1] i64."""
    fused_inst: torch.Tensor
    part_class: np.ndarray
    score: torch.Tensor
    n_views: np.ndarray
    parts: np.ndarray
    n_points: np.ndarray
    vol: np.ndarray
    links: np.ndarray
    dropped: np.ndarray
    valid: torch.Tensor
    bbox: torch.Tensor
    scale: torch.Tensor
    rotation: torch.Tensor
    translation: torch.Tensor
    member_offsets: np.ndarray
    member_src: torch.Tensor
    member_xyz: torch.Tensor
    member_npcs: Optional[torch.Tensor]

    def to_numpy(self) -> dict:
        return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in self.__dict__.items() if v is not None}


# ------------------------------------------------------------------------------------------------------------ the CPU path
def _world_numpy(rows, valid, inst, n_parts, R, t, GT: int):
    """-> (wrows [V*H*W,3] f32, part_of [V,H,W] i32, area [GT] i32, lo [3] f64)"""
    V, H, W = inst.shape
    n = np.clip(np.asarray(n_parts, np.int64), 0, GT)
    base = np.concatenate([[0], np.cumsum(n)])[:V]
    q = inst.astype(np.int64)
    member = (valid != 0) & (q >= 0) & (q < n[:, None, None]) & (base[:, None, None] + q < GT)
    part_of = np.where(member, base[:, None, None] + q, -1).astype(np.int32)
    xyz = rows.reshape(V, H * W, 6)[:, :, :3].astype(np.float64)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    Rv, tv = np.asarray(R, np.float64).reshape(V, 3, 3), np.asarray(t, np.float64).reshape(V, 3)
    with np.errstate(all="ignore"):
        w = np.stack([((x * Rv[:, k, 0, None] + y * Rv[:, k, 1, None]) + z * Rv[:, k, 2, None]) + tv[:, k, None] for k in range(3)], -1)
        wrows = w.astype(np.float32).reshape(V * H * W, 3)
    m = member.reshape(-1)
    wrows[~m] = np.nan
    area = np.bincount(part_of.reshape(-1)[m], minlength=GT)[:GT].astype(np.int32)
    lo = np.zeros(3, np.float64)
    if m.any():
        for k in range(3):
            col = wrows[m, k]
            col = col[~np.isnan(col)]
            if col.size:
                lo[k] = np.float64(col.min())
                if lo[k] == 0.0 and np.signbit(col[col == 0.0]).any():  # (the integer image puts -0.0 below +0.0)
                    lo[k] = -0.0
    return wrows, part_of, area, lo


def _keys_numpy(wrows, part_of, lo, cell: float, GT: int):
    """-> (keys [V,H,W] u64, dropped [V] i32)"""
    V = part_of.shape[0]
    g = part_of.reshape(-1).astype(np.int64)
    member = (g >= 0) & (g < GT)
    with np.errstate(all="ignore"):
        q = np.floor((wrows.astype(np.float64) - np.asarray(lo, np.float64)[None, :]) / np.float64(cell))
        ok = ((q >= 0) & (q < GRID_CELLS)).all(1)
    i = np.where(ok[:, None], q, 0).astype(np.int64)
    vox = (i[:, 0] << 20) | (i[:, 1] << 10) | i[:, 2]
    live = member & ok
    keys = np.where(live, ((vox << 9) | np.where(member, g, 0)).astype(np.uint64), DEAD_KEY)
    dropped = (member & ~ok).reshape(V, -1).sum(1).astype(np.int32)
    return keys.reshape(part_of.shape), dropped


def _tables_numpy(keys, GT: int):
    """-> (vol [GT] i32, inter [GT,GT] i32) over the distinct (vox, g)"""
    u = np.unique(keys.reshape(-1))
    u = u[u != DEAD_KEY].astype(np.int64)
    g, vox = u & 511, u >> 9
    vol = np.bincount(g, minlength=GT)[:GT].astype(np.int32)
    inter = np.zeros((GT, GT), np.int32)
    d = 1
    while d < u.shape[0]:
        same = vox[d:] == vox[:-d]
        if not same.any():
            break
        np.add.at(inter, (g[:-d][same], g[d:][same]), 1)
        np.add.at(inter, (g[d:][same], g[:-d][same]), 1)
        d += 1
    return vol, inter


def _before(p, q) -> int:
    """the order of the merge on (inter, min vol, g, h): the larger ratio first, exactly, then the smaller g, then h"""
    l, r = p[0] * q[1], q[0] * p[1]
    if l != r:
        return -1 if l > r else 1
    return -1 if p[2:] < q[2:] else (1 if p[2:] > q[2:] else 0)


def _merge_numpy(inter, vol, cls, n_parts, min_inter: int, min_overlap: float) -> dict:
    GT, V = int(vol.shape[0]), len(n_parts)
    n = np.clip(np.asarray(n_parts, np.int64), 0, GT)
    base = np.minimum(np.concatenate([[0], np.cumsum(n)]), GT)
    view_of = np.full(GT, -1, np.int64)
    for v in range(V):
        view_of[base[v]:base[v + 1]] = v
    svol = np.where(view_of >= 0, np.maximum(vol.astype(np.int64), 0), 0)
    cls = np.zeros(GT, np.int64) if cls is None else np.asarray(cls, np.int64)
    mi = max(int(min_inter), 1)
    gg, hh = np.nonzero(np.triu(inter >= mi, 1))
    cand = []
    for g, h in zip(gg.tolist(), hh.tolist()):
        c, m = int(inter[g, h]), int(min(svol[g], svol[h]))
        if m > 0 and cls[g] == cls[h] and float(c) >= float(min_overlap) * float(m):
            cand.append((c, m, g, h))
    rep = np.arange(GT)
    views = [(1 << int(v)) if v >= 0 else 0 for v in view_of]
    cvol = svol.copy()
    links = []
    # (the order is total and clusters only grow: walking the sorted list IS the repeated arg-max)
    for c, m, g, h in sorted(cand, key=functools.cmp_to_key(_before)):
        a, b = int(rep[g]), int(rep[h])
        if a == b or (views[a] & views[b]):
            continue
        keep, gone = min(a, b), max(a, b)
        rep[rep == gone] = keep
        views[keep] |= views[gone]
        cvol[keep] += cvol[gone]
        links.append((g, h, c))
    reps = [g for g in range(GT) if svol[g] > 0 and rep[g] == g]
    fid = {r: f for f, r in enumerate(reps)}
    F = len(reps)
    out = dict(fused_of=np.array([fid[int(rep[g])] if svol[g] > 0 else -1 for g in range(GT)], np.int32).reshape(GT),
               n_fused=np.array([F], np.int32), fused_views=np.zeros(GT, np.uint64), fused_class=np.full(GT, -1, np.int32),
               fused_vol=np.zeros(GT, np.int32), fused_parts=np.full((GT, V), -1, np.int32), links=np.zeros((GT, 3), np.int32),
               n_links=np.array([len(links)], np.int32))
    out["links"][:, :2] = -1
    for f, r in enumerate(reps):
        out["fused_views"][f], out["fused_class"][f], out["fused_vol"][f] = views[r], cls[r], cvol[r]
    for g in range(GT):
        if out["fused_of"][g] >= 0:
            out["fused_parts"][out["fused_of"][g], view_of[g]] = g - base[view_of[g]]
    if links:
        out["links"][:len(links)] = np.array(links, np.int32)
    return out


def _relabel_numpy(part_of, fused_of):
    GT = fused_of.shape[0]
    ok = (part_of >= 0) & (part_of < GT)
    return np.where(ok, np.concatenate([fused_of, [-1]]).astype(np.int32)[np.where(ok, part_of, GT)], -1).astype(np.int32)


def _gather_numpy(wrows, npcs, fused_inst, seg_start, n_total: int):
    """-> (xyz [M,3] f64, npcs_out [M,3] f64 or None, src [M] i64), rows no segment covers zero"""
    F = len(seg_start)
    flat = fused_inst.reshape(-1)
    xyz, src = np.zeros((n_total, 3), np.float64), np.zeros(n_total, np.int64)
    out_npcs = None if npcs is None else np.zeros((n_total, 3), np.float64)
    for f in range(F):
        s0 = int(seg_start[f])
        if s0 < 0:
            continue
        rows = np.flatnonzero(flat == f)
        rows = rows[:max(min(rows.shape[0], n_total - s0), 0)]
        xyz[s0:s0 + rows.shape[0]], src[s0:s0 + rows.shape[0]] = wrows[rows].astype(np.float64), rows
        if npcs is not None:
            out_npcs[s0:s0 + rows.shape[0]] = npcs.reshape(-1, 3)[rows].astype(np.float64)
    return xyz, out_npcs, src


# ------------------------------------------------------------------------------------------------------------ inputs
def _poses(R, t, V: int):
    R = torch.as_tensor(np.asarray(R, dtype=np.float64) if not torch.is_tensor(R) else R).detach().cpu().double().reshape(-1, 3, 3)
    t = torch.as_tensor(np.asarray(t, dtype=np.float64) if not torch.is_tensor(t) else t).detach().cpu().double().reshape(-1, 3)
    if R.shape[0] != V or t.shape[0] != V:
        raise ValueError(f"{V} views need R [{V},3,3] and t [{V},3]")
    return R.contiguous(), t.contiguous()


def ball_frame(xyz: torch.Tensor):
    """the ball of section CP over ``xyz`` [M,3] f64: c = (max + min) / 2, r = sqrt(max((dx*dx + dy*dy) + dz*dz)) -> (r [], c [3])
    on ``xyz``'s device"""
    c = (xyz.max(0)[0] + xyz.min(0)[0]) / 2
    d = xyz - c
    r = torch.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
    return r, c


# ------------------------------------------------------------------------------------------------------------ fusion
@torch.no_grad()
def fuse_parts(depth, K, inst, classes, R, t, npcs=None, scores=None, depth_scale: float = 1.0, keep=None, cell: float = 0.01,
               min_inter: int = 4, min_overlap: float = 0.25, picks=None, max_iters: int = 100) -> FusedParts:
    """V depth frames [V,H,W] of ONE object with intrinsics ``K`` ([3,3] or [V,3,3]), poses ``R`` [V,3,3], ``t`` [V,3] (a camera
    point is ``(world - t) @ R``), each view's instance map (pixel -> the part's position in the view's class list, anything else:
    no part; a pixel without depth belongs to no part) and class list -> ``FusedParts``.  The caller's own maps: ground-truth
    ``ins`` maps of ``render_views`` work as well as ``FramePrediction.instance``.  ``npcs`` [V,H,W,3] f32: with it, every fused
    part's box comes from one ``estimate_pose_from_npcs_batched`` pass over all fused parts (``npcs - 0.5``), run in the ball frame
    (section CP) of all fused member points and mapped back to the world frame; ``picks``: that pass's [F, iterations, 5] tensor, or
    a callable(sizes), drawn when None.  ``scores``: one list per view.  ``cell`` (in the units of depth / depth_scale),
    ``min_inter``, ``min_overlap``: the rules of include/gpn.h section MV - their defaults are NOT tuned on real data.  On the GPU:
    ONE host read (the small tables) in front of the fit."""
    from .. import inference
    depth, _, Kc, keep = inference._check_frames(depth, None, K, keep)
    inst = _maps(inst, "inst")
    if depth.shape != inst.shape or depth.device != inst.device:
        raise ValueError("the depth frames and instance maps have one shape and live on one device")
    V, H, W = (int(v) for v in depth.shape)
    if V > VIEWS_MAX:
        raise ValueError(f"at most {VIEWS_MAX} views, got {V}")
    if not float(cell) > 0.0:
        raise ValueError("cell must be positive")
    dev = depth.device
    cls = _lists(classes, V, "classes")
    n_parts = [int(c.shape[0]) for c in cls]
    GT = sum(n_parts)
    if GT > FUSE_PARTS_MAX:
        raise ValueError(f"at most {FUSE_PARTS_MAX} parts over all views, got {GT}")
    Rc, tc = _poses(R, t, V)
    cls_all = torch.cat([c.to(dev, non_blocking=True).to(torch.int32) for c in cls]) if V else torch.zeros(0, dtype=torch.int32, device=dev)
    score_all = None
    if scores is not None:
        sc = _lists(scores, V, "scores")
        if [int(s.shape[0]) for s in sc] != n_parts:
            raise ValueError("scores: one score per class entry")
        score_all = torch.cat([s.to(dev, non_blocking=True).to(torch.float32) for s in sc]) if V else torch.zeros(0, device=dev)
    if npcs is not None:
        npcs = torch.as_tensor(npcs)
        npcs = npcs[None] if npcs.dim() == 3 else npcs
        if tuple(npcs.shape) != (V, H, W, 3) or npcs.device != dev:
            raise ValueError(f"npcs must be [{V},{H},{W},3] on the frames' device")
        npcs = npcs.to(torch.float32).contiguous()
    # ---- 1 - 4. world rows, occupancy, merge, relabel; the one host read ----
    hip = _need_hip("fuse_parts") if dev.type == "cuda" else None
    rows, valid, _ = inference.backproject_frames(depth, None, Kc, keep, depth_scale, False)
    if dev.type == "cuda":
        wrows, part_of, area, lo = hip.views_world(rows, valid, inst, n_parts, Rc.to(dev, non_blocking=True), tc.to(dev, non_blocking=True), GT)
        vol, inter, dropped = hip.views_overlap(wrows, part_of, lo, cell, GT)
        m = hip.views_merge(inter, vol, cls_all, n_parts, min_inter, min_overlap)
        fused_inst = hip.views_relabel(part_of, m["fused_of"])
        fused_of_dev = m["fused_of"].long()
        flat = torch.cat([x.reshape(-1) for x in (area, dropped, m["fused_of"], m["n_fused"], m["fused_class"], m["fused_vol"],
                                                  m["fused_parts"], m["links"], m["n_links"], m["fused_views"].view(torch.int32))]).cpu().numpy()
        sizes = (GT, V, GT, 1, GT, GT, GT * V, GT * 3, 1, 2 * GT)
        parts = np.split(flat, np.cumsum(sizes)[:-1])
        area, dropped = parts[0], parts[1]
        m = dict(fused_of=parts[2], n_fused=parts[3], fused_class=parts[4], fused_vol=parts[5], fused_parts=parts[6].reshape(GT, V),
                 links=parts[7].reshape(GT, 3), n_links=parts[8], fused_views=np.ascontiguousarray(parts[9]).view(np.uint64))
    else:
        wrows, part_of, area, lo = _world_numpy(rows.numpy(), valid.numpy(), inst.numpy(), n_parts, Rc.numpy(), tc.numpy(), GT)
        keys, dropped = _keys_numpy(wrows, part_of, lo, float(cell), GT)
        vol, inter = _tables_numpy(keys, GT)
        m = _merge_numpy(inter, vol, cls_all.numpy(), n_parts, int(min_inter), float(min_overlap))
        fused_inst = torch.from_numpy(_relabel_numpy(part_of, m["fused_of"]))
        fused_of_dev = torch.from_numpy(m["fused_of"].astype(np.int64))
    # ---- 5. the fused parts' clouds ----
    F, L = int(m["n_fused"][0]), int(m["n_links"][0])
    fused_of = m["fused_of"].astype(np.int64)
    n_points = np.bincount(fused_of[fused_of >= 0], weights=area[fused_of >= 0].astype(np.float64), minlength=F).astype(np.int64)[:F]
    offsets = np.concatenate([[0], np.cumsum(n_points)]).astype(np.int64)
    M = int(offsets[-1])
    if dev.type == "cuda":
        xyz, npcs_m, src = hip.views_gather(wrows, npcs, fused_inst, torch.from_numpy(offsets[:-1].copy()), M)
    else:
        xyz, npcs_m, src = _gather_numpy(wrows, None if npcs is None else npcs.numpy(), fused_inst.numpy(), offsets[:-1], M)
        xyz, src = torch.from_numpy(xyz), torch.from_numpy(src)
        npcs_m = None if npcs_m is None else torch.from_numpy(npcs_m)
    # ---- 6. one fit over all fused parts, in the ball frame of all member points ----
    f64, nan = torch.float64, float("nan")
    full = lambda *shape: torch.full((F,) + shape, nan, dtype=f64, device=dev)  # noqa: E731
    valid_f = torch.zeros(F, dtype=torch.bool, device=dev)
    bbox, scale, rotation, translation = full(8, 3), full(), full(3, 3), full(3)
    if npcs is not None and F > 0 and M > 0:
        sizes_host = n_points.tolist()
        if callable(picks):
            picks = picks(sizes_host)
        elif picks is None:
            picks = draw_picks(sizes_host, max_iters)
        r, c = ball_frame(xyz)
        fit = estimate_pose_from_npcs_batched((xyz - c) / r, npcs_m - 0.5, torch.from_numpy(offsets).to(dev, non_blocking=True), picks=picks,
                                              max_iters=max_iters)
        valid_f = torch.from_numpy(n_points >= 5).to(dev, non_blocking=True) & fit["valid"]
        # world = normalised * r + c: the similarity's linear part and translation scale by r, the centre is added
        keep_f = lambda x, y: torch.where(valid_f.reshape((-1,) + (1,) * (x.dim() - 1)), x, y)  # noqa: E731
        bbox, scale = keep_f(fit["bbox"] * r + c, bbox), keep_f(fit["scale"] * r, scale)
        rotation, translation = keep_f(fit["rotation"], rotation), keep_f(fit["translation"] * r + c, translation)
    score = torch.full((F,), nan, dtype=torch.float32, device=dev)
    if score_all is not None and F > 0:
        slot = torch.where(fused_of_dev >= 0, fused_of_dev, F)  # (a part without voxels goes to a spare slot: no boolean index, no host read)
        score = torch.full((F + 1,), float("-inf"), dtype=torch.float32, device=dev).scatter_reduce_(0, slot, score_all, "amax")[:F]
    fv = m["fused_views"][:F]
    n_views = np.array([bin(int(x)).count("1") for x in fv], np.int64)
    return FusedParts(fused_inst=fused_inst, part_class=m["fused_class"][:F].astype(np.int64), score=score, n_views=n_views,
                      parts=m["fused_parts"][:F].astype(np.int64), n_points=n_points, vol=m["fused_vol"][:F].astype(np.int64),
                      links=m["links"][:L].astype(np.int64), dropped=np.asarray(dropped).astype(np.int64), valid=valid_f, bbox=bbox,
                      scale=scale, rotation=rotation, translation=translation, member_offsets=offsets, member_src=src, member_xyz=xyz,
                      member_npcs=npcs_m)


@torch.no_grad()
def fuse_frames(predictor, depth, rgb, K, R, t, presample: int = 4, seed=0, isolate=None, sampler: Optional[str] = None, frame_picks=None,
                depth_scale: float = 1.0, **kw):
    """``predictor.predict_frames`` on all views (``presample``, ``seed``, ``isolate``, ``depth_scale`` and ``frame_picks`` - its
    ``picks`` - go to it; ``sampler``: another sampler than the predictor's), then ``fuse_parts`` on their ``instance`` maps,
    ``proposal_classes``, ``proposal_scores`` and ``npcs`` (``kw``).  -> (frames, fused)"""
    predictor = predictor.with_sampler(sampler)
    frames = predictor.predict_frames(depth, rgb, K, picks=frame_picks, presample=presample, seed=seed, depth_scale=depth_scale,
                                      flip=False, isolate=isolate)
    fused = fuse_parts(depth, K, torch.stack([f.instance for f in frames]), [f.proposal_classes for f in frames], R, t,
                       npcs=torch.stack([f.npcs for f in frames]), scores=[f.proposal_scores for f in frames], depth_scale=depth_scale,
                       **kw)
    return frames, fused


def draw_fused(rgb, K, R, t, fused: FusedParts, view: int = 0) -> np.ndarray:
    """a copy of view ``view``'s ``rgb`` [H,W,3] u8 with every valid fused box drawn: the world-frame corners go to the view's
    camera frame by ``(world - t) @ R``, then ``project_corners`` / ``draw_overlays``.  ``K``, ``R``, ``t``: that view's, or all views'"""
    from .. import inference
    K = torch.as_tensor(np.asarray(K, np.float64)).reshape(-1, 3, 3)
    Rv = torch.as_tensor(np.asarray(R, np.float64)).reshape(-1, 3, 3)
    tv = torch.as_tensor(np.asarray(t, np.float64)).reshape(-1, 3)
    K, Rv, tv = (x[view if x.shape[0] > 1 else 0] for x in (K, Rv, tv))
    img = torch.as_tensor(rgb).detach().cpu()
    img = img[view] if img.dim() == 4 else img
    boxes = fused.bbox.detach().cpu()[fused.valid.detach().cpu()]
    cam = (boxes - tv) @ Rv
    return inference.draw_overlays(img[None].contiguous(), [cam], K[None])[0].numpy()


# ------------------------------------------------------------------------------------------------------------ command line
def _read_meta(path: str):
    with open(path) as fd:
        meta = json.load(fd)
    return (np.asarray(meta["camera_intrinsic"], np.float64).reshape(3, 3), np.asarray(meta["world2camera_rotation"], np.float64).reshape(3, 3),
            np.asarray(meta["camera2world_translation"], np.float64).reshape(3))


def _read_depth_any(path: str) -> np.ndarray:
    from .. import inference
    if path.endswith(".npz"):  # (the renderer's layout: write_view)
        return np.load(path)["depth_map"]
    return inference._read_depth(path)


def main(argv: Optional[Sequence[str]] = None) -> int:
    from .. import inference
    ap = argparse.ArgumentParser(prog="python -m gapartnet_amd.misc.multiview",
                                 description="the parts of one object from several posed RGB-D views, fused in the world frame")
    ap.add_argument("--depth", nargs="+", required=True, help="one depth map per view (.png 16-bit / .npy / the renderer's .npz)")
    ap.add_argument("--rgb", nargs="+", help="one image per view (needed with --ckpt; the overlays are drawn into them)")
    ap.add_argument("--meta", nargs="+", required=True, help="one metafile per view (write_view's .json): intrinsics and pose")
    ap.add_argument("--ckpt", help="checkpoint: the parts are predicted")
    ap.add_argument("--instances", nargs="+", help="instead of --ckpt: one [H,W] integer instance map per view (.npy)")
    ap.add_argument("--classes", nargs="+", help="with --instances: one class list per view (.npy)")
    ap.add_argument("--npcs", nargs="+", help="with --instances: one [H,W,3] NPCS map per view (.npy); without it no boxes are fitted")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--depth_scale", type=float, default=1.0)
    ap.add_argument("--cell", type=float, default=0.01, help="voxel edge (untuned default)")
    ap.add_argument("--min_inter", type=int, default=4, help="shared voxels a pair needs (untuned default)")
    ap.add_argument("--min_overlap", type=float, default=0.25, help="share of the smaller part's voxels a pair needs (untuned default)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--presample", type=int, default=4)
    ap.add_argument("--sampler", default="fps", choices=("fps", "grid"))
    ap.add_argument("--isolate", action="store_true", help="with --ckpt: cut the object out of the raw frames first")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args(argv)
    V = len(args.depth)
    if (args.ckpt is None) == (args.instances is None):
        ap.error("give --ckpt, or --instances with --classes")
    if args.instances is not None and args.classes is None:
        ap.error("--instances needs --classes")
    if args.ckpt is not None and args.rgb is None:
        ap.error("--ckpt needs --rgb")
    for name in ("meta", "rgb", "instances", "classes", "npcs"):
        if getattr(args, name) is not None and len(getattr(args, name)) != V:
            ap.error(f"--{name}: one file per view ({V})")
    random.seed(args.seed)
    np.random.seed(args.seed)
    dev = torch.device(args.device)
    depth = [_read_depth_any(p) for p in args.depth]
    if any(d.shape != depth[0].shape or d.dtype != depth[0].dtype for d in depth):
        ap.error("the depth maps have one size and type")
    K, R, t = (np.stack(x) for x in zip(*[_read_meta(p) for p in args.meta]))
    rgb = None if args.rgb is None else [np.ascontiguousarray(inference._read_image(p)[..., :3]).astype(np.uint8) for p in args.rgb]
    d = torch.from_numpy(np.stack(depth)).to(dev)
    kw = dict(depth_scale=args.depth_scale, cell=args.cell, min_inter=args.min_inter, min_overlap=args.min_overlap)
    if args.ckpt is not None:
        model = inference.load_model(args.ckpt, dev)
        predictor = inference.PartPredictor(model, num_points=args.num_points, sampler=args.sampler)
        _, fused = fuse_frames(predictor, d, torch.from_numpy(np.stack(rgb)).to(dev), K, R, t, presample=args.presample, seed=args.seed,
                               isolate=inference.IsolateConfig() if args.isolate else None, **kw)
    else:
        inst = torch.from_numpy(np.stack([np.load(p).astype(np.int64) for p in args.instances])).to(dev)
        cls = [np.load(p).astype(np.int64).reshape(-1) for p in args.classes]
        npcs = None if args.npcs is None else torch.from_numpy(np.stack([np.load(p).astype(np.float32) for p in args.npcs])).to(dev)
        fused = fuse_parts(d, K, inst, cls, R, t, npcs=npcs, **kw)
    os.makedirs(args.out, exist_ok=True)
    name = os.path.splitext(os.path.basename(args.depth[0]))[0]
    path = os.path.join(args.out, f"{name}_fused.npz")
    np.savez(path, **fused.to_numpy())
    print(path)
    for f in range(fused.part_class.shape[0]):
        print(f"fused part {f}: class {int(fused.part_class[f])}, {int(fused.n_views[f])} views, parts {fused.parts[f].tolist()}, "
              f"{int(fused.n_points[f])} points, {int(fused.vol[f])} voxels")
    if rgb is None:  # (no image given: the boxes are drawn on the depth maps, as grey levels)
        rgb = []
        for dm in depth:
            dm = np.nan_to_num(dm.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
            top = dm.max() if dm.max() > 0 else 1.0
            rgb.append(np.repeat(np.rint(dm / top * 255.0).astype(np.uint8)[..., None], 3, 2))
    from PIL import Image
    for v in range(V):
        vname = os.path.splitext(os.path.basename(args.depth[v]))[0]
        path = os.path.join(args.out, f"{vname}_fused_view{v}.png")
        Image.fromarray(draw_fused(rgb[v], K[v], R[v], t[v], fused, 0)).save(path)
        print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
