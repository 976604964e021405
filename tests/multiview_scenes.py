"""Scenes for the multi-view tests: axis-aligned boxes ray-cast through ``camera_frame`` (dataset/render_assets.py), so depth and
instance maps are exact and every view's pose is the renderer's.  Each view numbers the boxes it sees in its own, permuted order -
as independent per-frame predictions would - and ``truth`` keeps the box behind every local part."""
import math

import numpy as np

from gapartnet_amd.dataset.render_assets import camera_frame

# (lo, hi) of the identity scene: a cabinet body, two drawer fronts, a handle on the upper front, a lid
IDENTITY_BOXES = [
    ((-.30, -.25, -.30), (.30, .25, .30)),
    ((-.34, -.20, .05), (-.30, .20, .25)),
    ((-.34, -.20, -.25), (-.30, .20, -.05)),
    ((-.37, -.05, .13), (-.34, .05, .17)),
    ((-.20, -.15, .30), (.20, .15, .34)),
]
IDENTITY_AZIMUTHS = (150.0, 180.0, 210.0, 240.0)
IDENTITY_ELEVATION = 30.0  # degrees above the horizon: the lid's top face and the fronts are both seen
IDENTITY_DISTANCE = 2.2


def camera_position(azimuth_deg, elevation_deg, distance):
    a, e = math.radians(azimuth_deg), math.radians(elevation_deg)
    return np.array([distance * math.cos(e) * math.cos(a), distance * math.cos(e) * math.sin(a), distance * math.sin(e)])


def raycast(boxes, cam_pos, H, W):
    """-> (depth [H,W] f32 - 0 where no box is hit -, box [H,W] i64 - -1 where none -, npcs [H,W,3] f32, K, R, t).  The ray of pixel
    (u, v) is the one ``gpn_frame_backproject`` inverts: camera direction ((u - cx) / fx, (v - cy) / fy, 1), so depth = the ray's
    parameter.  npcs = the hit point's place inside its box, 0 .. 1 an axis (canonical per box, whatever the view)."""
    K, R, t = camera_frame(cam_pos, H, W)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    d = d_cam @ R.T  # world = cam @ R^T + t
    best = np.full((H, W), np.inf)
    which = np.full((H, W), -1, np.int64)
    with np.errstate(all="ignore"):
        for i, (lo, hi) in enumerate(boxes):
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            t0, t1 = (lo - t) / d, (hi - t) / d
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 0) & (near < best)
            best[hit], which[hit] = near[hit], i
    depth = np.where(which >= 0, best, 0.0).astype(np.float32)
    point = t + d * depth.astype(np.float64)[..., None]
    npcs = np.zeros((H, W, 3), np.float32)
    for i, (lo, hi) in enumerate(boxes):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        m = which == i
        npcs[m] = np.clip((point[m] - lo) / (hi - lo), 0.0, 1.0).astype(np.float32)
    return depth, which, npcs, K, R, t


def scene(boxes, cam_positions, H, W, seed=0, classes=None):
    """-> dict(depth [V,H,W] f32, inst [V,H,W] i64, npcs [V,H,W,3] f32, K, R, t, classes (V lists), truth (V lists: the box of every
    local part), n_boxes).  ``classes``: one class per box (default: all 1)."""
    rng = np.random.RandomState(seed)
    classes = [1] * len(boxes) if classes is None else list(classes)
    out = dict(depth=[], inst=[], npcs=[], K=[], R=[], t=[], classes=[], truth=[], n_boxes=len(boxes))
    for p in cam_positions:
        depth, which, npcs, K, R, t = raycast(boxes, p, H, W)
        seen = [int(b) for b in np.unique(which[which >= 0])]
        order = [seen[i] for i in rng.permutation(len(seen))]
        local = np.full(len(boxes) + 1, -1, np.int64)
        for j, b in enumerate(order):
            local[b] = j
        out["depth"].append(depth)
        out["inst"].append(local[which])
        out["npcs"].append(npcs)
        out["K"].append(K)
        out["R"].append(R)
        out["t"].append(t)
        out["classes"].append([classes[b] for b in order])
        out["truth"].append(order)
    for k in ("depth", "inst", "npcs", "K", "R", "t"):
        out[k] = np.stack(out[k])
    return out


def identity_scene(H=96, W=128, seed=0):
    return scene(IDENTITY_BOXES, [camera_position(a, IDENTITY_ELEVATION, IDENTITY_DISTANCE) for a in IDENTITY_AZIMUTHS], H, W, seed)


def small_scene(seed=1, H=40, W=48, classes=(1, 1, 2, 2, 3)):
    """the identity boxes at a small size with mixed classes: a quick scene for path-against-path comparisons"""
    return scene(IDENTITY_BOXES, [camera_position(a, 25.0, 2.0) for a in (160.0, 200.0, 250.0)], H, W, seed, classes)


def fused_identity(sc, fused_parts):
    """the boxes behind every fused part: [F] sets, from fused_parts [F,V] (the local part of each view, or -1)"""
    return [{sc["truth"][v][int(p)] for v, p in enumerate(row) if p >= 0} for row in fused_parts]
