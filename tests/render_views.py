"""Synthetic RGB-D views in the renderer's file layout (the reference's render_tools: rgb/*.png, depth/*.npz['depth_map'],
segmentation/*.npz['semantic_segmentation', 'instance_segmentation'], npcs/*.npz['npcs_map'], metafile/*.json, bbox/*.pkl).

A pinhole camera looks at a few boxes: each box shows a front face parallel to the image plane and, for some, a side face whose
depth grows linearly across it.  Background is -2 in both label maps; an "others" surface is -1 in both; parts carry a category id
and an instance id.  The cases a converter must get right are named views:

    plain        boxes and parts, enough pixels
    too_few      fewer valid pixels than num_points (skipped and logged)
    exact        exactly num_points valid pixels (arange, no sampling)
    holes        single-pixel parts the sampler rarely takes: instance ids open holes that the relabel loop closes
    ties         one fronto-parallel plane, symmetric about the principal point: exact distance ties in FPS
    mismatch     a pixel with sem == -1 and ins != -1 (the reference asserts)
    big_id       an instance id beyond the converter's table
"""
import json
import os
import pickle

import numpy as np


def intrinsics(H, W, f=None):
    f = float(f if f is not None else 1.1 * W)
    return np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=np.float64)


def _blank(H, W):
    return dict(depth=np.zeros((H, W), np.float32), sem=np.full((H, W), -2, np.int32), ins=np.full((H, W), -2, np.int32),
                npcs=np.zeros((H, W, 3), np.float32), rgb=np.zeros((H, W, 3), np.uint8))


def _paint(v, y0, y1, x0, x1, z0, sem, ins, rng, slope=0.0):
    """an axis-aligned face covering rows y0:y1, columns x0:x1 at depth z0 (+ slope per column)"""
    ys, xs = np.mgrid[y0:y1, x0:x1]
    v['depth'][y0:y1, x0:x1] = (z0 + slope * (xs - x0)).astype(np.float32)
    v['sem'][y0:y1, x0:x1] = sem
    v['ins'][y0:y1, x0:x1] = ins
    u = (xs - x0) / max(x1 - x0 - 1, 1) - 0.5
    w = (ys - y0) / max(y1 - y0 - 1, 1) - 0.5
    v['npcs'][y0:y1, x0:x1] = np.stack([u, w, np.full_like(u, 0.25 * slope)], -1).astype(np.float32)
    v['rgb'][y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)


def make_view(kind, H=60, W=80, num_points=512, seed=0):
    """one synthetic view -> dict(rgb, depth, sem, ins, npcs, K)"""
    rng = np.random.default_rng(seed)
    v = _blank(H, W)
    if kind == 'ties':
        v['depth'][:] = np.float32(1.5)
        v['sem'][:] = 0
        v['ins'][:] = 0
        v['rgb'][:] = 128
    elif kind == 'exact':
        # exactly num_points valid pixels: whole rows of one part plus the remainder on the next row
        rows, rest = divmod(num_points, W)
        _paint(v, 0, rows, 0, W, 1.2, 1, 0, rng)
        if rest:
            _paint(v, rows, rows + 1, 0, rest, 1.2, 1, 0, rng)
    elif kind == 'too_few':
        _paint(v, 10, 15, 10, 10 + max(1, num_points // 10), 1.0, 0, 0, rng)
    else:
        # "others": a back wall, then boxes in front of it
        _paint(v, 0, H, 0, W, 3.0, -1, -1, rng, slope=0.002)
        _paint(v, 8, 40, 6, 36, 1.6, 2, 0, rng)                 # box A front face (part 0, category 2)
        _paint(v, 8, 40, 36, 44, 1.6, 2, 1, rng, slope=0.05)    # box A side face (part 1), depth grows across it
        _paint(v, 30, 56, 48, 76, 2.1, 5, 2, rng)               # box B (part 2, category 5)
        _paint(v, 42, 52, 12, 30, 1.9, 0, 3, rng)               # box C (part 3)
        if kind == 'holes':
            # single-pixel parts inside larger faces: ids the sampler rarely takes
            v['sem'][20, 20], v['ins'][20, 20] = 3, 4
            v['sem'][44, 60], v['ins'][44, 60] = 4, 5
            v['sem'][24, 14], v['ins'][24, 14] = 1, 1
            v['ins'][8:40, 36:44] = 6  # box A's side face takes id 6: id 1 is a single pixel
        if kind == 'mismatch':
            v['sem'][50, 2], v['ins'][50, 2] = -1, 3
        if kind == 'big_id':
            v['ins'][30:56, 48:76] = 5000
    v['K'] = intrinsics(H, W)
    return v


def write_view(root, name, v):
    """one view in the renderer's layout under root (bbox/*.pkl: the reference's loader opens it; its content is unused)"""
    from PIL import Image
    for sub in ('rgb', 'depth', 'segmentation', 'npcs', 'metafile', 'bbox'):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    H, W = v['depth'].shape
    Image.fromarray(v['rgb']).save(os.path.join(root, 'rgb', f'{name}.png'))
    np.savez_compressed(os.path.join(root, 'depth', f'{name}.npz'), depth_map=v['depth'])
    np.savez_compressed(os.path.join(root, 'segmentation', f'{name}.npz'), semantic_segmentation=v['sem'],
                        instance_segmentation=v['ins'])
    np.savez_compressed(os.path.join(root, 'npcs', f'{name}.npz'), npcs_map=v['npcs'])
    meta = dict(width=W, height=H, camera_intrinsic=[float(x) for x in v['K'].reshape(-1)])
    with open(os.path.join(root, 'metafile', f'{name}.json'), 'w') as fh:
        json.dump(meta, fh)
    with open(os.path.join(root, 'bbox', f'{name}.pkl'), 'wb') as fh:
        pickle.dump({'bbox_pose_dict': {}}, fh)


def full_size_view(seed, H=800, W=800):
    """an 800 x 800 view with ~2.5 x 10^5 valid pixels (the benchmark's and the full-size test's input)"""
    rng = np.random.default_rng(seed)
    v = _blank(H, W)
    dz = 0.01 * (seed % 7)
    _paint(v, 100, 480, 80, 440, 1.6 + dz, 2, 0, rng)
    _paint(v, 100, 480, 440, 540, 1.6 + dz, 2, 1, rng, slope=0.004)
    _paint(v, 400, 740, 600, 780, 2.1, 5, 2, rng)
    _paint(v, 560, 690, 150, 400, 1.9, 0, 3, rng)
    v['K'] = intrinsics(H, W)
    return v
