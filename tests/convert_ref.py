"""Vectorised numpy restatement of the reference's sample_and_save (dataset/process_tools/convert_rendered_into_input.py:90-175):
the yardstick of the converter tests (tests/test_convert_cpu.py pins it to the reference's own run, tests/golden/convert_views.npz).
FPS indices come from a callable fps(xyz_f32 [n,3], m) -> [m] (the CPU oracle of the CUDA kernel, or the GPU entry point)."""
import io

import numpy as np

MAX_INSTANCE_NUM = 1000
OK, TOO_FEW, LABEL_MISMATCH = 0, 1, 2


def oracle_fps(xyz32, m):
    from oracle import pn2_furthest_point_sampling
    return pn2_furthest_point_sampling(xyz32[None], m)[0].astype(np.int64)


def back_project(depth, sem, ins, K):
    """valid pixels in row-major order (:53-56) -> float64 points [n,3] (:57-59, left to right), ys, xs"""
    ys, xs = np.nonzero((sem != -2) & (ins != -2))
    z = depth[ys, xs].astype(np.float64)
    x = ((xs.astype(np.float64) - K[0, 2]) * z) / K[0, 0]
    y = ((ys.astype(np.float64) - K[1, 2]) * z) / K[1, 1]
    return np.stack([x, y, z], 1), ys, xs


def relabel(ins):
    """:142-147, as written"""
    ins = ins.copy()
    j = 0
    while j < ins.max():
        if len(np.where(ins == j)[0]) == 0:
            ins[ins == ins.max()] = j
        j += 1
    return ins


def convert_view(rgb, depth, sem, ins, npcs, K, num_points, fps=oracle_fps):
    """-> (status, 6-tuple or None, scale_param f64 [4] or None, gt i32 [m] or None)"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    pcs, ys, xs = back_project(depth, sem, ins, K)
    pcs_sem, pcs_ins = sem[ys, xs], ins[ys, xs]
    if not ((pcs_sem == -1) == (pcs_ins == -1)).all():
        return LABEL_MISMATCH, None, None, None
    n = pcs.shape[0]
    if n < num_points:
        return TOO_FEW, None, None, None
    fps_idx = np.arange(n) if n == num_points else np.asarray(fps(pcs.astype(np.float32), num_points), dtype=np.int64)
    sampled = pcs[fps_idx]
    center = (sampled.max(0) + sampled.min(0)) / 2
    radius = ((((sampled - center) ** 2).sum(1)) ** 0.5).max()
    normalized = (sampled - center) / radius
    sem_c = pcs_sem[fps_idx] + 1
    ins_c = pcs_ins[fps_idx].copy()
    ins_c[ins_c == -1] = -100
    ins_c = relabel(ins_c)
    gt = np.ones(ins_c.shape, dtype=np.int32) * (-100)
    for inst_id in range(int(ins_c.max() + 1)):
        where = np.where(ins_c == inst_id)[0]
        assert where.shape[0] > 0 and int(sem_c[where[0]]) != 0
        gt[where] = int(sem_c[where[0]]) * MAX_INSTANCE_NUM + inst_id
    arrays = (normalized.astype(np.float32), (rgb[ys, xs][fps_idx] / 255.0).astype(np.float32), sem_c.astype(np.int32),
              ins_c.astype(np.int32), npcs[ys, xs][fps_idx].astype(np.float32),
              np.stack([ys, xs], 1)[fps_idx].astype(np.int32))
    return OK, arrays, np.array([radius, center[0], center[1], center[2]]), gt


def meta_text(scale_param):
    buf = io.BytesIO()
    np.savetxt(buf, scale_param, delimiter=',')
    return buf.getvalue()


def gt_text(gt):
    buf = io.BytesIO()
    np.savetxt(buf, gt, fmt='%d')
    return buf.getvalue()
