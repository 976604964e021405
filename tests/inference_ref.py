"""numpy restatement of the raw-cloud front and back end of label-free inference (include/gpn.h section CP): what
gpn_cloud_pack + gpn_view_fps + gpn_cloud_finish and gpn_cloud_nearest are held to.  The ball normalisation is the reference's
FindMaxDis / WorldSpaceToBallSpace (tools/visu_utils.py:157-173) in float64; FPS is tests/convert_ref.oracle_fps."""
import numpy as np
import torch

from gapartnet_amd.structure.point_cloud import PointCloud
from tests.convert_ref import oracle_fps

OK, FEW, EMPTY, DEGENERATE = 0, 1, 2, 3


def valid_rows(cloud):
    return np.nonzero(np.isfinite(cloud[:, :3].astype(np.float32)).all(1))[0].astype(np.int64)


def ball_space(p64):
    """the reference's formula on float64 points -> (normalized, radius, center)"""
    center = (p64.max(0) + p64.min(0)) / 2
    radius = ((((p64 - center) ** 2).sum(1)) ** 0.5).max()
    return (p64 - center) / radius, radius, center


def prepare_cloud(cloud, m, fps=oracle_fps):
    """one cloud [n, C] f32 -> dict(status, count = valid rows, sample_rows [m_s] i64, scale [4] f64, out [m_s, C] f32)"""
    cloud = np.asarray(cloud, dtype=np.float32)
    rows = valid_rows(cloud)
    n = rows.shape[0]
    res = dict(status=EMPTY, count=n, sample_rows=np.zeros(0, np.int64), scale=np.zeros(4), out=np.zeros((0, cloud.shape[1]), np.float32))
    if n == 0:
        return res
    if n > m:
        rows = rows[np.asarray(fps(np.ascontiguousarray(cloud[rows, :3]), m), dtype=np.int64)]
    with np.errstate(invalid="ignore", divide="ignore"):
        normalized, radius, center = ball_space(cloud[rows, :3].astype(np.float64))
    out = cloud[rows].copy()
    out[:, :3] = normalized.astype(np.float32) if radius > 0 else 0.0
    res.update(status=OK if radius > 0 else DEGENERATE, sample_rows=rows, scale=np.concatenate([[radius], center]), out=out)
    return res


def nearest(queries, samples, chunk=2048):
    """brute force: per query row the nearest sample by fp32 (dx*dx + dy*dy) + dz*dz, lowest index on ties; -1 / +inf for a row
    with a non-finite coordinate or when there are no samples -> (nn [n] i64, d2 [n] f32)"""
    q = np.asarray(queries, dtype=np.float32)[:, :3]
    s = np.asarray(samples, dtype=np.float32)[:, :3]
    nn = np.full(q.shape[0], -1, np.int64)
    d2 = np.full(q.shape[0], np.inf, np.float32)
    if s.shape[0] == 0:
        return nn, d2
    ok = np.isfinite(q).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, q.shape[0], chunk):
            d = q[a:a + chunk, None, :] - s[None, :, :]
            dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert dd.dtype == np.float32
            best = dd.argmin(1)  # (numpy: the first minimum)
            sel = ok[a:a + chunk]
            nn[a:a + chunk][sel] = best[sel]
            d2[a:a + chunk][sel] = dd[np.arange(dd.shape[0]), best][sel]
    return nn, d2


# ---------------------------------------------------------------------------------------------------- the model's side
def unlabelled(scenes):
    return [PointCloud(pc_id=pc.pc_id, points=pc.points, obj_cat=pc.obj_cat, voxel_features=pc.voxel_features,
                       voxel_coords=pc.voxel_coords, voxel_coords_range=pc.voxel_coords_range, pc_voxel_id=pc.pc_voxel_id)
            for pc in scenes]


def forward_formulation(model, pcs):
    """what ``model(pcs)`` must return, from the model's public pieces"""
    with torch.no_grad():
        batch = model._collate(pcs)
        feat = model.forward_backbone(pc_batch=batch)
        sem_preds = model.forward_sem_seg(feat).argmax(-1)
        offsets = model.forward_offset(feat)
        saved = model.sync_free_proposals, model._want_npcs_preds
        model.sync_free_proposals, model._want_npcs_preds = False, True  # (the stage's form with host reads)
        try:
            vt, pid, props = model.proposal_clustering_and_revoxelize(
                pt_xyz=batch.points[:, :3], batch_indices=batch.batch_indices, pt_features=feat, sem_preds=sem_preds,
                offset_preds=offsets, instance_labels=None, batch_size=batch.batch_size)
        finally:
            model.sync_free_proposals, model._want_npcs_preds = saved
        out = dict(sem_preds=sem_preds, props=props)
        if props is None:
            return out
        score_logits = model.forward_proposal_score(vt, pid, props)
        cls = props.sem_preds.long()
        first = cls[props.proposal_offsets[:-1].long()]
        out["score_preds"] = torch.sigmoid(score_logits[torch.arange(first.shape[0], device=first.device), first - 1])
        npcs_logits = model.forward_proposal_npcs(vt, pid)
        out["npcs_preds"] = torch.stack([npcs_logits[torch.arange(cls.shape[0], device=cls.device), 3 * (cls - 1) + k]
                                         for k in range(3)], 1)
        return out


def check_forward_against_formulation(got, want):
    pc_ids, seg, props = got
    assert torch.equal(seg.sem_preds, want["sem_preds"])
    assert seg.sem_labels is None and seg.all_accu is None
    assert (props is None) == (want["props"] is None)
    if props is None:
        return
    w = want["props"]
    for f in ("valid_mask", "sorted_indices", "pt_xyz", "batch_indices", "proposal_offsets", "proposal_indices",
              "num_points_per_proposal", "sem_preds"):
        assert torch.equal(getattr(props, f), getattr(w, f)), f
    assert props.instance_labels is None and props.sem_labels is None and props.ious is None
    assert torch.equal(props.score_preds, want["score_preds"])
    assert torch.equal(props.npcs_preds, want["npcs_preds"])
    M = props.sorted_indices.shape[0]
    assert props.npcs_preds.shape == (M, 3) and props.npcs_valid_mask.dtype == torch.bool
    assert props.npcs_valid_mask.shape == (M,) and bool(props.npcs_valid_mask.all())


def raw_clouds(n=1500):
    """the synthetic scenes as raw camera-frame clouds [n + 8, 6], each with the 8 corners of its bounding CUBE added.  Why the
    corners: a scene's backbone output depends on the batch's spatial shape (the per-axis maximum over the scenes, at least 128:
    a stride-2 conv drops voxels on the last odd plane, as the reference's spconv does), so a scene alone and in a batch differ
    unless all shapes are equal.  A cube with occupied corners normalises to an edge of 2 / sqrt(3) = 116 voxels: every such
    batch has the shape [128] * 3 and the comparison of a cloud alone with the same cloud in a batch is exact."""
    from tests.golden import recipe
    out = []
    for seed, _ in recipe.PIPELINE_SCENES:
        xyz, rgb = recipe.scene_arrays(seed, n)[:2]
        lo, hi = xyz.min(0), xyz.max(0)
        half = (hi - lo).max() / 2
        corners = (lo + hi) / 2 + half * np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)])
        xyz = np.concatenate([xyz, corners])
        rgb = np.concatenate([rgb, np.full((8, 3), 0.5)])
        out.append(torch.from_numpy(np.concatenate([xyz * 0.37 + [0.1, -0.2, 1.5], rgb], 1).astype(np.float32)))
    return out


def size_picks(sizes, H=16):
    """RANSAC draws that depend on the proposal's size alone: the same proposal gets the same draws in any batch"""
    return torch.from_numpy(np.stack([np.random.RandomState(n).randint(max(n, 2), size=(H, 5)) for n in sizes]
                                     or [np.zeros((0, H, 5), np.int64)]).astype(np.int64).reshape(-1, H, 5))


def synthetic_unlabelled(n_points, device, seeds=None):
    """the synthetic scenes of the pipeline fixture at ``n_points`` points, as un-voxelised clouds without any label"""
    from tests.golden import recipe
    out = []
    for seed, cat in (seeds or recipe.PIPELINE_SCENES):
        xyz, rgb = recipe.scene_arrays(seed, n_points)[:2]
        out.append(PointCloud(pc_id=f"{cat}_{seed}", obj_cat=0,
                              points=torch.from_numpy(np.concatenate([xyz, rgb], 1).astype(np.float32)).to(device)))
    return out
