"""Restatement of the mask stage (include/gpn.h section MP; GAPartNet.forward_with_masks / PartPredictor.predict_with_masks):
what gpn_mask_pack and gpn_proposals_from_masks are held to, in numpy for every integer table - one ``nonzero`` per mask - and
through ``segmented_voxelize`` for the voxel tables (the code tests/test_gpu_proposals.py holds the stage's tail bit-equal to)."""
import numpy as np
import torch

from gapartnet_amd.network.grouping_utils import segmented_voxelize
from gapartnet_amd.spconv import pytorch as spconv
from gapartnet_amd.structure.instances import Instances


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def members(counts, masks, sample_rows=None):
    """per mask of the concatenated list: (scene, ascending positions j of its members among the scene's network points).
    ``masks[s]`` [K_s, n_s]: on the network's points (n_s = counts[s]) or, with ``sample_rows`` [sum counts], on the rows of the
    caller's cloud, network point i being row sample_rows[i]"""
    rows = None if sample_rows is None else _np(sample_rows).astype(np.int64)
    out, first = [], 0
    for s, c in enumerate(counts):
        m = _np(masks[s]) if masks[s] is not None else np.zeros((0, c), np.uint8)
        for k in range(m.shape[0]):
            row = m[k] != 0
            if rows is not None:
                row = row[rows[first:first + c]]
            assert row.shape[0] == c
            out.append((s, np.nonzero(row)[0].astype(np.int64)))
        first += c
    return out


def pack(counts, masks, sample_rows=None):
    """[K, W] int64: the u64 words of gpn_mask_pack (bit j & 63 of word j >> 6 = member j), as two's-complement bit patterns"""
    mem = members(counts, masks, sample_rows)
    W = (max(list(counts) + [0]) + 63) // 64
    bits = np.zeros((len(mem), W), np.uint64)
    for k, (_, js) in enumerate(mem):
        np.bitwise_or.at(bits[k], js >> 6, np.uint64(1) << (js & 63).astype(np.uint64))
    return bits.view(np.int64)


def stage(xyz, counts, masks, labels, min_points, n_classes, sample_rows=None):
    """the proposal tables of the kept masks (>= min_points members, 1 <= label < n_classes; a label outside raises), or None when no
    mask is kept.  Torch tensors on ``xyz``'s device, dtypes of hip_ops.proposals_from_masks."""
    dev = xyz.device
    lab = np.concatenate([_np(v).astype(np.int64).reshape(-1) for v in labels] or [np.zeros(0, np.int64)])
    if ((lab < 1) | (lab >= n_classes)).any():
        raise ValueError("a mask label outside [1, n_classes)")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    kept = [(k, s, js + off[s]) for k, (s, js) in enumerate(members(counts, masks, sample_rows)) if js.shape[0] >= min_points]
    if not kept:
        return None
    N = int(off[-1])
    point_indices = np.concatenate([r for _, _, r in kept])
    sizes = np.array([r.shape[0] for _, _, r in kept], np.int64)
    proposal_indices = np.repeat(np.arange(len(kept), dtype=np.int64), sizes)
    valid = np.zeros(N, bool)
    valid[point_indices] = True
    rank = np.cumsum(valid) - 1
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)  # noqa: E731
    pi = t(point_indices, torch.int64)
    proposal_mask = np.array([k for k, _, _ in kept], np.int64)
    return dict(valid_mask=t(valid, torch.bool), valid_indices=t(np.nonzero(valid)[0], torch.int64),
                sorted_indices=t(rank[point_indices], torch.int64), point_indices=pi, proposal_indices=t(proposal_indices, torch.int64),
                batch_indices=t(np.repeat(np.array([s for _, s, _ in kept]), sizes), torch.int32), pt_xyz=xyz[pi],
                sem_preds=t(np.repeat(lab[proposal_mask], sizes), torch.int32), sizes=t(sizes, torch.int64),
                proposal_offsets=t(np.concatenate([[0], np.cumsum(sizes)]), torch.int32), proposal_mask=t(proposal_mask, torch.int64),
                P=len(kept), M=int(sizes.sum()), Q=int(valid.sum()))


def voxel_tables(st, feats, fullscale, max_scale, jitter):
    """the re-voxelisation of the stage's proposals by segmented_voxelize -> (voxel_features, voxel_coords [V,4] i32, pc_voxel_id,
    (point_order, voxel_point_start), dropped)"""
    vf, vc, pid, extras = segmented_voxelize(st["pt_xyz"], feats[st["point_indices"]], st["proposal_offsets"], st["proposal_indices"],
                                             st["sizes"], fullscale, max_scale, jitter=jitter, with_extras=True)
    return vf, vc.int(), pid, extras["csr"], extras["dropped"]


def forward_with_masks_formulation(model, pcs, masks, labels, min_points, sample_rows=None):
    """what ``model.forward_with_masks`` must return, from the model's public pieces and ``stage`` (the proposal U-Nets one after the
    other instead of paired - the same values, tests/test_gpu_model.py)"""
    with torch.no_grad():
        batch = model._collate(pcs)
        counts = [int(c) for c in batch.scene_counts]
        feat = model.forward_backbone(pc_batch=batch)
        out = dict(sem_preds=model.forward_sem_seg(feat).argmax(-1), props=None)
        st = stage(batch.points[:, :3], counts, masks, labels, min_points, model.num_part_classes, sample_rows)
        if st is None:
            return out
        vf, vc, pid, csr, dropped = voxel_tables(st, feat, model.score_fullscale, model.score_scale, model.revoxelize_jitter)
        assert dropped == 0
        vt = spconv.SparseConvTensor(vf, vc, spatial_shape=[model.score_fullscale] * 3, batch_size=st["P"])
        vt.point_csr = csr
        props = Instances(proposal_offsets=st["proposal_offsets"], sem_preds=st["sem_preds"])
        score_logits = model.forward_proposal_score(vt, pid, props)
        lab = torch.cat([torch.as_tensor(v).reshape(-1).long() for v in labels]).to(feat.device)[st["proposal_mask"]]
        npcs_logits = model.forward_proposal_npcs(vt, pid)
        cls = st["sem_preds"].long()
        out.update(props=st, voxel_coords=vc, pc_voxel_id=pid, proposal_sem_labels=lab,
                   score_preds=torch.sigmoid(score_logits[torch.arange(lab.shape[0], device=lab.device), lab - 1]),
                   npcs_preds=torch.stack([npcs_logits[torch.arange(cls.shape[0], device=cls.device), 3 * (cls - 1) + k]
                                           for k in range(3)], 1))
        return out


TABLES = ("valid_mask", "valid_indices", "sorted_indices", "point_indices", "proposal_indices", "batch_indices", "pt_xyz", "sem_preds",
          "proposal_offsets", "proposal_mask")


def check_forward_with_masks(got, want, exact=True):
    """``got`` = forward_with_masks' 4-tuple, ``want`` = forward_with_masks_formulation's dict"""
    pc_ids, seg, props, plabels = got
    assert torch.equal(seg.sem_preds, want["sem_preds"])
    assert (props is None) == (want["props"] is None)
    if props is None:
        assert plabels.shape == (0,)
        return
    w = want["props"]
    for f in TABLES:
        a, b = getattr(props, f), w[f]
        assert a.dtype == b.dtype and a.shape == b.shape, (f, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a, b), f
    assert torch.equal(props.num_points_per_proposal, w["sizes"])
    assert torch.equal(props.valid_indices[props.sorted_indices], props.point_indices)  # (the Instances contract)
    assert torch.equal(plabels, want["proposal_sem_labels"]) and plabels.dtype == torch.int64
    M = props.point_indices.shape[0]
    assert props.npcs_preds.shape == (M, 3) and props.npcs_valid_mask.dtype == torch.bool and bool(props.npcs_valid_mask.all())
    assert props.score_preds.shape == (w["P"],)
    if exact:
        assert torch.equal(props.score_preds, want["score_preds"]) and torch.equal(props.npcs_preds, want["npcs_preds"])
    assert props.instance_labels is None and props.sem_labels is None and props.ious is None


def scene_masks(xyz, n_masks, seed, extra=()):
    """``n_masks`` masks over one cloud [n, 3]: points inside random balls (spatially coherent, overlapping: a point sits in
    several), plus the given extra rows -> bool [n_masks + len(extra), n]"""
    rng = np.random.RandomState(seed)
    p = _np(xyz)[:, :3]
    ok = np.isfinite(p).all(1)
    centres = p[ok][rng.randint(ok.sum(), size=n_masks)]
    ext = np.ptp(p[ok], axis=0).max()
    radii = ext * rng.uniform(0.12, 0.3, size=n_masks)
    with np.errstate(invalid="ignore"):
        m = np.linalg.norm(p[None] - centres[:, None], axis=2) < radii[:, None]
    return np.concatenate([m] + [np.asarray(e, bool)[None] for e in extra]) if extra else m


def check_predictions(preds, predictor, clouds, masks, labels, picks, min_points):
    """``PartPredictor.predict_with_masks``' result against a step-by-step restatement from ``forward_with_masks``: every mask of
    every cloud, kept or not.  Boxes and poses agree at 1e-12 relative (the same fit; one multiplication and one addition apart)."""
    from gapartnet_amd import inference
    from gapartnet_amd.misc.pose_fitting_batched import estimate_pose_from_npcs_batched
    from gapartnet_amd.structure.point_cloud import PointCloud
    model = predictor.model
    prep = inference.prepare_clouds(clouds, predictor.num_points)
    dev = prep.source.device
    counts = prep.counts.tolist()
    net_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ok = [s for s, c in enumerate(counts) if c > 0]
    assert [p.status for p in preds] == prep.status.tolist()
    seen = {s: set() for s in range(len(clouds))}
    n_boxes = 0
    if ok:
        pcs = [PointCloud(pc_id=str(s), points=prep.points[net_off[s]:net_off[s + 1], :model.in_channels].contiguous(), obj_cat=0)
               for s in ok]
        _, seg, props, plabels = model.forward_with_masks(pcs, [masks[s] for s in ok], [labels[s] for s in ok], min_points=min_points,
                                                          sample_rows=prep.sample_rows)
        owner = [(s, j) for s in ok for j in range(int(masks[s].shape[0]))]
        if props is not None:
            po = props.proposal_offsets.long()
            sizes = (po[1:] - po[:-1]).tolist()
            fit = estimate_pose_from_npcs_batched(props.pt_xyz, props.npcs_preds - 0.5, po, picks=picks(sizes), max_iters=predictor.max_iters)
            close = lambda a, b: bool(((a - b).abs() <= 1e-12 * b.abs()).all())  # noqa: E731
            for p, g in enumerate(props.proposal_mask.tolist()):
                s, j = owner[g]
                seen[s].add(j)
                o = preds[s]
                a, b = int(po[p]), int(po[p + 1])
                sc = prep.scale[s].to(dev)
                r, c = sc[0], sc[1:]
                assert bool(o.kept[j]) and int(o.n_points[j]) == sizes[p] and int(o.label[j]) == int(plabels[p])
                assert torch.equal(o.score[j], props.score_preds[p])
                box = sizes[p] >= 5 and bool(fit["valid"][p])
                assert bool(o.valid[j]) == box
                lo, hi = int(o.member_offsets[j]), int(o.member_offsets[j + 1])
                assert hi - lo == sizes[p]
                assert torch.equal(o.member_rows[lo:hi], prep.sample_rows[props.point_indices[a:b]])
                assert torch.equal(o.member_npcs[lo:hi], props.npcs_preds[a:b])
                if not box:
                    assert bool(torch.isnan(o.bbox[j]).all()) and bool(torch.isnan(o.scale[j]))
                    continue
                n_boxes += 1
                assert o.bbox.dtype == torch.float64 and close(o.bbox[j], fit["bbox"][p] * r + c)
                assert torch.equal(o.bbox_normalised[j], fit["bbox"][p])
                assert close(o.scale[j], fit["scale"][p] * r) and torch.equal(o.rotation[j], fit["rotation"][p])
                assert close(o.translation[j], fit["translation"][p] * r + c)
                assert close(o.transform[j, :3, :3], fit["transform"][p, :3, :3] * r) and close(o.transform[j, :3, 3], o.translation[j])
                assert o.transform[j, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
                # the box is the NPCS-frame box under the caller-frame similarity: its corners are symmetric about the translation
                q = (o.bbox[j] - o.translation[j]) @ torch.linalg.inv(o.rotation[j]) / o.scale[j]
                assert float((q[0] + q[7]).abs().max()) <= 1e-9 * float(q.abs().max())
        for s in ok:
            a, b = prep.offsets[s], prep.offsets[s + 1]
            samples = slice(int(net_off[s]), int(net_off[s + 1]))
            assert torch.equal(preds[s].sem[prep.sample_rows[samples]] >= 0, torch.ones(counts[s], dtype=torch.bool, device=dev))
            assert torch.equal(preds[s].sampled_sem, seg.sem_preds.long()[samples]) and preds[s].sem.shape == (b - a,)
    for s, o in enumerate(preds):
        K = int(masks[s].shape[0])
        assert o.kept.shape == (K,) and o.bbox.shape == (K, 8, 3) and o.transform.shape == (K, 4, 4) and o.member_offsets.shape == (K + 1,)
        assert torch.equal(o.label, torch.as_tensor(labels[s]).to(dev).long())
        for j in range(K):
            if j in seen[s]:
                continue
            assert not bool(o.kept[j]) and not bool(o.valid[j]) and int(o.n_points[j]) == 0
            assert int(o.member_offsets[j]) == int(o.member_offsets[j + 1])
            assert bool(torch.isnan(o.score[j])) and bool(torch.isnan(o.bbox[j]).all()) and bool(torch.isnan(o.transform[j]).all())
        if s not in ok:
            assert bool((o.sem == -1).all()) and o.member_rows.shape == (0,)
    return n_boxes
