"""Parts from caller-supplied masks, stage by stage (GAPartNet.forward_with_masks; csrc/proposals.hip section MP)
-> profiles/mask_inference_bench.txt.

    python tools/mask_inference_bench.py [--out profiles/mask_inference_bench.txt] [--reps 7] [--clouds 8] [--masks 16]
                                         [--num_points 20000] [--rows 40000]

--clouds raw clouds of --rows rows, sampled to --num_points points, --masks masks per cloud on the raw rows (the points inside
random balls: overlapping, a point sits in several).  Device-event times, the shape warmed up, the median of --reps:
  pack        gpn_mask_pack through the sampling's sample_rows
  mask stage  gpn_proposals_from_masks with its one host read - against the torch formulation of the same stage on the same box
              (GAPartNet.proposals_from_masks_torch: a nonzero per mask, then segmented_voxelize), the two legs taking turns
  U-Nets      the paired proposal U-Nets, the score head and the NPCS head
  fit         estimate_pose_from_npcs_batched, every mask with its own NPCS
and the whole PartPredictor.predict_with_masks call.  The parent commit has no such path: the torch formulation is the baseline.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ball_masks(cloud, n_masks, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = cloud[:, :3]
    ok = torch.isfinite(xyz).all(1)
    pts = xyz[ok]
    centres = pts[torch.randint(pts.shape[0], (n_masks,), generator=g).to(cloud.device)]
    ext = float((pts.amax(0) - pts.amin(0)).max())
    radii = (ext * (0.12 + 0.18 * torch.rand(n_masks, generator=g))).to(cloud.device)
    return ((xyz[None] - centres[:, None]).norm(dim=2) < radii[:, None]) & ok[None]


def main():
    from inference_bench import alternating, make_clouds, timed
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_inference_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--masks", type=int, default=16)
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=40000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_inference_bench needs a GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    from gapartnet_amd import hip_ops, inference
    from gapartnet_amd.misc.pose_fitting_batched import draw_picks, estimate_pose_from_npcs_batched
    from gapartnet_amd.smoke import make_model
    from gapartnet_amd.structure.point_cloud import PointCloud
    S, K, m = args.clouds, args.masks, args.num_points
    model = make_model((0, 0)).to(dev).eval()
    model.revoxelize_jitter = (torch.tensor([0.3, 0.6, 0.1], device=dev), torch.tensor([0.5, 0.2, 0.9], device=dev))
    predictor = inference.PartPredictor(model, num_points=m)
    clouds = make_clouds(S, args.rows, dev)
    masks = [ball_masks(c, K, 100 + s) for s, c in enumerate(clouds)]
    labels = [torch.randint(1, model.num_part_classes, (K,), generator=torch.Generator().manual_seed(s)).to(dev) for s in range(S)]
    prep = inference.prepare_clouds(clouds, m)
    counts = prep.counts.tolist()
    net_off = np.concatenate([[0], np.cumsum(counts)]).tolist()
    pcs = [PointCloud(pc_id=str(s), points=prep.points[net_off[s]:net_off[s + 1], :model.in_channels].contiguous(), obj_cat=0)
           for s in range(S)]
    with torch.no_grad():
        batch = model._collate(pcs)
        xyz = batch.points[:, :3]
        feat = model.forward_backbone(pc_batch=batch)
        flat, per, lab = model._mask_lists(counts, masks, labels, prep.sample_rows, dev)
        tables = hip_ops.mask_tables(counts, per, dev)
        base = [s * K * args.rows + j * args.rows for s in range(S) for j in range(K)]
        flat1 = torch.cat([f.reshape(-1) for f in flat])
        state = {}

        def pack():
            state["bits"] = hip_ops.mask_pack(flat1, base, tables, prep.sample_rows)

        def stage_kernels():
            state["built"] = hip_ops.proposals_from_masks(state["bits"], tables, lab, xyz, model.num_part_classes, 6,
                                                          float(model.score_fullscale), float(model.score_scale), model.revoxelize_jitter)

        def stage_torch():
            state["torch"] = model.proposals_from_masks_torch(xyz, feat, counts, flat, per, lab, 6, prep.sample_rows,
                                                              model.revoxelize_jitter)

        def unets():
            vt, pid, props = state["stage"]
            pair = model.forward_proposal_unets(vt)
            state["score"] = model.forward_proposal_score(vt, pid, props, pair[0] if pair else None)
            logits = model.forward_proposal_npcs(vt, pid, pair[1] if pair else None, None)
            cls = props.sem_preds.long()
            state["npcs"] = logits.reshape(logits.shape[0], -1, 3).gather(1, (cls - 1)[:, None, None].expand(-1, 1, 3)).squeeze(1)

        def fit():
            props = state["stage"][2]
            state["fit"] = estimate_pose_from_npcs_batched(props.pt_xyz, state["npcs"] - 0.5, props.proposal_offsets.long(),
                                                           picks=state["picks"], max_iters=predictor.max_iters)

        pack(), stage_kernels(), stage_torch()   # warm-up
        b, t = state["built"], state["torch"][2]
        assert torch.equal(b["point_indices"], t.point_indices) and torch.equal(b["proposal_offsets"], t.proposal_offsets)
        state["stage"] = model._proposals_from_masks(xyz, feat, counts, flat, per, lab, 6, prep.sample_rows)
        np.random.seed(0)
        state["picks"] = draw_picks(b["sizes"].tolist(), predictor.max_iters).to(dev)
        unets(), fit()
        whole = lambda: predictor.predict_with_masks(clouds, masks, labels, picks=state["picks"])  # noqa: E731
        whole()
        lines = [f"parts from caller-supplied masks: {S} clouds x {args.rows} rows -> {m} sampled points, {K} masks per cloud "
                 f"({b['P']} kept, {b['M']} member points, {b['V']} voxels)",
                 f"median [min .. max] of {args.reps} in ms (device events), the shape warmed up; device: {torch.cuda.get_device_name(0)}", ""]
        res = {"pack": timed(pack, args.reps)}
        res.update(alternating({"mask stage (kernels)": stage_kernels, "mask stage (torch)": stage_torch}, args.reps))
        res["U-Nets + heads"] = timed(unets, args.reps)
        res["fit"] = timed(fit, args.reps)
        res["predict_with_masks"] = timed(whole, args.reps)
        for k, (med, lo, hi) in res.items():
            lines.append(f"  {k:<22} {med:9.3f} [{lo:9.3f} .. {hi:9.3f}]")
        lines.append(f"  mask stage: the torch formulation takes {res['mask stage (torch)'][0] / res['mask stage (kernels)'][0]:.1f} x "
                     f"the kernels' time")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
