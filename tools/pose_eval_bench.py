"""Pose evaluation: the three entry points of csrc/poseeval.hip and a whole PoseEvaluator.update, each against the torch formulation
of the same contract on the same GPU (gapartnet_amd/misc/pose_metrics.py) -> profiles/pose_eval_bench.txt.

    python tools/pose_eval_bench.py [--out profiles/pose_eval_bench.txt] [--reps 7]

Workload: 8 scenes x 20 000 points, 20 instances a scene (about 900 points each, the rest background), every instance with its
own pose; 128 matched pairs over all five symmetry types (a prediction a few degrees and per cent off a candidate of its type);
128 box pairs for the IoU alone.  The parent commit has no such path, so the baseline is the torch formulation: what its user
could have written.  The two legs of ``update`` differ in the three new stages only: both run the proposals' fit through
gpn_pose_fit, which the parent has.
Method: device events around each call, a warm-up of every leg, then --reps rounds in which the legs take turns; medians.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES, POINTS, INSTANCES, PAIRS = 8, 20000, 20, 128


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def take_turns(legs, reps):
    """legs: name -> callable.  One warm-up each, then `reps` rounds, the legs alternating -> name -> list of ms"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn)[0])
    return times


def line(name, ms):
    return f"  {name:<46s}{statistics.median(ms):10.3f} [{min(ms):10.3f} .. {max(ms):10.3f}]"


def scene_batch(dev, seed=0):
    from tests.pose_eval_cases import random_rotation
    rng = np.random.default_rng(seed)
    xyz, npcs, lab = [], [], []
    per = POINTS // (INSTANCES + 2)
    for s in range(SCENES):
        ids = np.concatenate([np.repeat(np.arange(INSTANCES), per), np.full(POINTS - INSTANCES * per, -1)])
        q = rng.uniform(-0.4, 0.4, (POINTS, 3))
        x = rng.normal(size=(POINTS, 3))
        for w in range(INSTANCES):
            sel = ids == w
            x[sel] = q[sel] @ (rng.uniform(0.2, 1.0) * random_rotation(rng)) + rng.uniform(-0.5, 0.5, 3)
        order = rng.permutation(POINTS)
        xyz.append(x[order]), npcs.append(q[order]), lab.append(ids[order])
    t = lambda a, d: torch.from_numpy(np.concatenate(a)).to(d).to(dev)
    return t(xyz, torch.float32), t(npcs, torch.float32), t(lab, torch.int64), [s * POINTS for s in range(SCENES + 1)]


def evaluator_batch(dev, xyz, npcs, lab, off):
    """the proposals are the first 16 instances of every scene (128 pairs) with their NPCS turned by 3 degrees"""
    from gapartnet_amd.structure.instances import Instances
    from gapartnet_amd.structure.point_cloud import PointCloudBatch
    from tests.pose_eval_cases import rot
    Q = torch.from_numpy(rot([1.0, 2.0, 3.0], 3.0)).float().to(dev)
    rows, p_off, cls, ious, labels = [], [0], [], [], torch.zeros(SCENES, INSTANCES, dtype=torch.int32)
    for s in range(SCENES):
        labels[s] = torch.arange(INSTANCES) % 9 + 1
        for w in range(PAIRS // SCENES):
            r = off[s] + torch.nonzero(lab[off[s]:off[s + 1]] == w).squeeze(1)
            rows.append(r), p_off.append(p_off[-1] + int(r.numel())), cls.append(int(labels[s, w]))
            row = torch.zeros(INSTANCES)
            row[w] = 1.0
            ious.append(row)
    rows = torch.cat(rows)
    bidx = torch.repeat_interleave(torch.arange(SCENES, device=dev), POINTS)
    kept = Instances(pt_xyz=xyz[rows], score_preds=torch.linspace(0.9, 0.5, PAIRS, device=dev), pt_sem_classes=torch.tensor(cls, device=dev),
                     batch_indices=bidx[rows], proposal_offsets=torch.tensor(p_off, device=dev), instance_sem_labels=labels.to(dev),
                     ious=torch.stack(ious).to(dev), npcs_preds=npcs[rows] @ Q + 0.5,
                     npcs_valid_mask=torch.ones(rows.numel(), dtype=torch.bool, device=dev))
    batch = PointCloudBatch(pc_ids=[str(s) for s in range(SCENES)], points=xyz, batch_indices=bidx, batch_size=SCENES, instance_labels=lab,
                            instance_sem_labels=labels.to(dev), gt_npcs=npcs)
    return kept, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_eval_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from gapartnet_amd.misc import pose_metrics as PM
    from gapartnet_amd.smoke import DEFAULT_CFG
    from tests.pose_eval_cases import pair_dicts, random_box_pairs, random_pairs
    dev = torch.device("cuda:0")
    out = [f"pose evaluation: {SCENES} scenes x {POINTS} points, {INSTANCES} instances a scene, {PAIRS} pairs over the five symmetry types",
           f"median [min .. max] of {args.reps} in ms by device events, after a warm-up of every leg; the legs take turns",
           f"device: {torch.cuda.get_device_name(0)}", ""]
    xyz, npcs, lab, off = scene_batch(dev)
    fit = lambda force_torch=False: PM.gt_part_poses(xyz, npcs, lab, off, INSTANCES, force_torch=force_torch)
    t = take_turns({"kernel": fit, "torch": lambda: fit(True)}, args.reps)
    a, b = fit(), fit(True)
    out += [f"== gpn_pose_gt_fit: {SCENES * INSTANCES} slots, one launch ==", line("kernel", t["kernel"]), line("torch formulation, same GPU", t["torch"]),
            f"  torch / kernel: {statistics.median(t['torch']) / statistics.median(t['kernel']):.2f} x; max |R kernel - R torch| "
            f"{float((a['rotation'] - b['rotation']).abs().max()):.1e}", ""]

    boxes = random_box_pairs(PAIRS, 11)
    ba, bb = (torch.from_numpy(np.stack([p[i] for p in boxes])).to(dev) for i in (0, 1))
    iou = lambda force_torch=False: PM.oriented_box_iou(ba, bb, force_torch=force_torch)
    t = take_turns({"kernel": iou, "torch": lambda: iou(True)}, args.reps)
    out += [f"== gpn_box_iou_3d: {PAIRS} pairs, one launch ==", line("kernel", t["kernel"]), line("torch formulation, same GPU", t["torch"]),
            f"  torch / kernel: {statistics.median(t['torch']) / statistics.median(t['kernel']):.2f} x; max |IoU kernel - IoU torch| "
            f"{float((iou() - iou(True)).abs().max()):.1e}", ""]

    pred, gt, ty = pair_dicts(random_pairs(21, PAIRS), dev)
    err = lambda force_torch=False: PM.pose_pair_errors(pred, gt, ty, force_torch=force_torch)
    t = take_turns({"kernel": err, "torch": lambda: err(True)}, args.reps)
    a, b = err(), err(True)
    out += [f"== gpn_pose_pair_errors: {PAIRS} pairs, up to 24 candidates each, one launch ==", line("kernel", t["kernel"]),
            line("torch formulation, same GPU", t["torch"]),
            f"  torch / kernel: {statistics.median(t['torch']) / statistics.median(t['kernel']):.2f} x; max |re| difference "
            f"{float((a['re_deg'] - b['re_deg']).abs().max()):.1e}, max |IoU| difference {float((a['iou'] - b['iou']).abs().max()):.1e}", ""]

    kept, batch = evaluator_batch(dev, xyz, npcs, lab, off)
    picks_cache = {}

    def picks(sizes):  # (drawn once: the draw itself is host work both legs share)
        key = tuple(sizes)
        if key not in picks_cache:
            picks_cache[key] = torch.from_numpy(np.stack([np.random.RandomState(7).randint(int(n), size=(100, 5)) for n in sizes])).to(dev)
        return picks_cache[key]

    def update(force_torch=False):
        ev = PM.PoseEvaluator(10, DEFAULT_CFG["symmetry_indices"], picks=picks, force_torch=force_torch)
        ev.update(kept, batch)
        return ev

    t = take_turns({"kernel": update, "torch": lambda: update(True)}, args.reps)
    res = update().compute()
    # the stages of the kernel leg, each alone
    m = PM.match_pairs(kept)
    stages = {"match_pairs": lambda: PM.match_pairs(kept), "gpn_pose_gt_fit (batch ground truth)": fit, "gpn_pose_pair_errors": err}
    from gapartnet_amd.misc.pose_fitting_batched import estimate_pose_from_npcs_batched
    po = kept.proposal_offsets
    stages["gpn_pose_fit (128 proposals, 100 hypotheses)"] = lambda: estimate_pose_from_npcs_batched(
        kept.pt_xyz, kept.npcs_preds - 0.5, po, picks=picks((po[1:] - po[:-1]).tolist()))
    ts = take_turns(stages, args.reps)
    out += [f"== PoseEvaluator.update: {int(m['proposal'].numel())} pairs matched, {res['total_pairs']} evaluated ==", line("with the kernels", t["kernel"]),
            line("with the torch formulation of the new stages", t["torch"]),
            f"  torch / kernel: {statistics.median(t['torch']) / statistics.median(t['kernel']):.2f} x", "  stages of the kernel leg, each timed alone:"]
    out += ["  " + line(k, v) for k, v in ts.items()]
    bound = max(ts, key=lambda k: statistics.median(ts[k]))
    rest = statistics.median(t["kernel"]) - sum(statistics.median(v) for v in ts.values())
    out += [f"  the largest stage is {bound}; update minus the four stages = {rest:.3f} ms of torch glue (index building, two host reads of sizes)", ""]
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
