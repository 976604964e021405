"""Pose evaluation on the host (gapartnet_amd/misc/pose_metrics.py): the numpy restatement (tests/pose_eval_ref.py) against scipy's
half-space intersection, the exact cases of the tie rule, the torch formulations against the restatement, recovery of known poses,
the symmetry-aware angle, the matching against the sequential AP walk, the evaluator against closed forms, the model switch, and
the renderer's NPCS frames recovered from a rendered view."""
import numpy as np
import pytest
import torch

from gapartnet_amd.misc import pose_metrics as PM
from gapartnet_amd.misc.info import PART_ID2NAME, SYMMETRY_MATRIX
from tests import pose_eval_ref as ref
from tests.pose_eval_cases import (assert_first_extrema, first_extremum_case, FIT_KINDS, FIT_SIZES, SYM_OF_CLASS, assert_fit_equals_ref, assert_pair_errors_equal_ref,
                                   coplanar_rotations, evaluator_case, turned_self_pairs, exact_cases, make_instances, pair_dicts, random_box_pairs,
                                   random_pairs, random_rotation, ref_pair_errors, rot, slots_of)



# ------------------------------------------------------------------------------------------------ box IoU
def test_restatement_equals_scipy_on_random_pairs():
    worst, overlapping = 0.0, 0
    for a, b in random_box_pairs(240, 7):
        inter, va, vb = ref.box_intersection(a, b)
        want = ref.scipy_intersection_volume(a, b)
        overlapping += want > 0
        worst = max(worst, abs(inter - want) / max(va, vb))
    print(f"worst |volume - scipy| / larger box volume = {worst:.3g} over 240 pairs, {overlapping} overlapping")
    assert overlapping >= 100
    assert worst <= 1e-12


@pytest.mark.parametrize("name", list(exact_cases()))
def test_exact_cases(name):
    a, b, want = exact_cases()[name]
    assert abs(ref.box_iou(a, b) - want) <= 1e-12
    assert abs(float(PM.oriented_box_iou(torch.from_numpy(a)[None], torch.from_numpy(b)[None])[0]) - want) <= 1e-12


def test_a_turned_box_against_itself_and_against_a_copy_off_by_round_off():
    """what the snap of the tie rule is for: with an exact test these come out anywhere between 0.1 and 15"""
    pairs = turned_self_pairs()
    for i, (a, b) in enumerate(pairs):
        assert abs(ref.box_iou(a, b) - 1.0) <= 1e-12, i
    a, b = (torch.from_numpy(np.stack([p[j] for p in pairs])) for j in (0, 1))
    assert float((PM.oriented_box_iou(a, b) - 1.0).abs().max()) <= 1e-12


def test_coplanar_rotations_equal_scipy():
    for a, b in coplanar_rotations():
        inter, va, vb = ref.box_intersection(a, b)
        assert abs(inter - ref.scipy_intersection_volume(a, b)) / max(va, vb) <= 1e-12
        got = float(PM.oriented_box_iou(torch.from_numpy(a)[None], torch.from_numpy(b)[None])[0])
        assert abs(got - inter / (va + vb - inter)) <= 1e-10


def test_torch_iou_equals_the_restatement():
    pairs = random_box_pairs(120, 11) + random_box_pairs(40, 12, max_aspect=100.0)
    a, b = (torch.from_numpy(np.stack([p[i] for p in pairs])) for i in (0, 1))
    want = np.array([ref.box_iou(*p) for p in pairs])
    assert np.abs(PM.oriented_box_iou(a, b).numpy() - want).max() <= 1e-10
    bad = a.clone()
    bad[0, 3, 1] = float("nan")
    bad[1] = bad[1, :1]  # every corner the same point: no volume
    got = PM.oriented_box_iou(bad, b)
    assert torch.isnan(got[:2]).all() and torch.isfinite(got[2:]).all()
    assert PM.oriented_box_iou(a[:0], b[:0]).shape == (0,)


# ------------------------------------------------------------------------------------------------ the instance fit
def test_gt_part_poses_torch_equals_the_restatement():
    W = 7
    xyz, npcs, lab, off, _ = make_instances(3, FIT_SIZES, W, FIT_KINDS)
    got = PM.gt_part_poses(torch.from_numpy(xyz), torch.from_numpy(npcs), torch.from_numpy(lab), off, W)
    want = ref.fit_slots(xyz, npcs, slots_of(lab, off, W), off, W)
    assert_fit_equals_ref(got, want, 1e-10)
    valid = got["valid"].reshape(2, W).tolist()
    assert valid[0] == [False, False, True, True, True, False, True] and valid[1] == [True, True, False, False, False, False, True]


def test_gt_part_poses_recovers_known_poses():
    W = 4
    xyz, npcs, lab, off, poses = make_instances(5, [[50, 400, 9, 120], [2000, 33, 64, 65]], W)
    got = PM.gt_part_poses(torch.from_numpy(xyz), torch.from_numpy(npcs), torch.from_numpy(lab), off, W)
    for s, w, scale, R, t in poses:
        g = s * W + w
        assert bool(got["valid"][g])
        assert ref.angle_deg(got["rotation"][g].numpy(), R) <= 1e-4
        assert abs(float(got["scale"][g]) - scale) <= 1e-5 * scale
        assert np.linalg.norm(got["translation"][g].numpy() - t) <= 1e-5 * np.linalg.norm(t)


# ------------------------------------------------------------------------------------------------ pair errors
def test_pose_pair_errors_torch_equals_the_restatement():
    d = random_pairs(21, 40)
    got = PM.pose_pair_errors(*pair_dicts(d))
    compared = assert_pair_errors_equal_ref(got, ref_pair_errors(d), 1e-10)
    assert compared[0] >= 30
    pred, gt, ty = pair_dicts(d)
    ty[0], pred["scale"][1] = 9, float("nan")
    got = PM.pose_pair_errors(pred, gt, ty)
    assert np.isnan(float(got["re_deg"][0])) and int(got["k_re"][0]) == -1 and int(got["k_iou"][0]) == -1
    assert np.isnan(float(got["iou"][1])) and np.isnan(float(got["se"][1])) and np.isfinite(float(got["re_deg"][1]))


def test_pose_pair_errors_torch_returns_the_first_extremum():
    d, table, want = first_extremum_case()
    pred, gt, ty = pair_dicts(d)
    got = PM.pose_pair_errors(pred, gt, ty, table=table)
    assert_first_extrema(got, d, want)
    for i, w in enumerate(want):
        assert abs(float(got["re_deg"][i]) - w["re_deg"]) <= 1e-10 and abs(float(got["iou"][i]) - w["iou"]) <= 1e-10, i
    # type 0 of SYMMETRY_MATRIX is [I, I]: a bit-exact tie, the first candidate is the answer
    d0 = random_pairs(3, 10)
    got = PM.pose_pair_errors(*pair_dicts(d0))
    sel = torch.from_numpy(d0["ty"] == 0)
    assert int(sel.sum()) == 2 and (got["k_re"][sel] == 0).all() and (got["k_iou"][sel] == 0).all()


def test_rotation_error_under_each_symmetry_type():
    rng = np.random.default_rng(4)
    Rg = random_rotation(rng)
    want = {0: 100.0, 1: 80.0, 2: 100.0, 3: 10.0, 4: 10.0}
    n = len(want)
    one = lambda v: torch.from_numpy(np.broadcast_to(np.asarray(v, np.float64), (n,) + np.shape(v)).copy())
    gt = {"scale": one(1.0), "rotation": one(Rg), "translation": one(np.zeros(3)), "half": one([0.3, 0.2, 0.1])}
    pred = dict(gt, rotation=one(rot([0, 0, 1], 100.0) @ Rg))
    got = PM.pose_pair_errors(pred, gt, torch.arange(n, dtype=torch.int32))
    for ty, deg in want.items():
        assert abs(float(got["re_deg"][ty]) - deg) <= 1e-9, ty
    # a prediction equal to any candidate of its type is right
    for ty, group in enumerate(SYMMETRY_MATRIX):
        k = len(group)
        many = lambda v: torch.from_numpy(np.broadcast_to(np.asarray(v, np.float64), (k,) + np.shape(v)).copy())
        gt = {"scale": many(1.0), "rotation": many(Rg), "translation": many(np.zeros(3)), "half": many([0.3, 0.2, 0.1])}
        pred = dict(gt, rotation=torch.from_numpy(np.array(group) @ Rg))
        got = PM.pose_pair_errors(pred, gt, torch.full((k,), ty, dtype=torch.int32))
        assert float(got["re_deg"].max()) < 1e-6, ty


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("quantised", [False, True])
def test_match_pairs_are_the_true_positives_of_the_sequential_walk(seed, quantised):
    from oracle import eval_ap
    from tests.test_eval_ap import _random_set
    rng = np.random.default_rng(seed)
    sets = [_random_set(rng, int(rng.integers(0, 60)), int(rng.integers(1, 5)), int(rng.integers(1, 12)), quantised)
            for _ in range(int(rng.integers(1, 5)))]
    if all(s.score_preds.shape[0] == 0 for s in sets):
        sets.append(_random_set(rng, 10, 2, 5, quantised))
    set_of = np.concatenate([np.full(s.score_preds.shape[0], i) for i, s in enumerate(sets)])
    local = np.concatenate([np.arange(s.score_preds.shape[0]) for s in sets])
    order = torch.argsort(torch.cat([s.score_preds for s in sets]), descending=True).numpy()
    for thr in (0.25, 0.5, 0.75):
        tp, _, _ = eval_ap.compute_tp_fp_sequential(sets, thr)
        want = sorted((int(set_of[i]), int(local[i])) for i in order[tp > 0])
        m = PM.match_pairs(sets, thr)
        assert sorted(zip(m["set"].tolist(), m["proposal"].tolist())) == want
        for i, p, sc, ins, c in zip(*(m[k].tolist() for k in ("set", "proposal", "scene", "instance", "cls"))):
            s = sets[i]
            assert sc == int(s.batch_indices[s.proposal_offsets[p]]) and c == int(s.pt_sem_classes[p])
            assert int(s.instance_sem_labels[sc, ins]) == c and float(s.ious[p, ins]) > thr


# ------------------------------------------------------------------------------------------------ the evaluator
def test_pose_evaluator_equals_the_closed_forms():
    kept, batch, picks, expect = evaluator_case()
    ev = PM.PoseEvaluator(10, SYM_OF_CLASS, picks=picks)
    ev.update(kept, batch)
    ev.update(None, batch)   # a batch without proposals still counts its ground truth
    out = ev.compute()
    assert out["pairs"].tolist() == [2, 0, 0, 0, 1, 0, 0, 1, 0] and out["total_pairs"] == 4
    assert out["gt_instances"].tolist() == [4, 0, 2, 2, 2, 0, 2, 2, 2]
    assert out["dropped_no_pose"][7 - 1] == 1 and out["dropped_no_pose"][[0, 4, 7]].sum() == 0
    assert out["dropped_degenerate_gt"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    # float32 inputs (6e-8 relative) over lever arms of 0.2 and more: a few 1e-5 degrees, a few 1e-7 in length
    for c, rows in expect.items():
        assert abs(out["Re"][c - 1] - np.mean([r[0] for r in rows])) <= 2e-4, c
        assert abs(out["Te"][c - 1] - np.mean([r[1] for r in rows])) <= 1e-5, c
        assert abs(out["Se"][c - 1] - np.mean([r[2] for r in rows])) <= 1e-5, c
        assert out["A5"][c - 1] == np.mean([r[0] <= 5 and r[1] <= 0.05 for r in rows]), c
        assert out["A10"][c - 1] == np.mean([r[0] <= 10 and r[1] <= 0.10 for r in rows]), c
        assert abs(out["mIoU"][c - 1] - np.mean([r[3] for r in rows])) <= 1e-5, c
        assert 0.0 < out["mIoU"][c - 1] < 1.0
    for c in range(1, 10):
        if c not in expect:
            assert all(np.isnan(out[k][c - 1]) for k in ("Re", "Te", "Se", "mIoU", "A5", "A10")), c
    have = sorted(expect)
    for k in ("Re", "Te", "Se", "mIoU", "A5", "A10"):
        assert abs(out["mean"][k] - np.mean([out[k][c - 1] for c in have])) <= 1e-15
    # scene_scale multiplies the two lengths, per scene
    ev2 = PM.PoseEvaluator(10, SYM_OF_CLASS, picks=picks, scene_scale=[2.0, 2.0])
    ev2.update(kept, batch)
    out2 = ev2.compute()
    assert np.allclose(out2["Te"][[0, 4, 7]], 2.0 * out["Te"][[0, 4, 7]], rtol=1e-12) and np.allclose(out2["Re"][[0, 4, 7]], out["Re"][[0, 4, 7]])
    empty = PM.PoseEvaluator(10, SYM_OF_CLASS).compute()
    assert empty["total_pairs"] == 0 and np.isnan(empty["mean"]["Re"])


# ------------------------------------------------------------------------------------------------ the model switch
def _test_epoch_keys(evaluate_pose):
    from gapartnet_amd import backend
    from gapartnet_amd.smoke import DEFAULT_CFG, make_batch
    from gapartnet_amd.network.model import GAPartNet
    from gapartnet_amd.trainer import MetricLog
    from oracle import torch_ops
    import copy
    cfg = copy.deepcopy(DEFAULT_CFG)
    cfg["training_schedule"], cfg["backbone_cfg"]["channels"] = [0, 0], [16, 32, 48]
    if evaluate_pose is not None:
        cfg["evaluate_pose"] = evaluate_pose
    with backend.using(torch_ops):
        torch.manual_seed(0)
        np.random.seed(0)
        model = GAPartNet(**cfg)
        model.eval()
        log = MetricLog()
        model._log_sink = log
        returned = []
        with torch.no_grad():
            for loader_idx in range(3):
                returned.append(model.test_step(make_batch(2, 2500, seed0=2000 + 10 * loader_idx), 0, loader_idx))
        model.on_test_epoch_end()
        assert model.validation_step_outputs == [] and model._pose_evaluators == {}
        return log.reduce(torch.device("cpu")), returned


def test_the_switch_adds_its_seven_keys_and_nothing_else():
    base, returned = _test_epoch_keys(None)
    off, _ = _test_epoch_keys(False)
    on, returned_on = _test_epoch_keys(True)
    splits = ("val", "test_intra", "test_inter")
    parent = {f"{s}/{k}" for s in splits for k in ["AP@50", "mAP", "all_accu", "pixel_accu", "miou"] + [f"AP@50_{PART_ID2NAME[c]}" for c in range(1, 10)]}
    parent |= {f"monitor_metrics/{k}" for k in ("mean_all_accu", "mean_pixel_accu", "mean_imou", "mean_AP@50", "mean_mAP")}
    # (the steps log their losses and accuracies as well: `parent` is what the epoch end logs, the rest comes with it unchanged)
    assert parent <= set(base) and set(off) == set(base) and not any("pose" in k for k in base)
    assert all(base[k] == off[k] or (np.isnan(base[k]) and np.isnan(off[k])) for k in base)
    pose = {f"{s}/pose_{k}" for s in splits for k in ("Re", "Te", "Se", "mIoU", "A5", "A10", "pairs")}
    assert set(base) <= set(on) and set(on) - set(base) <= pose and {f"{s}/pose_pairs" for s in splits} <= set(on)
    assert all(on[k] == off[k] or (np.isnan(on[k]) and np.isnan(off[k])) for k in base)
    print({k: on[k] for k in sorted(set(on) - set(base))})
    assert all(len(r) == 3 for r in returned_on)  # the returned tuple stays the reference's


# ------------------------------------------------------------------------------------------------ the renderer's frames
def test_rendered_views_give_back_their_npcs_frames():
    """every link of the fixture asset's golden view, rendered at 96 x 96 by the numpy path, with >= 64 visible pixels and an NPCS
    covariance of rank >= 2: gt_part_poses on the back-projected pixels reproduces the rotation of npcs_frames.  A pixel is
    camera = npcs @ (scaler R_frame R_camera) + (T - t) @ R_camera; float32 depth and NPCS leave about 1e-4 degrees."""
    import os
    from gapartnet_amd.dataset import render_assets as RA
    from tests import render_ref as RR
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_asset.npz"))
    asset = RA.load_asset(RR.fixture_asset())
    qpos = {str(n): float(q) for n, q in zip(golden["joint_names"], golden["qpos"])}
    H = W = 96
    g = RA.geometry_tables([asset])
    t, extras = RA.view_tables([asset], [RA.RenderRequest(0, qpos, golden["camera_pos"])], H, W)
    out = RA.render_tables_numpy(g, t)
    K, Rc = extras[0]["K"], extras[0]["R"]
    ys, xs = np.mgrid[0:H, 0:W]
    z = out["depth"][0].astype(np.float64)
    pc = np.stack([(xs - K[0, 2]) * z / K[0, 0], (ys - K[1, 2]) * z / K[1, 1], z], -1).reshape(-1, 3).astype(np.float32)
    ins, npcs = out["ins"][0].reshape(-1), out["npcs"][0].reshape(-1, 3)
    n_inst = int(ins.max()) + 1
    got = PM.gt_part_poses(torch.from_numpy(pc), torch.from_numpy(npcs), torch.from_numpy(ins.astype(np.int64)), [0, H * W], n_inst)
    qualified = 0
    for li, inst in enumerate(out["link_inst"][0]):
        if inst < 0 or int(got["count"][inst]) < 64 or not bool(got["valid"][inst]):
            continue
        frame = extras[0]["frames"][asset.links[li]]
        err = ref.angle_deg(got["rotation"][inst].numpy(), np.asarray(frame["R"]) @ Rc)
        print(f"{asset.links[li]}: {int(got['count'][inst])} pixels, rotation off by {err:.2e} degrees")
        assert err <= 0.01 and abs(float(got["scale"][inst]) / frame["scaler"] - 1.0) <= 1e-4
        qualified += 1
    print(f"{qualified} links qualified")
    assert qualified >= 1
