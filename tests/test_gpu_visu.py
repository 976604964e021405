"""Test-time rendering on the GPU (csrc/visu.hip through gapartnet_amd.hip_ops and gapartnet_amd/misc/visu.py): integer outputs
from IEEE float64 arithmetic, so every comparison with the fixture of the reference's visualize_gapartnet
(tests/golden/visu_panels.npz) and with the numpy restatement (tests/visu_ref.py) is byte for byte."""
import os

import numpy as np
import pytest
import torch

from tests import visu_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_CAM = (60.0, 45.0, 30.5, 20.25)   # a 48 x 64 image with its own intrinsics: fx != fy, u0 != v0, H != W
SMALL_H, SMALL_W, SMALL_EDGE = 48, 64, 4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "visu_panels.npz"))


def _tile(canvas, name, H, W, edge):
    y0, x0 = R.tile_origin(name, H, W, edge)
    return canvas[y0:y0 + H, x0:x0 + W]


def _cat(scenes, key, dtype, cuda):
    return torch.as_tensor(np.concatenate([np.asarray(sc[key]) for sc in scenes]).astype(dtype)).to(cuda)


def _render(scenes, cuda, palette, H, W, edge, cam, options=tuple(R.TILE_POS)):
    from gapartnet_amd.misc import visu
    off = np.concatenate([[0], np.cumsum([sc["xyz"].shape[0] for sc in scenes])])
    boxes = {k: torch.as_tensor(np.concatenate([np.asarray(sc[k], dtype=np.float64).reshape(-1, 8, 3) for sc in scenes])).to(cuda)
             for k in ("bbox_pred", "bbox_gt")}
    where = {k: torch.as_tensor(np.concatenate([np.full(np.asarray(sc[k]).reshape(-1, 8, 3).shape[0], s) for s, sc in
                                                enumerate(scenes)]).astype(np.int32)).to(cuda) for k in ("bbox_pred", "bbox_gt")}
    return visu.render_panels(
        _cat(scenes, "xyz", np.float32, cuda), _cat(scenes, "rgb", np.float32, cuda), off,
        torch.as_tensor(np.stack([sc["trans"] for sc in scenes])).to(cuda), sem_pred=_cat(scenes, "sem_pred", np.int32, cuda),
        ins_pred=_cat(scenes, "ins_pred", np.int32, cuda), npcs_pred=_cat(scenes, "npcs_pred", np.float32, cuda),
        bbox_pred=boxes["bbox_pred"], bbox_pred_scene=where["bbox_pred"], sem_gt=_cat(scenes, "sem_gt", np.int32, cuda),
        ins_gt=_cat(scenes, "ins_gt", np.int32, cuda), npcs_gt=_cat(scenes, "npcs_gt", np.float32, cuda), bbox_gt=boxes["bbox_gt"],
        bbox_gt_scene=where["bbox_gt"], raw=[sc.get("raw") for sc in scenes], options=options, H=H, W=W, EDGE=edge, fx=cam[0],
        fy=cam[1], u0=cam[2], v0=cam[3], palette=palette)


def test_panels_equal_the_reference_fixture_and_the_restatement(cuda, gold):
    """both fixture scenes as one batch of two: winner, every colour rule, the layout and the boxes"""
    from gapartnet_amd import hip_ops
    H, W, EDGE = R.golden_geometry(gold)
    scenes = [R.golden_scene(gold, s) for s in range(2)]
    off = torch.tensor([0, scenes[0]["xyz"].shape[0], scenes[0]["xyz"].shape[0] + scenes[1]["xyz"].shape[0]], device=cuda)
    winner = hip_ops.points_winner(_cat(scenes, "xyz", np.float32, cuda), off,
                                   torch.as_tensor(np.stack([sc["trans"] for sc in scenes])).to(cuda), H, W, *R.CAM).cpu().numpy()
    runs = [_render(scenes, cuda, gold["COLOR20"], H, W, EDGE, R.CAM).cpu().numpy() for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]), "two runs are bit-identical"
    assert runs[0].shape == (2,) + R.canvas_shape(H, W, EDGE) + (3,) and runs[0].dtype == np.uint8
    for s, scene in enumerate(scenes):
        assert np.array_equal(winner[s], R.points_winner(scene["xyz"], scene["trans"], H, W)), s
        want = R.render_tiles(scene, gold["COLOR20"], H, W)
        for name in R.TILE_POS:
            got = _tile(runs[0][s], name, H, W, EDGE)
            assert np.array_equal(got, want[name]), (s, name)                         # the restatement, lines included
            if not name.startswith("bbox"):
                assert np.array_equal(got, gold[f"s{s}_tile_{name}"]), (s, name)       # what the reference wrote
        assert np.array_equal(runs[0][s], R.assemble(want, H, W, EDGE)), s
        lines = np.zeros(runs[0][s].shape[:2], bool)
        for name in ("bbox_pred", "bbox_pred_pure", "bbox_gt", "bbox_gt_pure"):
            y0, x0 = R.tile_origin(name, H, W, EDGE)
            white = np.full((H, W, 3), 255, np.uint8)
            boxes = scene["bbox_pred" if "pred" in name else "bbox_gt"]
            lines[y0:y0 + H, x0:x0 + W] = (R.draw_boxes(white.copy(), boxes, scene["trans"]) != white).any(-1)
        assert np.array_equal(runs[0][s][~lines], gold[f"s{s}_canvas"][~lines]), "the reference's canvas outside the line pixels"


def _small_scene(rng, n):
    """points around a 48 x 64 view: in and out of the image, on and behind the camera plane, colours in and out of range"""
    xyz = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), rng.uniform(-0.2, 1.0, n)], 1).astype(np.float32)
    xyz[rng.random(n) < 0.05, 2] = -0.75                     # z_cam = 0 for trans (2, ., ., 1.5)
    rgb = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    rgb[rng.random(n) < 0.05] = np.nan
    ins = rng.integers(-3, 45, n)
    ins[rng.random(n) < 0.2] = -100
    return dict(xyz=xyz, rgb=rgb, sem_gt=rng.integers(-21, 42, n), ins_gt=ins, npcs_gt=rng.uniform(-0.7, 0.7, (n, 3)).astype(np.float32),
                sem_pred=rng.integers(0, 21, n), ins_pred=rng.integers(0, 60, n),
                npcs_pred=rng.uniform(-0.1, 1.1, (n, 3)).astype(np.float32), bbox_pred=np.zeros((0, 8, 3)), bbox_gt=np.zeros((0, 8, 3)),
                trans=np.asarray([2.0, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 1.5]))


def test_non_square_image_ragged_batch_and_an_empty_scene(cuda, gold):
    """1, 37, 0 and 600 points in one batch, H != W, fx != fy: row / column swaps, the CSR walk, clamping outside [0, 256)"""
    rng = np.random.default_rng(5)
    scenes = [_small_scene(rng, n) for n in (1, 37, 0, 600)]
    scenes[0]["xyz"][:] = (0.1, -0.2, 0.3)                   # the single point is visible
    options = tuple(o for o in R.TILE_POS if o != "raw")
    runs = [_render(scenes, cuda, gold["COLOR20"], SMALL_H, SMALL_W, SMALL_EDGE, SMALL_CAM, options).cpu().numpy() for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    for s, scene in enumerate(scenes):
        want = R.assemble(R.render_tiles(scene, gold["COLOR20"], SMALL_H, SMALL_W, SMALL_CAM, options), SMALL_H, SMALL_W, SMALL_EDGE)
        assert np.array_equal(runs[0][s], want), s
    assert (runs[0][2] == 255).all(), "an empty scene is white"
    pc0 = _tile(runs[0][0], "pc", SMALL_H, SMALL_W, SMALL_EDGE)
    assert int((pc0 != 255).any(-1).sum()) in range(1, 5), "one point: one 2 x 2 splat"
    assert len({tuple(c) for c in _tile(runs[0][3], "pc", SMALL_H, SMALL_W, SMALL_EDGE).reshape(-1, 3)}) > 50


# ---------------------------------------------------------------------------------------------------- scene maps
def _torch_maps(vi, si, po, mask, preds, n_rows):
    """model.py:954-971 in torch on the CPU; the one assignment with repeated indices written as the loop it stands for"""
    vi, si, po = torch.as_tensor(vi).long(), torch.as_tensor(si).long(), torch.as_tensor(po).long()
    mask, preds = torch.as_tensor(mask).bool(), torch.as_tensor(preds).float()
    proposal_indices = vi[si]
    ins = torch.zeros(n_rows)
    for p in range(len(po) - 1):
        ins[proposal_indices[po[p]:po[p + 1]]] = p + 1
    npcs = torch.zeros(n_rows, 3)
    for j, row in enumerate(vi[si[torch.where(mask)[0]]].tolist()):
        npcs[row] = preds[j]
    fit = npcs[proposal_indices] - 0.5
    return ins.int().numpy(), npcs.numpy(), fit.numpy()


def _maps_case(rng, n_rows, proposals, masked):
    """proposals: lists of rows of the batch; masked: per proposal point whether it is NPCS-valid"""
    rows = sorted({r for p in proposals for r in p} | set(rng.choice(n_rows, n_rows // 2, replace=False).tolist()))
    vi = np.asarray(rows, dtype=np.int64)
    pos = {r: i for i, r in enumerate(rows)}
    si = np.asarray([pos[r] for p in proposals for r in p], dtype=np.int64)
    po = np.concatenate([[0], np.cumsum([len(p) for p in proposals])]).astype(np.int64)
    mask = np.asarray([m for ms in masked for m in ms], dtype=bool)
    preds = rng.uniform(0, 1, (int(mask.sum()), 3)).astype(np.float32)
    return vi, si, po, mask, preds, n_rows


def _check_maps(cuda, case):
    from gapartnet_amd import hip_ops
    vi, si, po, mask, preds, n_rows = case
    t = lambda a: torch.as_tensor(a).to(cuda)
    got = [hip_ops.scene_maps(t(vi), t(si), t(po), t(mask), t(preds).reshape(-1, 3), n_rows) for _ in range(2)]
    want = _torch_maps(*case)
    for g, g2, w, w2 in zip(got[0], got[1], want, R.scene_maps(*case)):
        assert torch.equal(g, g2)
        assert np.array_equal(g.cpu().numpy(), w) and np.array_equal(w, w2)
    return [g.cpu().numpy() for g in got[0]]


def test_scene_maps_equal_the_torch_formulation(cuda):
    rng = np.random.default_rng(0)
    # a proposal of 9 points and one of 10, partly masked
    nine, ten = list(range(3, 12)), list(range(20, 30))
    ins, _, _ = _check_maps(cuda, _maps_case(rng, 64, [nine, ten], [rng.random(9) < 0.7, rng.random(10) < 0.7]))
    assert (ins == 1).sum() == 9 and (ins == 2).sum() == 10
    # a point shared by two proposals: the higher one wins in both maps; a second shared point whose higher entry is outside
    # the mask keeps the lower proposal's NPCS and the higher proposal's instance id
    a, b = [5, 6, 7, 8, 9, 40], [9, 10, 11, 40, 12]
    ma, mb = [True] * 6, [True, True, False, False, True]
    case = _maps_case(rng, 50, [a, b], [ma, mb])
    ins, npcs, fit = _check_maps(cuda, case)
    preds = case[4]
    assert ins[9] == 2 and np.array_equal(npcs[9], preds[6]), "row 9: proposal 2's prediction (its first masked point)"
    assert ins[40] == 2 and np.array_equal(npcs[40], preds[5]), "row 40: proposal 2 unmasked there, proposal 1's prediction stays"
    assert np.array_equal(fit[4], preds[6] - np.float32(0.5)), "proposal 1 fits row 9 with the winner's NPCS"
    # a proposal without any NPCS-valid point enters the fit as -0.5
    case = _maps_case(rng, 40, [[1, 2, 3, 4, 5], [10, 11, 12, 13, 14, 15]], [[False] * 5, [True] * 6])
    _, npcs, fit = _check_maps(cuda, case)
    assert (fit[:5] == -0.5).all() and not npcs[1:6].any()
    # a few thousand points over several workgroups and scan tiles
    props = [rng.choice(5000, int(k), replace=False).tolist() for k in rng.integers(5, 900, 12)]
    _check_maps(cuda, _maps_case(rng, 5000, props, [rng.random(len(p)) < 0.6 for p in props]))
    # P = 0 with points left over, and M = 0
    vi = np.arange(0, 30, 2)
    ins, npcs, fit = _check_maps(cuda, (vi, np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, bool), np.zeros((0, 3), np.float32), 30))
    assert not ins.any() and not npcs.any() and fit.shape == (0, 3)
    ins, _, _ = _check_maps(cuda, (vi, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 3), np.float32), 30))
    assert ins.shape == (30,) and not ins.any()


@pytest.mark.parametrize("M", [1023, 1024, 1025, 2049])
def test_scene_maps_across_the_rank_scan_tiles(cuda, M):
    """M proposal points, every second one NPCS-valid: the rank of a valid point - its row of npcs_preds - is carried across the
    1024-entry tiles of the one-workgroup scan from M = 1025 on"""
    from gapartnet_amd.inference import scene_maps_torch
    rng = np.random.default_rng(M)
    rows = rng.permutation(M + 50)[:M].tolist()
    valid = (np.arange(M) % 2 == 0).tolist()
    case = _maps_case(rng, M + 50, [rows[:M // 3], rows[M // 3:]], [valid[:M // 3], valid[M // 3:]])
    got = _check_maps(cuda, case)
    for g, w in zip(got, scene_maps_torch(*[torch.as_tensor(a) for a in case[:5]], case[5])):
        assert np.array_equal(g, w.numpy())


# ---------------------------------------------------------------------------------------------------- predictions and boxes
def _part(rng, n, noise=0.002):
    """camera-frame points of a part and their NPCS (a similarity apart, plus noise)"""
    npcs = rng.uniform(-0.45, 0.45, (n, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    xyz = rng.uniform(0.15, 0.3) * npcs @ q + rng.uniform(-0.25, 0.25, 3) + rng.normal(scale=noise, size=(n, 3))
    return xyz.astype(np.float32), npcs.astype(np.float32)


def _sequential_box(xyz, npcs, picks, monkeypatch):
    from gapartnet_amd.misc.pose_fitting import estimate_pose_from_npcs
    it = iter(picks)
    monkeypatch.setattr(np.random, "randint", lambda n, size=None: np.asarray(next(it)))
    bbox, scale = estimate_pose_from_npcs(xyz, npcs)[:2]
    monkeypatch.undo()
    return None if scale[0] is None else np.asarray(bbox, dtype=np.float64)


def test_scene_predictions_boxes_and_their_drawing(cuda, monkeypatch):
    from gapartnet_amd import hip_ops
    from gapartnet_amd.misc import visu
    from gapartnet_amd.misc.pose_fitting_batched import draw_picks
    from gapartnet_amd.structure.instances import Instances
    rng = np.random.default_rng(3)
    sizes = [9, 10, 40, 25, 12]            # 9: no box; the last proposal has no NPCS-valid point: the fit marks it invalid
    n_rows, scene_offsets = 160, [0, 90, 160]
    parts = [_part(rng, n) for n in sizes]
    # proposals 0 - 2 lie in scene 0 (59 points), 3 and 4 in scene 1 (37 points)
    rows = np.concatenate([np.sort(rng.choice(90, 59, replace=False)), 90 + np.sort(rng.choice(70, 37, replace=False))])
    vi = np.sort(np.unique(np.concatenate([rows, rng.choice(n_rows, 20)])))
    si = np.searchsorted(vi, rows)
    po = np.concatenate([[0], np.cumsum(sizes)])
    mask = rng.random(sum(sizes)) < 0.85
    mask[po[4]:] = False
    npcs_all = np.concatenate([p[1] for p in parts])
    preds = (npcs_all[mask] + np.float32(0.5)).astype(np.float32)
    pt_xyz = np.concatenate([p[0] for p in parts])
    np.random.seed(11)
    picks = draw_picks(sizes, 100)
    t = lambda a: torch.as_tensor(a).to(cuda)
    kept = Instances(valid_indices=t(vi), sorted_indices=t(si), proposal_offsets=t(po).int(), npcs_valid_mask=t(mask),
                     npcs_preds=t(preds), pt_xyz=t(pt_xyz), batch_indices=t((rows >= 90).astype(np.int32)))
    pred = visu.scene_predictions(kept, scene_offsets, picks=picks)
    ins_w, npcs_w, fit_w = R.scene_maps(vi, si, po, mask, preds, n_rows)
    assert np.array_equal(pred.ins_map.cpu().numpy(), ins_w) and np.array_equal(pred.npcs_map.cpu().numpy(), npcs_w)
    want = [None if sizes[p] < 10 else _sequential_box(pt_xyz[po[p]:po[p + 1]].astype(np.float64),
                                                      fit_w[po[p]:po[p + 1]].astype(np.float64), picks[p].numpy(), monkeypatch)
            for p in range(len(sizes))]
    have = [p for p, b in enumerate(want) if b is not None]
    assert have == [1, 2, 3] and pred.box_proposal.tolist() == have and pred.box_scene.tolist() == [0, 0, 1]
    bbox = pred.bbox.cpu().numpy()
    assert bbox.dtype == np.float64
    for k, p in enumerate(have):
        assert np.allclose(bbox[k], want[p], rtol=0, atol=1e-8), p
    # drawing: the GPU's own boxes through the numpy rule, pixel for pixel (identical input: no tolerance enters)
    H, W, cam = 96, 128, (150.0, 140.0, 64.5, 47.0)
    trans = np.asarray([[1.0, 0.0, 0.0, 1.2], [1.0, 0.05, -0.05, 1.0]])
    canvas = torch.full((2, H, W, 3), 255, dtype=torch.uint8, device=cuda)
    hip_ops.boxes_draw(pred.bbox, pred.box_scene, t(trans), H, W, *cam, [(0, 0)], canvas, 0)
    again = torch.full((2, H, W, 3), 255, dtype=torch.uint8, device=cuda)
    hip_ops.boxes_draw(pred.bbox, pred.box_scene, t(trans), H, W, *cam, [(0, 0)], again, 0)
    assert torch.equal(canvas, again)
    got = canvas.cpu().numpy()
    for s in range(2):
        white = np.full((H, W, 3), 255, np.uint8)
        want_img = R.draw_boxes(white, bbox[pred.box_scene.cpu().numpy() == s], trans[s], cam)
        assert (want_img != 255).any() and np.array_equal(got[s], want_img), s


def test_a_later_box_is_drawn_over_an_earlier_one(cuda):
    """two crossing boxes in one scene, a third scene-less one, edges that leave the tile and a box behind the camera"""
    from gapartnet_amd import hip_ops
    H, W, cam = 96, 128, (150.0, 140.0, 64.5, 47.0)
    signs = np.asarray([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [1, 1, 1]], float)
    boxes = np.stack([signs * 0.2 + (0.0, 0.0, 1.5), signs * (0.25, 0.1, 0.2) + (-0.1, -0.1, 1.6), signs * 0.6 + (0.5, 0.3, 1.4),
                      signs * 0.2 + (0.0, 0.0, -1.0), signs * 0.2 + (0.0, 0.0, 0.2)])
    trans = np.asarray([[1.0, 0.0, 0.0, 0.0]])
    t = lambda a: torch.as_tensor(a).to(cuda)
    canvas = torch.full((1, H + 8, 2 * (W + 4) + 4, 3), 255, dtype=torch.uint8, device=cuda)
    hip_ops.boxes_draw(t(boxes), t(np.zeros(5, np.int32)), t(trans), H, W, *cam, [(0, 0), (0, 1)], canvas, 4)
    got = canvas.cpu().numpy()[0]
    white = np.full((H, W, 3), 255, np.uint8)
    want = R.draw_boxes(white.copy(), boxes, trans[0], cam)
    assert np.array_equal(got[4:4 + H, 4:4 + W], want) and np.array_equal(got[4:4 + H, W + 8:2 * W + 8], want)
    assert (got[:4] == 255).all() and (got[:, W + 4:W + 8] == 255).all(), "nothing outside the tiles"
    first, second = R.draw_boxes(white.copy(), boxes[:1], trans[0], cam), R.draw_boxes(white.copy(), boxes[1:2], trans[0], cam)
    axis = (first != 255).any(-1) & ~(first == (255, 0, 255)).all(-1)           # the first box's axes ...
    over = axis & (second == (255, 0, 255)).all(-1)                             # ... where the second box's edges cross them
    canvas.fill_(255)
    hip_ops.boxes_draw(t(boxes[:2]), t(np.zeros(2, np.int32)), t(trans), H, W, *cam, [(0, 0)], canvas, 4)
    two = canvas.cpu().numpy()[0][4:4 + H, 4:4 + W]
    assert np.array_equal(two, R.draw_boxes(white.copy(), boxes[:2], trans[0], cam))
    assert over.any() and (two[over] == (255, 0, 255)).all(), "the later box wins, whatever the colour"
    # a box whose scene is out of range is not drawn
    canvas.fill_(255)
    hip_ops.boxes_draw(t(boxes[:1]), t(np.asarray([3], np.int32)), t(trans), H, W, *cam, [(0, 0)], canvas, 4)
    assert bool((canvas == 255).all())


# ---------------------------------------------------------------------------------------------------- end to end
def test_trainer_test_writes_the_panels_and_keeps_the_metrics(cuda, tmp_path):
    from PIL import Image
    from gapartnet_amd.dataset.gapartnet import GAPartNetInst
    from gapartnet_amd.misc import visu
    from gapartnet_amd.smoke import make_model
    from gapartnet_amd.trainer import Trainer
    from tests.golden import recipe
    n_points, root, out = 2000, str(tmp_path / "data"), str(tmp_path / "visu")
    scenes = {}
    for split, seed0 in (("val", 5000), ("test_intra", 6000), ("test_inter", 7000)):
        os.makedirs(os.path.join(root, split, "pth"))
        os.makedirs(os.path.join(root, split, "meta"))
        for i in range(2):
            name = f"StorageFurniture_{seed0 + i:05d}_00_{i:03d}"
            arrays = recipe.scene_arrays(seed0 + i, n_points)
            torch.save(tuple(arrays), os.path.join(root, split, "pth", name + ".pth"))
            trans = np.asarray([0.5, 0.01 * i, -0.02, 1.8])
            np.savetxt(os.path.join(root, split, "meta", name + ".txt"), trans)
            scenes[(split, name)] = dict(xyz=np.asarray(arrays[0], np.float32), rgb=np.asarray(arrays[1], np.float32),
                                         sem_gt=np.asarray(arrays[2]), ins_gt=np.asarray(arrays[3]),
                                         npcs_gt=np.asarray(arrays[4], np.float32), trans=trans)
    model = make_model((0, 0))           # start_scorenet = 0
    model.load_state_dict(recipe.name_keyed_state(model))
    model.revoxelize_jitter = (torch.tensor([0.3, 0.6, 0.1], device=cuda), torch.tensor([0.5, 0.2, 0.9], device=cuda))
    trainer = Trainer(max_epochs=1, accelerator="gpu", enable_checkpointing=False, default_root_dir=str(tmp_path), seed=11)
    dm = GAPartNetInst(root, max_points=n_points, val_batch_size=2, test_batch_size=2, num_workers=0)
    dm.setup("validate")
    plain = trainer.test(model, datamodule=dm)
    assert not os.path.exists(out)
    model.visualize_cfg = dict(visualize=True, SAVE_ROOT=out, GAPARTNET_DATA_ROOT=root, RAW_IMG_ROOT=str(tmp_path / "raw"),
                               save_option=list(visu.OPTIONS), sample_num=0)
    drawn = trainer.test(model, datamodule=dm)
    assert set(plain) == set(drawn) and len(plain) > 5
    for k in plain:
        assert plain[k] == drawn[k] or (np.isnan(plain[k]) and np.isnan(drawn[k])), k
    H, W, EDGE = visu.HEIGHT, visu.WIDTH, visu.EDGE
    palette = visu.default_palette()
    colours = {tuple(c) for c in palette[:20]} | {(255, 255, 255)}
    for (split, name), scene in scenes.items():
        img = np.asarray(Image.open(os.path.join(out, split, name + ".png")).convert("RGB"))
        assert img.shape == R.canvas_shape(H, W, EDGE) + (3,)
        want = R.render_tiles(scene, palette, H, W, options=("pc", "sem_gt", "ins_gt", "npcs_gt"))
        for tile, ref in want.items():
            assert (ref != 255).any() and np.array_equal(_tile(img, tile, H, W, EDGE), ref), (split, name, tile)
        ins_pred = _tile(img, "ins_pred", H, W, EDGE)
        assert {tuple(c) for c in np.unique(ins_pred.reshape(-1, 3), axis=0)} <= colours
        assert np.array_equal((ins_pred != 255).any(-1), R.points_winner(scene["xyz"], scene["trans"], H, W) >= 0)
        assert (_tile(img, "raw", H, W, EDGE) == 255).all(), "no raw file: the tile stays empty"
