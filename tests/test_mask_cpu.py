"""Parts from caller-supplied masks without a GPU: the CPU path of ``GAPartNet.forward_with_masks`` / ``estimate_pose_from_mask``
over the oracle operators against the restatement of tests/mask_ref.py, the ``PointCloud`` fields, the conventions of
``PartPredictor.predict_with_masks``, the command line, and the new symbols of the library."""
import os
import re

import numpy as np
import pytest
import torch

from gapartnet_amd import backend, inference
from gapartnet_amd.structure.point_cloud import PointCloud
from tests import inference_ref as R
from tests import mask_ref as MR
from tests import pipeline_runner as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])


@pytest.fixture(scope="module")
def oracle_model():
    from oracle import torch_ops
    with backend.using(torch_ops):
        model = PR.build_model(torch.device("cpu")).eval()
        model.revoxelize_jitter = tuple(torch.tensor(j) for j in JITTER)
        yield model


def _masks_for(scenes, n_masks=5):
    masks, labels = [], []
    for s, pc in enumerate(scenes):
        n = pc.points.shape[0]
        few = np.zeros(n, bool)
        few[[3, 40, 41, 500]] = True          # below min_points: dropped
        m = MR.scene_masks(pc.points, n_masks, seed=70 + s, extra=(np.zeros(n, bool), np.ones(n, bool), few))
        m[1] = m[0]                            # two identical masks
        masks.append(torch.from_numpy(m))
        labels.append(torch.from_numpy(np.random.RandomState(s).randint(1, 10, size=m.shape[0])))
    return masks, labels


def test_forward_with_masks_over_the_oracle_equals_the_restatement(oracle_model):
    model = oracle_model
    scenes = PR.load_scenes(torch.device("cpu"))
    masks, labels = _masks_for(scenes)
    plan_before = (model._prop_plan, list(model._prop_hist))
    got = model.forward_with_masks(R.unlabelled(scenes), masks, labels)
    assert (model._prop_plan, list(model._prop_hist)) == plan_before and model.sync_free_proposals is True
    assert got[0] == [pc.pc_id for pc in scenes] and got[2] is not None
    want = MR.forward_with_masks_formulation(model, R.unlabelled(scenes), masks, labels, model.min_num_points_per_proposal)
    MR.check_forward_with_masks(got, want)
    K0 = masks[0].shape[0]
    kept = got[2].proposal_mask.tolist()
    assert K0 - 3 not in kept and K0 - 1 not in kept and K0 - 2 in kept, "empty and 4-point masks dropped, the full mask kept"
    # the semantic predictions are the network's own: those of model(pcs)
    assert torch.equal(got[1].sem_preds, model(R.unlabelled(scenes))[1].sem_preds)
    # labels the clouds carry are not read; u8 masks; a cloud without masks; gradients requested by the caller
    with torch.enable_grad():
        again = model.forward_with_masks(scenes, [masks[0].to(torch.uint8) * 7, None], [labels[0], None])
    one = MR.forward_with_masks_formulation(model, R.unlabelled(scenes), [masks[0], None], [labels[0], []], model.min_num_points_per_proposal)
    MR.check_forward_with_masks(again, one)
    assert not again[2].score_preds.requires_grad and int(again[2].batch_indices.max()) == 0
    # no mask at all, every mask dropped, a label outside the classes
    none = model.forward_with_masks(R.unlabelled(scenes), [None, None], [None, None])
    assert none[2] is None and none[3].shape == (0,) and torch.equal(none[1].sem_preds, got[1].sem_preds)
    none = model.forward_with_masks(R.unlabelled(scenes), [masks[0][-1:], masks[1][-3:-2]], [labels[0][-1:], labels[1][-3:-2]])
    assert none[2] is None
    for bad in (0, model.num_part_classes):
        with pytest.raises(RuntimeError, match="label"):
            model.forward_with_masks(R.unlabelled(scenes), [masks[0][:1], None], [torch.tensor([bad]), None])
    with pytest.raises(ValueError):
        model.forward_with_masks(R.unlabelled(scenes), [masks[0][:, :-1], None], [labels[0], None])


def test_estimate_pose_from_mask_reads_the_point_cloud_fields(oracle_model):
    model = oracle_model
    scenes = R.unlabelled(PR.load_scenes(torch.device("cpu")))
    masks, labels = _masks_for(scenes)
    want = model.forward_with_masks(scenes, masks, labels)
    scenes[0].pc_masks, scenes[0].mask_labels, scenes[0].mask_ids = [m.numpy() for m in masks[0]], labels[0].numpy(), \
        [f"part{k}" for k in range(masks[0].shape[0])]
    scenes[1].pc_masks, scenes[1].mask_labels = masks[1], labels[1]
    scenes = [pc.to_tensor() for pc in scenes]
    assert torch.equal(scenes[0].pc_masks, masks[0]) and torch.equal(scenes[0].mask_labels, labels[0])
    ids, props = model.estimate_pose_from_mask(scenes)
    assert ids == want[0]
    for f in MR.TABLES + ("score_preds", "npcs_preds"):
        assert torch.equal(getattr(props, f), getattr(want[2], f)), f
    K0 = masks[0].shape[0]
    assert props.mask_ids == [f"part{k}" if k < K0 else k - K0 for k in props.proposal_mask.tolist()]


def test_point_cloud_mask_fields_round_trip():
    pc = PointCloud(pc_id="x", points=np.zeros((4, 6), np.float32))
    assert pc.pc_masks is None and pc.mask_labels is None and pc.mask_ids is None
    assert pc.to_tensor().pc_masks is None
    pc = PointCloud(pc_id="x", points=np.zeros((4, 6), np.float32), pc_masks=[np.array([1, 0, 0, 1], bool), np.array([0, 0, 1, 1], bool)],
                    mask_labels=np.array([3, 4]), mask_ids=["a", "b"])
    t = pc.to_tensor()
    assert torch.is_tensor(t.pc_masks) and t.pc_masks.shape == (2, 4) and t.pc_masks.dtype == torch.bool
    assert torch.equal(t.mask_labels, torch.tensor([3, 4])) and t.mask_ids == ["a", "b"]
    moved = t.to("cpu")
    assert torch.equal(moved.pc_masks, t.pc_masks) and torch.equal(moved.mask_labels, t.mask_labels) and moved.mask_ids == ["a", "b"]
    batch = PointCloud.collate([PointCloud(pc_id="x", points=torch.rand(50, 6), pc_masks=torch.ones(1, 50, dtype=torch.bool),
                                           mask_labels=torch.tensor([1]))], voxel_size=(0.01,) * 3, voxels=False)
    assert batch.points.shape == (50, 6) and not hasattr(batch, "pc_masks")


def _raw_case():
    a, c = R.raw_clouds()
    a = a.clone()
    a[[3, 700], [0, 2]] = float("nan")
    b = torch.full((40, 6), float("nan"))  # no valid row: not OK, in the middle of the batch
    clouds = [a, b, c]
    masks, labels = [], []
    for s, cloud in enumerate(clouds):
        n = cloud.shape[0]
        if s == 1:
            masks.append(torch.ones((2, n), dtype=torch.bool))
            labels.append(torch.tensor([2, 5]))
            continue
        on_nan = np.zeros(n, bool)
        on_nan[[3, 700]] = True                 # only on rows that are never sampled
        m = MR.scene_masks(cloud, 4, seed=5 + s, extra=(on_nan, np.zeros(n, bool)))
        masks.append(torch.from_numpy(m))
        labels.append(torch.from_numpy(np.random.RandomState(9 + s).randint(1, 10, size=m.shape[0])))
    return clouds, masks, labels


def test_predict_with_masks_conventions_on_cpu_tensors(oracle_model):
    clouds, masks, labels = _raw_case()
    predictor = inference.PartPredictor(oracle_model, num_points=1024, max_iters=16)
    picks = lambda sizes: R.size_picks(sizes, 16)  # noqa: E731
    preds = predictor.predict_with_masks(clouds, masks, labels, picks=picks)
    assert [p.status for p in preds] == [R.OK, R.EMPTY, R.OK]
    n_boxes = MR.check_predictions(preds, predictor, clouds, masks, labels, picks, 6)
    assert n_boxes > 0, "the synthetic clouds' masks give boxes"
    assert not bool(preds[1].kept.any()) and preds[1].kept.shape == (2,)
    for s in (0, 2):
        assert not bool(preds[s].kept[-1]) and not bool(preds[s].kept[-2]) and bool(preds[s].kept[:4].any())
    assert bool((preds[0].sem[[3, 700]] == -1).all())
    # the semantic map is predict's
    plain = predictor.predict(clouds, picks=R.size_picks)
    for p, q in zip(preds, plain):
        assert torch.equal(p.sem, q.sem)
    with pytest.raises(ValueError):
        predictor.predict_with_masks(clouds, masks[:2], labels[:2])


def test_command_line_writes_the_mask_arrays(oracle_model, tmp_path):
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": oracle_model.state_dict(), "hyper_parameters": dict(oracle_model.hparams)}, ckpt)
    clouds, masks, labels = _raw_case()
    paths, mask_paths = [], []
    for name, s in (("first", 0), ("second", 2)):
        paths.append(str(tmp_path / f"{name}.npy"))
        np.save(paths[-1], clouds[s].numpy())
        mask_paths.append(str(tmp_path / f"{name}_masks.npz"))
        np.savez(mask_paths[-1], masks=masks[s].numpy(), labels=labels[s].numpy())
    out = tmp_path / "out"
    rc = inference.main(["--ckpt", str(ckpt), "--input", *paths, "--masks", *mask_paths, "--out", str(out), "--num_points", "512",
                         "--device", "cpu"])
    assert rc == 0
    for name, s in (("first", 0), ("second", 2)):
        got = np.load(out / f"{name}.npz")
        K = masks[s].shape[0]
        for f in ("sem", "instance", "bbox", "status") + tuple("mask_" + f for f in inference.MASK_FIELDS):
            assert f in got.files, f
        assert got["mask_kept"].shape == (K,) and got["mask_bbox"].shape == (K, 8, 3) and got["mask_transform"].shape == (K, 4, 4)
        assert np.array_equal(got["mask_label"], labels[s].numpy()) and got["mask_member_offsets"].shape == (K + 1,)
        assert got["mask_member_rows"].shape[0] == got["mask_member_offsets"][-1] == got["mask_n_points"].sum()
        assert got["mask_kept"].any() and not got["mask_kept"][-1]
    with pytest.raises(SystemExit):
        inference.main(["--ckpt", str(ckpt), "--input", *paths, "--masks", mask_paths[0], "--out", str(out), "--device", "cpu"])


def test_new_symbols_are_declared_and_listed():
    from gapartnet_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpn_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_C.SO_PATH):
        _C.build()
    lib = _C.lib()
    listed = {lib.gpn_entry_point_name(i).decode() for i in range(lib.gpn_num_entry_points())}
    for name in ("gpn_mask_pack", "gpn_proposals_from_masks", "gpn_proposals_from_masks_ws_bytes"):
        assert name in declared and name in listed and hasattr(lib, name), name
    # argument checks that need no device
    assert lib.gpn_mask_pack(None, None, None, None, None, _C.i64(-1), _C.i64(1), None, None) != 0
    assert lib.gpn_mask_pack(None, None, None, None, None, _C.i64(0), _C.i64(4), None, None) == 0
    assert lib.gpn_proposals_from_masks_ws_bytes(_C.i64(16), _C.i64(2), _C.i64(32), _C.i64(4096)) > 0
