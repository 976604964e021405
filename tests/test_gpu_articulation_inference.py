"""``articulation_from_frames`` on the GPU with the synthetic weights of the other inference tests: it equals
``articulation_from_maps`` fed with the two predictions' own maps, it runs with no predicted part at all, and the command line with
``--ckpt`` writes its files.  3 frame pairs of 96 x 128 (one of them empty), 2048 points.  Synthetic weights say nothing about the
quality of the matches on real data: these tests hold the plumbing."""
import random

import numpy as np
import pytest
import torch

from gapartnet_amd.misc import articulation as AR
from tests import frame_ref as F
from tests import inference_ref as R
from tests import pipeline_runner as PR

pytestmark = pytest.mark.gpu
H, W, M, PRE = 96, 128, 2048, 2
RANSAC, SAMPLES = 32, 64


def _model(cuda):
    model = PR.build_model(cuda).eval()
    model.inference_dtype = None
    model.revoxelize_jitter = tuple(torch.tensor(j, device=cuda) for j in ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9]))
    return model


def _picks(sizes):
    return R.size_picks(sizes, RANSAC)


@pytest.fixture(scope="module")
def frames():
    """the synthetic scenes seen by a camera in front of a wall (as the frame-inference tests build them), each against itself - the
    two predictions of a pair are then one prediction twice, whatever the weights - with an empty pair between them"""
    a, c = (x.numpy()[:-8] for x in R.raw_clouds(20000))
    depth, rgb, K = F.frames_from_clouds([a, c], H, W)
    wall = np.zeros((H, W), bool)
    wall[8:-8, 10:-10] = True
    for v in range(2):
        depth[v][(depth[v] == 0) & wall] = depth[v].max() + np.float32(0.25)
    z, zc = np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.uint8)
    da, ca = np.stack([depth[0], z, depth[1]]), np.stack([rgb[0], zc, rgb[1]])
    return da, ca, da.copy(), ca.copy(), K[0]


def _eq(a, b):
    return torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0))


def test_articulation_from_frames_equals_articulation_from_maps_on_its_own_predictions(cuda, frames):
    from gapartnet_amd import inference
    da, ca, db, cb, K = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    predictor = inference.PartPredictor(_model(cuda), num_points=M, max_iters=RANSAC)
    random.seed(5)
    np.random.seed(5)
    fa, fb, got = AR.articulation_from_frames(predictor, t(da), t(ca), t(db), t(cb), K, presample=PRE, seed=3, frame_picks=_picks, flip=True,
                                              sample_number=SAMPLES)
    assert [p.status for p in fa] == [R.OK, R.EMPTY, R.OK] and len(fb) == 3
    random.seed(5)
    np.random.seed(5)
    want = AR.articulation_from_maps(t(da), t(db), K, torch.stack([p.instance for p in fa]), torch.stack([p.instance for p in fb]),
                                     [p.proposal_classes for p in fa], [p.proposal_classes for p in fb], flip=True, sample_number=SAMPLES)
    G = len(got.joint_type)
    print(f"{[int(p.proposal_classes.shape[0]) for p in fa]} and {[int(p.proposal_classes.shape[0]) for p in fb]} parts, {G} matched pairs: "
          f"{got.joint_type}")
    assert G > 0 and 0 in got.frame and 1 not in got.frame, "identical frames match, the empty pair has nothing"
    for f in ("frame", "part_a", "part_b", "part_class", "iou2d", "n_points_a", "n_points_b"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert got.joint_type == want.joint_type and _eq(got.iterations, want.iterations) and _eq(got.norm, want.norm)
    for leg in ("cpd", "ransac"):
        for f in ("axis", "pivot", "angle", "scale", "rotation", "translation"):
            assert _eq(getattr(getattr(got, leg), f), getattr(getattr(want, leg), f)), (leg, f)
    # pair 0 is one frame twice: every part is matched to itself with IoU 1
    n0 = int(fa[0].proposal_classes.shape[0])
    first = got.frame == 0
    covered = [p for p in range(n0) if bool((fa[0].instance == p).any())]
    assert got.part_a[first].tolist() == covered and got.part_b[first].tolist() == covered and (got.iou2d[first] == 1.0).all()
    assert got.cpd.axis.shape == (G, 3) and got.cpd.axis.is_cuda
    img = AR.draw_articulation(ca[0], K, got, 0)
    assert img.shape == (H, W, 3)


def test_sampler_and_isolate_are_passed_through(cuda, frames):
    """``sampler="grid"`` on an FPS predictor and an ``IsolateConfig``: the predictions are those of a grid predictor's
    ``predict_frames(isolate=...)``, and the articulation is that of their maps"""
    from gapartnet_amd import inference
    da, ca, db, cb, K = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    model = _model(cuda)
    cfg = inference.IsolateConfig()
    fps = inference.PartPredictor(model, num_points=M, max_iters=RANSAC)
    grid = inference.PartPredictor(model, num_points=M, max_iters=RANSAC, sampler="grid")
    random.seed(6)
    np.random.seed(6)
    fa, fb, got = AR.articulation_from_frames(fps, t(da), t(ca), t(db), t(cb), K, presample=PRE, seed=3, isolate=cfg, sampler="grid",
                                              frame_picks=_picks, flip=True, sample_number=SAMPLES)
    assert fps.sampler == "fps", "the caller's predictor is left as it is"
    want_a = grid.predict_frames(t(da), t(ca), K, picks=_picks, presample=PRE, seed=3, flip=True, isolate=cfg)
    plain_a = fps.predict_frames(t(da), t(ca), K, picks=_picks, presample=PRE, seed=3, flip=True)
    for p, q in zip(fa, want_a):
        assert p.keep is not None and p.isolate_status == q.isolate_status and torch.equal(p.keep, q.keep)
        for f in ("sem", "instance", "sample_rows", "proposal_classes"):
            assert torch.equal(getattr(p, f), getattr(q, f)), f
    assert not torch.equal(fa[0].sample_rows, plain_a[0].sample_rows), "another sampler and a cut frame sample other pixels"
    random.seed(6)
    np.random.seed(6)
    want = AR.articulation_from_maps(t(da), t(db), K, torch.stack([p.instance for p in fa]), torch.stack([p.instance for p in fb]),
                                     [p.proposal_classes for p in fa], [p.proposal_classes for p in fb], flip=True, sample_number=SAMPLES)
    for f in ("frame", "part_a", "part_b", "part_class", "iou2d", "n_points_a", "n_points_b"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert _eq(got.cpd.axis, want.cpd.axis) and _eq(got.cpd.angle, want.cpd.angle)


def test_no_predicted_part_gives_an_empty_articulation(cuda):
    from gapartnet_amd import inference
    predictor = inference.PartPredictor(_model(cuda), num_points=M, max_iters=RANSAC)
    d = torch.zeros((1, H, W), dtype=torch.float32, device=cuda)
    c = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=cuda)
    K = np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]])
    fa, fb, art = AR.articulation_from_frames(predictor, d, c, d, c, K, presample=PRE, frame_picks=_picks)
    assert fa[0].status == R.EMPTY and art.frame.shape == (0,) and art.joint_type == [] and art.cpd.axis.shape == (0, 3)
    assert art.matches.pairs[0].shape == (0, 2) and art.matches.area_a[0].shape == (0,) and art.iterations.shape == (0,)


def test_command_line_with_a_checkpoint_end_to_end(cuda, frames, tmp_path):
    from PIL import Image
    da, ca, db, cb, K = frames
    model = _model(cuda)
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": model.state_dict(), "hyper_parameters": dict(model.hparams)}, ckpt)
    np.save(tmp_path / "a.npy", da[0] * np.float32(1000))
    np.save(tmp_path / "b.npy", db[0] * np.float32(1000))
    Image.fromarray(ca[0]).save(tmp_path / "a_rgb.png")
    Image.fromarray(cb[0]).save(tmp_path / "b_rgb.png")
    np.savetxt(tmp_path / "K.txt", K)
    p = lambda *names: [str(tmp_path / n) for n in names]  # noqa: E731
    out = tmp_path / "out"
    assert AR.main(["--ckpt", str(ckpt), "--depth", *p("a.npy", "b.npy"), "--rgb", *p("a_rgb.png", "b_rgb.png"), "--intrinsics",
                    str(tmp_path / "K.txt"), "--out", str(out), "--depth_scale", "1000", "--flip", "--presample", str(PRE), "--seed", "3",
                    "--num_points", str(M), "--sample_number", str(SAMPLES), "--device", "cuda:0"]) == 0
    got = np.load(out / "a_articulation.npz")
    for f in ("frame", "part_a", "part_b", "part_class", "joint_type", "iou2d", "cpd_axis", "cpd_pivot", "cpd_angle", "ransac_axis",
              "cpd_rotation", "iterations", "norm"):
        assert f in got.files, f
    G = len(got["joint_type"])   # (a loaded checkpoint draws its re-voxelisation jitter: the two predictions need not be equal)
    print(f"{G} matched pairs, IoU {got['iou2d'].tolist()}")
    assert got["cpd_axis"].shape == (G, 3) and got["frame"].shape == (G,) and got["norm"].shape == (G, 4)
    assert set(got["joint_type"].tolist()) <= {"revolute", "prismatic", "fixed"}
    assert np.asarray(Image.open(out / "a_articulation.png")).shape == (H, W, 3)
