"""Multi-view fusion end to end on the GPU (gapartnet_amd/misc/multiview.py, include/gpn.h section MV): ``fuse_frames`` against
``fuse_parts`` on the outputs of ``predict_frames``, the GPU path against the CPU path on the same maps, the fused boxes against
``estimate_pose_from_npcs_batched`` on the reference's clouds, and the identity scene.  The network carries SYNTHETIC weights: its
parts mean nothing, so these tests check the plumbing - which pixels, which order, which frame - and not the quality of a fusion.
4 views of 96 x 128 (one of them empty, one seen twice from one pose so that parts do fuse), 2048 points."""
import numpy as np
import pytest
import torch

from tests import frame_ref as F
from tests import inference_ref as R
from tests import multiview_ref as REF
from tests import multiview_scenes as SC
from tests import pipeline_runner as PR

pytestmark = pytest.mark.gpu
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])
H, W, M, PRE = 96, 128, 2048, 2
SEEDS = [3, 4, 5, 3]
RANSAC = 32
KW = dict(cell=0.05, min_inter=2, min_overlap=0.2)
EXACT = ("fused_inst", "part_class", "score", "n_views", "parts", "n_points", "vol", "links", "dropped", "member_offsets", "member_src",
         "member_xyz", "member_npcs")
BOXES = ("valid", "bbox", "scale", "rotation", "translation")


def _picks(sizes):
    return R.size_picks(sizes, RANSAC)


@pytest.fixture(scope="module")
def views():
    """two synthetic scenes in front of a wall, an empty frame between them, and the first scene once more from its own pose"""
    a, c = (x.numpy()[:-8] for x in R.raw_clouds(20000))
    depth, rgb, K = F.frames_from_clouds([a, c], H, W)
    wall = np.zeros((H, W), bool)
    wall[8:-8, 10:-10] = True
    for v in range(2):
        depth[v][(depth[v] == 0) & wall] = depth[v].max() + np.float32(0.25)
    order = [0, None, 1, 0]
    pick = lambda x, zero: np.stack([zero if v is None else x[v] for v in order])  # noqa: E731
    rng = np.random.RandomState(2)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Rv = np.stack([np.eye(3), np.eye(3), q, np.eye(3)])
    tv = np.stack([np.zeros(3), np.zeros(3), rng.uniform(-0.1, 0.1, 3), np.zeros(3)])
    return (pick(depth, np.zeros((H, W), np.float32)), pick(rgb, np.zeros((H, W, 3), np.uint8)), pick(K, K[0]), Rv, tv)


@pytest.fixture(scope="module")
def fused(cuda, views):
    from gapartnet_amd import inference
    from gapartnet_amd.misc import multiview as MV
    depth, rgb, K, Rv, tv = views
    model = PR.build_model(cuda).eval()
    model.inference_dtype = None
    model.revoxelize_jitter = tuple(torch.tensor(j, device=cuda) for j in JITTER)
    predictor = inference.PartPredictor(model, num_points=M, max_iters=RANSAC)
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    frames, out = MV.fuse_frames(predictor, t(depth), t(rgb), K, Rv, tv, presample=PRE, seed=SEEDS, frame_picks=_picks, picks=_picks, **KW)
    return predictor, frames, out


def _assert_same(a, b, fields):
    a, b = a.to_numpy(), b.to_numpy()
    for f in fields:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)  # (NaN equals NaN here)


def test_fuse_frames_equals_fuse_parts_on_the_frame_predictions(cuda, views, fused):
    from gapartnet_amd.misc import multiview as MV
    depth, rgb, K, Rv, tv = views
    predictor, frames, out = fused
    assert [f.status for f in frames] == [R.OK, R.EMPTY, R.OK, R.OK]
    again = predictor.predict_frames(torch.from_numpy(depth).to(cuda), torch.from_numpy(rgb).to(cuda), K, picks=_picks, presample=PRE,
                                     seed=SEEDS)
    for p, q in zip(frames, again):
        assert torch.equal(p.instance, q.instance) and torch.equal(p.npcs, q.npcs)
    want = MV.fuse_parts(torch.from_numpy(depth).to(cuda), K, torch.stack([f.instance for f in again]), [f.proposal_classes for f in again],
                         Rv, tv, npcs=torch.stack([f.npcs for f in again]), scores=[f.proposal_scores for f in again], picks=_picks, **KW)
    _assert_same(out, want, EXACT + BOXES)
    n = [int(f.proposal_classes.shape[0]) for f in frames]
    assert n[1] == 0 and n[0] > 0 and n[3] > 0, "the views carry parts"
    F_ = out.part_class.shape[0]
    assert 0 < F_ < sum(n), "the view seen twice fuses with itself"
    assert out.parts.shape == (F_, 4) and (out.parts[:, 1] == -1).all()
    assert ((out.parts[:, 0] >= 0) & (out.parts[:, 3] >= 0)).any()
    assert out.fused_inst.is_cuda and out.bbox.is_cuda and out.fused_inst.shape == (4, H, W)


def test_gpu_path_equals_cpu_path_on_the_same_maps(cuda, views, fused):
    from gapartnet_amd.misc import multiview as MV
    depth, rgb, K, Rv, tv = views
    _, frames, out = fused
    cpu = MV.fuse_parts(torch.from_numpy(depth), K, torch.stack([f.instance.cpu() for f in frames]), [f.proposal_classes.cpu() for f in frames],
                        Rv, tv, npcs=torch.stack([f.npcs.cpu() for f in frames]), scores=[f.proposal_scores.cpu() for f in frames],
                        picks=_picks, **KW)
    _assert_same(out, cpu, EXACT)


def test_fused_boxes_equal_the_batched_fit_on_the_reference_clouds(cuda, views, fused):
    from gapartnet_amd import inference
    from gapartnet_amd.misc import multiview as MV
    from gapartnet_amd.misc.pose_fitting_batched import estimate_pose_from_npcs_batched
    depth, rgb, K, Rv, tv = views
    _, frames, out = fused
    V = depth.shape[0]
    rows, valid = inference._backproject_numpy(depth, np.zeros((V, H, W, 3), np.uint8), K, None, 1.0, False)
    cls = np.concatenate([f.proposal_classes.cpu().numpy() for f in frames])
    ref = REF.fuse(rows, valid.reshape(V, H, W), np.stack([f.instance.cpu().numpy() for f in frames]),
                   [int(f.proposal_classes.shape[0]) for f in frames], cls, Rv, tv, KW["cell"], KW["min_inter"], KW["min_overlap"],
                   npcs=np.stack([f.npcs.cpu().numpy() for f in frames]), fast=True)
    np.testing.assert_array_equal(out.member_xyz.cpu().numpy(), ref["xyz"])
    np.testing.assert_array_equal(out.member_npcs.cpu().numpy(), ref["npcs"])
    xyz, npcs = torch.from_numpy(ref["xyz"]).to(cuda), torch.from_numpy(ref["npcs"]).to(cuda)
    r, c = MV.ball_frame(xyz)
    fit = estimate_pose_from_npcs_batched((xyz - c) / r, npcs - 0.5, torch.from_numpy(ref["offsets"]).to(cuda),
                                          picks=_picks(ref["n_points"].tolist()), max_iters=RANSAC)
    ok = fit["valid"] & torch.from_numpy(ref["n_points"] >= 5).to(cuda)
    assert torch.equal(out.valid, ok) and bool(ok.any()), "some fused part has a box"
    assert torch.equal(out.bbox[ok], (fit["bbox"] * r + c)[ok]) and bool(torch.isnan(out.bbox[~ok]).all())
    assert torch.equal(out.scale[ok], (fit["scale"] * r)[ok]) and torch.equal(out.rotation[ok], fit["rotation"][ok])
    assert torch.equal(out.translation[ok], (fit["translation"] * r + c)[ok])
    # the overlay of one view: the boxes in its camera frame
    img = MV.draw_fused(rgb[2], K[2], Rv[2], tv[2], out, 0)
    assert img.shape == (H, W, 3) and img.dtype == np.uint8


def _sync_count(fn):
    """the synchronising torch calls fn() makes, as torch's sync debug mode reports them"""
    import warnings
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def test_fuse_parts_reads_the_host_once(cuda):
    """without ``npcs`` the call makes ONE synchronising call, the read of the small tables; with it, that one and the fit's own"""
    from gapartnet_amd.misc import multiview as MV
    from gapartnet_amd.misc.pose_fitting_batched import estimate_pose_from_npcs_batched
    sc = SC.identity_scene()
    d, inst, npcs = (torch.from_numpy(sc[k]).to(cuda) for k in ("depth", "inst", "npcs"))
    scores = [np.linspace(0.1, 0.9, len(c)).astype(np.float32) for c in sc["classes"]]
    kw = dict(cell=0.02, min_inter=4, min_overlap=0.25, scores=scores)
    plain = lambda: MV.fuse_parts(d, sc["K"], inst, sc["classes"], sc["R"], sc["t"], **kw)  # noqa: E731
    out = plain()  # (warm-up: first calls build caches)
    assert _sync_count(plain) == 1
    assert out.score.tolist() == pytest.approx([max(float(scores[v][p]) for v, p in enumerate(row) if p >= 0) for row in out.parts])
    picks = _picks(out.n_points.tolist()).to(cuda)
    boxed = lambda: MV.fuse_parts(d, sc["K"], inst, sc["classes"], sc["R"], sc["t"], npcs=npcs, picks=picks, **kw)  # noqa: E731
    got = boxed()
    offsets = torch.from_numpy(got.member_offsets).to(cuda)
    fit = lambda: estimate_pose_from_npcs_batched(got.member_xyz, got.member_npcs - 0.5, offsets, picks=picks, max_iters=RANSAC)  # noqa: E731
    fit()
    assert _sync_count(boxed) == 1 + _sync_count(fit)


@pytest.mark.parametrize("min_overlap", [0.1, 0.25, 0.5])
def test_identity_scene_fuses_to_the_boxes_on_the_gpu(cuda, min_overlap):
    from gapartnet_amd.misc import multiview as MV
    sc = SC.identity_scene()
    kw = dict(cell=0.02, min_inter=4, min_overlap=min_overlap)
    args = lambda dev: (torch.from_numpy(sc["depth"]).to(dev), sc["K"], torch.from_numpy(sc["inst"]).to(dev), sc["classes"], sc["R"],  # noqa: E731
                        sc["t"])
    gpu = MV.fuse_parts(*args(cuda), npcs=torch.from_numpy(sc["npcs"]).to(cuda), picks=_picks, **kw)
    ident = SC.fused_identity(sc, gpu.parts)
    assert len(ident) == 5 and all(len(s) == 1 for s in ident) and set.union(*ident) == set(range(5))
    cpu = MV.fuse_parts(*args("cpu"), npcs=torch.from_numpy(sc["npcs"]), picks=_picks, **kw)
    _assert_same(gpu, cpu, EXACT)
    assert bool(gpu.valid.any())
