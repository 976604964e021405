"""Part inference with the opt-in octree-cell sampler (``sampler="grid"``) on the GPU: the frame entries against the cloud entries
on the NaN-masked rows (bit for bit), every pixel through its nearest grid sample, the host reads of the FPS path and no more,
the default sampler unchanged, the command line.  Tiny frames: 3 of 48 x 64 (one cut by the presample and sampled, one with fewer
valid pixels than num_points, one empty) and 2 of 24 x 32 (fewer pixels than num_points), 512 points."""
import numpy as np
import pytest
import torch

from tests import frame_ref as F
from tests import inference_ref as R
from tests import pipeline_runner as PR

pytestmark = pytest.mark.gpu
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])
M, PRE, RANSAC = 512, 2, 16
SEEDS = [0, 1, 2]   # (``predict`` gives cloud i the seed i)


def _model(cuda):
    model = PR.build_model(cuda).eval()
    model.revoxelize_jitter = tuple(torch.tensor(j, device=cuda) for j in JITTER)
    return model


@pytest.fixture(scope="module")
def model(cuda):
    return _model(cuda)


def _frames(size):
    H, W = size
    if size == (48, 64):
        a, c = (x.numpy()[:-8] for x in R.raw_clouds(20000))
        depth, rgb, K = F.frames_from_clouds([a, c], H, W)
        wall = np.zeros((H, W), bool)
        wall[4:-4, 5:-5] = True
        depth[0][(depth[0] == 0) & wall] = depth[0].max() + np.float32(0.25)   # more than PRE * M valid pixels: cut and sampled
        depth[1][:, W // 2:] = 0                                               # fewer than M valid pixels: every one is kept
        z = np.zeros((1, H, W), np.float32)
        depth, rgb, K = np.concatenate([depth, z]), np.concatenate([rgb, np.zeros((1, H, W, 3), np.uint8)]), np.concatenate([K, K[:1]])
        valid = (depth > 0).reshape(3, -1).sum(1)
        assert valid[0] > PRE * M and 0 < valid[1] < M and valid[2] == 0
        return depth, rgb, K
    depth, rgb, K = F.synthetic_frames(2, H, W, seed=5)
    return depth, rgb, K


def _masked(frames, V):
    depth, rgb, K = frames
    out = []
    for v in range(V):
        rows, valid = F.backproject_np(depth[v], rgb[v], K[v], flip=True)
        cloud = F.masked_rows(rows, F.select_np(valid, SEEDS[v], PRE * M))
        out.append((cloud, valid))
    return out


def _picks(sizes):
    return R.size_picks(sizes, RANSAC)


@pytest.mark.parametrize("size", [(48, 64), (24, 32)])
def test_predict_frames_with_the_grid_sampler_equals_predict_on_the_masked_cloud(cuda, model, size):
    from gapartnet_amd import inference
    H, W = size
    depth, rgb, K = _frames(size)
    V = depth.shape[0]
    masked = _masked((depth, rgb, K), V)
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    predictor = inference.PartPredictor(model, num_points=M, max_iters=RANSAC, sampler="grid")
    got = predictor.predict_frames(t(depth), t(rgb), torch.from_numpy(K), picks=_picks, presample=PRE, seed=SEEDS[:V], flip=True)
    want = predictor.predict([t(c) for c, _ in masked], picks=_picks)
    prep = inference.prepare_frames(t(depth), t(rgb), torch.from_numpy(K), num_points=M, presample=PRE, seed=SEEDS[:V], flip=True,
                                    sampler="grid")
    if size == (48, 64):
        assert [p.status for p in got] == [R.OK, R.OK, R.EMPTY]
        assert int(prep.level[0]) >= 1 and prep.level.tolist()[1:] == [-1, -1]
        assert int(got[0].sample_rows.shape[0]) == M and 0 < int(got[1].sample_rows.shape[0]) < M
    else:
        assert [p.status for p in got] == [R.OK, R.OK] and prep.level.tolist() == [-1, -1]
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device=cuda)
    for v, (p, w) in enumerate(zip(got, want)):
        cloud, valid = masked[v]
        kept = torch.from_numpy(np.isfinite(cloud[:, 0])).to(cuda)
        for f in ("sem", "instance", "npcs"):
            x = getattr(p, f).reshape((H * W,) + tuple(getattr(p, f).shape[2:]))
            assert torch.equal(x[kept], getattr(w, f)[kept]), (v, f)
        for f in ("proposal_scores", "proposal_classes", "box_proposal", "scale", "sample_rows"):
            assert torch.equal(getattr(p, f), getattr(w, f)), (v, f)
        assert torch.equal(p.bbox, w.bbox * sign)
        hole = torch.from_numpy(~valid).to(cuda)
        flat = p.sem.reshape(-1)
        assert bool((flat[hole] == -1).all())
        if p.status != R.OK:
            continue
        assert bool((p.sample_rows[1:] > p.sample_rows[:-1]).all()), "grid samples come in ascending pixel order"
        # every pixel with depth carries the prediction of its nearest grid sample (separate torch ops, lowest index on ties)
        rows = t(F.backproject_np(depth[v], rgb[v], K[v], flip=True)[0])
        q, s = rows[~hole, :3], rows[p.sample_rows, :3]
        ms = s.shape[0]
        dx, dy, dz = q[:, None, 0] - s[None, :, 0], q[:, None, 1] - s[None, :, 1], q[:, None, 2] - s[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        nn = torch.where(d == d.amin(1, keepdim=True), torch.arange(ms, device=cuda)[None, :], ms).amin(1)
        assert torch.equal(flat[~hole], flat[p.sample_rows[nn]]), v
        assert bool((flat[~hole] >= 0).all())


def test_predict_frames_with_masks_and_the_grid_sampler(cuda, model):
    from gapartnet_amd import inference
    H, W = 48, 64
    depth, rgb, K = _frames((H, W))
    masked = _masked((depth, rgb, K), 3)
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    rng = np.random.RandomState(4)
    masks, labels = [], []
    for k in (4, 2, 3):
        mk = np.zeros((k, H, W), bool)
        for j in range(k):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            mk[j, y0:y0 + H // 2, x0:x0 + W // 2] = True
        masks.append(t(mk))
        labels.append(t(rng.randint(1, 4, size=k)))
    predictor = inference.PartPredictor(model, num_points=M, max_iters=RANSAC, sampler="grid")
    got = predictor.predict_frames_with_masks(t(depth), t(rgb), torch.from_numpy(K), masks, labels, picks=_picks, presample=PRE, seed=SEEDS,
                                              flip=True)
    want = predictor.predict_with_masks([t(c) for c, _ in masked], [m.reshape(m.shape[0], H * W) for m in masks], labels, picks=_picks)
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device=cuda)
    for v, (p, w) in enumerate(zip(got, want)):
        assert p.status == w.status and p.masks is not None
        for f in inference.MASK_FIELDS:
            x, y = getattr(p.masks, f), getattr(w, f)
            if x.dtype.is_floating_point:
                x, y = torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)
            assert torch.equal(x, y), (v, f)
        kept = torch.from_numpy(np.isfinite(masked[v][0][:, 0])).to(cuda)
        assert torch.equal(p.sem.reshape(-1)[kept], w.sem[kept]) and torch.equal(p.sample_rows, w.sample_rows)
        assert torch.equal(torch.nan_to_num(p.bbox, nan=-7.0), torch.nan_to_num(w.bbox * sign, nan=-7.0))
    assert int(sum(p.masks.kept.sum() for p in got)) > 0, "a mask is kept"


def _sync_count(fn):
    """the synchronising torch calls fn() makes, as torch's sync debug mode reports them (tests/test_gpu_frame_inference.py)"""
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


def test_the_grid_sampler_reads_the_host_as_often_as_fps_and_the_default_is_unchanged(cuda, model):
    from gapartnet_amd import hip_ops, inference
    H, W = 48, 64
    depth, rgb, K = _frames((H, W))
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    d, c, Kt = t(depth), t(rgb), torch.from_numpy(K)
    clouds = [t(x) for x, _ in _masked((depth, rgb, K), 3)]
    kw = dict(picks=_picks, presample=PRE, seed=SEEDS, flip=True)
    fps = inference.PartPredictor(model, num_points=M, max_iters=RANSAC)
    named = inference.PartPredictor(model, num_points=M, max_iters=RANSAC, sampler="fps")
    grid = inference.PartPredictor(model, num_points=M, max_iters=RANSAC, sampler="grid")
    calls = {"fps_frames": lambda: fps.predict_frames(d, c, Kt, **kw), "grid_frames": lambda: grid.predict_frames(d, c, Kt, **kw),
             "fps_clouds": lambda: fps.predict(clouds, picks=_picks), "grid_clouds": lambda: grid.predict(clouds, picks=_picks)}
    first = {k: fn() for k, fn in calls.items()}   # (warm-up: first calls build caches)
    n = {k: _sync_count(fn) for k, fn in calls.items()}
    print(n)
    assert n["fps_frames"] > 0, "the sync debug mode reports nothing on this build"
    assert n["grid_frames"] == n["fps_frames"] and n["grid_clouds"] == n["fps_clouds"], n
    # the default: the same bits with and without the keyword, and another sample set than the grid's
    for p, q in zip(first["fps_frames"], named.predict_frames(d, c, Kt, **kw)):
        for f in ("sem", "instance", "npcs", "proposal_scores", "bbox", "overlay", "sample_rows"):
            assert torch.equal(getattr(p, f), getattr(q, f)), f
    assert not torch.equal(first["fps_frames"][0].sample_rows, first["grid_frames"][0].sample_rows)
    a = hip_ops.frame_prepare(d, c, Kt.to(cuda), M, PRE * M, SEEDS, flip=True)
    b = hip_ops.frame_prepare(d, c, Kt.to(cuda), M, PRE * M, SEEDS, flip=True, sampler="fps")
    assert "level" not in a and "level" not in b
    for f in ("out", "sample_rows", "counts", "status", "scale"):
        assert torch.equal(a[f], b[f]), f


def test_command_line_with_the_grid_sampler_on_frames_and_clouds(cuda, model, tmp_path):
    from PIL import Image
    from gapartnet_amd import inference
    H, W = 48, 64
    depth, rgb, K = _frames((H, W))
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": model.state_dict(), "hyper_parameters": dict(model.hparams)}, ckpt)
    np.save(tmp_path / "first.npy", depth[0])
    Image.fromarray(rgb[0]).save(tmp_path / "first_rgb.png")
    np.savetxt(tmp_path / "K0.txt", K[0])
    out = tmp_path / "out"
    common = ["--ckpt", str(ckpt), "--out", str(out), "--num_points", str(M), "--device", "cuda:0", "--sampler", "grid"]
    assert inference.main(common + ["--depth", str(tmp_path / "first.npy"), "--rgb", str(tmp_path / "first_rgb.png"), "--intrinsics",
                                    str(tmp_path / "K0.txt"), "--flip", "--presample", str(PRE), "--seed", "0"]) == 0
    got = np.load(out / "first.npz")
    predictor = inference.PartPredictor(model, num_points=M, sampler="grid")
    want = predictor.predict_frames(torch.from_numpy(depth[:1]).to(cuda), torch.from_numpy(rgb[:1]).to(cuda), torch.from_numpy(K[:1]),
                                    presample=PRE, seed=[0], flip=True)[0]
    assert np.array_equal(got["sem"], want.sem.cpu().numpy()) and np.array_equal(got["sample_rows"], want.sample_rows.cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(out / "first_overlay.png")), got["overlay"])
    cloud, _ = R.raw_clouds()
    np.save(tmp_path / "cloud.npy", cloud.numpy())
    assert inference.main(common + ["--input", str(tmp_path / "cloud.npy")]) == 0
    got = np.load(out / "cloud.npz")
    want = inference.prepare_clouds([cloud.to(cuda)], M, sampler="grid")
    assert np.array_equal(got["sample_rows"], want.sample_rows.cpu().numpy()) and int(want.level[0]) >= 0
