"""Part inference on RGB-D frames on the GPU: ``predict_frames`` / ``predict_frames_with_masks`` against ``predict`` /
``predict_with_masks`` on the cloud of the frame's rows with every pixel the presample dropped set to NaN (bit for bit), the
overlay against the restatement (tests/frame_ref.py), the command line.  2 frames of 96 x 128 and an empty one, 2048 points."""
import numpy as np
import pytest
import torch

from tests import frame_ref as F
from tests import inference_ref as R
from tests import pipeline_runner as PR

pytestmark = pytest.mark.gpu
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])
H, W, M, PRE = 96, 128, 2048, 2
SEEDS = [3, 4, 0xffffffff]
RANSAC = 32


def _model(cuda, inference_dtype=None):
    model = PR.build_model(cuda).eval()
    model.inference_dtype = inference_dtype
    model.revoxelize_jitter = tuple(torch.tensor(j, device=cuda) for j in JITTER)
    return model


@pytest.fixture(scope="module")
def frames():
    """the synthetic scenes seen by a camera, in front of a wall that fills the middle of the image (so that more than
    PRE * M pixels have depth: the presample cuts, FPS samples), and an empty frame between them"""
    a, c = (x.numpy()[:-8] for x in R.raw_clouds(20000))
    depth, rgb, K = F.frames_from_clouds([a, c], H, W)
    wall = np.zeros((H, W), bool)
    wall[8:-8, 10:-10] = True
    for v in range(2):
        depth[v][(depth[v] == 0) & wall] = depth[v].max() + np.float32(0.25)
    assert ((depth > 0).reshape(2, -1).sum(1) > PRE * M).all()
    z = np.zeros((1, H, W), np.float32)
    return (np.concatenate([depth[:1], z, depth[1:]]), np.concatenate([rgb[:1], np.zeros((1, H, W, 3), np.uint8), rgb[1:]]),
            np.concatenate([K[:1], K[:1], K[1:]]))


@pytest.fixture(scope="module")
def masked(frames):
    """per frame: (the NaN-masked rows [H*W, 6], valid [H*W], dropped [H*W] = valid but cut by the presample), flipped rows"""
    depth, rgb, K = frames
    out = []
    for v in range(3):
        rows, valid = F.backproject_np(depth[v], rgb[v], K[v], flip=True)
        cloud = F.masked_rows(rows, F.select_np(valid, SEEDS[v], PRE * M))
        out.append((cloud, valid, valid & ~np.isfinite(cloud[:, 0])))
    return out


def _picks(sizes):
    return R.size_picks(sizes, RANSAC)


@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_predict_frames_equals_predict_on_the_masked_cloud(cuda, frames, masked, dtype):
    from gapartnet_amd import inference
    depth, rgb, K = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    predictor = inference.PartPredictor(_model(cuda, dtype), num_points=M, max_iters=RANSAC)
    got = predictor.predict_frames(t(depth), t(rgb), torch.from_numpy(K), picks=_picks, presample=PRE, seed=SEEDS, flip=True)
    want = predictor.predict([t(c) for c, _, _ in masked], picks=_picks)
    assert [p.status for p in got] == [R.OK, R.EMPTY, R.OK]
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device=cuda)
    for v, (p, w) in enumerate(zip(got, want)):
        cloud, valid, dropped = masked[v]
        assert p.sem.shape == (H, W) and p.instance.shape == (H, W) and p.npcs.shape == (H, W, 3) and p.overlay.shape == (H, W, 3)
        sel = torch.from_numpy(~dropped).to(cuda)
        for f in ("sem", "instance", "npcs"):
            x = getattr(p, f).reshape((H * W,) + tuple(getattr(p, f).shape[2:]))
            assert torch.equal(x[sel], getattr(w, f)[sel]), (v, f)
        for f in ("proposal_scores", "proposal_classes", "box_proposal", "scale", "sample_rows"):
            assert torch.equal(getattr(p, f), getattr(w, f)), (v, f)
        hole = torch.from_numpy(~valid).to(cuda).reshape(H, W)
        assert bool((p.sem[hole] == -1).all()) and bool((p.instance[hole] == -1).all())
        assert torch.equal(p.bbox, w.bbox * sign)
        if p.status == R.OK:
            assert int(dropped.sum()) > 0 and int(p.sample_rows.shape[0]) == M
            assert bool((p.sem[~hole] >= 0).all())
            # a pixel the presample dropped carries the prediction of its nearest SAMPLED pixel (separate torch ops, lowest index on
            # ties), in the rows' coordinates
            rows = t(F.backproject_np(depth[v], rgb[v], K[v], flip=True)[0])
            q = rows[torch.from_numpy(dropped).to(cuda), :3]
            s = rows[p.sample_rows, :3]
            dx, dy, dz = q[:, None, 0] - s[None, :, 0], q[:, None, 1] - s[None, :, 1], q[:, None, 2] - s[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            nn = torch.where(d == d.amin(1, keepdim=True), torch.arange(M, device=cuda)[None, :], M).amin(1)
            flat = p.sem.reshape(-1)
            assert torch.equal(flat[torch.from_numpy(dropped).to(cuda)], flat[p.sample_rows[nn]])
        Q = p.bbox.shape[0]
        assert np.array_equal(p.corners_px.cpu().numpy(), F.corners_px(p.bbox.cpu().numpy(), K[v]).reshape(Q, 8, 2))
        assert np.array_equal(p.overlay.cpu().numpy(), F.overlay(rgb[v], p.bbox.cpu().numpy(), K[v])), v
    if dtype is None:
        assert sum(p.bbox.shape[0] for p in got) > 0, "the frames give boxes"
        assert any((p.overlay.cpu().numpy() != rgb[v]).any() for v, p in enumerate(got)), "a box is drawn"
    again = predictor.predict_frames(t(depth), t(rgb), torch.from_numpy(K), picks=_picks, presample=PRE, seed=SEEDS, flip=True)
    for p, q in zip(got, again):
        for f in ("sem", "instance", "npcs", "proposal_scores", "bbox", "overlay"):
            assert torch.equal(getattr(p, f), getattr(q, f)), f


def test_predict_frames_with_masks_equals_predict_with_masks(cuda, frames, masked):
    from gapartnet_amd import inference
    depth, rgb, K = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    rng = np.random.RandomState(4)
    masks, labels = [], []
    for k in (4, 2, 3):
        mk = np.zeros((k, H, W), bool)
        for j in range(k):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            mk[j, y0:y0 + H // 3, x0:x0 + W // 3] = True
        masks.append(t(mk))
        labels.append(t(rng.randint(1, 4, size=k)))
    predictor = inference.PartPredictor(_model(cuda), num_points=M, max_iters=RANSAC)
    got = predictor.predict_frames_with_masks(t(depth), t(rgb), torch.from_numpy(K), masks, labels, picks=_picks, presample=PRE, seed=SEEDS,
                                              flip=True)
    want = predictor.predict_with_masks([t(c) for c, _, _ in masked], [m.reshape(m.shape[0], H * W) for m in masks], labels, picks=_picks)
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device=cuda)
    for v, (p, w) in enumerate(zip(got, want)):
        assert p.status == w.status and p.masks is not None
        for f in inference.MASK_FIELDS:
            x, y = getattr(p.masks, f), getattr(w, f)
            if x.dtype.is_floating_point:
                x, y = torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)
            assert torch.equal(x, y), (v, f)
        sel = torch.from_numpy(~masked[v][2]).to(cuda)
        assert torch.equal(p.sem.reshape(-1)[sel], w.sem[sel])
        Km = w.valid.shape[0]
        assert p.bbox.shape == (Km, 8, 3) and torch.equal(torch.nan_to_num(p.bbox, nan=-7.0), torch.nan_to_num(w.bbox * sign, nan=-7.0))
        assert torch.equal(torch.isfinite(p.bbox).all(2).all(1), w.valid) and torch.equal(p.box_proposal, torch.arange(Km, device=cuda))
        assert torch.equal(torch.isfinite(p.corners_px).all(2).all(1), w.valid)
        assert bool((p.instance == -1).all()) and not bool(p.npcs.any())
        assert np.array_equal(p.overlay.cpu().numpy(), F.overlay(rgb[v], (w.bbox[w.valid] * sign).cpu().numpy(), K[v])), v
    assert int(sum(p.masks.kept.sum() for p in got)) > 0 and int(sum(p.masks.valid.sum() for p in got)) > 0, "a mask is kept and gets a box"
    assert any(int((~p.masks.valid).sum()) > 0 for p in got), "a mask without a box: its NaN corners are skipped by the drawing"


def test_command_line_on_frames_end_to_end(cuda, frames, tmp_path):
    from PIL import Image
    from gapartnet_amd import inference
    depth, rgb, K = frames
    model = _model(cuda)
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": model.state_dict(), "hyper_parameters": dict(model.hparams)}, ckpt)
    Image.fromarray(np.rint(depth[0] * 1000).astype(np.uint16)).save(tmp_path / "first.png")
    np.save(tmp_path / "second.npy", depth[2] * np.float32(1000))
    for name, img in (("first", rgb[0]), ("second", rgb[2])):
        Image.fromarray(img).save(tmp_path / f"{name}_rgb.png")
    np.savetxt(tmp_path / "K0.txt", K[0])
    np.save(tmp_path / "K2.npy", K[2])
    out = tmp_path / "out"
    p = lambda *names: [str(tmp_path / n) for n in names]  # noqa: E731
    assert inference.main(["--ckpt", str(ckpt), "--depth", *p("first.png", "second.npy"), "--rgb", *p("first_rgb.png", "second_rgb.png"),
                           "--intrinsics", *p("K0.txt", "K2.npy"), "--depth_scale", "1000", "--flip", "--presample", str(PRE), "--seed", "3",
                           "--out", str(out), "--num_points", str(M), "--device", "cuda:0"]) == 0
    for name in ("first", "second"):
        got = np.load(out / f"{name}.npz")
        for f in ("sem", "instance", "npcs", "proposal_scores", "proposal_classes", "bbox", "corners_px", "overlay", "scale", "status"):
            assert f in got.files, f
        assert got["sem"].shape == (H, W) and int(got["status"]) == R.OK
        assert np.array_equal(np.asarray(Image.open(out / f"{name}_overlay.png")), got["overlay"])
    # the float frame is its own batch (another depth type): the API on the same data gives the same maps
    predictor = inference.PartPredictor(model, num_points=M)
    want = predictor.predict_frames(torch.from_numpy(depth[2:] * np.float32(1000)).to(cuda), torch.from_numpy(rgb[2:]).to(cuda),
                                    torch.from_numpy(K[2:]), presample=PRE, seed=[4], depth_scale=1000.0, flip=True)[0]
    got = np.load(out / "second.npz")
    assert np.array_equal(got["sem"], want.sem.cpu().numpy()) and np.array_equal(got["scale"], want.scale.cpu().numpy())


def _sync_count(fn):
    """the synchronising torch calls fn() makes (device-to-host copies, nonzero, item ...), as torch's sync debug mode reports them"""
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


def test_frame_entries_read_the_host_as_often_as_the_cloud_entries(cuda, frames, masked):
    """host reads per call: ``predict_frames`` as ``predict`` and ``predict_frames_with_masks`` as ``predict_with_masks`` on the same
    data - nothing behind the shared bodies has a data-dependent size.  The debug mode also reports a blocking
    upload of host data, so the frame entries' small uploads (seeds, cameras, box scenes) have to be non-blocking as well"""
    from gapartnet_amd import inference
    depth, rgb, K = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    predictor = inference.PartPredictor(_model(cuda), num_points=M, max_iters=RANSAC)
    d, c, Kt, clouds = t(depth), t(rgb), torch.from_numpy(K), [t(x) for x, _, _ in masked]
    rng = np.random.RandomState(4)
    masks = [t(rng.rand(k, H, W) < 0.3) for k in (4, 2, 3)]
    labels = [t(rng.randint(1, 4, size=k)) for k in (4, 2, 3)]
    flat = [m.reshape(m.shape[0], H * W) for m in masks]
    kw = dict(picks=_picks, presample=PRE, seed=SEEDS, flip=True)
    calls = {"predict": lambda: predictor.predict(clouds, picks=_picks),
             "predict_frames": lambda: predictor.predict_frames(d, c, Kt, **kw),
             "predict_with_masks": lambda: predictor.predict_with_masks(clouds, flat, labels, picks=_picks),
             "predict_frames_with_masks": lambda: predictor.predict_frames_with_masks(d, c, Kt, masks, labels, **kw)}
    for fn in calls.values():
        fn()   # (warm-up: first calls build caches)
    n = {k: _sync_count(fn) for k, fn in calls.items()}
    print(n)
    assert n["predict"] > 0 and n["predict_with_masks"] > 0, "the sync debug mode reports nothing on this build"
    assert n["predict_frames"] == n["predict"], n
    assert n["predict_frames_with_masks"] == n["predict_with_masks"], n


def test_overlay_with_cameras_that_alternate(cuda):
    """frames 0 and 2 share a camera, frame 1 has another: the group of frames 0 and 2 is not a run of the batch"""
    from gapartnet_amd import inference
    Hh, Ww = 48, 64
    rng = np.random.RandomState(9)
    rgb = rng.randint(0, 256, size=(3, Hh, Ww, 3)).astype(np.uint8)
    A = np.array([[70.5, 0.0, 31.25], [0.0, 66.0, 24.5], [0.0, 0.0, 1.0]])
    B = np.array([[55.0, 0.0, 30.0], [0.0, 58.5, 22.75], [0.0, 0.0, 1.0]])
    K = np.stack([A, B, A])
    boxes = [rng.rand(q, 8, 3) * [1.2, 1.0, 0.5] + [-0.6, -0.5, 1.5] for q in (2, 3, 1)]
    boxes[1][0, 3] = np.nan                                    # a corner that is skipped
    got = inference.draw_overlays(torch.from_numpy(rgb).to(cuda), [torch.from_numpy(b).to(cuda) for b in boxes], torch.from_numpy(K))
    for v in range(3):
        want = F.overlay(rgb[v], boxes[v], K[v])
        assert np.array_equal(got[v].cpu().numpy(), want) and (want != rgb[v]).any(), v
