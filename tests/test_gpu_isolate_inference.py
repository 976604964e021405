"""Object isolation in the frame entries on the GPU: ``prepare_frames`` / ``predict_frames`` / ``predict_frames_with_masks`` and the
command line with ``isolate``, against the same calls fed ``isolate_objects``' mask by hand.  2 scenes of 96 x 128 (a sphere on a
tilted table, tests/isolate_scenes.py) and an empty frame, 512 points."""
import numpy as np
import pytest
import torch

from tests import isolate_scenes as S
from tests import pipeline_runner as PR

pytestmark = pytest.mark.gpu
H, W, M, PRE = 96, 128, 512, 2
SEEDS = [3, 4, 0xffffffff]
RANSAC = 32
FIELDS = ("points", "counts", "sample_rows", "scale", "status", "source")


def _cfg(**kw):
    from gapartnet_amd.inference import IsolateConfig
    return IsolateConfig(**dict(S.CFG, **kw))


def _model(cuda):
    model = PR.build_model(cuda).eval()
    model.inference_dtype = None
    model.revoxelize_jitter = tuple(torch.tensor(j, device=cuda) for j in ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9]))
    return model


@pytest.fixture(scope="module")
def frames():
    a, b = S.make_scene(H, W, 41, radius=0.13), S.make_scene(H, W, 42, wall=True, radius=0.13)
    depth = np.stack([a["depth"], np.zeros((H, W), np.float32), b["depth"]])
    rgb = np.stack([a["rgb"], np.zeros((H, W, 3), np.uint8), b["rgb"]])
    assert a["object"].sum() > PRE * M, "the presample cuts the object's pixels"
    return depth, rgb, np.stack([a["K"]] * 3), [a, None, b]


def _eq(a, b):
    return torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0))


@pytest.mark.parametrize("sampler", ["fps", "grid"])
def test_prepare_frames_with_isolate_equals_the_mask_by_hand(cuda, frames, sampler):
    from gapartnet_amd import inference
    depth, rgb, K, scenes = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    keep = torch.ones((3, H, W), dtype=torch.uint8, device=cuda)
    keep[:, :, :55] = 0  # the caller's own mask cuts a part of the sphere
    cfg = _cfg(max_planes=2)
    kw = dict(num_points=M, presample=PRE, seed=SEEDS, flip=True, sampler=sampler)
    iso = inference.isolate_objects(t(depth), K, flip=True, keep=keep, seed=SEEDS, config=cfg)
    assert iso.status.cpu().tolist() == [inference.ISOLATE_OK, inference.ISOLATE_EMPTY, inference.ISOLATE_OK]
    assert not bool((iso.keep & (1 - keep)).any()) and int(iso.keep[0].sum()) > 0 and int(iso.keep[2].sum()) > 0
    for v in (0, 2):
        k = iso.keep[v].cpu().numpy() != 0
        assert not (k & ~scenes[v]["object"]).any(), "the mask lies inside the object"
    got = inference.prepare_frames(t(depth), t(rgb), K, keep=keep, isolate=cfg, **kw)
    want = inference.prepare_frames(t(depth), t(rgb), K, keep=iso.keep & keep, **kw)
    for f in FIELDS:
        assert _eq(getattr(got, f), getattr(want, f)), f
    for f in ("keep", "labels", "sizes", "planes", "plane_inliers", "n_planes", "chosen", "status"):
        assert _eq(getattr(got.isolation, f), getattr(iso, f)), f
    plain = inference.prepare_frames(t(depth), t(rgb), K, keep=keep, **kw)
    none = inference.prepare_frames(t(depth), t(rgb), K, keep=keep, isolate=None, **kw)
    for f in FIELDS:
        assert _eq(getattr(plain, f), getattr(none, f)), f
    assert none.isolation is None and not _eq(plain.sample_rows, got.sample_rows)


def _sync_count(fn):
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


def test_predict_frames_with_isolate(cuda, frames):
    from gapartnet_amd import inference
    from tests import inference_ref as R
    depth, rgb, K, _ = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    picks = lambda sizes: R.size_picks(sizes, RANSAC)  # noqa: E731
    predictor = inference.PartPredictor(_model(cuda), num_points=M, max_iters=RANSAC)
    cfg = _cfg()
    d, c, Kt = t(depth), t(rgb), torch.from_numpy(K)
    kw = dict(picks=picks, presample=PRE, seed=SEEDS, flip=True)
    got = predictor.predict_frames(d, c, Kt, isolate=cfg, **kw)
    iso = inference.isolate_objects(d, K, flip=True, seed=SEEDS, config=cfg)
    by_hand = predictor.predict_frames(d, c, Kt, keep=iso.keep, **kw)
    plain = predictor.predict_frames(d, c, Kt, **kw)
    status = iso.status.cpu().tolist()
    for v, (p, q) in enumerate(zip(got, by_hand)):
        assert torch.equal(p.keep, iso.keep[v]) and _eq(p.planes, iso.planes[v]) and p.isolate_status == status[v]
        outside = p.keep == 0
        assert bool((p.sem[outside] == -1).all()) and bool((p.instance[outside] == -1).all())
        for f in ("sem", "instance", "npcs", "proposal_scores", "bbox", "overlay", "sample_rows"):
            assert torch.equal(getattr(p, f), getattr(q, f)), (v, f)
        assert q.keep is None and q.planes is None and q.isolate_status is None
        assert {"keep", "planes", "isolate_status"} <= set(p.to_numpy()) and "keep" not in q.to_numpy()
    assert bool((got[0].sem[got[0].keep != 0] >= 0).all()) and bool((plain[0].sem >= 0).sum() > (got[0].sem >= 0).sum())
    n_plain = _sync_count(lambda: predictor.predict_frames(d, c, Kt, **kw))
    n_iso = _sync_count(lambda: predictor.predict_frames(d, c, Kt, isolate=cfg, **kw))
    print({"plain": n_plain, "isolate": n_iso})
    assert n_plain > 0, "the sync debug mode reports nothing on this build"
    assert n_iso <= n_plain + 1, (n_plain, n_iso)


def test_predict_frames_with_masks_and_isolate(cuda, frames):
    from gapartnet_amd import inference
    from tests import inference_ref as R
    depth, rgb, K, scenes = frames
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    masks, labels = [], []
    for sc in scenes:
        mk = np.zeros((2, H, W), bool)
        if sc is not None:
            mk[0], mk[1] = sc["object"], sc["object"]
            mk[0, :, W // 2:] = False
            mk[1, :, :W // 2] = False
        masks.append(t(mk))
        labels.append(torch.tensor([1, 2], device=cuda))
    predictor = inference.PartPredictor(_model(cuda), num_points=M, max_iters=RANSAC)
    got = predictor.predict_frames_with_masks(t(depth), t(rgb), torch.from_numpy(K), masks, labels, picks=lambda s: R.size_picks(s, RANSAC),
                                              presample=PRE, seed=SEEDS, flip=True, isolate=_cfg())
    assert [p.isolate_status for p in got] == [inference.ISOLATE_OK, inference.ISOLATE_EMPTY, inference.ISOLATE_OK]
    for p in got:
        assert p.masks is not None and p.keep.shape == (H, W) and p.planes.shape == (1, 4)
        assert bool((p.sem[p.keep == 0] == -1).all())
    assert int(got[0].masks.kept.sum()) > 0


def test_command_line_with_isolate(cuda, frames, tmp_path):
    from gapartnet_amd import inference
    depth, rgb, K, _ = frames
    model = _model(cuda)
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": model.state_dict(), "hyper_parameters": dict(model.hparams)}, ckpt)
    from PIL import Image
    np.save(tmp_path / "a.npy", depth[0])
    Image.fromarray(rgb[0]).save(tmp_path / "a_rgb.png")
    np.savetxt(tmp_path / "K.txt", K[0])
    out = tmp_path / "out"
    assert inference.main(["--ckpt", str(ckpt), "--depth", str(tmp_path / "a.npy"), "--rgb", str(tmp_path / "a_rgb.png"), "--intrinsics",
                           str(tmp_path / "K.txt"), "--flip", "--presample", str(PRE), "--seed", "3", "--out", str(out), "--num_points", str(M),
                           "--device", "cuda:0", "--isolate", "--isolate_planes", "1", "--plane_tol", "0.005", "--isolate_select", "largest",
                           "--z_max", "3.0"]) == 0
    got = np.load(out / "a.npz")
    assert {"keep", "planes", "isolate_status"} <= set(got.files)
    assert got["keep"].shape == (H, W) and got["planes"].shape == (1, 4) and int(got["isolate_status"]) == inference.ISOLATE_OK
    assert got["keep"].any() and (got["sem"][got["keep"] == 0] == -1).all()
