"""RGB-D frames without a GPU: the numpy restatement of include/gpn.h section FR (tests/frame_ref.py) against the reference's own
back-projection and box drawing (tests/golden/frames_backproject.npz), the properties of the seeded presample, and
``prepare_frames`` / ``PartPredictor.predict_frames`` / ``predict_frames_with_masks`` / the command line on CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from gapartnet_amd import backend, inference
from tests import frame_ref as F
from tests import inference_ref as R
from tests import pipeline_runner as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "frames_backproject.npz")
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---------------------------------------------------------------------------------------------------- restatement vs reference
def test_restatement_reproduces_the_references_back_projection(gold):
    for name in gold["names"]:
        depth, rgb, K = gold[f"{name}/depth"], gold[f"{name}/rgb"], gold[f"{name}/K"]
        H, W = depth.shape
        assert K[0, 0] != K[1, 1] and (depth == 0).any() and (depth >= 0).all()
        rows, valid = F.backproject(depth, rgb, K)
        assert np.array_equal(valid, (depth != 0).reshape(-1)), name                     # the reference's valid_point_mask
        assert np.array_equal(rows[valid, :3], gold[f"{name}/xyz"].astype(np.float32)[valid]), name
        assert np.isnan(rows[~valid, :3]).all()
        assert np.array_equal(rows[:, 3:], gold[f"{name}/colour"].astype(np.float32)), name
        # row = pixel in row-major order: the reference's per_point_idx
        assert np.array_equal(gold[f"{name}/pixel"], np.stack(np.divmod(np.arange(H * W), W), 1))
        # ... and the package's own host formulation gives the same rows
        got, gv = inference._backproject_numpy(depth[None], rgb[None], K[None], None, 1.0, False)
        assert np.array_equal(gv[0], valid) and np.array_equal(got, rows, equal_nan=True)
        fast, fastv = F.backproject_np(depth, rgb, K)
        assert np.array_equal(fastv, valid) and np.array_equal(fast, rows, equal_nan=True)
        # mode 2 of get_pc: y and z negated
        flipped, fv = F.backproject(depth, rgb, K, flip=True)
        assert np.array_equal(fv, valid) and np.array_equal(flipped[valid, :3], rows[valid, :3] * np.float32([1, -1, -1]))


def test_restatement_reproduces_the_references_box_corners_and_draw_order(gold):
    corners = F.corners_px(gold["boxes"], gold["boxes_K"])
    assert np.isfinite(corners).all()
    a, b, bgr, t = gold["line_a"], gold["line_b"], gold["line_bgr"], gold["line_thickness"]
    assert a.shape == (2 * len(F.VR.BOX_DRAWS), 2)
    k = 0
    for q in range(gold["boxes"].shape[0]):
        for ca, cb, colour, thick in F.VR.BOX_DRAWS:
            assert np.array_equal(corners[q, ca], a[k]) and np.array_equal(corners[q, cb], b[k]), (q, ca, cb)
            assert tuple(bgr[k][::-1]) == colour and t[k] == thick   # (cv2 takes BGR; the header lists the colours as written)
            k += 1
    got = inference.project_corners(torch.from_numpy(gold["boxes"]), torch.from_numpy(gold["boxes_K"]))
    assert np.array_equal(got.numpy(), corners)
    # the overlay of the package's host path is the restatement's
    H, W = (int(v) for v in gold["boxes_hw"])
    rgb = np.random.RandomState(0).randint(0, 256, size=(1, H, W, 3)).astype(np.uint8)
    over = inference.draw_overlays(torch.from_numpy(rgb), [torch.from_numpy(gold["boxes"])], torch.from_numpy(gold["boxes_K"])[None])
    want = F.overlay(rgb[0], gold["boxes"], gold["boxes_K"])
    assert np.array_equal(over[0].numpy(), want) and (want != rgb[0]).any()


def test_validity_rule():
    depth = np.array([[1.0, 0.0, -1.0, np.nan], [np.inf, -np.inf, 2.0, 3.0e38]], np.float32)
    rgb = np.zeros((2, 4, 3), np.uint8)
    K = np.array([[0.5, 0, 10.0], [0, 0.5, 10.0], [0, 0, 1]])
    keep = np.ones((2, 4), np.uint8)
    keep[1, 2] = 0
    rows, valid = F.backproject(depth, rgb, K, keep=keep)
    # finite and > 0 and kept; 3e38 overflows float32 in x: invalid as well
    assert valid.tolist() == [True, False, False, False, False, False, False, False]
    assert np.isnan(rows[~valid, :3]).all()
    got, gv = inference._backproject_numpy(depth[None], rgb[None], K[None], keep[None], 1.0, False)
    assert np.array_equal(gv[0], valid) and np.array_equal(got, rows, equal_nan=True)
    fast, fastv = F.backproject_np(depth, rgb, K, keep=keep)
    assert np.array_equal(fastv, valid) and np.array_equal(fast, rows, equal_nan=True)
    # u16 with a scale
    d16 = np.array([[0, 1000, 65535]], np.uint16)
    rows, valid = F.backproject(d16, np.zeros((1, 3, 3), np.uint8), K, depth_scale=1000.0)
    assert valid.tolist() == [False, True, True] and rows[1, 2] == np.float32(1.0) and rows[2, 2] == np.float32(65.535)


# ---------------------------------------------------------------------------------------------------- selection
def test_hash_is_the_one_written_in_the_header():
    text = open(os.path.join(ROOT, "include", "gpn.h")).read()
    for token in ("0x7feb352d", "0x846ca68b", "0x9E3779B9", "x >> 16", "x >> 15"):
        assert token in text, token
    pix = np.arange(0, 5000, 7)
    for seed in (0, 1, 0xffffffff, 123456789):
        for bits in (32, 4, 1):
            want = np.asarray([F.hash_pixel(seed, int(p), bits) for p in pix], dtype=np.uint32)
            assert np.array_equal(inference.frame_hash(seed, pix, bits), want)
            assert np.array_equal(F.hash_np(seed, pix, bits), want.astype(np.uint64))
    assert F.hash_pixel(0, 0) == 0 and F.hash_pixel(1, 0) != F.hash_pixel(0, 1)


@pytest.mark.parametrize("seed", range(8))
def test_selection_properties(seed):
    rng = np.random.RandomState(100 + seed)
    valid = rng.rand(40 * 50) < 0.7
    cap = 300
    kept = F.select(valid, seed, cap)
    assert kept.shape == (cap,) and bool((np.diff(kept) > 0).all()) and bool(valid[kept].all())
    assert np.array_equal(kept, F.select(valid, seed, cap))
    assert not np.array_equal(kept, F.select(valid, seed + 8, cap))
    assert np.array_equal(inference.select_pixels(np.nonzero(valid)[0], seed, cap), kept)
    assert np.array_equal(F.select_np(valid, seed, cap), kept) and np.array_equal(F.select_np(valid, seed, cap, 4), F.select(valid, seed, cap, 4))
    # at most cap valid pixels: all of them
    few = valid & (np.arange(valid.shape[0]) < 350)
    assert np.array_equal(F.select(few, seed, int(few.sum())), np.nonzero(few)[0])
    assert np.array_equal(F.select(few, seed, 0), np.nonzero(few)[0])
    # ties: with 4 and 1 hash bits most keys share their hash, the pixel index decides
    for bits in (4, 1):
        kept = F.select(valid, seed, cap, bits)
        pix = np.nonzero(valid)[0]
        h = np.asarray([F.hash_pixel(seed, int(p), bits) for p in pix])
        order = np.lexsort((pix, h))      # by hash, then by pixel
        assert np.array_equal(kept, np.sort(pix[order[:cap]]))
        assert np.array_equal(inference.select_pixels(pix, seed, cap, bits), kept)
        t = h[order[cap - 1]]
        assert (h == t).sum() > 1, "the case has ties on the threshold"


@pytest.mark.parametrize("seed", range(8))
def test_selection_is_uniform_over_the_frame(seed):
    """256 x 256 all-valid, cap 16384: the kept pixels of every 32 x 32 block, row and column within 5 sigma of the
    hypergeometric mean (drawing n of N pixels without replacement, a cell of c pixels: mean n c / N,
    variance n (c / N) (1 - c / N) (N - n) / (N - 1))"""
    H = W = 256
    N, n = H * W, 16384
    kept = inference.select_pixels(np.arange(N), seed, n)
    assert np.array_equal(kept, F.select(np.ones(N, bool), seed, n))
    img = np.zeros(N, bool)
    img[kept] = True
    img = img.reshape(H, W)
    worst = 0.0
    for counts, c in ((img.reshape(8, 32, 8, 32).sum((1, 3)).reshape(-1), 32 * 32), (img.sum(1), W), (img.sum(0), H)):
        mean = n * c / N
        sigma = np.sqrt(n * (c / N) * (1 - c / N) * (N - n) / (N - 1))
        worst = max(worst, float(np.abs(counts - mean).max() / sigma))
    print(f"seed {seed}: worst deviation {worst:.2f} sigma")
    assert worst <= 5.0


# ---------------------------------------------------------------------------------------------------- prepare_frames on CPU
def _prep_equal(prep, want):
    assert prep.status.tolist() == want.status.tolist() and prep.counts.tolist() == want.counts.tolist()
    assert list(prep.offsets) == list(want.offsets)
    for f in ("points", "sample_rows", "scale"):
        assert torch.equal(getattr(prep, f), getattr(want, f)), f


@pytest.mark.parametrize("kind", ["f32", "f64", "u16"])
def test_prepare_frames_on_cpu_equals_prepare_clouds_on_the_masked_rows(kind):
    V, H, W, m, pre = 3, 23, 31, 64, 4
    depth, rgb, K = F.synthetic_frames(V, H, W, seed=3)
    depth[1] = 0                                          # an empty frame in the middle
    scale = 1.0
    if kind == "f64":
        depth = depth.astype(np.float64)
    elif kind == "u16":
        depth, scale = np.rint(depth * 1000).astype(np.uint16), 1000.0
    keep = np.ones((V, H, W), np.uint8)
    keep[0, :3] = 0
    seeds = [5, 6, 0xffffffff]
    prep = inference.prepare_frames(torch.from_numpy(depth), torch.from_numpy(rgb), torch.from_numpy(K), num_points=m, presample=pre,
                                    seed=seeds, keep=torch.from_numpy(keep), depth_scale=scale, flip=True)
    clouds, n_valid = [], []
    for v in range(V):
        rows, valid = F.backproject(depth[v], rgb[v], K[v], keep=keep[v], depth_scale=scale, flip=True)
        n_valid.append(int(valid.sum()))
        assert np.array_equal(prep.source[v * H * W:(v + 1) * H * W].numpy(), rows, equal_nan=True)
        clouds.append(torch.from_numpy(F.masked_rows(rows, F.select(valid, seeds[v], pre * m))))
    assert n_valid[0] > pre * m and n_valid[1] == 0, "the case cuts frame 0 and has an empty frame"
    want = inference.prepare_clouds(clouds, num_points=m)
    _prep_equal(prep, want)
    assert prep.status.tolist() == [R.OK, R.EMPTY, R.OK]
    # nearest: every VALID pixel finds a sample, also the ones the presample dropped
    nn = inference.nearest_samples(prep).numpy()
    assert np.array_equal(nn >= 0, np.isfinite(prep.source[:, 0].numpy()) & np.repeat(prep.status.numpy() == R.OK, H * W))
    # presample 0: no cut; an int seed s gives frame v the seed s + v
    full = inference.prepare_frames(torch.from_numpy(depth), torch.from_numpy(rgb), torch.from_numpy(K), num_points=m, presample=0)
    _prep_equal(full, inference.prepare_clouds([full.source[v * H * W:(v + 1) * H * W] for v in range(V)], num_points=m))
    a = inference.prepare_frames(torch.from_numpy(depth), torch.from_numpy(rgb), torch.from_numpy(K), num_points=m, seed=7)
    b = inference.prepare_frames(torch.from_numpy(depth), torch.from_numpy(rgb), torch.from_numpy(K), num_points=m, seed=[7, 8, 9])
    _prep_equal(a, b)


# ---------------------------------------------------------------------------------------------------- predictor, command line
@pytest.fixture(scope="module")
def oracle_model():
    from oracle import torch_ops
    with backend.using(torch_ops):
        model = PR.build_model(torch.device("cpu")).eval()
        model._current_epoch = 10
        model.revoxelize_jitter = tuple(torch.tensor(j) for j in JITTER)
        yield model


@pytest.fixture(scope="module")
def frames():
    """two frames that show the synthetic scenes and an empty one between them: depth [3,H,W] f32, rgb, K"""
    H, W = 64, 88
    a, c = (x.numpy() for x in R.raw_clouds(4000))
    depth, rgb, K = F.frames_from_clouds([a, c], H, W)
    z = np.zeros((1, H, W), np.float32)
    return (np.concatenate([depth[:1], z, depth[1:]]), np.concatenate([rgb[:1], np.zeros((1, H, W, 3), np.uint8), rgb[1:]]),
            np.concatenate([K[:1], K[:1], K[1:]]))


FIELDS = ("sem", "instance", "npcs", "proposal_scores", "proposal_classes", "box_proposal", "scale", "sample_rows")


@pytest.mark.parametrize("flip", [False, True])
def test_predict_frames_on_cpu_tensors(oracle_model, frames, flip):
    depth, rgb, K = frames
    V, H, W = depth.shape
    m, pre, seeds = 512, 1, [3, 4, 5]
    predictor = inference.PartPredictor(oracle_model, num_points=m, max_iters=16)
    t = lambda x: torch.from_numpy(x)  # noqa: E731
    preds = predictor.predict_frames(t(depth), t(rgb), t(K), picks=R.size_picks, presample=pre, seed=seeds, flip=flip)
    assert [p.status for p in preds] == [R.OK, R.EMPTY, R.OK]
    clouds, valids = [], []
    for v in range(V):
        rows, valid = F.backproject(depth[v], rgb[v], K[v], flip=flip)
        valids.append(valid)
        clouds.append(torch.from_numpy(F.masked_rows(rows, F.select(valid, seeds[v], pre * m))))
    assert int(valids[0].sum()) > pre * m, "the presample cuts frame 0"
    want = predictor.predict(clouds, picks=R.size_picks)
    sign = torch.tensor([1.0, -1.0, -1.0] if flip else [1.0, 1.0, 1.0], dtype=torch.float64)
    for v, (p, w) in enumerate(zip(preds, want)):
        assert p.sem.shape == (H, W) and p.sem.dtype == torch.int64 and p.instance.shape == (H, W) and p.npcs.shape == (H, W, 3)
        assert p.overlay.shape == (H, W, 3) and p.overlay.dtype == torch.uint8 and p.bbox.dtype == torch.float64
        Q = p.bbox.shape[0]
        assert p.bbox.shape == (Q, 8, 3) and p.corners_px.shape == (Q, 8, 2)
        # the presample drops pixels from the SAMPLING only: a dropped valid pixel still gets its nearest sample's prediction,
        # the masked cloud's row of it is invalid
        dropped = torch.from_numpy(valids[v]) & ~torch.isfinite(clouds[v][:, 0])
        sel = ~dropped
        for f in FIELDS:
            x, y = getattr(p, f), getattr(w, f)
            if f in ("sem", "instance", "npcs"):
                x = x.reshape((H * W,) + tuple(x.shape[2:]))
                assert torch.equal(x[sel], y[sel]), f
            else:
                assert torch.equal(x, y), f
        hole = torch.from_numpy(~valids[v]).reshape(H, W)
        assert bool((p.sem[hole] == -1).all()) and bool((p.instance[hole] == -1).all())
        if p.status == R.OK:
            assert bool((p.sem[~hole] >= 0).all())
        assert torch.equal(p.bbox, w.bbox * sign)                       # the camera frame: un-flipped
        assert np.array_equal(p.corners_px.numpy(), F.corners_px(p.bbox.numpy(), K[v]).reshape(Q, 8, 2))
        assert np.array_equal(p.overlay.numpy(), F.overlay(rgb[v], p.bbox.numpy(), K[v]))
    assert sum(p.proposal_scores.shape[0] for p in preds) > 0 and sum(p.bbox.shape[0] for p in preds) > 0, "the frames give parts"
    if flip:
        plain = predictor.predict_frames(t(depth), t(rgb), t(K), picks=R.size_picks, presample=pre, seed=seeds)
        assert not torch.equal(plain[0].scale[2:], preds[0].scale[2:])   # the network saw mirrored rows


def test_predict_frames_with_masks_on_cpu_tensors(oracle_model, frames):
    depth, rgb, K = frames
    V, H, W = depth.shape
    m, pre, seeds = 512, 1, [3, 4, 5]
    rng = np.random.RandomState(2)
    masks, labels = [], []
    for v, k in enumerate((3, 2, 0)):
        mk = np.zeros((k, H, W), bool)
        for j in range(k):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            mk[j, y0:y0 + H // 2, x0:x0 + W // 2] = True
        masks.append(torch.from_numpy(mk))
        labels.append(torch.from_numpy(rng.randint(1, 4, size=k)))
    predictor = inference.PartPredictor(oracle_model, num_points=m, max_iters=16)
    t = lambda x: torch.from_numpy(x)  # noqa: E731
    got = predictor.predict_frames_with_masks(t(depth), t(rgb), t(K), masks, labels, picks=R.size_picks, presample=pre, seed=seeds, flip=True)
    clouds = []
    for v in range(V):
        rows, valid = F.backproject(depth[v], rgb[v], K[v], flip=True)
        clouds.append(torch.from_numpy(F.masked_rows(rows, F.select(valid, seeds[v], pre * m))))
    want = predictor.predict_with_masks(clouds, [mk.reshape(mk.shape[0], H * W) for mk in masks], labels, picks=R.size_picks)
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)
    for v, (p, w) in enumerate(zip(got, want)):
        assert p.masks is not None and p.status == w.status
        for f in inference.MASK_FIELDS:
            x, y = getattr(p.masks, f), getattr(w, f)
            assert torch.equal(x, y) or (x.dtype.is_floating_point and torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))), f
        # per mask, in the caller's order; NaN where the mask has no valid box; only the valid ones are drawn
        Km = w.valid.shape[0]
        assert torch.equal(torch.nan_to_num(p.bbox, nan=-7.0), torch.nan_to_num(w.bbox * sign, nan=-7.0)) and p.bbox.shape == (Km, 8, 3)
        assert torch.equal(torch.isfinite(p.bbox).all(2).all(1), w.valid) and torch.equal(p.box_proposal, torch.arange(Km))
        assert torch.equal(torch.isfinite(p.corners_px).all(2).all(1), w.valid)
        assert torch.equal(torch.nan_to_num(p.proposal_scores, nan=-7.0), torch.nan_to_num(w.score, nan=-7.0))
        assert torch.equal(p.proposal_classes, w.label)
        assert p.sem.shape == (H, W) and bool((p.instance == -1).all()) and not bool(p.npcs.any())
        assert np.array_equal(p.overlay.numpy(), F.overlay(rgb[v], (w.bbox[w.valid] * sign).numpy(), K[v]))
        assert "mask_bbox" in p.to_numpy() and "masks" not in p.to_numpy()
    assert int(got[0].masks.kept.sum()) > 0, "a mask of frame 0 is kept"
    with pytest.raises(ValueError):
        predictor.predict_frames_with_masks(t(depth), t(rgb), t(K), [mk[:, :-1] for mk in masks], labels)


def test_command_line_on_frames(oracle_model, frames, tmp_path):
    from PIL import Image
    depth, rgb, K = frames
    V, H, W = depth.shape
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": oracle_model.state_dict(), "hyper_parameters": dict(oracle_model.hparams)}, ckpt)
    mm = np.rint(depth[0] * 1000).astype(np.uint16)
    Image.fromarray(mm).save(tmp_path / "first.png")                     # a 16-bit PNG in millimetres
    np.save(tmp_path / "second.npy", (depth[2].astype(np.float64) * 1000))
    small = np.ascontiguousarray(depth[2][:48, :64])
    np.save(tmp_path / "third.npy", small * 1000)                        # another size: its own batch
    for name, img in (("first", rgb[0]), ("second", rgb[2]), ("third", np.ascontiguousarray(rgb[2][:48, :64]))):
        Image.fromarray(img).save(tmp_path / f"{name}_rgb.png")
    np.savetxt(tmp_path / "K0.txt", K[0])
    np.save(tmp_path / "K2.npy", K[2])
    keep = np.full((H, W), 255, np.uint8)
    keep[:, :4] = 0
    for name, k in (("first", keep), ("second", keep), ("third", keep[:48, :64])):
        Image.fromarray(np.ascontiguousarray(k)).save(tmp_path / f"{name}_keep.png")
    out = tmp_path / "out"
    p = lambda *names: [str(tmp_path / n) for n in names]  # noqa: E731
    rc = inference.main(["--ckpt", str(ckpt), "--depth", *p("first.png", "second.npy", "third.npy"), "--rgb",
                         *p("first_rgb.png", "second_rgb.png", "third_rgb.png"), "--intrinsics", *p("K0.txt", "K2.npy", "K2.npy"),
                         "--depth_scale", "1000", "--keep_mask", *p("first_keep.png", "second_keep.png", "third_keep.png"), "--flip",
                         "--presample", "1", "--seed", "3", "--out", str(out), "--num_points", "512", "--device", "cpu"])
    assert rc == 0
    for name, shape in (("first", (H, W)), ("second", (H, W)), ("third", (48, 64))):
        got = np.load(out / f"{name}.npz")
        for f in ("sem", "instance", "npcs", "proposal_scores", "proposal_classes", "bbox", "corners_px", "overlay", "scale", "status"):
            assert f in got.files, f
        assert got["sem"].shape == shape and got["npcs"].shape == shape + (3,) and int(got["status"]) == R.OK
        assert (got["sem"][:, :4] == -1).all()                           # the keep mask
        png = np.asarray(Image.open(out / f"{name}_overlay.png"))
        assert np.array_equal(png, got["overlay"])
    # the u16 PNG went in as uint16 with the scale: the API on the same data gives the same maps
    predictor = inference.PartPredictor(oracle_model, num_points=512)
    want = predictor.predict_frames(torch.from_numpy(mm[None]), torch.from_numpy(rgb[:1]), torch.from_numpy(K[:1]), presample=1, seed=3,
                                    keep=torch.from_numpy(keep[None]), depth_scale=1000.0, flip=True)[0]
    got = np.load(out / "first.npz")
    assert np.array_equal(got["sem"], want.sem.numpy()) and np.array_equal(got["scale"], want.scale.numpy())
    with pytest.raises(SystemExit):
        inference.main(["--ckpt", str(ckpt), "--out", str(out)])


def test_header_declares_the_frame_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpn.h")).read(), flags=re.S)
    for name in ("gpn_frame_backproject", "gpn_frame_select_ws_bytes", "gpn_frame_select"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
    core = open(os.path.join(ROOT, "gapartnet_amd", "csrc", "gpn_core.hip")).read()
    assert '"gpn_frame_backproject"' in core and '"gpn_frame_select"' in core and '"gpn_frame_select_ws_bytes"' in core
    assert "frameprep.hip" in open(os.path.join(ROOT, "gapartnet_amd", "csrc", "Makefile")).read()
