"""The grounding path without a GPU: the oracle (tests/ground_ref.py) against Pillow itself and against the golden file recorded
from Pillow and scikit-learn (tests/golden/grounding.npz), the module's CPU formulation against both, the bank reader, the
command line's argument errors."""
import os

import numpy as np
import pytest
import torch

from tests import ground_ref as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grounding.npz")
SHAPES = [((96, 128), (50, 50)), ((50, 50), (50, 50)), ((37, 53), (16, 12)), ((8, 8), (50, 50)), ((101, 64), (1, 1)), ((800, 800), (50, 50))]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_masks(golden, name):
    K, H, W, Hf, Wf = (int(v) for v in golden[f"masks_{name}_shape"])
    masks = np.unpackbits(golden[f"masks_{name}_bits"], axis=1)[:, :H * W].reshape(K, H, W).astype(bool)
    return masks, (Hf, Wf), golden[f"levels_{name}"]


def random_masks(seed, K, H, W):
    rng = np.random.default_rng(seed)
    m = rng.random((K, H, W)) < 0.3
    m[0, H // 4:H // 2 + 1, W // 4:W // 2 + 1] = True
    return m


@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_ref_resize_equals_pillow(src, dst):
    Image = pytest.importorskip("PIL.Image")
    masks = np.concatenate([random_masks(1, 2, *src), np.zeros((1,) + src, bool), np.ones((1,) + src, bool)])
    want = np.stack([np.array(Image.fromarray(np.where(m, 0, 128).astype(np.uint8)).resize((dst[1], dst[0]))).clip(0, 128) for m in masks])
    assert np.array_equal(G.mask_levels(masks, dst), want)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_ref_and_cpu_path_equal_the_golden_pillow_levels(golden, name):
    from gapartnet_amd.misc import grounding
    masks, size, want = golden_masks(golden, name)
    assert np.array_equal(G.mask_levels(masks, size), want)
    assert np.array_equal(grounding.resize_masks(torch.from_numpy(masks), size).numpy(), want)
    assert np.array_equal(grounding.resize_masks(torch.from_numpy(masks.astype(np.uint8) * 7), size).numpy(), want)
    assert want.min() == 0 and want.max() == 128


def test_ref_and_cpu_path_equal_the_golden_sklearn_predictions(golden):
    from gapartnet_amd.misc import grounding
    bank, labels, q = golden["knn_bank"], golden["knn_labels"], golden["knn_queries"]
    idx, d2, votes, label, _ = G.knn(q, bank, labels, 5, 10)
    assert np.array_equal(idx, golden["knn_index"]) and np.array_equal(label, golden["knn_pred"])
    assert np.allclose(np.sqrt(d2), golden["knn_dist"], rtol=1e-5, atol=0)
    g = grounding.PartGrounder(torch.from_numpy(bank), torch.from_numpy(labels), k=5, n_classes=10)
    got = g.kneighbors(torch.from_numpy(q))
    assert np.array_equal(got["index"].numpy(), idx) and np.array_equal(got["votes"].numpy(), votes)
    assert np.array_equal(g.predict(torch.from_numpy(q)).numpy(), golden["knn_pred"])
    assert got["index"].dtype == torch.int32 and got["d2"].dtype == torch.float32 and got["label"].dtype == torch.int32


def test_cpu_path_equals_ref_on_resize_pool_and_ties():
    from gapartnet_amd.misc import grounding
    for (src, dst) in SHAPES[:5]:
        masks = random_masks(2, 3, *src)
        assert np.array_equal(grounding.resize_masks(torch.from_numpy(masks), dst).numpy(), G.mask_levels(masks, dst)), (src, dst)
    rng = np.random.default_rng(3)
    fea = rng.normal(size=(2, 16, 12, 7)).astype(np.float32)
    masks = random_masks(4, 5, 37, 53)
    view = np.array([0, 1, 1, 0, 1])
    levels = G.mask_levels(masks, (16, 12))
    got = grounding.mask_features(torch.from_numpy(fea), torch.from_numpy(masks), view).numpy()
    want = G.mask_pool(fea, levels, view)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))
    # small integers: exact distances, duplicated rows, an equidistant 5th and 6th neighbour, a 2-2-1 vote
    bank = np.array([[0, 0], [1, 0], [1, 0], [0, 2], [2, 0], [0, -2], [5, 5], [0, 3]], dtype=np.float32)
    labels = np.array([3, 3, 1, 1, 2, 0, 4, 4])
    g = grounding.PartGrounder(torch.from_numpy(bank), torch.from_numpy(labels), k=5, n_classes=6)
    got = g.kneighbors(torch.zeros(1, 2))
    assert got["index"].tolist() == [[0, 1, 2, 3, 4]] and got["d2"].tolist() == [[0.0, 1.0, 1.0, 4.0, 4.0]]
    assert got["votes"].tolist() == [[0, 2, 1, 2, 0, 0]] and got["label"].tolist() == [1]
    idx, d2, votes, label, _ = G.knn(np.zeros((1, 2)), bank, labels, 5, 6)
    assert idx.tolist() == [[0, 1, 2, 3, 4]] and label.tolist() == [1]
    out = g.label_masks(torch.zeros(4, 4, 2), torch.ones(2, 9, 9, dtype=torch.bool))
    assert out["label"].tolist() == [1, 1] and out["features"].shape == (2, 2) and out["label"].dtype == torch.int64


def test_load_feature_bank_round_trips(tmp_path):
    from gapartnet_amd.misc import grounding
    rng = np.random.default_rng(5)
    feas = rng.normal(size=(9, 4)).astype(np.float32)
    data = {"feas": [row for row in feas], "cat_ids": [str(i % 3) for i in range(9)], "part_ids": list(range(9)),
            "obj_codes": ["x"] * 9, "splits": ["train", "test", "train", "val", "train", "train", "test", "train", "val"]}
    path = tmp_path / "bank.npy"
    np.save(path, data, allow_pickle=True)
    keep = np.array(data["splits"]) == "train"
    f, lab = grounding.load_feature_bank(str(path))
    assert f.dtype == torch.float32 and lab.dtype == torch.int64
    assert np.array_equal(f.numpy(), feas[keep]) and lab.tolist() == [i % 3 for i in range(9) if keep[i]]
    f, lab = grounding.load_feature_bank(str(path), split=None)
    assert np.array_equal(f.numpy(), feas) and lab.tolist() == [i % 3 for i in range(9)]
    f, lab = grounding.load_feature_bank(str(path), split="val")
    assert f.shape == (2, 4) and lab.tolist() == [0, 2]
    np.savez(tmp_path / "bank.npz", feas=feas, cat_ids=np.arange(9) % 3)
    f, lab = grounding.load_feature_bank(str(tmp_path / "bank.npz"))
    assert np.array_equal(f.numpy(), feas) and lab.tolist() == [i % 3 for i in range(9)]
    np.save(tmp_path / "bad.npy", {"feas": feas}, allow_pickle=True)
    with pytest.raises(ValueError):
        grounding.load_feature_bank(str(tmp_path / "bad.npy"))


def test_argument_errors_on_the_cpu():
    from gapartnet_amd import _C
    from gapartnet_amd.misc import grounding
    bank, lab = torch.zeros(6, 3), torch.tensor([0, 1, 2, 3, 4, 5])
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank[:4], lab[:4], k=5)
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank, lab, k=5, n_classes=5)
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank, -lab, k=5)
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank, lab, k=0)
    with pytest.raises(_C.GpnError):
        grounding.resize_masks(torch.zeros(2, 8, 8), (4, 4))  # float masks
    with pytest.raises(_C.GpnError):
        grounding.mask_features(torch.zeros(2, 4, 4, 3), torch.zeros(3, 8, 8, dtype=torch.bool))  # two maps, no mask_view
    with pytest.raises(_C.GpnError):
        grounding.mask_features(torch.zeros(2, 4, 4, 3), torch.zeros(3, 8, 8, dtype=torch.bool), [0, 1, 2])
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank, lab, k=5).predict(torch.zeros(2, 4))


@pytest.mark.parametrize("extra,needle", [
    (["--bank", "bank.npy"], "--features"),
    (["--features", "f.npy"], "--bank"),
    (["--bank", "bank.npy", "--features", "f.npy", "g.npy"], "one feature map per"),
])
def test_cli_argument_errors(tmp_path, capsys, extra, needle):
    from gapartnet_amd import inference
    argv = ["--ckpt", str(tmp_path / "none.ckpt"), "--depth", str(tmp_path / "d.npy"), "--intrinsics", str(tmp_path / "k.npy"),
            "--masks", str(tmp_path / "m.npz"), "--out", str(tmp_path / "out")] + extra
    with pytest.raises(SystemExit) as e:
        inference.main(argv)
    assert e.value.code == 2 and needle in capsys.readouterr().err


def test_command_line_labels_class_agnostic_masks(tmp_path):
    """--bank / --features next to --depth / --masks on CPU tensors: a masks file without `labels` is labelled by the bank, one
    with labels is left alone; the output carries the labels and the votes PartGrounder gives"""
    from PIL import Image
    from gapartnet_amd import backend, inference
    from gapartnet_amd.misc import grounding
    from oracle import torch_ops
    from tests import frame_ref as F
    from tests import inference_ref as R
    from tests import pipeline_runner as PR
    H, W = 64, 88
    a, c = (x.numpy() for x in R.raw_clouds(4000))
    depth, rgb, K = F.frames_from_clouds([a, c], H, W)
    rng = np.random.RandomState(6)
    masks = np.zeros((2, 3, H, W), bool)
    for v in range(2):
        for j in range(3):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            masks[v, j, y0:y0 + H // 2, x0:x0 + W // 2] = True
    feas = rng.normal(size=(2, 10, 12, 8)).astype(np.float32)
    bank = {"feas": rng.normal(size=(40, 8)).astype(np.float32), "cat_ids": [str(v) for v in rng.randint(1, 4, size=40)],
            "splits": ["train"] * 30 + ["test"] * 10}
    np.save(tmp_path / "bank.npy", bank, allow_pickle=True)
    given = np.array([2, 1, 3])
    np.savez(tmp_path / "m0.npz", masks=masks[0])
    np.savez(tmp_path / "m1.npz", masks=masks[1], labels=given)
    for v in range(2):
        np.save(tmp_path / f"d{v}.npy", depth[v])
        np.save(tmp_path / f"f{v}.npy", feas[v])
        np.save(tmp_path / f"K{v}.npy", K[v])
        Image.fromarray(rgb[v]).save(tmp_path / f"i{v}.png")
    p = lambda *names: [str(tmp_path / n) for n in names]  # noqa: E731
    with backend.using(torch_ops):
        model = PR.build_model(torch.device("cpu")).eval()
        ckpt = tmp_path / "random.ckpt"
        torch.save({"state_dict": model.state_dict(), "hyper_parameters": dict(model.hparams)}, ckpt)
        rc = inference.main(["--ckpt", str(ckpt), "--depth", *p("d0.npy", "d1.npy"), "--rgb", *p("i0.png", "i1.png"), "--intrinsics",
                             *p("K0.npy", "K1.npy"), "--masks", *p("m0.npz", "m1.npz"), "--bank", str(tmp_path / "bank.npy"), "--features",
                             *p("f0.npy", "f1.npy"), "--presample", "1", "--num_points", "512", "--out", str(tmp_path / "out"), "--device", "cpu"])
    assert rc == 0
    g = grounding.PartGrounder(*grounding.load_feature_bank(str(tmp_path / "bank.npy")))
    assert g.feats.shape == (30, 8)
    want = g.label_masks(torch.from_numpy(feas[0]), torch.from_numpy(masks[0]))
    got0, got1 = np.load(tmp_path / "out" / "d0.npz"), np.load(tmp_path / "out" / "d1.npz")
    assert np.array_equal(got0["mask_label"], want["label"].numpy()) and np.array_equal(got0["mask_label_votes"], want["votes"].numpy())
    assert np.array_equal(got0["proposal_classes"], want["label"].numpy()) and got0["mask_label_votes"].sum(1).tolist() == [5, 5, 5]
    assert np.array_equal(got1["mask_label"], given) and "mask_label_votes" not in got1.files


def test_cli_refuses_a_bank_without_masks(tmp_path, capsys):
    from gapartnet_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main(["--ckpt", "x", "--depth", "d.npy", "--intrinsics", "k.npy", "--out", str(tmp_path), "--bank", "b.npy", "--features",
                        "f.npy"])
    assert e.value.code == 2 and "--masks" in capsys.readouterr().err
