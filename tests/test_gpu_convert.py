"""Rendered views -> training scenes on the GPU (include/gpn.h section VP, gapartnet_amd/dataset/convert_rendered.py) against the
reference's own run (tests/golden/convert_views.npz), the numpy restatement (tests/convert_ref.py) and the per-view FPS entry
point: integers exact, float32 outputs and scale_param bit-equal, meta / gt text byte-equal."""
import os

import numpy as np
import pytest
import torch

from tests import convert_ref as R
from tests import render_views as RV

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("rgb", "depth", "sem", "ins", "npcs", "K")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "convert_views.npz"))


def _stack(views):
    return [np.stack([v[k] for v in views]) for k in KEYS]


def _golden_views(golden):
    names = [str(n) for n in golden["names"]]
    return names, [{k: golden[f"{n}/in_{k}"] for k in KEYS} for n in names]


def _assert_same(res, status, arrays, scale, gt):
    assert res.status == status
    if status != R.OK:
        assert res.arrays is None
        return
    for got, want in zip(res.arrays, arrays):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    assert np.array_equal(res.scale_param.view(np.uint8), scale.view(np.uint8))
    assert R.meta_text(res.scale_param) == R.meta_text(scale)
    assert R.gt_text(res.gt) == R.gt_text(gt)


def test_golden_views_match_the_reference(cuda, golden):
    from gapartnet_amd.dataset.convert_rendered import convert_views
    names, views = _golden_views(golden)
    m = int(golden["num_points"])
    written = set(str(n) for n in golden["written"])
    for max_groups in (0, 1):  # the cooperative multi-workgroup form and the wait-free form
        results = convert_views(*_stack(views), m, device=cuda, max_groups=max_groups)
        for name, v, res in zip(names, views, results):
            if int(golden[f"{name}/ret"]) == -1:
                assert res.status == R.TOO_FEW
                continue
            assert res.status == R.OK, name
            if name not in written:  # (outside every category: the driver skipped it)
                _assert_same(res, *R.convert_view(*[v[k] for k in KEYS], m))
                continue
            for i in range(6):
                want = golden[f"{name}/out_pth{i}"]
                assert res.arrays[i].dtype == want.dtype and np.array_equal(res.arrays[i], want), (name, i)
            assert R.meta_text(res.scale_param) == bytes(golden[f"{name}/out_meta"]), name
            assert R.gt_text(res.gt) == bytes(golden[f"{name}/out_gt"]), name


def test_bad_views_get_statuses_and_the_batch_goes_on(cuda):
    from gapartnet_amd import hip_ops
    from gapartnet_amd.dataset.convert_rendered import convert_views, VIEW_INSTANCE_BOUND, VIEW_LABEL_MISMATCH
    assert hip_ops.view_max_instance_ids() <= 5000
    kinds = ["plain", "mismatch", "big_id", "too_few", "holes", "exact"]
    views = [RV.make_view(k, seed=i) for i, k in enumerate(kinds)]
    results = convert_views(*_stack(views), 512, device=cuda)
    assert [r.status for r in results] == [R.OK, VIEW_LABEL_MISMATCH, VIEW_INSTANCE_BOUND, R.TOO_FEW, R.OK, R.OK]
    for v, r in zip(views, results):
        if r.status == R.OK:
            _assert_same(r, *R.convert_view(*[v[k] for k in KEYS], 512))


def test_float64_depth_is_used_exactly(cuda):
    from gapartnet_amd.dataset.convert_rendered import convert_views
    v = RV.make_view("plain", seed=9)
    v["depth"] = v["depth"].astype(np.float64) + 1e-9  # not representable in float32
    res = convert_views(*_stack([v]), 512, device=cuda)[0]
    _assert_same(res, *R.convert_view(*[v[k] for k in KEYS], 512))


def _gpu_fps(cuda):
    from gapartnet_amd import hip_ops

    def fps(xyz32, m):
        return hip_ops.pn2_furthest_point_sampling(torch.from_numpy(xyz32[None]).to(cuda), m)[0].cpu().numpy().astype(np.int64)
    return fps


@pytest.mark.parametrize("max_groups", [0, 1])
def test_ragged_fps_equals_per_view_fps(cuda, max_groups):
    from gapartnet_amd import hip_ops
    rng = np.random.default_rng(3)
    m = 700
    sizes = [300, 700, 701, 1024, 5000, 65535, 65536, 120000, 640000]
    n_max = max(sizes)
    xyz = np.zeros((len(sizes) + 1, n_max, 3), np.float32)
    for i, n in enumerate(sizes):
        xyz[i, :n] = rng.standard_normal((n, 3)).astype(np.float32)
    # the tie geometry: a symmetric grid on a plane (many exactly equal distances)
    g = np.stack(np.meshgrid(np.arange(-40, 40), np.arange(-30, 30), indexing="xy"), -1).reshape(-1, 2).astype(np.float32)
    xyz[len(sizes), :len(g), :2] = g
    counts = np.array(sizes + [len(g)], np.int32)
    idx, status = hip_ops.view_fps_ragged(torch.from_numpy(xyz).to(cuda), torch.from_numpy(counts).to(cuda), m, max_groups)
    idx, status = idx.cpu().numpy(), status.cpu().numpy()
    fps = _gpu_fps(cuda)
    for v, n in enumerate(counts):
        if n < m:
            assert status[v] == R.TOO_FEW
        elif n == m:
            assert status[v] == R.OK and np.array_equal(idx[v], np.arange(m))
        else:
            assert status[v] == R.OK
            assert np.array_equal(idx[v], fps(np.ascontiguousarray(xyz[v, :n]), m)), (v, int(n))


def test_full_size_views_match_the_restatement(cuda):
    from gapartnet_amd.dataset.convert_rendered import convert_views
    views = [RV.full_size_view(s) for s in range(8)]
    results = convert_views(*_stack(views), 20000, device=cuda)
    fps = _gpu_fps(cuda)
    for v, r in zip(views, results):
        _assert_same(r, *R.convert_view(*[v[k] for k in KEYS], 20000, fps=fps))


def _write_renders(root, golden):
    names, views = _golden_views(golden)
    for n, v in zip(names, views):
        RV.write_view(root, n, v)
    RV.write_view(root, "Oven_0007_00_000", RV.make_view("mismatch", seed=7))
    return names


def test_cli_end_to_end_and_training(cuda, golden, tmp_path):
    from gapartnet_amd.dataset import convert_rendered as CR
    data = str(tmp_path / "rendered")
    _write_renders(data, golden)
    outs = []
    for run in (0, 1):
        save = str(tmp_path / f"out{run}")
        CR.main(["--data_path", data, "--save_path", save, "--num_points", str(int(golden["num_points"])), "--batch", "3",
                 "--workers", "4", "--log", str(tmp_path / f"log{run}.txt")])
        outs.append(save)
    written = sorted(str(n) for n in golden["written"])
    for save in outs:
        assert sorted(f[:-4] for f in os.listdir(os.path.join(save, "pth"))) == written  # the mismatch view: no files
        for name in written:
            arrays = torch.load(os.path.join(save, "pth", name + ".pth"), weights_only=False)
            for i in range(6):
                want = golden[f"{name}/out_pth{i}"]
                assert arrays[i].dtype == want.dtype and np.array_equal(arrays[i], want), (name, i)
            for sub in ("meta", "gt"):
                with open(os.path.join(save, sub, name + ".txt"), "rb") as fh:
                    assert fh.read() == bytes(golden[f"{name}/out_{sub}"]), (name, sub)
    log = open(tmp_path / "log0.txt").read()
    assert "Error in Oven_0007_00_000 Oven, semantic and instance labels do not match!" in log
    assert log.replace("Sampling 0/1 Oven_0007_00_000\nError in Oven_0007_00_000 Oven, semantic and instance labels do not "
                       "match!\n", "").replace("Oven : 1", "Oven : 0") == bytes(golden["log"]).decode()
    assert open(tmp_path / "log1.txt").read() == log  # two runs, identical outputs
    for name in written:
        for sub in ("meta", "gt"):
            assert open(os.path.join(outs[0], sub, name + ".txt"), "rb").read() == \
                open(os.path.join(outs[1], sub, name + ".txt"), "rb").read()

    # the existing loader reads the files and one training step runs on them
    from gapartnet_amd.dataset.gapartnet import GAPartNetDataset
    from gapartnet_amd.smoke import make_model
    ds = GAPartNetDataset(os.path.join(outs[0], "pth"), max_points=512, voxel_size=(0.01, 0.01, 0.01))
    assert len(ds) == len(written)
    scenes = [ds[i] for i in range(len(ds)) if bool((ds[i].instance_labels >= 0).any())]
    model = make_model((0, 0), seed=0).to(cuda)
    model.train()
    batch = [s.to(cuda) for s in scenes[:2]]
    loss = model.training_step(batch, 0)
    loss.backward()
    assert torch.isfinite(loss).item()
