"""The opt-in octree-cell sampler (include/gpn.h section GS) on the host: ``inference.grid_sample_rows`` against the independent
restatement (tests/grid_ref.py), the properties the contract promises, and ``sampler="grid"`` through ``prepare_clouds``,
``prepare_frames``, ``PartPredictor`` and the command line on CPU tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gapartnet_amd import backend, inference
from tests import frame_ref as F
from tests import grid_ref as G
from tests import inference_ref as R
from tests import pipeline_runner as PR

JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])


def _same(xyz, m, seed=0, hash_bits=32):
    rows, level = inference.grid_sample_rows(xyz, m, seed, hash_bits)
    want, want_level = G.grid_sample(xyz, m, seed, hash_bits)
    assert level == want_level and rows.tolist() == want, (len(xyz), m, seed, hash_bits, level, want_level)
    assert rows.dtype == np.int64
    return rows, level


def test_random_clouds_every_m():
    rng = np.random.RandomState(0)
    levels = set()
    for n in list(range(2, 40)) + [63, 64, 65, 130, 257, 400]:
        xyz = (rng.randn(n, 3) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
        for m in range(1, n):
            rows, level = _same(xyz, m, seed=n * 7 + m)
            levels.add(level)
            assert len(rows) == m and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    assert levels >= {0, 1, 2, 3}


def test_small_m_forces_level_zero():
    rng = np.random.RandomState(1)
    xyz = rng.randn(300, 3).astype(np.float32)   # all eight octants are occupied: C_1 = 8
    for m in range(1, 8):
        assert _same(xyz, m, seed=m)[1] == 0


def test_every_level_is_reached():
    rng = np.random.RandomState(2)
    seen = set()
    for L in range(11):
        xyz = G.level_cloud(rng, L)
        rows, level = _same(xyz, 12 if L else 7, seed=L)   # (level 0 has one cell, and the 50 points fill all 8 octants)
        seen.add(level)
        assert level == L, (L, level)
    assert seen == set(range(11))


@pytest.mark.parametrize("seed,hash_bits", [(0, 32), (0xffffffff, 32), (0, 1), (0xffffffff, 4)])
def test_degenerate_families_seeds_and_hash_ties(seed, hash_bits):
    rng = np.random.RandomState(3)
    fam = G.families(rng)
    levels = {}
    for name, (xyz, m) in fam.items():
        rows, levels[name] = _same(xyz, m, seed, hash_bits)
        assert len(set(rows.tolist())) == m
    assert levels["duplicates_L10"] == 10 and levels["duplicates_fill"] == 10 and levels["all_equal"] == 10
    assert levels["overflow"] == 10, "every code is 0: one cell at every level"
    for n in (90, 200):   # ties at every rank: hash_bits 1 leaves two hash values
        xyz = rng.randn(n, 3).astype(np.float32)
        for m in (9, n // 2, n - 1):
            _same(xyz, m, seed, hash_bits)


def test_a_cloud_does_not_depend_on_its_neighbours():
    rng = np.random.RandomState(4)
    clouds = [rng.randn(n, 6).astype(np.float32) for n in (300, 90, 150)]
    m = 64
    prep = inference.prepare_clouds([torch.from_numpy(c) for c in clouds], m, sampler="grid", seed=[5, 6, 7])
    for s, c in enumerate(clouds):
        alone = inference.prepare_clouds([torch.from_numpy(c)], m, sampler="grid", seed=[5 + s])
        assert torch.equal(alone.sample_rows, prep.sample_rows[s * m:(s + 1) * m]) and int(alone.level[0]) == int(prep.level[s])
        assert torch.equal(alone.points, prep.points[s * m:(s + 1) * m])


def test_coverage_bound():
    """every point lies within sqrt(3) e / 2^L* + e 2^-18 of a sample: it shares a level-L* cell with a stage-A sample"""
    rng = np.random.RandomState(5)
    clouds = [rng.randn(2000, 3), rng.rand(1500, 3) * [4, 1, 0.01], G.level_cloud(rng, 6, 40, 20), G.level_cloud(rng, 3, 9, 60)]
    for xyz in clouds:
        xyz = xyz.astype(np.float32)
        for m in (16, 100, 700):
            rows, level = inference.grid_sample_rows(xyz, m, seed=1)
            p = xyz.astype(np.float64)
            e = float((p.max(0) - p.min(0)).max())
            d = np.sqrt(((p[:, None, :] - p[None, rows, :]) ** 2).sum(-1)).min(1)
            assert d.max() <= math.sqrt(3) * e / 2 ** level + e * 2.0 ** -18, (m, level, d.max())


def test_prepare_clouds_with_the_grid_sampler():
    rng = np.random.RandomState(6)
    clouds = [rng.randn(500, 6).astype(np.float32), rng.randn(200, 6).astype(np.float32), np.zeros((0, 6), np.float32),
              np.ones((30, 6), np.float32), rng.randn(128, 6).astype(np.float32)]
    clouds[1][[0, 50, 199], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    m = 128
    tens = [torch.from_numpy(c) for c in clouds]
    prep = inference.prepare_clouds(tens, num_points=m, sampler="grid", seed=9)
    assert prep.status.tolist() == [R.OK, R.OK, R.EMPTY, R.DEGENERATE, R.OK] and prep.counts.tolist() == [128, 128, 0, 0, 128]
    first = 0
    want_level = []
    for s, c in enumerate(clouds):
        valid = np.nonzero(np.isfinite(c[:, :3]).all(1))[0]
        if len(valid) > m:
            picked, level = G.grid_sample(c[valid, :3], m, seed=9 + s)
            rows = valid[picked]
        else:
            rows, level = valid, -1
        want_level.append(level)
        if prep.counts[s] == 0:
            continue
        got = prep.sample_rows[first:first + m].numpy()
        assert np.array_equal(got, rows), s
        p = c[rows, :3].astype(np.float64)           # centre and radius over the SAMPLED rows
        ctr = (p.max(0) + p.min(0)) / 2
        dd = p - ctr
        r = np.sqrt(((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).max())
        assert np.array_equal(prep.scale[s].numpy(), np.concatenate([[r], ctr]))
        assert np.array_equal(prep.points[first:first + m, :3].numpy(), (dd / r).astype(np.float32))
        assert np.array_equal(prep.points[first:first + m, 3:].numpy(), c[rows, 3:])
        first += m
    assert prep.level.tolist() == want_level and want_level[0] >= 0 and want_level[4] == -1
    # the default is what it was: bit-equal with and without the argument, and no level
    a, b = inference.prepare_clouds(tens, m), inference.prepare_clouds(tens, m, sampler="fps")
    for f in ("points", "counts", "sample_rows", "scale", "status"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.level is None and b.level is None and not torch.equal(a.sample_rows, prep.sample_rows)
    with pytest.raises(ValueError):
        inference.prepare_clouds(tens, m, sampler="octree")
    with pytest.raises(ValueError):
        inference.PartPredictor(torch.nn.Identity(), sampler="random")
    with pytest.raises(ValueError):
        inference.prepare_clouds(tens, m, sampler="grid", seed=[1, 2])


def test_prepare_frames_with_the_grid_sampler_equals_prepare_clouds_on_the_masked_rows():
    rng = np.random.RandomState(7)
    V, H, W, m, pre = 3, 24, 32, 64, 4
    depth = (rng.rand(V, H, W) * 2 + 0.5).astype(np.float32)
    depth[rng.rand(V, H, W) < 0.2] = 0
    depth[1, 3:, :] = 0                                     # frame 1: 96 pixels at most, fewer than cap; frame 2 empty
    depth[2] = 0
    rgb = rng.randint(0, 256, size=(V, H, W, 3)).astype(np.uint8)
    K = np.array([[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1]])
    seeds = [11, 0xffffffff, 3]
    prep = inference.prepare_frames(torch.from_numpy(depth), torch.from_numpy(rgb), K, num_points=m, presample=pre, seed=seeds,
                                    sampler="grid")
    masked = []
    for v in range(V):
        rows, valid = F.backproject_np(depth[v], rgb[v], K, flip=False)
        masked.append(torch.from_numpy(F.masked_rows(rows, F.select_np(valid, seeds[v], pre * m))))
    want = inference.prepare_clouds(masked, m, sampler="grid", seed=seeds)
    for f in ("points", "counts", "sample_rows", "scale", "status", "level"):
        assert torch.equal(getattr(prep, f), getattr(want, f)), f
    assert prep.status.tolist() == [R.OK, R.OK, R.EMPTY] and prep.level[0] >= 0 and prep.level[2] == -1
    plain = inference.prepare_frames(torch.from_numpy(depth), torch.from_numpy(rgb), K, num_points=m, presample=pre, seed=seeds)
    assert plain.level is None


@pytest.fixture(scope="module")
def oracle_model():
    from oracle import torch_ops
    with backend.using(torch_ops):
        model = PR.build_model(torch.device("cpu")).eval()
        model._current_epoch = 10
        model.revoxelize_jitter = tuple(torch.tensor(j) for j in JITTER)
        yield model


def test_part_predictor_with_the_grid_sampler(oracle_model):
    """the predictor's conventions with a cloud that keeps every row (FEW), an empty one and one of exactly num_points rows"""
    a, c = R.raw_clouds()
    m = 1024
    few, empty, exact = a[:700].clone(), torch.full((40, 6), float("nan")), c[:m].clone()
    assert a.shape[0] > m
    predictor = inference.PartPredictor(oracle_model, num_points=m, max_iters=16, sampler="grid")
    clouds = [a, few, empty, exact]
    preds = predictor.predict(clouds, picks=R.size_picks)
    assert [p.status for p in preds] == [R.OK, R.OK, R.EMPTY, R.OK]
    prep = inference.prepare_clouds(clouds, m, sampler="grid")
    assert prep.level.tolist()[1:] == [-1, -1, -1] and int(prep.level[0]) >= 0
    assert [int(p.sample_rows.shape[0]) for p in preds] == [m, 700, 0, m]
    assert torch.equal(preds[0].sample_rows, prep.sample_rows[:m]) and bool((preds[0].sample_rows[1:] > preds[0].sample_rows[:-1]).all())
    assert torch.equal(preds[1].sample_rows, torch.arange(700)) and torch.equal(preds[3].sample_rows, torch.arange(m))
    for cloud, p in zip(clouds, preds):
        n = cloud.shape[0]
        assert p.sem.shape == (n,) and p.instance.shape == (n,) and p.npcs.shape == (n, 3)
        if p.status != R.OK:
            assert bool((p.sem == -1).all()) and p.bbox.shape[0] == 0
            continue
        assert bool((p.sem >= 0).all()) and torch.equal(p.sem[p.sample_rows], p.sampled_sem)
        inside = p.instance >= 0
        assert torch.equal(p.proposal_classes[p.instance[inside]], p.sem[inside])
    # the clouds that are not sampled do not see the sampler
    fps = inference.PartPredictor(oracle_model, num_points=m, max_iters=16).predict([few, exact], picks=R.size_picks)
    grid = predictor.predict([few, exact], picks=R.size_picks)
    for p, q in zip(fps, grid):
        for f in ("sem", "instance", "npcs", "bbox", "sample_rows"):
            assert torch.equal(getattr(p, f), getattr(q, f)), f


def test_command_line_with_the_grid_sampler(oracle_model, tmp_path):
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": oracle_model.state_dict(), "hyper_parameters": dict(oracle_model.hparams)}, ckpt)
    a, _ = R.raw_clouds()
    np.save(tmp_path / "first.npy", a.numpy())
    out = tmp_path / "out"
    args = ["--ckpt", str(ckpt), "--input", str(tmp_path / "first.npy"), "--out", str(out), "--num_points", "512", "--device", "cpu"]
    assert inference.main(args + ["--sampler", "grid"]) == 0
    got = np.load(out / "first.npz")
    want = inference.prepare_clouds([a], 512, sampler="grid")
    assert np.array_equal(got["sample_rows"], want.sample_rows.numpy()) and int(got["status"]) == R.OK
    assert got["sem"].shape == (a.shape[0],)
    with pytest.raises(SystemExit):
        inference.main(args + ["--sampler", "voxel"])


def test_symbols_are_exported_and_registered():
    from gapartnet_amd import _C, hip_ops
    lib = _C.lib()
    names = {lib.gpn_entry_point_name(i).decode() for i in range(lib.gpn_num_entry_points())}
    for sym in ("gpn_cloud_grid_sample_ws_bytes", "gpn_cloud_grid_sample"):
        assert sym in names and hasattr(lib, sym), sym
    assert callable(hip_ops.cloud_grid_sample) and hip_ops.SAMPLERS == inference.SAMPLERS == ("fps", "grid")
    ws = lib.gpn_cloud_grid_sample_ws_bytes
    assert ws(ctypes.c_int(0), ctypes.c_int64(100)) == 0 and ws(ctypes.c_int(2), ctypes.c_int64(0)) == 0
    assert ws(ctypes.c_int(2), ctypes.c_int64(5000)) > 2 * 5000 * (8 + 8 + 4 + 4 + 1 + 1)
    with open(_C.CSRC + "/../../include/gpn.h") as fh:
        header = fh.read()
    assert "gpn_cloud_grid_sample(" in header and " GS - " in header
