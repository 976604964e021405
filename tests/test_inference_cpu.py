"""Label-free inference without a GPU: the numpy restatement of the raw-cloud front / back end (tests/inference_ref.py) against the
reference's own results (tests/golden/cloud_ball_space.npz), ``GAPartNet.forward`` over the CPU oracle operators against the
validation step and a torch formulation, ``prepare_clouds`` / ``PartPredictor`` / the command line on CPU tensors."""
import os

import numpy as np
import pytest
import torch

from gapartnet_amd import backend, inference
from tests import inference_ref as R
from tests import pipeline_runner as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_ball_space.npz")
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---------------------------------------------------------------------------------------------------- restatement vs reference
def test_restatement_reproduces_the_references_ball_space_bit_for_bit(gold):
    for name in gold["names"]:
        xyz = gold[f"{name}/in"]
        assert np.array_equal(xyz, xyz.astype(np.float32).astype(np.float64))  # float32 values: what the library is given
        normalized, radius, center = R.ball_space(xyz)
        assert np.array_equal(center, gold[f"{name}/center"]), name
        assert radius == gold[f"{name}/radius"], name
        assert np.array_equal(normalized, gold[f"{name}/normalized"]), name
        # ... and through the whole pack / sample / finish restatement (fewer points than m: every point kept, in order)
        cloud = np.concatenate([xyz, np.arange(xyz.shape[0] * 3).reshape(-1, 3)], 1).astype(np.float32)
        got = R.prepare_cloud(cloud, 256)
        assert got["status"] == R.OK and np.array_equal(got["sample_rows"], np.arange(xyz.shape[0]))
        assert np.array_equal(got["scale"], np.concatenate([[gold[f"{name}/radius"]], gold[f"{name}/center"]]))
        assert np.array_equal(got["out"][:, :3], gold[f"{name}/normalized"].astype(np.float32))
        assert np.array_equal(got["out"][:, 3:], cloud[:, 3:])


def test_read_obj_points_equals_the_references_reader(gold, tmp_path):
    path = tmp_path / "scan.obj"
    path.write_bytes(gold["obj_text"].tobytes())
    got = inference.read_obj_points(str(path))
    assert got.dtype == np.float64 and np.array_equal(got, gold["obj_points"])
    assert got.shape == (4, 6)  # the `v` line behind the first `vt` is not read


def test_restatement_samples_skips_and_flags():
    rng = np.random.RandomState(0)
    cloud = rng.randn(300, 5).astype(np.float32)
    cloud[[0, 17, 299], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    got = R.prepare_cloud(cloud, 64)
    rows = R.valid_rows(cloud)
    assert rows.shape[0] == 297 and got["count"] == 297 and got["status"] == R.OK
    assert np.array_equal(got["sample_rows"], rows[R.oracle_fps(cloud[rows, :3], 64)])
    assert np.abs(np.linalg.norm(got["out"][:, :3].astype(np.float64), axis=1).max() - 1) < 1e-6
    assert R.prepare_cloud(np.full((5, 3), np.nan, np.float32), 4)["status"] == R.EMPTY
    assert R.prepare_cloud(np.zeros((0, 3), np.float32), 4)["status"] == R.EMPTY
    assert R.prepare_cloud(np.ones((9, 3), np.float32), 4)["status"] == R.DEGENERATE
    assert R.prepare_cloud(np.ones((1, 3), np.float32), 4)["status"] == R.DEGENERATE


def test_restatement_of_nearest_sample_edge_cases():
    g = lambda *v: np.asarray(v, np.float32) / 64  # noqa: E731
    s = np.stack([g(0, 0, 0), g(64, 0, 0), g(0, 0, 0), g(64, 0, 0)])  # duplicated samples
    q = np.stack([g(32, 0, 0), g(64, 0, 0), g(-640, 5, 5), g(33, 1, 1), np.asarray([np.nan, 0, 0], np.float32)])
    nn, d2 = R.nearest(q, s)
    assert nn.tolist() == [0, 1, 0, 1, -1]   # an exact tie goes to the lowest sample; a query equal to a sample finds its first copy
    assert d2[0] == 0.25 and d2[1] == 0 and np.isinf(d2[4])
    nn, d2 = R.nearest(q, np.zeros((0, 3), np.float32))
    assert (nn == -1).all() and np.isinf(d2).all()
    nn, _ = R.nearest(q[:4], s[1:2])  # one sample
    assert nn.tolist() == [0, 0, 0, 0]
    # samples on a plane, on a line, and 49 in one spot with one far away (exact inputs: fp32 == fp64)
    rng = np.random.RandomState(1)
    plane = (rng.randint(-128, 129, size=(50, 3)) / 64).astype(np.float32)
    plane[:, 2] = 0.5
    line = plane.copy()
    line[:, 1] = -0.25
    lump = np.repeat(g(-128, -128, -128)[None], 50, 0) + (rng.randint(0, 2, size=(50, 3)) / 64).astype(np.float32)
    lump[49] = g(128, 128, 128)
    qs = (rng.randint(-128, 129, size=(200, 3)) / 64).astype(np.float32)
    qs[:6] = [g(-640, 0, 0), g(640, 0, 0), g(0, -640, 0), g(0, 640, 0), g(0, 0, -640), g(0, 0, 640)]  # far outside the samples' box
    for samples in (plane, line, lump):
        nn, d2 = R.nearest(qs, samples)
        full = ((qs[:, None, :].astype(np.float64) - samples[None].astype(np.float64)) ** 2).sum(-1)
        assert np.array_equal(d2.astype(np.float64), full.min(1)) and np.array_equal(nn, full.argmin(1))


# ---------------------------------------------------------------------------------------------------- CPU path of prepare_clouds
def test_prepare_clouds_on_cpu_tensors_equals_the_restatement():
    rng = np.random.RandomState(5)
    clouds = [rng.randn(500, 6).astype(np.float32), rng.randn(200, 6).astype(np.float32), np.zeros((0, 6), np.float32),
              np.ones((30, 6), np.float32), rng.randn(128, 6).astype(np.float32)]
    clouds[1][[0, 50, 199], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    m = 128
    prep = inference.prepare_clouds([torch.from_numpy(c) for c in clouds], num_points=m)
    want = [R.prepare_cloud(c, m) for c in clouds]
    assert prep.status.tolist() == [R.OK, R.OK, R.EMPTY, R.DEGENERATE, R.OK]
    assert prep.counts.tolist() == [128, 128, 0, 0, 128]
    ok = [w for w in want if w["status"] == R.OK]
    assert np.array_equal(prep.points.numpy(), np.concatenate([w["out"] for w in ok]))
    assert np.array_equal(prep.sample_rows.numpy(), np.concatenate([w["sample_rows"] for w in ok]))
    for s, w in enumerate(want):
        if w["status"] != R.EMPTY:
            assert np.array_equal(prep.scale[s].numpy(), w["scale"])
    nn = inference.nearest_samples(prep).numpy()
    first = 0
    for s, (c, w) in enumerate(zip(clouds, want)):
        a, b = prep.offsets[s], prep.offsets[s + 1]
        if w["status"] == R.OK:
            assert np.array_equal(nn[a:b], R.nearest(c, c[w["sample_rows"]])[0])
            assert np.array_equal(nn[a:b][w["sample_rows"]] <= np.arange(len(w["sample_rows"])), np.ones(len(w["sample_rows"]), bool))
        else:
            assert (nn[a:b] == -1).all()
    with pytest.raises(ValueError):
        inference.prepare_clouds([torch.zeros(4, 2)])


# ---------------------------------------------------------------------------------------------------- forward over the oracle
@pytest.fixture(scope="module")
def oracle_model():
    from oracle import torch_ops
    with backend.using(torch_ops):
        model = PR.build_model(torch.device("cpu")).eval()
        model._current_epoch = 10
        model.revoxelize_jitter = tuple(torch.tensor(j) for j in JITTER)
        yield model


def test_forward_on_unlabelled_scenes_over_the_oracle(oracle_model):
    model = oracle_model
    scenes = PR.load_scenes(torch.device("cpu"))
    plan_before = (model._prop_plan, list(model._prop_hist))
    got = model(R.unlabelled(scenes))
    assert (model._prop_plan, list(model._prop_hist)) == plan_before and model.sync_free_proposals is True
    assert got[0] == [pc.pc_id for pc in scenes]
    assert got[2] is not None, "the synthetic scenes give proposals"
    # predictions before the proposal stage do not depend on labels
    with torch.no_grad():
        _, seg_val, _ = model.validation_step(PR.load_scenes(torch.device("cpu")), 0, 0)
    model.validation_step_outputs.clear()
    assert torch.equal(got[1].sem_preds, seg_val.sem_preds)
    R.check_forward_against_formulation(got, R.forward_formulation(model, R.unlabelled(scenes)))
    # labels that are present are not read
    with_labels = model(scenes)
    assert torch.equal(with_labels[1].sem_preds, got[1].sem_preds)
    for f in ("sorted_indices", "proposal_offsets", "score_preds", "npcs_preds", "sem_preds"):
        assert torch.equal(getattr(with_labels[2], f), getattr(got[2], f)), f
    assert with_labels[2].instance_labels is None
    # a batch that was collated before, and gradients requested by the caller
    batch = model._collate(R.unlabelled(scenes))
    with torch.enable_grad():
        again = model(batch)
    assert torch.equal(again[2].score_preds, got[2].score_preds) and not again[2].score_preds.requires_grad


# ---------------------------------------------------------------------------------------------------- predictor, command line
FIELDS = {"sem": torch.int64, "instance": torch.int64, "npcs": torch.float32, "proposal_scores": torch.float32,
          "proposal_classes": torch.int64, "bbox": torch.float64, "box_proposal": torch.int64, "scale": torch.float64}


def test_part_predictor_on_cpu_tensors(oracle_model):
    a, c = R.raw_clouds()
    a = a.clone()
    a[[3, 700], [0, 2]] = float("nan")
    b = torch.full((40, 6), float("nan"))  # no valid row: not OK, in the middle of the batch
    predictor = inference.PartPredictor(oracle_model, num_points=1024, max_iters=16)
    preds = predictor.predict([a, b, c], picks=R.size_picks)
    assert [p.status for p in preds] == [R.OK, R.EMPTY, R.OK]
    for cloud, p in zip((a, b, c), preds):
        n = cloud.shape[0]
        for f, dt in FIELDS.items():
            assert getattr(p, f).dtype == dt, f
        assert p.sem.shape == (n,) and p.instance.shape == (n,) and p.npcs.shape == (n, 3)
        P, Q = p.proposal_scores.shape[0], p.bbox.shape[0]
        assert p.proposal_classes.shape == (P,) and p.bbox.shape == (Q, 8, 3) and p.box_proposal.shape == (Q,)
        bad = ~torch.isfinite(cloud[:, :3]).all(1)
        if p.status != R.OK:
            assert P == 0 and Q == 0 and bool((p.sem == -1).all()) and bool((p.instance == -1).all()) and not bool(p.npcs.any())
            continue
        assert bool((p.sem[bad] == -1).all()) and bool((p.instance[bad] == -1).all()) and bool((p.sem[~bad] >= 0).all())
        assert int(p.instance.max()) < max(P, 1) and int(p.instance.min()) >= -1
        assert bool((p.npcs[p.instance < 0] == 0).all())
        assert bool(((p.box_proposal >= 0) & (p.box_proposal < max(P, 1))).all())
        # a sampled row carries its own sample's prediction (its nearest sample is itself, or an earlier copy of the same point)
        assert torch.equal(p.sem[p.sample_rows], p.sampled_sem) and torch.equal(p.npcs[p.sample_rows], p.sampled_npcs)
        # a point of a part sits in that part's class
        inside = p.instance >= 0
        assert torch.equal(p.proposal_classes[p.instance[inside]], p.sem[inside])
    assert sum(p.proposal_scores.shape[0] for p in preds) > 0, "the synthetic clouds give parts"
    # the not-OK cloud leaves the others unchanged: bit for bit against the batch without it, and against each cloud alone.
    # Alone, every field is bit-equal but the scores: torch's CPU sigmoid takes its vector or its scalar path by an element's
    # position in the tensor, and the two differ by one unit in the last place; a score lies in (0, 1), where that unit is at
    # most 2^-24 - so 2^-23 bounds the difference of two such values.
    others = predictor.predict([a, c], picks=R.size_picks)
    every = list(FIELDS) + ["sampled_sem", "sampled_instance", "sampled_npcs", "sample_rows", "bbox_normalised"]
    for p, q in ((preds[0], others[0]), (preds[2], others[1])):
        for f in every:
            assert torch.equal(getattr(p, f), getattr(q, f)), f
    for cloud, p in ((a, preds[0]), (c, preds[2])):
        alone = predictor.predict([cloud], picks=R.size_picks)[0]
        for f in every:
            x, y = getattr(alone, f), getattr(p, f)
            if f == "proposal_scores":
                assert x.shape == y.shape and float((x - y).abs().max()) <= 2.0 ** -23, f
            else:
                assert torch.equal(x, y), f


def test_command_line_writes_the_documented_fields(oracle_model, tmp_path):
    ckpt = tmp_path / "random.ckpt"
    torch.save({"state_dict": oracle_model.state_dict(), "hyper_parameters": dict(oracle_model.hparams)}, ckpt)
    a, c = R.raw_clouds()
    np.save(tmp_path / "first.npy", a.numpy())
    with open(tmp_path / "second.obj", "w") as fh:
        for row in c.numpy().astype(np.float64):
            fh.write("v " + " ".join(repr(float(v)) for v in row) + "\n")
        fh.write("vt 0.0 0.0\nv 1 1 1 1 1 1\n")
    out = tmp_path / "out"
    rc = inference.main(["--ckpt", str(ckpt), "--input", str(tmp_path / "first.npy"), str(tmp_path / "second.obj"), "--out", str(out),
                         "--num_points", "512", "--device", "cpu"])
    assert rc == 0
    for name, cloud in (("first", a), ("second", c)):
        got = np.load(out / f"{name}.npz")
        for f in ("sem", "instance", "npcs", "proposal_scores", "proposal_classes", "bbox", "box_proposal", "scale", "status"):
            assert f in got.files, f
        assert got["sem"].shape == (cloud.shape[0],) and got["npcs"].shape == (cloud.shape[0], 3) and int(got["status"]) == R.OK
    # the .obj cloud went in with the reference's sign flips of y and z: its centre is the mirrored one
    flipped = np.load(out / "second.npz")["scale"]
    plain = inference.prepare_clouds([c], 512).scale[0].numpy()
    assert np.allclose(flipped[[0, 1]], plain[[0, 1]], rtol=1e-6) and np.allclose(flipped[[2, 3]], -plain[[2, 3]], rtol=1e-6)
