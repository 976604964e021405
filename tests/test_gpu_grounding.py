"""The grounding kernels (csrc/ground.hip, include/gpn.h section GR) on the GPU against tests/ground_ref.py: the mask resize byte
for byte, the mask pool to one fp32 rounding, the k-nearest-neighbour vote exactly on integer data (both tie rules) and within
the derived bound of the fp32 expansion on float data, the golden file recorded from Pillow and scikit-learn, and
``predict_frames_with_masks`` with class-agnostic masks end to end."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import ground_ref as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grounding.npz")


def _t(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


# ---- resize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("src,dst", [((96, 128), (50, 50)), ((50, 50), (50, 50)), ((37, 53), (16, 12)), ((8, 8), (50, 50)), ((101, 64), (1, 1))],
                         ids=["down", "identity", "odd", "upscale", "to-one-pixel"])
def test_resize_bytes_equal_ref(cuda, src, dst, K):
    from gapartnet_amd.misc import grounding
    rng = np.random.default_rng(K * 1000 + src[0])
    masks = rng.random((K,) + src) < 0.35
    masks[0, src[0] // 4:src[0] // 2 + 1, src[1] // 3:src[1] // 2 + 1] = True
    if K > 2:
        masks[1], masks[2] = False, True  # an all-zero and an all-one mask
    want = G.mask_levels(masks, dst)
    got = grounding.resize_masks(_t(masks, cuda), dst)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got8 = grounding.resize_masks(_t(masks.astype(np.uint8) * 255, cuda), dst)  # any non-zero byte is a member
    assert np.array_equal(got8.cpu().numpy(), want)
    if K > 2:
        assert (want[1] == 128).all() and (want[2] == 0).all()


# ---- pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 33])
@pytest.mark.parametrize("C", [1, 3, 130, 384])
def test_pool_within_one_rounding_and_batch_independent(cuda, C, K):
    from gapartnet_amd.misc import grounding
    rng = np.random.default_rng(C * 100 + K)
    Hf, Wf = 16, 12
    fea = rng.normal(size=(2, Hf, Wf, C)).astype(np.float32)
    levels = rng.integers(0, 129, size=(K, Hf, Wf)).astype(np.uint8)
    levels[rng.random(levels.shape) < 0.05] = 200  # beyond 128: no weight
    levels[0] = 128 if K > 1 else levels[0]       # an empty mask: every product is a zero
    view = rng.integers(0, 2, size=K)
    want = G.mask_pool(fea, levels, view)
    got_dev = grounding.pool_levels(_t(fea, cuda), _t(levels, cuda), _t(view, cuda))
    got = got_dev.cpu().numpy().astype(np.float64)
    assert got_dev.dtype == torch.float32 and got.shape == (K, C)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))
    if K > 1:
        assert np.all(got[0] == 0.0)
        k = K - 1  # alone, and with only its own map in the call
        alone = grounding.pool_levels(_t(fea[view[k]:view[k] + 1], cuda), _t(levels[k:k + 1], cuda), None)
        assert torch.equal(alone[0], got_dev[k])


# ---- kNN, exact ---------------------------------------------------------------------------------------------------------------------
def _exact_case(Q, M, D, n_classes, seed):
    rng = np.random.default_rng(seed)
    bank = rng.integers(-3, 4, size=(M, D)).astype(np.float32)
    if M >= 6:
        bank[M // 2] = bank[0]  # duplicated rows
        bank[M - 1] = bank[1]
    q = rng.integers(-3, 4, size=(Q, D)).astype(np.float32)
    q[0] = bank[0]
    return q, bank, rng.integers(0, n_classes, size=M)


def _assert_knn_equals_ref(cuda, q, bank, labels, k, n_classes):
    from gapartnet_amd.misc import grounding
    idx, d2, votes, label, _ = G.knn(q, bank, labels, k, n_classes)
    g = grounding.PartGrounder(_t(bank, cuda), _t(labels, cuda), k=k, n_classes=n_classes)
    got = g.kneighbors(_t(q, cuda))
    assert np.array_equal(got["index"].cpu().numpy(), idx)
    assert np.array_equal(got["d2"].cpu().numpy().astype(np.float64), d2)
    assert np.array_equal(got["votes"].cpu().numpy(), votes) and np.array_equal(got["label"].cpu().numpy(), label)
    return got


@pytest.mark.parametrize("Q,M,D,k", [(1, 5, 1, 5), (31, 6, 3, 5), (33, 127, 130, 5), (65, 129, 3, 5), (65, 1000, 130, 5), (1, 1000, 1, 1),
                                     (33, 129, 130, 32), (31, 1000, 3, 32), (65, 32, 1, 32), (2, 70000, 3, 5)])
def test_knn_exact_cases_equal_ref(cuda, Q, M, D, k):
    """integer features: every distance is exact in fp32 and in the oracle, ties are everywhere (D = 1: seven distinct values), so
    both tie rules are pinned; M = 70000 has more tiles than slices (a slice walks two tiles)"""
    q, bank, labels = _exact_case(Q, M, D, 4, seed=Q * 7 + M + D + k)
    _assert_knn_equals_ref(cuda, q, bank, labels, k, 4)


def test_knn_crafted_ties(cuda):
    """duplicated bank rows, an equidistant 5th and 6th neighbour (the lower row wins), a 2-2-1 vote (the smaller class wins)"""
    bank = np.array([[0, 0], [1, 0], [1, 0], [0, 2], [2, 0], [0, -2], [5, 5], [0, 3]], dtype=np.float32)
    labels = np.array([3, 3, 1, 1, 2, 0, 4, 4])
    got = _assert_knn_equals_ref(cuda, np.zeros((1, 2), np.float32), bank, labels, 5, 6)
    assert got["index"].tolist() == [[0, 1, 2, 3, 4]] and got["votes"].tolist() == [[0, 2, 1, 2, 0, 0]] and got["label"].tolist() == [1]
    # the same rows in another order: the equidistant pair swaps with the rows
    perm = np.array([5, 4, 3, 2, 1, 0, 6, 7])
    got = _assert_knn_equals_ref(cuda, np.zeros((1, 2), np.float32), bank[perm], labels[perm], 5, 6)
    assert got["index"].tolist() == [[5, 3, 4, 0, 1]]


# ---- kNN, float ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_case(M, D, Q):
    rng = np.random.default_rng(M + D + Q)
    centres = rng.normal(size=(10, D))
    labels = rng.integers(0, 10, size=M)
    bank = (centres[labels] + 0.7 * rng.normal(size=(M, D))).astype(np.float32)
    q = (centres[rng.integers(0, 10, size=Q)] + 0.7 * rng.normal(size=(Q, D))).astype(np.float32)
    return q, bank, labels, G.knn(q, bank, labels, 6, 10)  # (six neighbours: the gap behind the fifth)


@pytest.mark.parametrize("M,D,Q", [(1000, 130, 37), (2048, 384, 64), (4096, 1024, 48)])
def test_knn_float_cases_within_the_expansion_bound(cuda, M, D, Q):
    """bound = (D + 3) 2^-24 max_b(|q|^2 + |b|^2): the worst-case error of (|q|^2 + |b|^2) - 2 q.b in fp32 - D + 1 roundings of the
    dot product's chain against sum |q_i b_i| <= (|q|^2 + |b|^2) / 2, doubled, the norms' own chains and the two additions.  Derived,
    not measured.  A query whose true 5th / 6th gap exceeds 2 bound is decided: same neighbours, same label."""
    from gapartnet_amd.misc import grounding
    q, bank, labels, (idx6, d6, _, _, all_d2) = _float_case(M, D, Q)
    idx, d5 = idx6[:, :5], d6[:, :5]
    votes = np.stack([np.bincount(labels[i], minlength=10) for i in idx])
    b64, q64 = bank.astype(np.float64), q.astype(np.float64)
    bound = (D + 3) * 2.0 ** -24 * ((q64 ** 2).sum(1) + (b64 ** 2).sum(1).max())
    decided = (d6[:, 5] - d6[:, 4]) > 2 * bound
    print(f"M={M} D={D} Q={Q}: undecided {int((~decided).sum())} of {Q}")
    assert (~decided).mean() <= 0.25, "a condition on the inputs"
    g = grounding.PartGrounder(_t(bank, cuda), _t(labels, cuda), k=5, n_classes=10)
    got = g.kneighbors(_t(q, cuda))
    gi, gd = got["index"].cpu().numpy(), got["d2"].cpu().numpy().astype(np.float64)
    true_d = np.take_along_axis(all_d2, gi.astype(np.int64), 1)
    print("largest |d2 - true| / bound:", float((np.abs(gd - true_d) / bound[:, None]).max()))
    for i in range(Q):
        if decided[i]:
            assert set(gi[i]) == set(idx[i]) and int(got["label"][i]) == int(votes[i].argmax()), i
            assert np.all(np.abs(np.sort(gd[i]) - d5[i]) <= bound[i]), i
        assert np.all(true_d[i] <= d5[i, 4] + 2 * bound[i]), i
        assert len(set(gi[i])) == 5 and np.all(np.diff(gd[i]) >= 0)
    # the same queries over two calls: bit-equal rows
    h = Q // 3
    a, b = g.kneighbors(_t(q[:h], cuda)), g.kneighbors(_t(q[h:], cuda))
    for f in ("index", "d2", "votes", "label"):
        assert torch.equal(torch.cat([a[f], b[f]]), got[f]), f


# ---- golden -------------------------------------------------------------------------------------------------------------------------
def test_device_path_reproduces_the_golden(cuda):
    from gapartnet_amd.misc import grounding
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    for name in ("a", "b", "c"):
        K, H, W, Hf, Wf = (int(v) for v in golden[f"masks_{name}_shape"])
        masks = np.unpackbits(golden[f"masks_{name}_bits"], axis=1)[:, :H * W].reshape(K, H, W).astype(bool)
        assert np.array_equal(grounding.resize_masks(_t(masks, cuda), (Hf, Wf)).cpu().numpy(), golden[f"levels_{name}"]), name
    g = grounding.PartGrounder(_t(golden["knn_bank"], cuda), _t(golden["knn_labels"], cuda), k=5, n_classes=10)
    got = g.kneighbors(_t(golden["knn_queries"], cuda))
    assert np.array_equal(got["label"].cpu().numpy(), golden["knn_pred"])
    assert np.array_equal(got["index"].cpu().numpy(), golden["knn_index"])
    assert np.allclose(np.sqrt(got["d2"].cpu().numpy()), golden["knn_dist"], rtol=1e-4, atol=0)
    assert np.array_equal(g.predict(_t(golden["knn_queries"], cuda)).cpu().numpy(), golden["knn_pred"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
H, W, NPTS, PRE, RANSAC = 96, 128, 2048, 2, 32
SEEDS = [3, 4]


def test_label_masks_equals_the_steps(cuda):
    from gapartnet_amd.misc import grounding
    rng = np.random.default_rng(11)
    fea = rng.normal(size=(2, 12, 16, 24)).astype(np.float32)
    masks = rng.random((5, H, W)) < 0.4
    view = np.array([0, 1, 1, 0, 1])
    bank, labels = rng.normal(size=(60, 24)).astype(np.float32), rng.integers(0, 10, size=60)
    g = grounding.PartGrounder(_t(bank, cuda), _t(labels, cuda))
    out = g.label_masks(_t(fea, cuda), _t(masks, cuda), view)
    levels = G.mask_levels(masks, (12, 16))
    assert torch.equal(out["features"], grounding.pool_levels(_t(fea, cuda), _t(levels, cuda), _t(view, cuda)))
    idx, _, votes, label, _ = G.knn(out["features"].cpu().numpy(), bank, labels, 5, 10)
    assert np.array_equal(out["index"].cpu().numpy(), idx) and np.array_equal(out["votes"].cpu().numpy(), votes)
    assert out["label"].dtype == torch.int64 and np.array_equal(out["label"].cpu().numpy(), label)
    cpu = grounding.PartGrounder(torch.from_numpy(bank), torch.from_numpy(labels)).label_masks(torch.from_numpy(fea), torch.from_numpy(masks), view)
    assert np.array_equal(cpu["label"].numpy(), label)


def test_predict_frames_with_class_agnostic_masks(cuda):
    from gapartnet_amd import inference
    from gapartnet_amd.misc import grounding
    from tests import frame_ref as F
    from tests import inference_ref as R
    from tests import pipeline_runner as PR
    model = PR.build_model(cuda).eval()
    model.revoxelize_jitter = tuple(torch.tensor(j, device=cuda) for j in ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9]))
    a, c = (x.numpy()[:-8] for x in R.raw_clouds(20000))
    depth, rgb, K = F.frames_from_clouds([a, c], H, W)
    rng = np.random.RandomState(4)
    masks = []
    for k in (4, 3):
        mk = np.zeros((k, H, W), bool)
        for j in range(k):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            mk[j, y0:y0 + H // 3, x0:x0 + W // 3] = True
        masks.append(_t(mk, cuda))
    feats = [_t(rng.normal(size=(12, 16, 24)).astype(np.float32), cuda) for _ in range(2)]
    grounder = grounding.PartGrounder(_t(rng.normal(size=(60, 24)).astype(np.float32), cuda), _t(rng.randint(1, 4, size=60), cuda))
    predictor = inference.PartPredictor(model, num_points=NPTS, max_iters=RANSAC)
    picks = lambda sizes: R.size_picks(sizes, RANSAC)  # noqa: E731
    call = lambda labels, **kw: predictor.predict_frames_with_masks(  # noqa: E731
        _t(depth, cuda), _t(rgb, cuda), torch.from_numpy(K), masks, labels, picks=picks, presample=PRE, seed=SEEDS, flip=True, **kw)

    def same(x, y, fields):
        for p, w in zip(x, y):
            for f in fields:
                u, v = getattr(p.masks, f), getattr(w.masks, f)
                if u.dtype.is_floating_point:
                    u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
                assert torch.equal(u, v), f
            assert torch.equal(p.overlay, w.overlay) and torch.equal(p.proposal_classes, w.proposal_classes)

    asked = [grounder.label_masks(feats[v], masks[v]) for v in range(2)]
    got = call(None, features=feats, grounder=grounder)
    want = call([o["label"] for o in asked])
    same(got, want, inference.MASK_FIELDS)
    for v in range(2):
        assert torch.equal(got[v].masks.label, asked[v]["label"]) and torch.equal(got[v].masks.label_votes, asked[v]["votes"])
        assert want[v].masks.label_votes is None and "mask_label_votes" in got[v].to_numpy() and "mask_label_votes" not in want[v].to_numpy()
        assert bool(((asked[v]["label"] >= 1) & (asked[v]["label"] <= 3)).all())
    # one frame labelled by the caller, one by the bank; explicit labels with a grounder in the call: nothing changes
    mixed = call([asked[0]["label"], None], features=feats, grounder=grounder)
    same(mixed, want, inference.MASK_FIELDS)
    assert mixed[0].masks.label_votes is None and torch.equal(mixed[1].masks.label_votes, asked[1]["votes"])
    same(call([o["label"] for o in asked], features=feats, grounder=grounder), want, inference.MASK_FIELDS)
    assert int(sum(p.masks.kept.sum() for p in got)) > 0


def test_argument_errors(cuda):
    from gapartnet_amd import _C, hip_ops, inference
    from gapartnet_amd.misc import grounding
    bank, lab = torch.zeros(6, 3, device=cuda), torch.arange(6, device=cuda)
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank[:4], lab[:4], k=5)
    with pytest.raises(_C.GpnError):
        grounding.PartGrounder(bank, lab, k=5, n_classes=5)  # label 5 is out of range
    norms = hip_ops.ground_bank_norms(bank)
    q = torch.zeros(2, 3, device=cuda)
    for kw in (dict(k=7, n_classes=10), dict(k=0, n_classes=10), dict(k=33, n_classes=10), dict(k=5, n_classes=65)):
        with pytest.raises(_C.GpnError, match="bad argument"):
            hip_ops.ground_knn(q, bank, norms, lab.int(), **kw)
    with pytest.raises(_C.GpnError):
        hip_ops.ground_knn(q.cpu(), bank, norms, lab.int(), 5, 10)
    g = grounding.PartGrounder(bank, lab, k=5)
    predictor = inference.PartPredictor(torch.nn.Identity())  # (never reached: the arguments are refused first)
    z = torch.zeros(2, 8, 8, device=cuda)
    with pytest.raises(_C.GpnError, match="feature maps"):
        predictor.predict_frames_with_masks(z, torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=cuda), torch.eye(3).repeat(2, 1, 1),
                                            [torch.zeros(1, 8, 8, dtype=torch.bool)] * 2, None, features=[torch.zeros(4, 4, 3, device=cuda)],
                                            grounder=g)
    with pytest.raises(_C.GpnError, match="no labels"):
        predictor.predict_frames_with_masks(z, torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=cuda), torch.eye(3).repeat(2, 1, 1),
                                            [torch.zeros(1, 8, 8, dtype=torch.bool)] * 2, [None, torch.zeros(1)])
