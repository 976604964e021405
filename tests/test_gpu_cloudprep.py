"""csrc/cloudprep.hip (include/gpn.h section CP) on the GPU against the numpy restatement (tests/inference_ref.py): integers exact,
floats bit-equal."""
import numpy as np
import pytest
import torch

from tests import inference_ref as R

pytestmark = pytest.mark.gpu
M_SAMPLES = 256


def _main_clouds():
    """the seven clouds of the main case, stride 6"""
    rng = np.random.RandomState(11)
    clean = rng.randn(1000, 6).astype(np.float32)
    holes = rng.randn(1000, 6).astype(np.float32)
    bad = np.concatenate([[0, 1, 998, 999], rng.choice(np.arange(2, 998), 116, replace=False)])
    holes[bad, rng.randint(0, 3, size=120)] = rng.choice([np.nan, np.inf, -np.inf], size=120)
    exact = rng.randn(300, 6).astype(np.float32)   # exactly 256 valid rows
    exact[rng.choice(300, 44, replace=False), 1] = np.nan
    few = rng.randn(130, 6).astype(np.float32)     # 100 valid rows: all kept
    few[rng.choice(130, 30, replace=False), 2] = np.inf
    empty = np.zeros((0, 6), np.float32)
    same = np.tile(rng.randn(1, 6).astype(np.float32), (300, 1))
    same[:, 3:] = rng.randn(300, 3)                # (the feature columns differ: sample_rows are visible in them)
    big = rng.randn(70000, 6).astype(np.float32)   # gpn_view_fps shares a cloud of this size between workgroups
    return [clean, holes, exact, few, empty, same, big]


@pytest.fixture(scope="module")
def main_case():
    clouds = _main_clouds()
    assert int(np.isfinite(clouds[1][:, :3]).all(1).sum()) == 880 and int(np.isfinite(clouds[2][:, :3]).all(1).sum()) == 256
    assert int(np.isfinite(clouds[3][:, :3]).all(1).sum()) == 100
    return clouds, [R.prepare_cloud(c, M_SAMPLES) for c in clouds]


def _offsets(clouds):
    return [0] + np.cumsum([c.shape[0] for c in clouds]).tolist()


def _check_prepared(got, clouds, want, m):
    out, rows = got["out"].cpu().numpy(), got["sample_rows"].cpu().numpy()
    for s, (c, w) in enumerate(zip(clouds, want)):
        assert int(got["status"][s]) == w["status"], s
        ms = min(w["count"], m)
        assert int(got["counts"][s]) == ms, s
        assert np.array_equal(got["scale"][s].numpy(), w["scale"]), (s, got["scale"][s], w["scale"])
        assert np.array_equal(rows[s, :ms], w["sample_rows"]) and (rows[s, ms:] == -1).all(), s
        assert np.array_equal(out[s, :ms].view(np.uint32), w["out"].view(np.uint32)), s
        assert not out[s, ms:].any(), s
        if ms:  # sample_rows point at the caller's rows
            assert np.array_equal(out[s, :ms, 3:].view(np.uint32), c[rows[s, :ms], 3:].view(np.uint32)), s


@pytest.mark.parametrize("max_groups", [0, 1])
def test_cloud_prepare_equals_the_restatement(cuda, main_case, max_groups):
    from gapartnet_amd import hip_ops
    clouds, want = main_case
    assert [w["status"] for w in want] == [R.OK, R.OK, R.OK, R.OK, R.EMPTY, R.DEGENERATE, R.OK]
    pts = torch.from_numpy(np.concatenate(clouds)).to(cuda)
    got = hip_ops.cloud_prepare(pts, _offsets(clouds), M_SAMPLES, max_groups=max_groups)
    _check_prepared(got, clouds, want, M_SAMPLES)
    if max_groups == 0:  # two runs on the same input are bit-equal
        again = hip_ops.cloud_prepare(pts, _offsets(clouds), M_SAMPLES)
        for k in ("out", "sample_rows", "counts", "status", "scale"):
            assert torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                               again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]), k


def test_cloud_prepare_strides(cuda, main_case):
    """no feature columns; a column slice of a wider tensor, read through its row pitch"""
    from gapartnet_amd import hip_ops
    clouds, want = main_case
    pick = [1, 3, 4, 0]
    sub, wsub = [clouds[i] for i in pick], [want[i] for i in pick]
    xyz = [np.ascontiguousarray(c[:, :3]) for c in sub]
    got = hip_ops.cloud_prepare(torch.from_numpy(np.concatenate(xyz)).to(cuda), _offsets(xyz), M_SAMPLES)
    assert tuple(got["out"].shape) == (4, M_SAMPLES, 3)
    w3 = [dict(w, out=np.ascontiguousarray(w["out"][:, :3])) for w in wsub]
    _check_prepared(got, xyz, w3, M_SAMPLES)
    wide = torch.from_numpy(np.concatenate([np.concatenate([np.full((c.shape[0], 2), 7, np.float32), c, np.full((c.shape[0], 3), -7, np.float32)], 1)
                                            for c in sub])).to(cuda)
    view = wide[:, 2:8]
    assert not view.is_contiguous()
    got = hip_ops.cloud_prepare(view, _offsets(sub), M_SAMPLES)
    _check_prepared(got, sub, wsub, M_SAMPLES)


def test_cloud_entry_points_check_their_arguments():
    import ctypes
    from gapartnet_amd import _C
    lib = _C.lib()
    i64, i32 = ctypes.c_int64, ctypes.c_int
    assert lib.gpn_cloud_pack(None, i64(5), i32(2), None, i32(1), i64(5), None, None, None, None, None) == 1
    assert b"bad argument" in lib.gpn_last_error()
    assert lib.gpn_cloud_finish(None, i64(5), i32(3), i32(3), None, i32(1), i64(5), None, None, None, i32(0), None, None, None, None, None) == 1
    assert lib.gpn_cloud_nearest(None, i64(5), i32(3), None, i32(1), None, None, None, i32(4), None, None, None, ctypes.c_size_t(0), None) == 1
    assert lib.gpn_cloud_nearest_ws_bytes(i32(4), i32(700)) > 4 * 700 * 16


# ---------------------------------------------------------------------------------------------------- nearest sample
def _grid(rng, lo, hi, n):
    return (rng.randint(int(lo * 64), int(hi * 64) + 1, size=(n, 3)) / 64).astype(np.float32)


def _samples_700(rng, kind):
    if kind == "duplicates":      # 350 distinct positions, each twice, inside [-0.5, 0.5]: queries up to 1.5 outside on each side
        s = _grid(rng, -0.5, 0.5, 350)
        return np.concatenate([s, s])[rng.permutation(700)]
    if kind == "plane":
        s = _grid(rng, -1, 1, 700)
        s[:, 1] = 0.25
        return s
    if kind == "line":
        s = _grid(rng, -1, 1, 700)
        s[:, 0], s[:, 2] = -0.5, 1.0
        return s
    assert kind == "one_cell"     # 699 samples inside one cell of the 18-cell grid over [-2, 2], one at the opposite corner
    s = (rng.randint(-128, -128 + 8, size=(700, 3)) / 64).astype(np.float32)
    s[345] = 2.0
    return s


@pytest.mark.parametrize("kind", ["duplicates", "plane", "line", "one_cell"])
def test_cloud_nearest_on_exact_inputs(cuda, kind):
    """coordinates are multiples of 1/64 in [-2, 2]: every d2 is exact in fp32 and ties are real.  Clouds with 1, 2, 700 and 0
    samples, 5000 rows each: the samples themselves (queries equal to samples), queries all over [-2, 2] (outside the samples' box,
    far more than eight cells of it), rows with NaN / inf."""
    from gapartnet_amd import hip_ops
    rng = np.random.RandomState({"duplicates": 1, "plane": 2, "line": 3, "one_cell": 4}[kind])
    n_samples, Q, m = [1, 2, 700, 0], 5000, 700
    clouds, srows = [], np.full((4, m), -1, np.int32)
    for s, k in enumerate(n_samples):
        if k == 2:
            samples = np.repeat(_grid(rng, -1, 1, 1), 2, 0) if kind == "duplicates" else _grid(rng, -1, 1, 2)
        else:
            samples = _samples_700(rng, kind)[:k]
        extra = _grid(rng, -2, 2, Q - k)
        if k:
            extra[:200] = samples[rng.randint(0, k, size=200)]  # more queries equal to samples
        order = rng.permutation(Q)
        cloud = np.concatenate([samples, extra])[order]
        where = np.argsort(order)[:k]                           # the rows the samples moved to
        bad = rng.choice(np.setdiff1d(np.arange(Q), where), 40, replace=False)
        cloud[bad, rng.randint(0, 3, size=40)] = rng.choice([np.nan, np.inf, -np.inf], size=40)
        srows[s, :k] = where
        clouds.append(cloud)
    counts = torch.tensor(n_samples, dtype=torch.int32)
    status = torch.tensor([R.OK, R.OK, R.OK, R.EMPTY], dtype=torch.int32)
    pts = torch.from_numpy(np.concatenate(clouds)).to(cuda)
    nn, d2 = hip_ops.cloud_nearest(pts, [0, Q, 2 * Q, 3 * Q, 4 * Q], torch.from_numpy(srows).to(cuda), counts.to(cuda),
                                   status.to(cuda), want_d2=True)
    nn, d2 = nn.cpu().numpy(), d2.cpu().numpy()
    for s, k in enumerate(n_samples):
        want_nn, want_d2 = R.nearest(clouds[s], clouds[s][srows[s, :k]])
        assert np.array_equal(nn[s * Q:(s + 1) * Q], want_nn), (kind, s, np.nonzero(nn[s * Q:(s + 1) * Q] != want_nn)[0][:10])
        assert np.array_equal(d2[s * Q:(s + 1) * Q], want_d2), (kind, s)
    if kind == "duplicates":  # a tie between the two copies of a position goes to the lower sample
        s700 = clouds[2][srows[2]]
        first = np.array([np.nonzero((s700 == p).all(1))[0][0] for p in s700])
        assert np.array_equal(nn[2 * Q:3 * Q][srows[2]], first) and (first != np.arange(700)).sum() >= 350


def test_cloud_nearest_at_size(cuda):
    """200 000 uniform queries against 20 000 of them as samples, against torch ops on the device"""
    from gapartnet_amd import hip_ops
    g = torch.Generator().manual_seed(3)
    N, ms = 200000, 20000
    pts = torch.rand((N, 3), generator=g).to(cuda)
    srows = torch.randperm(N, generator=g)[:ms].to(torch.int32).to(cuda)
    nn = hip_ops.cloud_nearest(pts, [0, N], srows[None], torch.tensor([ms], dtype=torch.int32, device=cuda),
                               torch.zeros(1, dtype=torch.int32, device=cuda)).long()
    samples = pts[srows.long()]
    ar = torch.arange(ms, device=cuda)
    want = torch.empty(N, dtype=torch.int64, device=cuda)
    for a in range(0, N, 8192):
        q = pts[a:a + 8192]
        dx, dy, dz = q[:, None, 0] - samples[None, :, 0], q[:, None, 1] - samples[None, :, 1], q[:, None, 2] - samples[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        want[a:a + 8192] = torch.where(d == d.amin(1, keepdim=True), ar[None, :], ms).amin(1)
    assert torch.equal(nn, want), int((nn != want).sum())
    assert torch.equal(nn[srows.long()], ar)  # (no duplicate positions among uniform draws: a sample's nearest sample is itself)
