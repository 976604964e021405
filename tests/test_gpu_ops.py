"""GPU parity: every C-ABI entry point of libgpn_hip.so (called through gapartnet_amd.hip_ops) against the
CPU oracle on the same seeded inputs.  Integer outputs (voxel ids, rulebooks, neighbour lists, labels, argmax,
NMS keep lists, FPS / kNN indices) must be bit-exact; floating-point outputs are compared with the tolerance
written next to each check (north_star: 1e-4 for features)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle as O
from tests import synth

pytestmark = pytest.mark.gpu

FP_TOL = 1e-4  # north_star tolerance for features


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def H():
    from gapartnet_amd import hip_ops
    return hip_ops


if os.environ.get("GPN_TEST_LOGIC_ON_CPU"):
    # self-check of the test logic in a GPU-less container: oracle vs oracle on CPU tensors (proves nothing about
    # the kernels; never set on the GPU box)
    @pytest.fixture(scope="module")
    def H():  # noqa: F811
        from oracle import torch_ops
        return torch_ops

    @pytest.fixture(scope="module")
    def cuda():  # noqa: F811
        return torch.device("cpu")


# ------------------------------------------------------------------------------------------------ V
@pytest.mark.parametrize("M,S,C,vs", [(20000, 1, 6, 0.01), (30000, 4, 6, 0.01), (5000, 37, 16, 0.05), (1, 1, 3, 0.1)])
def test_voxelize_matches_oracle(H, cuda, M, S, C, vs):
    rng = np.random.default_rng(M + S)
    pts = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    pts[: M // 10] = pts[M // 10: 2 * (M // 10)][: M // 10]  # exact duplicates
    feats = rng.normal(size=(M, C)).astype(np.float32)
    cuts = np.sort(rng.choice(np.arange(1, M), size=S - 1, replace=False)) if S > 1 else np.array([], np.int64)
    offs = np.concatenate([[0], cuts, [M]]).astype(np.int64)
    rmin = np.stack([pts[offs[s]:offs[s + 1]].min(0) - 1e-4 for s in range(S)]).astype(np.float32)
    rmax = np.stack([pts[offs[s]:offs[s + 1]].max(0) + 1e-4 for s in range(S)]).astype(np.float32)
    grid = [int(2.1 / vs) + 2] * 3
    ref = O.voxelize(pts, feats, offs, rmin, rmax, [vs] * 3, grid)
    got = H.voxelize(dev(pts, cuda), dev(feats, cuda), dev(offs, cuda), dev(rmin, cuda), dev(rmax, cuda), [vs] * 3,
                     grid, want_csr=True)
    vf, vc, vseg, pid, order, vstart = [host(t) for t in got]
    assert np.array_equal(vc, ref[1]) and np.array_equal(vseg, ref[2]) and np.array_equal(pid, ref[3])
    assert np.array_equal(vf, ref[0]), "means are ordered sums: expected bit-exact"
    # CSR consistency
    V = vc.shape[0]
    assert vstart[0] == 0 and vstart[V] == M and np.array_equal(pid[order[:vstart[V]]], np.repeat(np.arange(V), np.diff(vstart)))


def test_voxelize_drops_out_of_range(H, cuda):
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    feats = pts.copy()
    offs = np.array([0, 4000], np.int64)
    rmin, rmax = np.array([[-0.5, -0.5, -0.5]], np.float32), np.array([[0.5, 0.5, 0.5]], np.float32)
    ref = O.voxelize(pts, feats, offs, rmin, rmax, [0.1] * 3, [12] * 3)
    got = [host(t) for t in H.voxelize(dev(pts, cuda), dev(feats, cuda), dev(offs, cuda), dev(rmin, cuda), dev(rmax, cuda), [0.1] * 3, [12] * 3)]
    assert (ref[3] < 0).any()
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ K
def _check_rb(rb, ref):
    P = ref[0].shape[0]
    assert int(rb.num_pairs.item()) == P
    assert np.array_equal(host(rb.pair_src)[:P], ref[0])
    assert np.array_equal(host(rb.pair_dst)[:P], ref[1])
    assert np.array_equal(host(rb.tile_off), ref[2])


@pytest.mark.parametrize("kind,batch,shape,n", [("random", 2, [12, 10, 14], 700), ("surface", 3, [64, 64, 64], 5000),
                                                 ("random", 1, [5, 5, 5], 125), ("random", 1, [3, 3, 3], 1)])
def test_rulebooks_bit_exact(H, cuda, kind, batch, shape, n):
    rng = np.random.default_rng(n)
    idx = synth.random_sparse_indices(rng, batch, shape, n) if kind == "random" else synth.surface_indices(rng, batch, shape, n)
    _check_rb(H.rulebook_subm3(dev(idx, cuda), shape), O.rulebook_subm3(idx, shape))
    d = O.rulebook_down(idx, shape)
    out_idx, out_shape, rb_f, rb_b = H.rulebook_down(dev(idx, cuda), shape, batch)
    assert out_shape == d["out_shape"]
    assert np.array_equal(host(out_idx), d["out_indices"])
    _check_rb(rb_f, d["fwd"])
    _check_rb(rb_b, d["bwd"])


@pytest.mark.parametrize("kind,batch,shape,n,levels", [("surface", 3, [64, 64, 64], 5000, 5), ("random", 2, [12, 10, 14], 700, 3),
                                                        ("surface", 8, [190, 200, 130], 40000, 6), ("random", 1, [3, 3, 3], 1, 1)])
def test_level_counts_equal_the_chain_of_down_rulebooks(H, cuda, kind, batch, shape, n, levels):
    """gpn_rulebook_level_counts (one pass, one read) == the row counts n successive stride-2 rulebooks produce (oracle), and
    rulebook_down fed with the count builds what it builds when it reads the count itself; odd extents drop the last plane"""
    rng = np.random.default_rng(n + levels)
    idx = synth.random_sparse_indices(rng, batch, shape, n) if kind == "random" else synth.surface_indices(rng, batch, shape, n)
    want, cur, cur_shape = [], idx, list(shape)
    for _ in range(levels):
        d = O.rulebook_down(cur, cur_shape)
        want.append(d["out_indices"].shape[0])
        cur, cur_shape = d["out_indices"], d["out_shape"]
    got = H.rulebook_level_counts(dev(idx, cuda), shape, batch, levels).tolist()
    assert got == want
    a = H.rulebook_down(dev(idx, cuda), shape, batch)
    b = H.rulebook_down(dev(idx, cuda), shape, batch, n_out=got[0])
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    for ra, rb in ((a[2], b[2]), (a[3], b[3])):
        P = int(ra.num_pairs.item())  # (the pair arrays are capacity-sized: only the first P entries are defined)
        assert P == int(rb.num_pairs.item()) and torch.equal(ra.tile_off, rb.tile_off)
        assert torch.equal(ra.pair_src[:P], rb.pair_src[:P]) and torch.equal(ra.pair_dst[:P], rb.pair_dst[:P])


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 1000, 65537])
def test_identity_rulebook_equals_the_torch_formulation(H, cuda, n):
    """gpn_rulebook_identity (one launch) == the arange / clamp / cat construction the K = 1 convs used before"""
    rb = H.rulebook_identity(n, cuda)
    rows = torch.arange(n, dtype=torch.int32, device=cuda)
    tiles = (n + 31) // 32
    assert torch.equal(rb.pair_src, rows) and torch.equal(rb.pair_dst, rows) and int(rb.num_pairs.item()) == n
    assert torch.equal(rb.tile_off.reshape(-1), torch.clamp(torch.arange(tiles + 1, dtype=torch.int32, device=cuda) * 32, max=n))
    assert torch.equal(rb.nbr, torch.cat([rows, torch.full((1,), -1, dtype=torch.int32, device=cuda)]))
    assert (rb.K, rb.n_src, rb.n_dst) == (1, n, n)


def test_scene_batch_voxelisation_with_one_host_read(H, cuda):
    """gpn_voxelize_scenes (per-scene ranges on the device, packed keys, voxel count + extent + coarse-level row counts in
    ONE read) == the two-read path (torch min / max, grid extent read, gpn_voxelize_ex, separate level-count call): same
    voxel order, bit-equal means, same extent and level counts; ragged scene sizes; a grid too fine for the packed keys
    falls back"""
    from gapartnet_amd.structure import point_cloud as PC
    from gapartnet_amd import backend
    rng = np.random.default_rng(21)
    for counts in ([5000] * 4, [3000, 1, 4500, 777]):
        M = sum(counts)
        xyz = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(np.float32)).to(cuda)
        n7 = xyz[3::7].shape[0]
        xyz[0:7 * n7:7] = xyz[3::7]  # duplicates: voxels with several points
        feats = torch.cat([xyz, torch.from_numpy(rng.uniform(0, 1, (M, 3)).astype(np.float32)).to(cuda)], 1)
        one = PC.voxelize_scenes(xyz, feats, counts, (0.01, 0.01, 0.01), pyramid_levels=5)
        import gapartnet_amd.hip_ops as HO
        saved = HO.voxelize_scenes
        del HO.voxelize_scenes
        try:
            two = PC.voxelize_scenes(xyz, feats, counts, (0.01, 0.01, 0.01))
        finally:
            HO.voxelize_scenes = saved
        assert torch.equal(one[0], two[0]), "indices (scene, x, y, z) in the same order"
        assert torch.equal(one[1], two[1]), "ordered means: bit-equal"
        assert one[2] == two[2] and torch.equal(one[3], two[3])
        assert torch.equal(one[4][0], two[4][0]) and torch.equal(one[4][1], two[4][1])
        ref_counts = H.rulebook_level_counts(two[0], two[2], len(counts), 5).tolist()
        assert list(one[5]) == ref_counts, (one[5], ref_counts)
    # 0.001 voxels on a 2 m scene: 2000 cells per axis do not fit 10-bit packed coordinates -> the generic path answers
    xyz = torch.from_numpy(rng.uniform(-1, 1, (4000, 3)).astype(np.float32)).to(cuda)
    assert H.voxelize_scenes(xyz, xyz, torch.tensor([0, 4000], device=cuda), [0.001] * 3) is None
    out = PC.voxelize_scenes(xyz, xyz, [4000], (0.001, 0.001, 0.001), pyramid_levels=3)
    assert out[5] is None and out[0].shape[0] > 3900 and max(out[2]) > 1024


@pytest.mark.parametrize("case", ["bench", "ragged", "heavy", "dropped", "one_point", "many_blocks"])
def test_sort_free_scene_voxelisation_equals_the_sorting_form(H, cuda, case):
    """gpn_voxelize_scenes (round 5: occupancy bitmap in key order + popcount ranks + counting placement, no sort) against
    gpn_voxelize_scenes_sorted (stable radix sort of packed keys; pinned to the oracle through the per-call path): voxel order,
    point -> voxel map, the points-by-voxel CSR (ascending point order inside a voxel, dropped points last), ordered means,
    extent, dropped count and the coarse levels' row counts - all EQUAL.  Cases: the bench's batch, ragged scene sizes, voxels
    holding hundreds of points, points that are dropped (NaN coordinates), a one-point scene, and five sparse scenes of 193 cells
    per axis: a bitmap of 1.12 M words = 1097 blocks of 1024, more than one tile of the one-workgroup scan of the block sums."""
    rng = np.random.default_rng({"bench": 1, "ragged": 2, "heavy": 3, "dropped": 4, "one_point": 5, "many_blocks": 6}[case])
    counts = {"bench": [20000] * 8, "ragged": [3000, 1, 4500, 777, 12000], "heavy": [6000, 6000], "dropped": [5000, 4000, 3000],
              "one_point": [1], "many_blocks": [2000] * 5}[case]
    M = sum(counts)
    half = 0.96 if case == "many_blocks" else 0.5
    xyz = rng.uniform(-half, half, (M, 3)).astype(np.float32)
    if case == "many_blocks":
        cells = [int(np.floor((np.ptp(xyz[:, a].astype(np.float64))) / 0.01)) for a in range(3)]  # (a lower bound of the grid)
        assert 1024 * 1024 * 32 < 5 * cells[0] * cells[1] * cells[2] and 5 * 194 ** 3 < 2 ** 27 and max(cells) < 1024
    if case == "heavy":
        xyz[::2] = np.round(xyz[::2] * 4) / 4 + 0.003   # a few hundred points per voxel on a coarse lattice
    if case == "dropped":
        xyz[rng.choice(M, 37, replace=False), rng.integers(0, 3, 37)] = np.nan
    xyz = torch.from_numpy(xyz).to(cuda)
    feats = torch.cat([xyz.nan_to_num(0.0), torch.from_numpy(rng.uniform(0, 1, (M, 3)).astype(np.float32)).to(cuda)], 1)
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64, device=cuda)
    a = H.voxelize_scenes(xyz, feats, offsets, [0.01] * 3, 5, sorted_form=True)
    b = H.voxelize_scenes(xyz, feats, offsets, [0.01] * 3, 5)
    assert a is not None and b is not None
    names = ("voxel_feats", "indices", "pc_voxel_id", "point_order", "voxel_point_start")
    for name, x, y in zip(names, a[:5], b[:5]):
        assert x.shape == y.shape and x.dtype == y.dtype, name
        assert torch.equal(x, y), name
    assert list(a[5]) == list(b[5]) and a[6] == b[6] and list(a[7]) == list(b[7]), (a[5:], b[5:])
    if case == "dropped":
        assert a[6] == 37 and int((b[2] < 0).sum()) == 37
    if case == "heavy":
        sizes = torch.diff(b[4])
        assert int(sizes.max()) > 40


# ------------------------------------------------------------------------------------------------ C
CONV_SHAPES = [(16, 16), (32, 32), (48, 48), (64, 64), (80, 80), (96, 96), (112, 112), (32, 16), (64, 32), (96, 48),
               (128, 64), (160, 80), (192, 96), (16, 32), (96, 112)]


@pytest.mark.parametrize("cin,cout", CONV_SHAPES)
def test_subm_conv_fwd_dgrad_wgrad(H, cuda, cin, cout):
    rng = np.random.default_rng(cin * 1000 + cout)
    shape = [40, 40, 40]
    idx = synth.surface_indices(rng, 2, shape, 1500)
    N = idx.shape[0]
    f = rng.normal(size=(N, cin)).astype(np.float32)
    W = (rng.normal(size=(27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    g = rng.normal(size=(N, cout)).astype(np.float32)
    rb_ref = O.rulebook_subm3(idx, shape)
    rb = H.rulebook_subm3(dev(idx, cuda), shape)
    out = host(H.conv_fwd(dev(f, cuda), dev(W, cuda), rb))
    assert np.allclose(out, O.spconv_fwd(f, W, rb_ref, N), atol=FP_TOL, rtol=1e-4)
    din = host(H.conv_dgrad(dev(g, cuda), dev(W, cuda), rb, rb, True))
    assert np.allclose(din, O.spconv_dgrad(g, W, rb_ref, N, N), atol=FP_TOL, rtol=1e-4)
    dW = host(H.conv_wgrad(dev(f, cuda), dev(g, cuda), rb))
    ref_dW = O.spconv_wgrad(f, g, rb_ref, N, 27)
    # sums over ~1500 pairs per tap of O(1) products: entries are O(40); bound relative to the tensor's scale (north_star 1e-4)
    assert np.abs(dW - ref_dW).max() <= 1e-4 * np.abs(ref_dW).max(), (np.abs(dW - ref_dW).max(), np.abs(ref_dW).max())


@pytest.mark.parametrize("cin,cout", CONV_SHAPES + [(224, 112)])
@pytest.mark.parametrize("n_target", [1500, 37])
def test_weight_gradient_kernel_on_every_channel_pair(H, cuda, cin, cout, n_target):
    """the weight-gradient contraction (csrc/spconv.hip) on every channel pair of the U-Net (decoder concat widths included), a
    full-size and a tiny ragged input (fewer pairs per tap than one step; taps without pairs): against the oracle at 1e-4 of
    the tensor's scale, bit-reproducible, both layouts.  (Round 4's second contraction - gathered rows straight into MFMA
    operands, csrc/spconv_wgrad.hip - lost in the training step and was removed in round 5.)"""
    rng = np.random.default_rng(cin * 977 + cout + n_target)
    shape = [40, 40, 40]
    idx = synth.surface_indices(rng, 2, shape, n_target)
    N = idx.shape[0]
    f = rng.normal(size=(N, cin)).astype(np.float32)
    g = rng.normal(size=(N, cout)).astype(np.float32)
    rb_ref = O.rulebook_subm3(idx, shape)
    rb = H.rulebook_subm3(dev(idx, cuda), shape)
    ref = O.spconv_wgrad(f, g, rb_ref, N, 27)
    scale = np.abs(ref).max()
    a = H.conv_wgrad(dev(f, cuda), dev(g, cuda), rb)
    b = H.conv_wgrad(dev(f, cuda), dev(g, cuda), rb)
    assert torch.equal(a, b), "two runs differ"
    oki = H.conv_wgrad(dev(f, cuda), dev(g, cuda), rb, layout="oki")
    assert torch.equal(oki.permute(1, 2, 0), a), "[Cout, K, Cin] layout differs"
    assert np.abs(host(a) - ref).max() <= 1e-4 * scale, (np.abs(host(a) - ref).max(), scale)


@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 48), (96, 112)])
def test_down_and_inverse_conv(H, cuda, cin, cout):
    rng = np.random.default_rng(cin + cout)
    shape = [33, 40, 37]  # odd sizes: last plane dropped
    idx = synth.random_sparse_indices(rng, 2, shape, 4000)
    N = idx.shape[0]
    d = O.rulebook_down(idx, shape)
    No = d["out_indices"].shape[0]
    out_idx, out_shape, rb_f, rb_b = H.rulebook_down(dev(idx, cuda), shape, 2)
    f = rng.normal(size=(N, cin)).astype(np.float32)
    W = (rng.normal(size=(8, cin, cout)) / np.sqrt(8 * cin)).astype(np.float32)
    out = host(H.conv_fwd(dev(f, cuda), dev(W, cuda), rb_f))
    ref = O.spconv_fwd(f, W, d["fwd"], No)
    assert np.allclose(out, ref, atol=FP_TOL, rtol=1e-4)
    g = rng.normal(size=(No, cout)).astype(np.float32)
    din = host(H.conv_dgrad(dev(g, cuda), dev(W, cuda), rb_f, rb_b, False))
    assert np.allclose(din, O.spconv_dgrad(g, W, d["fwd"], No, N), atol=FP_TOL, rtol=1e-4)
    dW, ref_dW = host(H.conv_wgrad(dev(f, cuda), dev(g, cuda), rb_f)), O.spconv_wgrad(f, g, d["fwd"], No, 8)
    assert np.abs(dW - ref_dW).max() <= 1e-4 * np.abs(ref_dW).max(), (np.abs(dW - ref_dW).max(), np.abs(ref_dW).max())
    # inverse conv: coarse -> fine over the bwd lists
    Wi = (rng.normal(size=(8, cout, cin)) / np.sqrt(cout)).astype(np.float32)
    up = host(H.conv_fwd(dev(ref, cuda), dev(Wi, cuda), rb_b))
    assert np.allclose(up, O.spconv_fwd(ref, Wi, d["bwd"], N), atol=FP_TOL, rtol=1e-4)
    gi = rng.normal(size=(N, cin)).astype(np.float32)
    dci = host(H.conv_dgrad(dev(gi, cuda), dev(Wi, cuda), rb_b, rb_f, False))
    assert np.allclose(dci, O.spconv_dgrad(gi, Wi, d["bwd"], N, No), atol=FP_TOL, rtol=1e-4)


@pytest.fixture
def tiles_everywhere():
    """route every conv of >= 16 tiles through the masked-tile kernel (by default it takes layers of >= 4096 tiles)"""
    from gapartnet_amd import _C
    prev = _C.lib().gpn_spconv_tiles_min_tiles(16)
    yield
    _C.lib().gpn_spconv_tiles_min_tiles(prev)


@pytest.mark.parametrize("cin,cout", CONV_SHAPES)
def test_masked_tile_kernel_fwd_dgrad(H, cuda, tiles_everywhere, cin, cout):
    """the masked-tile kernel (csrc/spconv_tiles.hip) on every channel pair of the U-Net, voxel order and tile order:
    oracle values at 1e-4, and bit-equal to the direct kernel (same per-row summation order)"""
    from gapartnet_amd import _C
    rng = np.random.default_rng(cin * 1000 + cout + 7)
    shape = [40, 40, 40]
    idx = synth.surface_indices(rng, 2, shape, 1500)
    N = idx.shape[0]
    f = rng.normal(size=(N, cin)).astype(np.float32)
    W = (rng.normal(size=(27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    g = rng.normal(size=(N, cout)).astype(np.float32)
    rb_ref = O.rulebook_subm3(idx, shape)
    rb = H.rulebook_subm3(dev(idx, cuda), shape)
    assert rb.perm is None
    ref_out, ref_din = O.spconv_fwd(f, W, rb_ref, N), O.spconv_dgrad(g, W, rb_ref, N, N)
    outs, dins = [], []
    for ordered in (False, True):
        if ordered:
            rb.perm, rb.nbr_p = H.tile_order(rb.nbr, 27, N)
        outs.append(H.conv_fwd_ordered(dev(f, cuda), dev(W, cuda), rb))
        dins.append(H.conv_fwd_ordered(dev(g, cuda), dev(W, cuda), rb, flags=H.PACK_TRANSPOSE | H.PACK_REVERSE))
        assert np.allclose(host(outs[-1]), ref_out, atol=FP_TOL, rtol=1e-4)
        assert np.allclose(host(dins[-1]), ref_din, atol=FP_TOL, rtol=1e-4)
    assert torch.equal(outs[0], outs[1]) and torch.equal(dins[0], dins[1]), "the tile order must not change a bit"
    prev = _C.lib().gpn_spconv_tiles_min_tiles(1 << 40)  # the (unsplit) direct kernel on the same inputs
    _C.lib().gpn_spconv_direct_split(0, 0)
    _C.lib().gpn_spconv_msplit(0, -1, -1)
    try:
        assert torch.equal(outs[0], H.conv_fwd_ordered(dev(f, cuda), dev(W, cuda), rb))
    finally:
        _C.lib().gpn_spconv_tiles_min_tiles(prev)
        _C.lib().gpn_spconv_direct_split(12000, 0)
        _C.lib().gpn_spconv_msplit(1, -1, -1)


@pytest.mark.parametrize("ways", [2, 4])
@pytest.mark.parametrize("cin,cout", [(16, 16), (48, 48), (80, 80), (160, 80), (96, 112)])
def test_tap_split_direct_kernel(H, cuda, ways, cin, cout):
    """the direct kernel's tap-split forms (2 / 4 waves per (tile, column) unit, partial sums added in LDS in wave order):
    oracle values at 1e-4 for SubM (27 taps: 14 + 13 / 7 + 7 + 7 + 6) and stride-2 (8 taps) tables, two runs bit-equal"""
    from gapartnet_amd import _C
    big = 1 << 40
    _C.lib().gpn_spconv_direct_split(big if ways == 4 else 0, big if ways == 2 else 0)
    _C.lib().gpn_spconv_msplit(0, -1, -1)  # (round 6: these layers are the masked tap-split kernel's by default, tests/test_gpu_msplit.py)
    try:
        rng = np.random.default_rng(cin + 3 * cout + ways)
        shape = [40, 40, 40]
        idx = synth.surface_indices(rng, 2, shape, 1500)
        N = idx.shape[0]
        f = rng.normal(size=(N, cin)).astype(np.float32)
        W = (rng.normal(size=(27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
        rb_ref = O.rulebook_subm3(idx, shape)
        rb = H.rulebook_subm3(dev(idx, cuda), shape)
        out = H.conv_fwd(dev(f, cuda), dev(W, cuda), rb)
        assert np.allclose(host(out), O.spconv_fwd(f, W, rb_ref, N), atol=FP_TOL, rtol=1e-4)
        assert torch.equal(out, H.conv_fwd(dev(f, cuda), dev(W, cuda), rb)), "fixed summation order"
        g = rng.normal(size=(N, cout)).astype(np.float32)
        din = host(H.conv_dgrad(dev(g, cuda), dev(W, cuda), rb, rb, True))
        assert np.allclose(din, O.spconv_dgrad(g, W, rb_ref, N, N), atol=FP_TOL, rtol=1e-4)
        if cin <= 96 and cout <= 112:
            d = O.rulebook_down(idx, shape)
            _, _, rb_f, _rb_b = H.rulebook_down(dev(idx, cuda), shape, 2)
            W8 = (rng.normal(size=(8, cin, cout)) / np.sqrt(8 * cin)).astype(np.float32)
            down = host(H.conv_fwd(dev(f, cuda), dev(W8, cuda), rb_f))
            assert np.allclose(down, O.spconv_fwd(f, W8, d["fwd"], d["out_indices"].shape[0]), atol=FP_TOL, rtol=1e-4)
    finally:
        _C.lib().gpn_spconv_direct_split(12000, 0)
        _C.lib().gpn_spconv_msplit(1, -1, -1)


def test_masked_tile_kernel_down_inverse_and_ragged_tail(H, cuda, tiles_everywhere):
    """K = 8 tables (stride-2 conv and its inverse, rows without any tap), a row count that is not a multiple of 16,
    and the accumulate form the executor's backward uses"""
    rng = np.random.default_rng(99)
    shape = [33, 40, 37]
    idx = synth.random_sparse_indices(rng, 2, shape, 4001)
    N = idx.shape[0]
    d = O.rulebook_down(idx, shape)
    No = d["out_indices"].shape[0]
    _, _, rb_f, rb_b = H.rulebook_down(dev(idx, cuda), shape, 2)
    for cin, cout in ((16, 32), (48, 64)):
        f = rng.normal(size=(N, cin)).astype(np.float32)
        W = (rng.normal(size=(8, cin, cout)) / np.sqrt(8 * cin)).astype(np.float32)
        for ordered in (False, True):
            for rb in (rb_f, rb_b):
                rb.perm, rb.nbr_p = H.tile_order(rb.nbr, 8, rb.n_dst) if ordered else (None, None)
            out = host(H.conv_fwd_ordered(dev(f, cuda), dev(W, cuda), rb_f))
            ref = O.spconv_fwd(f, W, d["fwd"], No)
            assert np.allclose(out, ref, atol=FP_TOL, rtol=1e-4)
            Wi = (rng.normal(size=(8, cout, cin)) / np.sqrt(cout)).astype(np.float32)
            up = host(H.conv_fwd_ordered(dev(ref, cuda), dev(Wi, cuda), rb_b))
            assert np.allclose(up, O.spconv_fwd(ref, Wi, d["bwd"], N), atol=FP_TOL, rtol=1e-4)


def test_conv_large_batch_uses_wide_tiles(H, cuda):
    """>= 4096 32-row tiles selects the 64-row wave tile variant."""
    rng = np.random.default_rng(11)
    shape = [128, 128, 128]
    idx = synth.surface_indices(rng, 10, shape, 22000)
    N = idx.shape[0]
    assert N >= 4096 * 32
    f = rng.normal(size=(N, 16)).astype(np.float32)
    W = (rng.normal(size=(27, 16, 16)) / 20).astype(np.float32)
    rb = H.rulebook_subm3(dev(idx, cuda), shape)
    out = host(H.conv_fwd(dev(f, cuda), dev(W, cuda), rb))
    ref = O.spconv_fwd(f, W, O.rulebook_subm3(idx, shape), N)
    assert np.allclose(out, ref, atol=FP_TOL, rtol=1e-4)


def test_gather_scatter_rows(H, cuda):
    rng = np.random.default_rng(5)
    table = rng.normal(size=(3000, 16)).astype(np.float32)
    idx = rng.integers(-1, 3000, 20000).astype(np.int32)
    assert np.array_equal(host(H.gather_rows(dev(table, cuda), dev(idx, cuda))), O.gather_rows(table, idx))
    g = rng.normal(size=(20000, 16)).astype(np.float32)
    got = host(H.scatter_rows(dev(g, cuda), dev(idx, cuda), 3000))
    assert np.array_equal(got, O.scatter_rows(g, idx, 3000)), "ordered sums: bit-exact"
    for C in (3, 27):
        t2 = rng.normal(size=(100, C)).astype(np.float32)
        i2 = rng.integers(0, 100, 1000).astype(np.int32)
        assert np.array_equal(host(H.gather_rows(dev(t2, cuda), dev(i2, cuda))), O.gather_rows(t2, i2))


# ------------------------------------------------------------------------------------------------ B / L
@pytest.mark.parametrize("K,labels", [(50, True), (300, True), (8, False)])
def test_ball_query_and_ccl(H, cuda, K, labels):
    rng = np.random.default_rng(K)
    pts, batch = synth.clustered_points(rng, 3, 3000)
    offs = np.array([0, 3000, 6000, 9000], np.int32)
    lab = rng.integers(1, 4, pts.shape[0]).astype(np.int32) if labels else None
    ref_idx, ref_cnt = O.ball_query(pts, pts, batch, offs, 0.04, K, lab, lab)
    idx, cnt = H.ball_query(dev(pts, cuda), dev(pts, cuda), dev(batch, cuda), dev(offs, cuda), 0.04, K,
                            None if lab is None else dev(lab, cuda), None if lab is None else dev(lab, cuda))
    assert np.array_equal(host(cnt), ref_cnt) and np.array_equal(host(idx), ref_idx)
    Q = pts.shape[0]
    begin = np.arange(Q, dtype=np.int32) * K
    be = np.stack([begin, begin + ref_cnt], 1).reshape(-1)
    for compacted in (False, True):
        got = host(H.ccl(dev(be, cuda), idx.reshape(-1), compacted))
        assert np.array_equal(got, O.ccl(be, ref_idx.reshape(-1), compacted))


@pytest.mark.parametrize("Q", [1, 1023, 1024, 1025, 2049])
def test_ccl_compacted_labels_across_the_rank_scan_tiles(H, cuda, Q):
    """vertices 2 i and 2 i + 1 joined (an odd Q leaves the last one alone): every second vertex is a root, and the ranks of the
    roots - the compacted labels - are carried across the 1024-entry tiles of the one-workgroup scan from Q = 1025 on"""
    v = np.arange(Q, dtype=np.int32)
    has = (v ^ 1) < Q
    end = np.cumsum(has).astype(np.int32)
    be = np.stack([end - has, end], 1).reshape(-1)
    edges = (v ^ 1)[has]
    for compacted in (False, True):
        want = O.ccl(be, edges, compacted)
        assert np.array_equal(host(H.ccl(dev(be, cuda), dev(edges, cuda), compacted)), want)
    assert np.array_equal(want, v // 2)


def test_ball_query_unsorted_batches_and_empty_segment(H, cuda):
    rng = np.random.default_rng(8)
    pts = rng.uniform(-0.2, 0.2, (1000, 3)).astype(np.float32)
    offs = np.array([0, 400, 400, 1000], np.int32)  # segment 1 is empty
    q = rng.uniform(-0.2, 0.2, (777, 3)).astype(np.float32)
    qb = rng.integers(0, 3, 777).astype(np.int32)
    ref = O.ball_query(pts, q, qb, offs, 0.05, 16)
    got = H.ball_query(dev(pts, cuda), dev(q, cuda), dev(qb, cuda), dev(offs, cuda), 0.05, 16)
    assert np.array_equal(host(got[0]), ref[0]) and np.array_equal(host(got[1]), ref[1])


# ------------------------------------------------------------------------------------------------ R / I / N
def test_segmented_ops(H, cuda):
    rng = np.random.default_rng(9)
    sizes = rng.integers(1, 400, 300)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    vals = rng.normal(size=(offs[-1], 16)).astype(np.float32)
    vals[10:20] = vals[10]  # ties
    for mode in ("sum", "min", "max"):
        got = host(H.segmented_reduce(dev(vals, cuda), dev(offs[:-1], cuda), dev(offs[1:], cuda), mode))
        assert np.array_equal(got, O.segmented_reduce(vals, offs[:-1], offs[1:], mode)), mode
    p, a = H.segmented_maxpool_fwd(dev(vals, cuda), dev(offs[:-1], cuda), dev(offs[1:], cuda))
    rp, ra = O.segmented_maxpool(vals, offs[:-1], offs[1:])
    assert np.array_equal(host(p), rp) and np.array_equal(host(a), ra)
    g = rng.normal(size=rp.shape).astype(np.float32)
    assert np.array_equal(host(H.segmented_maxpool_bwd(dev(g, cuda), a, vals.shape[0])), O.segmented_maxpool_bwd(g, ra, vals.shape[0]))


def test_instance_iou_and_nms(H, cuda):
    rng = np.random.default_rng(10)
    B, I, P = 4, 9, 200
    sizes = rng.integers(5, 300, P)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = offs[-1]
    prop_b = np.sort(rng.integers(0, B, P)).astype(np.int32)
    bi = np.repeat(prop_b, sizes).astype(np.int32)
    il = rng.integers(-1, I, M).astype(np.int32)
    npi = rng.integers(0, 500, (B, I)).astype(np.int32)
    npi[:, -1] = 0
    got = host(H.instance_iou(dev(offs, cuda), dev(il, cuda), dev(bi, cuda), dev(npi, cuda)))
    assert np.array_equal(got, O.instance_iou(offs, il, bi, npi))
    ious = rng.uniform(0, 1, (P, P)).astype(np.float32)
    ious = np.maximum(ious, ious.T) * (rng.uniform(size=(P, P)) < 0.1)
    ious = np.maximum(ious, ious.T).astype(np.float32)
    scores = rng.uniform(size=P).astype(np.float32)
    scores[5] = scores[17]
    got = host(H.nms(dev(ious, cuda), dev(scores, cuda), 0.3))
    assert np.array_equal(got, O.nms(ious, scores, 0.3))


# ------------------------------------------------------------------------------------------------ F
def test_pointnet2_family(H, cuda):
    rng = np.random.default_rng(12)
    b, n, m, c = 2, 3000, 500, 8
    xyz = rng.uniform(-1, 1, (b, n, 3)).astype(np.float32)
    new_xyz = xyz[:, :m].copy()
    idx = host(H.pn2_ball_query(0.2, 32, dev(xyz, cuda), dev(new_xyz, cuda)))
    assert np.array_equal(idx, O.pn2_ball_query(0.2, 32, xyz, new_xyz))
    feats = rng.normal(size=(b, c, n)).astype(np.float32)
    grouped = host(H.pn2_group_points(dev(feats, cuda), dev(idx, cuda)))
    assert np.array_equal(grouped, O.pn2_group_points(feats, idx))
    gg = rng.normal(size=grouped.shape).astype(np.float32)
    assert np.allclose(host(H.pn2_group_points_grad(dev(gg, cuda), dev(idx, cuda), n)), O.pn2_group_points_grad(gg, idx, n), atol=1e-4)
    fps = host(H.pn2_furthest_point_sampling(dev(xyz, cuda), 256))
    assert np.array_equal(fps, O.pn2_furthest_point_sampling(xyz, 256))
    gathered = host(H.pn2_gather_points(dev(feats, cuda), dev(fps, cuda)))
    assert np.array_equal(gathered, O.pn2_gather_points(feats, fps))
    g2 = rng.normal(size=gathered.shape).astype(np.float32)
    assert np.allclose(host(H.pn2_gather_points_grad(dev(g2, cuda), dev(fps, cuda), n)), O.pn2_gather_points_grad(g2, fps, n), atol=1e-5)
    known = xyz[:, fps[0]][:, :256] if False else np.stack([xyz[i, fps[i]] for i in range(b)])
    d2, i3 = H.pn2_three_nn(dev(xyz, cuda), dev(known, cuda))
    rd2, ri3 = O.pn2_three_nn(xyz, known)
    assert np.array_equal(host(i3), ri3) and np.array_equal(host(d2), rd2)
    kd2, ki = H.pn2_knn(dev(xyz[:, :400], cuda), dev(known, cuda), 5)
    rkd2, rki = O.pn2_knn(xyz[:, :400], known, 5)
    assert np.array_equal(host(ki), rki) and np.array_equal(host(kd2), rkd2)
    w = rng.uniform(size=(b, n, 3)).astype(np.float32)
    kf = rng.normal(size=(b, c, 256)).astype(np.float32)
    interp = host(H.pn2_three_interpolate(dev(kf, cuda), dev(ri3, cuda), dev(w, cuda)))
    assert np.array_equal(interp, O.pn2_three_interpolate(kf, ri3, w))
    gi = rng.normal(size=interp.shape).astype(np.float32)
    assert np.allclose(host(H.pn2_three_interpolate_grad(dev(gi, cuda), dev(ri3, cuda), dev(w, cuda), 256)),
                       O.pn2_three_interpolate_grad(gi, ri3, w, 256), atol=1e-3)


def test_fps_tie_break_small_cloud(H, cuda):
    # regular grid -> many exact distance ties; n = 1000 -> reference block size 512
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)
    assert np.array_equal(host(H.pn2_furthest_point_sampling(dev(g, cuda), 64)), O.pn2_furthest_point_sampling(g, 64))


# ------------------------------------------------------------------------------------------------ BN
@pytest.mark.parametrize("N,C,relu,with_res,training", [(20000, 16, True, True, True), (777, 48, True, False, True),
                                                          (136, 112, False, False, True), (5000, 32, True, True, False),
                                                          (3, 16, True, False, True), (1024, 64, True, True, True),
                                                          (1025, 16, True, True, True), (900, 20, True, True, True),
                                                          (3000, 224, True, True, True), (2000, 320, True, False, True),
                                                          (1500, 768, True, True, True)])
def test_fused_batchnorm_matches_torch(H, cuda, N, C, relu, with_res, training):
    """fp32 torch.nn.functional.batch_norm (+ add + relu) is the reference for this floating-point kernel family;
    tolerance 1e-4 (north_star) on outputs, 1e-3 relative on the reduced parameter gradients."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(N + C)
    x = (torch.randn(N, C, generator=g) * 2 + 0.5).to(cuda).requires_grad_(True)
    res = torch.randn(N, C, generator=g).to(cuda).requires_grad_(True) if with_res else None
    w = (torch.rand(C, generator=g) + 0.5).to(cuda).requires_grad_(True)
    b = torch.randn(C, generator=g).to(cuda).requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g).to(cuda) * 0.1, (torch.rand(C, generator=g) + 0.5).to(cuda)
    rm, rv = rm0.clone(), rv0.clone()
    ref = F.batch_norm(x, rm, rv, w, b, training=training, momentum=0.1, eps=1e-4)
    if with_res:
        ref = ref + res
    if relu:
        ref = F.relu(ref)
    dy = torch.randn(N, C, generator=g).to(cuda)
    grads_ref = torch.autograd.grad(ref, [x, w, b] + ([res] if with_res else []), dy)
    rm2, rv2 = rm0.clone(), rv0.clone()
    y, mean, invstd = H.bn_fwd(x.detach(), None if res is None else res.detach(), w.detach(), b.detach(), rm2, rv2,
                               training, 0.1, 1e-4, relu)
    assert torch.allclose(y, ref.detach(), atol=1e-4, rtol=1e-4)
    if training and N > 1:
        assert torch.allclose(rm2, rm, atol=1e-5) and torch.allclose(rv2, rv, atol=1e-4, rtol=1e-4)
    dx, dres, dw, db = H.bn_bwd(x.detach(), y, dy, w.detach(), mean, invstd, relu, training, with_res)
    assert torch.allclose(dx, grads_ref[0], atol=2e-4, rtol=1e-3)
    assert torch.allclose(dw, grads_ref[1], atol=1e-3 * max(1.0, float(grads_ref[1].abs().max())), rtol=1e-3)
    assert torch.allclose(db, grads_ref[2], atol=1e-3 * max(1.0, float(grads_ref[2].abs().max())), rtol=1e-3)
    if with_res:
        assert torch.allclose(dres, grads_ref[3], atol=1e-6)


def test_conv_parameter_layout_matches_canonical(H, cuda):
    """weights given in the spconv-2.x parameter layout [Cout, K, Cin] (no permute/copy) == canonical [K, Cin, Cout]"""
    rng = np.random.default_rng(21)
    shape = [40, 40, 40]
    idx = synth.surface_indices(rng, 2, shape, 1500)
    N = idx.shape[0]
    f = dev(rng.normal(size=(N, 32)).astype(np.float32), cuda)
    g = dev(rng.normal(size=(N, 48)).astype(np.float32), cuda)
    W = dev((rng.normal(size=(27, 32, 48)) / 30).astype(np.float32), cuda)
    Wp = W.permute(2, 0, 1).contiguous()
    rb = H.rulebook_subm3(dev(idx, cuda), shape)
    assert torch.equal(H.conv_fwd(f, W, rb), H.conv_fwd(f, Wp, rb, "oki"))
    assert torch.equal(H.conv_dgrad(g, W, rb, rb, True), H.conv_dgrad(g, Wp, rb, rb, True, "oki"))
    assert torch.equal(H.conv_wgrad(f, g, rb).permute(2, 0, 1), H.conv_wgrad(f, g, rb, "oki"))


@pytest.mark.parametrize("n,cin,cout", [(20000, 16, 10), (5000, 32, 27), (4096, 16, 16), (513, 16, 3), (1, 64, 64), (37, 16, 27)])
@pytest.mark.parametrize("bias", [True, False])
def test_dense_heads_match_torch(H, cuda, n, cin, cout, bias):
    """GF.linear on the library's own head kernels (csrc/linear.hip: gpn_linear_fwd / gpn_linear_bwd) vs a float64
    F.linear: values and the three gradients at 1e-5 relative to the tensor's largest entry; two runs bit-equal (fixed-order
    sums); outputs that are not needed are not computed"""
    import torch.nn.functional as F
    from gapartnet_amd import functional as GF
    assert H.linear_supported(cin, cout)
    g = torch.Generator().manual_seed(n + cout)
    x = torch.randn(n, cin, generator=g).to(cuda).requires_grad_(True)
    w = (torch.randn(cout, cin, generator=g) * 0.2).to(cuda).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(cuda).requires_grad_(True) if bias else None
    dy = torch.randn(n, cout, generator=g).to(cuda)
    leaves = [x, w] + ([b] if bias else [])
    ref = F.linear(x.double(), w.double(), b.double() if bias else None)
    gref = torch.autograd.grad(ref, leaves, dy.double())
    got = GF.linear(x, w, b)
    ggot = torch.autograd.grad(got, leaves, dy)

    def close(a, r):
        return torch.allclose(a.double(), r.double(), rtol=0, atol=1e-5 * max(1.0, float(r.abs().max())))
    assert close(got, ref)
    for a, r in zip(ggot, gref):
        assert close(a, r)
    again = torch.autograd.grad(GF.linear(x, w, b), leaves, dy)
    assert all(torch.equal(a, c) for a, c in zip(ggot, again)), "fixed summation order"
    dx, dw, db = H.linear_bwd(x.detach(), w.detach(), dy, False, True, False)
    assert dx is None and db is None and torch.equal(dw, ggot[1])


@pytest.mark.parametrize("P,I,labels64", [(300, 40, True), (7, 3, False), (1, 1, True), (2000, 64, False)])
def test_fused_score_loss_matches_the_torch_formulation(H, cuda, P, I, labels64):
    """gpn_score_loss (class selection, get_gt_scores on the row maxima of the IoU matrix, BCE-with-logits mean, sigmoid scores,
    gradient) vs the reference's chain of torch ops (model.py:560-566, 373-383; grouping_utils.py:144-156): targets are the
    same floats (mul then add), loss / scores / gradient at 1e-6"""
    import torch.nn.functional as F
    from gapartnet_amd import functional as GF
    from gapartnet_amd.network.grouping_utils import get_gt_scores
    g = torch.Generator().manual_seed(P + I)
    C1 = 9
    sizes = torch.randint(1, 50, (P,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(cuda)
    M = int(sizes.sum())
    cls = torch.randint(1, C1 + 1, (M,), generator=g).to(torch.int64 if labels64 else torch.int32).to(cuda)
    ious = torch.rand(P, I, generator=g).to(cuda)
    ious[::3] *= 0.2          # rows entirely below the background threshold
    ious[1::3, 0] = 0.9       # rows above the foreground threshold
    logits = (torch.randn(P, C1, generator=g) * 3).to(cuda).requires_grad_(True)
    sel = logits.gather(1, cls[offsets[:-1].long()].long()[:, None] - 1).squeeze(1)
    want = F.binary_cross_entropy_with_logits(sel, get_gt_scores(ious.max(-1)[0], 0.75, 0.25))
    (gw,) = torch.autograd.grad(want * 1.7, logits)
    assert GF.score_loss_available(logits)
    got, preds = GF.score_loss(logits, cls, offsets, ious, 0.75, 0.25)
    (gg,) = torch.autograd.grad(got * 1.7, logits)
    assert got.shape == want.shape and abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    assert torch.allclose(preds, sel.detach().sigmoid(), rtol=0, atol=1e-6) and not preds.requires_grad
    assert torch.allclose(gg, gw, rtol=0, atol=1e-6 * max(1.0, float(gw.abs().max())))
    again, _ = GF.score_loss(logits, cls, offsets, ious, 0.75, 0.25)
    assert torch.equal(again, got)


def test_linear_through_the_conv_kernels_matches_torch(H, cuda):
    """widths the head kernels do not take (> 64) keep the K = 1 case of the fused conv family (output channels zero-padded to
    16) vs F.linear, 1e-4"""
    import torch.nn.functional as F
    from gapartnet_amd import functional as GF
    n, cin, cout = 4096, 80, 10
    assert not H.linear_supported(cin, cout)
    g = torch.Generator().manual_seed(n + cout)
    x = torch.randn(n, cin, generator=g).to(cuda).requires_grad_(True)
    w = (torch.randn(cout, cin, generator=g) * 0.2).to(cuda).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(cuda).requires_grad_(True)
    dy = torch.randn(n, cout, generator=g).to(cuda)
    ref = F.linear(x, w, b)
    gref = torch.autograd.grad(ref, [x, w, b], dy)
    got = GF.linear(x, w, b)
    ggot = torch.autograd.grad(got, [x, w, b], dy)
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4)
    assert torch.allclose(ggot[0], gref[0], atol=1e-4, rtol=1e-4)
    assert torch.allclose(ggot[1], gref[1], atol=1e-3 * max(1.0, float(gref[1].abs().max())), rtol=1e-3)
    assert torch.allclose(ggot[2], gref[2], atol=1e-3 * max(1.0, float(gref[2].abs().max())), rtol=1e-3)


@pytest.mark.parametrize("case", ["surface", "dense", "labels", "far_queries"])
def test_grid_ball_query_is_bit_exact(H, cuda, case):
    """the grid-accelerated ball query (>= 2048 points) == the oracle's index-order scan: sparse neighbourhoods (ranked hit
    lists), dense ones (more hits than the per-wave list: in-kernel fallback scan, truncation at K), label filter, queries
    outside the points' bounding box, an empty segment"""
    rng = np.random.default_rng({"surface": 1, "dense": 2, "labels": 3, "far_queries": 4}[case])
    if case == "dense":
        centres = rng.uniform(-0.5, 0.5, (6, 3))
        pts = (centres[rng.integers(0, 6, 9000)] + rng.normal(scale=0.004, size=(9000, 3))).astype(np.float32)
        offs = np.array([0, 4000, 4000, 9000], np.int32)
        K, r = 300, 0.03
    else:
        pts, _ = synth.clustered_points(rng, 3, 3000)
        offs = np.array([0, 3000, 6000, 9000], np.int32)
        K, r = 50, 0.04
    batch = np.repeat(np.arange(3, dtype=np.int32), np.diff(offs))
    lab = rng.integers(1, 4, pts.shape[0]).astype(np.int32) if case == "labels" else None
    if case == "far_queries":
        q = np.concatenate([pts[::3] + 0.01, rng.uniform(-3, 3, (500, 3))]).astype(np.float32)
        qb = rng.integers(0, 3, q.shape[0]).astype(np.int32)
        ql = None
    else:
        q, qb, ql = pts, batch, lab
    ref_idx, ref_cnt = O.ball_query(pts, q, qb, offs, r, K, lab, ql)
    idx, cnt = H.ball_query(dev(pts, cuda), dev(q, cuda), dev(qb, cuda), dev(offs, cuda), r, K,
                            None if lab is None else dev(lab, cuda), None if ql is None else dev(ql, cuda))
    assert np.array_equal(host(cnt), ref_cnt)
    assert np.array_equal(host(idx), ref_idx)
    if case == "dense":
        assert (ref_cnt == K).mean() > 0.5, "the dense case must exercise truncation"


@pytest.mark.parametrize("block", [16384, 8192, 4096, 1024, 512])
def test_tile_order_is_the_stable_sort_by_neighbour_mask(H, cuda, block):
    """gpn_rulebook_tile_order: inside every block of `block` rows the rows are ordered by their K-bit neighbour mask, equal
    masks in ascending row order (blocks of 4096 / 8192 / 16384 rows are sorted in one workgroup's LDS, other sizes by the
    device-wide sort: same permutation); perm is padded with the last row, the permuted table ends in the -1 sentinel"""
    import ctypes
    from gapartnet_amd import _C
    rng = np.random.default_rng(block)
    shape = [96, 96, 96]
    idx = dev(synth.surface_indices(rng, 3, shape, 7000), cuda)
    n = idx.shape[0]
    assert n % 16 != 0, "a ragged last tile: the padding checks below need one (all five seeds give one)"
    rb = H.rulebook_subm3(idx, shape)
    K = 27
    perm = torch.empty(((n + 15) // 16 * 16 + 16,), dtype=torch.int32, device=cuda)
    nbr_p = torch.empty((K * n + 1,), dtype=torch.int32, device=cuda)
    L = _C.lib()
    ws = torch.empty((int(L.gpn_rulebook_tile_order_ws_bytes(H.i64(n))),), dtype=torch.uint8, device=cuda)
    rc = L.gpn_rulebook_tile_order(H.ptr(rb.nbr), H.i32(K), H.i64(n), H.i32(block), H.ptr(perm), H.ptr(nbr_p), H.ptr(ws),
                                   H.szt(ws.numel()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.gpn_last_error()
    table = host(rb.nbr[:K * n].view(K, n))
    mask = np.zeros(n, np.int64)
    for k in range(K):
        mask |= (table[k] >= 0).astype(np.int64) << k
    want = np.lexsort((np.arange(n), mask, np.arange(n) // block))  # by block, then mask, then row (stable)
    assert np.array_equal(host(perm[:n]), want)
    assert np.all(host(perm[n:]) == n - 1)
    assert np.array_equal(host(nbr_p[:K * n].view(K, n)), table[:, want]) and int(nbr_p[K * n]) == -1


def test_tile_ordered_conv_is_bit_equal(H, cuda):
    """the rulebook's tile order (rows sorted by neighbour mask inside 16384-row blocks) changes which taps a tile skips,
    not a single output bit: forward and dgrad through (nbr_p, perm) == through the plain table"""
    import ctypes
    from gapartnet_amd import _C
    rng = np.random.default_rng(5)
    shape = [160, 160, 160]
    idx = dev(synth.surface_indices(rng, 4, shape, 9000), cuda)
    n = idx.shape[0]
    rb = H.rulebook_subm3(idx, shape)
    if rb.perm is None:  # the order is an option of the rulebook builder (off by default since the direct conv kernel)
        rb.perm, rb.nbr_p = H.tile_order(rb.nbr, 27, n)
    assert rb.perm is not None and rb.nbr_p is not None
    perm = rb.perm[:n].long()
    assert torch.equal(torch.sort(perm)[0], torch.arange(n, device=cuda)), "perm is a permutation"
    assert torch.equal(rb.nbr_p[:27 * n].view(27, n), rb.nbr[:27 * n].view(27, n)[:, perm])
    blocks = perm // H.TILE_ORDER_BLOCK
    assert torch.equal(blocks, torch.sort(blocks)[0]), "rows stay inside their 16384-row block"
    L = _C.lib()
    for cin, cout in ((16, 16), (32, 32), (48, 48)):
        x = dev(rng.normal(size=(n, cin)).astype(np.float32), cuda)
        w = dev((rng.normal(size=(27, cin, cout)) / 20).astype(np.float32), cuda)
        for flags in (0, H.PACK_TRANSPOSE | H.PACK_REVERSE):  # forward, and dgrad (same table, reversed transposed weights)
            packed = H.pack_weights(w, flags)
            outs = []
            for ordered in (False, True):
                out = torch.empty((n, cout), dtype=torch.float32, device=cuda)
                ws = torch.empty((64 << 20,), dtype=torch.uint8, device=cuda)
                rc = L.gpn_spconv_fwd_ordered(
                    H.ptr(x), H.ptr(packed), H.ptr(rb.nbr), H.ptr(rb.nbr_p if ordered else None),
                    H.ptr(rb.perm if ordered else None), H.i32(27), H.i64(n), H.i32(cin), H.i32(cout), H.ptr(out),
                    H.ptr(ws), H.szt(ws.numel()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, L.gpn_last_error()
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), (cin, cout, flags)
        packed = H.pack_weights(w, 0)
        outs = []
        for ordered in (False, True):
            out = torch.empty((n, cout), dtype=torch.float32, device=cuda)
            ws = torch.empty((64 << 20,), dtype=torch.uint8, device=cuda)
            rc = L.gpn_spconv_fwd_ordered(
                H.ptr(x), H.ptr(packed), H.ptr(rb.nbr), H.ptr(rb.nbr_p if ordered else None),
                H.ptr(rb.perm if ordered else None), H.i32(27), H.i64(n), H.i32(cin), H.i32(cout), H.ptr(out), H.ptr(ws),
                H.szt(ws.numel()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, L.gpn_last_error()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), (cin, cout)
        assert torch.equal(outs[0], H.conv_fwd(x, w, rb))


def test_empty_and_degenerate_inputs(H, cuda):
    """zero-sized inputs through every operator of the path: same shapes / values as the oracle, no launch errors"""
    f32, i32, i64 = np.float32, np.int32, np.int64
    e3 = np.zeros((0, 3), f32)
    # V: no points (one empty segment)
    got = H.voxelize(dev(e3, cuda), dev(np.zeros((0, 4), f32), cuda), dev(np.array([0, 0], i64), cuda),
                     dev(np.zeros((1, 3), f32), cuda), dev(np.ones((1, 3), f32), cuda), [0.1] * 3, [11] * 3)
    assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[3].shape == (0,)
    # K1 / K2: no voxels
    idx0 = dev(np.zeros((0, 4), i32), cuda)
    rb = H.rulebook_subm3(idx0, [8, 8, 8])
    assert rb.n_dst == 0 and int(rb.num_pairs.item()) == 0
    out_idx, out_shape, rb_f, rb_b = H.rulebook_down(idx0, [8, 8, 8], 1)
    assert out_idx.shape == (0, 4) and out_shape == [4, 4, 4] and rb_f.n_dst == 0
    assert H.rulebook_level_counts(idx0, [8, 8, 8], 1, 3).tolist() == [0, 0, 0]
    # C: a conv over nothing, and over one isolated voxel (only the centre tap exists)
    w = dev(np.ones((27, 16, 16), f32), cuda)
    assert H.conv_fwd(dev(np.zeros((0, 16), f32), cuda), w, rb).shape == (0, 16)
    one = dev(np.array([[0, 3, 3, 3]], i32), cuda)
    rb1 = H.rulebook_subm3(one, [8, 8, 8])
    ref1 = O.rulebook_subm3(host(one), [8, 8, 8])
    _check_rb(rb1, ref1)
    x1 = dev(np.arange(16, dtype=f32)[None], cuda)
    assert torch.equal(H.conv_fwd(x1, w, rb1), torch.full((1, 16), float(np.arange(16).sum()), device=cuda))
    # G
    assert H.gather_rows(dev(np.ones((5, 8), f32), cuda), dev(np.zeros((0,), i32), cuda)).shape == (0, 8)
    assert torch.equal(H.scatter_rows(dev(np.zeros((0, 8), f32), cuda), dev(np.zeros((0,), i32), cuda), 5),
                       torch.zeros((5, 8), device=cuda))
    # B / L: no queries
    idx, cnt = H.ball_query(dev(np.zeros((4, 3), f32), cuda), dev(e3, cuda), dev(np.zeros((0,), i32), cuda),
                            dev(np.array([0, 4], i32), cuda), 0.1, 8)
    assert idx.shape == (0, 8) and cnt.shape == (0,)
    assert H.ccl(dev(np.zeros((0,), i32), cuda), dev(np.zeros((0,), i32), cuda)).shape == (0,)
    # R / I / N: no proposals
    v = dev(np.ones((6, 4), f32), cuda)
    z = dev(np.zeros((0,), i32), cuda)
    assert H.segmented_reduce(v, z, z, "sum").shape == (0, 4)
    p, a = H.segmented_maxpool_fwd(v, z, z)
    assert p.shape == (0, 4) and a.shape == (0, 4)
    assert H.nms(dev(np.zeros((0, 0), f32), cuda), dev(np.zeros((0,), f32), cuda), 0.3).shape == (0,)
    # an empty segment among non-empty ones keeps its slot (sum 0, min/max = the oracle's convention)
    b, e = np.array([0, 3, 3], i32), np.array([3, 3, 6], i32)
    for mode in ("sum", "min", "max"):
        assert np.array_equal(host(H.segmented_reduce(v, dev(b, cuda), dev(e, cuda), mode)),
                              O.segmented_reduce(host(v), b, e, mode)), mode


def test_voxel_mean_gradient_on_the_gpu(H, cuda):
    """the differentiable voxelize wrapper on the HIP kernels == on the oracle (forward bit-exact, gradient 1e-6)"""
    from gapartnet_amd import backend, functional as GF
    from oracle import torch_ops
    rng = np.random.default_rng(12)
    pts = rng.uniform(0, 16, (5000, 3)).astype(np.float32)
    feats = rng.normal(size=(5000, 16)).astype(np.float32)
    offs = np.array([0, 1000, 5000], np.int64)
    res = []
    for on_gpu in (False, True):
        d = cuda if on_gpu else torch.device("cpu")
        f = torch.from_numpy(feats).to(d).requires_grad_(True)
        args = (torch.from_numpy(pts).to(d), f, torch.from_numpy(offs).to(d), torch.zeros((1, 3), device=d),
                torch.full((1, 3), 16.0, device=d), [1.0, 1.0, 1.0], [17, 17, 17])
        if on_gpu:
            out = GF.voxelize_mean(*args)
        else:
            with backend.using(torch_ops):
                out = GF.voxelize_mean(*args)
        vf = out[0]
        w = torch.linspace(-1, 1, vf.numel(), device=d).view_as(vf)
        if on_gpu:
            (vf * w).sum().backward()
        else:
            with backend.using(torch_ops):
                (vf * w).sum().backward()
        res.append((vf.detach().cpu(), out[3].cpu(), f.grad.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.allclose(res[0][2], res[1][2], atol=1e-6)


@pytest.mark.parametrize("case", ["normal", "ignored_rows", "no_part_points", "zero_offsets"])
def test_fused_point_losses_match_the_torch_formulas(H, cuda, case):
    """kernel family P vs the plain-torch losses it replaces (focal_loss + dice_loss + loss_offset, themselves pinned to
    the reference by tests/golden): values 1e-5 relative, gradients 1e-4 relative"""
    from gapartnet_amd import functional as GF
    from gapartnet_amd.network.losses import dice_loss, focal_loss
    g = torch.Generator().manual_seed(7)
    M, C = 30000, 10
    logits = (torch.randn(M, C, generator=g) * 2).to(cuda).requires_grad_(True)
    offsets = (torch.randn(M, 3, generator=g) * 0.1).to(cuda)
    if case == "zero_offsets":
        offsets[::5] = 0.0
    offsets.requires_grad_(True)
    gt = (torch.randn(M, 3, generator=g) * 0.1).to(cuda)
    labels = torch.randint(0, C, (M,), generator=g).to(cuda)
    inst = torch.randint(-1, 6, (M,), generator=g).to(torch.int32).to(cuda)
    if case == "no_part_points":
        labels.zero_()
    wts = torch.tensor([0.7, 1.3, 0.9, 1.1], device=cuda)

    def reference(lab_for_focal):
        on = (labels > 0) & (inst >= 0)
        cnt = on.sum()
        zero = offsets.new_zeros(())
        l_dist = torch.where(on, (offsets - gt).abs().sum(-1), zero).sum() / cnt
        gdir = gt / (torch.norm(gt, p=2, dim=-1)[:, None] + 1e-8)
        pdir = offsets / (torch.norm(offsets, p=2, dim=-1)[:, None] + 1e-8)
        l_dir = torch.where(on, -(gdir * pdir).sum(-1), zero).sum() / cnt
        return torch.stack([focal_loss(logits, lab_for_focal, gamma=2.0, ignore_index=-100),
                            dice_loss(logits[:, :, None, None], labels[:, None, None]), l_dist, l_dir])

    lab_focal = labels.clone()
    if case == "ignored_rows":
        lab_focal[::3] = -100
    if case == "ignored_rows":
        # the fused op takes ONE label vector: ignored rows are also class-less for dice (one-hot = smoothing only)
        want = reference(lab_focal)
        keep = lab_focal != -100
        y = torch.zeros((M, C), device=cuda).scatter_(1, labels[:, None], 1.0) * keep[:, None] + 1e-6
        p = torch.softmax(logits, 1)
        want = torch.stack([want[0], (1 - 2 * (p * y).sum(1) / ((p + y).sum(1) + 1e-8)).mean(), want[2], want[3]])
        # offsets use labels > 0: -100 rows are off-part
        on = (lab_focal > 0) & (inst >= 0)
        cnt = on.sum()
        zero = offsets.new_zeros(())
        gdir = gt / (torch.norm(gt, p=2, dim=-1)[:, None] + 1e-8)
        pdir = offsets / (torch.norm(offsets, p=2, dim=-1)[:, None] + 1e-8)
        want = torch.stack([want[0], want[1], torch.where(on, (offsets - gt).abs().sum(-1), zero).sum() / cnt,
                            torch.where(on, -(gdir * pdir).sum(-1), zero).sum() / cnt])
    else:
        want = reference(lab_focal)
    got = GF.point_losses(logits, offsets, lab_focal, gt, inst, -100)
    if case == "no_part_points":
        assert torch.isnan(got[2]) and torch.isnan(got[3]) and torch.isnan(want[2])
        assert torch.allclose(got[:2], want[:2], rtol=1e-5, atol=1e-6)
        gg = torch.autograd.grad((got[:2] * wts[:2]).sum(), [logits])[0]
        gw = torch.autograd.grad((want[:2] * wts[:2]).sum(), [logits])[0]
        assert torch.allclose(gg, gw, rtol=1e-4, atol=1e-9)
        return
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (got, want)
    gg = torch.autograd.grad((got * wts).sum(), [logits, offsets])
    gw = torch.autograd.grad((want * wts).sum(), [logits, offsets])
    assert torch.allclose(gg[0], gw[0], rtol=1e-4, atol=1e-9)
    assert torch.allclose(gg[1], gw[1], rtol=1e-4, atol=1e-9)


@pytest.mark.gpu
def test_fps_big_cloud_shared_by_workgroups(H, cuda):
    """>= 65536 points: several workgroups share a cloud (counter barrier per sample); the samples are those of the
    single-workgroup kernel and of the oracle, including ties (a grid of points has many equal distances)"""
    rng = np.random.default_rng(3)
    n = 70000
    cloud = rng.random((n, 3)).astype(np.float32)
    side = int(round(n ** (1 / 3))) + 1
    gx = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * 0.25
    xyz = np.stack([cloud, gx])
    got = host(H.pn2_furthest_point_sampling(dev(xyz, cuda), 300))
    assert np.array_equal(got, O.pn2_furthest_point_sampling(xyz, 300))
    # the plain entry point (one workgroup per cloud) on the same input
    t = torch.from_numpy(xyz).to(cuda)
    temp = torch.full((2, n), 1e10, dtype=torch.float32, device=cuda)
    idx = torch.zeros((2, 300), dtype=torch.int32, device=cuda)
    from gapartnet_amd import _C
    rc = _C.lib().gpn_pn2_furthest_point_sampling(2, n, 300, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(temp.data_ptr()),
                                                  ctypes.c_void_p(idx.data_ptr()),
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and np.array_equal(idx.cpu().numpy(), got)


def fps_batch_clouds(n=65536):
    """[3, n, 3]: a random cloud, a 0.25-spaced grid (many distances exactly equal), n copies of one point (all distances equal)"""
    rng = np.random.default_rng(11)
    side = int(np.ceil(n ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * 0.25
    same = np.tile(np.array([[0.5, -1.25, 2.0]], dtype=np.float32), (n, 1))
    return np.stack([rng.random((n, 3)).astype(np.float32), grid, same])


@pytest.mark.gpu
def test_fps_batch_of_clouds_shared_by_workgroups(cuda):
    """A batch of clouds of 65536 points, the smallest size at which gpn_pn2_furthest_point_sampling_ws shares a cloud between
    workgroups: one kernel serves (cloud, member) pairs, so the members of three clouds meet at three counters at once.  The
    samples are those of the plain entry point (one workgroup per cloud, the same kernel without meetings) and of the oracle;
    a second call on the same workspace gives them again (the arrival counters are zeroed by every call).  What it cannot see:
    a non-empty workspace says that the host chose G > 1, not that the cooperative launch was accepted - had the runtime refused
    it, the library would have run one workgroup per cloud and all three runs would have taken that form (as in
    test_fps_big_cloud_shared_by_workgroups; the library has no way to observe the fallback)."""
    from gapartnet_amd import _C
    L = _C.lib()
    b, n, m = 3, 65536, 40
    xyz = fps_batch_clouds(n)
    want = O.pn2_furthest_point_sampling(xyz, m)
    t = torch.from_numpy(xyz).to(cuda)
    vp, stream = ctypes.c_void_p, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_bytes = L.gpn_pn2_furthest_point_sampling_ws_bytes(b, n)
    assert ws_bytes > 0  # (several workgroups per cloud)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)

    def run(shared):
        temp = torch.full((b, n), 1e10, dtype=torch.float32, device=cuda)
        idx = torch.full((b, m), -1, dtype=torch.int32, device=cuda)
        args = [b, n, m, vp(t.data_ptr()), vp(temp.data_ptr()), vp(idx.data_ptr())]
        if shared:
            rc = L.gpn_pn2_furthest_point_sampling_ws(*args, vp(ws.data_ptr()), ctypes.c_size_t(ws_bytes), stream)
        else:
            rc = L.gpn_pn2_furthest_point_sampling(*args, stream)
        assert rc == 0
        return idx.cpu().numpy()

    first, again, plain = run(True), run(True), run(False)
    assert np.array_equal(first, want)
    assert np.array_equal(again, want)
    assert np.array_equal(plain, want)


def test_copy_many_segments_in_one_launch(H, cuda):
    """gpn_copy_many (section O): any number of fp32 segments - more than one launch's 96, empty ones, odd lengths - land
    in their destinations; used by FusedAdam for the gradients autograd allocates afresh every step"""
    from gapartnet_amd import optim
    rng = np.random.default_rng(3)
    sizes = [0, 1, 3, 64, 4097, 70000] + [int(n) for n in rng.integers(1, 3000, size=120)]
    srcs = [torch.randn(n, device=cuda) for n in sizes]
    dsts = [torch.full((n,), -7.0, device=cuda) for n in sizes]
    optim._copy_many(dsts, srcs)
    for d, s_ in zip(dsts, srcs):
        assert torch.equal(d, s_)
    # a pair the fast path cannot take (non-contiguous source) falls back to torch for the whole list
    src2 = torch.randn(8, 6, device=cuda).t()
    dst2 = torch.zeros(6, 8, device=cuda)
    optim._copy_many([dst2, dsts[4]], [src2, srcs[5][:4097]])
    assert torch.equal(dst2, src2) and torch.equal(dsts[4], srcs[5][:4097])


def test_point_losses_emit_predictions_and_accuracies(H, cuda):
    """gpn_point_losses_fwd_metrics: the losses of gpn_point_losses_fwd bit for bit, plus torch.argmax of the logits (first
    maximum on ties) and the two accuracies exactly as network/model.py:535-541 forms them"""
    rng = np.random.default_rng(11)
    M, C = 5000, 10
    logits = torch.from_numpy(rng.normal(size=(M, C)).astype(np.float32)).to(cuda)
    logits[::7, 3] = logits[::7].max(dim=1).values  # ties: the first maximum wins
    labels = torch.from_numpy(rng.integers(0, C, size=M)).to(cuda)
    labels[::5] = 0
    off = torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)).to(cuda)
    gt = torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)).to(cuda)
    inst = torch.from_numpy(rng.integers(-1, 6, size=M).astype(np.int32)).to(cuda)
    base, _ = H.point_losses_fwd(logits, labels, off, gt, inst, -100)
    losses, _, preds, accu = H.point_losses_fwd(logits, labels, off, gt, inst, -100, metrics=True)
    assert torch.equal(losses, base)
    want = torch.argmax(logits, dim=-1)
    assert preds.dtype == torch.int64 and torch.equal(preds, want)
    all_accu = (want == labels).sum().float() / M
    on_part = labels > 0
    pixel_accu = ((want == labels) & on_part).sum() / on_part.sum()
    assert torch.equal(accu[0], all_accu) and torch.equal(accu[1], pixel_accu)
