"""csrc/proposals.hip section MP - gpn_mask_pack and gpn_proposals_from_masks - against the restatement of tests/mask_ref.py on the
same GPU inputs: every integer table and the voxel tables EQUAL (the tail is the code tests/test_gpu_proposals.py holds bit-equal to
segmented_voxelize)."""
import numpy as np
import pytest
import torch

from tests import mask_ref as MR

pytestmark = pytest.mark.gpu
JITTER = ([0.3, 0.6, 0.1], [0.5, 0.2, 0.9])
N_CLASSES, MIN_POINTS = 10, 5
FIELDS = ("valid_mask", "valid_indices", "sorted_indices", "point_indices", "proposal_indices", "batch_indices", "pt_xyz", "sem_preds",
          "sizes", "proposal_offsets", "proposal_mask")
OUT = FIELDS + ("voxel_coords", "pc_voxel_id", "point_order", "voxel_point_start")


def _xyz(counts, seed, cuda):
    rng = np.random.RandomState(seed)
    # (clouds around different centres, one extra column: a row stride of 4)
    pts = np.concatenate([rng.uniform(-1, 1, size=(c, 4)) + 3 * s for s, c in enumerate(counts)] or [np.zeros((0, 4))])
    return torch.from_numpy(pts.astype(np.float32)).to(cuda)[:, :3]


def _run(cuda, counts, masks, labels, xyz, sample_rows=None, min_points=MIN_POINTS, fullscale=28.0, max_scale=50.0, M_cap=None, new=None):
    """pack (checked against the restatement) + the stage through the binding"""
    from gapartnet_amd import hip_ops as H
    per = [int(m.shape[0]) for m in masks]
    tables = H.mask_tables(counts, per, cuda)
    base, first = [], 0
    for m in masks:
        base += [first + k * m.shape[1] for k in range(m.shape[0])]
        first += m.size
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks] or [np.zeros(0)]).astype(np.uint8) * 3).to(cuda)
    rows = None if sample_rows is None else torch.from_numpy(sample_rows).to(cuda)
    bits = H.mask_pack(flat, base, tables, rows)
    assert bits.shape == (sum(per), (max(list(counts) + [0]) + 63) // 64)
    assert np.array_equal(bits.cpu().numpy(), MR.pack(counts, masks, sample_rows)), "gpn_mask_pack"
    jitter = tuple(torch.tensor(j, device=cuda) for j in JITTER)
    lab = torch.from_numpy(np.concatenate(labels or [np.zeros(0)]).astype(np.int64)).to(cuda)
    built = H.proposals_from_masks(bits, tables, lab, xyz, N_CLASSES, min_points, fullscale, max_scale, jitter, M_cap=M_cap, _new=new)
    return built, jitter


def _check(cuda, counts, masks, labels, xyz, sample_rows=None, min_points=MIN_POINTS, fullscale=28.0, max_scale=50.0):
    built, jitter = _run(cuda, counts, masks, labels, xyz, sample_rows, min_points, fullscale, max_scale)
    st = MR.stage(xyz, counts, masks, labels, min_points, N_CLASSES, sample_rows)
    assert (built is None) == (st is None)
    if st is None:
        return None
    for f in FIELDS:
        a, b = built[f], st[f]
        assert a.dtype == b.dtype and a.shape == b.shape, (f, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a, b), f
    assert (built["Q"], built["M"], built["P"]) == (st["Q"], st["M"], st["P"]) and "member_slot" not in built
    assert torch.equal(built["valid_indices"][built["sorted_indices"]], built["point_indices"])
    _, vc, pid, (order, starts), dropped = MR.voxel_tables(st, xyz.contiguous(), fullscale, max_scale, jitter)
    assert built["dropped"] == dropped == 0 and built["V"] == vc.shape[0]
    assert torch.equal(built["voxel_coords"], vc) and torch.equal(built["pc_voxel_id"], pid)
    assert torch.equal(built["point_order"], order) and torch.equal(built["voxel_point_start"], starts)
    assert built["coarse"] == int(torch.unique(torch.cat([vc[:, :1], vc[:, 1:] // 2], 1), dim=0).shape[0])
    again, _ = _run(cuda, counts, masks, labels, xyz, sample_rows, min_points, fullscale, max_scale)
    for f in OUT:
        assert torch.equal(again[f], built[f]), ("rerun", f)
    return built


def _edge_masks(m, rng):
    """0 members, all, min_points - 1, exactly min_points, a random one twice, and (m >= 65) one point in five masks"""
    rows = [np.zeros(m, bool), np.ones(m, bool)]
    for n in (MIN_POINTS - 1, MIN_POINTS):
        if m >= n:
            r = np.zeros(m, bool)
            r[rng.choice(m, n, replace=False)] = True
            rows.append(r)
    r = rng.rand(m) < 0.4
    rows += [r, r.copy()]
    if m >= 65:
        for _ in range(5):
            r = rng.rand(m) < 0.2
            r[m - 2] = True
            rows.append(r)
    return np.stack(rows)


def test_scene_sizes_around_the_word_length(cuda):
    counts = [1, 63, 64, 65, 130]
    rng = np.random.RandomState(0)
    masks = [_edge_masks(m, rng) for m in counts]
    labels = [rng.randint(1, N_CLASSES, size=m.shape[0]) for m in masks]
    built = _check(cuda, counts, masks, labels, _xyz(counts, 1, cuda))
    kept = set(built["proposal_mask"].tolist())
    first = np.concatenate([[0], np.cumsum([m.shape[0] for m in masks])])
    assert not kept & set(range(first[0], first[1])), "a one-point scene keeps nothing"
    for s in range(1, 5):
        assert first[s] not in kept and first[s] + 1 in kept and first[s] + 2 not in kept and first[s] + 3 in kept
    shared = int(np.cumsum(counts)[-1] - 2)
    assert int((built["point_indices"] == shared).sum()) >= 6, "one point in (at least) five masks and the full one"


@pytest.mark.parametrize("fullscale", [28.0, 40.0])  # (the sort-free re-voxelisation; above 30 the sorting voxeliser)
def test_a_scene_without_masks_between_two_with(cuda, fullscale):
    counts = [65, 2048, 700]
    rng = np.random.RandomState(3)
    masks = [rng.rand(4, 65) < 0.5, np.zeros((0, 2048), bool), rng.rand(7, 700) < rng.uniform(0.01, 0.6, size=(7, 1))]
    labels = [rng.randint(1, N_CLASSES, size=m.shape[0]) for m in masks]
    built = _check(cuda, counts, masks, labels, _xyz(counts, 4, cuda), fullscale=fullscale)
    assert set(built["batch_indices"].tolist()) == {0, 2} and not bool(built["valid_mask"][65:65 + 2048].any())


def test_one_mask_none_and_all_dropped(cuda):
    rng = np.random.RandomState(5)
    xyz = _xyz([100], 6, cuda)
    built = _check(cuda, [100], [rng.rand(1, 100) < 0.5], [np.array([9])], xyz)
    assert built["P"] == 1
    assert _check(cuda, [100], [np.zeros((0, 100), bool)], [np.zeros(0, np.int64)], xyz) is None                     # K = 0
    few = np.zeros((2, 100), bool)
    few[0, :4] = True
    assert _check(cuda, [100], [few], [np.array([1, 2])], xyz) is None                                                 # all dropped
    assert _check(cuda, [100, 30], [few, np.zeros((0, 30), bool)], [np.array([1, 2]), np.zeros(0, np.int64)], _xyz([100, 30], 7, cuda)) is None


def test_a_label_outside_the_classes_raises(cuda):
    from gapartnet_amd import _C
    rng = np.random.RandomState(8)
    masks = [rng.rand(3, 100) < 0.5]
    for bad in (0, N_CLASSES, -1):
        with pytest.raises(_C.GpnError, match="label"):
            _run(cuda, [100], masks, [np.array([1, bad, 2])], _xyz([100], 9, cuda))


class _Guarded:
    """allocator for the binding's outputs: every buffer with 64 sentinel elements behind it"""
    PAD, MARK = 64, 90

    def __init__(self, device):
        self.device, self.bufs = device, []

    def __call__(self, shape, dtype):
        n = int(np.prod(shape))
        raw = torch.full((n + self.PAD,), self.MARK, dtype=torch.uint8 if dtype == torch.bool else dtype, device=self.device)
        self.bufs.append((raw, n))
        view = raw[:n].view(torch.bool) if dtype == torch.bool else raw[:n]
        return view.view(shape)

    def intact(self):
        return all(bool((raw[n:] == self.MARK).all()) for raw, n in self.bufs)


def test_a_capacity_below_the_member_total_raises_and_writes_nothing_past_it(cuda):
    from gapartnet_amd import _C
    counts = [65, 300]
    rng = np.random.RandomState(10)
    masks = [rng.rand(3, 65) < 0.5, rng.rand(4, 300) < 0.5]
    labels = [rng.randint(1, N_CLASSES, size=m.shape[0]) for m in masks]
    xyz = _xyz(counts, 11, cuda)
    total = int(sum(m.sum() for m in masks))
    guard = _Guarded(cuda)
    built, _ = _run(cuda, counts, masks, labels, xyz, M_cap=total, new=guard)       # exactly enough
    assert built["M"] == total and len(guard.bufs) == 15 and guard.intact()
    guard = _Guarded(cuda)
    with pytest.raises(_C.GpnError, match=f"{total} members"):
        _run(cuda, counts, masks, labels, xyz, M_cap=total - 1, new=guard)
    assert len(guard.bufs) == 15 and guard.intact(), "a write past the capacity"


@pytest.mark.parametrize("n_rows", [(1000, 1023, 1025)])
def test_pack_through_non_monotone_sample_rows(cuda, n_rows):
    """masks on the caller's raw rows (lengths that are no multiples of 64, each above the largest scene), gathered through sample_rows"""
    counts = [130, 64, 65]
    rng = np.random.RandomState(12)
    sample_rows = np.concatenate([rng.permutation(n)[:c] for n, c in zip(n_rows, counts)]).astype(np.int64)
    assert (np.diff(sample_rows[:130]) < 0).any()
    masks = [rng.rand(5, n) < 0.5 for n in n_rows]
    masks[1][0] = True
    masks[2][0] = False
    masks[2][0, np.setdiff1d(np.arange(n_rows[2]), sample_rows[194:])[:40]] = True    # members on unsampled rows only
    labels = [rng.randint(1, N_CLASSES, size=5) for _ in counts]
    built = _check(cuda, counts, masks, labels, _xyz(counts, 13, cuda), sample_rows=sample_rows)
    assert 10 not in built["proposal_mask"].tolist() and 5 in built["proposal_mask"].tolist()


def test_one_large_scene_crosses_every_per_pass_word_limit(cuda):
    """70 000 points = 1094 words: more than the 64 words a wave scans per pass and the 1024 entries of the scan kernel's pass"""
    counts = [70000]
    rng = np.random.RandomState(14)
    masks = [rng.rand(1, 70000) < 0.5]
    built = _check(cuda, counts, masks, [np.array([4])], _xyz(counts, 15, cuda))
    assert built["M"] == int(masks[0].sum()) and built["P"] == 1


def test_more_masks_than_one_tile_of_the_mask_scan(cuda):
    """1025 masks over a scene of 64 points, min_points = 1: the number of a kept mask, its first member slot and the count of
    unknown labels are carried across the 1024-mask tiles of the one-workgroup scan (the last mask sits in the second tile)"""
    from gapartnet_amd import _C
    counts, K = [64], 1025
    rng = np.random.RandomState(16)
    masks = [rng.rand(K, 64) < rng.choice([0.0, 0.02, 0.05], size=(K, 1))]
    masks[0][[0, 1023, 1024]] = False
    masks[0][0, :3] = masks[0][1023, 5:7] = masks[0][1024, 60:] = True
    sizes = masks[0].sum(1)
    assert (sizes == 0).sum() > 100 and (sizes > 0).sum() > 500 and sizes.max() < 12, "masks of a few points, many of them dropped"
    labels = [rng.randint(1, N_CLASSES, size=K)]
    xyz = _xyz(counts, 17, cuda)
    built = _check(cuda, counts, masks, labels, xyz, min_points=1)
    assert built["P"] == int((sizes > 0).sum()) and built["proposal_mask"][-1] == 1024 and built["sizes"][-1] == 4
    labels[0][[3, 1023, 1024]] = [0, N_CLASSES, -1]
    with pytest.raises(ValueError, match="label"):
        MR.stage(xyz, counts, masks, labels, 1, N_CLASSES)
    with pytest.raises(_C.GpnError, match="^proposals_from_masks: 3 mask"):
        _run(cuda, counts, masks, labels, xyz, min_points=1)
