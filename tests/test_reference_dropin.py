"""Drop-in check against the reference's OWN glue code: the reference's `network/backbone.py` and
`network/grouping_utils.py`, imported unmodified with this repo's mirrors registered under the names `spconv.pytorch` /
`epic_ops.*` (oracle raw-op backend), were run on the inputs below and their outputs recorded in
tests/golden/reference_dropin.npz (tests/golden/make_golden_dropin.py; the weights as checksums of their seeded
initialisation).  This repo's re-implementation of that glue must give the same results (same weights, same inputs,
oracle raw-op backend)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_dropin.npz")


@pytest.fixture()
def recorded():
    from gapartnet_amd import backend
    from oracle import torch_ops
    with np.load(GOLDEN) as d, backend.using(torch_ops):
        yield {k: d[k] for k in d.files}


def test_reference_backbone_runs_on_the_mirrors_and_matches(recorded):
    from gapartnet_amd.network.backbone import SparseUNet
    from gapartnet_amd.spconv import pytorch as spconv
    from tests import synth
    norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1)
    torch.manual_seed(0)
    mine = SparseUNet.build(6, [16, 32, 48], 2, norm_fn)
    sd = mine.state_dict()
    assert [str(k) for k in recorded["bb_keys"]] == list(sd.keys()), "the reference's module tree (state_dict keys)"
    # the weights the reference ran with: the same seeded initialisation, checked tensor by tensor against its sums
    assert np.allclose([v.double().sum().item() for v in sd.values()], recorded["bb_wsum"], rtol=1e-9, atol=1e-9)
    assert np.allclose([v.double().abs().sum().item() for v in sd.values()], recorded["bb_wabs"], rtol=1e-9, atol=1e-9)
    rng = np.random.default_rng(0)
    idx = synth.surface_indices(rng, 2, [40, 40, 40], 900)
    feats = rng.normal(size=(idx.shape[0], 6)).astype(np.float32)
    assert idx.shape[0] == int(recorded["bb_n"])
    x = spconv.SparseConvTensor(torch.from_numpy(feats), torch.from_numpy(idx), [40, 40, 40], 2)
    out = mine(x).features
    # same module tree and weights; this repo fuses BatchNorm + residual + ReLU into one op, so equality is to rounding
    assert torch.allclose(out, torch.from_numpy(recorded["bb_out"]), atol=1e-5, rtol=1e-5)


def test_reference_grouping_glue_matches(recorded):
    from gapartnet_amd.network import grouping_utils as G
    from tests import synth
    rng = np.random.default_rng(1)
    pts, batch = synth.clustered_points(rng, 2, 700, n_clusters=5)
    offs = torch.tensor([0, 700, 1400], dtype=torch.int32)
    sem = torch.from_numpy(rng.integers(1, 3, 1400).astype(np.int32))
    mine = G.cluster_proposals(torch.from_numpy(pts), torch.from_numpy(batch), offs, sem, 0.05, 30)
    assert torch.equal(mine[0], torch.from_numpy(recorded["cl_labels"]))  # labels; the reference's sort is unstable, so membership only:
    assert torch.equal(torch.sort(mine[1])[0], torch.from_numpy(recorded["cl_order_sorted"]).to(mine[1].dtype))
    # re-voxelisation with a pinned RNG: the reference draws torch.rand(3) twice
    labels, order = mine
    _, prop_idx, sizes = torch.unique_consecutive(labels, return_inverse=True, return_counts=True)
    offsets = G.offsets_from_counts(sizes)
    xyz = torch.from_numpy(pts)[order]
    feats = torch.from_numpy(rng.normal(size=(1400, 4)).astype(np.float32))
    torch.manual_seed(5)
    b = G.segmented_voxelize(xyz, feats, offsets, prop_idx, sizes, 28, 50)
    assert len(b) == int(recorded["vx_n"])
    for i, t_mine in enumerate(b):
        assert torch.equal(torch.from_numpy(recorded[f"vx_out{i}"]), t_mine)
    ious = torch.from_numpy(recorded["gt_ious"])
    assert torch.equal(torch.from_numpy(recorded["gt_scores"]), G.get_gt_scores(ious))
