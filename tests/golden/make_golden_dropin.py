"""Generates tests/golden/reference_dropin.npz for tests/test_reference_dropin.py: the reference's OWN glue code
(`network/backbone.py`, `network/grouping_utils.py`) imported unmodified, with this repo's mirrors registered under the
names `spconv.pytorch` / `epic_ops.*` and the oracle raw-op backend, run on the inputs the test uses.  The reference's outputs
(and checksums of the seeded weights) are written; no reference source text goes anywhere.

    python tests/golden/make_golden_dropin.py <reference checkout>/gapartnet
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_dropin.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(ref):
    assert os.path.isdir(os.path.join(ref, "network")), f"{ref}: not the reference's gapartnet/ directory"
    import gapartnet_amd.epic_ops as eo
    import gapartnet_amd.spconv
    import gapartnet_amd.spconv.pytorch
    from gapartnet_amd import backend
    from gapartnet_amd.network import grouping_utils as G
    from gapartnet_amd.network.backbone import SparseUNet
    from gapartnet_amd.spconv import pytorch as spconv
    from oracle import torch_ops
    from tests import synth
    sys.modules["spconv"] = gapartnet_amd.spconv
    sys.modules["spconv.pytorch"] = gapartnet_amd.spconv.pytorch
    sys.modules["epic_ops"] = eo
    for sub in ("voxelize", "ball_query", "ccl", "reduce", "iou", "nms"):
        sys.modules[f"epic_ops.{sub}"] = getattr(eo, sub)
    sys.path.insert(0, ref)
    out = {}
    with backend.using(torch_ops):
        import network.backbone as ref_backbone
        import network.grouping_utils as ref_grouping
        # ---- backbone: the reference's SparseUNet with this repo's weights
        norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1)
        torch.manual_seed(0)
        mine = SparseUNet.build(6, [16, 32, 48], 2, norm_fn)
        theirs = ref_backbone.SparseUNet.build(6, [16, 32, 48], 2, norm_fn)
        assert list(theirs.state_dict().keys()) == list(mine.state_dict().keys())
        theirs.load_state_dict(mine.state_dict())
        # (the weights themselves are not stored: the test rebuilds them from the same seed and checks these sums)
        out["bb_keys"] = np.array(list(mine.state_dict().keys()))
        out["bb_wsum"] = np.array([v.double().sum().item() for v in mine.state_dict().values()])
        out["bb_wabs"] = np.array([v.double().abs().sum().item() for v in mine.state_dict().values()])
        rng = np.random.default_rng(0)
        idx = synth.surface_indices(rng, 2, [40, 40, 40], 900)
        feats = rng.normal(size=(idx.shape[0], 6)).astype(np.float32)
        x = spconv.SparseConvTensor(torch.from_numpy(feats), torch.from_numpy(idx), [40, 40, 40], 2)
        out.update(bb_n=np.array(idx.shape[0]), bb_out=theirs(x).features.detach().numpy())
        # ---- grouping glue
        rng = np.random.default_rng(1)
        pts, batch = synth.clustered_points(rng, 2, 700, n_clusters=5)
        offs = torch.tensor([0, 700, 1400], dtype=torch.int32)
        sem = rng.integers(1, 3, 1400).astype(np.int32)
        labels, order = ref_grouping.cluster_proposals(torch.from_numpy(pts), torch.from_numpy(batch), offs, torch.from_numpy(sem),
                                                       0.05, 30)
        out.update(cl_labels=labels.numpy(), cl_order_sorted=torch.sort(order)[0].numpy().astype(np.int32))
        # re-voxelisation with a pinned RNG (the reference draws torch.rand(3) twice) on this repo's cluster order, as the test does
        my_labels, my_order = G.cluster_proposals(torch.from_numpy(pts), torch.from_numpy(batch), offs, torch.from_numpy(sem), 0.05, 30)
        _, prop_idx, sizes = torch.unique_consecutive(my_labels, return_inverse=True, return_counts=True)
        offsets = G.offsets_from_counts(sizes)
        xyz = torch.from_numpy(pts)[my_order]
        vfeats = rng.normal(size=(1400, 4)).astype(np.float32)
        torch.manual_seed(5)
        vox = ref_grouping.segmented_voxelize(xyz, torch.from_numpy(vfeats), offsets, prop_idx, sizes, 28, 50)
        out["vx_n"] = np.array(len(vox))
        for i, t in enumerate(vox):
            out[f"vx_out{i}"] = t.numpy()
        ious = torch.tensor([0.1, 0.3, 0.6, 0.8])
        out.update(gt_ious=ious.numpy(), gt_scores=ref_grouping.get_gt_scores(ious).numpy())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
