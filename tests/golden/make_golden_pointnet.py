"""Generates tests/golden/pointnet_backbone.npz: what the reference's own ``PointNetBackbone(3, 16)`` - run UNMODIFIED on the
CPU - computes for B = 2 scenes of N = 300 points, in eval mode and in train mode.

    python tests/golden/make_golden_pointnet.py        (build container only: needs the reference tree)

The reference is imported at run time; only inputs, recorded outputs and lists of names are written, no reference source text.
Weights are not stored: they are the closed-form hash of tests/pointnet_ref.py (``hash_tensor``), which the tests rebuild.
Recorded: the input, the cotangent, the eval output; the train output, the gradients of sum(out * cotangent) with respect to the
input and to the parameters ``pointnet_ref.GRAD_PARAMS`` (gradients above 16384 elements as every stride-th flat element,
``pointnet_ref.recorded``), the running statistics of the BatchNorms ``pointnet_ref.STAT_BNS`` after that one training pass, and
the sorted state_dict names and shapes.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import pointnet_ref as R  # noqa: E402
from tests.golden.make_golden_pipeline import REF, install_reference_environment  # noqa: E402


def main():
    assert os.path.isdir(REF), "reference tree not present: fixtures can only be regenerated in the build container"
    install_reference_environment()
    from network.backbone import PointNetBackbone
    torch.manual_seed(0)
    B, n = R.FIXTURE_B, R.FIXTURE_N
    model = PointNetBackbone(3, 16).backbone
    names_shapes = sorted((k, tuple(v.shape)) for k, v in model.state_dict().items())
    model.load_state_dict(R.hash_state_dict(names_shapes), strict=True)
    points = R.hash_input(B, n)
    cotangent = (2.0 * R.hash_uniform("cotangent", B * n * 16) - 1.0).reshape(B * n, 16).astype(np.float32)
    out = {"input": points, "cotangent": cotangent,
           "state_dict": np.array(json.dumps([[k, list(s)] for k, s in names_shapes]))}

    model.eval()
    with torch.no_grad():  # (model.py:155 of the reference: points.reshape(-1, 6, N))
        out["eval.out"] = model(torch.from_numpy(points).reshape(-1, 6, n)).reshape(B * n, 16).numpy()

    model.train()
    pts = torch.from_numpy(points).clone().requires_grad_(True)
    y = model(pts.reshape(-1, 6, n)).reshape(B * n, 16)
    (y * torch.from_numpy(cotangent)).sum().backward()
    out["train.out"] = y.detach().numpy()
    out["train.grad.input"] = pts.grad.numpy()
    params = dict(model.named_parameters())
    for name in R.GRAD_PARAMS:
        out["train.grad." + name] = R.recorded(params[name].grad.numpy())
    sd = model.state_dict()
    for bn in R.STAT_BNS:
        for k in ("running_mean", "running_var"):
            out[f"train.stat.{bn}.{k}"] = sd[f"{bn}.{k}"].numpy()
    path = os.path.join(HERE, "pointnet_backbone.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
