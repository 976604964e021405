"""PointNet segmentation backbone (reference: network/pointnet/pointnet_sem_seg.py:8-30): encoder, then four per-point
layers 1088 -> 512 -> 256 -> 256 -> fea_dim.

The reference concatenates each scene's 1024 global channels (repeated for every point) with the 64 per-point channels and runs
``conv1`` over the 1088-wide rows.  The global half is constant within a scene, so its product with ``conv1.weight[:, :1024]`` is
one [B, 512] row per scene; only the 64 -> 512 half runs per point, with that row added per scene.  The 1088-wide tensor is never
built, in training and inference alike, and per-point multiply-adds fall from 1 180 416 to 656 128.
"""
from typing import Optional, Sequence

import torch
import torch.nn as nn

from ... import backend
from ... import functional as GF
from .pointnet_utils import PointNetEncoder, Run, input_view


class PointNetSegBackbone(nn.Module):
    # False: the plain-torch formulation of the same graph on any device (what CPU tensors always take; the baseline of
    # tools/pointnet_bench.py)
    use_native_kernels = True

    def __init__(self, pc_dim, fea_dim):
        super().__init__()
        self.fea_dim = fea_dim
        self.feat = PointNetEncoder(global_feat=False, feature_transform=True, channel=3 + pc_dim)
        self.conv1 = torch.nn.Conv1d(1088, 512, 1)
        self.conv2 = torch.nn.Conv1d(512, 256, 1)
        self.conv3 = torch.nn.Conv1d(256, 256, 1)
        self.conv4 = torch.nn.Conv1d(256, self.fea_dim, 1)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.bn3 = nn.BatchNorm1d(256)

    def forward_rows(self, points: torch.Tensor, counts: Sequence[int], layout: str = "reference",
                     seg: Optional[GF.PointSegments] = None) -> torch.Tensor:
        """points [sum N, channels] row-major with ``counts`` points per scene -> features [sum N, fea_dim]"""
        channels = self.feat.conv1.weight.shape[1]
        if seg is None:
            seg = GF.PointSegments(counts, points.device)
        assert points.dim() == 2 and points.shape == (seg.N, channels), (tuple(points.shape), seg.N, channels)
        view = input_view(layout, seg, channels)
        native = self.use_native_kernels and GF.point_mlp_available(points, channels, 64)
        run = Run(seg, native, not self.training and not torch.is_grad_enabled())
        x = points.contiguous()
        g, pointfeat, _, _ = self.feat.encode_rows(run, x.view(-1) if view is not None else x, view)
        w = self.conv1.weight.view(512, 1088)
        w_global, w_point = w[:, :1024].contiguous(), w[:, 1024:].contiguous()
        if run.fused:
            per_scene, _ = backend.raw().pointmlp_fwd(g, w_global)
        else:
            per_scene = run.dense(g, w_global, per_point=False)  # [B, 512]: the scene-constant half of conv1
        h, _ = run.layer(pointfeat, self.conv1, self.bn1, True, G=per_scene, weight=w_point)
        h, _ = run.layer(h, self.conv2, self.bn2, True)
        h, _ = run.layer(h, self.conv3, self.bn3, True)
        if run.fused:
            out, _ = backend.raw().pointmlp_fwd(h, self.conv4.weight.view(self.fea_dim, -1), self.conv4.bias, offsets=seg.offsets,
                                                offsets_host=seg.host)
            return out
        return run.dense(h, self.conv4.weight.view(self.fea_dim, -1), self.conv4.bias)

    def forward(self, x):
        """the reference's contract: x [B, channels, N] -> [B, N, fea_dim]"""
        B, C, N = x.shape
        return self.forward_rows(x.contiguous().view(B * N, C), [N] * B, "reference").view(B, N, self.fea_dim)
