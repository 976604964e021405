"""PointNet encoder and its two spatial-transformer networks (reference: network/pointnet/pointnet_utils.py:10-133).

Same module tree, parameter / buffer names and shapes as the reference (``Conv1d`` weights [cout, cin, 1]), so its
``state_dict`` loads with ``strict=True``.  The forward functions are written on rows: activations are [points of all scenes,
channels] with the scenes as contiguous row segments (``functional.PointSegments``), per-scene quantities are [B, channels].

  * every Conv1d(k = 1) / Linear is one dense layer of csrc/pointmlp.hip (``functional.point_mlp``); ``fc1 .. fc3`` of the
    transformers are the same kernel on B rows;
  * the two ``torch.bmm`` with the predicted 3 x 3 / 64 x 64 transforms are layers with one weight matrix per scene; the 3 x 3
    one is folded into the first conv's weights (W_b = [W[:, :3] T_b^T, W[:, 3:]]), so the transformed points are never stored;
  * training: dense layer -> ``GF.bn_act`` -> ``GF.segmented_maxpool``;  inference (eval mode, gradients off): BatchNorm's
    running statistics and the ReLU ride in the layer's epilogue, and the 1024-wide layers return only their per-scene maxima;
  * on CPU tensors, over another raw-operator backend, or with ``native=False``: the same graph in plain torch ops.

These BatchNorms keep torch's defaults (eps 1e-5, momentum 0.1), not the model's ``norm_fn``.  The transformers apply the ReLU
before their max; the encoder's ``bn3`` has none.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import backend
from ... import functional as GF

LAYOUTS = ("reference", "points")


def input_view(layout: str, seg: GF.PointSegments, channels: int):
    """how the first layers read the batch's row-major point array [sum N, channels]: None = as rows (each point its own
    values, ``"points"``), or the strides (scene, channel, point) of the reference's ``points.reshape(-1, channels, N)``, a
    reinterpretation in which "channel c of point n" of scene b is flat element b channels N + c N + n (``"reference"``)."""
    if layout not in LAYOUTS:
        raise ValueError(f"pointnet_input_layout must be one of {LAYOUTS}, got {layout!r}")
    if layout == "points":
        return None
    if not seg.equal:
        raise ValueError('pointnet_input_layout="reference" reinterprets the point array as [B, channels, N] and needs '
                         f'equal-sized scenes, got {seg.counts}; use "points" for ragged batches')
    n = seg.counts[0]
    return (channels * n, n, 1)


class Run:
    """one forward pass: its scenes, and whether it runs on the point-MLP kernels (``native``) and with fused inference
    epilogues (``fused``: eval mode without gradients)"""

    def __init__(self, seg: GF.PointSegments, native: bool, fused: bool):
        self.seg, self.native, self.fused = seg, native, native and fused
        self._ids = None

    def _rows(self, x, cin, view, seg):
        """the [N, cin] matrix a strided view stands for (torch formulation)"""
        if view is None:
            return x
        sb, sc, sn = view
        return torch.as_strided(x, (seg.S, seg.counts[0], cin), (sb, sn, sc)).reshape(seg.N, cin)

    def dense(self, x, weight, bias=None, G=None, per_point=True, view=None):
        """x~ W_s^T + bias + G[s]; ``per_point`` False: x is [B, cin], one row per scene"""
        seg = self.seg if per_point else None
        if self.native:
            return GF.point_mlp(x, weight, bias, G, seg, view)
        x = self._rows(x, weight.shape[-1], view, seg)
        if weight.dim() == 2:
            y = F.linear(x, weight, bias)
        else:
            if seg.equal:
                y = torch.bmm(x.view(seg.S, seg.counts[0], -1), weight.transpose(1, 2)).reshape(seg.N, -1)
            else:
                y = torch.cat([x[seg.host[s]:seg.host[s + 1]] @ weight[s].t() for s in range(seg.S)])
            if bias is not None:
                y = y + bias
        if G is not None:
            if self._ids is None:
                self._ids = torch.repeat_interleave(torch.arange(seg.S, device=x.device),
                                                    torch.as_tensor(seg.counts, device=x.device), output_size=seg.N)
            y = y + G[self._ids]
        return y

    def pool(self, y):
        seg = self.seg
        if self.native:
            return GF.segmented_maxpool(y, seg.begin, seg.end)[0]
        if seg.equal:
            return y.view(seg.S, seg.counts[0], -1).max(dim=1)[0]
        return torch.stack([y[seg.host[s]:seg.host[s + 1]].max(dim=0)[0] for s in range(seg.S)])

    def layer(self, x, conv, bn, relu, G=None, weight=None, per_point=True, view=None, pool=False, keep=True):
        """conv / linear -> BatchNorm -> (ReLU) [-> max over each scene's points] -> (y or None, pooled or None); ``weight``
        overrides the module's own (a per-scene product, a column slice); ``keep`` False: only the pooled rows are wanted"""
        if weight is None:
            weight = conv.weight.view(conv.weight.shape[0], -1)
        if self.fused:
            scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
            shift = bn.bias - bn.running_mean * scale
            seg = self.seg if per_point else None
            return backend.raw().pointmlp_fwd(x, weight, conv.bias, G, scale, shift, relu,
                                              offsets=seg.offsets if seg is not None else None,
                                              offsets_host=seg.host if seg is not None else None, view=view, want_y=keep,
                                              want_max=pool)
        y = self.dense(x, weight, conv.bias, G, per_point, view)
        if self.native:
            y = GF.bn_act(y, bn, relu=relu)
        else:
            y = bn(y)
            y = F.relu(y) if relu else y
        return (y if keep else None), (self.pool(y) if pool else None)


class _STN(nn.Module):
    """shared forward of STN3d / STNkd: three point layers, max over the scene, three per-scene layers, + identity"""

    k = 3

    def transform_rows(self, run: Run, x, view=None):
        """x: the rows [sum N, channels] (or the flat array behind ``view``) -> [B, k, k]"""
        k = self.k
        h, _ = run.layer(x, self.conv1, self.bn1, True, view=view)
        h, _ = run.layer(h, self.conv2, self.bn2, True)
        _, g = run.layer(h, self.conv3, self.bn3, True, pool=True, keep=False)  # (ReLU before the max)
        g, _ = run.layer(g, self.fc1, self.bn4, True, per_point=False)
        g, _ = run.layer(g, self.fc2, self.bn5, True, per_point=False)
        if run.fused:
            g, _ = backend.raw().pointmlp_fwd(g, self.fc3.weight, self.fc3.bias)
        else:
            g = run.dense(g, self.fc3.weight, self.fc3.bias, per_point=False)
        iden = torch.eye(k, dtype=g.dtype, device=g.device).view(1, k * k)
        return (g + iden).view(-1, k, k)

    def forward(self, x):
        """x [B, channels, N] as in the reference -> [B, k, k]"""
        B, C, N = x.shape
        seg = GF.PointSegments([N] * B, x.device)
        run = Run(seg, GF.point_mlp_available(x, C, 64), not self.training and not torch.is_grad_enabled())
        return self.transform_rows(run, x.contiguous().view(-1), (C * N, N, 1))


class STN3d(_STN):
    def __init__(self, channel):
        super().__init__()
        self.conv1 = torch.nn.Conv1d(channel, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.relu = nn.ReLU()

        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)


class STNkd(_STN):
    def __init__(self, k=64):
        super().__init__()
        self.conv1 = torch.nn.Conv1d(k, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.relu = nn.ReLU()

        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

        self.k = k


class PointNetEncoder(nn.Module):
    def __init__(self, global_feat=True, feature_transform=False, channel=3):
        super().__init__()
        self.stn = STN3d(channel)
        self.conv1 = torch.nn.Conv1d(channel, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if self.feature_transform:
            self.fstn = STNkd(k=64)

    def encode_rows(self, run: Run, x, view=None):
        """-> (global feature [B, 1024], per-point feature [sum N, 64], trans [B, 3, 3], trans_feat [B, 64, 64] or None)"""
        trans = self.stn.transform_rows(run, x, view)
        # conv1 on [xyz . T, rest] = x . [W[:, :3] T^T, W[:, 3:]]^T: one weight matrix per scene, nothing stored in between
        w = self.conv1.weight.view(64, -1)
        w_xyz = (w[None, :, None, :3] * trans[:, None, :, :]).sum(-1)  # [B, 64, 3]: sum_j W[o, j] T[b, i, j]
        w_b = torch.cat([w_xyz, w[None, :, 3:].expand(trans.shape[0], -1, -1)], dim=2) if w.shape[1] > 3 else w_xyz
        h, _ = run.layer(x, self.conv1, self.bn1, True, weight=w_b.contiguous(), view=view)
        trans_feat = None
        if self.feature_transform:
            trans_feat = self.fstn.transform_rows(run, h)
            w_f = trans_feat.transpose(1, 2).contiguous()  # x . T as a layer: W_b[o, i] = T_b[i, o]
            if run.fused:
                h, _ = backend.raw().pointmlp_fwd(h, w_f, offsets=run.seg.offsets, offsets_host=run.seg.host)
            else:
                h = run.dense(h, w_f)
        pointfeat = h
        h, _ = run.layer(h, self.conv2, self.bn2, True)
        _, g = run.layer(h, self.conv3, self.bn3, False, pool=True, keep=False)  # (no ReLU before this max)
        return g, pointfeat, trans, trans_feat

    def forward(self, x):
        """the reference's contract: x [B, D, N] -> (global [B, 1024] or [B, 1088, N], trans, trans_feat)"""
        B, D, N = x.shape
        seg = GF.PointSegments([N] * B, x.device)
        run = Run(seg, GF.point_mlp_available(x, D, 64), not self.training and not torch.is_grad_enabled())
        g, pointfeat, trans, trans_feat = self.encode_rows(run, x.contiguous().view(-1), (D * N, N, 1))
        if self.global_feat:
            return g, trans, trans_feat
        return torch.cat([g.view(B, 1024, 1).expand(-1, -1, N), pointfeat.view(B, N, 64).transpose(1, 2)], 1), trans, trans_feat

