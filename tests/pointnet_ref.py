"""Float64 restatement of the PointNet path, shared by the fixture generator (tests/golden/make_golden_pointnet.py) and the tests.

  * ``hash_tensor`` / ``hash_state_dict``: weights as a closed-form integer hash of (parameter name, flat index) in exact
    uint64 arithmetic, scaled per fan-in.  The fixture stores no weights (3.5 M floats): generator and tests rebuild them.
  * ``dense`` / ``wgrad``: the layer contracts of csrc/pointmlp.hip (include/gpn.h section PM) in float64, each with its
    ``absolute`` twin - the same expression with every operand replaced by its absolute value, the ``A`` of the error bound
    ``|got - ref| <= gamma_n A``.
  * ``backbone``: the whole PointNetSegBackbone as the reference states it (transforms applied to the points with a batched
    product, the 1088-wide concatenation built, BatchNorm by its definition), in float64 torch ops so that autograd gives the
    float64 gradients.  It deliberately does not share the product's reformulations (folded 3 x 3 transform, split conv1).
"""
import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of fp32


def gamma(n):
    """gamma_n = n u / (1 - n u): the standard bound on the relative error of an n-term fp32 sum of products"""
    return n * U / (1.0 - n * U)


# ---- weights ---------------------------------------------------------------------------------------------------------------
def _name_key(name: str) -> np.uint64:
    h = 0xCBF29CE484222325  # FNV-1a over the name's bytes
    for ch in name.encode():
        h = ((h ^ ch) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return np.uint64(h)


def hash_uniform(name: str, count: int) -> np.ndarray:
    """count float64 values in [0, 1): splitmix64 of (FNV-1a(name) + index * golden ratio), top 53 bits"""
    with np.errstate(over="ignore"):
        z = _name_key(name) + np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def hash_tensor(name: str, shape) -> np.ndarray:
    """the fixture's value of parameter / buffer ``name``: matrices uniform in +-sqrt(3 / fan_in) (unit gain), BatchNorm
    weights in [0.75, 1.25], running variances in [0.5, 1.5], biases and running means in +-0.1.

    ``fc1`` / ``fc2`` of the transformers (weights and biases) are scaled by a further 1e-3.  Their BatchNorms see B = 2 rows
    in training, where y = d / sqrt(d^2 + eps) with d = half the rows' difference.  With unit-gain weights some of the 768
    channels land at |d| near sqrt(eps) = 3e-3, where the rows' absolute rounding error becomes a relative one of d; with
    O(0.1) biases d is a small difference of large operands.  Either way fp32 rounding grew to 1e-5 of the activations
    (measured), enough to flip ReLUs in every later layer, and the reference's own fp32 gradients were 2e-3 from float64.
    At 1e-3 every |d| stays below sqrt(eps) and is not a cancellation: the BatchNorm works in its near-linear regime (gain
    1 / sqrt(eps), so eps still shows) and the reference's fp32 result is a usable yardstick."""
    shape = tuple(int(s) for s in shape)
    if name.endswith("num_batches_tracked"):
        return np.zeros(shape, np.int64)
    count = int(np.prod(shape)) if shape else 1
    s = 2.0 * hash_uniform(name, count) - 1.0
    if name.endswith("running_var"):
        v = 1.0 + 0.5 * s
    elif name.endswith(".weight") and len(shape) >= 2:
        v = s * np.sqrt(3.0 / np.prod(shape[1:])) * (1e-3 if ".fc1." in name or ".fc2." in name else 1.0)
    elif name.endswith(".weight"):
        v = 1.0 + 0.25 * s
    else:
        v = 0.1 * s * (1e-3 if ".fc1." in name or ".fc2." in name else 1.0)
    return v.reshape(shape).astype(np.float32)


def hash_state_dict(names_shapes):
    return {n: torch.from_numpy(hash_tensor(n, s)) for n, s in names_shapes}


def hash_input(B: int, n: int, channels: int = 6) -> np.ndarray:
    """the fixture's point array [B n, channels]: scene b uniform in +-1 / (1 + 2 b).  Scenes of one distribution have nearly
    equal global features, and the transformers' fc BatchNorms (B rows in training) then normalise a difference that is a
    1 / 150 of its operands: fp32 rounding grows by that factor and flips ReLUs all the way down."""
    x = (2.0 * hash_uniform("input", B * n * channels) - 1.0).reshape(B, n * channels)
    return (x / (1.0 + 2.0 * np.arange(B))[:, None]).reshape(B * n, channels).astype(np.float32)


# ---- layer contracts -------------------------------------------------------------------------------------------------------
def view_rows(flat: np.ndarray, S: int, n: int, cin: int, strides) -> np.ndarray:
    """the [S n, cin] matrix of a strided view: element (b, c, p) = flat[b sb + c sc + p sn]"""
    sb, sc, sn = strides
    b, p, c = np.meshgrid(np.arange(S), np.arange(n), np.arange(cin), indexing="ij")
    return flat[b * sb + c * sc + p * sn].reshape(S * n, cin)


def _segments(offsets, N):
    return [(0, N)] if offsets is None else [(int(offsets[s]), int(offsets[s + 1])) for s in range(len(offsets) - 1)]


def dense(X, W, b=None, G=None, offsets=None, scale=None, shift=None, relu=False, absolute=False):
    """-> (Y [N, cout], M [S, cout]) in float64; ``absolute``: the bound's A (every operand by its absolute value; ReLU and max
    are 1-Lipschitz, so Y's A passes through the ReLU and M's A is the largest row bound of the segment)"""
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    X, W = f(X), f(W)
    N, cout = X.shape[0], W.shape[-2]
    segs = _segments(offsets, N)
    Y = np.empty((N, cout))
    for s, (r0, r1) in enumerate(segs):
        y = X[r0:r1] @ (W[s] if W.ndim == 3 else W).T
        if b is not None:
            y = y + f(b)
        if G is not None:
            y = y + f(G)[s]
        if scale is not None:
            y = f(scale) * y + f(shift)
        Y[r0:r1] = y
    if relu and not absolute:
        Y = np.maximum(Y, 0.0)
    M = np.stack([Y[r0:r1].max(0) for r0, r1 in segs])
    return Y, M


def wgrad(X, dY, offsets=None, per_segment=False, absolute=False):
    """-> (dW [cout, cin] or [S, cout, cin] = dY^T X, db [cout]) in float64"""
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    X, dY = f(X), f(dY)
    if per_segment:
        dW = np.stack([dY[r0:r1].T @ X[r0:r1] for r0, r1 in _segments(offsets, X.shape[0])])
    else:
        dW = dY.T @ X
    return dW, dY.sum(0)


# ---- the backbone ----------------------------------------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1  # torch's BatchNorm1d defaults (not the model's norm_fn)


class _Net:
    """parameters by name in float64; ``new_stats`` collects the running statistics a training pass would leave"""

    def __init__(self, params, training):
        self.p, self.training, self.new_stats = params, training, {}

    def lin(self, x, name):
        w = self.p[name + ".weight"]
        return x @ w.reshape(w.shape[0], -1).t() + self.p[name + ".bias"]

    def bn(self, x, name, relu):
        w, b = self.p[name + ".weight"], self.p[name + ".bias"]
        rm, rv = self.p[name + ".running_mean"], self.p[name + ".running_var"]
        if self.training:
            n = x.shape[0]
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
            self.new_stats[name + ".running_mean"] = ((1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean).detach()
            self.new_stats[name + ".running_var"] = ((1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var * n / (n - 1)).detach()
        else:
            mean, var = rm, rv
        y = (x - mean) / torch.sqrt(var + BN_EPS) * w + b
        return torch.clamp(y, min=0.0) if relu else y

    def stn(self, x, scenes, name, k):
        h = self.bn(self.lin(x, name + ".conv1"), name + ".bn1", True)
        h = self.bn(self.lin(h, name + ".conv2"), name + ".bn2", True)
        h = self.bn(self.lin(h, name + ".conv3"), name + ".bn3", True)
        g = torch.stack([h[a:b].max(0)[0] for a, b in scenes])
        g = self.bn(self.lin(g, name + ".fc1"), name + ".bn4", True)
        g = self.bn(self.lin(g, name + ".fc2"), name + ".bn5", True)
        g = self.lin(g, name + ".fc3") + torch.eye(k, dtype=g.dtype).reshape(1, k * k)
        return g.reshape(-1, k, k)


def input_rows(points: torch.Tensor, counts, layout: str) -> torch.Tensor:
    """the [sum N, C] rows the network sees: "points" = the array itself; "reference" = points.reshape(B, C, N) read as
    (scene, channel, point), i.e. row (b, n) = flat[b C N + c N + n] over c"""
    if layout == "points":
        return points
    assert layout == "reference" and len(set(counts)) == 1
    B, n, C = len(counts), counts[0], points.shape[1]
    return points.reshape(B, C, n).transpose(1, 2).reshape(B * n, C)


def backbone(params, points, counts, layout="reference", training=False):
    """PointNetSegBackbone (pointnet_sem_seg.py:21-30 over pointnet_utils.py:103-133) -> (features [sum N, fea_dim], new_stats).
    ``params``: name -> float64 tensor (names relative to the PointNetSegBackbone); ``points`` [sum N, C] float64."""
    net = _Net(params, training)
    x = input_rows(points, counts, layout)
    offs = np.concatenate([[0], np.cumsum(counts)])
    scenes = [(int(offs[i]), int(offs[i + 1])) for i in range(len(counts))]
    trans = net.stn(x, scenes, "feat.stn", 3)
    x = torch.cat([torch.cat([x[a:b, :3] @ trans[s], x[a:b, 3:]], dim=1) for s, (a, b) in enumerate(scenes)])
    h = net.bn(net.lin(x, "feat.conv1"), "feat.bn1", True)
    trans_feat = net.stn(h, scenes, "feat.fstn", 64)
    pointfeat = torch.cat([h[a:b] @ trans_feat[s] for s, (a, b) in enumerate(scenes)])
    h = net.bn(net.lin(pointfeat, "feat.conv2"), "feat.bn2", True)
    h = net.bn(net.lin(h, "feat.conv3"), "feat.bn3", False)
    g = torch.stack([h[a:b].max(0)[0] for a, b in scenes])
    wide = torch.cat([torch.cat([g[s].expand(b - a, -1), pointfeat[a:b]], dim=1) for s, (a, b) in enumerate(scenes)])
    h = net.bn(net.lin(wide, "conv1"), "bn1", True)
    h = net.bn(net.lin(h, "conv2"), "bn2", True)
    h = net.bn(net.lin(h, "conv3"), "bn3", True)
    return net.lin(h, "conv4"), net.new_stats


# what the fixture records -----------------------------------------------------------------------------------------------------
FIXTURE_B, FIXTURE_N = 2, 300
GRAD_PARAMS = ("feat.stn.conv1.weight", "feat.fstn.fc3.weight", "feat.conv1.weight", "feat.bn3.weight", "conv1.weight",
               "conv4.bias")
STAT_BNS = ("feat.stn.bn1", "bn1")
GRAD_KEEP = 16384  # gradients larger than this are recorded as every stride-th flat element (a committed file stays small)


def grad_stride(numel: int) -> int:
    return max(1, -(-numel // GRAD_KEEP))


def recorded(grad) -> np.ndarray:
    flat = np.asarray(grad).reshape(-1)
    return flat[::grad_stride(flat.size)]


def run_f64(names_shapes, points_f32, counts, layout, training, cotangent=None):
    """the float64 restatement on the hash weights -> dict of the arrays the fixture records (same keys)"""
    params = {}
    for n, s in names_shapes:
        if n.endswith("num_batches_tracked"):
            continue
        params[n] = torch.from_numpy(hash_tensor(n, s)).double()
    for n in GRAD_PARAMS:
        params[n].requires_grad_(True)
    pts = torch.from_numpy(np.asarray(points_f32)).double().requires_grad_(training)
    out, stats = backbone(params, pts, counts, layout, training)
    res = {"out": out.detach().numpy()}
    if training:
        (out * torch.from_numpy(np.asarray(cotangent)).double()).sum().backward()
        res["grad.input"] = pts.grad.numpy()
        for n in GRAD_PARAMS:
            res["grad." + n] = recorded(params[n].grad.numpy())
        for bn in STAT_BNS:
            for k in ("running_mean", "running_var"):
                res[f"stat.{bn}.{k}"] = stats[f"{bn}.{k}"].numpy()
    return res


def rel_err(got, ref) -> float:
    """max |got - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())
