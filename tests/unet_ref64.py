"""A float64 reference of the sparse U-Net, op by op, that can be TEACHER-FORCED with a device's own activations.

Why forcing: an end-to-end float64 U-Net cannot be compared with an fp32 one at a useful tolerance - one pre-activation within
fp32 rounding of zero flips its ReLU between the two precisions and everything behind it moves by O(1e-3).  Here every float64 op
reads the RECORDED input of that op (``v = chain + (rec - chain).detach()``: the recorded value, the float64 chain's gradient) and
takes its ReLU mask from the recorded ``y > 0``.  Each op's float64 output is compared with the recorded output of that op alone,
and autograd through the chain yields the backward pass linearised at the recorded forward pass.

Geometry comes from the coordinates alone (no rulebook of the library or of the oracle is read):
  submanifold 3x3x3   tap k = (dx+1)*9 + (dy+1)*3 + (dz+1), source = the voxel at coordinate + (dx, dy, dz)
  stride-2 down conv  coarse coordinate = fine // 2, tap = (x&1)*4 + (y&1)*2 + (z&1); an odd extent drops its last plane
  inverse conv        the transpose of the same pairs
The ORDER of the coarse rows is taken from the recorder's level indices (the reference reads the recorded buffers row for row)
after their coordinate SET has been checked against {fine // 2}.

Two walks: ``walk_modules`` recurses over the module tree as network/backbone.py's ``forward`` does (the definition);
``walk_program`` walks ``NetProgram.ops`` and is the one that can be forced.  Two recorders produce the same ``Record``:
``record_executor`` (GPU: what ``net_exec._NetFn`` does, by hand, keeping every slot) and ``record_modules`` (the layer-by-layer
path, on the GPU or on the CPU over ``oracle.torch_ops``).  ``compare`` is the one comparator: per tensor max|got - ref| / max|ref|.

All inputs used with this reference are well conditioned (|mean| of the order of std in every channel): the fp32 accumulation of x
and x^2 in the stand-alone statistics kernels is a known property of the library and not what is tested here.  One place cannot be
conditioned by the choice of inputs: a BatchNorm over 2 rows (case B's deepest level, the stand-alone shape (2, 16)).  There
|mean| / std = |x1 + x2| / |x1 - x2| is a ratio of two independent normals, so a few of every hundred channels are ill-conditioned
whatever the inputs.  ``well_conditioned`` draws the line from the reference alone, and save_invstd is compared on the channels
inside it; everything else (the op's output, gradients, running statistics, save_mean) is compared on all channels.
"""
import copy
import functools
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from gapartnet_amd import backend
from gapartnet_amd import functional as GF
from gapartnet_amd.network import net_exec
from gapartnet_amd.network.backbone import SparseUNet
from gapartnet_amd.spconv import pytorch as spconv
from tests import synth

OP_NAMES = {net_exec.OP_CONV: "CONV", net_exec.OP_BN: "BN", net_exec.OP_CONCAT: "CONCAT"}
CLASSES = ("conv", "bn", "stat", "running", "din", "wgrad", "bn_grad")

# Worst error of an fp32 evaluation of this reference against its own float64, per quantity class, over the cases A-D below in
# training and eval mode and over two fp32 evaluations: this file's walk in torch fp32 on ONE thread (torch's CPU sums are then
# sequential in the rows, the order the margin below is argued from, and the figure does not depend on the machine's core count:
# with 16 threads it is up to 3.5x smaller) and the C oracle through record_modules.
# MEASURED by tests/test_unet_ref_cpu.py::test_floor*, which fail if a re-measured value exceeds its entry here by more than half
# or falls below a quarter of it (so the table can neither lag behind nor be padded).  Never a number taken from the kernels.
FLOORS = {"conv": 1.60e-6, "bn": 3.40e-6, "stat": 2.69e-7, "running": 4.18e-7, "din": 5.78e-6, "wgrad": 9.05e-6, "bn_grad": 1.56e-5}
MARGIN = 8.0  # the kernels sum in other orders (MFMA k-blocks, 16-row tiles, strided rows, fixed-point words), none worse than a sequential fp32 sum
TOL = {k: MARGIN * v for k, v in FLOORS.items()}


# ------------------------------------------------------------------------------------------------------------------ cases
CASES = {
    "A": dict(channels=[16, 32, 48, 64], stem=True, batch=3, shape=[64, 64, 64], n=2500, seed=7),
    "B": dict(channels=[16, 32, 48, 64, 80, 96, 112], stem=False, batch=2, shape=[96, 96, 96], n=4000, seed=7),
    "C": dict(channels=[16, 32], stem=False, batch=1, shape=[24, 24, 24], n=150, seed=7),
    "D": dict(channels=[16, 32], stem=True, batch=1, shape=[192, 192, 192], n=30000, seed=7),
}


def make_case(name, stem: Optional[bool] = None, net_seed=3):
    """-> namespace(net [CPU, fp32, BatchNorm parameters and running statistics away from 1 / 0], idx, feats N(0,1), shape, batch, dy)"""
    c = CASES[name]
    stem = c["stem"] if stem is None else stem
    cin = 6 if stem else c["channels"][0]
    torch.manual_seed(net_seed)
    net = SparseUNet.build(cin, c["channels"], 2, functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1), without_stem=not stem)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 2.0)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.2)
    rng = np.random.default_rng(c["seed"])
    idx = torch.from_numpy(synth.surface_indices(rng, c["batch"], c["shape"], c["n"]))
    feats = torch.from_numpy(rng.normal(size=(idx.shape[0], cin)).astype(np.float32))
    dy = torch.from_numpy(rng.normal(size=(idx.shape[0], c["channels"][0])).astype(np.float32))
    return SimpleNamespace(name=name, net=net, idx=idx, feats=feats, shape=list(c["shape"]), batch=c["batch"], dy=dy, stem=stem)


# --------------------------------------------------------------------------------------------------------------- geometry
def _keys(b, xyz, shape):
    return ((b * shape[0] + xyz[:, 0]) * shape[1] + xyz[:, 1]) * shape[2] + xyz[:, 2]


def _lookup(keys, query):
    """row of each query key in ``keys`` (unique), -1 where absent"""
    sk, order = keys.sort()
    pos = torch.searchsorted(sk, query).clamp(max=sk.numel() - 1)
    return torch.where(sk[pos] == query, order[pos], torch.full_like(pos, -1))


def subm_pairs(idx, shape):
    i = idx.long()
    keys = _keys(i[:, 0], i[:, 1:], shape)
    assert keys.unique().numel() == keys.numel(), "duplicate voxels"
    lim = torch.tensor(shape)
    pairs = []
    for k in range(27):
        n = i[:, 1:] + torch.tensor([k // 9 - 1, k // 3 % 3 - 1, k % 3 - 1])
        ok = ((n >= 0) & (n < lim)).all(1)
        j = torch.where(ok, _lookup(keys, _keys(i[:, 0], n, shape)), torch.full_like(keys, -1))
        dst = (j >= 0).nonzero()[:, 0]
        if dst.numel():
            pairs.append((k, j[dst], dst))
    return pairs


def coarse_keys(idx, shape):
    """sorted unique keys {fine // 2} on the coarse grid (an odd extent drops its last plane), the coarse shape"""
    i = idx.long()
    out_shape = [s // 2 for s in shape]
    c = i[:, 1:] // 2
    ok = (c < torch.tensor(out_shape)).all(1)
    return _keys(i[ok, 0], c[ok], out_shape).unique(), out_shape


def down_pairs(idx, shape, coarse_idx):
    """pairs (tap, fine row, coarse row) of the stride-2 conv whose output rows are ``coarse_idx`` in that order"""
    i, ci = idx.long(), coarse_idx.long()
    want, out_shape = coarse_keys(idx, shape)
    ck = _keys(ci[:, 0], ci[:, 1:], out_shape)
    assert torch.equal(ck.sort()[0], want), "the coarse level's coordinate set is not {fine // 2}"
    c = i[:, 1:] // 2
    ok = (c < torch.tensor(out_shape)).all(1)
    row = _lookup(ck, _keys(i[:, 0], c, out_shape))
    tap = (i[:, 1] & 1) * 4 + (i[:, 2] & 1) * 2 + (i[:, 3] & 1)
    pairs = []
    for k in range(8):
        src = (ok & (tap == k)).nonzero()[:, 0]
        if src.numel():
            assert (row[src] >= 0).all()
            pairs.append((k, src, row[src]))
    return pairs, out_shape


class Geometry:
    """per level: indices, shape, row count and the pair lists of its convs.  ``coarse`` = the recorder's indices of levels
    1 .. n-1 (their row order is adopted); None: ascending key order"""

    def __init__(self, idx, shape, n_levels, coarse=None):
        self.idx, self.shape, self.subm, self.down = [idx.cpu()], [list(shape)], [], []
        for lvl in range(n_levels):
            self.subm.append(subm_pairs(self.idx[lvl], self.shape[lvl]))
            if lvl + 1 == n_levels:
                break
            if coarse is not None:
                nxt = coarse[lvl].cpu()
            else:
                keys, s = coarse_keys(self.idx[lvl], self.shape[lvl])
                z = keys % s[2]; y = keys // s[2] % s[1]; x = keys // (s[2] * s[1]) % s[0]; b = keys // (s[2] * s[1] * s[0])
                nxt = torch.stack([b, x, y, z], 1).to(torch.int32)
            pairs, out_shape = down_pairs(self.idx[lvl], self.shape[lvl], nxt)
            self.down.append(pairs)
            self.idx.append(nxt)
            self.shape.append(out_shape)
        self.rows = [int(i.shape[0]) for i in self.idx]

    def pairs(self, kind, lvl):
        """-> (pairs, destination rows) of a program rulebook key"""
        if kind == "subm":
            return self.subm[lvl], self.rows[lvl]
        if kind == "down":
            return self.down[lvl], self.rows[lvl + 1]
        if kind == "inv":
            return [(k, dst, src) for k, src, dst in self.down[lvl]], self.rows[lvl]
        r = torch.arange(self.rows[lvl])
        return [(0, r, r)], self.rows[lvl]


# -------------------------------------------------------------------------------------------------------------------- ops
def conv(x, W, pairs, n_dst, drop=None):
    """W in the parameter layout [Cout, kz, ky, kx, Cin]; ``drop`` = (tap, first row, end row): that tap's contribution to those
    output rows is left out (a fault for the teeth tests)"""
    Wk = W.reshape(W.shape[0], -1, W.shape[-1])
    out = torch.zeros((n_dst, W.shape[0]), dtype=x.dtype)
    for k, src, dst in pairs:
        if drop is not None and drop[0] == k:
            keep = (dst < drop[1]) | (dst >= drop[2])
            src, dst = src[keep], dst[keep]
        out = out.index_add(0, dst, x[src] @ Wk[:, k, :].T)
    return out


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum, eps, res=None, relu=False, mask=None):
    """-> (y, mean, invstd, new running_mean, new running_var); ``mask``: the ReLU as multiplication by a recorded mask"""
    rm, rv = running_mean.clone(), running_var.clone()
    y = F.batch_norm(x, rm, rv, weight, bias, training, momentum, eps)
    if training:
        xd = x.detach()
        mean, invstd = xd.mean(0), (xd.var(0, unbiased=False) + eps).rsqrt()
    else:
        mean, invstd = running_mean, (running_var + eps).rsqrt()
    if res is not None:
        y = y + res
    if relu:
        y = y * ((y.detach() > 0) if mask is None else mask).to(y.dtype)
    return y, mean, invstd, rm, rv


class Params:
    """the network's parameters (leaves that require a gradient) and buffers in ``dtype``, from a state dict, by module"""

    def __init__(self, net, state, dtype):
        self.names = {id(m): n for n, m in net.named_modules()}
        is_param = {n for n, _ in net.named_parameters()}
        self.t = {}
        for k, v in state.items():
            t = v.detach().cpu().clone()
            if t.is_floating_point():
                t = t.to(dtype)
                if k in is_param:
                    t.requires_grad_(True)
            self.t[k] = t
        self.after = {k: v for k, v in self.t.items() if k not in is_param}  # buffers after the pass (filled by bn)

    def name(self, m):
        return self.names[id(m)]

    def w(self, m):
        return self.t[self.name(m) + ".weight"]

    def bn(self, m, x, training, res=None, relu=False, mask=None):
        n = self.name(m)
        y, mean, invstd, rm, rv = batch_norm(x, self.t[n + ".weight"], self.t[n + ".bias"], self.t[n + ".running_mean"],
                                             self.t[n + ".running_var"], training, m.momentum, m.eps, res, relu, mask)
        if training:
            self.after[n + ".running_mean"], self.after[n + ".running_var"] = rm, rv
            self.after[n + ".num_batches_tracked"] = self.t[n + ".num_batches_tracked"] + 1
        return y, mean, invstd

    def grads(self):
        return {k: v.grad for k, v in self.t.items() if v.requires_grad}


# ------------------------------------------------------------------------------------------------- the definition: modules
def walk_modules(net, P: Params, geom: Geometry, x, training):
    """network/backbone.py's forward over the module tree, in x's dtype -> output features"""
    def conv_bn(seq, x, kind, lvl, relu, res=None):
        mods = list(seq._modules.values())
        pairs, n = geom.pairs(kind, lvl)
        return P.bn(mods[1], conv(x, P.w(mods[0]), pairs, n), training, res, relu)[0]

    def resblock(blk, x, lvl):
        skip = x if isinstance(blk.shortcut, nn.Identity) else conv_bn(blk.shortcut, x, "ident", lvl, False)
        y = conv_bn(blk.conv1, x, "subm", lvl, True)
        return conv_bn(blk.conv2, y, "subm", lvl, True, res=skip)

    def ublock(ub, x, lvl):
        for blk in ub.encoder_blocks._modules.values():
            x = resblock(blk, x, lvl)
        if len(ub.channels) == 1:
            return x
        skip = x
        x = conv_bn(ub.downsample, x, "down", lvl, True)
        x = ublock(ub.ublock, x, lvl + 1)
        x = conv_bn(ub.upsample, x, "inv", lvl, True)
        x = torch.cat([x, skip], dim=-1)
        for blk in ub.decoder_blocks._modules.values():
            x = resblock(blk, x, lvl)
        return x

    stem = list(net.stem._modules.values())
    if len(stem) == 3:
        x = conv_bn(net.stem, x, "subm", 0, True)
    else:
        x = P.bn(stem[0], x, training, None, True)[0]
    return ublock(net.ublock, x, 0)


# ------------------------------------------------------------------------------------------------------------ the record
class Record(SimpleNamespace):
    """what a pass left behind (CPU tensors, live rows only):
    training, inference (conv outputs not kept), x (the raw input features), levels [(indices, shape)], stem_out (output of the
    6-channel stem conv that runs in front of the program = slot 0, or None), slots [per program slot; slot 0 = the program's
    input], save_mean / save_invstd [per BatchNorm, None = not written in this mode], state_before / state_after (state dicts),
    dy, din, grads {parameter name: gradient}"""


def _cpu(t):
    return None if t is None else t.detach().cpu().clone()


def _state(net):
    return {k: _cpu(v) for k, v in net.state_dict().items()}


def op_label(prog, P_or_names, i):
    names = P_or_names.names if isinstance(P_or_names, Params) else P_or_names
    if i < 0:
        return f"op -1 CONV {names[id(prog.python_stem_conv)]} level 0 (the stem conv in front of the program)"
    kind, s0, s1, dst, rb, param, flags = prog.ops[i]
    mod = prog.convs[param] if kind == net_exec.OP_CONV else prog.bns[param] if kind == net_exec.OP_BN else None
    return f"op {i} {OP_NAMES[kind]} {names[id(mod)] if mod is not None else '(concat)'} level {prog.slot_level[dst]}"


# --------------------------------------------------------------------------------------------------- the program, forced
def walk_program(prog, net, geom, state, x, dy, training, dtype=torch.float64, rec: Optional[Record] = None, force_convs=True,
                 fault=None, backward=True):
    """walk ``prog.ops`` in ``dtype`` from the buffers of ``state``.  With ``rec`` every op reads the recorded value of its input
    slots (the chain's gradient) and ReLU masks come from the recorded outputs; ``force_convs = False`` leaves conv outputs
    unforced (the inference form keeps none: the compared op is then conv o BatchNorm).  ``fault`` = (op index, kind) computes
    that op wrongly, the rest consistently with it (teeth tests; only sensible without ``rec``).
    -> namespace(P, outs [unforced output of every op], stem_out, slots [the values passed on], mean / invstd [per BatchNorm],
    after (expected buffers), din, grads)"""
    P = Params(net, state, dtype)
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)

    def forced(chain, slot):
        return chain if rec is None else chain + (rec.slots[slot].to(dtype) - chain).detach()

    f_op, f_kind = fault if fault is not None else (None, None)
    stem_out = None
    if prog.python_stem_conv is not None:
        pairs, n = geom.pairs("subm", 0)
        stem_out = conv(x, P.w(prog.python_stem_conv), pairs, n)
        slots = [forced(stem_out, 0)]
    else:
        slots = [x]
    slots += [None] * (len(prog.slot_level) - 1)
    outs, mean, invstd = [], [None] * len(prog.bns), [None] * len(prog.bns)
    for i, (kind, s0, s1, dst, rb, param, flags) in enumerate(prog.ops):
        bad = f_kind if i == f_op else None
        if kind == net_exec.OP_CONV:
            pairs, n = geom.pairs(*prog.rb_keys[rb])
            o = conv(slots[s0], P.w(prog.convs[param]), pairs, n, drop=(pairs[len(pairs) // 2][0], 16, 32) if bad == "drop_tap_tile" else None)
            slots[dst] = forced(o, dst) if force_convs else o
        elif kind == net_exec.OP_BN:
            bn, relu, xin = prog.bns[param], bool(flags & net_exec.FLAG_RELU), slots[s0]
            res = None if s1 < 0 or bad == "no_residual" else slots[s1]
            mask = None if rec is None or not relu else rec.slots[dst] > 0
            if bad == "stats_without_last_row":
                o, mean[param], invstd[param] = _bn_stats_of(P, bn, xin, xin[:-1], res, relu)
            elif bad == "mask_from_x":
                o, mean[param], invstd[param] = P.bn(bn, xin, training, res, False)
                fwd, bwd = o * (o.detach() > 0), o * (xin.detach() > 0)
                o = bwd + (fwd - bwd).detach()
            elif bad == "dweight_without_a_block":
                o, mean[param], invstd[param] = P.bn(bn, xin, training, res, relu)
                n = P.name(bn)
                w = P.t[n + ".weight"]
                P.t[n + ".weight"] = w.detach()
                o_cut = P.bn(bn, xin, training, res, relu)[0]  # (the same values; no gradient reaches the weight)
                P.t[n + ".weight"] = w
                block = torch.zeros((o.shape[0], 1), dtype=torch.bool)
                block[32:64] = True
                o = torch.where(block, o_cut, o)
            else:
                o, mean[param], invstd[param] = P.bn(bn, xin, training, res, relu, mask)
                if bad == "biased_running_var":
                    n, N = P.name(bn), xin.shape[0]
                    old = P.t[n + ".running_var"]
                    P.after[n + ".running_var"] = old + (P.after[n + ".running_var"] - old * (1 - bn.momentum)) * ((N - 1) / N) - old * bn.momentum
            slots[dst] = forced(o, dst)
        else:
            o = torch.cat([slots[s1], slots[s0]] if bad == "concat_swapped" else [slots[s0], slots[s1]], dim=-1)
            slots[dst] = forced(o, dst)
        outs.append(o.detach())
    out = SimpleNamespace(P=P, outs=outs, stem_out=None if stem_out is None else stem_out.detach(), mean=mean, invstd=invstd,
                          slots=[s.detach() for s in slots], din=None, grads=None)
    if backward:
        (slots[prog.out_slot] * dy.to(dtype)).sum().backward()
        out.din, out.grads = x.grad, P.grads()
    out.after = {k: v.detach() for k, v in P.after.items()}
    return out


def _bn_stats_of(P, bn, x, sample, res, relu):
    """training BatchNorm of ``x`` with the statistics of ``sample`` (a fault)"""
    n = P.name(bn)
    mean, var = sample.mean(0), sample.var(0, unbiased=False)
    invstd = (var + bn.eps).rsqrt()
    y = (x - mean) * invstd * P.t[n + ".weight"] + P.t[n + ".bias"]
    if res is not None:
        y = y + res
    if relu:
        y = y * (y.detach() > 0)
    N = sample.shape[0]
    P.after[n + ".running_mean"] = (P.t[n + ".running_mean"] * (1 - bn.momentum) + bn.momentum * mean).detach()
    P.after[n + ".running_var"] = (P.t[n + ".running_var"] * (1 - bn.momentum) + bn.momentum * var * N / (N - 1)).detach()
    P.after[n + ".num_batches_tracked"] = P.t[n + ".num_batches_tracked"] + 1
    return y, mean.detach(), invstd.detach()


def record_walk(case, training, dtype, geom=None, fault=None, prog=None) -> Record:
    """this file's own walk of the program as a 'device' (torch fp32: one of the two floor evaluations; float64: the
    self-consistency tests; with ``fault``: the teeth tests)"""
    prog = prog or net_exec.program_for(case.net)
    geom = geom or Geometry(case.idx, case.shape, prog.n_levels)
    before = _state(case.net)
    w = walk_program(prog, case.net, geom, before, case.feats, case.dy, training, dtype, fault=fault)
    after = dict(before)
    after.update(w.after)  # (running statistics stay in the walk's dtype)
    return Record(training=training, inference=False, x=case.feats.clone(), levels=list(zip(geom.idx, geom.shape)), stem_out=w.stem_out,
                  slots=w.slots, save_mean=w.mean if training else [None] * len(w.mean), save_invstd=w.invstd,
                  state_before=before, state_after=after, dy=case.dy.clone(), din=w.din, grads=w.grads)


# ------------------------------------------------------------------------------------------------------------ comparator
# A channel with |mean| > 8 std (float64 batch statistics) is ill-conditioned.  Why 8: a variance taken as E[x^2] - mean^2 from
# squares rounded to fp32 (relative 2^-24 each) is off by at most 2^-24 (mean^2 + var), 1/std by half of that relatively:
# 3e-8 (1 + 8^2) = 1.9e-6 is where that rounding alone reaches the tolerance of the class (8 x 2.69e-7).
ILL_CONDITIONED = 8.0


def well_conditioned(mean, invstd):
    return mean.abs() * invstd <= ILL_CONDITIONED


def rel_err(got, ref, scale=None):
    """max|got - ref| / scale, scale = max|ref| over the tensor (1 if the reference is all zero); inf for a NaN or a shape mismatch"""
    if got is None or tuple(got.shape) != tuple(ref.shape):
        return float("inf")
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if ref.numel() == 0:
        return 0.0
    s = float(ref.abs().max()) if scale is None else float(scale)
    d = float((got - ref).abs().max())
    return float("inf") if d != d else d / (s if s > 0 else 1.0)


class Report:
    """entries (class, label, op index or None, error); class "exact" = structural (error 0 or inf)"""

    def __init__(self):
        self.entries = []
        self.channels = self.skipped = 0  # BatchNorm channels whose save_invstd was due / was left out as ill-conditioned

    def add(self, cls, label, op, err):
        self.entries.append((cls, label, op, err))

    def worst(self):
        w = {}
        for cls, label, op, err in self.entries:
            if cls != "exact" and err >= w.get(cls, (-1.0, ""))[0]:
                w[cls] = (err, label)
        return w

    def failures(self, tol):
        return [e for e in self.entries if not e[3] <= (0.0 if e[0] == "exact" else tol[e[0]])]

    def check(self, tol, what=""):
        bad = self.failures(tol)
        lines = [f"{label}: {cls} error {err:.3e} > {0.0 if cls == 'exact' else tol[cls]:.3e}" for cls, label, op, err in bad]
        assert not bad, f"{what}: {len(bad)} quantities off their float64 reference\n  " + "\n  ".join(lines[:20])


def reference_for(prog, net, rec: Record, geom=None):
    geom = geom or Geometry(rec.levels[0][0], rec.levels[0][1], prog.n_levels, coarse=[l[0] for l in rec.levels[1:]])
    return walk_program(prog, net, geom, rec.state_before, rec.x, rec.dy, rec.training, torch.float64, rec=rec,
                        force_convs=not rec.inference, backward=rec.din is not None)


def compare(prog, net, rec: Record, ref, report: Optional[Report] = None, tag="") -> Report:
    """every recorded quantity of ``rec`` against the forced float64 walk ``ref`` of the same record"""
    R = report or Report()
    P = ref.P
    if rec.stem_out is not None:
        R.add("conv", tag + op_label(prog, P, -1), -1, rel_err(rec.slots[0], ref.stem_out))
    for i, (kind, s0, s1, dst, rb, param, flags) in enumerate(prog.ops):
        label = tag + op_label(prog, P, i)
        if kind == net_exec.OP_CONCAT:
            R.add("exact", label, i, 0.0 if torch.equal(rec.slots[dst], torch.cat([rec.slots[s0], rec.slots[s1]], dim=-1)) else float("inf"))
        elif kind == net_exec.OP_CONV:
            if not rec.inference:
                R.add("conv", label, i, rel_err(rec.slots[dst], ref.outs[i]))
        else:
            R.add("bn", label, i, rel_err(rec.slots[dst], ref.outs[i]))
            if rec.save_mean[param] is not None:
                R.add("stat", label + " save_mean", i, rel_err(rec.save_mean[param], ref.mean[param], scale=float((1.0 / ref.invstd[param]).max())))
            if rec.save_invstd[param] is not None:
                want = ref.invstd[param]
                keep = well_conditioned(ref.mean[param], want) if rec.training else torch.ones_like(want, dtype=torch.bool)
                R.channels, R.skipped = R.channels + keep.numel(), R.skipped + int((~keep).sum())
                got = rec.save_invstd[param]
                R.add("stat", label + " save_invstd", i, rel_err(got[keep] if got.shape == want.shape else None, want[keep]))
    op_of = {}
    for i, (kind, s0, s1, dst, rb, param, flags) in enumerate(prog.ops):
        if kind != net_exec.OP_CONCAT:
            op_of[P.name(prog.convs[param] if kind == net_exec.OP_CONV else prog.bns[param])] = i
    if prog.python_stem_conv is not None:
        op_of[P.name(prog.python_stem_conv)] = -1
    for k, want in ref.after.items():
        got = rec.state_after[k]
        i = op_of[k.rsplit(".", 1)[0]]
        label = f"{tag}{op_label(prog, P, i)} {k.rsplit('.', 1)[1]}"
        if not rec.training or not want.is_floating_point():
            R.add("exact", label, i, 0.0 if torch.equal(got, want.to(got.dtype)) else float("inf"))
        else:
            R.add("running", label, i, rel_err(got, want))
    if ref.din is not None:
        R.add("din", tag + "input gradient", None, rel_err(rec.din, ref.din))
        for k, want in ref.grads.items():
            mod, leaf = k.rsplit(".", 1)
            i = op_of[mod]
            is_bn = i >= 0 and prog.ops[i][0] == net_exec.OP_BN
            R.add("bn_grad" if is_bn else "wgrad", f"{tag}{op_label(prog, P, i)} d{leaf}", i, rel_err(rec.grads.get(k), want))
    return R


# --------------------------------------------------------------------------------------------------------------- recorders
def _assemble(prog, rec_kw, conv_out, bn_out, bn_stats, x_prog):
    """slots and statistics of the program from per-module outputs"""
    slots = [x_prog] + [None] * (len(prog.slot_level) - 1)
    n_bn = len(prog.bns)
    mean, invstd = [None] * n_bn, [None] * n_bn
    for kind, s0, s1, dst, rb, param, flags in prog.ops:
        if kind == net_exec.OP_CONV:
            slots[dst] = conv_out[id(prog.convs[param])]
        elif kind == net_exec.OP_BN:
            slots[dst] = bn_out[id(prog.bns[param])]
            mean[param], invstd[param] = bn_stats[id(prog.bns[param])]
        else:
            slots[dst] = torch.cat([slots[s0], slots[s1]], dim=-1)
    return Record(slots=slots, save_mean=mean, save_invstd=invstd, **rec_kw)


def record_modules(case, training, device=None, ops=None):
    """the layer-by-layer path (``use_native_executor = False``) of a copy of ``case.net``: inputs and outputs of every conv module
    and of every ``functional.bn_act`` call are kept, gradients come from autograd.  ``device`` = a GPU (the stand-alone
    BatchNorm kernels behind hip_ops.bn_fwd / bn_bwd), or ``ops`` = a raw-op module for CPU tensors (oracle.torch_ops).
    -> (Record, the copy's program, the copy)"""
    net = copy.deepcopy(case.net)
    prog = net_exec.NetProgram(net)  # (not cached on the network: only its flattening is used)
    net.use_native_executor = False
    net.train(training)
    if device is not None:
        net = net.to(device)
    dev = torch.device("cpu") if device is None else device
    before = _state(net)
    conv_out, bn_out, bn_stats = {}, {}, {}
    orig_bn_act = GF.bn_act
    conv_types = (spconv.SubMConv3d, spconv.SparseConv3d, spconv.SparseInverseConv3d)
    orig_fwd = {t: t.forward for t in conv_types}

    def bn_act(x, bn, relu, residual=None):
        y = orig_bn_act(x, bn, relu, residual)
        bn_out[id(bn)] = _cpu(y)
        saved = y.grad_fn.saved_tensors  # (_BnActFn: x, y, weight, mean, invstd)
        bn_stats[id(bn)] = (_cpu(saved[3]) if training else None, _cpu(saved[4]))
        return y

    def make_fwd(t):
        def fwd(self, x):
            y = orig_fwd[t](self, x)
            conv_out[id(self)] = _cpu(y.features)
            return y
        return fwd

    f = case.feats.to(dev).clone().requires_grad_(True)
    x = spconv.SparseConvTensor(f, case.idx.to(dev), case.shape, case.batch)
    ctx = backend.using(ops) if ops is not None else backend.using(backend.raw())
    try:
        GF.bn_act = bn_act
        for t in conv_types:
            t.forward = make_fwd(t)
        with ctx:
            y = net(x)
            (y.features * case.dy.to(dev)).sum().backward()
    finally:
        GF.bn_act = orig_bn_act
        for t in conv_types:
            t.forward = orig_fwd[t]
    levels = [(case.idx.cpu(), list(case.shape))]
    for lvl in range(prog.n_levels - 1):
        r = x.indice_dict[prog.level_keys[lvl][1]]
        levels.append((_cpu(r.out_indices), list(r.out_shape)))
    stem = prog.python_stem_conv
    x_prog = conv_out[id(stem)] if stem is not None else _cpu(f)
    kw = dict(training=training, inference=False, x=_cpu(f), levels=levels, stem_out=x_prog if stem is not None else None,
              state_before=before, state_after=_state(net), dy=case.dy.clone(), din=_cpu(f.grad),
              grads={k: _cpu(p.grad) for k, p in net.named_parameters()})
    return _assemble(prog, kw, conv_out, bn_out, bn_stats, x_prog), prog, net


def _slices(prog, state, live):
    """per-slot tensors and per-BatchNorm statistics of a forward pass's arena (rows behind the live count cut off)"""
    features, arena, stats, _slots, _ct, _bt, sizes, _params = state
    offs = np.concatenate([[0], np.cumsum(sizes)])
    slots = []
    for s in range(len(prog.slot_level)):
        ch, lv = int(prog.slot_channels_np[s]), prog.slot_level[s]
        t = features if s == 0 else arena[int(offs[s]):int(offs[s + 1])].view(-1, ch)
        slots.append(_cpu(t[:live[lv]]))
    mean = [_cpu(stats[0, int(prog.bn_off[j]):int(prog.bn_off[j + 1])]) for j in range(len(prog.bns))]
    invstd = [_cpu(stats[1, int(prog.bn_off[j]):int(prog.bn_off[j + 1])]) for j in range(len(prog.bns))]
    return slots, mean, invstd


def record_executor(nets, feats, idx, shape, batch, dy, mode, rows_dev=None):
    """what ``net_exec._NetFn`` / ``_NetPairFn`` do, by hand, on the GPU: the rulebooks, the tables, gpn_net_forward[_pair],
    every slot and statistic sliced out of the arena, gpn_net_backward[_pair], the training bookkeeping of ``run``.
    ``nets``: one network or two of the same structure (paired launches; ``dy`` then a pair); ``mode``: "train" | "eval" |
    "inference" (the networks are switched accordingly); ``rows_dev``: a hip_ops.DevCount - ``feats`` / ``idx`` / ``dy`` then have
    the rows of its bound.  -> [Record per network]"""
    training, inference = mode == "train", mode == "inference"
    pair = len(nets) == 2
    dys = [d.contiguous() for d in (dy if pair else [dy])]
    progs = []
    for net in nets:
        net.train(training)
        prog = net_exec.program_for(net)
        assert prog is not None
        progs.append(prog)
    prog = progs[0]
    dev = feats.device
    before = [_state(net) for net in nets]
    f = feats.clone().requires_grad_(not inference)
    x = spconv.SparseConvTensor(f, idx, shape, batch)
    stem = prog.python_stem_conv
    stem_feats = None
    with torch.set_grad_enabled(not inference):
        if stem is not None:
            assert not pair and rows_dev is None, "the 6-channel stem conv runs as a module in front of the program"
            x = stem(x)
            stem_feats = x.features
    lvl_dev = None
    if rows_dev is not None:
        x.rows_dev = rows_dev
        rows, rb_table, rb_objs, levels, lvl_dev = prog.rulebooks_dev(x)
    else:
        rows, rb_table, rb_objs, levels = prog.rulebooks(x)
    if training:
        with torch.no_grad():
            bufs = [b for p in progs for b in p.buffers("num_batches_tracked")]
            net_exec._count_batches(bufs, x)
    fmode = 1 if training else (net_exec.NET_INFERENCE if inference else 0)
    xin = x.features.detach().contiguous()
    states = [net_exec._forward_tables(xin, p, rows, lvl_dev)[1] for p in progs]
    if pair:
        net_exec._call_pair("gpn_net_forward_pair", prog, states[0][3], states[1][3], rb_table, states[0][4], states[1][4], states[0][5],
                            states[1][5], (fmode,), dev)
    else:
        net_exec._call("gpn_net_forward", prog, states[0][3], rb_table, states[0][4], states[0][5], (fmode,), dev)
    torch.cuda.synchronize()
    live = [int(c.t.item()) for c in lvl_dev] if lvl_dev is not None else [int(r) for r in rows]
    dins, views = [None] * len(nets), [None] * len(nets)
    if not inference:
        tabs = [net_exec._backward_tables(p, st, d.contiguous(), True) for p, st, d in zip(progs, states, dys)]
        extra = (1 if training else 0, 1)
        if pair:
            net_exec._call_pair("gpn_net_backward_pair", prog, tabs[0][1], tabs[1][1], rb_table, tabs[0][2], tabs[1][2], tabs[0][3],
                                tabs[1][3], extra, dev)
        else:
            net_exec._call("gpn_net_backward", prog, tabs[0][1], rb_table, tabs[0][2], tabs[0][3], extra, dev)
        torch.cuda.synchronize()
        for t, tab in enumerate(tabs):
            dins[t] = tab[0][:xin.numel()].view_as(xin)
            views[t] = tab[5]
    recs = []
    for t, (net, p, st) in enumerate(zip(nets, progs, states)):
        slots, mean, invstd = _slices(p, st, live)
        names = {id(m): n for n, m in net.named_modules()}
        grads, din = {}, None
        if not inference:
            mods = p.convs + p.bns + p.bns
            leaves = ["weight"] * (len(p.convs) + len(p.bns)) + ["bias"] * len(p.bns)
            grads = {f"{names[id(m)]}.{leaf}": _cpu(g) for m, leaf, g in zip(mods, leaves, views[t])}
            din = dins[t]
            if stem is not None:  # the stem conv's own backward, from the program's input gradient
                gw, gf = torch.autograd.grad(stem_feats, [stem.weight, f], din)
                grads[names[id(stem)] + ".weight"], din = _cpu(gw), gf
            din = _cpu(din[:live[0]])
        recs.append(Record(training=training, inference=inference, x=_cpu(feats[:live[0]]),
                           levels=[(_cpu(i[:n]), list(s)) for (i, s), n in zip(levels, live)],
                           stem_out=slots[0] if stem is not None else None, slots=slots,
                           save_mean=mean if training else [None] * len(mean), save_invstd=[None] * len(mean) if inference else invstd,
                           state_before=before[t], state_after=_state(net), dy=_cpu(dys[t][:live[0]]), din=din, grads=grads))
    return recs


# ------------------------------------------------------------------------------------------- stand-alone BatchNorm shapes
# hip_ops.bn_fwd / bn_bwd where the U-Net never goes: 2 rows, both sides of the small-kernel threshold of 1024 rows, C / 4 = 5 (the
# one-column small kernel at 900 rows, the reduce's ragged thread layout at 1025), the finalize path above 256 channels
BN_SHAPES = [(2, 16), (1024, 64), (1025, 16), (1025, 20), (900, 20), (3000, 320), (1500, 768)]
# fp32 floors of these shapes where they lie ABOVE the class floors of the U-Net cases (torch fp32 on one thread against float64,
# measured and checked by test_unet_ref_cpu.py::test_standalone_batchnorm_floor).  Only the input gradient of the 2-row training
# BatchNorm does: there dx = +-(g1 - g2) / 2 * eps / (var + eps) * w / std is what is left of O(|g|) terms that cancel to four
# digits, and max|dx| sits in the channel with the smallest variance, the worst conditioned one.
BN_FLOORS = {(2, 16): {"din": 8.80e-5}}


def bn_tol(N, C, cls):
    return MARGIN * max(FLOORS[cls], BN_FLOORS.get((N, C), {}).get(cls, 0.0))


def bn_inputs(N, C):
    """x = 2 N(0,1) + 0.5, a residual, dy, affine parameters and running statistics away from 1 / 0"""
    g = torch.Generator().manual_seed(100 * N + C)
    x = torch.randn((N, C), generator=g) * 2 + 0.5
    res, dy = torch.randn((N, C), generator=g), torch.randn((N, C), generator=g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) * 1.5 + 0.5
    return SimpleNamespace(x=x, res=res, dy=dy, w=w, b=b, rm=rm, rv=rv, eps=1e-4, momentum=0.1)


def bn_torch(inp, dtype, training, relu, has_res, mask=None):
    """this file's BatchNorm op and autograd in ``dtype`` -> (y, mean, invstd, dx, dres, dweight, dbias, running_mean, running_var)"""
    x, r, w, b = (t.detach().clone().to(dtype).requires_grad_(True) for t in (inp.x, inp.res, inp.w, inp.b))
    y, mean, invstd, rm, rv = batch_norm(x, w, b, inp.rm.to(dtype), inp.rv.to(dtype), training, inp.momentum, inp.eps,
                                         r if has_res else None, relu, mask)
    (y * inp.dy.to(dtype)).sum().backward()
    return y.detach(), mean.detach(), invstd.detach(), x.grad, r.grad if has_res else None, w.grad, b.grad, rm, rv


def bn_errors(inp, run):
    """``run(training, relu, has_res)`` (same outputs as bn_torch) against float64 over relu x residual x training
    -> [(class, what, (training, relu, has_res), error)]; save_invstd on the well-conditioned channels (2 rows: see the top)"""
    N, C = inp.x.shape
    out = []
    for training in (True, False):
        for relu in (False, True):
            for has_res in (False, True):
                y, mean, invstd, dx, dres, dw, db, rm, rv = (None if t is None else t.detach().cpu() for t in run(training, relu, has_res))
                ry, rmean, rinvstd, rdx, rdres, rdw, rdb, rrm, rrv = bn_torch(inp, torch.float64, training, relu, has_res, (y > 0) if relu else None)
                keep = well_conditioned(rmean, rinvstd) if training else torch.ones(C, dtype=torch.bool)
                assert N == 2 or bool(keep.all()), "2 N(0,1) + 0.5 is well conditioned"
                got = [("bn", "y", y, ry), ("stat", "invstd", invstd[keep], rinvstd[keep]), ("din", "dx", dx, rdx),
                       ("bn_grad", "dweight", dw, rdw), ("bn_grad", "dbias", db, rdb)]
                if training:
                    got += [("stat", "mean", mean, rmean), ("running", "running_mean", rm, rrm), ("running", "running_var", rv, rrv)]
                else:
                    assert torch.equal(rm, inp.rm.to(rm.dtype)) and torch.equal(rv, inp.rv.to(rv.dtype)) and torch.equal(mean, inp.rm.to(mean.dtype))
                assert (dres is not None) == has_res
                if has_res:
                    got.append(("din", "dres", dres, rdres))
                for cls, what, a, ref in got:
                    out.append((cls, what, (training, relu, has_res), rel_err(a, ref, scale=float((1.0 / rinvstd).max()) if what == "mean" else None)))
    return out
