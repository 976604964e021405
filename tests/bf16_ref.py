"""Host references of the bf16 inference path (include/gpn.h section C16): round-to-nearest-even fp32 -> bf16 in numpy bit
arithmetic, the float64 epilogue, and an EMULATED network pass that shares no code with the feature - the op list of a
NetProgram walked in Python with the existing fp32 ops only, on weights and activations rounded to bf16 and widened back.

bf16 values are carried as float32 arrays whose low 16 bits are zero ("widened") or as uint16 bit patterns."""
import numpy as np

# ---------------------------------------------------------------------------------------------------- rounding


def bf16_bits(x):
    """fp32 array -> uint16 bf16 bit patterns, round to nearest even (NaN stays a quiet NaN)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    rounded = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), rounded)


def widen(bits):
    """uint16 bf16 bit patterns -> float32 (exact)"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16(x):
    """fp32 array -> the nearest bf16 values (ties to even), as float32"""
    return widen(bf16_bits(x))


def torch_bits(t):
    """a torch.bfloat16 tensor's bit patterns as a uint16 numpy array"""
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def torch_from_bits(bits, device):
    """uint16 bit patterns -> torch.bfloat16 tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(device).view(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------- epilogue
def epilogue64(acc, bn=None, res=None, relu=False):
    """the conv epilogue / gpn_bn_act_bf16 in float64: v = (acc - mean) / sqrt(var + eps) * weight + bias, + res, max(0, .);
    ``bn`` = (mean, var, weight, bias, eps) or None.  No rounding: the caller compares against the stored value's bound."""
    v = np.asarray(acc, np.float64)
    if bn is not None:
        mean, var, weight, bias, eps = bn
        v = (v - np.asarray(mean, np.float64)) / np.sqrt(np.asarray(var, np.float64) + float(eps)) * np.asarray(weight, np.float64) \
            + np.asarray(bias, np.float64)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    if relu:
        v = np.maximum(v, 0.0)
    return v


# ---------------------------------------------------------------------------------------------------- network walks
def _torch_round(t):
    """torch float32 tensor -> rounded to bf16 and widened back (torch's own conversion: round to nearest even)"""
    import torch
    return t.to(torch.bfloat16).to(torch.float32)


def folded_ops(prog):
    """[(conv op or None, bn op or None, concat op or None)] groups of a NetProgram in launch order: a BatchNorm that directly and
    solely follows a conv rides in that conv's launch (the rule of gpn_net_forward's inference mode)"""
    ops = prog.ops
    readers = {}
    for kind, s0, s1, dst, rb, param, flags in ops:
        readers[s0] = readers.get(s0, 0) + 1
        if s1 >= 0:
            readers[s1] = readers.get(s1, 0) + 1
    groups, i = [], 0
    while i < len(ops):
        op = ops[i]
        if op[0] == 0:
            nxt = ops[i + 1] if i + 1 < len(ops) else None
            if nxt is not None and nxt[0] == 1 and nxt[1] == op[3] and readers.get(op[3], 0) == 1 and nxt[2] != op[3]:
                groups.append((op, nxt, None))
                i += 2
                continue
            groups.append((op, None, None))
        elif op[0] == 1:
            groups.append((None, op, None))
        else:
            groups.append((None, None, op))
        i += 1
    return groups


def emulated_pass(prog, features, rb_objs):
    """``yemu``: the program walked with EXISTING fp32 ops only (hip_ops.conv_fwd_ordered - the exact-fp32 MFMA, so products of
    bf16-valued operands are exact there too - and torch's eval BatchNorm arithmetic), weights and every stored activation rounded
    to bf16 and widened back, the output left unrounded.  ``rb_objs``: per rulebook index (rb, rb_t) as NetProgram.rulebooks
    returns them.  -> float32 [rows, C] on the device"""
    import torch
    from gapartnet_amd import hip_ops as H
    out_slot = prog.out_slot
    vals = {0: features}
    rounded0 = None

    def get(slot, as_bn_input=False):
        nonlocal rounded0
        if slot == 0 and not as_bn_input:
            if rounded0 is None:
                rounded0 = _torch_round(features)
            return rounded0
        return vals[slot]

    def bn_apply(v, op):
        bn = prog.bns[op[5]]
        y = (v - bn.running_mean) * (1.0 / torch.sqrt(bn.running_var + bn.eps)) * bn.weight + bn.bias
        if op[2] >= 0:
            y = y + get(op[2])
        if op[6] & 1:
            y = torch.relu(y)
        return y

    with torch.no_grad():
        for conv_op, bn_op, cat_op in folded_ops(prog):
            if conv_op is not None:
                conv = prog.convs[conv_op[5]]
                W = conv.weight.detach()
                W = W.reshape(W.shape[0], -1, W.shape[-1]) if W.dim() != 3 else W  # [Cout, K, Cin]
                Wk = _torch_round(W.permute(1, 2, 0).contiguous())                # [K, Cin, Cout], bf16 values
                v = H.conv_fwd_ordered(get(conv_op[1]).contiguous(), Wk, rb_objs[conv_op[4]][0])
                dst = conv_op[3]
                if bn_op is not None:
                    v = bn_apply(v, bn_op)
                    dst = bn_op[3]
            elif bn_op is not None:
                v = bn_apply(get(bn_op[1], as_bn_input=True), bn_op)
                dst = bn_op[3]
            else:
                v = torch.cat([get(cat_op[1]), get(cat_op[2])], dim=1)
                dst = cat_op[3]
            vals[dst] = v if dst == out_slot else _torch_round(v)
    return vals[out_slot]


def chained_pass(prog, features, rb_objs):
    """the same walk through the single-op bf16 wrappers (hip_ops.conv_pack_bf16 / conv_fwd_bf16 / rows_to_bf16 / bn_act_bf16;
    torch.cat stands for the concat of two bf16 slots): what gpn_net_forward_bf16 must equal bit for bit.  The output-producing
    launch writes fp32."""
    import torch
    from gapartnet_amd import hip_ops as H
    out_slot = prog.out_slot
    vals = {}
    f16 = None

    def get(slot):
        nonlocal f16
        if slot == 0:
            if f16 is None:
                f16 = H.rows_to_bf16(features)
            return f16
        return vals[slot]

    def bn_args(op):
        bn = prog.bns[op[5]]
        return (bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), bn.eps)

    with torch.no_grad():
        for conv_op, bn_op, cat_op in folded_ops(prog):
            if conv_op is not None:
                conv = prog.convs[conv_op[5]]
                W = conv.weight.detach()
                W = W.reshape(W.shape[0], -1, W.shape[-1]) if W.dim() != 3 else W  # parameter layout [Cout, K, Cin]
                packed = H.conv_pack_bf16(W.contiguous(), layout="oki")
                dst = bn_op[3] if bn_op is not None else conv_op[3]
                kw = {}
                if bn_op is not None:
                    kw = dict(bn=bn_args(bn_op), res=get(bn_op[2]) if bn_op[2] >= 0 else None, relu=bool(bn_op[6] & 1))
                v = H.conv_fwd_bf16(get(conv_op[1]), packed, rb_objs[conv_op[4]][0], conv.in_channels, conv.out_channels,
                                    out_f32=dst == out_slot, **kw)
            elif bn_op is not None:
                dst = bn_op[3]
                assert dst != out_slot, "this walk has no fp32-output BatchNorm launch"
                mean, var, weight, bias, eps = bn_args(bn_op)
                x = features if bn_op[1] == 0 else get(bn_op[1])
                v = H.bn_act_bf16(x, weight, bias, mean, var, eps, bool(bn_op[6] & 1), res=get(bn_op[2]) if bn_op[2] >= 0 else None)
            else:
                dst = cat_op[3]
                v = torch.cat([get(cat_op[1]), get(cat_op[2])], dim=1)
            vals[dst] = v
    return vals[out_slot]
