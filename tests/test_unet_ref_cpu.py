"""CPU: pin the float64 U-Net reference (tests/unet_ref64.py), measure its fp32 floor, and prove that the comparator has teeth.

1. dense equivalence   walk_modules == a dense conv3d / conv_transpose3d formulation (no pair list of any kind), 1e-12
2. program             walk_program, unforced, == walk_modules, 1e-12: NetProgram's flattening against the module definition
3. self-consistency    forced with its own float64 recording: forward residuals <= 1e-14, gradients == plain float64 autograd
4. floor               fp32 evaluations of the reference (torch fp32; the C oracle through record_modules) against float64 for every
                       case of the GPU test, training and eval: the numbers behind unet_ref64.FLOORS, from which the GPU test's
                       tolerances are 8x
5. teeth               eight single faults injected into a clean fp32 pass of case A: each is reported at the GPU test's tolerances,
                       and at the op it was injected into
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gapartnet_amd.network import net_exec
from tests import unet_ref64 as U


@functools.lru_cache(maxsize=None)
def _case(name, stem=None):
    return U.make_case(name, stem)


@functools.lru_cache(maxsize=None)
def _geom(name):
    c = _case(name)
    return U.Geometry(c.idx, c.shape, len(U.CASES[name]["channels"]))


def _prog(case):
    return net_exec.program_for(case.net)


# ------------------------------------------------------------------------------------------------- 1. dense equivalence
def _dense_unet(net, P, idx, shape, batch, x, training):
    """the U-Net on dense [B, X, Y, Z, C] grids: torch's conv3d / conv_transpose3d, active sets by max-pooling the occupancy,
    BatchNorm over the active rows (which ``grid[mask]`` lists in ascending key order - the order of ``idx``)"""
    i = idx.long()
    mask0 = torch.zeros((batch, *shape), dtype=torch.bool)
    mask0[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
    assert torch.equal(mask0.nonzero().to(idx.dtype), idx), "rows must come in ascending key order"

    def grid(rows, mask):
        return torch.zeros((*mask.shape, rows.shape[1]), dtype=rows.dtype).index_put(mask.nonzero(as_tuple=True), rows)

    def bn(m, g, mask, relu, res=None):
        y = P.bn(m, g[mask], training, None if res is None else res[mask], relu)[0]
        return grid(y, mask)

    def conv(m, g, mask, pad):
        w = P.w(m).permute(0, 4, 1, 2, 3)
        return F.conv3d(g.permute(0, 4, 1, 2, 3), w, padding=pad).permute(0, 2, 3, 4, 1) * mask[..., None]

    def conv_bn(seq, g, mask, relu, res=None):
        c, b = list(seq._modules.values())[:2]
        return bn(b, conv(c, g, mask, 1 if c.kernel_size == [3, 3, 3] else 0), mask, relu, res)

    def resblock(blk, g, mask):
        skip = g if isinstance(blk.shortcut, nn.Identity) else conv_bn(blk.shortcut, g, mask, False)
        return conv_bn(blk.conv2, conv_bn(blk.conv1, g, mask, True), mask, True, res=skip)

    def ublock(ub, g, mask):
        for blk in ub.encoder_blocks._modules.values():
            g = resblock(blk, g, mask)
        if len(ub.channels) == 1:
            return g
        skip = g
        down, dbn, _ = ub.downsample._modules.values()
        up, ubn, _ = ub.upsample._modules.values()
        coarse = F.max_pool3d(mask[:, None].double(), 2)[:, 0] > 0  # (floor mode: an odd extent drops its last plane)
        d = F.conv3d(g.permute(0, 4, 1, 2, 3), P.w(down).permute(0, 4, 1, 2, 3), stride=2).permute(0, 2, 3, 4, 1)
        d = ublock(ub.ublock, bn(dbn, d, coarse, True), coarse)
        u = F.conv_transpose3d(d.permute(0, 4, 1, 2, 3), P.w(up).permute(4, 0, 1, 2, 3), stride=2)
        u = F.pad(u, [v for s, t in reversed(list(zip(mask.shape[1:], u.shape[2:]))) for v in (0, s - t)])
        g = torch.cat([bn(ubn, u.permute(0, 2, 3, 4, 1) * mask[..., None], mask, True), skip], dim=-1)
        for blk in ub.decoder_blocks._modules.values():
            g = resblock(blk, g, mask)
        return g

    g = grid(x, mask0)
    stem = list(net.stem._modules.values())
    g = conv_bn(net.stem, g, mask0, True) if len(stem) == 3 else bn(stem[0], g, mask0, True)
    return ublock(net.ublock, g, mask0)[mask0]


@pytest.mark.parametrize("stem", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_walk_modules_equals_a_dense_formulation(stem, training):
    """grid [16, 15, 13] (odd extents: the dropped last plane, in the down conv and in its inverse), batch 2, channels [16, 32]"""
    import numpy as np
    from tests import synth
    shape, batch = [16, 15, 13], 2
    rng = np.random.default_rng(5)
    idx = synth.random_sparse_indices(rng, batch, shape, 300)
    idx = torch.from_numpy(idx[np.lexsort((idx[:, 3], idx[:, 2], idx[:, 1], idx[:, 0]))])
    assert int(idx[:, 2].max()) == 14 and int(idx[:, 3].max()) == 12, "voxels in the dropped planes"
    torch.manual_seed(1)
    cin = 6 if stem else 16
    net = U.SparseUNet.build(cin, [16, 32], 2, functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1), without_stem=not stem)
    x = torch.randn((idx.shape[0], cin), dtype=torch.float64)
    dy = torch.randn((idx.shape[0], 16), dtype=torch.float64)
    geom = U.Geometry(idx, shape, 2)
    results = []
    for dense in (False, True):
        P = U.Params(net, net.state_dict(), torch.float64)
        xi = x.clone().requires_grad_(True)
        y = _dense_unet(net, P, idx, shape, batch, xi, training) if dense else U.walk_modules(net, P, geom, xi, training)
        (y * dy).sum().backward()
        results.append((y.detach(), xi.grad, P.grads(), P.after))
    (y, din, grads, after), (yd, dind, gradsd, afterd) = results
    assert U.rel_err(y, yd) < 1e-12 and U.rel_err(din, dind) < 1e-12
    for k in gradsd:
        assert U.rel_err(grads[k], gradsd[k]) < 1e-12, k
    for k in afterd:
        assert U.rel_err(after[k], afterd[k]) < 1e-12, k


# ------------------------------------------------------------------------------------------------- 2. program == definition
@pytest.mark.parametrize("stem", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_walk_program_unforced_equals_walk_modules(stem, training):
    case = _case("A", stem)
    prog, geom = _prog(case), _geom("A")
    assert (prog.python_stem_conv is not None) == stem
    rec = U.record_walk(case, training, torch.float64, geom)
    P = U.Params(case.net, case.net.state_dict(), torch.float64)
    x = case.feats.double().requires_grad_(True)
    y = U.walk_modules(case.net, P, geom, x, training)
    (y * case.dy.double()).sum().backward()
    assert U.rel_err(rec.slots[prog.out_slot], y) < 1e-12
    assert U.rel_err(rec.din, x.grad) < 1e-12
    want = P.grads()
    assert set(want) == set(rec.grads) == {n for n, _ in case.net.named_parameters()}
    for k in want:
        assert U.rel_err(rec.grads[k], want[k]) < 1e-12, k
    for k, v in P.after.items():
        assert U.rel_err(rec.state_after[k], v) < 1e-12, k
        assert training == (not torch.equal(v, P.t[k])), f"{k}: buffers move in training and only there"


# ------------------------------------------------------------------------------------------------- 3. self-consistency
@pytest.mark.parametrize("training", [True, False])
def test_forced_with_its_own_recording_changes_nothing(training):
    case = _case("A")
    prog, geom = _prog(case), _geom("A")
    rec = U.record_walk(case, training, torch.float64, geom)
    ref = U.reference_for(prog, case.net, rec, geom)
    report = U.compare(prog, case.net, rec, ref)
    for cls, label, op, err in report.entries:
        assert err <= (1e-14 if cls in ("conv", "bn", "stat", "running", "exact") else 1e-12), (label, cls, err)
    assert len([e for e in report.entries if e[0] in ("wgrad", "bn_grad")]) == len(list(case.net.parameters()))


# ------------------------------------------------------------------------------------------------- 4. floor
MODES = [("A", True), ("A", False), ("B", True), ("B", False), ("C", True), ("C", False), ("D", True), ("D", False)]


@functools.lru_cache(maxsize=None)
def _floor(name, training):
    """worst error per class of the two fp32 evaluations of one case (eval mode also at the inference form's granularity: conv
    outputs unforced, conv o BatchNorm compared)"""
    import copy
    from oracle import torch_ops
    case, geom = _case(name), _geom(name)
    worst = {}

    def take(report, tag):
        for cls, (err, label) in report.worst().items():
            if err > worst.get(cls, (0.0, ""))[0]:
                worst[cls] = (err, f"{tag}: {label}")
        assert not [e for e in report.entries if e[0] == "exact" and e[3] > 0], tag

    def run(prog, net, rec, tag):
        take(U.compare(prog, net, rec, U.reference_for(prog, net, rec, geom)), tag)
        if not training:
            inf = copy.copy(rec)
            inf.inference, inf.din, inf.save_invstd = True, None, [None] * len(rec.save_invstd)
            take(U.compare(prog, net, inf, U.reference_for(prog, net, inf, geom)), tag + " (inference form)")

    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # sequential fp32 sums: the yardstick of the margin, and the same figure on every machine
    try:
        rec32 = U.record_walk(case, training, torch.float32, geom)
    finally:
        torch.set_num_threads(threads)
    run(_prog(case), case.net, rec32, "torch fp32")
    rec, prog, net = U.record_modules(case, training, ops=torch_ops)
    for (got, _), want in zip(rec.levels, geom.idx):
        assert torch.equal(got, want), "the oracle lists coarse rows in ascending key order"
    run(prog, net, rec, "oracle")
    return worst


@pytest.mark.parametrize("name,training", MODES)
def test_floor(name, training):
    worst = _floor(name, training)
    print(f"\nfloor {name} {'train' if training else 'eval'}: " + ", ".join(f"{c} {worst[c][0]:.2e}" for c in U.CLASSES if c in worst))
    for cls, (err, where) in worst.items():
        assert err <= 1.5 * U.FLOORS[cls], f"{cls}: fp32 floor {err:.3e} at {where} exceeds the table's {U.FLOORS[cls]:.3e}"


def test_floor_table_is_what_was_measured():
    """unet_ref64.FLOORS is neither behind the measurement nor padded: the worst over all cases, re-measured here, lies within
    [1/4, 3/2] of every entry (the slack is for other vector widths and BLAS blockings than the machine the table was taken on)"""
    worst = {}
    for name, training in MODES:
        for cls, (err, where) in _floor(name, training).items():
            worst[cls] = max(worst.get(cls, 0.0), err)
    print("\nclass      measured   table      tolerance")
    for cls in U.CLASSES:
        print(f"{cls:10s} {worst[cls]:.3e}  {U.FLOORS[cls]:.3e}  {U.TOL[cls]:.3e}")
        assert U.FLOORS[cls] / 4 <= worst[cls] <= 1.5 * U.FLOORS[cls], cls
        assert U.TOL[cls] == 8 * U.FLOORS[cls]
    assert max(U.TOL.values()) < 3e-3 / 20, "far below a dropped row at the 338-row level (3e-3); the teeth tests show each fault caught"


def test_standalone_batchnorm_floor():
    """the stand-alone BatchNorm shapes of the GPU test in torch fp32 (one thread) against float64: within the class floors,
    except where unet_ref64.BN_FLOORS says so - and those entries are what is measured"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for N, C in U.BN_SHAPES:
            inp = U.bn_inputs(N, C)
            worst = {}
            for cls, what, combo, err in U.bn_errors(inp, lambda *mode: U.bn_torch(inp, torch.float32, *mode)):
                if err > worst.get(cls, (0.0, ""))[0]:
                    worst[cls] = (err, f"{what} training, relu, residual = {combo}")
            print(f"\nfloor bn ({N}, {C}): " + ", ".join(f"{c} {e:.2e}" for c, (e, _) in sorted(worst.items())))
            own = U.BN_FLOORS.get((N, C), {})
            for cls, (err, where) in worst.items():
                assert err <= 1.5 * max(U.FLOORS[cls], own.get(cls, 0.0)), f"({N}, {C}) {cls}: fp32 floor {err:.3e} at {where}"
            for cls, floor in own.items():
                assert floor > U.FLOORS[cls] and floor / 4 <= worst[cls][0], f"({N}, {C}) {cls}: the table says {floor:.3e}, measured {worst[cls][0]:.3e}"
    finally:
        torch.set_num_threads(threads)


# ------------------------------------------------------------------------------------------------- 5. teeth
def _ops_of(prog, kind, level, relu=None, res=None):
    out = []
    for i, (k, s0, s1, dst, rb, param, flags) in enumerate(prog.ops):
        if k == kind and prog.slot_level[dst] == level and (relu is None or bool(flags & 1) == relu) and (res is None or (s1 >= 0) == res):
            out.append(i)
    return out


def _faulty_report(kind, op):
    case = _case("A")
    prog, geom = _prog(case), _geom("A")
    rec = U.record_walk(case, True, torch.float32, geom, fault=(op, kind) if op is not None else None)
    if kind == "din_last_row":
        rec.din = rec.din.clone()
        rec.din[-1] = 0
    return prog, U.compare(prog, case.net, rec, U.reference_for(prog, case.net, rec, geom))


def test_a_clean_fp32_pass_is_reported_clean():
    prog, report = _faulty_report(None, None)
    report.check(U.TOL, "clean")


def test_teeth_forward_faults_are_reported_at_their_op():
    prog = _prog(_case("A"))
    assert _geom("A").rows == [5953, 3513, 1230, 338]
    faults = [("stats_without_last_row", _ops_of(prog, net_exec.OP_BN, 3)[1]),       # statistics of a 338-row BatchNorm over 337 rows
              ("drop_tap_tile", _ops_of(prog, net_exec.OP_CONV, 1)[2]),              # one tap of one 16-row tile missing from a conv
              ("no_residual", _ops_of(prog, net_exec.OP_BN, 2, res=True)[0]),        # the residual left out of one BatchNorm
              ("concat_swapped", _ops_of(prog, net_exec.OP_CONCAT, 0)[0]),           # the two concat halves swapped
              ("biased_running_var", _ops_of(prog, net_exec.OP_BN, 3)[2])]           # running_var from the biased variance, N = 338
    for kind, op in faults:
        _, report = _faulty_report(kind, op)
        bad = report.failures(U.TOL)
        assert bad, f"{kind}: not noticed"
        forward = [e for e in bad if e[0] in ("conv", "bn", "stat", "running", "exact")]
        assert forward and {e[2] for e in forward} == {op}, (kind, op, [(e[1], e[3]) for e in forward[:5]])
        if kind == "biased_running_var":
            assert [e[0] for e in bad] == ["running"] and bad[0][1].endswith("running_var"), bad
            assert bad[0][3] < 3e-3, "a fault of momentum / N of the variance: the smallest of these faults"


def test_teeth_backward_faults_are_reported_at_their_op():
    """a fault in one op's backward spoils every gradient computed after it (the ops before it in program order) and none computed
    before it: the failing parameter gradient with the highest op index names the op"""
    prog = _prog(_case("A"))
    faults = [("mask_from_x", _ops_of(prog, net_exec.OP_BN, 1, relu=True, res=True)[1]),   # backward ReLU mask from x instead of y
              ("dweight_without_a_block", _ops_of(prog, net_exec.OP_BN, 2, relu=True)[1])]  # dweight without one 32-row block
    for kind, op in faults:
        _, report = _faulty_report(kind, op)
        bad = report.failures(U.TOL)
        assert bad and all(e[0] in ("din", "wgrad", "bn_grad") for e in bad), (kind, [(e[1], e[3]) for e in bad[:5]])
        assert max(e[2] for e in bad if e[2] is not None) == op, (kind, op, [(e[1], e[3]) for e in bad[:5]])
        if kind == "dweight_without_a_block":
            assert [e[1].split(" d")[-1] for e in bad] == ["weight"], bad
    _, report = _faulty_report("din_last_row", None)  # the last live row's gradient missing from the input gradient
    bad = report.failures(U.TOL)
    assert [e[0] for e in bad] == ["din"], bad
