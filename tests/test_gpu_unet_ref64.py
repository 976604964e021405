"""GPU: the sparse U-Net executor (csrc/net.hip, net_plan.h, net_wgrad.h), the layer-by-layer path and the stand-alone BatchNorm
kernels (csrc/bn.hip), op by op against float64, forward and backward.

The reference is tests/unet_ref64.py: a float64 walk of the program that is teacher-forced with the device's own activations, so
every op is compared on the device's own inputs and the backward pass is linearised at the device's forward pass (its docstring
says why an unforced end-to-end comparison cannot work).  tests/test_unet_ref_cpu.py pins that reference to a dense formulation
and to the module definition, and shows that the comparator reports eight kinds of single faults at the op they were injected in.

Cases (synth.surface_indices, block_repeat 2, BatchNorm1d(eps=1e-4, momentum=0.1) with randomised parameters and statistics,
N(0,1) features, a random fp32 dy shared by device and reference):
  A  [16,32,48,64], 6-channel stem, batch 3, 64^3     rows [5953,3513,1230,338]: both sides of kSmallRows = 1024, 8/4/2/1 slot sets
  B  [16..112] in steps of 16, no stem, batch 2, 96^3   rows [6748,4531,1737,488,129,30,2]: every width, one- and two-tile levels,
                                                        a 2-row level (unbiased factor 2) below a 3^3 level that drops a plane
  C  [16,32], no stem, batch 1, 24^3                    rows [140,109]: less than one workgroup of every kernel
  D  [16,32], 6-channel stem, one scene, 192^3          rows [22409,11816]: 32 slot sets, many-workgroup folds, a second apply round
Modes: training with the conv-epilogue BatchNorm sums on and off, eval with gradients (frozen statistics), inference (conv o
BatchNorm per launch, compared at that granularity, and bit-equal to eval).  Further forms: paired passes of two networks,
device-counted rows with NaN / out-of-grid garbage behind the live count, the layer-by-layer path, and hip_ops.bn_fwd / bn_bwd
at shapes the U-Net never reaches.

Tolerances are 8x the fp32 floor of the reference itself (unet_ref64.FLOORS: torch fp32 on one thread and the C oracle against
float64, measured on the CPU by test_unet_ref_cpu.py over all four cases, training and eval) - never a number taken from the
kernels.  Worst on the device: over every test of this file on an MI355X.

  class                         CPU floor   tolerance   worst on the device
  conv output                   1.60e-06    1.28e-05    4.40e-07  (B eval)
  BatchNorm output              3.40e-06    2.72e-05    8.51e-06  (stand-alone (2, 16); 7.25e-06 in B, sums not fused)
  save_mean / save_invstd       2.69e-07    2.15e-06    7.35e-07  (B training, sums not fused)
  running statistics            4.18e-07    3.34e-06    5.96e-08
  input gradient                5.78e-06    4.62e-05    3.43e-06  (B training, sums not fused)
  conv weight gradient          9.05e-06    7.24e-05    5.97e-06  (B training, sums not fused)
  BatchNorm dweight / dbias     1.56e-05    1.25e-04    8.71e-06  (B training, sums not fused)
With the sums fused (the default) case B stays below 2.1e-06 in every class, cases A, C and D below 1.7e-06.
The stand-alone shape (2, 16) has an fp32 floor of its own for the input gradient, 8.80e-05 (unet_ref64.BN_FLOORS says why):
tolerance 7.04e-04, on the device 2.31e-04.

All inputs are well conditioned (|mean| of the order of std per channel).  bn_reduce_kernel and bn_small_fwd_kernel accumulate x
and x^2 per thread in fp32 before widening; channels with |mean| >> std are a known property of those kernels and out of scope
here, as are the bf16 path and conv instantiation coverage (test_conv_instantiations.py).  A BatchNorm over 2 rows has such
channels whatever its inputs (|mean| / std is a ratio of two normals): there save_invstd is compared on the channels with
|mean| <= 8 std of the float64 statistics (unet_ref64.well_conditioned; 43 of case B's 4256 channels fall outside, none
elsewhere); the stand-alone kernels are off by up to 3.1e-05 on those, the fused sums by less than the tolerance.
"""
import copy
import functools

import pytest
import torch

from tests import unet_ref64 as U

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name, stem=None):
    return U.make_case(name, stem)


_GEOMS = {}


def _geom(name, rec):
    """the case's geometry, built once (the device lists coarse rows in ascending key order; any other order gets its own)"""
    g = _GEOMS.get(name)
    if g is None or len(g.idx) != len(rec.levels) or not all(torch.equal(a, b[0]) for a, b in zip(g.idx, rec.levels)):
        g = U.Geometry(rec.levels[0][0], rec.levels[0][1], len(rec.levels), coarse=[l[0] for l in rec.levels[1:]])
        _GEOMS.setdefault(name, g)
    return g


def _check(prog, net, rec, name, what):
    ref = U.reference_for(prog, net, rec, _geom(name, rec))
    report = U.compare(prog, net, rec, ref)
    print(f"\nobserved {what}: " + ", ".join(f"{c}={e:.2e}" for c, (e, _) in sorted(report.worst().items())) +
          f" (save_invstd left out as ill-conditioned: {report.skipped} of {report.channels} channels)")
    report.check(U.TOL, what)
    assert report.skipped <= 0.02 * report.channels, "ill-conditioned channels are the exception (2-row levels)"
    return report


@pytest.fixture
def bn_fusion(request):
    """conv-epilogue BatchNorm sums (csrc/bn_stats.h) on / off for one test"""
    from gapartnet_amd import _C
    prev = _C.lib().gpn_net_bn_fusion(1 if request.param else 0)
    yield bool(request.param)
    _C.lib().gpn_net_bn_fusion(prev)


def _on_device(case, cuda):
    return copy.deepcopy(case.net).to(cuda), case.feats.to(cuda), case.idx.to(cuda), case.dy.to(cuda)


MODES = [("train", True), ("train", False), ("eval", True), ("inference", True)]


@pytest.mark.parametrize("mode,bn_fusion", MODES, indirect=["bn_fusion"], ids=["train-fused", "train-unfused", "eval", "inference"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_executor_against_float64(cuda, name, mode, bn_fusion):
    from gapartnet_amd.network import net_exec
    case = _case(name)
    if name == "B":
        assert U.CASES["B"]["channels"] == list(range(16, 113, 16))
    net, feats, idx, dy = _on_device(case, cuda)
    rec = U.record_executor([net], feats, idx, case.shape, case.batch, dy, mode)[0]
    prog = net_exec.program_for(net)
    assert len(rec.levels) == len(U.CASES[name]["channels"]) and rec.levels[-1][0].shape[0] >= 2, "torch's training BatchNorm rejects 1 row"
    _check(prog, net, rec, name, f"{name} {mode} fusion={bn_fusion}")
    if mode == "inference":  # the header's promise: the same bits as the eval pass that keeps its BatchNorm launches
        twin = copy.deepcopy(case.net).to(cuda)
        ev = U.record_executor([twin], feats, idx, case.shape, case.batch, dy, "eval")[0]
        assert torch.equal(rec.slots[prog.out_slot], ev.slots[prog.out_slot])


def test_executor_against_float64_at_32_slot_sets(cuda):
    """case D, training with the fused sums: level 0 above 16384 rows"""
    from gapartnet_amd import _C
    from gapartnet_amd.network import net_exec
    assert _C.lib().gpn_net_bn_fusion(-1) == 1, "fusion is the default"
    case = _case("D")
    net, feats, idx, dy = _on_device(case, cuda)
    rec = U.record_executor([net], feats, idx, case.shape, case.batch, dy, "train")[0]
    assert rec.levels[0][0].shape[0] > 16384
    _check(net_exec.program_for(net), net, rec, "D", "D train fusion=True")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_paired_passes_against_float64(cuda, mode):
    """gpn_net_forward_pair / gpn_net_backward_pair: each of the two networks against its own reference, both outputs in the loss"""
    from gapartnet_amd.network import net_exec
    case = _case("A", False)
    net_a, feats, idx, dy_a = _on_device(case, cuda)
    torch.manual_seed(11)
    net_b = copy.deepcopy(net_a)
    with torch.no_grad():
        for p in net_b.parameters():
            p.add_(0.05 * torch.randn_like(p))
    dy_b = torch.randn(dy_a.shape, generator=torch.Generator().manual_seed(12)).to(cuda)
    recs = U.record_executor([net_a, net_b], feats, idx, case.shape, case.batch, (dy_a, dy_b), mode)
    for tag, net, rec in zip("ab", (net_a, net_b), recs):
        _check(net_exec.program_for(net), net, rec, "A", f"A pair {mode} network {tag}")


@pytest.mark.parametrize("name", ["A", "C"])
def test_device_counted_rows_against_float64(cuda, name):
    """the buffers have the rows of a bound (live + 37), the live count is a device counter; behind it the features are NaN and
    the indices out of the grid.  The reference sees the live rows only (the networks without the 6-channel stem conv, which
    runs as a module in front of the program and cannot take a counted tensor)"""
    from gapartnet_amd import hip_ops
    from gapartnet_amd.network import net_exec
    case = _case(name, False)
    net, feats, idx, dy = _on_device(case, cuda)
    live, pad = idx.shape[0], 37
    feats = torch.cat([feats, torch.full((pad, feats.shape[1]), float("nan"), device=cuda)])
    junk = torch.tensor([case.batch + 5, -1, case.shape[1] + 7, 1 << 20], dtype=torch.int32, device=cuda).repeat(pad, 1)
    idx = torch.cat([idx, junk])
    dy = torch.cat([dy, torch.randn((pad, dy.shape[1]), generator=torch.Generator().manual_seed(13)).to(cuda)])
    count = torch.tensor([live], dtype=torch.int64, device=cuda)
    rec = U.record_executor([net], feats, idx, case.shape, case.batch, dy, "train", rows_dev=hip_ops.DevCount(count, live + pad))[0]
    assert rec.levels[0][0].shape[0] == live and rec.x.shape[0] == live and rec.din.shape[0] == live
    report = _check(net_exec.program_for(net), net, rec, name, f"{name} device-counted train")
    assert all(e[3] == e[3] and e[3] != float("inf") for e in report.entries), "nothing compared may be NaN"


@pytest.mark.parametrize("name", ["A", "B"])
def test_layer_by_layer_path_against_float64(cuda, name):
    """use_native_executor = False: the stand-alone kernels behind hip_ops.bn_fwd / bn_bwd (bn_small_*, reduce + fold) and the conv
    ops one by one, through the same comparator"""
    rec, prog, net = U.record_modules(_case(name), True, device=cuda)
    _check(prog, net, rec, name, f"{name} layer by layer train")


@pytest.mark.parametrize("N,C", U.BN_SHAPES)
def test_standalone_batchnorm_against_float64(cuda, N, C):
    """hip_ops.bn_fwd / bn_bwd at the shapes of unet_ref64.BN_SHAPES, relu x residual x training, against the same float64
    BatchNorm op through the same error measure; tolerances of the classes (unet_ref64.bn_tol)"""
    from gapartnet_amd import hip_ops
    inp = U.bn_inputs(N, C)

    def run(training, relu, has_res):
        x, res, dy, w, b, rm, rv = (t.to(cuda) for t in (inp.x, inp.res, inp.dy, inp.w, inp.b, inp.rm, inp.rv))
        y, mean, invstd = hip_ops.bn_fwd(x, res if has_res else None, w, b, rm, rv, training, inp.momentum, inp.eps, relu)
        dx, dres, dw, db = hip_ops.bn_bwd(x, y, dy, w, mean, invstd, relu, training, has_res)
        return y, mean, invstd, dx, dres, dw, db, rm, rv

    errors = U.bn_errors(inp, run)
    worst = {}
    for cls, what, combo, err in errors:
        worst[cls] = max(worst.get(cls, 0.0), err)
    print(f"\nobserved bn ({N}, {C}): " + ", ".join(f"{c}={e:.2e}" for c, e in sorted(worst.items())))
    for cls, what, (training, relu, has_res), err in errors:
        assert err <= U.bn_tol(N, C, cls), f"({N}, {C}) training={training} relu={relu} residual={has_res}: {what} {err:.3e} > {U.bn_tol(N, C, cls):.3e}"
