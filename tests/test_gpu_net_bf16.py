"""The bf16 inference pass of the sparse U-Net (gpn_net_forward_bf16, SparseUNet.inference_dtype) on the GPU.

(d) the executor is the chain of its ops: bit-equal to walking the op list through the single-op wrappers;
(e) the network against fp32, with the margin taken from an emulation that shares no code with the feature (tests/bf16_ref.py):
    y32 = today's inference pass, yemu = the op list on existing fp32 ops with bf16-rounded weights and activations, ybf = the new
    path; D = |yemu - y32| / |y32| is what bf16 storage costs by itself, and |ybf - y32| / |y32| <= 1.5 D,
    |ybf - yemu| / |yemu| <= 2 D: ybf and yemu are two realisations of the same rounding process that differ in fp32 summation
    order - each as far from fp32 as the other (ratio ~ 1), at most sqrt(2) D from each other; a kernel that truncates instead of
    rounding sits at 13 in a CPU model of this;
(f) the knob does what it says and nothing else."""
import copy

import numpy as np
import pytest
import torch

from tests import bf16_ref as B
from tests import conv_ref64 as R64
from tests.test_gpu_conv_bf16 import bf16_kernel_id
from tests.test_gpu_model import _unet_case

pytestmark = pytest.mark.gpu


def _randomise_norms(net):
    """non-trivial running statistics and affine parameters"""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 2.0)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.2)


def _program_inputs(net, x):
    """(program, features the program starts from, rulebook objects) of one pass: the 6-channel stem conv of the backbone runs as an
    fp32 module in front of the program"""
    from gapartnet_amd.network import net_exec
    prog = net_exec.program_for(net)
    assert prog is not None
    if prog.python_stem_conv is not None:
        x = prog.python_stem_conv(x)
    rows, rb_table, rb_objs, levels = prog.rulebooks(x)
    return prog, x.features.contiguous(), rb_objs


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _three_outputs(net, make_x):
    """(y32, yemu, ybf, chained) of one network on one input"""
    net.eval()
    with torch.no_grad():
        net.inference_dtype = None
        y32 = net(make_x()).features.clone()
        x = make_x()
        prog, feats, rb_objs = _program_inputs(net, x)
        yemu = B.emulated_pass(prog, feats, rb_objs)
        chained = B.chained_pass(prog, feats, rb_objs)
        net.inference_dtype = torch.bfloat16
        ybf = net(make_x()).features.clone()
        ybf2 = net(make_x()).features.clone()
    assert ybf.dtype == torch.float32 and ybf.shape == y32.shape
    assert torch.equal(ybf, ybf2), "two bf16 passes differ"
    return y32, yemu, ybf, chained


@pytest.mark.parametrize("without_stem", [False, True])
def test_bf16_pass_is_the_chain_of_its_ops_and_tracks_fp32(cuda, without_stem):
    net, idx, feats, spconv = _unet_case(cuda, without_stem)
    _randomise_norms(net)

    def make_x():
        return spconv.SparseConvTensor(feats.clone(), idx, [64, 64, 64], 3)

    y32, yemu, ybf, chained = _three_outputs(net, make_x)
    # (d) fold logic, residual wiring, concat and buffer layout: the executor's output is the chain's, bit for bit
    assert chained.dtype == torch.float32
    assert torch.equal(ybf, chained), f"executor vs chained single ops: {_rel(ybf, chained):.3e} relative"
    # (e)
    D = _rel(yemu, y32)
    r32, remu = _rel(ybf, y32) / D, _rel(ybf, yemu) / D
    print(f"test U-Net without_stem={without_stem}: D = {D:.4e}, |ybf - y32| / |y32| = {r32:.3f} D, |ybf - yemu| / |yemu| = {remu:.3f} D")
    assert torch.isfinite(ybf).all()
    assert 0 < D < 0.1, D  # (bf16 storage costs something, and not everything)
    assert r32 <= 1.5, (r32, D)
    assert remu <= 2.0, (remu, D)


def test_bf16_pass_full_backbone_figures(cuda):
    """the full backbone (channels [16, ..., 112], 8 x 20k points): the same three outputs and margins; D and both ratios are
    printed for DESIGN.md"""
    from gapartnet_amd.smoke import make_batch, make_model
    from tests.golden import recipe
    model = make_model((0, 0))
    model.load_state_dict(recipe.name_keyed_state(model))
    model = model.to(cuda).eval()
    batch = [pc.to(cuda) for pc in make_batch(8, 20000, seed0=4100)]
    with torch.no_grad():
        vt = model._collate(batch).voxel_tensor
    feats, idx, shape, bs = vt.features.clone(), vt.indices, list(vt.spatial_shape), vt.batch_size
    from gapartnet_amd.spconv import pytorch as spconv

    def make_x():
        return spconv.SparseConvTensor(feats.clone(), idx, shape, bs)

    y32, yemu, ybf, chained = _three_outputs(model.backbone, make_x)
    assert torch.equal(ybf, chained), f"executor vs chained single ops: {_rel(ybf, chained):.3e} relative"
    D = _rel(yemu, y32)
    r32, remu = _rel(ybf, y32) / D, _rel(ybf, yemu) / D
    print(f"full backbone, {feats.shape[0]} voxels: D = {D:.4e}, |ybf - y32| / |y32| = {r32:.3f} D, |ybf - yemu| / |yemu| = {remu:.3f} D")
    assert r32 <= 1.5, (r32, D)
    assert remu <= 2.0, (remu, D)


def _conv_kernels(prof):
    bf16, fp32 = set(), set()
    for e in prof.key_averages():
        if bf16_kernel_id(e.key) is not None:
            bf16.add(bf16_kernel_id(e.key))
        k = R64.kernel_id(e.key)
        if k is not None and k[0] != "wgrad":
            fp32.add(k)
    return bf16, fp32


def _eval_model(cuda, inference_dtype):
    from gapartnet_amd.smoke import DEFAULT_CFG
    from gapartnet_amd.network.model import GAPartNet
    from tests.golden import recipe
    cfg = copy.deepcopy(DEFAULT_CFG)
    cfg["training_schedule"] = [0, 0]
    torch.manual_seed(0)
    model = GAPartNet(**cfg, inference_dtype=inference_dtype)
    model.load_state_dict(recipe.name_keyed_state(model))
    model = model.to(cuda)
    model.revoxelize_jitter = (torch.tensor([0.3, 0.6, 0.1], device=cuda), torch.tensor([0.5, 0.2, 0.9], device=cuda))
    model._log_sink = lambda name, value, bs, sync: None
    return model


def test_knob_runs_the_backbone_in_bf16_and_nothing_else(cuda):
    from gapartnet_amd.smoke import make_batch
    batch = [pc.to(cuda) for pc in make_batch(4, 20000, seed0=1700)]
    on, off = _eval_model(cuda, torch.bfloat16), _eval_model(cuda, None)
    assert on.inference_dtype is torch.bfloat16 and on.backbone.inference_dtype is torch.bfloat16
    assert off.inference_dtype is None
    assert on.score_unet.inference_dtype is None and on.npcs_unet.inference_dtype is None  # the proposal networks stay fp32
    on.eval(), off.eval()
    # the backbone pass alone: the bf16 kernel and no fp32 conv kernel of the program
    with torch.no_grad():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            ids_on, seg_on, kept_on = on.validation_step(batch, 0, 0)
            torch.cuda.synchronize()
        bf16_all, _ = _conv_kernels(prof)
        assert bf16_all, "the validation step launched no bf16 conv kernel"
        ids_off, seg_off, kept_off = off.validation_step(batch, 0, 0)
    assert ids_on == ids_off
    assert seg_on.sem_preds.shape == seg_off.sem_preds.shape
    differ = float((seg_on.sem_preds != seg_off.sem_preds).float().mean())
    print(f"validation step, 4 x 20k points: semantic argmax differs from the fp32 pass at {100 * differ:.3f} % of the points")
    # the backbone alone, on the voxel tensor of the same batch
    from gapartnet_amd.spconv import pytorch as spconv
    rng = np.random.default_rng(3)
    from tests import synth
    idx = torch.from_numpy(synth.surface_indices(rng, 2, [128, 128, 128], 9000)).to(cuda)
    feats = torch.from_numpy(rng.normal(size=(idx.shape[0], 6)).astype(np.float32)).to(cuda)
    with torch.no_grad():
        on.backbone(spconv.SparseConvTensor(feats.clone(), idx, [128, 128, 128], 2))  # (rulebooks, caches)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            y = on.backbone(spconv.SparseConvTensor(feats.clone(), idx, [128, 128, 128], 2)).features
            torch.cuda.synchronize()
    bf16, fp32 = _conv_kernels(prof)
    assert torch.isfinite(y).all() and y.dtype == torch.float32
    assert bf16, "the backbone pass launched no bf16 conv kernel"
    # the 6-channel stem conv runs as an fp32 module in front of the program (one launch, 6 -> 16 padded): nothing else is fp32
    n_fp32 = sum(e.count for e in prof.key_averages() if (R64.kernel_id(e.key) or ("wgrad",))[0] != "wgrad")
    assert n_fp32 <= 1, f"fp32 conv kernels of the program ran in a bf16 pass: {sorted(fp32, key=str)}"
    # with gradients enabled the eval pass is today's fp32 pass, bit for bit; so is a training step
    with torch.enable_grad():
        a = on.backbone(spconv.SparseConvTensor(feats.clone(), idx, [128, 128, 128], 2)).features
        b = off.backbone(spconv.SparseConvTensor(feats.clone(), idx, [128, 128, 128], 2)).features
    assert torch.equal(a, b), "an eval pass with gradients enabled must keep the fp32 path"
    with torch.enable_grad():
        ids_a, seg_a, kept_a = on.validation_step(batch, 0, 0)
        ids_b, seg_b, kept_b = off.validation_step(batch, 0, 0)
    assert torch.equal(seg_a.sem_preds, seg_b.sem_preds)
    on.train(), off.train()
    small = [pc.to(cuda) for pc in make_batch(2, 5000, seed0=1900)]
    loss_a = on.training_step(small, 0)
    loss_b = off.training_step(small, 0)
    assert torch.equal(loss_a.detach(), loss_b.detach()), "a training step must not depend on the knob"
    loss_a.backward(), loss_b.backward()
    for (n, p), (_, q) in zip(on.backbone.named_parameters(), off.backbone.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), n


def test_bf16_pass_rejects_what_it_does_not_cover(cuda):
    """device-counted rows keep the fp32 path (the proposal networks); run_pair ignores the knob"""
    from gapartnet_amd.network import net_exec
    net, idx, feats, spconv = _unet_case(cuda, True)
    twin = copy.deepcopy(net)
    net.eval(), twin.eval()
    net.inference_dtype = twin.inference_dtype = torch.bfloat16
    with torch.no_grad():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            pair = net_exec.run_pair(net, twin, spconv.SparseConvTensor(feats.clone(), idx, [64, 64, 64], 3))
            torch.cuda.synchronize()
        net.inference_dtype = twin.inference_dtype = None
        ref = net_exec.run_pair(net, twin, spconv.SparseConvTensor(feats.clone(), idx, [64, 64, 64], 3))
    bf16, _ = _conv_kernels(prof)
    assert pair is not None and not bf16
    assert torch.equal(pair[0].features, ref[0].features) and torch.equal(pair[1].features, ref[1].features)
