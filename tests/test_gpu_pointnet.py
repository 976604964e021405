"""The PointNet backbone on the GPU: the module on the point-MLP kernels against the float64 restatement (the reference's
recorded run as the yardstick), against its own plain-torch path, and inside the model.

Tolerance of the parity tests: E = max|got - f64| / max|f64| per array must stay within 4 E_ref + 1e-6, E_ref being the same figure
for the fp32 result it is measured against (the reference's recorded CPU run on the fixture, the plain-torch path on the GPU at
the larger shape).  Both are fp32 evaluations of one graph that differ only in summation order, so their errors are of one size
class; 4 x admits reordering, and a semantic error (a missing ReLU, the wrong eps, the wrong layout) shows at 1e-2."""
import numpy as np
import pytest
import torch

from tests import pointnet_ref as R
from tests.test_pointnet_cpu import (check_against, fx, load_hash_weights, model_cfg, module_run, names_shapes,  # noqa: F401
                                     ref64)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_backbone_on_the_fixture(cuda, fx, names_shapes, ref64, mode):  # noqa: F811
    from gapartnet_amd.network.pointnet import PointNetSegBackbone
    bb = load_hash_weights(PointNetSegBackbone(3, 16), names_shapes).to(cuda)
    check_against(module_run(bb, fx, "reference", mode == "train"), ref64, mode, "gpu")


def _run_at(bb, points, cot, counts, layout, training):
    bb.train(training)
    pts = points.clone().requires_grad_(training)
    with torch.set_grad_enabled(training):
        out = bb.forward_rows(pts, counts, layout)
    res = {"out": out.detach().cpu().numpy()}
    if training:
        bb.zero_grad()
        (out * cot).sum().backward()
        res["grad.input"] = pts.grad.cpu().numpy()
        params = dict(bb.named_parameters())
        for n in R.GRAD_PARAMS:
            res["grad." + n] = R.recorded(params[n].grad.cpu().numpy())
        sd = bb.state_dict()
        for bn in R.STAT_BNS:
            for k in ("running_mean", "running_var"):
                res[f"stat.{bn}.{k}"] = sd[f"{bn}.{k}"].cpu().numpy()
    return res


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_native_path_against_the_torch_path(cuda, names_shapes, mode):  # noqa: F811
    """B = 2, N = 2048: both paths on the GPU against the float64 restatement at that shape; E_ref = the torch path's error"""
    from gapartnet_amd.network.pointnet import PointNetSegBackbone
    B, n = 2, 2048
    counts, training = [n] * B, mode == "train"
    points = R.hash_input(B, n)
    cot = (2.0 * R.hash_uniform("cotangent", B * n * 16) - 1.0).reshape(B * n, 16).astype(np.float32)
    ref = R.run_f64(names_shapes, points, counts, "reference", training, cot)
    got = {}
    for native in (False, True):
        bb = load_hash_weights(PointNetSegBackbone(3, 16), names_shapes).to(cuda)
        bb.use_native_kernels = native
        got[native] = _run_at(bb, torch.from_numpy(points).to(cuda), torch.from_numpy(cot).to(cuda), counts, "reference", training)
    bad = []
    for k, v in ref.items():
        e_ref, e = R.rel_err(got[False][k], v), R.rel_err(got[True][k], v)
        print(f"{mode}.{k:<40} E_torch {e_ref:.3e}   E_native {e:.3e}   bound {4 * e_ref + 1e-6:.3e}")
        if not e <= 4 * e_ref + 1e-6:
            bad.append((k, e, e_ref))
    assert not bad, bad


def _model_and_batch(cuda):
    from gapartnet_amd.network.model import GAPartNet
    from gapartnet_amd.smoke import make_batch
    torch.manual_seed(0)
    model = GAPartNet(**model_cfg(backbone_cfg={"pc_dim": 3, "feature_dim": 16, "channels": [16, 32, 48], "block_repeat": 2})).to(cuda)
    return model, [pc.to(cuda) for pc in make_batch(2, 2048)]


def test_model_training_and_validation_step(cuda):
    model, batch = _model_and_batch(cuda)
    model.train()
    params = dict(model.backbone.named_parameters())
    before = {k: p.detach().clone() for k, p in params.items()}
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    loss = model.training_step(batch, 0)
    assert torch.isfinite(loss)
    loss.backward()
    for k, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), k
    opt.step()
    for k, p in params.items():
        assert not torch.equal(p.detach(), before[k]), k
    model.eval()
    with torch.no_grad():
        pc_ids, sem_seg, kept = model.validation_step(batch, 0, 0)
    assert len(pc_ids) == 2
    assert sem_seg is not None


def test_eval_forward_stores_no_1024_wide_tensor(cuda, names_shapes):  # noqa: F811
    """checked through the profiler scope's byte count of GPN_K_POINTMLP (not the allocator's peak): the same forward in its
    training form stores the three 1024-wide activations for backward and otherwise moves the same data, so its launches must
    account at least three [B N, 1024] fp32 tensors more than the eval forward's - whose total stays below what the layers
    narrower than 1024 read and write plus one such tensor"""
    import ctypes
    from gapartnet_amd import _C
    from gapartnet_amd.network.pointnet import PointNetSegBackbone
    lib = _C.lib()
    K_POINTMLP = 8
    B, n = 2, 2048
    bb = load_hash_weights(PointNetSegBackbone(3, 16), names_shapes).to(cuda)
    pts = torch.from_numpy(R.hash_input(B, n)).to(cuda)

    def accounted(training):
        bb.train(training)
        lib.gpn_prof_reset()
        lib.gpn_prof_enable(1)
        try:
            with torch.set_grad_enabled(training):
                bb.forward_rows(pts, [n] * B, "reference")
            launches, ms, flops, nbytes = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            _C.check(lib.gpn_prof_get(K_POINTMLP, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(flops), ctypes.byref(nbytes)))
        finally:
            lib.gpn_prof_enable(0)
        return launches.value, nbytes.value

    wide = 4.0 * B * n * 1024
    launches, eval_bytes = accounted(False)
    _, train_bytes = accounted(True)
    print(f"GPN_K_POINTMLP bytes: eval {eval_bytes:.4g}, training form {train_bytes:.4g}, one [B N, 1024] tensor {wide:.4g}")
    assert launches >= 20, launches
    assert train_bytes - eval_bytes >= 3 * wide * 0.999, (eval_bytes, train_bytes, wide)
    # per row the narrower layers read and write 3484 floats in all (the layer list of the module), the weights are 3.5 M floats
    assert eval_bytes < 4.0 * (B * n * 3484 + 2 * 3.6e6) + wide, (eval_bytes, wide)
