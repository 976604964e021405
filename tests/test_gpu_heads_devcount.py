"""GPU: the dense heads (csrc/linear.hip) over their supported range against float64, and the device-counted (hip_ops.DevCount)
variants of the head, max-pool, instance-IoU and gather / scatter kernels against their host-counted forms.

DevCount's contract: the tensors are allocated for a bound, the live count is read on the device, `plan` only sizes grids -
results never depend on it.  So for every plan in {0, 1, live, bound} the live rows must be torch.equal to the host-counted
call on the truncated inputs (dW / db too: the extra workgroups contribute exact zeros in the same summation slots)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gapartnet_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------ H
# cin = 4 (below every earlier test; (4, <= 4): the group-reduction scratch is larger than the row tiles), the row-group form at
# its limit (16 x 32: 128 owners, 2 groups) and just past it (16 x 33, 12 x 43: 132 / 129 owners, ungrouped, threads with 0 - 1
# pairs), threads owning 1 - 2 pairs (64 x 17) and 3 - 4 (60 x 64), odd cout, the 128-row tile at exactly 64 KB of LDS (64 x 63)
HEAD_PAIRS = [(4, 1), (4, 2), (4, 3), (4, 4), (4, 5), (4, 64), (8, 1), (12, 7), (16, 32), (16, 33), (60, 64), (64, 16), (64, 17),
              (64, 63), (12, 43)]
HEAD_CASES = [(300, ci, co) for ci, co in HEAD_PAIRS] + [(n, ci, co) for n in (1, 127, 128, 129)
                                                         for ci, co in ((4, 2), (16, 32), (64, 63))]


@pytest.mark.parametrize("n,cin,cout", HEAD_CASES)
@pytest.mark.parametrize("bias", [True, False])
def test_dense_heads_over_the_supported_range(H, cuda, n, cin, cout, bias):
    """the assertions and the tolerance of test_gpu_ops.test_dense_heads_match_torch: float64 F.linear, values and the three
    gradients at 1e-5 relative to the tensor's largest entry, two runs bit-equal, unneeded outputs not computed"""
    import torch.nn.functional as F
    from gapartnet_amd import functional as GF
    assert H.linear_supported(cin, cout)
    g = torch.Generator().manual_seed(1000 * n + 64 * cin + cout)
    x = torch.randn(n, cin, generator=g).to(cuda).requires_grad_(True)
    w = (torch.randn(cout, cin, generator=g) * 0.2).to(cuda).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(cuda).requires_grad_(True) if bias else None
    dy = torch.randn(n, cout, generator=g).to(cuda)
    leaves = [x, w] + ([b] if bias else [])
    ref = F.linear(x.double(), w.double(), b.double() if bias else None)
    gref = torch.autograd.grad(ref, leaves, dy.double())
    got = GF.linear(x, w, b)
    ggot = torch.autograd.grad(got, leaves, dy)

    def close(a, r):
        err, tol = float((a.double() - r.double()).abs().max()), 1e-5 * max(1.0, float(r.abs().max()))
        print(f"n={n} {cin}->{cout} max err {err:.3e} tol {tol:.3e}")
        return err <= tol
    assert close(got, ref)
    for a, r in zip(ggot, gref):
        assert close(a, r)
    again = torch.autograd.grad(GF.linear(x, w, b), leaves, dy)
    assert all(torch.equal(a, c) for a, c in zip(ggot, again)), "fixed summation order"
    dx, dw, db = H.linear_bwd(x.detach(), w.detach(), dy, False, True, False)
    assert dx is None and db is None and torch.equal(dw, ggot[1])


# ------------------------------------------------------------------------------------------------ DEV
def _count(H, cuda, live, plan):
    return H.DevCount(torch.tensor([live], dtype=torch.int64, device=cuda), plan)


def _plans(live, bound):
    return sorted({0, 1, live, bound})


@pytest.mark.parametrize("live", [0, 700, 1000])
@pytest.mark.parametrize("cin,cout", [(16, 10), (4, 2), (64, 63)])
def test_device_counted_linear(H, cuda, cin, cout, live):
    """gpn_linear_fwd_dev / gpn_linear_bwd_dev, bound 1000 rows: live = 0, 700 (ends inside the sixth 128-row workgroup of the
    dW pass) and the bound; plan = 1 launches ONE forward workgroup that strides over all rows"""
    bound = 1000
    g = torch.Generator().manual_seed(bound + cin + cout + live)
    x = torch.randn(bound, cin, generator=g).to(cuda)
    w = (torch.randn(cout, cin, generator=g) * 0.2).to(cuda)
    b = torch.randn(cout, generator=g).to(cuda)
    dy = torch.randn(bound, cout, generator=g).to(cuda)
    y0 = H.linear_fwd(x[:live].contiguous(), w, b)
    dx0, dw0, db0 = H.linear_bwd(x[:live].contiguous(), w, dy[:live].contiguous(), True, True, True)
    for plan in _plans(live, bound):
        rows = _count(H, cuda, live, plan)
        assert torch.equal(H.linear_fwd(x, w, b, rows=rows)[:live], y0), plan
        dx, dw, db = H.linear_bwd(x, w, dy, True, True, True, rows=rows)
        assert torch.equal(dx[:live], dx0), plan
        assert torch.equal(dw, dw0) and torch.equal(db, db0), plan


def _tiny_segments(cuda, n_seg, rows_per):
    begin = torch.arange(n_seg, dtype=torch.int32, device=cuda) * rows_per
    return begin, begin + rows_per


@pytest.mark.parametrize("live", [0, 1300, 1500])
def test_device_counted_maxpool(H, cuda, live):
    """gpn_segmented_maxpool_fwd_dev / _bwd_dev over a bound of 1500 twenty-row segments: more than the 1024-workgroup floor of
    the device-counted grids, so with plan = 1 the workgroups really stride over segments"""
    bound, rows_per, C = 1500, 20, 16
    g = torch.Generator().manual_seed(live)
    vals = torch.randn(bound * rows_per, C, generator=g).to(cuda)
    vals[40:60] = vals[40]  # ties
    begin, end = _tiny_segments(cuda, bound, rows_per)
    dp = torch.randn(bound, C, generator=g).to(cuda)
    m_live = live * rows_per
    p0, a0 = H.segmented_maxpool_fwd(vals, begin[:live].contiguous(), end[:live].contiguous())
    dv0 = H.segmented_maxpool_bwd(dp[:live].contiguous(), a0, m_live)
    for plan in _plans(live, bound):
        p, a = H.segmented_maxpool_fwd(vals, begin, end, rows=_count(H, cuda, live, plan))
        assert torch.equal(p[:live], p0) and torch.equal(a[:live], a0), plan
        # (the arg-max rows past the live count are undefined: the backward gets the host-counted table there)
        arg = torch.cat([a0, torch.full((bound - live, C), -1, dtype=torch.int32, device=cuda)])
        dv = H.segmented_maxpool_bwd(dp, arg, bound * rows_per, rows=_count(H, cuda, live, plan),
                                     m_rows=_count(H, cuda, m_live, plan * rows_per))
        assert torch.equal(dv[:m_live], dv0), plan


@pytest.mark.parametrize("live", [0, 1300, 1500])
def test_device_counted_instance_iou(H, cuda, live):
    """gpn_instance_iou_dev over a bound of 1500 twenty-point proposals (above the 1024-workgroup floor: plan = 1 strides)"""
    bound, rows_per, B, I = 1500, 20, 4, 9
    rng = np.random.default_rng(live)
    offs = torch.arange(bound + 1, dtype=torch.int32, device=cuda) * rows_per
    pb = np.sort(rng.integers(0, B, bound)).astype(np.int32)
    bi = torch.from_numpy(np.repeat(pb, rows_per)).to(cuda)
    il = torch.from_numpy(rng.integers(-1, I, bound * rows_per).astype(np.int32)).to(cuda)
    npi = rng.integers(1, 60, (B, I)).astype(np.int32)
    npi[:, -1] = 0
    npi = torch.from_numpy(npi).to(cuda)
    want = H.instance_iou(offs[:live + 1].contiguous(), il, bi, npi)
    assert live == 0 or float(want.max()) > 0
    for plan in _plans(live, bound):
        got = H.instance_iou(offs, il, bi, npi, rows=_count(H, cuda, live, plan))
        assert torch.equal(got[:live], want), plan


@pytest.mark.parametrize("live", [0, 89000, 90000])
@pytest.mark.parametrize("C", [16, 3])
def test_device_counted_gather_and_scatter_rows(H, cuda, C, live):
    """gpn_gather_rows_dev (live length of idx) and gpn_scatter_rows_csr_dev (live number of table rows), bound 90000 rows:
    above the 1024-workgroup floor for both the float4 (C = 16) and the scalar (C = 3) kernels, so plan = 1 strides; a large
    plan takes the four-elements-per-thread gather"""
    bound = 90000
    rng = np.random.default_rng(C + live)
    table = torch.from_numpy(rng.normal(size=(3000, C)).astype(np.float32)).to(cuda)
    idx = torch.from_numpy(rng.integers(-1, 3000, bound).astype(np.int32)).to(cuda)
    want = H.gather_rows(table, idx[:live].contiguous())
    for plan in _plans(live, bound):
        got = H.gather_rows(table, idx, rows=_count(H, cuda, live, plan))
        assert torch.equal(got[:live], want), plan
    # scatter: 80000 gradient rows into a table of (bound) 90000 rows of which `live` exist
    n = 80000
    dout = torch.from_numpy(rng.normal(size=(n, C)).astype(np.float32)).to(cuda)
    sidx = torch.from_numpy(rng.integers(-1, max(live, 1), n).astype(np.int32)).to(cuda)
    order, starts = H.rows_csr(sidx, bound)
    want = H.scatter_rows(dout, sidx, live, csr=(order, starts[:live + 1].contiguous()))
    for plan in _plans(live, bound):
        got = H.scatter_rows(dout, sidx, bound, csr=(order, starts), rows=_count(H, cuda, live, plan))
        assert torch.equal(got[:live], want), plan
