"""The bf16 inference conv (csrc/spconv_bf16.hip, include/gpn.h section C16) and its elementwise kernels on the GPU.

(a) packing rounds to nearest even; (b) every instantiation against the float64 reference of tests/conv_ref64.py over a
declarative case table; (c) gpn_rows_to_bf16 / gpn_bn_act_bf16.

Inputs of (b) are fp32 randoms rounded to bf16 (exact operands), weights arbitrary fp32; the reference is conv_ref64.fwd on the
input and the numpy-rounded weights, then the float64 epilogue.  A product of two bf16 values is exact in fp32, so the only kernel
error before the store is fp32 accumulation, and the bounds are derived, not tuned:
  fp32 output:  max|got - ref| <= 1e-4 max(1, max|ref|)                       (the project's conv bound, test_gpu_conv_shapes.TOL)
  bf16 output:  |got - ref| <= 2^-8 |ref| + 1e-4 max(1, max|ref|) elementwise  (half a bf16 ulp is at most 2^-8 |x|)
Also per case: rows without any pair are exactly 0 with no epilogue; two runs are bit-equal; voxel order and tile order are
bit-equal; a forward into a sentinel-filled buffer touches nothing past n_dst x cout elements; the profiler's kernel names show
that the instantiation the case names is the one that ran.  tests/test_bf16_cpu.py checks that the table reaches every
instantiation the source builds."""
import dataclasses
import os
import re
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import oracle as O
from tests import bf16_ref as B
from tests import conv_ref64 as R64
from tests.test_gpu_conv_shapes import down_fine_rows, down_indices, subm_indices

pytestmark = pytest.mark.gpu

TOL = 1e-4
HALF_ULP = 2.0 ** -8
BF16_CB = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14)

_DEMANGLED = re.compile(r"(?<![A-Za-z0-9_])spconv_bf16_kernel<(\d+), (\d+)>")
_MANGLED = re.compile(r"18spconv_bf16_kernelILi(\d+)ELi(\d+)EE")


def bf16_kernel_id(name):
    """profiler kernel name (demangled or Itanium-mangled) -> (CB, NT) of a spconv_bf16_kernel instantiation, else None"""
    m = _DEMANGLED.search(name) or _MANGLED.search(name)
    return (int(m.group(1)), int(m.group(2))) if m else None


def cols_per_wave(nt_total):
    """restated from csrc/spconv_bf16.hip: the widest divisor (<= 7) of the layer's column tiles"""
    for d in range(min(nt_total, 7), 1, -1):
        if nt_total % d == 0:
            return d
    return 1


def route(K, n_dst, cin, cout):
    """restated from csrc/spconv_bf16.hip: one wave per row tile with the widest divisor of the column tiles, whatever K and the
    row count"""
    return (cin // 16, cols_per_wave(cout // 16))


@dataclass(frozen=True)
class Case:
    id: str
    kind: str   # "subm" (K = 27), "down" (K = 8, stride 2), "inv" (K = 8, the inverse conv: fine rows out), "ident" (K = 1)
    n: int      # subm / ident: rows; down: coarse (destination) rows; inv: coarse (SOURCE) rows, 1 + i % 8 fine rows each
    cin: int
    cout: int
    seed: int = 0

    @property
    def K(self):
        return {"subm": 27, "down": 8, "inv": 8, "ident": 1}[self.kind]

    @property
    def n_dst(self):
        return down_fine_rows(self.n) if self.kind == "inv" else self.n

    @property
    def instantiation(self):
        return route(self.K, self.n_dst, self.cin, self.cout)


def _cases():
    cs = []
    tails = (1, 15, 17, 33, 3001, 500)
    i = 0
    # every CB x every NT (cout = 16 NT, NT <= 7: the widest divisor is NT itself) at k = 1
    for cb in BF16_CB:
        for nt in range(1, 8):
            n = tails[i % len(tails)]
            cs.append(Case(f"ident-cb{cb}-nt{nt}-n{n}", "ident", n, 16 * cb, 16 * nt, seed=1000 + i))
            i += 1
    # every CB on the three rulebook kinds with more than one tap, over every output width
    kinds = ("subm", "down", "inv")
    for j, cb in enumerate(BF16_CB):
        for m, kind in enumerate(kinds):
            n = (3001, 700, 300)[m] if (j + m) % 2 == 0 else tails[(j + m) % 4]
            cs.append(Case(f"{kind}-cb{cb}-n{n}", kind, n, 16 * cb, 16 * (1 + (j + 2 * m) % 7), seed=1500 + 3 * j + m))
    # the tile tails on every rulebook kind, at a width with an odd 16-channel block and one without
    for kind in ("subm", "down", "inv", "ident"):
        for n in (1, 15, 17, 33):
            cs.append(Case(f"tail-{kind}-48to32-n{n}", kind, n, 48, 32, seed=2000 + n))
            cs.append(Case(f"tail-{kind}-64to48-n{n}", kind, n, 64, 48, seed=2100 + n))
    # more column tiles than a wave takes: 8 -> 2 groups of 4, 11 -> 11 groups of 1, 12 -> 2 groups of 6, 14 -> 2 groups of 7
    for cout in (128, 176, 192, 224):
        cs.append(Case(f"groups-subm-32to{cout}", "subm", 6000, 32, cout, seed=3000 + cout))
    # tens of thousands of rows at k = 27 / 8: the network's large levels, a decoder's 2c -> c, the stride-2 / inverse pair
    cs += [Case("wide-subm-32to32", "subm", 33000, 32, 32, seed=11), Case("wide-subm-96to48", "subm", 22000, 96, 48, seed=12),
           Case("wide-subm-48to112", "subm", 9400, 48, 112, seed=17), Case("wide-down-16to32", "down", 33000, 16, 32, seed=13),
           Case("wide-inv-32to16", "inv", 15000, 32, 16, seed=14), Case("wide-subm-224to112", "subm", 9400, 224, 112, seed=15)]
    # one bench-size level: level 0 of 8 x 20k-point scenes (~144k voxels), 16 -> 16, k = 27
    cs.append(Case("bench-level0-16to16", "subm", 144000, 16, 16, seed=16))
    return cs


CASES = _cases()


def expected_instantiations():
    """{(CB, NT)} the case table launches (imported by the CPU coverage check)"""
    return {c.instantiation for c in CASES}


class Inputs:
    def __init__(self, case, cuda):
        from gapartnet_amd import hip_ops as H
        rng = np.random.default_rng(case.seed)
        K, cin, cout = case.K, case.cin, case.cout
        if case.kind == "subm":
            idx, shape = subm_indices(rng, case.n)
            rb = H.rulebook_subm3(torch.from_numpy(idx).to(cuda), shape)
            pairs = O.rulebook_subm3(idx, shape)
        elif case.kind in ("down", "inv"):
            idx, shape = down_indices(rng, case.n)
            _, _, rb_fwd, rb_bwd = H.rulebook_down(torch.from_numpy(idx).to(cuda), shape, 1)
            d = O.rulebook_down(idx, shape)
            assert d["out_indices"].shape[0] == case.n and idx.shape[0] == down_fine_rows(case.n)
            rb, pairs = (rb_fwd, d["fwd"]) if case.kind == "down" else (rb_bwd, d["bwd"])
        else:
            n = case.n
            rb = H.rulebook_identity(n, cuda)
            pairs = (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.array([[0, n]], np.int32))
        self.rb_voxel = dataclasses.replace(rb, nbr_p=None, perm=None)
        perm, nbr_p = H.tile_order(rb.nbr, rb.K, rb.n_dst)
        self.rb_tiles = dataclasses.replace(rb, nbr_p=nbr_p, perm=perm)
        n_src, n_dst = rb.n_src, rb.n_dst
        self.n_dst = n_dst
        assert n_dst == case.n_dst
        self.f = B.round_bf16(rng.normal(size=(n_src, cin)).astype(np.float32))                 # exact bf16 operands
        self.W = (rng.normal(size=(K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)        # arbitrary fp32
        self.res = B.round_bf16(rng.normal(size=(n_dst, cout)).astype(np.float32))
        self.bn = (rng.normal(0.0, 0.3, cout).astype(np.float32), rng.uniform(0.5, 2.0, cout).astype(np.float32),
                   rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0.0, 0.2, cout).astype(np.float32), 1e-4)
        self.acc = R64.fwd(self.f, B.round_bf16(self.W), pairs, n_dst)
        self.empty = np.setdiff1d(np.arange(n_dst), pairs[1])
        self.fd = B.torch_from_bits(B.bf16_bits(self.f), cuda)
        self.resd = B.torch_from_bits(B.bf16_bits(self.res), cuda)
        self.bnd = tuple(torch.from_numpy(a).to(cuda) for a in self.bn[:4]) + (self.bn[4],)
        self.packed = H.conv_pack_bf16(torch.from_numpy(self.W).to(cuda))


# (bn, res, relu, out_f32): each part of the epilogue alone, all together, and nothing - in both output formats
VARIANTS = [(False, False, False, False), (False, False, False, True), (True, False, False, False), (False, True, False, False),
            (False, False, True, False), (True, True, True, False), (True, True, True, True), (True, True, False, True)]


def _sentinel_run(H, inp, case, rb, cuda, kw, out_f32):
    n_out = inp.n_dst * case.cout
    pad = 4096 + 17
    dt = torch.float32 if out_f32 else torch.bfloat16
    big = torch.empty((n_out + pad,), dtype=dt, device=cuda)
    ints = big.view(torch.int32 if out_f32 else torch.int16)
    sentinel = 0x7FC0DEAD if out_f32 else 0x7FC5  # (NaN bit patterns no kernel produces)
    ints.fill_(sentinel)
    out = big[:n_out].view(inp.n_dst, case.cout)
    H.conv_fwd_bf16(inp.fd, inp.packed, rb, case.cin, case.cout, out_f32=out_f32, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((ints[n_out:] == sentinel).all()), "the forward wrote past the end of its output"
    return out.clone()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_bf16_conv_instantiation_vs_float64(cuda, case):
    from gapartnet_amd import hip_ops as H
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    inp = Inputs(case, cuda)
    ran = set()
    report = []
    try:
        outs = []
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            for with_bn, with_res, relu, out_f32 in VARIANTS:
                kw = dict(bn=inp.bnd if with_bn else None, res=inp.resd if with_res else None, relu=relu)
                a = H.conv_fwd_bf16(inp.fd, inp.packed, inp.rb_voxel, case.cin, case.cout, out_f32=out_f32, **kw)
                a2 = H.conv_fwd_bf16(inp.fd, inp.packed, inp.rb_voxel, case.cin, case.cout, out_f32=out_f32, **kw)
                t = H.conv_fwd_bf16(inp.fd, inp.packed, inp.rb_tiles, case.cin, case.cout, out_f32=out_f32, **kw)
                s = _sentinel_run(H, inp, case, inp.rb_voxel, cuda, kw, out_f32)
                outs.append((a, a2, t, s))
            torch.cuda.synchronize()
        for e in prof.key_averages():
            k = bf16_kernel_id(e.key)
            if k is not None:
                ran.add(k)
            assert R64.kernel_id(e.key) is None, f"an fp32 conv kernel ran: {e.key}"
        for (with_bn, with_res, relu, out_f32), (a, a2, t, s) in zip(VARIANTS, outs):
            what = f"{case.id} bn={with_bn} res={with_res} relu={relu} out_f32={out_f32}"
            assert a.dtype == (torch.float32 if out_f32 else torch.bfloat16)
            view = (lambda x: x) if out_f32 else (lambda x: x.view(torch.int16))
            assert torch.equal(view(a), view(a2)), f"{what}: two runs differ"
            assert torch.equal(view(a), view(t)), f"{what}: voxel order and tile order differ"
            assert torch.equal(view(a), view(s)), f"{what}: the run into the sentinel buffer differs"
            ref = B.epilogue64(inp.acc, inp.bn if with_bn else None, inp.res if with_res else None, relu)
            got = a.float().cpu().numpy().astype(np.float64)
            scale = max(1.0, float(np.max(np.abs(ref))))
            err = np.abs(got - ref)
            if out_f32:
                bound = TOL * scale
                worst = float(err.max())
                report.append(f"{what}: max err {worst:.3e} / bound {bound:.3e}")
                assert worst <= bound, report[-1]
            else:
                bound = HALF_ULP * np.abs(ref) + TOL * scale
                worst = float((err / bound).max())
                report.append(f"{what}: worst err / bound {worst:.3f}")
                assert worst <= 1.0, report[-1]
            if not (with_bn or with_res) and len(inp.empty):
                assert not np.any(got[inp.empty]), f"{what}: rows without a pair are not exactly 0"
        print("\n".join(report))
        assert ran == {case.instantiation}, f"expected spconv_bf16_kernel<{case.instantiation}> to run, ran {sorted(ran)}"
    finally:
        del inp
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- (a) packing
@pytest.mark.parametrize("cin,cout,layout", [(48, 32, "kio"), (64, 112, "oki"), (16, 16, "kio"), (224, 48, "oki")])
def test_packing_rounds_to_nearest_even(cuda, cin, cout, layout):
    """weights of exact ties and near-ties, one-hot bf16 inputs, K = 1: the fp32 output IS the packed weight, element by element"""
    from gapartnet_amd import hip_ops as H
    rng = np.random.default_rng(cin + cout)
    base = B.round_bf16(rng.normal(size=(cin, cout)).astype(np.float32))
    ulp = np.ldexp(np.float32(1.0), np.frexp(np.abs(base))[1] - 8).astype(np.float32)  # one bf16 ulp of base (|base| in [2^(e-1), 2^e))
    kind = rng.integers(0, 5, size=base.shape)
    W = base.copy()
    W[kind == 0] += (ulp / 2)[kind == 0]                                   # exact ties: to the even neighbour
    W[kind == 1] -= (ulp / 4)[kind == 1]                                   # (a tie or inside, depending on the exponent edge)
    W[kind == 2] = np.nextafter(W[kind == 2] + (ulp / 2)[kind == 2], np.float32(np.inf), dtype=np.float32)   # just above a tie
    W[kind == 3] = np.nextafter(W[kind == 3] + (ulp / 2)[kind == 3], np.float32(-np.inf), dtype=np.float32)  # just below a tie
    W[0, 0], W[0, 1] = np.float32(1.0 + 2.0 ** -8), np.float32(1.0 + 3 * 2.0 ** -8)  # -> 1, 1 + 2^-6
    W = W.astype(np.float32)
    want = B.round_bf16(W)
    assert want[0, 0] == 1.0 and want[0, 1] == np.float32(1.0 + 2.0 ** -6)
    assert np.count_nonzero(want != base) > 0 and np.count_nonzero(want == base) > 0
    stored = torch.from_numpy(W.T.copy().reshape(cout, 1, cin) if layout == "oki" else W.reshape(1, cin, cout)).to(cuda)
    packed = H.conv_pack_bf16(stored, layout=layout)
    eye = torch.eye(cin, device=cuda).to(torch.bfloat16)
    out = H.conv_fwd_bf16(eye, packed, H.rulebook_identity(cin, cuda), cin, cout, out_f32=True)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # and the packed buffer holds exactly those values, each once
    assert np.array_equal(np.sort(B.torch_bits(packed)), np.sort(B.bf16_bits(W).reshape(-1)))


# ---------------------------------------------------------------------------------------------------- (c) elementwise kernels
@pytest.mark.parametrize("n,C", [(1, 16), (1000, 16), (777, 48), (5, 3)])
def test_rows_to_bf16_is_round_to_nearest_even(cuda, n, C):
    from gapartnet_amd import hip_ops as H
    rng = np.random.default_rng(n + C)
    x = (rng.normal(size=(n, C)) * 10.0 ** rng.uniform(-3, 3, size=(n, C))).astype(np.float32)
    x.reshape(-1)[:4] = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, np.inf][: min(4, x.size)]
    y = H.rows_to_bf16(torch.from_numpy(x).to(cuda))
    assert y.dtype == torch.bfloat16 and y.shape == (n, C)
    assert np.array_equal(B.torch_bits(y), B.bf16_bits(x))


@pytest.mark.parametrize("x_f32", [True, False])
@pytest.mark.parametrize("with_res,relu", [(False, False), (True, False), (False, True), (True, True)])
def test_bn_act_bf16_vs_float64(cuda, x_f32, with_res, relu):
    """bound: half a bf16 ulp (2^-8 |ref|) plus a few fp32 roundings of the affine expression at |x| <~ 10 (1e-5 max(1, max|ref|))"""
    from gapartnet_amd import hip_ops as H
    rng = np.random.default_rng(5)
    n, C = 3001, 48
    x = (3.0 * rng.normal(size=(n, C))).astype(np.float32)
    if not x_f32:
        x = B.round_bf16(x)
    res = B.round_bf16(rng.normal(size=(n, C)).astype(np.float32))
    bn = (rng.normal(0.0, 0.3, C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32),
          rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0.0, 0.2, C).astype(np.float32), 1e-4)
    xd = torch.from_numpy(x).to(cuda) if x_f32 else B.torch_from_bits(B.bf16_bits(x), cuda)
    mean, var, weight, bias = (torch.from_numpy(a).to(cuda) for a in bn[:4])
    y = H.bn_act_bf16(xd, weight, bias, mean, var, bn[4], relu, res=B.torch_from_bits(B.bf16_bits(res), cuda) if with_res else None)
    y2 = H.bn_act_bf16(xd, weight, bias, mean, var, bn[4], relu, res=B.torch_from_bits(B.bf16_bits(res), cuda) if with_res else None)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    ref = B.epilogue64(x, bn, res if with_res else None, relu)
    got = y.float().cpu().numpy().astype(np.float64)
    bound = HALF_ULP * np.abs(ref) + 1e-5 * max(1.0, float(np.max(np.abs(ref))))
    worst = float((np.abs(got - ref) / bound).max())
    print(f"bn_act_bf16 x_f32={x_f32} res={with_res} relu={relu}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


def test_bf16_ops_refuse_autograd_and_wrong_dtypes(cuda):
    from gapartnet_amd import _C, hip_ops as H
    rb = H.rulebook_identity(32, cuda)
    W = torch.randn(1, 16, 16, device=cuda)
    packed = H.conv_pack_bf16(W)
    x = torch.randn(32, 16, device=cuda)
    with pytest.raises(_C.GpnError, match="inference-only"):
        H.rows_to_bf16(x.clone().requires_grad_(True))
    with pytest.raises(_C.GpnError, match="inference-only"):
        H.conv_pack_bf16(W.clone().requires_grad_(True))
    with pytest.raises(_C.GpnError, match="bfloat16"):
        H.conv_fwd_bf16(x, packed, rb, 16, 16)
    with pytest.raises(_C.GpnError, match="inference-only"):
        H.bn_act_bf16(x.clone().requires_grad_(True), torch.ones(16, device=cuda), torch.zeros(16, device=cuda),
                      torch.zeros(16, device=cuda), torch.ones(16, device=cuda), 1e-4, True)
