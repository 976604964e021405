"""The dense point-MLP kernels (csrc/pointmlp.hip, include/gpn.h section PM) on the GPU against the float64 statement of their
contracts (tests/pointnet_ref.py), over a declarative case table.

The bound is derived, not tuned: the kernels are fp32 fma chains, so elementwise
    |got - ref64| <= gamma_n A,    gamma_n = n u / (1 - n u),  u = 2^-24,
with n = the number of terms of the sum plus 4 (bias, G and the two operations of the affine epilogue) and A the float64 value
of the same expression with every operand replaced by its absolute value.  n = cin + 4 forward, cout + 4 for the data gradient,
N + 4 for the weight gradient.  ReLU and max are 1-Lipschitz, so the bound passes through them; a segment's maximum takes the
largest row bound of the segment.

Per case: forward (Y and M) within the bound; two runs bit-equal; the max-only form (Y == NULL) bit-equal to the maxima of the
stored form; a run into sentinel-filled buffers changes nothing past N x cout (S x cout for M); dgrad and wgrad within the
bound; wgrad bit-equal across two runs.  The shapes are the smallest at which the kernels can go wrong: one row, rows around the
16-row MFMA tile and the 128-row workgroup tile, segment boundaries inside a tile and on a tile's edge, a one-row segment, both
column-tile instantiations (cout <= 64 and above), K below / at / above the 16-wide LDS stage, widths that are no multiple of 4."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

from tests import pointnet_ref as R

pytestmark = pytest.mark.gpu


@dataclass(frozen=True)
class Case:
    id: str
    cin: int
    cout: int
    counts: Tuple[int, ...]            # rows per segment
    offsets: bool = True               # False: S == 1 without an offsets array
    view: Optional[str] = None         # "reference" (6N, N, 1) / "points" (6N, 1, 6): X~ is a strided view of a flat array
    per_segment: bool = False
    bias: bool = False
    G: bool = False
    affine: bool = False
    relu: bool = False

    @property
    def N(self):
        return sum(self.counts)


CASES = [
    Case("6-64-strided-reference", 6, 64, (43, 43, 43), view="reference"),                       # N = 129, no epilogue
    Case("6-64-strided-points", 6, 64, (500, 500), view="points", bias=True, affine=True, relu=True),  # N = 1000
    Case("6-64-per-segment-3x3-in-6", 6, 64, (1, 126), per_segment=True, bias=True),             # N = 127, a one-row segment
    Case("64-128", 64, 128, (300, 1, 699), bias=True, affine=True, relu=True),                   # N = 1000, boundaries inside tiles
    Case("128-1024-affine-only", 128, 1024, (129,), offsets=False, bias=True, affine=True),      # the encoder's bn3 form
    Case("64-512-G", 64, 512, (100, 27), bias=True, G=True, affine=True, relu=True),             # N = 127
    Case("512-256-relu-only", 512, 256, (17,), relu=True),
    Case("256-16", 256, 16, (128, 872), bias=True),                                              # a boundary on a tile's edge
    Case("1024-512", 1024, 512, (7, 8), bias=True),                                              # N = 15
    Case("256-9", 256, 9, (1,), offsets=False, bias=True),                                       # N = 1
    Case("256-4096", 256, 4096, (2,), offsets=False, bias=True),                                 # N = 2
    Case("64-64-per-segment", 64, 64, (64, 65), per_segment=True),                               # N = 129
]


def test_the_table_covers_what_the_contract_names():
    assert {c.N for c in CASES} >= {1, 15, 17, 127, 129, 1000}
    assert {len(c.counts) for c in CASES} == {1, 2, 3}
    assert {(c.affine, c.relu) for c in CASES} == {(False, False), (True, False), (False, True), (True, True)}
    assert {(c.cin, c.cout) for c in CASES} >= {(6, 64), (64, 128), (128, 1024), (64, 512), (512, 256), (256, 16), (1024, 512),
                                                (256, 9), (256, 4096), (64, 64)}


def make(case, cuda):
    rng = np.random.default_rng(sum(map(ord, case.id)))
    S, N = len(case.counts), case.N
    host = [0] + list(np.cumsum(case.counts))
    d = {"host": [int(v) for v in host], "S": S}
    if case.view is not None:
        n = case.counts[0]
        flat = rng.standard_normal(S * n * case.cin).astype(np.float32)
        strides = (case.cin * n, n, 1) if case.view == "reference" else (case.cin * n, 1, case.cin)
        d["x_arg"], d["strides"], d["X"] = flat, strides, R.view_rows(flat, S, n, case.cin, strides)
    else:
        d["X"] = rng.standard_normal((N, case.cin)).astype(np.float32)
        d["x_arg"], d["strides"] = d["X"], None
    wshape = (S, case.cout, case.cin) if case.per_segment else (case.cout, case.cin)
    d["W"] = (rng.standard_normal(wshape) / np.sqrt(case.cin)).astype(np.float32)
    d["b"] = rng.standard_normal(case.cout).astype(np.float32) if case.bias else None
    d["G"] = rng.standard_normal((S, case.cout)).astype(np.float32) if case.G else None
    d["scale"] = rng.uniform(-1.5, 1.5, case.cout).astype(np.float32) if case.affine else None
    d["shift"] = rng.standard_normal(case.cout).astype(np.float32) if case.affine else None
    d["dY"] = rng.standard_normal((N, case.cout)).astype(np.float32)
    t = lambda a: None if a is None else torch.from_numpy(a).to(cuda)
    d["t"] = {k: t(d[k]) for k in ("x_arg", "W", "b", "G", "scale", "shift", "dY")}
    d["off"] = torch.tensor(d["host"], dtype=torch.int64, device=cuda) if case.offsets else None
    return d


def run_fwd(ops, case, d, want_y=True, want_max=True):
    t = d["t"]
    return ops.pointmlp_fwd(t["x_arg"], t["W"], t["b"], t["G"], t["scale"], t["shift"], case.relu, offsets=d["off"],
                            offsets_host=d["host"] if case.offsets else ([0, case.N] if case.view else None), view=d["strides"],
                            want_y=want_y, want_max=want_max)


def within(got, ref, A, n, what):
    err = np.abs(got.astype(np.float64) - ref)
    bound = R.gamma(n) * A
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max err {err.max():.3e}, worst err / bound {worst:.3f} (n = {n})")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case(cuda, case):
    from gapartnet_amd import _C, hip_ops as ops
    from gapartnet_amd._C import i32, i64, ptr
    d = make(case, cuda)
    if case.view is not None and not case.offsets:
        pytest.fail("a strided view needs offsets")
    kw = dict(b=d["b"], G=d["G"], offsets=d["host"], scale=d["scale"], shift=d["shift"])
    Yr, Mr = R.dense(d["X"], d["W"], relu=case.relu, **kw)
    Ya, _ = R.dense(d["X"], d["W"], absolute=True, **kw)
    Ma = np.stack([Ya[a:b].max(0) for a, b in zip(d["host"][:-1], d["host"][1:])])
    n = case.cin + 4

    # forward: stored form, run twice; max-only form
    Y, M = run_fwd(ops, case, d)
    Y2, M2 = run_fwd(ops, case, d)
    none, M3 = run_fwd(ops, case, d, want_y=False)
    assert Y.shape == (case.N, case.cout) and M.shape == (d["S"], case.cout) and none is None
    within(Y.cpu().numpy(), Yr, Ya, n, "Y")
    within(M.cpu().numpy(), Mr, Ma, n, "M")
    assert torch.equal(Y, Y2) and torch.equal(M, M2), "two runs differ"
    assert torch.equal(M3, M), "the max-only form differs from the stored form's maxima"
    begin = d["host"][:-1]
    stored_max = torch.stack([Y[a:b].max(0)[0] for a, b in zip(begin, d["host"][1:])])
    assert torch.equal(M.view(torch.int32), stored_max.view(torch.int32)) or torch.equal(M, stored_max)

    # sentinel: nothing past N x cout / S x cout is written
    t, pad = d["t"], 4096
    Yb = torch.full((case.N * case.cout + pad,), 12345.0, device=cuda)
    Mb = torch.full((d["S"] * case.cout + pad,), 12345.0, device=cuda)
    strided = d["strides"] is not None
    sb, sc, sn = d["strides"] if strided else (0, 0, 0)
    host = (_C.ctypes.c_int64 * len(d["host"]))(*d["host"])
    _C.check(_C.lib().gpn_pointmlp_fwd(ptr(t["x_arg"]), i32(strided), i64(sb), i64(sc), i64(sn), ptr(t["W"]), i32(case.per_segment),
                                       ptr(t["b"]), ptr(t["G"]), ptr(t["scale"]), ptr(t["shift"]), i32(case.relu), ptr(d["off"]),
                                       host if case.offsets else None, i64(d["S"]), i64(case.N), i32(case.cin), i32(case.cout),
                                       ptr(Yb), ptr(Mb), ops._stream()), "gpn_pointmlp_fwd")
    assert torch.equal(Yb[:case.N * case.cout].view(case.N, case.cout), Y) and bool((Yb[case.N * case.cout:] == 12345.0).all())
    assert torch.equal(Mb[:d["S"] * case.cout].view(d["S"], case.cout), M) and bool((Mb[d["S"] * case.cout:] == 12345.0).all())

    # dgrad: the same kernel on transposed weights
    Wt = np.ascontiguousarray(np.swapaxes(d["W"], -1, -2))
    dX, _ = ops.pointmlp_fwd(t["dY"], torch.from_numpy(Wt).to(cuda), offsets=d["off"], offsets_host=d["host"] if case.offsets else None)
    dXr, _ = R.dense(d["dY"], Wt, offsets=d["host"])
    dXa, _ = R.dense(d["dY"], Wt, offsets=d["host"], absolute=True)
    within(dX.cpu().numpy(), dXr, dXa, case.cout + 4, "dX")

    # wgrad, twice
    wkw = dict(offsets=d["off"], offsets_host=d["host"] if (case.offsets or strided) else None, view=d["strides"],
               per_segment=case.per_segment, need_dw=True, need_db=True)
    if strided and not case.offsets:
        wkw["offsets_host"] = [0, case.N]
    dW, db = ops.pointmlp_wgrad(t["x_arg"], t["dY"], case.cin, **wkw)
    dW = dW.clone()  # (the workspace is reused; the outputs are not, but keep the first run's values apart anyway)
    dW2, db2 = ops.pointmlp_wgrad(t["x_arg"], t["dY"], case.cin, **wkw)
    dWr, dbr = R.wgrad(d["X"], d["dY"], d["host"], case.per_segment)
    dWa, dba = R.wgrad(d["X"], d["dY"], d["host"], case.per_segment, absolute=True)
    within(dW.cpu().numpy(), dWr, dWa, case.N + 4, "dW")
    within(db.cpu().numpy(), dbr, dba, case.N + 4, "db")
    assert torch.equal(dW, dW2) and torch.equal(db, db2), "two wgrad runs differ"
