"""CPU checks behind the conv instantiation sweep (tests/test_gpu_conv_shapes.py): the float64 reference of tests/conv_ref64.py
pinned against torch's dense conv3d / conv_transpose3d, the profiler kernel-name parser, a coverage check - every
instantiation the conv sources build (the instantiation lists and constants of csrc/spconv_dispatch.h, which every dispatch
expands) is launched by some case of the GPU module's table, or listed in UNREACHABLE with the reason the dispatch cannot produce
it - and the library's routing decision (gpn_spconv_fwd_route) against the GPU module's restatement of it.

The DEV (device-counted rows) and EP (an inference pass's BatchNorm in the epilogue) variants are outside this sweep; they run
through the network executor in tests/test_gpu_model.py::test_inference_pass_applies_batchnorm_in_the_conv_epilogue,
tests/test_gpu_proposals.py::test_validation_step_with_batchnorm_in_the_conv_epilogues_equals_batchnorm_launches and
tests/test_gpu_proposals.py::test_validation_step_without_a_host_read_equals_the_blocking_step."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as O
from tests import conv_ref64 as R64
from tests import synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gapartnet_amd", "csrc")

# instantiations the sources build that no dispatch path can launch: {(family, args): reason}
UNREACHABLE = {}


# ---------------------------------------------------------------------------------------------------- float64 reference pins
def _dense(idx, feats, batch, shape):
    d = torch.zeros(batch, feats.shape[1], *shape, dtype=torch.float64)
    i = torch.from_numpy(idx).long()
    d[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = torch.from_numpy(feats).double()
    return d, i


@pytest.mark.parametrize("cin,cout", [(16, 32), (48, 16)])
def test_ref64_subm_vs_dense_conv3d(cin, cout):
    rng = np.random.default_rng(cin + cout)
    shape, batch = [9, 11, 10], 2
    idx = synth.random_sparse_indices(rng, batch, shape, 500)
    N = idx.shape[0]
    f, g = rng.normal(size=(N, cin)), rng.normal(size=(N, cout))
    W = rng.normal(size=(27, cin, cout))
    pairs = O.rulebook_subm3(idx, shape)
    dense, i = _dense(idx, f, batch, shape)
    dense.requires_grad_(True)
    wt = torch.from_numpy(W).reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous().requires_grad_(True)
    ref = F.conv3d(dense, wt, padding=1)[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]]
    ref.backward(torch.from_numpy(g))
    assert np.allclose(R64.fwd(f, W, pairs, N), ref.detach().numpy(), rtol=1e-12, atol=1e-10)
    assert np.allclose(R64.dgrad(g, W, pairs, N), dense.grad[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]].numpy(), rtol=1e-12, atol=1e-10)
    dW = wt.grad.permute(2, 3, 4, 1, 0).reshape(27, cin, cout).numpy()
    assert np.allclose(R64.wgrad(f, g, pairs), dW, rtol=1e-12, atol=1e-9)
    # the sampled-row form over the neighbour table the pair lists describe
    nbr = np.full((27, N), -1, np.int64)
    for k, (s, d) in enumerate(R64.tap_pairs(pairs)):
        nbr[k, d] = s
    rows = R64.sample_rows(rng, N, 50)
    assert np.allclose(R64.fwd_rows(f, W, nbr[:, rows], rows), ref.detach().numpy()[rows], rtol=1e-12, atol=1e-10)


def test_ref64_down_and_inverse_vs_dense():
    rng = np.random.default_rng(5)
    shape, batch, cin, cout = [10, 12, 8], 2, 16, 32
    idx = synth.random_sparse_indices(rng, batch, shape, 600)
    N = idx.shape[0]
    f = rng.normal(size=(N, cin))
    W = rng.normal(size=(8, cin, cout))
    d = O.rulebook_down(idx, shape)
    No = d["out_indices"].shape[0]
    dense, _ = _dense(idx, f, batch, shape)
    wt = torch.from_numpy(W).reshape(2, 2, 2, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
    oi = torch.from_numpy(d["out_indices"]).long()
    ref = F.conv3d(dense, wt, stride=2)[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]].numpy()
    out = R64.fwd(f, W, d["fwd"], No)
    assert np.allclose(out, ref, rtol=1e-12, atol=1e-10)
    # inverse conv = conv_transpose3d restricted to the fine rows; equals the dgrad of the down conv with the same weight
    Wi = rng.normal(size=(8, cout, cin))
    up = R64.fwd(out, Wi, d["bwd"], N)
    dense_c = torch.zeros(batch, cout, *d["out_shape"], dtype=torch.float64)
    dense_c[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]] = torch.from_numpy(out)
    wti = torch.from_numpy(Wi).reshape(2, 2, 2, cout, cin).permute(3, 4, 0, 1, 2).contiguous()
    ref_up = F.conv_transpose3d(dense_c, wti, stride=2)[:, :, : shape[0], : shape[1], : shape[2]]
    i = torch.from_numpy(idx).long()
    assert np.allclose(up, ref_up[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]].numpy(), rtol=1e-12, atol=1e-10)
    Wd = np.ascontiguousarray(Wi.transpose(0, 2, 1))  # [8, cin, cout]
    assert np.allclose(R64.dgrad(out, Wd, d["fwd"], N), up, rtol=1e-12, atol=1e-10)


# ---------------------------------------------------------------------------------------------------- kernel names
@pytest.mark.parametrize("name,want", [
    ("void (anonymous namespace)::spconv_msplit_kernel<14, 4, 4, false, false>(float const*, float const*, int const*)",
     ("msplit", (14, 4, 4, False, False))),
    ("_ZN12_GLOBAL__N_120spconv_msplit_kernelILi14ELi4ELi4ELb0ELb0EEEvPKfS2_PKiS4_iliiiimiN3gpn9ConvStatsEPfPKl",
     ("msplit", (14, 4, 4, False, False))),
    ("void (anonymous namespace)::spconv_tiles_kernel<7, 7, 1, false, true>(float const*)", ("tiles", (7, 7, 1, False, True))),
    ("_ZN12_GLOBAL__N_119spconv_tiles_kernelILi12ELi7ELi1ELb1ELb0EEEvPKf", ("tiles", (12, 7, 1, True, False))),
    ("void (anonymous namespace)::spconv_fwd_direct_kernel<27, 10, false, false>(float const*)", ("direct", (27, 10, False, False))),
    ("_ZN12_GLOBAL__N_124spconv_fwd_direct_kernelILi8ELi3ELb0ELb0EEEvPKf", ("direct", (8, 3, False, False))),
    ("void (anonymous namespace)::spconv_fwd_split_kernel<8, 2, 4, false>(float const*)", ("split", (8, 2, 4, False))),
    ("_ZN12_GLOBAL__N_123spconv_fwd_split_kernelILi27ELi12ELi2ELb0EEEvPKf", ("split", (27, 12, 2, False))),
    ("void (anonymous namespace)::spconv_fwd_kernel<3, 4, 2>(float const*, float const*)", ("lockstep", (3, 4, 2))),
    ("_ZN12_GLOBAL__N_117spconv_fwd_kernelILi4ELi2ELi1EEEvPKfS2_PKiilii", ("lockstep", (4, 2, 1))),
    ("(anonymous namespace)::reduce_partials_kernel(float const*, int, long, int, float*)", ("reduce", ())),
    ("_ZN12_GLOBAL__N_122reduce_partials_kernelEPKfilPf", ("reduce", ())),
    ("void (anonymous namespace)::spconv_wgrad_lds_kernel<4, 8>(gpn::WgradSets, long, int)", ("wgrad", (4, 8))),
    ("_ZN12_GLOBAL__N_123spconv_wgrad_lds_kernelILi1ELi3EEEvN3gpn9WgradSetsElii", ("wgrad", (1, 3))),
    ("(anonymous namespace)::wgrad_reduce_many_kernel((anonymous namespace)::ReduceBatch)", None),
    ("void (anonymous namespace)::pack_weights_kernel(float const*, int, int, int, int, float*)", None),
    ("_ZN12_GLOBAL__N_125my_spconv_fwd_kernelILi1ELi1ELi1EEEvPKf", None),
])
def test_kernel_name_parser(name, want):
    assert R64.kernel_id(name) == want


# ---------------------------------------------------------------------------------------------------- coverage
def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return re.sub(r"//[^\n]*", "", fh.read())  # (comments dropped: they mention kernels and cases in prose)


def _ints(pattern, text):
    vals = sorted({int(v) for v in re.findall(pattern, text)})
    assert vals, f"nothing parsed by {pattern!r}: the source changed shape, update the parser"
    return vals


def _width_list(src, macro):
    m = re.search(r"#define " + macro + r"\(X\)((?:\s*X\(\d+\))+)", src)
    assert m, f"no {macro} list"
    return _ints(r"X\((\d+)\)", m.group(1))


def _const(src, name):
    m = re.search(r"constexpr int " + name + r" = (\d+);", src)
    assert m, f"no constant {name}"
    return int(m.group(1))


def parsed_instantiations():
    """{(family, args)} the conv sources instantiate (DEV / EP = false): every dispatch of csrc/ is an expansion of a
    ``#define NAME(X) X(..) X(..)`` list of csrc/spconv_dispatch.h, so the lists and its named constants are all that is read"""
    src = _src("spconv_dispatch.h")
    owners = {"GPN_CONV_CB": ("spconv_tiles.hip", "spconv_msplit.hip"), "GPN_TILES_NT": ("spconv_tiles.hip",),
              "GPN_MSPLIT_NT": ("spconv_msplit.hip",), "GPN_MSPLIT_SP": ("spconv_msplit.hip",), "GPN_DIRECT_KT": ("spconv_fwd.hip",),
              "GPN_DIRECT_CB": ("spconv_fwd.hip",), "GPN_SPLIT_WAYS": ("spconv_fwd.hip",), "GPN_LOCKSTEP_NTW": ("spconv_fwd.hip",),
              "GPN_LOCKSTEP_CW": ("spconv_fwd.hip",), "GPN_LOCKSTEP_WAVES": ("spconv_fwd.hip",), "GPN_WGRAD_CT": ("spconv.hip",),
              "GPN_WGRAD_NT": ("spconv.hip",)}

    def lst(macro):  # (a list counts only if the dispatch of the file that owns the kernel expands it)
        for fn in owners[macro]:
            assert macro + "(GPN_X)" in _src(fn), f"{fn} does not expand {macro}"
        return _width_list(src, macro)

    out = set()
    # masked-tile: input widths x column tiles per wave, R row tiles per wave
    out.update(("tiles", (cb, nt, _const(src, "kTilesR"), False, False)) for cb in lst("GPN_CONV_CB") for nt in lst("GPN_TILES_NT"))
    # masked tap-split: input widths x column tiles per workgroup x waves per row tile (nine where the ring fits)
    fit9 = _const(src, "kMsplitSp9MaxRegs4")
    out.update(("msplit", (cb, nt, sp, False, False)) for cb in lst("GPN_CONV_CB") for nt in lst("GPN_MSPLIT_NT")
               for sp in lst("GPN_MSPLIT_SP") if sp != 9 or cb * (1 + nt) <= fit9)
    # direct kernel and its tap-split forms (layers of at least kSplitMinTaps taps)
    for kt in lst("GPN_DIRECT_KT"):
        for cb in lst("GPN_DIRECT_CB"):
            out.add(("direct", (kt, cb, False, False)))
            if kt >= _const(src, "kSplitMinTaps"):
                out.update(("split", (kt, cb, w, False)) for w in lst("GPN_SPLIT_WAYS"))
    # lock-step: NS = ceil(CW NTW / waves per workgroup); its tap splits are summed by the reduce kernel
    out.update(("lockstep", (ntw, cw, -(-(cw * ntw) // w))) for ntw in lst("GPN_LOCKSTEP_NTW") for cw in lst("GPN_LOCKSTEP_CW")
               for w in lst("GPN_LOCKSTEP_WAVES"))
    if "reduce_partials_kernel" in _src("spconv_fwd.hip"):
        out.add(("reduce", ()))
    out.update(("wgrad", (ct, nt)) for ct in lst("GPN_WGRAD_CT") for nt in lst("GPN_WGRAD_NT"))
    return out


def test_every_conv_instantiation_has_a_case():
    from tests import test_gpu_conv_shapes as T
    built = parsed_instantiations()
    for fam in ("tiles", "msplit", "direct", "split", "lockstep", "reduce", "wgrad"):
        assert any(f == fam for f, _ in built), f"parsed no {fam} instantiation"
    covered = T.expected_instantiations()
    missing = sorted((k for k in built - covered if k not in UNREACHABLE), key=str)
    assert not missing, f"instantiations no case of tests/test_gpu_conv_shapes.py launches: {missing}"
    stale = sorted((k for k in UNREACHABLE if k not in built or k in covered), key=str)
    assert not stale, f"UNREACHABLE entries that are not built or are covered: {stale}"
    phantom = sorted(covered - built, key=str)
    assert not phantom, f"the case table expects instantiations the sources do not build: {phantom}"


def test_case_table_is_well_formed():
    from tests import test_gpu_conv_shapes as T
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
    for c in T.CASES:
        assert c.cin % 16 == 0 and c.cout % 16 == 0 and c.n >= 1 and c.routes
        # wide-channel cases stay small (the float64 reference runs on the host)
        if c.K == 27 and not c.large:
            assert c.n * c.cin * c.cout <= 50e6, c.id
    for cout in (16, 128, 144, 256, 496):
        assert sum(T.wgrad_chunks(cout)) == cout and max(T.wgrad_chunks(cout)) <= 128
    n_max = next(c.n for c in T.CASES if c.id == "guard-below")
    assert n_max * 8 * 16 * 4 < 2 ** 31 <= (n_max + 1) * 8 * 16 * 4
    assert T.route(27, n_max, 16, 16)[0][0] == "tiles" and T.route(27, n_max + 1, 16, 16)[0][0] == "lockstep"
    assert math.isclose(n_max, 4194303)


# ---------------------------------------------------------------------------------------------------- routing
KIND = {"tiles": 1, "msplit": 2, "direct": 3, "split": 3, "lockstep": 4}
UNROUTABLE = 5


def _flags(kind, K):
    """the rule of gpn::ConvRoute: which kinds have BatchNorm sums / an inference BatchNorm in their epilogue"""
    return kind | (kind in (1, 2, 3)) << 8 | (kind in (1, 2) or (kind == 3 and K == 1)) << 9


def test_library_route_equals_the_restated_route():
    """gpn_spconv_fwd_route (what spconv_fwd_into launches by and the executor plans by) against the independent restatement of
    tests/test_gpu_conv_shapes.py, at and either side of every threshold and under every knob setting of the case table; the
    device-counted rule (a kernel must fit at the bound AND, for the masked-tile kernel, at the plan) restated here."""
    import ctypes
    from gapartnet_amd import _C
    from tests import test_gpu_conv_shapes as T
    if not os.path.exists(_C.SO_PATH):
        _C.build()
    L = _C.lib()
    L.gpn_spconv_fwd_route.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    L.gpn_spconv_fwd_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    n_guard = next(c.n for c in T.CASES if c.id == "guard-below")
    knobs = (T.DEFAULT, T.LOW, T.NO_TILES, T.MS_OFF, T._direct(1), T._direct(2), T._direct(4), T.Knobs(ms=(0, 0, 0)))

    def tiles_ok(K, n, cin, cout, kn):
        return 1 <= K <= 27 and T._fits32(K, n, cin, cout) and T.cdiv(n, 16) >= max(kn.min_tiles, 16) and cin // 16 in T.TILES_CB

    def route_dev(K, bound, plan, cin, cout, kn):
        p = min(plan, bound) if plan > 0 else bound
        fits = T._fits32(K, bound, cin, cout)
        if tiles_ok(K, bound, cin, cout, kn) and tiles_ok(K, p, cin, cout, kn):
            return 1
        if kn.ms[0] and K in (27, 8) and fits and cin // 16 in T.MSPLIT_CB:
            return 2
        if K in (27, 8, 1) and cin // 16 in T.DIRECT_CB and T._fits32(K, max(bound, 256), cin, cout):
            return 3  # (max(bound, 256) rows are 16 row tiles: the direct kernel's size floor never refuses)
        return UNROUTABLE

    try:
        for kn in knobs:
            T._knobs(L, kn)
            for K in (1, 2, 8, 27):
                for cb in range(1, 17):
                    for cout in (16, 64, 224, 256):
                        cin = 16 * cb
                        n_fit = (1 << 31) // (8 * max(cin, cout) * 4)  # the first row count past the 32-bit offsets
                        for n in (1, 15, 240, 255, 256, 257, 16 * 4095, 16 * 4096 - 1, 16 * 4096, 16 * 4096 + 1, n_fit - 1, n_fit, n_guard,
                                  n_guard + 1):
                            fam = T.route(K, n, cin, cout, kn)[0][0]
                            got = L.gpn_spconv_fwd_route(K, n, -1, cin, cout)
                            assert got == _flags(KIND[fam], K), (kn, K, n, cin, cout, fam, got)
                            if tiles_ok(K, n, cin, cout, kn):
                                assert fam == "tiles"
                            ws = L.gpn_spconv_fwd_ws_bytes(K, n, cin, cout)
                            splits = T.plan_fwd(K, n, cin, cout)[3]
                            want = -(-splits * n * cout * 4 // 256) * 256 if fam == "lockstep" and splits > 1 else 0
                            assert ws == want, (kn, K, n, cin, cout, fam, ws, want)
                        # device-counted rows: bounds and plans on both sides of the 16-tile and the 4096-tile threshold
                        for bound in (200, 257, 16 * 4096 - 1, 16 * 4096 + 1, n_fit) if cout in (16, 256) else ():
                            for plan in (0, 240, 255, 257, 16 * 4095, 16 * 4096 - 1, 16 * 4096 + 1, bound + 5):
                                want = route_dev(K, bound, plan, cin, cout, kn)
                                got = L.gpn_spconv_fwd_route(K, bound, plan, cin, cout)
                                assert got == _flags(want, K), (kn, K, bound, plan, cin, cout, want, got)
            assert L.gpn_spconv_fwd_route(27, 0, -1, 16, 16) == 0 and L.gpn_spconv_fwd_route(27, 0, 0, 16, 16) == 0
        # a bound above the masked-tile kernel's size and a plan below it must not take that kernel
        for kn, bound, plan, want in ((T.DEFAULT, 70000, 60000, 2), (T.Knobs(ms=(0, 0, 0)), 70000, 60000, 3), (T.LOW, 300, 200, 2),
                                      (T.DEFAULT, 70000, 70000, 1), (T.DEFAULT, 70000, 0, 1), (T.LOW, 300, 260, 1)):
            T._knobs(L, kn)
            assert L.gpn_spconv_fwd_route(27, bound, plan, 32, 32) & 0xff == want, (kn, bound, plan)
    finally:
        T._knobs(L, T.DEFAULT)
