"""CPU checks behind the conv instantiation sweep (tests/test_gpu_conv_shapes.py): the float64 reference of tests/conv_ref64.py
pinned against torch's dense conv3d / conv_transpose3d, the profiler kernel-name parser, and a coverage check - every
instantiation the conv sources build (parsed from their width lists and dispatch switches) is launched by some case of the GPU
module's table, or listed in UNREACHABLE with the reason the dispatch cannot produce it.

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


def _body(src, head):
    """the brace-balanced body of the first function whose text starts with the regex ``head``"""
    m = re.search(head, src)
    assert m, f"no {head!r} in the source"
    i = src.index("{", m.end())
    depth = 0
    for j in range(i, len(src)):
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
    raise AssertionError(f"unbalanced body of {head!r}")


def _ints(pattern, text):
    vals = sorted({int(v) for v in re.findall(pattern, text)})
    assert vals, f"nothing parsed by {pattern!r}: the source changed shape, update the parser"
    return vals


def _width_list(src, macro):
    m = re.search(r"#define " + macro + r"\(X\)((?:\s*X\(\d+\))+)", src)
    assert m, f"no {macro} list"
    return _ints(r"X\((\d+)\)", m.group(1))


def parsed_instantiations():
    """{(family, args)} the conv sources instantiate (DEV / EP = false)"""
    out = set()
    # masked-tile: GPN_TILES_CB x the column-tile counts of dispatch_cols, R of launch_tiles
    src = _src("spconv_tiles.hip")
    R = _ints(r"constexpr int R = (\d+);", _body(src, r"int launch_tiles\("))
    for cb in _width_list(src, "GPN_TILES_CB"):
        for nt in _ints(r"launch_tiles<CB, (\d+)>", _body(src, r"int dispatch_cols\(")):
            out.update(("tiles", (cb, nt, r, False, False)) for r in R)
    # masked tap-split: GPN_MSPLIT_CB x dispatch_nt's NT x dispatch_sp's SP (SP 9 where ms_fits9)
    src = _src("spconv_msplit.hip")
    fit = re.search(r"ms_fits9\(int CB, int NT\) \{ return CB \* \(1 \+ NT\) <= (\d+); \}", src)
    assert fit, "ms_fits9 changed shape"
    sps = _ints(r"launch_msplit<CB, NT, (\d+)>", _body(src, r"int dispatch_sp\("))
    for cb in _width_list(src, "GPN_MSPLIT_CB"):
        for nt in _ints(r"dispatch_sp<CB, (\d+)>", _body(src, r"int dispatch_nt\(")):
            for sp in sps:
                if sp != 9 or cb * (1 + nt) <= int(fit.group(1)):
                    out.add(("msplit", (cb, nt, sp, False, False)))
    # direct kernel (KT from spconv_fwd_into's dispatch_direct<KT>, CB from dispatch_direct) and its tap-split forms (KT >= 8)
    src = _src("spconv_fwd.hip")
    fwd_into = _body(src, r"int gpn::spconv_fwd_into\(")
    kts = _ints(r"dispatch_direct<(\d+)>", fwd_into)
    cbs = _ints(r"launch_direct<KT, (\d+)>", _body(src, r"int dispatch_direct\("))
    ld = _body(src, r"int launch_direct\(")
    split_from = int(re.search(r"if constexpr \(KT >= (\d+)\)", ld).group(1))
    ways = _ints(r"launch_split<KT, CB, (\d+)>", ld)
    for kt in kts:
        for cb in cbs:
            out.add(("direct", (kt, cb, False, False)))
            if kt >= split_from:
                out.update(("split", (kt, cb, w, False)) for w in ways)
    # lock-step: NTW from spconv_fwd_into's switch, CW from dispatch_cw, NS = ceil(CW NTW / waves) for dispatch_ns's wave counts
    ntws = _ints(r"dispatch_cw<(\d+)>", fwd_into)
    cws = _ints(r"dispatch_ns<NTW, (\d+)>", _body(src, r"int dispatch_cw\("))
    waves = _ints(r"\(X \+ \d+\) / (\d+)", _body(src, r"int dispatch_ns\("))
    for ntw in ntws:
        for cw in cws:
            out.update(("lockstep", (ntw, cw, -(-(cw * ntw) // w))) for w in waves)
    if "reduce_partials_kernel" in fwd_into:
        out.add(("reduce", ()))
    # weight gradient: wgrad_contract's CT switch x dispatch_wgrad_nt's cases
    src = _src("spconv.hip")
    cts = _ints(r"dispatch_wgrad_nt<(\d+)>", _body(src, r"int wgrad_contract\("))
    nts = _ints(r"GPN_CASE\((\d+)\)", _body(src, r"int dispatch_wgrad_nt\("))
    out.update(("wgrad", (ct, nt)) for ct in cts for nt in nts)
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
