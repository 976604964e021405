"""CPU checks of the bf16 inference path (include/gpn.h section C16): the numpy rounding reference against torch's, the new entry
points' export / registration / argument checking without a device, the workspace of a bf16 pass derived from the shapes, the
coverage of the GPU case table (tests/test_gpu_conv_bf16.py) over the instantiations csrc/spconv_bf16.hip builds, and the knob's
validation."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import bf16_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gapartnet_amd", "csrc")
NEW_SYMBOLS = ("gpn_spconv_pack_weights_bf16", "gpn_spconv_fwd_bf16", "gpn_rows_to_bf16", "gpn_bn_act_bf16",
               "gpn_net_forward_bf16_ws_bytes", "gpn_net_forward_bf16")


@pytest.fixture(scope="module")
def lib():
    from gapartnet_amd import _C
    if not os.path.exists(_C.SO_PATH):
        _C.build()
    L = _C.lib()
    L.gpn_last_error.restype = ctypes.c_char_p
    return L


# ---------------------------------------------------------------------------------------------------- (a) rounding
def _torch_bits(x):
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_numpy_rounding_equals_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.normal(size=200000).astype(np.float32),
        (rng.normal(size=50000) * 10.0 ** rng.uniform(-30, 30, size=50000)).astype(np.float32),
        rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32),  # every kind of bit pattern
    ])
    finite = ~np.isnan(x)
    assert np.array_equal(B.bf16_bits(x)[finite], _torch_bits(x)[finite])
    assert np.all(np.isnan(B.widen(B.bf16_bits(x)[~finite])))


def test_numpy_rounding_ties_and_specials():
    one = np.float32(1.0)
    ties = np.array([one + np.float32(2.0 ** -8), one + np.float32(3 * 2.0 ** -8), -(one + np.float32(2.0 ** -8)),
                     -(one + np.float32(3 * 2.0 ** -8))], np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6)], np.float32)
    assert np.array_equal(B.round_bf16(ties), want)               # ties go to the even mantissa, in both directions
    assert np.array_equal(B.bf16_bits(ties), _torch_bits(ties))
    near = np.array([one + np.float32(2.0 ** -8) + np.float32(2.0 ** -23), one + np.float32(2.0 ** -8) - np.float32(2.0 ** -23)], np.float32)
    assert np.array_equal(B.round_bf16(near), np.array([1.0 + 2.0 ** -7, 1.0], np.float32))
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 1.1754942e-38, 3.4028235e38], np.float32)
    assert np.array_equal(B.bf16_bits(special), _torch_bits(special))
    assert B.bf16_bits(np.array([-0.0], np.float32))[0] == 0x8000 and B.bf16_bits(np.array([0.0], np.float32))[0] == 0
    nan = np.array([np.nan, -np.nan], np.float32)
    nan_bits = np.array([0x7F800001, 0xFF800001, 0x7FFFFFFF], np.uint32).view(np.float32)  # signalling / all-ones payloads
    assert np.all(np.isnan(B.round_bf16(nan))) and np.all(np.isnan(B.round_bf16(nan_bits)))
    assert np.all(np.isnan(torch.from_numpy(nan_bits).to(torch.bfloat16).float().numpy()))


# ---------------------------------------------------------------------------------------------------- (b) the C ABI without a device
def test_new_entry_points_are_exported_and_registered(lib):
    names = {lib.gpn_entry_point_name(i).decode() for i in range(lib.gpn_num_entry_points())}
    header = open(os.path.join(ROOT, "include", "gpn.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in names, s
        assert re.search(r"\b" + s + r"\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), s


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


FAKE = 0x1000  # a non-null pointer no call below may dereference


def test_conv_rejects_bad_arguments_without_a_device(lib):
    p = ctypes.c_void_p(FAKE)

    def fwd(K=27, n=100, cin=32, cout=32, nbr_p=None, perm=None):
        return lib.gpn_spconv_fwd_bf16(p, p, p, nbr_p, perm, ctypes.c_int(K), ctypes.c_int64(n), ctypes.c_int(cin), ctypes.c_int(cout),
                                       None, p, None)

    assert fwd(cin=24) == 1 and b"multiples of 16" in lib.gpn_last_error() and b"cin = 24" in lib.gpn_last_error()
    assert fwd(cout=40) == 1 and b"multiples of 16" in lib.gpn_last_error()
    assert fwd(cin=144) == 1 and b"no bf16 kernel for 144 input channels" in lib.gpn_last_error()
    assert fwd(K=28) == 1 and b"1 <= K <= 27" in lib.gpn_last_error()
    assert fwd(K=0) == 1
    assert fwd(nbr_p=p) == 1 and b"bad argument" in lib.gpn_last_error()  # a tile order needs nbr_p and perm
    # the 32-bit byte-offset guard: 8 n_dst * 2 max(cin, cout) < 2^31
    n_max = (1 << 31) // (8 * 2 * 32) - 1
    assert fwd(n=n_max + 1) == 1 and b"32-bit byte offsets" in lib.gpn_last_error()
    assert fwd(n=0) == 0  # nothing to do, nothing launched
    rc = lib.gpn_spconv_pack_weights_bf16(p, 27, 32, 32, 1, p, None)  # GPN_PACK_TRANSPOSE is not a bf16 flag
    assert rc == 1 and b"bad argument" in lib.gpn_last_error()
    assert lib.gpn_spconv_pack_weights_bf16(None, 27, 32, 32, 0, p, None) == 1
    assert lib.gpn_rows_to_bf16(None, ctypes.c_int64(4), 16, p, None) == 1
    assert lib.gpn_bn_act_bf16(p, 1, None, None, p, p, p, ctypes.c_float(1e-4), ctypes.c_int64(4), 16, 1, p, None) == 1


def _tiny_program():
    """slot 0 -BN+ReLU-> 1 -conv-> 2 -BN+ReLU-> 3: 100 rows of 16 channels; pointers are fakes that must never be dereferenced"""
    from gapartnet_amd.network import net_exec as NX
    slots = np.zeros(4, NX.SLOT_DT)
    slots["rows"], slots["channels"] = 100, 16
    slots["data"][0] = slots["data"][3] = FAKE
    rbs = np.zeros(1, NX.RB_DT)
    rbs["n_src"], rbs["n_dst"], rbs["K"], rbs["nbr"] = 100, 100, 27, FAKE
    convs = np.zeros(1, NX.CONV_DT)
    convs["cin"], convs["cout"], convs["W"] = 16, 16, FAKE
    bns = np.zeros(2, NX.BN_DT)
    for f in ("weight", "bias", "running_mean", "running_var"):
        bns[f] = FAKE
    bns["C"], bns["eps"] = 16, 1e-4
    ops = np.zeros(3, NX.OP_DT)
    ops[0] = (NX.OP_BN, 0, -1, 1, -1, 0, NX.FLAG_RELU, 0)
    ops[1] = (NX.OP_CONV, 1, -1, 2, 0, 0, 0, 0)
    ops[2] = (NX.OP_BN, 2, -1, 3, -1, 1, NX.FLAG_RELU, 0)
    return ops, slots, rbs, convs, bns


def _net_bf16(lib, ops, slots, rbs, convs, bns, ws=FAKE, ws_bytes=1 << 30):
    return lib.gpn_net_forward_bf16(_vp(ops), len(ops), _vp(slots), len(slots), _vp(rbs), len(rbs), _vp(convs), len(convs), _vp(bns),
                                    len(bns), ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)


def test_net_forward_bf16_validates_before_the_first_launch(lib):
    lib.gpn_net_forward_bf16_ws_bytes.restype = ctypes.c_size_t
    ops, slots, rbs, convs, bns = _tiny_program()
    need = lib.gpn_net_forward_bf16_ws_bytes(_vp(ops), len(ops), _vp(slots), len(slots), _vp(rbs), _vp(convs))
    # the packed weight and ONE bf16 buffer (slot 1: slot 2 rides in the conv launch, slot 3 is the fp32 output, slot 0 is read as fp32)
    assert need == 27 * 16 * 16 * 2 + 100 * 16 * 2 + (256 - (100 * 16 * 2) % 256) % 256
    assert _net_bf16(lib, ops, slots, rbs, convs, bns, ws_bytes=need - 1) == 2 and b"workspace too small" in lib.gpn_last_error()
    assert _net_bf16(lib, ops, slots, rbs, convs, bns, ws=0) == 2
    counter = np.zeros(1, np.int64)
    s = slots.copy()
    s["rows_dev"][2] = counter.ctypes.data
    assert _net_bf16(lib, ops, s, rbs, convs, bns) == 1 and b"rows_dev" in lib.gpn_last_error()
    for field in ("weight", "bias", "running_mean", "running_var"):
        b = bns.copy()
        b[field][1] = 0
        assert _net_bf16(lib, ops, slots, rbs, convs, b) == 1 and b"BatchNorm needs weight, bias, running_mean and running_var" in lib.gpn_last_error(), field
    c, s = convs.copy(), slots.copy()
    c["cin"], s["channels"][1] = 24, 24
    b = bns.copy()
    b["C"][0] = 24
    s["channels"][0] = 24
    assert _net_bf16(lib, ops, s, rbs, c, b) == 1 and b"multiples of 16" in lib.gpn_last_error()
    for slot in (0, 3):
        s = slots.copy()
        s["data"][slot] = 0
        assert _net_bf16(lib, ops, s, rbs, convs, bns) == 1 and b"null activation pointer" in lib.gpn_last_error(), slot
    bad = ops.copy()
    bad["dst"][2] = 9
    assert _net_bf16(lib, bad, slots, rbs, convs, bns) == 1 and b"out of range" in lib.gpn_last_error()


# ---------------------------------------------------------------------------------------------------- (c) workspace from shapes
def _unet_program(without_stem):
    import torch.nn as nn
    from gapartnet_amd.network import net_exec as NX
    from gapartnet_amd.network.backbone import SparseUNet
    norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1)
    net = SparseUNet.build(16 if without_stem else 6, [16, 32, 48, 64], 2, norm_fn, without_stem=without_stem)
    return NX, NX.NetProgram(net)


@pytest.mark.parametrize("without_stem", [False, True])
def test_bf16_workspace_is_half_of_the_fp32_activations_and_weights(lib, without_stem):
    lib.gpn_net_forward_bf16_ws_bytes.restype = ctypes.c_size_t
    NX, prog = _unet_program(without_stem)
    level_rows = np.asarray([7013, 2205, 611, 97], np.int64)  # (by hand: no device, no rulebook)
    n_slots = len(prog.slot_level)
    slots = np.zeros(n_slots, NX.SLOT_DT)
    slots["rows"] = level_rows[prog.slot_level_np]
    slots["channels"] = prog.slot_channels_np
    K_of = {"subm": 27, "down": 8, "inv": 8, "ident": 1}
    rbs = np.zeros(len(prog.rb_keys), NX.RB_DT)
    for i, (kind, lvl) in enumerate(prog.rb_keys):
        src = lvl + 1 if kind == "inv" else lvl
        dst = lvl + 1 if kind == "down" else lvl
        rbs[i]["n_src"], rbs[i]["n_dst"], rbs[i]["K"], rbs[i]["nbr"] = level_rows[src], level_rows[dst], K_of[kind], FAKE
    convs = np.zeros(len(prog.convs), NX.CONV_DT)
    convs["cin"], convs["cout"], convs["W"] = prog.conv_cin, prog.conv_cout, FAKE
    need = lib.gpn_net_forward_bf16_ws_bytes(_vp(prog.ops_np), len(prog.ops_np), _vp(slots), n_slots, _vp(rbs), _vp(convs))
    assert need > 0
    interior = sum(int(slots["rows"][s]) * int(slots["channels"][s]) for s in range(n_slots) if s not in (0, prog.out_slot))
    weights = sum(K_of[prog.rb_keys[op[4]][0]] * prog.conv_cin[op[5]] * prog.conv_cout[op[5]] for _, op in prog.conv_ops)
    assert weights == int(prog.conv_numel.sum())
    bound = 2 * (interior + weights) + 256 * (n_slots + len(prog.convs))
    assert need <= bound, (need, bound)
    assert need >= 2 * weights
    # the fp32 pass holds 4 bytes per element of the same slots and weights
    assert need <= (4 * (interior + weights)) // 2 + 256 * (n_slots + len(prog.convs))
    # and the whole pass runs its validation on these tables without a device: one byte short is refused, before any launch
    bns = np.zeros(len(prog.bns), NX.BN_DT)
    for f in ("weight", "bias", "running_mean", "running_var"):
        bns[f] = FAKE
    bns["C"], bns["eps"] = prog.bn_C, 1e-4
    slots["data"][0] = slots["data"][prog.out_slot] = FAKE
    rc = lib.gpn_net_forward_bf16(_vp(prog.ops_np), len(prog.ops_np), _vp(slots), n_slots, _vp(rbs), len(rbs), _vp(convs), len(convs),
                                  _vp(bns), len(bns), ctypes.c_void_p(FAKE), ctypes.c_size_t(need - 1), None)
    assert rc == 2 and b"workspace too small" in lib.gpn_last_error()


# ---------------------------------------------------------------------------------------------------- (d) coverage of the GPU table
def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return re.sub(r"//[^\n]*", "", fh.read())


def parsed_instantiations():
    """{(CB, NT)} csrc/spconv_bf16.hip instantiates: the shared input-width list x the masked-tile column-tile counts"""
    from tests.test_conv_instantiations import _width_list
    src = _src("spconv_bf16.hip")
    assert "GPN_CONV_CB(GPN_X)" in src and "GPN_TILES_NT(GPN_X)" in src
    lists = _src("spconv_dispatch.h")
    return {(cb, nt) for cb in _width_list(lists, "GPN_CONV_CB") for nt in _width_list(lists, "GPN_TILES_NT")}


def test_every_bf16_instantiation_has_a_gpu_case():
    from tests import test_gpu_conv_bf16 as T
    built = parsed_instantiations()
    assert len(built) == 77, len(built)
    covered = T.expected_instantiations()
    assert not built - covered, f"instantiations no case of tests/test_gpu_conv_bf16.py launches: {sorted(built - covered)}"
    assert not covered - built, f"the case table expects instantiations the source does not build: {sorted(covered - built)}"
    # the table spans what the issue sets: the four rulebook kinds, every input width, every output width, the tile tails
    assert {c.kind for c in T.CASES} == {"subm", "down", "inv", "ident"}
    assert {c.cin // 16 for c in T.CASES} == {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14}
    assert {c.cout // 16 for c in T.CASES} >= {1, 2, 3, 4, 5, 6, 7}
    assert {1, 15, 17, 33} <= {c.n for c in T.CASES}
    assert any(2000 <= c.n <= 9000 for c in T.CASES) and any(c.n >= 100000 for c in T.CASES)
    for c in T.CASES:  # (the float64 reference runs on the host)
        assert c.n_dst * c.cin * c.cout * c.K <= 7e9, c.id
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


def test_bf16_kernel_name_parser():
    from tests import test_gpu_conv_bf16 as T
    assert T.bf16_kernel_id("void (anonymous namespace)::spconv_bf16_kernel<14, 7>((anonymous namespace)::Bf16ConvArgs)") == (14, 7)
    assert T.bf16_kernel_id("_ZN12_GLOBAL__N_118spconv_bf16_kernelILi3ELi2EEEvNS_12Bf16ConvArgsE") == (3, 2)
    assert T.bf16_kernel_id("void (anonymous namespace)::spconv_tiles_kernel<7, 7, 1, false, true>(float const*)") is None


# ---------------------------------------------------------------------------------------------------- (e) the knob
def test_inference_dtype_other_than_bf16_raises():
    import torch.nn as nn
    from gapartnet_amd.network.backbone import SparseUNet
    from gapartnet_amd.spconv import pytorch as spconv
    assert SparseUNet.inference_dtype is None
    norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1)
    net = SparseUNet.build(16, [16, 32], 1, norm_fn, without_stem=True).eval()
    x = spconv.SparseConvTensor(torch.zeros(4, 16), torch.zeros(4, 4, dtype=torch.int32), [8, 8, 8], 1)
    prev = SparseUNet.inference_dtype
    try:
        for bad in (torch.float16, torch.float32, "bf16"):
            SparseUNet.inference_dtype = bad
            with pytest.raises(ValueError, match="inference_dtype"):
                net(x)
    finally:
        SparseUNet.inference_dtype = prev
    assert "inference_dtype" not in net.__dict__


def test_gapartnet_knob_sets_the_backbone_only():
    import inspect
    from gapartnet_amd.network.model import GAPartNet
    sig = inspect.signature(GAPartNet.__init__)
    assert sig.parameters["inference_dtype"].default is None
    assert isinstance(GAPartNet.inference_dtype, property)
