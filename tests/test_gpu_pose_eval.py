"""The pose-evaluation kernels (csrc/poseeval.hip, include/gpn.h section PE) on the device against the numpy float64 restatement
(tests/pose_eval_ref.py): sizes around the workgroup's 256 rows and the wave's 64, degenerate and empty slots, the tie rule's
exact cases, every symmetry type, sentinels behind every output, bit-equal reruns, argument errors without a launch."""
import ctypes

import numpy as np
import pytest
import torch

from gapartnet_amd import _C, hip_ops
from gapartnet_amd.misc import pose_metrics as PM
from gapartnet_amd.misc.info import SYMMETRY_MATRIX
from tests import pose_eval_ref as ref
from tests.pose_eval_cases import (assert_first_extrema, first_extremum_case, assert_fit_equals_ref, assert_pair_errors_equal_ref, coplanar_rotations, exact_cases,
                                   make_instances, pair_dicts, random_box_pairs, random_pairs, random_rotation, ref_pair_errors, rot,
                                   slots_of, turned_self_pairs)

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _guarded(cuda, shape, dtype):
    """an output buffer with 64 sentinel elements behind it -> (the output view, the whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 64,), SENTINEL if dtype.is_floating_point else 93, dtype=dtype, device=cuda)
    return whole[:n].view(*shape), whole


def _untouched(whole, n):
    tail = whole[n:]
    return bool((tail == (SENTINEL if whole.dtype.is_floating_point else 93)).all())


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


# ------------------------------------------------------------------------------------------------ gpn_pose_gt_fit
def _gt_fit_raw(cuda, xyz, npcs, slot, off, W):
    """the entry point itself, into guarded buffers -> dict of outputs (views), and whether every guard is intact"""
    S = len(off) - 1
    G = S * W
    shapes = {"count": ((G,), torch.int64), "valid": ((G,), torch.uint8), "scale": ((G,), torch.float64),
              "rotation": ((G, 3, 3), torch.float64), "translation": ((G, 3), torch.float64), "half": ((G, 3), torch.float64),
              "bbox": ((G, 8, 3), torch.float64)}
    bufs = {k: _guarded(cuda, s, d) for k, (s, d) in shapes.items()}
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(t).to(cuda)
    args = (d(xyz, torch.float32), d(npcs, torch.float32), d(slot, torch.int32), d(off, torch.int64))
    rc = _C.lib().gpn_pose_gt_fit(*(_C.ptr(a) for a in args), _C.i64(len(slot)), _C.i32(S), _C.i32(W),
                                  *(_C.ptr(bufs[k][0]) for k in shapes), hip_ops._stream())
    _C.check(rc, "gpn_pose_gt_fit")
    torch.cuda.synchronize()
    return {k: v[0] for k, v in bufs.items()}, all(_untouched(v[1], v[0].numel()) for v in bufs.values())


def test_gt_fit_matches_the_restatement_across_sizes(cuda):
    """1, 2, 3, 63, 64, 65, 257 and 5 000 points, a planar and a collinear instance, an empty slot, a scene with no instance, rows of
    no instance (negative slots), scenes of different size"""
    W = 6
    sizes = [[1, 2, 3, 63, 64, 65], [257, 5000, 40, 30, 0, 12], [0, 0, 0, 0, 0, 0]]
    xyz, npcs, lab, off, _ = make_instances(3, sizes, W, {(1, 2): "planar", (1, 3): "collinear"})
    slot = slots_of(lab, off, W)
    assert (slot < 0).sum() == 3 * 17 and off[1] - off[0] != off[2] - off[1]
    got, intact = _gt_fit_raw(cuda, xyz, npcs, slot, off, W)
    assert intact
    want = ref.fit_slots(xyz, npcs, slot, off, W)
    got["valid"] = got["valid"].bool()
    assert_fit_equals_ref(got, want, 1e-10)
    assert got["valid"].cpu().reshape(3, W).tolist() == [[False, False, True, True, True, True], [True, True, True, False, False, True],
                                                         [False] * 6]
    again, _ = _gt_fit_raw(cuda, xyz, npcs, slot, off, W)
    for k in got:
        a, b = _bits(got[k] if k != "valid" else got[k].to(torch.uint8)), _bits(again[k])
        assert torch.equal(a, b), k
    # through the module: the same values
    via = PM.gt_part_poses(torch.from_numpy(xyz).to(cuda), torch.from_numpy(npcs).to(cuda), torch.from_numpy(lab).to(cuda), off, W)
    assert all(torch.equal(_bits(via[k]), _bits(got[k])) for k in ("scale", "rotation", "translation", "half", "bbox", "count"))


def test_gt_fit_of_an_instance_does_not_depend_on_its_company(cuda):
    """an instance's result is bit-equal to its run alone: its points in the same order, nothing else in the scene, W = 1"""
    W = 6
    xyz, npcs, lab, off, _ = make_instances(9, [[300, 700, 65, 5000, 64, 3], [40, 1000, 0, 0, 0, 0]], W)
    slot = slots_of(lab, off, W)
    full, _ = _gt_fit_raw(cuda, xyz, npcs, slot, off, W)
    for g in (0, 1, 2, 3, 4, 5, 6, 7):
        rows = np.nonzero(slot == g)[0]
        alone, intact = _gt_fit_raw(cuda, xyz[rows], npcs[rows], np.zeros(len(rows), np.int64), np.array([0, len(rows)]), 1)
        assert intact
        for k in full:
            assert torch.equal(_bits(full[k][g]), _bits(alone[k][0])), (g, k)


def test_gt_fit_edges_and_argument_errors(cuda):
    L = _C.lib()
    z = ctypes.c_void_p(0)
    st = hip_ops._stream()
    # counts of 0 launch nothing (the pointers are never looked at)
    assert L.gpn_pose_gt_fit(z, z, z, z, _C.i64(0), _C.i32(0), _C.i32(4), z, z, z, z, z, z, z, st) == 0
    assert L.gpn_pose_gt_fit(z, z, z, z, _C.i64(0), _C.i32(3), _C.i32(0), z, z, z, z, z, z, z, st) == 0
    out = hip_ops.pose_gt_fit(torch.zeros(0, 3, device=cuda), torch.zeros(0, 3, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda),
                              torch.zeros(3, dtype=torch.int64, device=cuda), 2)   # two scenes without a row
    assert out["count"].tolist() == [0] * 4 and not out["valid"].any() and torch.isnan(out["bbox"]).all()
    # bad arguments are refused before a launch
    assert L.gpn_pose_gt_fit(z, z, z, z, _C.i64(-1), _C.i32(1), _C.i32(1), z, z, z, z, z, z, z, st) != 0
    assert b"gpn_pose_gt_fit" in L.gpn_last_error()
    assert L.gpn_pose_gt_fit(z, z, z, z, _C.i64(5), _C.i32(1), _C.i32(1), z, z, z, z, z, z, z, st) != 0       # NULL buffers
    assert L.gpn_pose_gt_fit(z, z, z, z, _C.i64(0), _C.i32(1 << 20), _C.i32(1 << 20), z, z, z, z, z, z, z, st) != 0  # S * W too large
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gpn_box_iou_3d
def _iou_raw(cuda, a, b):
    P = len(a)
    out, whole = _guarded(cuda, (P,), torch.float64)
    ta, tb = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).reshape(P, 8, 3)).to(cuda) for v in (a, b))
    _C.check(_C.lib().gpn_box_iou_3d(_C.ptr(ta), _C.ptr(tb), _C.i64(P), _C.ptr(out), hip_ops._stream()), "gpn_box_iou_3d")
    torch.cuda.synchronize()
    assert _untouched(whole, P)
    return out.clone()


def test_box_iou_exact_cases_and_coplanar_rotations(cuda):
    cases = list(exact_cases().values())
    got = _iou_raw(cuda, [c[0] for c in cases], [c[1] for c in cases]).cpu().numpy()
    assert np.abs(got - np.array([c[2] for c in cases])).max() <= 1e-12, got
    turned = coplanar_rotations()
    got = _iou_raw(cuda, [c[0] for c in turned], [c[1] for c in turned]).cpu().numpy()
    assert np.abs(got - np.array([ref.box_iou(a, b) for a, b in turned])).max() <= 1e-12
    same = turned_self_pairs()   # turned boxes against themselves and against copies off by round-off: the snap of the tie rule
    got = _iou_raw(cuda, [c[0] for c in same], [c[1] for c in same]).cpu().numpy()
    assert np.abs(got - 1.0).max() <= 1e-12, got
    one = _iou_raw(cuda, [cases[3][0]], [cases[3][1]])          # P = 1
    assert abs(float(one[0]) - 1.0 / 3.0) <= 1e-12


def test_box_iou_random_pairs_and_bad_boxes(cuda):
    pairs = random_box_pairs(200, 11)
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = np.array([ref.box_iou(*p) for p in pairs])
    got = _iou_raw(cuda, a, b)
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-12
    assert (want > 0).sum() >= 100
    assert torch.equal(_bits(got), _bits(_iou_raw(cuda, a, b)))          # bit-equal rerun
    # 65 pairs: 13 full workgroups of 5; a NaN corner and a box without a volume among them, their neighbours untouched
    a65, b65 = a[:65].copy(), b[:65].copy()
    a65[7, 3, 1] = np.nan
    b65[64] = b65[64, 0]
    got65 = _iou_raw(cuda, a65, b65).cpu().numpy()
    assert np.isnan(got65[[7, 64]]).all()
    keep = np.setdiff1d(np.arange(65), [7, 64])
    assert np.array_equal(got65[keep], got.cpu().numpy()[keep])    # a pair's result does not depend on the others


def test_box_iou_long_boxes(cuda):
    """aspect ratios up to 100: half extents 0.05 .. 0.1 with one axis stretched to at most 5, centres within 0.2, so coordinates
    stay below L = 5.2.  A clipped vertex carries a few eps L of absolute error, a face's area (perimeter x displacement) a few
    eps L^2, a cone area * height / 3 a few eps L^3, and twelve of them are added: about 100 eps L^3 = 100 x 2.2e-16 x 141 = 3e-12
    in the intersection's volume.  The IoU divides by the union, which is at least the smallest box, 8 x 0.05^3 = 1e-3: 3e-9 for
    either side, so kernel and restatement may differ by 6e-9; the bound asserted is 1e-8 (the measured figure is printed)."""
    pairs = random_box_pairs(60, 12, max_aspect=100.0)
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = np.array([ref.box_iou(*p) for p in pairs])
    got = _iou_raw(cuda, a, b).cpu().numpy()
    print(f"long boxes: worst |IoU - restatement| = {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= 1e-8


def test_box_iou_edges_and_argument_errors(cuda):
    L = _C.lib()
    z = ctypes.c_void_p(0)
    assert L.gpn_box_iou_3d(z, z, _C.i64(0), z, hip_ops._stream()) == 0
    assert hip_ops.box_iou_3d(torch.zeros(0, 8, 3, dtype=torch.float64, device=cuda), torch.zeros(0, 8, 3, dtype=torch.float64, device=cuda)).shape == (0,)
    assert L.gpn_box_iou_3d(z, z, _C.i64(-2), z, hip_ops._stream()) != 0 and b"gpn_box_iou_3d" in L.gpn_last_error()
    assert L.gpn_box_iou_3d(z, z, _C.i64(3), z, hip_ops._stream()) != 0
    with pytest.raises(_C.GpnError):
        hip_ops.box_iou_3d(torch.zeros(2, 8, 3, dtype=torch.float64), torch.zeros(2, 8, 3, dtype=torch.float64))   # CPU tensors
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gpn_pose_pair_errors
def test_pair_errors_match_the_restatement_for_every_type(cuda):
    d = random_pairs(21, 65)
    got = PM.pose_pair_errors(*pair_dicts(d, cuda))
    torch.cuda.synchronize()
    got_h = {k: v.cpu() for k, v in got.items()}
    compared = assert_pair_errors_equal_ref(got_h, ref_pair_errors(d), 1e-10)
    assert compared[0] >= 50 and set(d["ty"].tolist()) == set(range(len(SYMMETRY_MATRIX)))
    again = PM.pose_pair_errors(*pair_dicts(d, cuda))
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got)
    # the first 7 pairs alone: the same bits
    few = PM.pose_pair_errors(*pair_dicts({k: v[:7] for k, v in d.items()}, cuda))
    assert all(torch.equal(_bits(got[k][:7]), _bits(few[k])) for k in got)


def test_pair_errors_return_the_first_extremum(cuda):
    """on a candidate table of its own, where the winner is not a matter of round-off (tests/pose_eval_cases.py): every position of
    the table wins somewhere, duplicated candidates tie bit for bit and the first is returned, as for type 0 of SYMMETRY_MATRIX"""
    d, table, want = first_extremum_case()
    pred, gt, ty = pair_dicts(d, cuda)
    got = {k: v.cpu() for k, v in PM.pose_pair_errors(pred, gt, ty, table=table).items()}
    assert_first_extrema(got, d, want)
    for i, w in enumerate(want):
        assert abs(float(got["re_deg"][i]) - w["re_deg"]) <= 1e-10 and abs(float(got["iou"][i]) - w["iou"]) <= 1e-10, i
    d0 = random_pairs(3, 10)
    got = PM.pose_pair_errors(*pair_dicts(d0, cuda))
    sel = torch.from_numpy(d0["ty"] == 0)
    assert int(sel.sum()) == 2 and (got["k_re"].cpu()[sel] == 0).all() and (got["k_iou"].cpu()[sel] == 0).all()


@pytest.mark.parametrize("deg", [0.0, 1e-4, 5.0, 90.0, 179.9, 180.0])
def test_pair_error_angles(cuda, deg):
    """a prediction turned by `deg` about a generic axis, type 0: the angle comes out to 1e-9 degrees at both ends of the range (acos
    would give 1e-6 at 0); with the twelve-fold type and the turn about z the error is the distance to the next multiple of 30.
    The IoU of two boxes whose faces meet at the angle a has its intersection points conditioned like eps / a (t = dp / (dp - dq)
    with |dp - dq| ~ a L and dp known to a few eps L), so kernel and restatement may differ by 16 eps / a there: 2e-9 at 1e-4
    degrees, below 1e-10 from 2e-3 degrees on."""
    rng = np.random.default_rng(2)
    Rg = random_rotation(rng)
    axis = np.array([0.3, -0.5, 0.8])
    base = {"gs": [0.8] * 2, "gR": [Rg] * 2, "gt": [np.zeros(3)] * 2, "gh": [[0.3, 0.2, 0.1]] * 2, "ps": [0.8] * 2, "pt": [np.zeros(3)] * 2,
            "ph": [[0.3, 0.2, 0.1]] * 2, "pR": [rot(axis, deg) @ Rg, rot([0, 0, 1], deg) @ Rg], "ty": [0, 3]}
    d = {k: np.array(v) for k, v in base.items()}
    got = PM.pose_pair_errors(*pair_dicts(d, cuda))
    re = got["re_deg"].cpu().numpy()
    assert abs(re[0] - deg) <= 1e-9, re
    assert abs(re[1] - abs(deg - 30.0 * round(deg / 30.0))) <= 1e-9, re
    want = ref_pair_errors(d)
    # (faces meeting at less than 1e-9 rad are inside the snap of the tie rule, 2^-26 of the extent: no intersection point is formed)
    iou_tol = lambda a: max(1e-10, 16 * 2.2e-16 / np.radians(a)) if np.radians(a) > 1e-9 else 1e-10
    assert abs(re[0] - want[0]["re_deg"]) <= 1e-10 and abs(float(got["iou"][0]) - want[0]["iou"]) <= iou_tol(deg)
    # the twelve-fold pair: the best candidate's box meets the prediction's at the residual angle
    assert abs(re[1] - want[1]["re_deg"]) <= 1e-10 and abs(float(got["iou"][1]) - want[1]["iou"]) <= iou_tol(want[1]["re_deg"])


def test_pair_errors_sentinels_bad_types_and_argument_errors(cuda):
    d = random_pairs(5, 10)
    pred, gt, ty = pair_dicts(d, cuda)
    ty[3] = 7          # outside the table
    pred["rotation"][4, 1, 1] = float("nan")
    table, start, count = PM.symmetry_table(cuda)
    P = 10
    bufs = {k: _guarded(cuda, (P,), torch.float64 if k in ("re_deg", "te", "se", "iou") else torch.int32)
            for k in ("re_deg", "k_re", "te", "se", "iou", "k_iou")}
    sides = [pred[k].contiguous() for k in ("scale", "rotation", "translation", "half")] + [gt[k].contiguous() for k in ("scale", "rotation", "translation", "half")]
    L = _C.lib()
    call = lambda n, K, T: L.gpn_pose_pair_errors(*(_C.ptr(t) for t in sides), _C.ptr(ty), _C.i64(n), _C.ptr(table), _C.i32(K), _C.ptr(start),
                                                  _C.ptr(count), _C.i32(T), *(_C.ptr(bufs[k][0]) for k in bufs), hip_ops._stream())
    _C.check(call(P, int(table.shape[0]), int(start.numel())), "gpn_pose_pair_errors")
    torch.cuda.synchronize()
    assert all(_untouched(w, P) for _, w in bufs.values())
    out = {k: v[0].cpu() for k, v in bufs.items()}
    assert np.isnan(float(out["re_deg"][3])) and int(out["k_re"][3]) == -1 and int(out["k_iou"][3]) == -1 and np.isnan(float(out["iou"][3]))
    assert np.isnan(float(out["re_deg"][4])) and np.isnan(float(out["iou"][4])) and np.isfinite(float(out["te"][4]))
    want = ref_pair_errors(d)
    for i in (0, 1, 2, 5, 6, 7, 8, 9):
        assert abs(float(out["re_deg"][i]) - want[i]["re_deg"]) <= 1e-10 and abs(float(out["iou"][i]) - want[i]["iou"]) <= 1e-10
    # a table shorter than the type's range: NaN and -1, nothing read past it
    _C.check(call(P, 3, int(start.numel())), "gpn_pose_pair_errors")
    torch.cuda.synchronize()
    late = (start.cpu() + count.cpu() > 3)[ty.cpu().clamp(0, 4).long()] | (ty.cpu() > 4)
    assert (bufs["k_re"][0].cpu()[late] == -1).all() and torch.isnan(bufs["iou"][0].cpu()[late]).all()
    assert call(0, 1, 1) == 0
    assert call(-1, 42, 5) != 0 and b"gpn_pose_pair_errors" in L.gpn_last_error()
    assert call(P, 0, 5) != 0 and call(P, 42, 0) != 0
    torch.cuda.synchronize()
