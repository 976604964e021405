"""Articulation from two frames without a GPU (include/gpn.h section AR): the numpy path of gapartnet_amd/misc/articulation.py against
the restatement in plain loops (tests/articulation_ref.py), exactly - everything is integer - and the whole call on a rendered
two-frame scene (tests/articulation_scenes.py): a door that turned, a drawer that moved, a handle that stayed."""
import os
import re

import numpy as np
import pytest
import torch

from gapartnet_amd.misc import articulation as AR
from tests import articulation_ref as REF
from tests import articulation_scenes as SC
from tests import joint_ref as JR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SCENE = 256   # sample_number of the scene tests: every part is smaller, so every part is taken whole


def _check_against_ref(d, cls_a, cls_b, min_iou, default_valid=False):
    """match_parts on the CPU == the restatement, field by field, for every frame pair of the batch"""
    t = torch.from_numpy
    got = AR.match_parts(t(d["inst_a"]), t(d["inst_b"]), cls_a, cls_b, None if default_valid else t(d["valid_a"]),
                         None if default_valid else t(d["valid_b"]), min_iou=min_iou)
    for v in range(d["inst_a"].shape[0]):
        va = (d["inst_a"][v] >= 0) if default_valid else d["valid_a"][v]
        vb = (d["inst_b"][v] >= 0) if default_valid else d["valid_b"][v]
        inter, area_a, area_b = REF.overlap(d["inst_a"][v], va, d["n_a"][v], d["inst_b"][v], vb, d["n_b"][v])
        taken = sorted(REF.match(inter, area_a, area_b, cls_a[v], cls_b[v], min_iou))
        assert got.pairs[v].tolist() == [[i, j] for i, j, _, _ in taken], v
        assert got.inter[v].tolist() == [c for _, _, c, _ in taken] and got.union[v].tolist() == [u for _, _, _, u in taken], v
        assert got.iou[v].tolist() == [c / u for _, _, c, u in taken], v
        assert got.area_a[v].tolist() == [area_a.get(i, 0) for i in range(d["n_a"][v])], v
        assert got.area_b[v].tolist() == [area_b.get(j, 0) for j in range(d["n_b"][v])], v
        assert got.unmatched_a[v].tolist() == sorted(set(range(d["n_a"][v])) - {i for i, _, _, _ in taken}), v
        assert got.unmatched_b[v].tolist() == sorted(set(range(d["n_b"][v])) - {j for _, j, _, _ in taken}), v
    return got


@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (33, 33)])
@pytest.mark.parametrize("counts", [([0], [0]), ([1], [1]), ([2], [2]), ([64], [64]), ([0, 1, 64, 2], [3, 0, 64, 5])])
def test_random_maps_equal_the_restatement(shape, counts):
    n_a, n_b = counts
    V = len(n_a)
    d = SC.random_pair(11 + shape[1] + sum(n_a), V, shape[0], shape[1], n_a, n_b, junk=True)
    cls_a, cls_b = SC.class_lists(1, n_a, 2), SC.class_lists(2, n_b, 2)
    got = _check_against_ref(d, cls_a, cls_b, 0.05)
    if shape == (33, 33) and n_a == [2]:
        assert sum(len(p) for p in got.pairs) > 0, "something is matched"


def test_valid_defaults_to_inst_at_least_zero_and_zero_valid_takes_a_pixel_out():
    d = SC.random_pair(5, 2, 9, 14, [3, 4], [4, 2], junk=True)
    cls_a, cls_b = SC.class_lists(3, d["n_a"], 1), SC.class_lists(4, d["n_b"], 1)
    _check_against_ref(d, cls_a, cls_b, 0.1, default_valid=True)
    full = dict(d, valid_a=np.ones_like(d["valid_a"]), valid_b=np.ones_like(d["valid_b"]))
    a = _check_against_ref(full, cls_a, cls_b, 0.1)
    b = _check_against_ref(d, cls_a, cls_b, 0.1)      # (a fifth of the pixels have valid = 0 under inst >= 0)
    assert any(x.tolist() != y.tolist() for x, y in zip(a.area_a, b.area_a)), "valid = 0 changes the areas"


def _line(pairs, n):
    """1 x n maps from a list of (a, b) per pixel"""
    a, b = np.array([p[0] for p in pairs], np.int32).reshape(1, 1, n), np.array([p[1] for p in pairs], np.int32).reshape(1, 1, n)
    return a, b


def _match_line(pixels, cls_a, cls_b, min_iou):
    a, b = _line(pixels, len(pixels))
    d = dict(inst_a=a, inst_b=b, valid_a=np.ones_like(a, np.uint8), valid_b=np.ones_like(b, np.uint8), n_a=[len(cls_a)], n_b=[len(cls_b)])
    return _check_against_ref(d, [np.array(cls_a)], [np.array(cls_b)], min_iou)


def test_the_class_veto_passes_over_the_largest_overlap():
    # A0 overlaps B0 in 6 pixels (other class) and B1 in 2 (same class)
    got = _match_line([(0, 0)] * 6 + [(0, 1)] * 2 + [(-1, 1)], [4], [5, 4], 0.1)
    assert got.pairs[0].tolist() == [[0, 1]] and got.inter[0].tolist() == [2] and got.union[0].tolist() == [9]


def test_the_threshold_itself_is_eligible_and_one_pixel_less_is_not():
    on = _match_line([(0, -1), (0, 0), (-1, 0), (-1, 0)], [1], [1], 0.25)          # inter 1, union 4
    assert on.pairs[0].tolist() == [[0, 0]] and on.iou[0].tolist() == [0.25]
    off = _match_line([(0, -1), (0, 0), (-1, 0), (-1, 0), (-1, 0)], [1], [1], 0.25)  # inter 1, union 5
    assert off.pairs[0].tolist() == [] and off.unmatched_a[0].tolist() == [0] and off.unmatched_b[0].tolist() == [0]


def test_ties_go_to_the_smaller_i_then_the_smaller_j():
    # (0,0), (1,0) and (1,1) all have IoU 1/3: (0,0) first, which leaves (1,1)
    got = _match_line([(0, -1), (0, 0), (1, 0), (1, 1), (-1, 1)], [1, 1], [1, 1], 0.1)
    assert got.pairs[0].tolist() == [[0, 0], [1, 1]]
    # (0,0) and (0,1) both 2/4: the smaller j
    got = _match_line([(0, 0), (0, 0), (0, 1), (0, 1)], [1], [1, 1], 0.1)
    assert got.pairs[0].tolist() == [[0, 0]] and got.unmatched_b[0].tolist() == [1]
    # two identical parts on each side, laid over each other crosswise: every pair has IoU 1/3
    got = _match_line([(0, 0), (0, 1), (1, 0), (1, 1)], [1, 1], [1, 1], 0.1)
    assert got.pairs[0].tolist() == [[0, 0], [1, 1]]


def test_greedy_is_what_comes_out_where_the_optimal_assignment_differs():
    """IoU (0,0) = 6/12, (0,1) = (1,0) = 3/9, (1,1) = 0: the optimal assignment is {(0,1), (1,0)} (sum 2/3); greedy takes (0,0) and
    then has nothing left"""
    got = _match_line([(0, 0)] * 6 + [(0, 1)] * 3 + [(1, 0)] * 3, [1, 1], [1, 1], 0.1)
    assert got.pairs[0].tolist() == [[0, 0]] and got.inter[0].tolist() == [6] and got.union[0].tolist() == [12]
    assert got.unmatched_a[0].tolist() == [1] and got.unmatched_b[0].tolist() == [1]


def test_more_than_64_parts_raise():
    inst = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        AR.match_parts(inst, inst, [np.ones(65, np.int64)], [np.ones(3, np.int64)])
    with pytest.raises(ValueError):
        AR.match_parts(inst, inst, [np.ones(3, np.int64)], [np.ones(65, np.int64)])
    AR.match_parts(inst, inst, [np.ones(64, np.int64)], [np.ones(64, np.int64)])


# ---- the rendered scene ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return SC.cabinet_scene()


def _scene_call(s, dev="cpu"):
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    sizes1 = [int((s["inst_a"] == i).sum()) for i in range(3)]
    sizes2 = [int((s["inst_b"] == s["partner"][i]).sum()) for i in range(3)]
    assert max(sizes1 + sizes2) <= K_SCENE and min(sizes1 + sizes2) >= 16, (sizes1, sizes2)
    picks, ransac = SC.whole_picks(sizes1, sizes2, K_SCENE)
    return AR.articulation_from_maps(t(s["depth_a"]), t(s["depth_b"]), s["K"], t(s["inst_a"]), t(s["inst_b"]), s["classes_a"], s["classes_b"],
                                     sample_number=K_SCENE, picks=picks, ransac_picks=ransac)


def test_the_scene_gives_a_turned_door_a_moved_drawer_and_a_fixed_handle(scene):
    from gapartnet_amd import inference
    art = _scene_call(scene)
    assert art.frame.tolist() == [0, 0, 0] and art.part_a.tolist() == [0, 1, 2]
    assert art.part_b.tolist() == [scene["partner"][i] for i in range(3)]
    assert art.part_class.tolist() == [SC.DOOR, SC.DRAWER, SC.HANDLE] and art.joint_type == ["revolute", "prismatic", "fixed"]
    assert art.matches.unmatched_a[0].tolist() == [] and art.matches.unmatched_b[0].tolist() == []
    assert art.n_points_a.tolist() == [int((scene["inst_a"] == i).sum()) for i in range(3)]
    axis, hinge, angle = scene["door"]
    # the door: the bounds of the turned-slab test of the joint kernels, which the numpy oracle meets on the same pixels
    clouds = []
    for side, part in (("a", 0), ("b", scene["partner"][0])):
        depth = scene["depth_" + side]
        rows, valid = inference._backproject_numpy(depth[None], np.zeros((1,) + depth.shape + (3,), np.uint8), scene["K"][None], None, 1.0, False)
        clouds.append(REF.gather(rows[:, :3], scene["inst_" + side], valid[0], 3, part))
    x, y, nrm = JR.joint_sample_ref(clouds[0], clouds[1], np.arange(len(clouds[0])), np.arange(len(clouds[1])))
    ref = JR.cpd_rigid_ref(x, y)
    ref_axis, _, ref_angle = JR.joint_from_rigid_ref(ref["R"], ref["t"], nrm)

    def off_axis(a):
        return np.rad2deg(np.arccos(min(1.0, abs(float(np.dot(a, axis))))))
    for name, ax, an in (("oracle", ref_axis, ref_angle), ("cpu path", art.cpd.axis[0].numpy(), float(art.cpd.angle[0]))):
        print(f"door, {name}: angle {np.rad2deg(an):.3f} deg (truth {np.rad2deg(angle):.1f}), axis off by {off_axis(ax):.3f} deg")
        assert abs(np.rad2deg(an) - np.rad2deg(angle)) <= 1.0, name
        assert off_axis(ax) <= 2.0, name
    # the drawer: prismatic, the displacement is reported (not bounded: a flat front slides in its own plane under CPD)
    print(f"drawer: displacement {float(art.cpd.angle[1]):.4f} along {art.cpd.axis[1].tolist()} (truth {scene['drawer_move']} along -z)")
    assert bool(torch.isfinite(art.cpd.angle[1])) and bool(torch.isfinite(art.cpd.axis[1]).all())
    assert torch.equal(art.cpd.pivot[1], art.norm[1, 1:])
    # the handle: fixed - no joint, but its rigid transform is there
    for leg in (art.cpd, art.ransac):
        assert bool(torch.isnan(leg.axis[2]).all()) and bool(torch.isnan(leg.pivot[2]).all()) and bool(torch.isnan(leg.angle[2]))
    assert bool(torch.isfinite(art.cpd.rotation[2]).all()) and bool(torch.isfinite(art.cpd.translation[2]).all())


def test_draw_articulation_draws_the_moving_parts_only(scene):
    art = _scene_call(scene)
    rgb = np.zeros(scene["depth_a"].shape + (3,), np.uint8)
    img = AR.draw_articulation(rgb, scene["K"], art, 0)
    assert img.shape == rgb.shape and (img != rgb).any()
    assert not (AR.draw_articulation(rgb, scene["K"], art, 1) != rgb).any(), "another frame pair has no joints"


def test_no_parts_give_an_empty_articulation(scene):
    t = torch.from_numpy
    none = torch.full((48, 64), -1, dtype=torch.int64)
    art = AR.articulation_from_maps(t(scene["depth_a"]), t(scene["depth_b"]), scene["K"], none, none, [], [])
    assert art.frame.shape == (0,) and art.joint_type == [] and art.cpd.axis.shape == (0, 3) and art.norm.shape == (0, 4)
    assert art.matches.pairs[0].shape == (0, 2)


def test_command_line_with_instance_maps(scene, tmp_path):
    for side in "ab":
        np.save(tmp_path / f"{side}.npy", scene["depth_" + side])
        np.save(tmp_path / f"{side}_inst.npy", scene["inst_" + side])
        np.save(tmp_path / f"{side}_cls.npy", scene["classes_" + side])
    np.savetxt(tmp_path / "K.txt", scene["K"])
    p = lambda *names: [str(tmp_path / n) for n in names]  # noqa: E731
    out = tmp_path / "out"
    assert AR.main(["--depth", *p("a.npy", "b.npy"), "--instances", *p("a_inst.npy", "b_inst.npy"), "--classes", *p("a_cls.npy", "b_cls.npy"),
                    "--intrinsics", str(tmp_path / "K.txt"), "--out", str(out), "--sample_number", str(K_SCENE), "--device", "cpu"]) == 0
    got = np.load(out / "a_articulation.npz")
    assert got["joint_type"].tolist() == ["revolute", "prismatic", "fixed"] and got["part_b"].tolist() == [2, 0, 1]
    assert got["cpd_axis"].shape == (3, 3) and abs(np.rad2deg(got["cpd_angle"][0]) - 24.0) <= 1.0
    from PIL import Image
    assert np.asarray(Image.open(out / "a_articulation.png")).shape == (48, 64, 3)
    with pytest.raises(SystemExit):
        AR.main(["--depth", *p("a.npy", "b.npy"), "--intrinsics", str(tmp_path / "K.txt"), "--out", str(out)])


def test_argument_errors_do_not_touch_the_device():
    import ctypes
    from gapartnet_amd import _C
    L = _C.lib()
    buf = np.zeros(64, np.int64)
    p, nul, i32 = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(0), ctypes.c_int
    assert L.gpn_parts_overlap(p, p, p, p, p, p, i32(1), i32(2), i32(2), i32(65), i32(1), p, p, p, nul) == 1
    assert b"bad argument" in L.gpn_last_error()
    assert L.gpn_parts_overlap(p, p, p, p, p, p, i32(65536), i32(2), i32(2), i32(1), i32(1), p, p, p, nul) == 1
    assert L.gpn_parts_overlap(p, p, p, p, p, p, i32(1), i32(2), i32(16385), i32(1), i32(1), p, p, p, nul) == 1
    assert L.gpn_parts_overlap(p, nul, p, p, p, p, i32(1), i32(2), i32(2), i32(1), i32(1), p, p, p, nul) == 1
    assert L.gpn_parts_match(p, p, p, p, p, nul, nul, ctypes.c_double(0.1), i32(1), i32(65), i32(1), p, p, p, p, p, nul) == 1
    assert L.gpn_parts_match(p, p, p, p, p, nul, nul, ctypes.c_double(0.1), i32(1), i32(1), i32(1), p, p, nul, p, p, nul) == 1
    assert L.gpn_parts_gather(p, p, p, p, p, i32(1), i32(2), i32(2), i32(65), ctypes.c_int64(4), p, nul, ctypes.c_size_t(0), nul) == 1
    assert L.gpn_parts_gather(p, p, p, p, nul, i32(1), i32(2), i32(2), i32(2), ctypes.c_int64(4), p, nul, ctypes.c_size_t(0), nul) == 1
    assert L.gpn_parts_gather(p, p, p, p, p, i32(1), i32(2), i32(2), i32(2), ctypes.c_int64(4), p, nul, ctypes.c_size_t(0), nul) == 2
    # counts of 0 are valid calls that launch nothing
    assert L.gpn_parts_overlap(nul, nul, nul, nul, nul, nul, i32(0), i32(2), i32(2), i32(4), i32(4), nul, nul, nul, nul) == 0
    assert L.gpn_parts_match(nul, nul, nul, nul, nul, nul, nul, ctypes.c_double(0.1), i32(0), i32(4), i32(4), nul, nul, nul, nul, nul, nul) == 0
    assert L.gpn_parts_gather(nul, nul, nul, nul, nul, i32(0), i32(2), i32(2), i32(4), ctypes.c_int64(0), nul, nul, ctypes.c_size_t(0), nul) == 0
    assert L.gpn_parts_gather_ws_bytes(i32(0), i32(2), i32(2), i32(4)) == 0
    assert L.gpn_parts_gather_ws_bytes(i32(2), i32(33), i32(32), i32(3)) >= 2 * 3 * 2 * 4


def test_header_registry_and_makefile_name_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpn.h")).read(), flags=re.S)
    core = open(os.path.join(ROOT, "gapartnet_amd", "csrc", "gpn_core.hip")).read()
    for name in ("gpn_parts_overlap", "gpn_parts_match", "gpn_parts_gather_ws_bytes", "gpn_parts_gather"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert f'"{name}"' in core, name
    assert "GPN_PARTS_MAX 64" in text
    assert "articulate.hip" in open(os.path.join(ROOT, "gapartnet_amd", "csrc", "Makefile")).read()
