"""Articulated assets -> training views on the host (gapartnet_amd/dataset/render_assets.py): the loader, the draw order, the box
articulation and the NPCS frames pinned to the reference's own run (tests/golden/render_asset.npz, made by
tests/golden/make_golden_render.py); the package's numpy path against the per-pixel restatement (tests/render_ref.py); the file
layout; a generated box asset that ties the forward kinematics to the box articulation; the OBJ reader; the CLI; the C ABI."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

from gapartnet_amd.dataset import render_assets as RA
from tests import render_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("gpn_render_max_links", "gpn_render_ws_bytes", "gpn_render_setup", "gpn_render_raster", "gpn_render_annotate")
RANGE_KEYS = ("theta_min", "theta_max", "phi_min", "phi_max", "distance_min", "distance_max")
EXACT = ("depth", "tri", "sem", "ins", "link_area", "link_inst", "npcs", "counters")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "render_asset.npz"))


@pytest.fixture(scope="module")
def asset():
    return RA.load_asset(RR.fixture_asset())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_images(got, want, keys=EXACT):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert np.abs(got["rgb"].astype(np.int32) - want["rgb"].astype(np.int32)).max(initial=0) <= 1


def _qpos(golden):
    return {str(n): float(q) for n, q in zip(golden["joint_names"], golden["qpos"])}


@pytest.fixture(scope="module")
def golden_render(golden, asset):
    """the golden view's tables, the package's numpy path and the restatement on them (computed once)"""
    H, W = int(golden["H"]), int(golden["W"])
    g = RA.geometry_tables([asset])
    t, extras = RA.view_tables([asset], [RA.RenderRequest(0, _qpos(golden), golden["camera_pos"])], H, W)
    t["background"] = RA.BACKGROUND_RGB
    return g, t, extras, RA.render_tables_numpy(g, t), RR.render(g, t)


def test_the_fixture_asset_is_what_the_issue_describes(asset):
    assert len(asset.links) == 6 and asset.links[0] == "base"  # 5 links and the base
    assert asset.verts.shape == (2080, 3) and asset.tris.shape == (5384, 3)
    assert asset.verts.dtype == np.float32 and asset.tris.dtype == np.int32
    assert list(asset.targets) == ["link_0", "link_1", "link_3", "link_4"]
    assert asset.link_cat.tolist() == [-1, 3, 3, -1, 0, 0] and asset.link_rank.tolist() == [-1, 0, 1, -1, 2, 3]
    assert RA.GAPART_NAMES.index("hinge_door") == 3 and len(RA.GAPART_NAMES) == 9


def test_joints_dictionary_matches_the_reference(golden, asset):
    names = [str(n) for n in golden["joint_names"]]
    assert list(asset.joints) == names
    for i, n in enumerate(names):
        j = asset.joints[n]
        assert list(j) == ["type", "parent", "child", "xyz", "rpy", "axis", "limit"]
        assert (j["type"], j["parent"], j["child"]) == tuple(str(golden[f"joint_{k}"][i]) for k in ("type", "parent", "child"))
        assert j["xyz"] == golden["joint_xyz"][i].tolist() and j["rpy"] == golden["joint_rpy"][i].tolist()
        for k in ("axis", "limit"):
            want = golden[f"joint_{k}"][i]
            assert (j[k] is None) if np.isnan(want).all() else (j[k] == want.tolist()), (n, k)


def test_draw_order_and_camera_position(golden, asset):
    rng = np.random.RandomState(int(golden["seed"]))
    qpos = RA.sample_qpos(asset, rng)
    cam = RA.sample_camera(dict(zip(RANGE_KEYS, golden["camera_range"].tolist())), rng)
    assert list(qpos) == [str(n) for n in golden["joint_names"]]
    assert np.array_equal(np.array(list(qpos.values())), golden["qpos"])
    assert np.array_equal(cam, golden["camera_pos"])


def test_part_boxes_and_npcs_frames_match_the_reference(golden, asset):
    boxes = RA.part_boxes(asset, _qpos(golden))
    assert list(boxes) == [str(n) for n in golden["box_links"]]
    for i, n in enumerate(boxes):
        assert boxes[n]["category_id"] == int(golden["box_category"][i])
        assert str(boxes[n]["bbox"].dtype) == str(golden["box_dtypes"][i])
        assert np.abs(boxes[n]["bbox"] - golden["boxes"][i]).max() <= 1e-12
    frames = RA.npcs_frames(boxes)
    for i, n in enumerate(str(v) for v in golden["valid_links"]):
        assert list(frames[n]) == ["R", "T", "S", "scaler"]
        for k in ("R", "T", "S"):
            assert np.abs(frames[n][k] - golden[f"rts_{k}"][i]).max() <= 1e-12, (n, k)
        assert abs(frames[n]["scaler"] - golden["rts_scaler"][i]) <= 1e-12
    b = golden["boxes"][0]
    c = b - b.mean(0)
    spin = RA.axangle_matrix(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), 0.7)
    assert np.abs(RA.fit_rotation(c, c @ spin.T) - golden["rotation_probe"]).max() <= 1e-12


def test_camera_frame(golden):
    H, W = int(golden["H"]), int(golden["W"])
    K, R, t = RA.camera_frame(golden["camera_pos"], H, W)
    assert np.array_equal(K, golden["K"]) and np.array_equal(R, golden["R"]) and np.array_equal(t, golden["t"])
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
    origin = (np.zeros(3) - t) @ R  # the camera looks at the origin: it projects to the principal point, in front
    assert abs(origin[0]) < 1e-12 and abs(origin[1]) < 1e-12 and origin[2] > 0
    above = (np.array([0.0, 0.0, 1.0]) - t) @ R  # world +z is up in the image: smaller y
    assert above[1] / above[2] < origin[1] / origin[2]
    assert K[0, 2] == W / 2 and K[1, 2] == H / 2 and abs(K[0, 0] - W / 2 / np.tan(np.radians(35.0) / 2)) < 1e-12


def test_numpy_path_equals_the_restatement(golden, golden_render):
    g, t, _, got, want = golden_render
    assert_same_images(got, want)
    assert (got["depth"] > 0).sum() > 500 and got["link_inst"][0].tolist() == [-1, 0, 1, -1, 2, 3]
    # and both reproduce the maps the fixture's NPCS run was made on
    assert np.array_equal(_bits(got["depth"][0]), _bits(golden["depth"])) and np.array_equal(got["ins"][0], golden["ins"])
    assert np.array_equal(got["sem"][0], golden["sem"])


def test_npcs_map_matches_the_reference_run(golden, golden_render):
    """the reference's `@` may sum the three products in another order: a float64 difference of a few 1e-16 on values below 1,
    which the float32 cast turns into at most one float32 ulp; where the value itself is tiny, 1e-12 absolute"""
    got, want = golden_render[3]["npcs"][0], golden["npcs"]
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert (diff <= np.maximum(ulp.astype(np.float64), 1e-12)).all()
    assert np.array_equal(got[golden["ins"] < 0], np.zeros_like(got[golden["ins"] < 0]))
    assert np.abs(got[golden["ins"] >= 0]).max() <= 0.51  # on the surface of a part: inside its normalised box


def test_written_files_have_the_reference_layout(golden, asset, tmp_path):
    H, W = int(golden["H"]), int(golden["W"])
    view, = RA.render_views([asset], [RA.RenderRequest(0, _qpos(golden), golden["camera_pos"])], H, W, device="cpu")
    name = "StorageFurniture_45780_0_0"
    RA.write_view(str(tmp_path), name, view, dict(model_id=45780, category="StorageFurniture", camera_idx=0, render_idx=0))
    files = sorted(f"{sub}/{fn}" for sub in os.listdir(tmp_path) for fn in os.listdir(tmp_path / sub))
    assert files == sorted(str(f) for f in golden["files"])
    members = []
    for f in files:
        if f.endswith(".npz"):
            z = np.load(tmp_path / f)
            members += [f"{f.split('/')[0]}:{k}:{z[k].dtype}:{'x'.join(str(s) for s in z[k].shape)}" for k in z.files]
    assert members == [str(m) for m in golden["npz_members"]]
    from PIL import Image
    im = Image.open(tmp_path / "rgb" / f"{name}.png")
    assert [im.mode, f"{im.size[0]}x{im.size[1]}"] == [str(s) for s in golden["png"]]
    with open(tmp_path / "bbox" / f"{name}.pkl", "rb") as fd:
        pk = pickle.load(fd)
    assert list(pk) == [str(k) for k in golden["pkl_top_keys"]]
    assert list(pk["bbox_pose_dict"]) == [str(k) for k in golden["pkl_links"]]
    for i, (link, entry) in enumerate(pk["bbox_pose_dict"].items()):
        assert list(entry) == [str(k) for k in golden["pkl_entry_keys"]]
        assert [type(entry[k]).__name__ for k in entry] == [str(k) for k in golden["pkl_entry_types"]]
        assert list(entry["pose_RTS_param"]) == [str(k) for k in golden["pkl_rts_keys"]]
        assert entry["instance_id"] == int(golden["valid_ids"][i])
        assert np.abs(entry["bbox"] - golden["boxes"][i]).max() <= 1e-12
    with open(tmp_path / "metafile" / f"{name}.json") as fd:
        meta = json.load(fd)
    assert list(meta) == [str(k) for k in golden["meta_keys"]]
    assert meta["target_gaparts"] == [str(k) for k in golden["target_gaparts"]]
    assert list(meta["joint_qpos"]) == [str(n) for n in golden["joint_names"]]
    assert meta["camera_intrinsic"] == golden["K"].reshape(-1).tolist() and meta["width"] == W and meta["height"] == H
    # the converter's reader takes them back
    from gapartnet_amd.dataset.convert_rendered import read_view
    back = read_view(str(tmp_path), name)
    assert np.array_equal(back["rgb"], view.rgb) and np.array_equal(_bits(back["depth"]), _bits(view.depth))
    assert np.array_equal(back["sem"], view.sem) and np.array_equal(back["ins"], view.ins)
    assert np.array_equal(_bits(back["npcs"]), _bits(view.npcs)) and np.array_equal(back["K"], view.camera_intrinsic)


# ---- a generated asset: body, revolute door with a fixed handle, prismatic drawer, one link that is no GAPart ---------------
def _box_obj(path, lo, hi, quads=True, mtl=None):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    c = [[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)]
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(path, "w") as fd:
        if mtl:
            fd.write(f"mtllib {mtl}\nusemtl paint\n")
        for v in c:
            fd.write("v %.6f %.6f %.6f\n" % tuple(v))
        for f in faces:
            if quads:
                fd.write("f " + " ".join(str(i + 1) for i in f) + "\n")
            else:
                fd.write("f %d %d %d\nf %d %d %d\n" % (f[0] + 1, f[1] + 1, f[2] + 1, f[0] + 1, f[2] + 1, f[3] + 1))


def _corners(lo, hi):
    """the annotation's corner order: |b1 - b0|, |b1 - b2|, |b0 - b4| are the three extents"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return [[x0, y1, z1], [x1, y1, z1], [x1, y0, z1], [x0, y0, z1], [x0, y1, z0], [x1, y1, z0], [x1, y0, z0], [x0, y0, z0]]


PARTS = {  # link -> (box in the rest world frame, category or None)
    "link_body": ((-0.4, -0.5, -0.5), (0.4, 0.5, 0.1), None),
    "link_door": ((-0.45, -0.5, -0.5), (-0.4, 0.0, 0.1), "hinge_door"),
    "link_handle": ((-0.55, -0.15, -0.3), (-0.45, -0.05, 0.0), "line_fixed_handle"),
    "link_drawer": ((-0.45, -0.45, 0.15), (0.3, 0.45, 0.4), "slider_drawer"),
}


@pytest.fixture(scope="module")
def box_asset(tmp_path_factory):
    """the base joint carries a yaw of 90 degrees and an offset, as PartNet-Mobility's base joints carry a rotation: meshes are
    written in the body frame, boxes annotated in the world frame"""
    root = tmp_path_factory.mktemp("box_asset")
    os.makedirs(root / "objs")
    yaw, off = np.pi / 2, np.array([0.05, -0.1, 0.2])
    Rb = RA.rpy_matrix([0, 0, yaw])
    with open(root / "objs" / "paint.mtl", "w") as fd:
        fd.write("newmtl paint\nKd 0.9 0.5 0.1\nmap_Kd none.jpg\n")
    for i, (link, (lo, hi, _)) in enumerate(PARTS.items()):
        _box_obj(root / "objs" / f"{link}.obj", lo, hi, quads=i % 2 == 0, mtl="paint.mtl" if i == 0 else None)

    def joint(name, jt, parent, child, xyz=(0, 0, 0), rpy=(0, 0, 0), axis=None, limit=None):
        s = f'<joint name="{name}" type="{jt}"><origin xyz="%r %r %r" rpy="%r %r %r"/>' % tuple(float(a) for a in (*xyz, *rpy))
        if axis:
            s += '<axis xyz="%g %g %g"/>' % tuple(axis)
        if limit:
            s += '<limit lower="%g" upper="%g"/>' % tuple(limit)
        return s + f'<child link="{child}"/><parent link="{parent}"/></joint>'

    def link(name, origin=(0, 0, 0)):
        return (f'<link name="{name}"><visual name="{name}-0"><origin xyz="%g %g %g"/><geometry><mesh filename="objs/{name}.obj"/>'
                '</geometry></visual></link>') % tuple(origin)

    hinge = (-0.4, -0.5, 0.0)  # the door's hinge line, body frame; its mesh is shifted back by the visual origin
    urdf = ('<?xml version="1.0"?><robot name="boxes"><link name="base"/>' + link("link_body")
            + link("link_door", [-h for h in hinge]) + link("link_handle", [-h for h in hinge]) + link("link_drawer")
            + joint("joint_base", "fixed", "base", "link_body", off, (0, 0, yaw))
            + joint("joint_door", "revolute", "link_body", "link_door", hinge, axis=(0, 0, 1), limit=(0, 1.5))
            + joint("joint_handle", "fixed", "link_door", "link_handle")
            + joint("joint_drawer", "prismatic", "link_body", "link_drawer", axis=(-1, 0, 0), limit=(0, 0.3)) + '</robot>')
    (root / "mobility_annotation_gapartnet.urdf").write_text(urdf)
    anno = []
    for name, (lo, hi, cat) in PARTS.items():
        world = (np.array(_corners(lo, hi)) @ Rb.T + off).tolist()
        anno.append(dict(link_name=name, is_gapart=cat is not None, category=cat or "", bbox=world if cat else []))
    anno.append(dict(link_name="link_body", is_gapart=True, category="not_a_gapart_class", bbox=_corners(*PARTS["link_body"][:2])))
    (root / "link_annotation_gapartnet.json").write_text(json.dumps(anno))
    return RA.load_asset(str(root))


def _world_vertices(asset, qpos, link):
    poses = RA.link_poses(asset, qpos)
    pts = []
    for vi in np.nonzero(asset.visual_link == asset.links.index(link))[0]:
        v = asset.verts[np.unique(asset.tris[asset.tri_visual == vi])].astype(np.float64)
        m = poses[link] @ asset.visual_origin[vi]
        pts.append(v @ m[:3, :3].T + m[:3, 3])
    return np.concatenate(pts)


def _inside(points, bbox, tol=1e-6):
    """points inside the oriented box given by the annotation's corner order"""
    bbox = np.asarray(bbox, np.float64)
    centre = bbox.mean(0)
    for a, b in ((1, 0), (1, 2), (0, 4)):
        ax = bbox[a] - bbox[b]
        half = np.linalg.norm(ax) / 2
        if (np.abs((points - centre) @ (ax / np.linalg.norm(ax))) > half + tol).any():
            return False
    return True


@pytest.mark.parametrize("qpos", [dict(joint_door=0.0, joint_drawer=0.0), dict(joint_door=1.1, joint_drawer=0.25)])
def test_forward_kinematics_and_box_articulation_agree(box_asset, qpos):
    qpos = dict(joint_base=0.0, joint_handle=0.0, **qpos)
    assert list(box_asset.targets) == ["link_door", "link_handle", "link_drawer"]
    assert box_asset.tris.shape == (4 * 12, 3)  # quads are fanned into two triangles
    assert np.allclose(box_asset.tri_color[:12], [0.9, 0.5, 0.1]) and np.allclose(box_asset.tri_color[12:], RA.DEFAULT_GREY)
    boxes = RA.part_boxes(box_asset, qpos)
    for link in box_asset.targets:
        pts = _world_vertices(box_asset, qpos, link)
        assert _inside(pts, boxes[link]["bbox"]), link
        # and the box is no larger than the part: every corner is a mesh vertex
        d = np.linalg.norm(boxes[link]["bbox"][:, None, :] - pts[None], axis=-1).min(1)
        assert d.max() < 1e-6, link
    # projected box corners bracket the part's pixels
    cam = np.array([1.5, -3.2, 1.5])
    H, W = 48, 64
    view, = RA.render_views([box_asset], [RA.RenderRequest(0, qpos, cam)], H, W, device="cpu")
    K, R, t = RA.camera_frame(cam, H, W)
    assert len(view.bbox_pose_dict) == 3 and view.counters["near"] == 0 and view.counters["index"] == 0
    assert (view.sem == -1).any() and (view.sem == -2).any()  # the body is "others", the rest is background
    for link, entry in view.bbox_pose_dict.items():
        pc = (entry["bbox"] - t) @ R
        u, v = K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2]
        ys, xs = np.nonzero(view.ins == entry["instance_id"])
        assert len(ys) > 0
        assert u.min() - 1 <= xs.min() and xs.max() <= u.max() + 1 and v.min() - 1 <= ys.min() and ys.max() <= v.max() + 1, link
        assert np.abs(view.npcs[ys, xs]).max() <= 0.5 + 1e-3
        assert (view.sem[ys, xs] == entry["category_id"]).all()


def test_obj_reader_edge_cases(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("mtllib gone.mtl\nusemtl nothing\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvn 0 0 1\n"
                 "f 1//1 2//1 3//1 4//1\n"       # a quad in a//c form
                 "f -5/1/1 -4/2/1 -1/3/1\n"      # negative indices, a/b/c form
                 "f 1 2 3 4 5\n")                # a pentagon: three triangles in a fan
    v, t, c = RA.read_obj(str(p))
    assert v.shape == (5, 3) and v.dtype == np.float32
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    assert np.allclose(c, RA.DEFAULT_GREY) and c.shape == (6, 3)  # the mtl file is missing: grey
    (tmp_path / "bad.obj").write_text("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        RA.read_obj(str(tmp_path / "bad.obj"))


def test_cli_end_to_end_on_the_cpu(tmp_path):
    data = tmp_path / "data"
    os.makedirs(data)
    os.symlink(RR.fixture_asset(), data / "45780")
    (tmp_path / "ids.txt").write_text("Box 100\nStorageFurniture 45780\n")
    ranges = {"StorageFurniture": [dict(zip(RANGE_KEYS, (40.0, 70.0, 150.0, 210.0, 3.6, 4.2))),
                                   dict(zip(RANGE_KEYS, (40.0, 70.0, -30.0, 30.0, 3.6, 4.2)))]}
    (tmp_path / "ranges.json").write_text(json.dumps(ranges))
    out = tmp_path / "out"
    args = ["--dataset", "partnet", "--data_path", str(data), "--id_list", str(tmp_path / "ids.txt"), "--model_ids", "45780",
            "--views", "2", "--height", "40", "--width", "40", "--batch", "3", "--seed", "5", "--save_path", str(out), "--device", "cpu"]
    assert RA.main(args + ["--camera_ranges", str(tmp_path / "ranges.json")]) == 0
    names = sorted(f[:-5] for f in os.listdir(out / "metafile"))
    assert names == [f"StorageFurniture_45780_{c}_{r}" for c in (0, 1) for r in (0, 1)]
    from gapartnet_amd.dataset.convert_rendered import read_view
    front = read_view(str(out), names[0])
    assert front["depth"].shape == (40, 40) and (front["sem"] >= 0).any() and (front["sem"] == -2).any()
    with open(out / "metafile" / f"{names[2]}.json") as fd:
        meta = json.load(fd)
    assert meta["camera_idx"] == 1 and meta["model_id"] == 45780 and meta["camera_pos"][0] > 0  # the second range: from behind
    # the same seed gives the same files; without the ranges file the built-in range applies
    out2 = tmp_path / "out2"
    assert RA.main(args[:-4] + ["--save_path", str(out2), "--device", "cpu", "--camera_ranges", str(tmp_path / "ranges.json")]) == 0
    for n in names:
        assert np.array_equal(read_view(str(out2), n)["depth"], read_view(str(out), n)["depth"])
    out3 = tmp_path / "out3"
    assert RA.main(args[:-4] + ["--save_path", str(out3), "--device", "cpu"]) == 0
    assert sorted(os.listdir(out3 / "depth")) == ["StorageFurniture_45780_0_0.npz", "StorageFurniture_45780_0_1.npz"]
    with pytest.raises(ValueError):
        RA.main(args[:7] + ["7"] + args[8:])


def test_cli_batches_hold_only_the_assets_they_show(tmp_path, monkeypatch):
    """three models, batches of two views: every batch's geometry tables hold the assets of its own views, and the files are
    those of a run that renders one view at a time"""
    data = tmp_path / "data"
    os.makedirs(data)
    for mid in (1, 2, 3):
        os.symlink(RR.fixture_asset(), data / str(mid))
    (tmp_path / "ids.txt").write_text("Safe 1\nSafe 2\nOven 3\n")
    seen = []
    real = RA.render_views
    monkeypatch.setattr(RA, "render_views", lambda assets, reqs, *a, **k: seen.append((len(assets), len(reqs))) or real(assets, reqs, *a, **k))
    for out, batch in (("a", 2), ("b", 1)):
        RA.render_dataset("partnet", str(data), str(tmp_path / "ids.txt"), [1, 2, 3], 1, str(tmp_path / out), None, 32, 32, batch, 3,
                          "cpu", echo=False)
    assert seen == [(2, 2), (1, 1), (1, 1), (1, 1), (1, 1)]
    from gapartnet_amd.dataset.convert_rendered import read_view
    for name in ("Safe_1_0_0", "Safe_2_0_0", "Oven_3_0_0"):
        a, b = read_view(str(tmp_path / "a"), name), read_view(str(tmp_path / "b"), name)
        assert all(np.array_equal(a[k], b[k]) for k in a), name


def test_c_abi_symbols_and_argument_checks():
    from gapartnet_amd import _C
    lib = _C.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    i, st = ctypes.c_int, ctypes.c_size_t
    assert lib.gpn_render_max_links() == 1024
    assert lib.gpn_render_ws_bytes(i(0), i(100)) == 0 and lib.gpn_render_ws_bytes(i(2), i(0)) == 0
    assert lib.gpn_render_ws_bytes(i(2), i(100)) >= 2 * 100 * 72
    args = (None, i(0), None, None, i(0), None, i(0), None, None, None, i(0))
    rc = lib.gpn_render_setup(*args, i(1), i(0), i(8), i(0), None, st(0), None, None)
    assert rc == 1 and b"bad argument" in lib.gpn_last_error()  # H = 0
    rc = lib.gpn_render_setup(*args, i(1), i(8), i(8), i(5), None, st(0), None, None)
    assert rc == 1 and b"Nt_max <= Nt" in lib.gpn_last_error()
    rc = lib.gpn_render_raster(None, i(0), None, i(0), i(1), i(8), i(20000), i(0), None, st(0), None, None, None)
    assert rc == 1 and b"16384" in lib.gpn_last_error()
    assert lib.gpn_render_raster(None, i(0), None, i(0), i(0), i(8), i(8), i(0), None, st(0), None, None, None) == 0  # V = 0
    assert lib.gpn_render_setup(*args, i(0), i(8), i(8), i(0), None, st(0), None, None) == 0
