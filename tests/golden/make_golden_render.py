"""Generates tests/golden/render_asset.npz: what the reference's OWN render_tools functions compute for asset 45780
(tests/golden/assets/45780.zip), run unmodified.

    python tests/golden/make_golden_render.py        (build container only: needs the reference tree)

Run from the reference: read_joints_from_urdf_file; get_cam_pos under np.random.seed (after the joint draws of render.py's step 3,
made here in its order with np.random.uniform); query_part_pose_from_joint_qpos; compute_rotation_matrix and
get_NPCS_map_from_oriented_bbox on the 48 x 64 depth and instance maps that tests/render_ref.py renders; save_rgb_image,
save_depth_map, save_anno_dict and save_meta, of whose files the member names, dtypes, shapes, pickle structure and JSON key order
are recorded.

``sapien`` and ``transforms3d`` are absent here.  Both are stubbed: ``sapien.core`` is an empty module with the two class names the
reference's annotations mention; ``transforms3d.euler.axangle2mat`` is a Rodrigues rotation written here; the ``robot`` handed to
query_part_pose_from_joint_qpos is a stand-in whose joints report the parent link poses of OUR forward kinematics
(render_assets.link_poses) and a joint frame whose x axis is the URDF axis, which is SAPIEN's convention.  So the fixture pins the
reference's box articulation, NPCS frames, draw order and file layout - not SAPIEN's kinematics, which the generated-asset test of
tests/test_render_cpu.py ties to the boxes instead.
Stored: arrays and names only.  No reference text is stored.
"""
import json
import math
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/dataset/render_tools"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gapartnet_amd.dataset import render_assets as RA  # noqa: E402
from tests import render_ref  # noqa: E402

ASSET = render_ref.fixture_asset()
SEED = 20240
H, W = 48, 64
CAMERA_RANGE = dict(theta_min=40.0, theta_max=70.0, phi_min=150.0, phi_max=210.0, distance_min=3.6, distance_max=4.2)


def axangle2mat(axis, angle, is_normalized=False):
    x, y, z = axis
    if not is_normalized:
        n = math.sqrt(x * x + y * y + z * z)
        x, y, z = x / n, y / n, z / n
    c, s = math.cos(angle), math.sin(angle)
    C = 1 - c
    return np.array([[x * x * C + c, x * y * C - z * s, z * x * C + y * s], [x * y * C + z * s, y * y * C + c, y * z * C - x * s],
                     [z * x * C - y * s, y * z * C + x * s, z * z * C + c]])


class Pose:
    def __init__(self, m):
        self.m = np.asarray(m, np.float64)

    @property
    def p(self):
        return self.m[:3, 3].copy()

    def to_transformation_matrix(self):
        return self.m.copy()

    def __mul__(self, other):
        return Pose(self.m @ other.m)


def x_to(axis):
    """a rotation whose first column is the unit axis"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.eye(3)[int(np.argmin(np.abs(a)))]
    b = np.cross(a, h)
    b /= np.linalg.norm(b)
    return np.stack([a, b, np.cross(a, b)], axis=1)


class Robot:
    def __init__(self, asset, qpos):
        poses = RA.link_poses(asset, qpos)
        self.joints = []
        for name, j in asset.joints.items():
            frame = RA._pose(j['xyz'], j['rpy'])
            if j['axis'] is not None:
                frame[:3, :3] = frame[:3, :3] @ x_to(j['axis'])
            link = types.SimpleNamespace(pose=Pose(poses[j['parent']]))
            self.joints.append(types.SimpleNamespace(get_name=lambda n=name: n, get_parent_link=lambda l=link: l,
                                                     get_pose_in_parent=lambda f=frame: Pose(f)))

    def get_joints(self):
        return self.joints


def main():
    assert os.path.isdir(REF), "reference tree not present: the fixture can only be regenerated in the build container"
    core = types.ModuleType("sapien.core")
    core.KinematicArticulation = core.Scene = object
    sapien = types.ModuleType("sapien")
    sapien.core = core
    t3 = types.ModuleType("transforms3d")
    t3.euler = types.ModuleType("transforms3d.euler")
    t3.axangles = types.ModuleType("transforms3d.axangles")
    t3.euler.axangle2mat = t3.axangles.axangle2mat = axangle2mat
    sys.modules.update({"sapien": sapien, "sapien.core": core, "transforms3d": t3, "transforms3d.euler": t3.euler,
                        "transforms3d.axangles": t3.axangles})
    sys.path.insert(0, REF)
    from utils import pose_utils, read_utils, render_utils
    from utils.config_utils import TARGET_GAPARTS

    out = {"seed": np.int64(SEED), "H": np.int64(H), "W": np.int64(W),
           "camera_range": np.array([CAMERA_RANGE[k] for k in ("theta_min", "theta_max", "phi_min", "phi_max", "distance_min",
                                                              "distance_max")]),
           "target_gaparts": np.asarray(TARGET_GAPARTS)}
    # 1. joints
    joints = read_utils.read_joints_from_urdf_file(ASSET, "mobility_annotation_gapartnet.urdf")
    names = list(joints)
    out["joint_names"] = np.asarray(names)
    for k in ("type", "parent", "child"):
        out[f"joint_{k}"] = np.asarray([joints[n][k] for n in names])
    out["joint_xyz"] = np.array([joints[n]["xyz"] for n in names], np.float64)
    out["joint_rpy"] = np.array([joints[n]["rpy"] for n in names], np.float64)
    out["joint_axis"] = np.array([joints[n]["axis"] or [np.nan] * 3 for n in names], np.float64)
    out["joint_limit"] = np.array([joints[n]["limit"] or [np.nan] * 2 for n in names], np.float64)
    # 2. draw order: joints in dictionary order, then the camera
    np.random.seed(SEED)
    qpos = {}
    for n in names:
        jt = joints[n]["type"]
        if jt in ("prismatic", "revolute"):
            qpos[n] = np.random.uniform(joints[n]["limit"][0], joints[n]["limit"][1])
        elif jt == "fixed":
            qpos[n] = 0.0
        else:
            qpos[n] = np.random.uniform(-10000.0, 10000.0)
    cam_pos = render_utils.get_cam_pos(theta_min=CAMERA_RANGE["theta_min"], theta_max=CAMERA_RANGE["theta_max"],
                                       phi_min=CAMERA_RANGE["phi_min"], phi_max=CAMERA_RANGE["phi_max"],
                                       dis_min=CAMERA_RANGE["distance_min"], dis_max=CAMERA_RANGE["distance_max"])
    out["qpos"] = np.array([qpos[n] for n in names], np.float64)
    out["camera_pos"] = cam_pos
    # 3. part boxes
    asset = RA.load_asset(ASSET)
    poses = pose_utils.query_part_pose_from_joint_qpos(data_path=ASSET, anno_file="link_annotation_gapartnet.json", joint_qpos=qpos,
                                                       joints_dict=joints, target_parts=TARGET_GAPARTS, base_link_name="base",
                                                       robot=Robot(asset, qpos))
    links = list(poses)
    out["box_links"] = np.asarray(links)
    out["box_category"] = np.array([poses[n]["category_id"] for n in links], np.int64)
    out["boxes"] = np.array([poses[n]["bbox"] for n in links], np.float64)
    out["box_dtypes"] = np.asarray([str(poses[n]["bbox"].dtype) for n in links])
    # 4. NPCS frames and map on the restatement's depth and instance maps
    K, R, t = RA.camera_frame(cam_pos, H, W)
    g = RA.geometry_tables([asset])
    tables, _ = RA.view_tables([asset], [RA.RenderRequest(0, qpos, cam_pos)], H, W)
    img = render_ref.render(g, dict(tables, background=RA.BACKGROUND_RGB))
    depth, ins, sem = img["depth"][0], img["ins"][0], img["sem"][0]
    link_inst = img["link_inst"][0]
    name_to_id = {n: int(link_inst[asset.links.index(n)]) for n in links if link_inst[asset.links.index(n)] >= 0}
    rts, npcs = pose_utils.get_NPCS_map_from_oriented_bbox(depth, ins, name_to_id, {n: poses[n] for n in name_to_id}, K, R, t)
    out.update(K=K, R=R, t=t, depth=depth, ins=ins, sem=sem, npcs=npcs, valid_links=np.asarray(list(name_to_id)),
               valid_ids=np.array(list(name_to_id.values()), np.int64))
    for k in ("R", "T", "S"):
        out[f"rts_{k}"] = np.array([rts[n][k] for n in name_to_id], np.float64)
    out["rts_scaler"] = np.array([rts[n]["scaler"] for n in name_to_id], np.float64)
    b = poses[links[0]]["bbox"]
    out["rotation_probe"] = pose_utils.compute_rotation_matrix(b - b.mean(0), (b - b.mean(0)) @ axangle2mat([1, 2, 3], 0.7).T)
    # 5. the files
    with tempfile.TemporaryDirectory() as tmp:
        name = "StorageFurniture_45780_0_0"
        read_utils.save_rgb_image(img["rgb"][0], tmp, name)
        read_utils.save_depth_map(depth, tmp, name)
        bbox_pose = {n: {"bbox": poses[n]["bbox"], "category_id": poses[n]["category_id"], "instance_id": name_to_id[n],
                         "pose_RTS_param": rts[n]} for n in name_to_id}
        read_utils.save_anno_dict({"semantic_segmentation": sem, "instance_segmentation": ins, "npcs_map": npcs,
                                   "bbox_pose_dict": bbox_pose}, tmp, name)
        meta = {"model_id": 45780, "category": "StorageFurniture", "camera_idx": 0, "render_idx": 0, "width": W, "height": H,
                "joint_qpos": qpos, "camera_pos": cam_pos.reshape(-1).tolist(), "camera_intrinsic": K.reshape(-1).tolist(),
                "world2camera_rotation": R.reshape(-1).tolist(), "camera2world_translation": t.reshape(-1).tolist(),
                "target_gaparts": TARGET_GAPARTS, "use_raytracing": False, "replace_texture": False}
        read_utils.save_meta(meta, tmp, name)
        files, members = [], []
        for sub in sorted(os.listdir(tmp)):
            for fn in sorted(os.listdir(os.path.join(tmp, sub))):
                files.append(f"{sub}/{fn}")
                if fn.endswith(".npz"):
                    z = np.load(os.path.join(tmp, sub, fn))
                    members += [f"{sub}:{k}:{z[k].dtype}:{'x'.join(str(s) for s in z[k].shape)}" for k in z.files]
        out["files"], out["npz_members"] = np.asarray(files), np.asarray(members)
        from PIL import Image
        im = Image.open(os.path.join(tmp, "rgb", name + ".png"))
        out["png"] = np.asarray([im.mode, f"{im.size[0]}x{im.size[1]}"])
        with open(os.path.join(tmp, "bbox", name + ".pkl"), "rb") as fd:
            pk = pickle.load(fd)
        first = pk["bbox_pose_dict"][list(name_to_id)[0]]
        out["pkl_top_keys"] = np.asarray(list(pk))
        out["pkl_links"] = np.asarray(list(pk["bbox_pose_dict"]))
        out["pkl_entry_keys"] = np.asarray(list(first))
        out["pkl_rts_keys"] = np.asarray(list(first["pose_RTS_param"]))
        out["pkl_entry_types"] = np.asarray([type(first[k]).__name__ for k in first])
        with open(os.path.join(tmp, "metafile", name + ".json")) as fd:
            out["meta_keys"] = np.asarray(list(json.load(fd)))
    path = os.path.join(HERE, "render_asset.npz")
    np.savez_compressed(path, **out)
    print("links with area:", name_to_id, f"{os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
