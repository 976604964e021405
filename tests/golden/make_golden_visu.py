"""Generates tests/golden/visu_panels.npz: what the reference's ``misc/visu.py visualize_gapartnet`` - run UNMODIFIED with
``save_detail=True`` - produces for two small synthetic scenes, plus its inputs and the constants it reads.

    python tests/golden/make_golden_visu.py        (build container only: needs the reference tree)

The reference needs ``cv2``, which is absent; its stand-in here does the bookkeeping only:
  cvtColor   channel reversal              imwrite   captures the array under the file's name
  imread     returns the stored raw image  putText   records (text, anchor)
  line       records (image, a, b, colour, thickness) WITHOUT drawing: OpenCV's line pixels are not pinned, its calls are
``np.random.randint`` and the pose fit are wrapped to record every draw and every fitted box.  The arrays the reference hands to
``imwrite`` are BGR; the fixture stores them as the written file shows them (channels reversed once more), and line colours
likewise.  Only inputs, recorded outputs and recorded constants are written; no reference source text goes anywhere.

What the scenes contain (tests/test_visu_cpu.py relies on it): two points on one pixel, overlapping 2 x 2 splats, projections that
land exactly on .5 (half to even), one at about -0.0015 (rounds to -0 and is kept), rows / columns H-2 (kept) and H-1 (dropped),
z = 0 and z < 0, colours with fractional parts, labels >= 20 for the modulo rules, -100 instance labels, an instance of 4 points
(no box).  Every colour source stays inside [0, 255.99] / 255, where the reference's cast is defined.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden.make_golden_pipeline import REF, install_reference_environment  # noqa: E402

OPTIONS = ["raw", "pc", "sem_pred", "ins_pred", "npcs_pred", "bbox_pred", "bbox_pred_pure", "sem_gt", "ins_gt", "npcs_gt", "bbox_gt",
           "bbox_gt_pure"]
FILE_OF = {"bbox_pred_pure": "bbox_pure"}   # the reference's file name of that tile
F = 1268.637939453125
SCENES = (("Box_visu_00_000", (2.0, 0.25, -0.5, 1.0)),                       # exactly representable: the special points below
          ("Door_visu_01_000", (0.7312459, 0.0131, -0.0217, 1.6108)))        # like a meta file


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _instance(rng, n, centre, scale):
    """n points of a part whose NPCS is exact: xyz = scale * npcs @ R + centre"""
    npcs = rng.uniform(-0.45, 0.45, (n, 3))
    return scale * npcs @ _rotation(rng) + centre, npcs


def _special_points(trans):
    """normalised-frame points whose camera-frame position is chosen: with z_cam = F the projection is x_cam + 400 exactly"""
    r, c = trans[0], np.asarray(trans[1:4])
    cam = []
    for u, v in ((100, 100), (100, 100), (101, 100), (100, 101),            # one pixel twice; overlapping splats
                 (410.5, 200), (411.5, 200), (300, 250.5), (300, 251.5),     # .5: half to even
                 (-0.0015, 300), (310, -0.0015),                             # rounds to -0: kept
                 (798, 320), (799, 320), (330, 798), (330, 799),             # H-2 / W-2 kept, H-1 / W-1 dropped
                 (-1, 340), (350, -1), (800, 360)):
        cam.append((u - 400.0, v - 400.0, F))
    cam += [(0.05, -0.02, 0.0), (0.0, 0.0, 0.0), (0.05, 0.07, -1.0), (-0.03, 0.02, -2.5)]   # z = 0 (inf, NaN), z < 0
    return ((np.asarray(cam) - c) / r).astype(np.float32)


def make_scene(seed, trans):
    rng = np.random.default_rng(seed)
    r, c = trans[0], np.asarray(trans[1:4])
    parts, labels = [], []
    for ins, (n, centre, scale) in enumerate(((180, (-0.12, 0.05, 1.45), 0.22), (150, (0.16, -0.08, 1.7), 0.3))):
        cam_xyz, npcs = _instance(rng, n, np.asarray(centre), scale)
        parts.append(((cam_xyz - c) / r, npcs))
        labels.append(np.full(n, ins))
    cam_xyz, npcs = _instance(rng, 4, np.asarray((0.0, 0.2, 1.5)), 0.05)     # instance 25: four points, no box
    parts.append(((cam_xyz - c) / r, npcs))
    labels.append(np.full(4, 25))
    n_bg = 240
    bg = np.stack([rng.uniform(-0.35, 0.35, n_bg), rng.uniform(-0.35, 0.35, n_bg), rng.uniform(1.2, 2.0, n_bg)], 1)
    parts.append(((bg - c) / r, rng.uniform(-0.5, 0.49, (n_bg, 3))))
    labels.append(np.full(n_bg, -100))
    special = _special_points(trans)
    parts.append((special, rng.uniform(-0.5, 0.49, (special.shape[0], 3))))
    labels.append(np.full(special.shape[0], -100))
    xyz = np.concatenate([p[0] for p in parts]).astype(np.float32)
    npcs = np.concatenate([p[1] for p in parts]).astype(np.float32)
    ins = np.concatenate(labels).astype(np.int64)
    n = xyz.shape[0]
    perm = rng.permutation(n)                                                # the specials are not the last writers everywhere
    xyz, npcs, ins = xyz[perm], npcs[perm], ins[perm]
    rgb = rng.uniform(0.0, 0.999, (n, 3)).astype(np.float32)
    sem = np.where(ins >= 0, (ins % 7) + 3, 0).astype(np.int64)
    sem[rng.random(n) < 0.1] = 20
    sem_pred = rng.integers(0, 21, n).astype(np.int64)
    ins_pred = rng.integers(0, 24, n).astype(np.float32)                     # 20 .. 23: the % 20 rule
    npcs_pred = rng.uniform(0.0, 0.999, (n, 3)).astype(np.float32)
    # predicted boxes: anything in front of the camera (one reaches outside the tile, one is far outside)
    boxes = []
    signs = np.asarray([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [1, 1, 1]], float)
    for centre, half in (((-0.1, 0.05, 1.5), 0.1), ((0.15, -0.1, 1.7), 0.15), ((0.3, 0.3, 1.3), 0.2), ((3.0, -2.0, 1.2), 0.1)):
        cam_box = signs * half @ _rotation(rng) + np.asarray(centre)
        boxes.append(((cam_box - c) / r).tolist())
    return dict(xyz=xyz, rgb=rgb, sem_gt=sem, ins_gt=ins, npcs_gt=npcs, sem_pred=sem_pred, ins_pred=ins_pred, npcs_pred=npcs_pred,
                bbox_pred=np.asarray(boxes), trans=np.asarray(trans, dtype=np.float64))


def raw_image(seed, H, W):
    """a blocky image (compresses to nothing)"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, (H // 50, W // 50, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 50, 0), 50, 1))


class Cv2Recorder:
    def __init__(self, cv2):
        self.written, self.lines, self.texts, self.images, self.raw = {}, [], [], [], {}
        cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1])
        cv2.imwrite = self.imwrite
        cv2.imread = lambda path: self.raw[os.path.basename(path)].copy()
        cv2.putText = lambda img, text, org, *a, **k: self.texts.append((text, tuple(int(v) for v in org)))
        cv2.line = self.line

    def line(self, img, a, b, color=None, thickness=None):
        self.images.append(img)   # (kept alive: ids stay unique)
        self.lines.append((id(img), int(a[0]), int(a[1]), int(b[0]), int(b[1])) + tuple(int(v) for v in color) + (int(thickness),))

    def imwrite(self, path, img):
        self.images.append(img)
        self.written[os.path.splitext(os.path.basename(path))[0]] = (id(img), np.array(img))


def main():
    assert os.path.isdir(REF), "reference tree not present: fixtures can only be regenerated in the build container"
    install_reference_environment()
    import structure.point_cloud  # noqa: F401  (before misc.visu: its sys.path.append would resolve `structure` elsewhere)
    import dataset.gapartnet  # noqa: F401
    import cv2
    rec = Cv2Recorder(cv2)
    import misc.visu as ref_visu
    import misc.visu_util as ref_util
    H, W, EDGE = int(ref_util.HEIGHT), int(ref_util.WIDTH), int(ref_util.EDGE)
    out = {"COLOR20": np.asarray(ref_util.COLOR20, dtype=np.uint8), "HEIGHT": np.int64(H), "WIDTH": np.int64(W), "EDGE": np.int64(EDGE),
           "K": np.asarray(ref_util.K, dtype=np.float64), "options": np.asarray(OPTIONS), "names": np.asarray([n for n, _ in SCENES])}

    load = torch.load
    torch.load = lambda *a, **k: load(*a, **{**k, "weights_only": False})
    draws, fits = [], []
    randint = np.random.randint

    def recording_randint(*a, **k):
        res = randint(*a, **k)
        draws.append(np.asarray(res).copy())
        return res
    np.random.randint = recording_randint
    fit = ref_visu.estimate_pose_from_npcs

    def recording_fit(xyz, npcs):
        first = len(draws)
        res = fit(xyz, npcs)
        fits.append((xyz.shape[0], np.stack(draws[first:]), None if res[0] is None else np.asarray(res[0], dtype=np.float64)))
        return res
    ref_visu.estimate_pose_from_npcs = recording_fit

    with tempfile.TemporaryDirectory() as tmp:
        for split_dir in ("pth", "meta"):
            os.makedirs(os.path.join(tmp, "data", "val", split_dir))
        os.makedirs(os.path.join(tmp, "raw"))
        for s, (name, trans) in enumerate(SCENES):
            scene = make_scene(100 + s, trans)
            torch.save((scene["xyz"], scene["rgb"], scene["sem_gt"], scene["ins_gt"], scene["npcs_gt"]),
                       os.path.join(tmp, "data", "val", "pth", name + ".pth"))
            np.savetxt(os.path.join(tmp, "data", "val", "meta", name + ".txt"), scene["trans"])
            scene["trans"] = np.loadtxt(os.path.join(tmp, "data", "val", "meta", name + ".txt"))   # as the reader sees it
            raw = raw_image(200 + s, H, W)
            rec.raw[name + ".png"] = raw
            open(os.path.join(tmp, "raw", name + ".png"), "wb").close()   # (the reference only asks whether it exists)
            rec.written.clear(); rec.lines.clear(); rec.texts.clear(); fits.clear(); draws.clear()
            np.random.seed(7 + s)
            ref_visu.visualize_gapartnet(
                SAVE_ROOT=os.path.join(tmp, "out"), GAPARTNET_DATA_ROOT=os.path.join(tmp, "data"), RAW_IMG_ROOT=os.path.join(tmp, "raw"),
                save_option=list(OPTIONS), name=name, split="val", bboxes=scene["bbox_pred"].tolist(), sem_preds=scene["sem_pred"],
                ins_preds=scene["ins_pred"], npcs_preds=scene["npcs_pred"], save_detail=True)
            pre = f"s{s}_"
            for k, v in scene.items():
                out[pre + k] = v
            out[pre + "raw"] = np.ascontiguousarray(raw[..., ::-1])          # as an RGB reader sees the raw file
            id_to_tile = {}
            for opt in OPTIONS:
                img_id, arr = rec.written[FILE_OF.get(opt, opt)]
                id_to_tile[img_id] = opt
                out[pre + "tile_" + opt] = np.ascontiguousarray(arr[..., ::-1])
            out[pre + "canvas"] = np.ascontiguousarray(rec.written[name][1][..., ::-1])
            # line calls: (tile index in `options`, ax, ay, bx, by, colour as written (r, g, b), thickness)
            out[pre + "lines"] = np.asarray([(OPTIONS.index(id_to_tile[l[0]]),) + l[1:5] + (l[7], l[6], l[5]) + (l[8],)
                                             for l in rec.lines], dtype=np.int64)
            out[pre + "texts"] = np.asarray([t for t, _ in rec.texts])
            out[pre + "text_anchor"] = np.asarray([o for _, o in rec.texts], dtype=np.int64)
            # the GT fits in call order (bbox_gt's instances, then bbox_gt_pure's): size, the draws consumed, the box
            out[pre + "fit_sizes"] = np.asarray([f[0] for f in fits], dtype=np.int64)
            out[pre + "fit_num_draws"] = np.asarray([f[1].shape[0] for f in fits], dtype=np.int64)
            out[pre + "fit_draws"] = np.concatenate([f[1] for f in fits]).astype(np.int64)
            out[pre + "fit_valid"] = np.asarray([f[2] is not None for f in fits])
            out[pre + "fit_bbox"] = np.stack([f[2] if f[2] is not None else np.full((8, 3), np.nan) for f in fits])
            print(name, "points", scene["xyz"].shape[0], "lines", len(rec.lines), "fits", [(f[0], f[1].shape[0]) for f in fits])
    path = os.path.join(HERE, "visu_panels.npz")
    np.savez_compressed(path, **out)
    print(f"visu_panels.npz: {len(out)} arrays, {os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
