"""Generates tests/golden/frames_backproject.npz: the reference's OWN back-projection and box drawing
(structure/utils.py: get_point_cloud :454-476, draw_bbox :55-90), run unmodified on two small frames with zero-depth holes and a
non-square camera, and on two boxes.

    python tests/golden/make_golden_frames.py REFERENCE_ROOT        (build container only: needs the reference tree)

How the reference runs here: ``cv2`` is a stub whose ``line`` records its arguments (every other attribute is 0), and a module the
reference imports at its top without using it in these two functions is an empty stub when it is not installed.  Depths are
float32 values, as a depth camera's driver hands them over.  Stored: inputs and recorded results.  No reference text is stored.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FRAMES = (("a", 1, 6, 7), ("b", 2, 5, 9))   # (name, seed, H, W)
LINES = []


def make_frame(seed, H, W):
    rng = np.random.RandomState(seed)
    depth = (0.4 + rng.rand(H, W) * 2.5).astype(np.float32)
    depth[rng.rand(H, W) < 0.3] = 0
    depth[0, 0] = 0          # a hole in a corner ...
    depth[H - 1, W - 1] = np.float32(1.75)  # ... and a point in the opposite one
    rgb = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    K = np.array([[W * 1.37, 0.0, W / 2 - 0.3], [0.0, W * 1.61, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    return depth, rgb, K


def make_boxes():
    """two boxes in front of a 64 x 48 camera: unit cube corners in the reference's corner order, scaled, turned and moved"""
    corners = np.array([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [1, 1, 1]], np.float64)
    out = []
    for k, (s, ang, t) in enumerate(((0.30, 0.4, (0.1, -0.05, 2.0)), (0.22, -0.9, (-0.35, 0.2, 1.6)))):
        c, sn = np.cos(ang), np.sin(ang)
        R = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]]) @ np.array([[1, 0, 0], [0, c, -sn], [0, sn, c]])
        out.append((corners * s) @ R.T + np.asarray(t))
    return np.stack(out)


def load_reference(ref_root):
    path = os.path.join(ref_root, "structure", "utils.py")
    assert os.path.isfile(path), "reference tree not given: the fixture can only be regenerated in the build container"
    def absent(attr):  # (dunder lookups of importlib / inspect must fail as on any module)
        if attr.startswith("__"):
            raise AttributeError(attr)
        return 0

    cv2 = types.ModuleType("cv2")
    cv2.__getattr__ = absent
    cv2.line = lambda img, a, b, color=None, thickness=None: LINES.append((list(a), list(b), list(color), int(thickness)))
    sys.modules["cv2"] = cv2
    for name in ("glob", "einops", "sklearn", "sklearn.neighbors", "scipy", "scipy.spatial", "scipy.spatial.transform", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:
            stub = types.ModuleType(name)
            stub.__getattr__ = absent
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_structure_utils", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAPARTNET_REFERENCE", ""))
    out = {"names": np.asarray([f[0] for f in FRAMES])}
    for name, seed, H, W in FRAMES:
        depth, rgb, K = make_frame(seed, H, W)
        zeros = np.zeros((H, W), np.int64)
        pc, col, _, _, idx = ref.get_point_cloud(rgb, depth, zeros, zeros, K)
        out[f"{name}/depth"], out[f"{name}/rgb"], out[f"{name}/K"] = depth, rgb, K
        out[f"{name}/xyz"] = np.asarray(pc, dtype=np.float64)       # [H*W, 3], every pixel (the caller filters depth != 0)
        out[f"{name}/colour"] = np.asarray(col, dtype=np.float64)   # [H*W, 3]
        out[f"{name}/pixel"] = np.asarray(idx, dtype=np.int64)      # [H*W, 2] = (y, x)
    boxes = make_boxes()
    K = np.array([[70.5, 0.0, 31.25], [0.0, 66.0, 24.5], [0.0, 0.0, 1.0]])
    img = np.zeros((48, 64, 3), np.uint8)
    del LINES[:]
    ref.draw_bbox(img, list(boxes), K=K)
    out["boxes"], out["boxes_K"], out["boxes_hw"] = boxes, K, np.asarray([48, 64])
    out["line_a"] = np.asarray([l[0] for l in LINES], dtype=np.int64)          # [30, 2] = (x, y)
    out["line_b"] = np.asarray([l[1] for l in LINES], dtype=np.int64)
    out["line_bgr"] = np.asarray([l[2] for l in LINES], dtype=np.int64)        # the colour as cv2 takes it (BGR)
    out["line_thickness"] = np.asarray([l[3] for l in LINES], dtype=np.int64)
    dst = os.path.join(HERE, "frames_backproject.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes;", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
