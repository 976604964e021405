"""Generates tests/golden/cloud_ball_space.npz: the reference's OWN ball normalisation and OBJ reader
(gapartnet/tools/visu_utils.py: FindMaxDis / WorldSpaceToBallSpace :157-173, OBJfile2points :141-155), run unmodified on a few small
seeded clouds and one OBJ text with a ``vt`` tail.

    python tests/golden/make_golden_inference.py REFERENCE_ROOT        (build container only: needs the reference tree)

How the reference runs here: ``cv2`` (imported at the top of the module, not used by these functions) is a stub whose every attribute is 0.  The clouds
are float32 values held in float64 arrays, as the reference holds the points it parsed from a file: the float64 arithmetic then has
exactly the inputs the library's float32 clouds give it.  Stored: inputs and recorded results.  No reference text is stored.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CLOUDS = (  # (name, seed, points, kind)
    ("blob", 1, 40, "normal"),
    ("sheet", 2, 64, "plane"),      # zero extent along z
    ("far", 3, 33, "offset"),       # a camera-frame cloud metres away from the origin
    ("pair", 4, 2, "normal"),
    ("tiny", 5, 17, "small"),       # millimetre-sized
)

OBJ_TEXT = """# a header line
v 0.5 -0.25 1.0 0.1 0.2 0.3
v -1.5 2.0 0.125 1.0 0.0 0.5
v 0.1 0.2 0.3 0.4 0.5 0.6
vn 0.0 1.0 0.0
v 3.0 -4.0 5.0 0.25 0.75 1.0
vt 0.5 0.5
v 9.0 9.0 9.0 9.0 9.0 9.0
f 1 2 3
"""


def make_cloud(seed, n, kind):
    rng = np.random.RandomState(seed)
    xyz = rng.randn(n, 3)
    if kind == "plane":
        xyz[:, 2] = 0.75
    elif kind == "offset":
        xyz = xyz * 0.3 + np.array([0.4, -0.2, 4.2])
    elif kind == "small":
        xyz = xyz * 1e-3
    return xyz.astype(np.float32).astype(np.float64)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAPARTNET_REFERENCE", "")
    path = os.path.join(ref_root, "gapartnet", "tools", "visu_utils.py")
    assert os.path.isfile(path), "reference tree not given: the fixture can only be regenerated in the build container"
    if "cv2" not in sys.modules:  # (module-level constants of the reference read attributes of it)
        stub = types.ModuleType("cv2")
        stub.__getattr__ = lambda name: 0
        sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("ref_visu_utils", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    out = {"names": np.asarray([c[0] for c in CLOUDS])}
    for name, seed, n, kind in CLOUDS:
        xyz = make_cloud(seed, n, kind)
        out[f"{name}/in"] = xyz.copy()
        normalized, radius, center = ref.WorldSpaceToBallSpace(xyz)
        out[f"{name}/normalized"] = np.asarray(normalized, dtype=np.float64)
        out[f"{name}/radius"] = np.float64(radius)
        out[f"{name}/center"] = np.asarray(center, dtype=np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "scan.obj")
        with open(obj, "w") as fh:
            fh.write(OBJ_TEXT)
        out["obj_text"] = np.frombuffer(OBJ_TEXT.encode(), dtype=np.uint8)
        out["obj_points"] = np.asarray(ref.OBJfile2points(obj), dtype=np.float64)
    dst = os.path.join(HERE, "cloud_ball_space.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes;", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
