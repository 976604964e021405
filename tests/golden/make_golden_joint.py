"""Generates tests/golden/joint_axis.npz: the reference's OWN ``estimate_joint_angle`` (structure/gapartnet.py:819-963), run
unmodified on three small synthetic hinge pairs (a slab turned 20, 30 and 35 degrees about an edge, 1 mm noise, 300 to 600 points,
sample_number 64, 200 and 37).

    python tests/golden/make_golden_joint.py REFERENCE_ROOT        (build container only: needs the reference tree)

How the reference runs here: its two commented-out imports are injected - ``estimate_pose_from_npcs`` from the reference's own
gapartnet/misc/pose_fitting.py, ``RigidRegistration`` from tests/joint_ref.py (pycpd is not installed; the class records the X and
Y it is given) - ``cv2`` is a stub whose ``line`` records its arguments, and modules the reference imports at its top without using
them in this function are empty stubs when they are not installed.  Every pair runs twice with ``random.seed`` and
``np.random.seed`` fixed: ``visu=False`` returns the CPD leg; ``visu=True`` with options ("joint", "joint_ransac") returns the RANSAC
leg and draws both legs' lines.  ``np.random.randint`` is wrapped to record the RANSAC picks.  Stored: inputs, seeds and recorded
results.  No reference text is stored.
"""
import importlib
import importlib.util
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import joint_ref as JR  # noqa: E402

#        name, seed, degrees, n1, n2, sample_number
PAIRS = (("a", 1, 20.0, 300, 420, 64), ("b", 2, 30.0, 600, 512, 200), ("c", 3, 35.0, 333, 301, 37))
IMAGE_HW = (48, 64)
CAMERA = np.array([[70.5, 0.0, 31.25], [0.0, 66.0, 24.5], [0.0, 0.0, 1.0]])
LINES, SAMPLES, PICKS = [], [], []


class RecordingRegistration(JR.RigidRegistration):
    def __init__(self, X, Y, **kw):
        SAMPLES.append((np.array(X), np.array(Y)))
        super().__init__(X, Y, **kw)


def _stub(name):
    class Anything:
        """a value that can be called, indexed and read from"""
        def __call__(self, *a, **k):
            return self

        def __getattr__(self, attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return self

    def absent(attr):  # (dunder lookups of importlib / inspect must fail as on any module)
        if attr.startswith("__"):
            raise AttributeError(attr)
        return Anything()
    mod = types.ModuleType(name)
    mod.__getattr__ = absent
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def load_reference(ref_root):
    path = os.path.join(ref_root, "structure", "gapartnet.py")
    assert os.path.isfile(path), "reference tree not given: the fixture can only be regenerated in the build container"
    cv2 = _stub("cv2")
    cv2.line = lambda img, a, b, color=None, thickness=None: LINES.append(([int(v) for v in a], [int(v) for v in b],
                                                                             [int(v) for v in color], int(thickness)))
    sys.path.insert(0, ref_root)
    spec = importlib.util.spec_from_file_location("ref_pose_fitting", os.path.join(ref_root, "gapartnet", "misc", "pose_fitting.py"))
    pose = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pose)
    for _ in range(64):  # stub whatever is not installed, one module per attempt
        try:
            spec = importlib.util.spec_from_file_location("ref_structure_gapartnet", path)
            ref = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(ref)
            break
        except ModuleNotFoundError as e:
            _stub(e.name)
    ref.estimate_pose_from_npcs = pose.estimate_pose_from_npcs
    ref.RigidRegistration = RecordingRegistration
    return ref


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAPARTNET_REFERENCE", ""))
    real_randint = np.random.randint

    def recording_randint(n, size=None):
        got = real_randint(n, size=size)
        PICKS.append(np.array(got))
        return got
    out = {"names": np.asarray([p[0] for p in PAIRS]), "K": CAMERA, "image_hw": np.asarray(IMAGE_HW)}
    H, W = IMAGE_HW
    for name, seed, deg, n1, n2, k in PAIRS:
        pc1, pc2, (axis, point, angle) = JR.hinge_pair(seed, deg, n1, n2)
        objs = [types.SimpleNamespace(pcs_xyz=pc, pcs_rgb=np.zeros_like(pc), image=np.zeros((H, W, 3), np.uint8), K=CAMERA, name=name)
                for pc in (pc1, pc2)]
        legs = {}
        for visu in (False, True):
            random.seed(seed)
            np.random.seed(seed)
            del LINES[:], SAMPLES[:], PICKS[:]
            np.random.randint = recording_randint
            try:
                with tempfile.TemporaryDirectory() as tmp:
                    got = ref.estimate_joint_angle(objs[0], objs[1], visu=visu, visu_root=tmp, options=["joint", "joint_ransac"],
                                                   sample_number=k)
            finally:
                np.random.randint = real_randint
            legs[visu] = [np.asarray(v, dtype=np.float64) for v in got]
        assert len(LINES) == 2 and len(SAMPLES) == 1
        X, Y = SAMPLES[0]
        out[f"{name}/pc1"], out[f"{name}/pc2"] = pc1, pc2
        out[f"{name}/seed"], out[f"{name}/sample_number"] = np.asarray(seed), np.asarray(k)
        out[f"{name}/truth_axis"], out[f"{name}/truth_point"], out[f"{name}/truth_angle"] = axis, point, np.asarray(angle)
        out[f"{name}/X"], out[f"{name}/Y"] = X, Y
        out[f"{name}/ransac_picks"] = np.stack(PICKS).astype(np.int64)                       # [iterations run, 5]
        for leg, visu in (("cpd", False), ("ransac", True)):
            out[f"{name}/{leg}_axis"], out[f"{name}/{leg}_pivot"], out[f"{name}/{leg}_angle"] = legs[visu]
        # the lines as drawn: first the CPD leg ("joint"), then the RANSAC leg ("joint_ransac"); (x, y) endpoints
        out[f"{name}/line_a"] = np.asarray([l[0] for l in LINES], dtype=np.int64)
        out[f"{name}/line_b"] = np.asarray([l[1] for l in LINES], dtype=np.int64)
        out[f"{name}/line_colour"] = np.asarray([l[2] for l in LINES], dtype=np.int64)
        out[f"{name}/line_thickness"] = np.asarray([l[3] for l in LINES], dtype=np.int64)
    dst = os.path.join(HERE, "joint_axis.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes;", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
