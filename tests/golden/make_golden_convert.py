"""Generates tests/golden/convert_views.npz: the reference's OWN conversion of rendered views into training scenes
(dataset/process_tools/convert_rendered_into_input.py), run unmodified on small synthetic views (tests/render_views.py).

    python tests/golden/make_golden_convert.py        (build container only: needs the reference tree)

How the reference runs here: ``open3d`` (imported, only used with --visualize) is an empty stub; utils/sample_utils.py takes its
CUDA branch (``CUDA = True``) with ``futils.furthest_point_sample`` backed by oracle.pn2_furthest_point_sampling, the CPU
restatement of the vendored CUDA kernel (start index 0).  ``sample_and_save`` is called on every view, and the driver is run as
a script (runpy, ``run_name='__main__'``) with its own arguments in a temporary working directory, which pins the name sorting,
the category grouping and log_sample.txt.  One name matches no category and one view has too few pixels.
Stored: the views' inputs, the files both runs wrote (the two must agree), the log.  No reference text is stored.
"""
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/dataset/process_tools"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import render_views  # noqa: E402

NUM_POINTS = 512
VIEWS = (  # (name, kind, seed)
    ("Box_0001_00_000", "plain", 1),
    ("Box_0002_00_001", "exact", 2),
    ("Camera_0003_00_000", "holes", 3),
    ("Safe_0004_00_000", "ties", 4),
    ("Table_0005_00_000", "too_few", 5),
    ("Zebra_0006_00_000", "plain", 6),
)


def _files(save, name):
    out = {}
    pth = os.path.join(save, "pth", name + ".pth")
    if not os.path.exists(pth):
        return None
    arrays = torch.load(pth, weights_only=False)
    for i, a in enumerate(arrays):
        out[f"pth{i}"] = np.asarray(a)
    for sub in ("meta", "gt"):
        with open(os.path.join(save, sub, name + ".txt"), "rb") as fh:
            out[sub] = np.frombuffer(fh.read(), dtype=np.uint8)
    return out


def main():
    assert os.path.isdir(REF), "reference tree not present: the fixture can only be regenerated in the build container"
    from oracle import pn2_furthest_point_sampling
    sys.modules["open3d"] = types.ModuleType("open3d")
    sys.path.insert(0, REF)
    import utils.sample_utils as su

    def furthest_point_sample(xyz, npoint):
        return torch.from_numpy(pn2_furthest_point_sampling(xyz.detach().cpu().numpy(), int(npoint)))
    su.CUDA = True
    su.futils = types.SimpleNamespace(furthest_point_sample=furthest_point_sample)
    import convert_rendered_into_input as ref

    out = {"num_points": np.int64(NUM_POINTS), "names": np.asarray([n for n, _, _ in VIEWS])}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "rendered")
        for name, kind, seed in VIEWS:
            v = render_views.make_view(kind, num_points=NUM_POINTS, seed=seed)
            render_views.write_view(data, name, v)
            for k in ("rgb", "depth", "sem", "ins", "npcs", "K"):
                out[f"{name}/in_{k}"] = v[k]
        direct = os.path.join(tmp, "direct")
        for name, _, _ in VIEWS:
            out[f"{name}/ret"] = np.int64(ref.sample_and_save(name, data, direct, NUM_POINTS))
        run = os.path.join(tmp, "run")
        os.makedirs(run)
        saved_argv = sys.argv
        try:
            os.chdir(run)
            sys.argv = ["convert_rendered_into_input.py", "--dataset", "partnet", "--data_path", data, "--save_path",
                        os.path.join(run, "sampled"), "--num_points", str(NUM_POINTS)]
            runpy.run_path(os.path.join(REF, "convert_rendered_into_input.py"), run_name="__main__")
        finally:
            sys.argv = saved_argv
            os.chdir(cwd)
        with open(os.path.join(run, "log_sample.txt"), "rb") as fh:
            out["log"] = np.frombuffer(fh.read(), dtype=np.uint8)
        written = []
        for name, _, _ in VIEWS:
            a, b = _files(direct, name), _files(os.path.join(run, "sampled"), name)
            if b is None:
                continue
            written.append(name)
            assert a is not None and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), name
            for k, v in b.items():
                out[f"{name}/out_{k}"] = v
        out["written"] = np.asarray(written)
    path = os.path.join(HERE, "convert_views.npz")
    np.savez_compressed(path, **out)
    print("written by the driver:", written, f"{os.path.getsize(path) / 1e6:.2f} MB")
    print(bytes(out["log"]).decode())


if __name__ == "__main__":
    main()
