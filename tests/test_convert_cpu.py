"""The rendered-views converter without a GPU: the numpy restatement (tests/convert_ref.py) against the reference's own run
(tests/golden/convert_views.npz), the new C entry points' declaration / registration / argument checks, and the CLI's directory
scan, category grouping, log lines and file writers reproducing the golden run from given per-view results."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import convert_ref as R
from tests import render_views as RV

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = ("rgb", "depth", "sem", "ins", "npcs", "K")
SYMBOLS = ("gpn_view_max_instance_ids", "gpn_view_backproject", "gpn_view_fps_ws_bytes", "gpn_view_fps", "gpn_view_finish")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "convert_views.npz"))


@pytest.fixture(scope="module")
def lib():
    from gapartnet_amd import _C
    if not os.path.exists(_C.SO_PATH):
        _C.build()
    return _C.lib()


def test_restatement_equals_the_reference_run(golden):
    m = int(golden["num_points"])
    relabelled = False
    for name in (str(n) for n in golden["names"]):
        v = {k: golden[f"{name}/in_{k}"] for k in KEYS}
        status, arrays, scale, gt = R.convert_view(*[v[k] for k in KEYS], m)
        assert (status == R.TOO_FEW) == (int(golden[f"{name}/ret"]) == -1), name
        if name not in set(golden["written"]):
            continue
        assert status == R.OK
        for i in range(6):
            want = golden[f"{name}/out_pth{i}"]
            assert arrays[i].dtype == want.dtype and np.array_equal(arrays[i], want), (name, i)
        assert R.meta_text(scale) == bytes(golden[f"{name}/out_meta"])
        assert R.gt_text(gt) == bytes(golden[f"{name}/out_gt"])
        raw = v["ins"][v["ins"] >= 0]
        relabelled |= int(arrays[3].max()) < int(raw.max())
    assert relabelled, "the fixture must exercise the relabel loop"


def test_fixture_covers_the_cases(golden):
    names = [str(n) for n in golden["names"]]
    assert any(int(golden[f"{n}/ret"]) == -1 for n in names)  # too few pixels
    assert "Zebra_0006_00_000" not in set(golden["written"])  # a name outside every category
    log = bytes(golden["log"]).decode()
    assert "Zebra" not in log and "num of points less than NUM_POINTS!" in log
    assert os.path.getsize(os.path.join(HERE, "golden", "convert_views.npz")) < 1 << 20


def test_opt_n_threads_host_formula_is_floor_log2():
    """viewprep.hip computes the reference's block size with integer ops; the host form is (int)(log(n) / log(2))"""
    for n in range(1, 1 << 21):
        assert int(math.log(n) / math.log(2)) == n.bit_length() - 1


def test_symbols_declared_registered_exported(lib):
    from tests.test_cabi import declared_symbols
    declared = set(declared_symbols())
    names = {lib.gpn_entry_point_name(i).decode() for i in range(lib.gpn_num_entry_points())}
    for s in SYMBOLS:
        assert s in declared and s in names and hasattr(lib, s), s
    assert lib.gpn_view_max_instance_ids() == 4096
    assert lib.gpn_view_fps_ws_bytes(ctypes.c_int(64)) > 0 and lib.gpn_view_fps_ws_bytes(ctypes.c_int(0)) == 0


def test_argument_errors_without_a_device(lib):
    i, vp = ctypes.c_int, ctypes.c_void_p
    rc = lib.gpn_view_backproject(None, i(2), None, None, None, i(1), i(8), i(8), None, None, None, None, None)
    assert rc == 1 and b"bad argument" in lib.gpn_last_error()
    rc = lib.gpn_view_backproject(None, i(4), None, None, None, i(1), i(8), i(8), None, None, None, None, None)
    assert rc == 1 and b"bad argument" in lib.gpn_last_error()
    rc = lib.gpn_view_fps(None, ctypes.c_int64(100), None, None, i(2), i(0), i(0), None, None, ctypes.c_size_t(0), None)
    assert rc == 1 and b"bad argument" in lib.gpn_last_error()
    rc = lib.gpn_view_fps(vp(16), ctypes.c_int64(100), vp(16), vp(16), i(2), i(10), i(0), vp(16), None, ctypes.c_size_t(0), None)
    assert rc == 2 and b"workspace" in lib.gpn_last_error()
    rc = lib.gpn_view_finish(None, i(4), None, None, None, None, None, i(1), i(8), i(8), None, None, i(10), None, None, None, None,
                             None, None, None, None, None, None)
    assert rc == 1 and b"bad argument" in lib.gpn_last_error()
    # nothing to do is not an error
    assert lib.gpn_view_backproject(None, i(4), None, None, None, i(0), i(8), i(8), None, None, None, None, None) == 0


def test_python_entry_refuses_cpu_tensors_and_bad_inputs():
    from gapartnet_amd import _C, hip_ops
    from gapartnet_amd.dataset.convert_rendered import convert_views
    with pytest.raises(_C.GpnError):
        hip_ops.view_backproject(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int32),
                                 torch.zeros(1, 4, 4, dtype=torch.int32), torch.eye(3, dtype=torch.float64)[None])
    v = RV.make_view("plain")
    with pytest.raises(ValueError):
        convert_views(v["rgb"][None, ..., :2], v["depth"][None], v["sem"][None], v["ins"][None], v["npcs"][None], v["K"][None], 512)
    with pytest.raises(TypeError):
        convert_views(v["rgb"][None], v["depth"][None].astype(np.float16), v["sem"][None], v["ins"][None], v["npcs"][None],
                      v["K"][None], 512)


def test_cli_reproduces_the_golden_run_from_given_results(golden, tmp_path, monkeypatch):
    """the driver with convert_views replaced by the golden results: names, grouping, log, writers byte for byte"""
    from gapartnet_amd.dataset import convert_rendered as CR
    data = str(tmp_path / "rendered")
    names = [str(n) for n in golden["names"]]
    for n in names:
        RV.write_view(data, n, {k: golden[f"{n}/in_{k}"] for k in KEYS})
    m = int(golden["num_points"])
    by_rgb = {}  # (the colours are seeded per view; two views share a depth map)
    for n in names:
        st, arrays, scale, gt = R.convert_view(*[golden[f"{n}/in_{k}"] for k in KEYS], m)
        by_rgb[golden[f"{n}/in_rgb"].tobytes()] = CR.ViewResult(st, arrays, scale, gt)
    seen = []

    def fake_convert_views(rgb, depth, sem, ins, npcs, K, num_points, device=None, max_groups=0):
        assert num_points == m and depth.shape[0] <= 2
        seen.append(depth.shape[0])
        return [by_rgb[c.numpy().tobytes()] for c in rgb]

    monkeypatch.setattr(CR, "convert_views", fake_convert_views)
    save, log = str(tmp_path / "out"), str(tmp_path / "log.txt")
    stats = CR.main(["--data_path", data, "--save_path", save, "--num_points", str(m), "--batch", "2", "--log", log])
    assert open(log, "rb").read() == bytes(golden["log"])
    written = sorted(str(n) for n in golden["written"])
    assert sorted(f[:-4] for f in os.listdir(os.path.join(save, "pth"))) == written and stats["written"] == len(written)
    for name in written:
        arrays = torch.load(os.path.join(save, "pth", name + ".pth"), weights_only=False)
        assert len(arrays) == 6
        for i in range(6):
            want = golden[f"{name}/out_pth{i}"]
            assert arrays[i].dtype == want.dtype and np.array_equal(arrays[i], want)
        for sub in ("meta", "gt"):
            assert open(os.path.join(save, sub, name + ".txt"), "rb").read() == bytes(golden[f"{name}/out_{sub}"])
    assert sum(seen) == 5  # every categorised view went through the converter, the Zebra view did not


def test_cli_refuses_visualize_and_unknown_dataset(tmp_path):
    from gapartnet_amd.dataset import convert_rendered as CR
    with pytest.raises(SystemExit):
        CR.main(["--data_path", str(tmp_path), "--visualize", "1"])
    os.makedirs(tmp_path / "rgb")
    with pytest.raises(ValueError):
        CR.main(["--data_path", str(tmp_path), "--save_path", str(tmp_path / "o"), "--dataset", "nope"])
