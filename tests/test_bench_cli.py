"""bench.py's command line, without a GPU: `python bench.py --gpus N` with no RANK in the environment starts its N ranks itself
under torch.distributed.run (the driver's contract wraps the script for N > 1; the plain form used to die on an assertion), and
the summary of the proposal stage's counts the line carries."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("gpn_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_multi_gpu_command_relaunches_itself(monkeypatch):
    bench = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "2"])
    monkeypatch.delenv("RANK", raising=False)
    args = bench.parse()
    assert bench.relaunch_under_torchrun(args) == 7, "the ranks' exit code is passed through"
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 <= int(cmd[cmd.index("--master-port") + 1]) < 65536
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "4", "--steps", "5", "--warmup", "2"], "the script's own arguments are handed on unchanged"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def test_main_relaunches_only_without_a_rank(monkeypatch):
    bench = _bench()
    called = []
    monkeypatch.setattr(bench, "relaunch_under_torchrun", lambda args: called.append(args.gpus) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("RANK", raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    assert called == [2]


def test_proposal_summary():
    bench = _bench()
    assert bench.proposal_summary([None, None]) is None
    s = bench.proposal_summary([None, [100, 18002, 487, 11211, 0, 0, 300], [90, 17000, 480, 11000, 0, 0, 290]])
    assert s["points_per_step"] == [18002, 17000] and s["proposals_min_max"] == [480, 487]


def test_secondary_measurements_are_off_unless_full(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "5", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 5 and args.warmup == 2 and not args.full and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "out"


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs: float arrays only, under 64 MB in all, the same sample positions in every run"""
    import numpy as np
    import torch
    bench = _bench()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 400), torch.nn.Linear(400, 3))
    model[1].bias.requires_grad_(False)
    opt = torch.optim.Adam(model.parameters())
    loss = model(torch.randn(5, 300)).square().mean()
    loss.backward()
    opt.step()
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), model, opt, loss)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["adam_exp_avg_sample.npy", "adam_exp_avg_sq_sample.npy", "grads.npy", "loss.npy", "params_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["loss.npy"].dtype == np.float64 and got["loss.npy"][0] == float(loss.detach())
    trainable = [p for p in model.parameters() if p.requires_grad]
    want = torch.cat([p.grad.reshape(-1) for p in trainable]).numpy()
    assert np.array_equal(got["grads.npy"], want)
    n = min(want.size, bench.DUMP_SAMPLE)
    assert got["params_sample.npy"].shape == (n,) and got["adam_exp_avg_sq_sample.npy"].shape == (n,)
    for f in files:
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f))
