#!/usr/bin/env python
"""bench.py — throughput of the GAPartNet hot path on MI355X (BASELINE.json metric: point-clouds/sec, 20k-pt scenes,
train step).

One "step" = one full training step of the perception pipeline on one batch of synthetic 20k-point scenes per rank:
on-device batched voxelisation + collate, sparse U-Net backbone, semantic / offset heads, dual-set clustering
(ball query + CCL), proposal re-voxelisation, ScoreNet, NPCS-Net, all five losses, backward, Adam.  Inputs (raw point
clouds + labels) are resident in HBM before the timed region.  Launch: ``python bench.py [--gpus N]`` - with N > 1 and no
RANK in the environment the script starts itself under ``python -m torch.distributed.run --nproc-per-node N`` (one rank per
GPU, gradient mean over RCCL); launched that way by somebody else (the driver) it runs as the rank it is told to be.

The timed workload is STATIONARY (round 6): every step is a full training step (forward, backward, gradient exchange, Adam)
from the SAME seeded parameters - after the optimizer's launch the parameter values are put back (gpn_copy_many: 32 MB in four
launches, inside the timed region: extra work, never less).  Trained on, the synthetic labels make the proposal stage's load fall from 18k to
1k points over the first 45 steps (profiles/r05_first_steps.txt), so that runs with different --warmup / --steps timed
different work; ``--moving`` restores that behaviour, and the line carries the proposal stage's counts of the timed steps
(``proposal_stage``) either way.

Prints ONE JSON line on rank 0 with the contract fields.  A plain run sets up, warms up, times --steps steps and prints;
``--full`` adds the secondary measurements: ``roofline`` (dominant kernel, measured with hipEvents inside libgpn_hip.so
during an extra instrumented step), ``validation`` (validation steps, BASELINE config 2 shape) and ``cpu_baseline`` (the
same train step through the CPU oracle on a bounded sample; rank 0, N=1 only).  ``--dump-outputs DIR`` writes what the
last timed step computed (loss, gradients, sampled parameters and Adam moments) as .npy files.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # see gapartnet_amd/__init__.py: one hardware queue per stream incl. RCCL's
import torch
import torch.distributed as dist

FP32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
HBM_PEAK_GBS = 8000.0           # same guide, HBM3E peak (spec)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8, help="scenes per GPU per step (BASELINE config 3: bs=8/GPU)")
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--schedule", type=str, default="0,0", help="training_schedule; 0,0 = every head active")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-validation", action="store_true",
                    help="skip the validation-step leg (BASELINE config 2 shape: eval mode, bs 4) reported under `validation`")
    ap.add_argument("--lib-knobs", type=str, default="",
                    help="library switches for A/B runs, e.g. msplit=0,bn_fusion=0,wgrad_group=1,tiles_min_tiles=1000000 "
                         "(the library reads no environment variables; these call its knob entry points)")
    ap.add_argument("--moving", action="store_true",
                    help="let the parameters train on (rounds 1-5: the proposal stage's load then depends on how many steps preceded)")
    ap.add_argument("--cpu-scenes", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also the secondary measurements: the instrumented roofline step, the validation-step leg and the CPU "
                         "baseline (--no-validation / --no-cpu-baseline still drop one of them); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed as DIR/<name>.npy (see dump_outputs)")
    return ap.parse_args()


class ParameterSnapshot:
    """the parameter values at construction, put back (gpn_copy_many: 96 tensors per launch) after every optimizer step: each timed
    step then does the work of a training step from the same weights (the stationary workload; see the module docstring)"""

    def __init__(self, model):
        self.params = [p for p in model.parameters() if p.requires_grad]
        with torch.no_grad():
            self.saved = [p.detach().clone() for p in self.params]

    def restore(self):
        from gapartnet_amd.optim import _copy_many
        with torch.no_grad():
            _copy_many([p.data for p in self.params], self.saved)


def build_step(model, optimizer, world, device, moving=False):
    grad_sync = None
    if world > 1 or os.environ.get("GPN_BENCH_FORCE_GRAD_SYNC") == "1":  # the switch: exchange cost measurable on one GPU
        from gapartnet_amd.grad_sync import GradSync
        grad_sync = GradSync(model)
        grad_sync.broadcast_parameters()
    snapshot = None if moving else ParameterSnapshot(model)

    def step(batch, i):
        optimizer.zero_grad(set_to_none=True)
        loss = model.training_step(batch, i)
        loss.backward()
        if grad_sync is not None:
            grad_sync.sync()  # mean of the ranks' gradients: the path's one collective
        optimizer.step()
        if snapshot is not None:
            snapshot.restore()
        return loss
    step.grad_sync = grad_sync
    return step


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` (N > 1) started by hand or by a driver that does not wrap it: start the N ranks ourselves -
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py ...` -
    and pass their output and exit code through"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: what RCCL needs between processes on this host driver)
    env.setdefault("OMP_NUM_THREADS", str(max(1, usable_cores() // args.gpus)))
    return subprocess.call(cmd, env=env)


def kernel_source_fingerprint():
    """sha256 over the HIP sources (and the Makefile) the kernels are built from: identifies WHICH kernels a PMC pass measured"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "gapartnet_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) or name == "Makefile":  # (the Makefile carries per-file compiler flags)
            with open(os.path.join(csrc, name), "rb") as fh:
                h.update(name.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def measured_traffic():
    """HBM bytes per launch of the conv kernel family from the committed PMC passes (profiles/traffic.json, produced by
    tools/pmc_traffic.py from separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` runs of this command).  Counters cannot
    be collected inside this process, so the figure is only reported when the passes were taken on EXACTLY the kernel
    sources this run is built from (fingerprint recorded by the tool); otherwise null - never a stale constant."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        with open(path) as fh:
            rec = json.load(fh)
        if rec.get("kernel_source_fingerprint") != kernel_source_fingerprint():
            return None
        return float(rec["traffic_bytes_per_launch"])
    except (OSError, KeyError, ValueError):
        return None


def profiled_kernel_time(family: str):
    """(ms per step, launches per step) of a kernel family from the committed rocprofv3 run of this command
    (profiles/profile_summary.json, written by tools/profile_summary.py from `rocprofv3 --kernel-trace --stats`), only when it
    was taken on exactly the kernel sources this run is built from - so that the bench line can be checked against
    profiles/ without trusting a stale number"""
    path = os.path.join(ROOT, "profiles", "profile_summary.json")
    try:
        with open(path) as fh:
            rec = json.load(fh)
        if rec.get("kernel_source_fingerprint") != kernel_source_fingerprint():
            return None
        fam = rec["families"][family]
        return float(fam["ms_per_step"]), float(fam["launches_per_step"])
    except (OSError, KeyError, ValueError):
        return None


def roofline_from_profile(device):
    """Σ algorithmic work / Σ hipEvent time per kernel family over one instrumented step."""
    import ctypes
    from gapartnet_amd import _C, functional as GF
    lib = _C.lib()
    out = {}
    names = {0: "spconv_fwd_kernel (fwd+dgrad launches)", 1: "spconv_wgrad_kernel", 6: "batchnorm passes"}
    # algorithmic flops/bytes per launch from the Python-side conv log (pair counts are device scalars: read now)
    per_kind = {"fwd": [0.0, 0.0, 0], "dgrad": [0.0, 0.0, 0], "wgrad": [0.0, 0.0, 0]}
    for (num_pairs, cin, cout, n_src, n_dst, K, kind, live) in GF.CONV_LOG:
        P = float(num_pairs.item())
        if live is not None:  # device-counted rulebook: n_src / n_dst are the buffers' bounds
            n_src, n_dst = int(live[0].t.item()), int(live[1].t.item())
        per_kind[kind][0] += 2.0 * P * cin * cout
        per_kind[kind][1] += 4.0 * n_src * cin + 4.0 * n_dst * cout + 8.0 * P + 4.0 * K * cin * cout
        per_kind[kind][2] += 1
    work = {0: (per_kind["fwd"][0] + per_kind["dgrad"][0], per_kind["fwd"][1] + per_kind["dgrad"][1]),
            1: (per_kind["wgrad"][0], per_kind["wgrad"][1]), 6: None}  # (BatchNorm: bytes counted by the library per call)
    for kid, label in names.items():
        launches, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _C.check(lib.gpn_prof_get(kid, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)))
        flops, nbytes = work[kid] if work[kid] is not None else (float(fl.value), float(by.value))
        out[kid] = dict(kernel=label, launches=int(launches.value), ms_raw=float(ms.value), flops=flops, bytes=nbytes,
                        bound="hbm" if kid == 6 else "mfma")
    # a (start event, launch, stop event) bracket adds a fixed cost to every launch (dispatch latency + two timestamp
    # packets): measured around an empty kernel on the same stream and subtracted, so that the durations agree with a
    # profiler's kernel durations (profiles/r01_bench_kernel_stats.csv)
    overhead = ctypes.c_double()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _C.check(lib.gpn_prof_bracket_overhead_us(stream, ctypes.byref(overhead)))
    for v in out.values():
        v["bracket_overhead_us"] = float(overhead.value)
        v["ms"] = max(v["ms_raw"] - v["launches"] * overhead.value * 1e-3, 0.0)
    out["levels"] = conv_levels(lib, float(overhead.value))
    return out


MACHINE_BALANCE = FP32_MFMA_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9)  # flop per byte above which the MFMA roofline binds


def conv_levels(lib, overhead_us):
    """the conv fwd / dgrad launches of the instrumented step by SHAPE (taps, output rows, channels): per shape the launches,
    their hipEvent time (raw, and minus the bracket cost), the algorithmic flops and bytes of SURVEY 8(d) from the live pair
    counts, and the roofline that binds that shape - flops / bytes under the machine balance (19.7 flop/B): HBM, else MFMA.
    (The family figure hides that the 16-channel level is byte-bound by the survey's own model.)"""
    import ctypes
    from gapartnet_amd import _C, functional as GF
    count = ctypes.c_int64()
    _C.check(lib.gpn_prof_get_launches(0, ctypes.c_int64(0), None, None, ctypes.byref(count)))
    n = int(count.value)
    ms = (ctypes.c_double * max(n, 1))()
    tags = (ctypes.c_int64 * max(n, 1))()
    _C.check(lib.gpn_prof_get_launches(0, ctypes.c_int64(n), ms, tags, ctypes.byref(count)))
    shapes = {}
    for i in range(n):
        t = int(tags[i])
        key = ((t >> 48) & 63, t & 0xffffffff, ((t >> 40) & 255) * 16, ((t >> 32) & 255) * 16)  # (K, rows, cin, cout)
        rec = shapes.setdefault(key, dict(launches=0, ms_raw=0.0, flops=0.0, bytes=0.0, layers=0))
        rec["launches"] += 1
        rec["ms_raw"] += float(ms[i])
    for (num_pairs, cin, cout, n_src, n_dst, K, kind, live) in GF.CONV_LOG:
        if kind == "wgrad":
            continue
        rec = shapes.get((K, n_dst, cin, cout))  # (the launch tag carries the row count the library was called with)
        if rec is None:  # (a launch path without a tag: not expected)
            continue
        P = float(num_pairs.item())
        if live is not None:  # device-counted rulebook: the tag's rows are the buffers' bound, the bytes those of the live rows
            n_src, n_dst = int(live[0].t.item()), int(live[1].t.item())
            rec["live_rows"] = n_dst
        rec["flops"] += 2.0 * P * cin * cout
        rec["bytes"] += 4.0 * n_src * cin + 4.0 * n_dst * cout + 8.0 * P + 4.0 * K * cin * cout
        rec["layers"] += 1
    rows = []
    for (K, n_rows, cin, cout), r in sorted(shapes.items(), key=lambda kv: -kv[1]["ms_raw"]):
        if r["layers"] == 0 or r["ms_raw"] <= 0:
            continue
        t_raw = r["ms_raw"] * 1e-3
        t_adj = max(r["ms_raw"] - r["launches"] * overhead_us * 1e-3, 1e-9) * 1e-3
        intensity = r["flops"] / r["bytes"]
        bound = "mfma" if intensity >= MACHINE_BALANCE else "hbm"
        peak = FP32_MFMA_PEAK_TFLOPS * 1e12 if bound == "mfma" else HBM_PEAK_GBS * 1e9
        work = r["flops"] if bound == "mfma" else r["bytes"]
        rows.append(dict(taps=K, rows=r.get("live_rows", n_rows), **({"rows_bound": n_rows} if "live_rows" in r else {}),
                         cin=cin, cout=cout, launches=r["launches"], layers=r["layers"],
                         us_per_launch_raw_events=r["ms_raw"] * 1e3 / r["launches"], flop_per_byte=intensity, bound=bound,
                         tflops_raw_events=r["flops"] / t_raw / 1e12, gbs_raw_events=r["bytes"] / t_raw / 1e9,
                         frac_raw_events=work / t_raw / peak, frac_minus_bracket=work / t_adj / peak,
                         share_of_family_time=r["ms_raw"]))
    total = sum(r["share_of_family_time"] for r in rows) or 1.0
    for r in rows:
        r["share_of_family_time"] /= total
    # (the shapes that make up the family's time; the tail - a dozen one-launch shapes of the deep levels - is summed)
    head, tail = rows[:12], rows[12:]
    if tail:
        head.append(dict(shapes=len(tail), launches=sum(r["launches"] for r in tail),
                         share_of_family_time=sum(r["share_of_family_time"] for r in tail), note="remaining shapes"))
    return head


def validation_leg(args, device):
    """BASELINE.json config 2's shape as a second, smaller measurement in the same line (rank 0, one GPU; round 6: the driver's
    record then also covers the evaluation path): validation steps of the full pipeline in eval mode, bs 4 x --points, the loop of
    gapartnet_amd.trainer.Trainer.validate (device prefetcher, the step's one host read deferred by a step), seeded weights with
    non-trivial BatchNorm statistics (tests/golden/recipe.py; release.ckpt is absent).  tools/eval_bench.py is the long form."""
    from gapartnet_amd.dataset.prefetch import DevicePrefetcher
    from gapartnet_amd.smoke import make_batch, make_model
    import importlib.util
    # (loaded by path: a top-level package named `tests` somewhere else on sys.path must not shadow the repo's)
    spec = importlib.util.spec_from_file_location("gpn_golden_recipe", os.path.join(ROOT, "tests", "golden", "recipe.py"))
    recipe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recipe)
    model = make_model((0, 0)).eval()
    model.load_state_dict(recipe.name_keyed_state(model))
    model = model.to(device)
    model._log_sink = lambda name, value, bs, sync: None
    model.defer_validation_outputs = True
    batch, steps = 4, 18
    pool = [[pc.to(device) for pc in make_batch(batch, args.points, seed0=2000 + 10 * j)] for j in range(2)]
    times = []
    with torch.no_grad():
        for epoch in range(4):  # the first one warms up
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for i, b in enumerate(DevicePrefetcher((pool[i % 2] for i in range(steps)), model, device)):
                model.validation_step(b, i, 0)
            model._resolve_pending_outputs()
            torch.cuda.synchronize(device)
            if epoch:
                times.append((time.perf_counter() - t0) / steps * 1e3)
            model.validation_step_outputs = [[] for _ in model.validation_step_outputs]
    ms = sorted(times)[len(times) // 2]
    return {"metric": "point-clouds/sec (validation step, eval mode)", "value": batch / ms * 1e3, "ms_per_step": ms,
            "batch": batch, "points_per_scene": args.points, "steps_timed": steps * len(times),
            "workload": "BASELINE config 2 shape: full pipeline, eval mode, score filter + NMS, bs 4; seeded weights (release.ckpt absent); "
                        "median of three 18-step loops after one warm-up loop"}


DUMP_SAMPLE = 1 << 20  # positions of the parameter-sized arrays sampled by dump_outputs (seeded: the same in every run)


def dump_outputs(directory, model, optimizer, loss):
    """--dump-outputs: what the timed train step returned to its caller in the last timed step, as .npy files (~44 MB) -
    loss.npy (float64, [1]); grads.npy (float32: every trainable parameter's gradient in model.parameters() order, flattened
    and concatenated, zeros where a parameter got none); and, at DUMP_SAMPLE positions of that same concatenation drawn with
    a fixed seed, the parameter values after the step (params_sample.npy) and Adam's two moment estimates
    (adam_exp_avg_sample.npy, adam_exp_avg_sq_sample.npy).  Inputs and weights are seeded, so two builds run with the same
    arguments can be compared file by file."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    params = [p for p in model.parameters() if p.requires_grad]

    def flat(tensors):
        return torch.cat([t.detach().reshape(-1).to(torch.float32) for t in tensors]).cpu().numpy()

    grads = flat([p.grad if p.grad is not None else torch.zeros_like(p) for p in params])
    idx = np.sort(np.random.default_rng(0).choice(grads.size, size=min(grads.size, DUMP_SAMPLE), replace=False))
    arrays = {"loss": np.array([float(loss.detach())], np.float64), "grads": grads, "params_sample": flat(params)[idx]}
    for key in ("exp_avg", "exp_avg_sq"):
        moments = [optimizer.state[p][key] if key in optimizer.state.get(p, {}) else torch.zeros_like(p) for p in params]
        arrays[f"adam_{key}_sample"] = flat(moments)[idx]
    for name, a in arrays.items():
        np.save(os.path.join(directory, f"{name}.npy"), a)


def apply_lib_knobs(spec: str):
    """--lib-knobs name=value,...: the library's measurement switches (include/gpn.h), all of them entry points"""
    import ctypes
    from gapartnet_amd import _C
    lib = _C.lib()
    for item in filter(None, (spec or "").split(",")):
        name, _, value = item.partition("=")
        v = int(value)
        if name == "msplit":
            lib.gpn_spconv_msplit(v, -1, -1)
        elif name == "bn_fusion":
            lib.gpn_net_bn_fusion(v)
        elif name == "wgrad_group":
            lib.gpn_net_wgrad_group(v)
        elif name == "tiles_min_tiles":
            lib.gpn_spconv_tiles_min_tiles(ctypes.c_int64(v))
        else:
            raise SystemExit(f"--lib-knobs: unknown switch {name!r}")


def proposal_summary(plans):
    rows = [p for p in plans if p]
    if not rows:
        return None
    pts, props, vox = [int(r[1]) for r in rows], [int(r[2]) for r in rows], [int(r[3]) for r in rows]
    return {"points_per_step": pts, "proposals_per_step": props, "voxels_per_step": vox,
            "points_min_max": [min(pts), max(pts)], "proposals_min_max": [min(props), max(props)]}


def usable_cores() -> int:
    """host cores this process may actually use: the smaller of the scheduler affinity and the cgroup CPU quota (the GPU
    boxes report 256 logical CPUs under a 16-CPU quota; 256 threads there run ~100x slower than 16)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:  # cgroup v2: "<quota> <period>" or "max <period>"
            quota, period = fh.read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fq, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fp:
                quota, period = int(fq.read()), int(fp.read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return max(1, n)


def _cpu_steps(args, n_scenes, threads, timed):
    """median seconds of `timed` full train steps (after one warm-up step) through the CPU oracle with `threads` threads"""
    import statistics
    import oracle
    from gapartnet_amd import backend
    from gapartnet_amd.smoke import make_batch, make_model
    from oracle import torch_ops as oracle_ops
    torch.set_num_threads(threads)
    oracle.set_threads(threads)
    model = make_model(tuple(int(s) for s in args.schedule.split(",")))
    opt = model.configure_optimizers()
    batches = [make_batch(n_scenes, args.points, seed0=5000 + 100 * j) for j in range(2)]
    times = []
    with backend.using(oracle_ops):
        for i in range(1 + timed):
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(batches[i % 2], i)
            loss.backward()
            opt.step()
            if i > 0:
                times.append(time.perf_counter() - t0)
    return statistics.median(times), sum(times)


def cpu_baseline(args):
    """the same train step through the CPU oracle (oracle/gpn_oracle.c, kind "port": the reference's spconv / epic_ops CPU
    path cannot be installed here) on a bounded sample: one warm-up step, then the median of 3 timed steps - with one
    thread, and with every host core (OpenMP over the rule pairs of a tap in the conv loops and over queries in the ball
    query, torch's own threads for the glue).  The reported value is the all-cores run."""
    cores = usable_cores()
    single_n = 1
    t1, spent1 = _cpu_steps(args, single_n, 1, 3)
    tn, spentn = _cpu_steps(args, args.cpu_scenes, cores, 3)
    torch.set_num_threads(cores)
    return dict(value=args.cpu_scenes / tn, unit="point-clouds/sec", cores=cores, kind="port",
                single_thread=dict(value=single_n / t1, cores=1, scenes_per_step=single_n, median_step_s=t1),
                sample=f"median of 3 full train steps (fwd+bwd+Adam) after 1 warm-up, {args.cpu_scenes} synthetic scene(s) x "
                       f"{args.points} pts per step, CPU oracle (oracle/gpn_oracle.c) with {cores} OpenMP/torch threads: "
                       f"{tn:.2f} s/step ({spentn:.0f} s timed); single thread on {single_n} scene: {t1:.2f} s/step "
                       f"({spent1:.0f} s timed)")


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(relaunch_under_torchrun(args))
    torch.set_num_threads(usable_cores())  # torch sizes its CPU pool from the logical CPU count, not from the cgroup quota
    from gapartnet_amd.trainer import init_distributed
    rank, local_rank, world, device = init_distributed("cuda")
    assert device.type == "cuda", "bench.py needs a GPU (the product has no CPU path)"
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if world == 1 and os.environ.get("GPN_BENCH_FORCE_GRAD_SYNC") == "1":  # a 1-rank RCCL group: the exchange on one GPU
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29531")
        from gapartnet_amd.trainer import native_stdout_to_stderr
        with native_stdout_to_stderr():
            dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=device)
    from gapartnet_amd import _C, functional as GF
    from gapartnet_amd.smoke import make_batch, make_model
    _C.lib()  # fail loudly if the HIP extension is missing
    apply_lib_knobs(args.lib_knobs)

    schedule = tuple(int(s) for s in args.schedule.split(","))
    model = make_model(schedule).to(device)
    optimizer = model.configure_optimizers()
    step = build_step(model, optimizer, world, device, moving=args.moving)
    # two resident batches per rank (alternated) of distinct synthetic scenes
    pool = [[pc.to(device) for pc in make_batch(args.batch, args.points, seed0=1000 + (2 * rank + j) * args.batch)]
            for j in range(2)]
    model.train()
    # batches are prepared (voxelised, rulebooks built) one step ahead on a second stream: the loader side of the path
    from gapartnet_amd.dataset.prefetch import DevicePrefetcher
    total_steps = args.warmup + args.steps + 1
    feed = iter(DevicePrefetcher((pool[i % 2] for i in range(total_steps)), model, device))
    for i in range(args.warmup):
        step(next(feed), i)
    torch.cuda.synchronize(device)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    cpu0 = time.process_time()  # CPU seconds of every thread of this process (main, weight-gradient helper, runtime threads)
    plans = []  # the proposal stage's counts as the host learns them (two steps late, never waited for): a list append per step
    for i in range(args.steps):
        loss = step(next(feed), i)
        plans.append(model._prop_hist[-1] if getattr(model, "_prop_hist", None) else None)
    torch.cuda.synchronize(device)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0
    host_cpu_ms = (time.process_time() - cpu0) / args.steps * 1e3
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, optimizer, loss)

    # --full: instrumented extra step (not timed): hipEvent pairs around the conv kernels on their launch stream
    roof = None
    if args.full and rank == 0:
        lib = _C.lib()
        lib.gpn_prof_reset(); lib.gpn_prof_enable(1)
        GF.CONV_LOG = []
        step(next(feed), 0)
        torch.cuda.synchronize(device)
        lib.gpn_prof_enable(0)
        prof = roofline_from_profile(device)
        GF.CONV_LOG = None
        levels = prof.pop("levels")
        dom = max((v for v in prof.values() if v["bound"] == "mfma"), key=lambda d: d["ms"])
        if dom["ms"] > 0 and dom["launches"] > 0:
            achieved = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
            # the same family in the committed rocprofv3 run of this command (same kernel sources): its time for the work
            # counted live here.  `frac` subtracts the measured cost of an event bracket from every launch, `frac_raw_events`
            # does not, `profile_frac` needs neither - the three must tell the same story
            # (the committed profile is of the DEFAULT workload: no profile figure for other batch sizes / schedules)
            default_workload = args.batch == 8 and args.points == 20000 and args.schedule == "0,0"
            prof_time = profiled_kernel_time("conv fwd/dgrad") if default_workload else None
            profile_frac = (dom["flops"] / (prof_time[0] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS) if prof_time else None

            profile_family = {"spconv_fwd_kernel (fwd+dgrad launches)": "conv fwd/dgrad", "spconv_wgrad_kernel": "wgrad (+reduce)",
                              "batchnorm passes": "batchnorm"}

            def family(v):
                """a kernel family: hipEvent figures of this run, and - when profiles/profile_summary.json is of these kernel
                sources - the rocprofv3 time of the same family for the work counted live here"""
                d = dict(ms_raw_events=v["ms_raw"], ms_minus_bracket=v["ms"], launches=v["launches"], bound=v["bound"])
                peak = FP32_MFMA_PEAK_TFLOPS * 1e12 if v["bound"] == "mfma" else HBM_PEAK_GBS * 1e9
                work = v["flops"] if v["bound"] == "mfma" else v["bytes"]
                if v["ms_raw"] > 0:
                    d["frac_raw_events"] = work / (v["ms_raw"] * 1e-3) / peak
                if v["ms"] > 0:
                    d["frac_minus_bracket"] = work / (v["ms"] * 1e-3) / peak
                pt = profiled_kernel_time(profile_family[v["kernel"]]) if default_workload else None
                if pt:
                    d["profile_ms_per_step"], d["profile_launches_per_step"] = pt
                    d["profile_frac"] = work / (pt[0] * 1e-3) / peak
                d["frac"] = d.get("profile_frac", d.get("frac_raw_events"))
                return d

            # Headline `frac` / `achieved`: the rocprofv3 duration of the family (profiles/profile_summary.json) when that
            # run is of exactly these kernel sources - the figure anybody can re-derive from profiles/ - else the live
            # hipEvent time as measured (raw: an event bracket only ever adds time, so this never overstates).  The
            # bracket-corrected figure (`frac_minus_bracket`: minus the cost measured around an empty kernel) is kept as a
            # secondary number: it over-corrects for back-to-back launches (0.18 against 0.15 from the profiler in round 3).
            raw_frac = dom["flops"] / (dom["ms_raw"] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS
            headline = profile_frac if profile_frac is not None else raw_frac
            roof = dict(bound="mfma", kernel=dom["kernel"], achieved=headline * FP32_MFMA_PEAK_TFLOPS, peak=FP32_MFMA_PEAK_TFLOPS,
                        unit="TFLOP/s", frac=headline,
                        frac_source="rocprofv3 (profiles/profile_summary.json, same kernel sources)" if profile_frac is not None
                        else "hipEvents of this run, raw",
                        frac_raw_events=raw_frac, frac_minus_bracket=achieved / FP32_MFMA_PEAK_TFLOPS,
                        profile_frac=profile_frac,
                        profile_ms_per_step=prof_time[0] if prof_time else None,
                        profile_launches_per_step=prof_time[1] if prof_time else None,
                        traffic=measured_traffic() if default_workload else None, launches=dom["launches"],
                        avg_launch_us=dom["ms"] * 1e3 / dom["launches"],
                        avg_launch_us_raw_events=dom["ms_raw"] * 1e3 / dom["launches"],
                        event_bracket_overhead_us=dom["bracket_overhead_us"],
                        algorithmic_gbs=dom["bytes"] / (dom["ms"] * 1e-3) / 1e9,
                        hbm_frac=dom["bytes"] / (dom["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        all_kernels={v["kernel"]: family(v) for v in prof.values()},
                        # per conv shape: which roofline binds (flop/B against the machine balance) and how far from it
                        levels=levels)
    elif args.full and world > 1:
        step(next(feed), 0)  # keep ranks in lock-step through the extra step's gradient exchange
    if world > 1:
        dist.barrier()

    if rank == 0:
        clouds = world * args.batch * args.steps
        out = {
            "metric": "point-clouds/sec (20k pts, train step)", "value": clouds / elapsed, "unit": "point-clouds/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"full pipeline train step (fwd+bwd+Adam), schedule {list(schedule)}, "
                                   f"{args.points}-pt scenes, bs={args.batch}/GPU (BASELINE config 3 per-GPU shape), "
                                   f"voxel 0.01, random-init weights, "
                                   + ("parameters train on (--moving)" if args.moving else
                                      "every step from the same seeded parameters (values put back by copy launches after Adam, inside the timed region)"),
                       "global_batch": world * args.batch, "points_per_scene": args.points, "parallelism": f"dp{world}"},
            # what the proposal stage saw in the timed steps (rank 0; counts reach the host two steps late): clustered points,
            # proposals, proposal voxels - per step, so that a reader can see whether the timed work was stationary
            "proposal_stage": proposal_summary(plans),
            "roofline": roof,
            # what a rank asks of the host: CPU milliseconds per step summed over its threads (rank 0's), and the cores it may
            # run on - at N ranks per node the node needs about N x cpu_ms_per_step / ms_per_step cores for this rate
            "host": {"cpu_ms_per_step": host_cpu_ms, "cores_in_use": host_cpu_ms / (elapsed / args.steps * 1e3),
                     "affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
                     "usable_cores": usable_cores()},
        }
        if step.grad_sync is not None:  # how the gradient exchange ran: buckets all-reduced in place / via one cat / skipped
            out["grad_exchange"] = dict(step.grad_sync.stats, backend=step.grad_sync.backend)
        if dist.is_available() and dist.is_initialized():  # proof of what the collective library saw (a SCALE record can be checked)
            out["distributed"] = {"world_size": dist.get_world_size(), "rank_reporting": dist.get_rank(),
                                  "backend": dist.get_backend(), "env_world_size": int(os.environ.get("WORLD_SIZE", "1")),
                                  "device": torch.cuda.get_device_name(device)}
        if args.full and world == 1 and not args.no_validation:
            try:  # (a secondary figure: it must never cost the run its headline)
                out["validation"] = validation_leg(args, device)
            except Exception as exc:  # noqa: BLE001
                out["validation"] = {"error": f"{type(exc).__name__}: {exc}"}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
