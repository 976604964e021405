"""The PointNet backbone alone at 8 x 20 000 points: the point-MLP kernel path (csrc/pointmlp.hip) against the plain-torch
formulation of the same module on the same GPU.  Writes profiles/pointnet_bench.txt.

  (i)  eval forward (no gradients: fused BatchNorm / ReLU / max epilogues)      (ii) training forward + backward
  legs alternating (native, torch, native, ...), median of --pairs pairs after a warm-up of each; ratio = torch / native
  per-layer rate of the dense kernels (in-library hipEvent timing, GPN_K_POINTMLP) against the 157.3 TF fp32 MFMA peak
  --parity FILE: copies the error columns a run of tests/test_gpu_pointnet.py -s printed into the report

    python tools/pointnet_bench.py [--pairs 7] [--scenes 8] [--points 20000] [--parity LOG]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_TF = 157.3
K_POINTMLP = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--parity", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_bench.txt"))
    args = ap.parse_args()
    assert args.pairs >= 5
    from gapartnet_amd import _C
    from gapartnet_amd.network.pointnet import PointNetSegBackbone
    dev = torch.device("cuda:0")
    B, n = args.scenes, args.points
    torch.manual_seed(0)
    model = PointNetSegBackbone(3, 16).to(dev)
    pts = torch.rand(B * n, 6, device=dev) * 2 - 1
    cot = torch.randn(B * n, 16, device=dev)
    counts = [n] * B

    def leg(native, training):
        model.use_native_kernels = native
        model.train(training)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if training:
            model.zero_grad(set_to_none=True)
            (model.forward_rows(pts, counts, "reference") * cot).sum().backward()
        else:
            with torch.no_grad():
                model.forward_rows(pts, counts, "reference")
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    lines = [f"PointNet backbone, {B} x {n} points, fp32, {torch.cuda.get_device_name(0)}; legs alternating, median of {args.pairs} pairs",
             f"{'leg':<28}{'native ms':>12}{'torch ms':>12}{'torch / native':>16}"]
    for name, training in (("eval forward", False), ("training forward + backward", True)):
        for native in (True, False):  # warm-up of both legs (allocator, BLAS initialisation)
            leg(native, training), leg(native, training)
        t = {True: [], False: []}
        for _ in range(args.pairs):
            for native in (True, False):
                t[native].append(leg(native, training))
        nat, tor = statistics.median(t[True]), statistics.median(t[False])
        lines.append(f"{name:<28}{nat:>12.3f}{tor:>12.3f}{tor / nat:>16.3f}")

    # per-launch rates of the dense kernels: one eval forward and one training step under the library's own timers
    lib = _C.lib()
    for name, training in (("eval forward", False), ("training forward + backward", True)):
        lib.gpn_prof_reset()
        lib.gpn_prof_enable(1)
        leg(True, training)
        launches, ms, flops, nbytes = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _C.check(lib.gpn_prof_get(K_POINTMLP, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(flops), ctypes.byref(nbytes)))
        lib.gpn_prof_enable(0)
        tf = flops.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0
        lines.append(f"dense kernels, {name}: {launches.value} launches, {ms.value:.3f} ms, {flops.value / 1e9:.1f} GFLOP, "
                     f"{tf:.1f} TFLOP/s = {100 * tf / PEAK_TF:.1f} % of {PEAK_TF} TF, {nbytes.value / 1e9:.2f} GB accounted")

    # per layer: forward, dgrad (same kernel, transposed weights) and wgrad of each distinct shape, timed alone
    from gapartnet_amd import hip_ops as ops
    N = B * n
    off = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    host = [i * n for i in range(B + 1)]
    lines.append(f"{'layer (rows x cin -> cout)':<34}{'fwd ms':>9}{'TF/s':>8}{'% peak':>8}{'max-only ms':>13}{'wgrad ms':>10}{'TF/s':>8}")

    def timed(fn, iters=5):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    for cin, cout in ((64, 64), (64, 128), (128, 1024), (64, 512), (512, 256), (256, 256), (256, 16), (1024, 128), (512, 64)):
        x = torch.randn(N, cin, device=dev)
        w = torch.randn(cout, cin, device=dev) / cin ** 0.5
        dy = torch.randn(N, cout, device=dev)
        one = torch.ones(cout, device=dev)
        f = timed(lambda: ops.pointmlp_fwd(x, w, one, None, one, one, True, offsets=off, offsets_host=host))
        m = timed(lambda: ops.pointmlp_fwd(x, w, one, None, one, one, True, offsets=off, offsets_host=host, want_y=False, want_max=True))
        g = timed(lambda: ops.pointmlp_wgrad(x, dy, cin, offsets=off, offsets_host=host, need_dw=True, need_db=True))
        fl = 2.0 * N * cin * cout / 1e9
        lines.append(f"{N:>8} x {cin:>4} -> {cout:<14}{f:>9.3f}{fl / f:>8.1f}{100 * fl / f / PEAK_TF:>8.1f}{m:>13.3f}{g:>10.3f}{fl / g:>8.1f}")
        del x, w, dy

    if args.parity and os.path.exists(args.parity):
        lines.append("")
        lines.append("parity against the float64 restatement (tests/test_gpu_pointnet.py -s): E = max|got - f64| / max|f64|")
        for ln in open(args.parity):
            if " E_ref " in ln or " E_torch " in ln:
                lines.append(ln.rstrip())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
